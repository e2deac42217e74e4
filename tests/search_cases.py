"""Hand-built cases of the homology-search rule, a few hundred bases each.
Every builder returns (contigs, subjects, P, n_records): the number of records the rule must
report is written down with the reasoning, and the tests compare it with both oracles and
with the GPU."""
import random

import numpy as np

import search_oracle as so


def rnd(n, seed):
    r = random.Random(seed)
    return "".join(r.choice("ACGT") for _ in range(n))


def mut(s):
    """Every base replaced by another: a mismatch in every column."""
    return "".join("ACGT"[("ACGT".index(ch) + 1) % 4] for ch in s)


def params(**kw):
    P = dict(so.DEFAULTS)
    P.update(kw)
    return P


def flat(seqs):
    """(uint8 bases, int64 offsets) of a list of strings."""
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.frombuffer("".join(seqs).encode(), np.uint8), off


def clip_ends():
    """An HSP cut at store position 0 and one cut at the end of the last contig: the subject
    goes on (with bases that would match nothing), the contig does not.  2 records."""
    a, b = rnd(200, 1), rnd(200, 2)
    return [a, b], [rnd(20, 3) + a[:60], b[150:] + rnd(20, 4)], params(), 2


def contig_junction():
    """The subject is the last 40 bases of contig 0 followed by the first 40 of contig 1,
    which are neighbours in the store: crossed, one HSP of 80; by the rule two of 40."""
    a, b = rnd(150, 5), rnd(150, 6)
    return [a, b], [a[-40:] + b[:40]], params(), 2


def subject_junction():
    """Two subjects that are neighbours in the chunk and in the contig: two HSPs of 40, in the
    plus store and (in reverse order) in the minus store."""
    r = rnd(300, 7)
    return [r], [r[100:140], r[140:180]], params(), 2


def minus_strand():
    """The reverse complement of contig bases 50..129: one record, minus, sstart 0."""
    r = rnd(300, 8)
    return [r], [so.revcomp(r[50:130])], params(), 1


def palindrome():
    """A subject equal to its own reverse complement hits as plus and as minus: 2 records."""
    h = rnd(30, 9)
    p = h + so.revcomp(h)
    return [rnd(100, 10) + p + rnd(100, 11)], [p], params(), 2


def n_bases():
    """Subject 0: an N in column 50 of a 100-base match (one mismatch column, one HSP of 99
    matches).  Subject 1: 30 bases whose two seeds both hold the N (nothing).  Subject 2: the
    N is in the contig.  2 records."""
    r, r2 = rnd(300, 12), rnd(300, 13)
    s0 = r[100:150] + "N" + r[151:200]
    s1 = r[210:225] + "n" + r[226:240]
    c2 = r2[:150] + "N" + r2[151:]
    return [r, c2], [s0, s1, r2[100:200]], params(), 2


def word_boundary_seed():
    """The only seed of subject 1 (25 bases after a 20-base subject: store 20..40) straddles
    the 32-base word boundary.  1 record of score 25."""
    r = rnd(300, 14)
    return [r], [rnd(20, 15), r[100:125]], params(min_score=20), 1


def seed_32():
    r = rnd(300, 16)
    return [r], [r[100:170]], params(S=32), 1


def seed_12():
    r = rnd(300, 17)
    return [r], [r[100:140]], params(S=12, T=4, min_score=12), 1


def _ends(k):
    """T = 32.  Subject 0: 21 + k matching bases, then 10 mismatches: the HSP ends k columns
    past the seed at 0.  Subject 1: 64 - k mismatches, then k + 21 matches: the seed at 64 is
    extended k columns to the left.  2 records."""
    r = rnd(400, 18)
    p = 64 - k
    s0 = r[100:121 + k] + mut(r[121 + k:131 + k])
    s1 = mut(r[200:200 + p]) + r[200 + p:200 + p + k + 21]
    return [r], [s0, s1], params(T=32), 2


def ends_31():
    return _ends(31)


def ends_32():
    return _ends(32)


def ends_33():
    return _ends(33)


def _dip(X, n):
    r = rnd(400, 19)
    return [r], [r[100:150] + mut(r[150:160]) + r[160:220]], params(X=X), n


def dip_exactly_x():
    """50 matches, 10 mismatches (a drop of 20 = X: goes on), 60 matches: one HSP of 120."""
    return _dip(20, 1)


def dip_x_plus_one():
    """The same with X = 19: the drop of 20 stops both sides, two HSPs."""
    return _dip(19, 2)


def tie_shortest():
    """40 matches, a mismatch, 2 matches, the subject's end: the running score comes back to
    its best but not above it, so the HSP is the 40 columns."""
    r = rnd(300, 20)
    return [r], [r[100:140] + mut(r[140]) + r[141:143]], params(), 1


def max_occ_exact():
    """A 30-base unit three times in the contigs, max_occ 3: both seeds are used, one HSP per
    copy."""
    u = rnd(30, 21)
    cs = [rnd(80, 22 + i) + u + rnd(80, 30 + i) for i in range(3)]
    return cs, [u], params(max_occ=3), 3


def max_occ_plus_one():
    """The unit four times, max_occ 3: the seeds inside the unit (40, 48) are unused; the
    subject carries 40 bases of contig 0's own flank, whose seeds find the HSP there.  The
    other three copies are not found."""
    u = rnd(30, 21)
    cs = [rnd(80, 22 + i) + u + rnd(80, 30 + i) for i in range(4)]
    return cs, [cs[0][40:110]], params(max_occ=3), 1


def run_28_all_phases():
    """An exact run of S + T - 1 = 28 between mismatches, starting at subject offset 20 + p,
    p = 0..7: always holds a seed.  8 records of score 28 = min_score."""
    r = rnd(400, 40)
    subs = [mut(r[80 - p:100]) + r[100:128] + mut(r[128:140]) for p in range(8)]
    return [r], subs, params(), 8


def run_27_all_phases():
    """The run of 27 at [20 + p, 47 + p) holds a seed offset a (a multiple of 8 with
    20 + p <= a <= 26 + p) for every p but 5: 7 records."""
    r = rnd(400, 41)
    subs = [mut(r[80 - p:100]) + r[100:127] + mut(r[127:140]) for p in range(8)]
    return [r], subs, params(min_score=20), 7


def same_hsp_two_runs():
    """Two exact runs of 40 with one mismatch between them: the seeds of either run give the
    same HSP of 81 columns.  1 record."""
    r = rnd(300, 42)
    return [r], [r[100:140] + mut(r[140]) + r[141:181]], params(), 1


def contained():
    """X = 60.  A: 60 matches, 15 mismatches, B: 28 matches.  From A the walk passes the gap
    (30 <= X) but B's 28 do not make a new best: [0, 60).  From B it reaches A: [0, 103),
    which contains the former.  1 record."""
    r = rnd(300, 43)
    return [r], [r[100:160] + mut(r[160:175]) + r[175:203]], params(X=60), 1


def partial_overlap():
    """X = 60, T = 1.  A 24, gap 13, B 40, gap 13, C 24.  From A: [0, 77) (B's 40 beat the gap's
    26, C's 24 do not); from C: [37, 114); from B: [37, 77), contained in both.  2 records."""
    r = rnd(300, 44)
    s = r[100:124] + mut(r[124:137]) + r[137:177] + mut(r[177:190]) + r[190:214]
    return [r], [s], params(X=60, T=1), 2


def min_score_edge():
    """Runs of 28 (score 28 = min_score, kept) and of 27 (dropped)."""
    r = rnd(400, 45)
    subs = [mut(r[80:100]) + r[100:128] + mut(r[128:140]), mut(r[180:200]) + r[200:227] + mut(r[227:240])]
    return [r], subs, params(), 1


def degenerate():
    """A subject shorter than S, an empty subject, an empty contig between two others."""
    r, r2 = rnd(200, 46), rnd(200, 47)
    return [r, "", r2], [r[10:25], "", r2[50:100]], params(), 1


def no_subjects():
    return [rnd(200, 48)], [], params(), 0


HAND_BUILT = {f.__name__: f for f in (
    clip_ends, contig_junction, subject_junction, minus_strand, palindrome, n_bases, word_boundary_seed,
    seed_32, seed_12, ends_31, ends_32, ends_33, dip_exactly_x, dip_x_plus_one, tie_shortest, max_occ_exact,
    max_occ_plus_one, run_28_all_phases, run_27_all_phases, same_hsp_two_runs, contained, partial_overlap,
    min_score_edge, degenerate, no_subjects)}


def random_small(seed=5, n_contigs=4, n_subjects=12):
    """A seeded set small enough for the brute oracle."""
    rng = random.Random(seed)
    contigs = [rnd(rng.randint(150, 400), 1000 + i) for i in range(n_contigs)]
    return contigs, _cut(rng, contigs, n_subjects, 40, 200), params()


def _cut(rng, contigs, n, lo, hi):
    subs = []
    for i in range(n):
        c = rng.choice([c for c in contigs if len(c) > lo])
        L = rng.randint(lo, min(hi, len(c)))
        p = rng.randint(0, len(c) - L)
        s = list(c[p:p + L])
        kind = rng.random()
        if kind < 0.1:                                   # unrelated
            s = list(rnd(L, 5000 + i))
        rate = rng.choice([0.0, 0.02, 0.05, 0.1, 0.15])
        for k in range(len(s)):
            if rng.random() < rate:
                s[k] = rng.choice("ACGTN")
        if 0.1 <= kind < 0.3 and L > 30:                 # a short indel
            k = rng.randint(10, L - 10)
            if rng.random() < 0.5:
                del s[k:k + rng.randint(1, 3)]
            else:
                s[k:k] = list(rnd(rng.randint(1, 3), 6000 + i))
        s = "".join(s)
        subs.append(so.revcomp(so.norm(s)) if rng.random() < 0.5 else s)
    return subs


def medium(seed=11):
    """About 40 contigs of 300..3000 bases and 200 subjects of 60..1500 bases cut from them
    (both strands, 0..15 % substitutions, some with a short indel, some unrelated), plus a
    repeat family of 70 copies, past max_occ = 64, with subjects cut from it."""
    rng = random.Random(seed)
    unit = rnd(120, 7777)
    contigs = []
    for i in range(40):
        c = rnd(rng.randint(300, 3000), 2000 + i)
        if i < 35:                                       # one copy in each half
            for lo, hi in ((0, len(c) // 2 - 120), (len(c) // 2, len(c) - 120)):
                p = rng.randint(lo, hi)
                c = c[:p] + unit + c[p + 120:]
        contigs.append(c)
    subs = _cut(rng, contigs, 196, 60, 1500)
    subs += [unit, unit[10:100], so.revcomp(unit), rnd(30, 1) + unit[:60]]
    return contigs, subs, params()
