"""Hand-built cases of the homology search with a low-complexity mask.
Every builder returns (contigs, subjects, P, n_plain, n_masked): the records the rule must
report without and with the mask (None: "at least one", see the case).  S = 21, T = 8 and the
defaults of both rules unless said."""
import random

import search_cases as sc
import search_dust_oracle as sdo
import search_oracle as so

rnd, mut = sc.rnd, sc.mut


def params(**kw):
    P = dict(sdo.DEFAULTS)
    P.update(kw)
    return P


def gap_params(**kw):
    P = dict(sdo.GAP_DEFAULTS)
    P.update(kw)
    return P


def _no_a(s):
    """The string with its first and last base made a C: a poly-A run next to it stays as it is."""
    return "C" + s[1:-1] + "C"


def poly_a_against_poly_a():
    """Unrelated flanks, the same 40-base poly-A in contig and subject.  Without the mask the
    subject's poly-A seeds (offsets 80, 88, 96) occur 20 times in the contig and give an HSP
    of 40 matches; with it no S-mer of the run is in the index."""
    contig = _no_a(rnd(100, 201)) + "A" * 40 + _no_a(rnd(100, 202))
    subject = _no_a(rnd(80, 203)) + "A" * 40 + _no_a(rnd(80, 204))
    return [contig], [subject], params(), None, 0


def internal_poly_a():
    """A 300-base exact homolog with a poly-A x20 inside it: the seeds outside the run find it
    and the extension passes through the mask.  The same single record either way."""
    r = rnd(600, 205)
    contig = r[:290] + "A" * 20 + r[310:]
    return [contig], [contig[150:450]], params(), 1, 1


def trap():
    """Contig 0: 25 masked bases (poly-A), then 45 random ones; the subject is that string.
    The first unmasked seed is at a = 32.  Its predecessor's 21-mer (columns 24..44: one A of
    the run and 20 random bases) also lies in contig 1 between mismatching flanks, so the
    predecessor slot has a count, while its window on contig 0's diagonal is masked.  A skip
    that ignores the mask loses the HSP on contig 0 altogether (the seeds at 40 and 48 are
    skipped behind 32).  The hit on contig 1 scores 21 and is not reported.  1 record."""
    tail = "C" + rnd(44, 206)
    c0 = "A" * 25 + tail
    pre = c0[24:45]
    left, right = rnd(60, 207), rnd(60, 208)
    left = left[:-1] + "C"                       # a mismatch before the copy (the subject has A),
    right = mut(c0[45:53]) + right[8:]           # eight after it
    return [c0, left + pre + right], [c0], params(), 1, 1


def max_occ_interplay():
    """max_occ 3.  A 30-base unit that begins AAAA, four times in the contigs; in contig 3 it
    follows a poly-A x20, so that copy's first four bases are masked with the run.  The seed at
    0 has four occurrences, one of them masked: usable with the mask (3 HSPs of 30), unused
    without.  The seed at 8 has four unmasked occurrences and is unused either way."""
    u = "AAAA" + _no_a(rnd(26, 209))
    cs = [_no_a(rnd(80, 210 + i)) + u + _no_a(rnd(80, 220 + i)) for i in range(3)]
    cs.append(_no_a(rnd(60, 213)) + "A" * 20 + u + _no_a(rnd(80, 223)))
    return cs, [u], params(max_occ=3), 0, 3


def no_low_complexity():
    """Random contigs whose mask is empty: the records are those without a mask."""
    contigs, subjects, P = sc.random_small()
    n = len(so.search_indexed(contigs, subjects, P))
    return contigs, subjects, params(), n, n


STRADDLE_MASK = (160, 200)       # the masked bases of the straddle cases' contig


def _straddle(S):
    """One contig of 300 bases whose only masked bases are a poly-A x40 at 160..199, the start
    of a 32-bit word of the mask plane.  q = 160 - (S - 1): the S-mer at q starts inside the
    word before (q & 31 != 0) and its only masked base is its last one, the first of the next
    word; the S-mer at q - 1 is unmasked.  Each is a subject of its own with the one seed at
    a = 0 (min_score S, so the S-base HSP is reported): without the mask a record each, with
    it only the S-mer at q - 1 is in the index."""
    contig = _no_a(rnd(160, 230)) + "A" * 40 + _no_a(rnd(100, 231))
    q = STRADDLE_MASK[0] - (S - 1)
    return [contig], [contig[q - 1:q - 1 + S], contig[q:q + S]], params(S=S, min_score=S), 2, 1


def straddle_s32():
    """_straddle at the longest seed: q = 129, the window of 32 bases spans two whole words."""
    return _straddle(32)


def straddle_s12():
    """_straddle at the shortest seed: q = 149, one base of the window in the next word."""
    return _straddle(12)


HAND_BUILT = {f.__name__: f for f in (poly_a_against_poly_a, internal_poly_a, trap, max_occ_interplay,
                                      no_low_complexity, straddle_s32, straddle_s12)}


def planted_gapped():
    """The planted homolog of DESIGN.md §12.5 (a 1000-base gene cut from a 3000-base contig,
    3 % substitutions, indels of -2, +3 and -1, as given and reverse-complemented) with a
    poly-A x30 in place of the contig's bases 1000..1029 and of the gene's 501..530, which
    align with them: the alignment crosses 30 masked columns.  Still one alignment each, the
    same as without the mask."""
    contig = rnd(3000, 1)
    rng = random.Random(7)
    gene = "".join(ch if rng.random() > 0.03 else rng.choice("ACGT") for ch in contig[500:1500])
    gene = gene[:200] + gene[202:]
    gene = gene[:480] + "ACG" + gene[480:]
    gene = gene[:760] + gene[761:]
    gene = gene[:501] + "A" * 30 + gene[531:]
    contig = contig[:1000] + "A" * 30 + contig[1030:]
    return [contig], [gene, so.revcomp(gene)], gap_params(), 2, 2


LOW = ("A", "T", "AC", "AG", "CT", "AAT", "ACG", "AAAC", "AGGT")


def _repeat(rng):
    u = rng.choice(LOW)
    n = rng.randint(30, 80)
    return (u * (n // len(u) + 1))[:n]


def medium_low(seed=17, n=30):
    """search_cases.medium with n low-complexity stretches (homopolymers and 2..4-base repeats
    of 30..80 bases) written over bases of the contigs, and the same number over the subjects."""
    contigs, subjects, P = sc.medium()
    rng = random.Random(seed)
    contigs, subjects = list(contigs), list(subjects)
    for seqs in (contigs, subjects):
        for _ in range(n):
            k = rng.choice([i for i, s in enumerate(seqs) if len(s) > 100])
            rep = _repeat(rng)
            p = rng.randint(0, len(seqs[k]) - len(rep))
            seqs[k] = seqs[k][:p] + rep + seqs[k][p + len(rep):]
    return contigs, subjects, params()
