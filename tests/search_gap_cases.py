"""Hand-built cases of the gapped extension.  Every builder returns
(contigs, subjects, P, n_records): the number of records the rule must report is written down
with the reasoning, and the tests compare it with both oracle forms and with the GPU.

Where a case needs an exact drop, the bases to be skipped are N: an N mismatches everything,
so no path gains by chance matches on a neighbouring diagonal and the cheapest way past k of
them is exactly k mismatch columns (-4 each) or k gap columns (-5 each)."""
import random

import search_cases as sc
import search_gap_oracle as go
import search_oracle as so

rnd, mut, flat = sc.rnd, sc.mut, sc.flat


def params(**kw):
    P = dict(go.GAP_DEFAULTS)
    P.update(kw)
    return P


def one_del_one_ins():
    """60 bases, a contig base skipped, 59 bases, a base the contig lacks, 60 bases: three
    ungapped HSPs, one alignment of 181 columns (180 + 180 bases, 2 gaps) from each.  1 record."""
    r = rnd(400, 101)
    ins = "ACGT"[("ACGT".index(r[220]) + 2) % 4]
    return [r], [r[100:160] + r[161:220] + ins + r[220:280]], params(), 1


def _gap_of(W, G, Xg):
    """The contig holds G bases (N) the subject lacks, between two pieces of 100."""
    r = rnd(500, 102)
    return [r[:200] + "N" * G + r[200:]], [r[100:300]], params(W=W, Xg=Xg)


def gap_w1_bridged():
    """G = W = 1: diagonal 1 is in the band.  1 record."""
    return _gap_of(1, 1, 30) + (1,)


def gap_w1_plus_one():
    """G = 2 > W = 1: neither anchor reaches the other piece.  2 records."""
    return _gap_of(1, 2, 30) + (2,)


def gap_w15_bridged():
    """G = W = 15, 75 half units <= 2 Xg = 80.  1 record."""
    return _gap_of(15, 15, 40) + (1,)


def gap_w15_plus_one():
    """G = 16: 80 half units would pass the x-drop, the band does not.  2 records."""
    return _gap_of(15, 16, 40) + (2,)


def gap_w31_bridged():
    return _gap_of(31, 31, 100) + (1,)


def gap_w31_plus_one():
    return _gap_of(31, 32, 100) + (2,)


def _dip_mismatch(Xg, n):
    """50 matches, 10 N in the subject (40 half units down), 70 matches; X = 19 keeps the two
    ungapped HSPs apart."""
    r = rnd(400, 103)
    return [r], [r[100:150] + "N" * 10 + r[160:230]], params(X=19, Xg=Xg), n


def dip_mismatch_exact():
    """A drop of 40 = 2 Xg lives: both anchors give the alignment of 130 columns.  1 record."""
    return _dip_mismatch(20, 1)


def dip_mismatch_over():
    """2 Xg = 38 < 40: each side stops at the run.  2 records."""
    return _dip_mismatch(19, 2)


def _dip_gap(G, Xg, n):
    """50 matches, G contig bases (N) skipped, 70 matches."""
    r = rnd(400, 104)
    return [r[:150] + "N" * G + r[150:]], [r[100:220]], params(Xg=Xg), n


def dip_gap_exact():
    """8 gap columns: 40 = 2 Xg lives.  1 record."""
    return _dip_gap(8, 20, 1)


def dip_gap_over():
    return _dip_gap(8, 19, 2)


def dip_gap_odd_under():
    """7 gap columns: 35 half units (17.5) <= 2 Xg = 36.  1 record."""
    return _dip_gap(7, 18, 1)


def dip_gap_odd_over():
    """35 > 2 Xg = 34: a raw-score comparison (17 against 17) would have passed.  2 records."""
    return _dip_gap(7, 17, 2)


def subject_ends():
    """The contig goes on matching nothing beyond the subject; the extensions end at the
    subject's first and last base (sstart 0, sspan M).  1 record."""
    r = rnd(400, 105)
    s = r[100:170] + r[172:260]
    return [r], [s], params(), 1


def store_ends():
    """Subject 0 runs into the first base of contig 0 (the store's start), subject 1 into the
    last base of the last contig, each across an indel; the subjects go on.  2 records."""
    a, b = rnd(200, 106), rnd(200, 107)
    return [a, b], [rnd(20, 108) + a[:30] + a[31:80], b[120:160] + "T" + b[160:] + rnd(20, 109)], params(), 2


def contig_junction():
    """The last 70 bases of contig 0 (one of them missing) followed by the first 50 of contig 1,
    its neighbour in the store: the extension must stop at the junction.  2 records."""
    a, b = rnd(200, 110), rnd(200, 111)
    return [a, b], [a[-70:-30] + a[-29:] + b[:50]], params(), 2


def minus_strand():
    """The reverse complement of 120 contig bases with two of them missing.  1 record, minus."""
    r = rnd(300, 112)
    return [r], [so.revcomp(r[50:110] + r[112:170])], params(), 1


def n_inside():
    """An N in the subject and one in the contig inside the extension, and an indel: N is a
    mismatch column.  1 record."""
    r = rnd(400, 113)
    c = r[:130] + "N" + r[131:]
    return [c], [r[100:150] + r[151:180] + "N" + r[181:250]], params(), 1


def homopolymer_indel():
    """AAAAAA in the contig, AAAAA in the subject, flanked by C and G: wherever the gap is put,
    168 columns, 167 matches, 1 gap.  1 record."""
    a, b = rnd(200, 114), rnd(200, 115)
    return [a + "CAAAAAAG" + b], [a[-80:] + "CAAAAAG" + b[:80]], params(), 1


def tie_smallest_k():
    """60 matches, a mismatch, 2 matches, the subject's end: the score comes back to its best
    on a later anti-diagonal, the earlier cell wins.  1 record of 60 columns."""
    r = rnd(300, 116)
    return [r], [r[100:160] + mut(r[160]) + r[161:163]], params(), 1


def tie_smallest_p():
    """The contig ends P GG ACACACACAC A, the subject P ACACACACACAC.  After P the main diagonal
    (2 mismatches, 10 matches) and the path that skips GG (2 gaps, 11 matches) reach the same
    anti-diagonal with the same score; the latter has the smaller p.  1 record, 2 gaps."""
    r = rnd(300, 117)
    p = r[200:280]
    return [r[:280] + "GG" + "AC" * 5 + "A"], [p + "AC" * 6], params(), 1


def _offset(r, test, lo=120):
    return next(a for a in range(lo, len(r)) if test(a))


def refill_lengths():
    """Exact runs of 62..66 and 126..130 bases between N: the anchor is the midpoint, so the
    extensions are 31 / 32 / 33 and 63 / 64 / 65 long on either side.  10 records."""
    r = rnd(400, 118)
    subs = ["NNNNN" + r[100 + k:100 + k + L] + "NNNNN"
            for k, L in enumerate((62, 63, 64, 65, 66, 126, 127, 128, 129, 130))]
    return [r], subs, params(), 10


def refill_gaps():
    """An HSP of L = 62..66, 126..130 bases with a skipped contig base right after it (then
    20 bases, too few for an HSP of their own), and the mirror image: the gap lies 31..33 and
    63..65 bases from the anchor, where the 64-step window is refilled.  20 records."""
    r = rnd(600, 119)
    subs = []
    for L in (62, 63, 64, 65, 66, 126, 127, 128, 129, 130):
        a = _offset(r, lambda a: r[a + L] != r[a + L + 1])
        subs.append(r[a:a + L] + r[a + L + 1:a + L + 21])
        a = _offset(r, lambda a: r[a - 1] != r[a - 2])
        subs.append(r[a - 21:a - 1] + r[a:a + L])
    return [r], subs, params(), 20


def four_anchors_one_alignment():
    """Four pieces of 60 with an indel between each two: four ungapped HSPs, the same
    alignment from each.  1 record."""
    r = rnd(500, 120)
    return [r], [r[100:160] + r[162:220] + "G" + r[220:280] + r[281:340]], params(), 1


def contained_dropped():
    """Three pieces of 60 with 8 skipped contig bases (N) between each two, W = 15.  From the
    middle anchor both gaps are within the band: the whole.  From an outer anchor the second
    gap would need diagonal 16: two pieces, covered by the whole.  1 record."""
    r = rnd(500, 121)
    c = r[:160] + "N" * 8 + r[160:220] + "N" * 8 + r[220:]
    return [c], [r[100:280]], params(), 1


def gene_twice():
    """The gene lies twice in one contig; the subject is the gene less two bases.  2 records."""
    gene = rnd(150, 122)
    c = rnd(100, 123) + gene + rnd(100, 124) + gene + rnd(100, 125)
    return [c], [gene[:70] + gene[72:]], params(), 2


def min_score_edge():
    """Exact runs of 28 (score2 56 = 2 min_score, kept) and of 27 (no ungapped record, so no
    anchor) between N.  1 record."""
    r = rnd(400, 126)
    return [r], ["NNN" + r[100:128] + "NNN", "NNN" + r[200:227] + "NNN"], params(), 1


def _cut_left(min_score):
    """26 matches, a mismatch, 27 matches between N: one ungapped HSP of score 51 whose
    midpoint is the first base after the mismatch.  With Xg = 1 the left extension dies on the
    mismatch (4 > 2), so the alignment is the 27 matches: score2 54."""
    r = rnd(400, 127)
    return [r], ["NNN" + r[100:126] + mut(r[126]) + r[127:154] + "NNN"], params(Xg=1, min_score=min_score)


def score2_at_min():
    """54 = 2 * 27.  1 record."""
    return _cut_left(27) + (1,)


def score2_below_min():
    """54 < 2 * 28: the anchor's own score (51) passes, its alignment does not.  0 records."""
    return _cut_left(28) + (0,)


def no_records():
    return [rnd(300, 128)], [rnd(100, 129)], params(), 0


def no_subjects():
    return [rnd(200, 130)], [], params(), 0


HAND_BUILT = {f.__name__: f for f in (
    one_del_one_ins, gap_w1_bridged, gap_w1_plus_one, gap_w15_bridged, gap_w15_plus_one, gap_w31_bridged,
    gap_w31_plus_one, dip_mismatch_exact, dip_mismatch_over, dip_gap_exact, dip_gap_over, dip_gap_odd_under,
    dip_gap_odd_over, subject_ends, store_ends, contig_junction, minus_strand, n_inside, homopolymer_indel,
    tie_smallest_k, tie_smallest_p, refill_lengths, refill_gaps, four_anchors_one_alignment, contained_dropped,
    gene_twice, min_score_edge, score2_at_min, score2_below_min, no_records, no_subjects)}

# (qstart, qspan, sstart, sspan, length, matches, gaps) of single-record cases worth pinning
PINNED = {
    "one_del_one_ins": (100, 180, 0, 180, 181, 179, 2),
    "dip_mismatch_exact": (100, 130, 0, 130, 130, 120, 0),
    "dip_gap_exact": (100, 128, 0, 120, 128, 120, 8),
    "homopolymer_indel": (120, 168, 0, 167, 168, 167, 1),
    "tie_smallest_k": (100, 60, 0, 60, 60, 60, 0),
    "tie_smallest_p": (200, 93, 0, 91, 93, 91, 2),
    "contained_dropped": (100, 196, 0, 180, 196, 180, 16),
    "score2_at_min": (127, 27, 30, 27, 27, 27, 0),
}


def planted():
    """The planted homolog of DESIGN.md §12.5: a 1000-base gene cut from a 3000-base contig,
    3 % substitutions, indels of -2, +3 and -1; as given and reverse-complemented."""
    contig = rnd(3000, 1)
    rng = random.Random(7)
    gene = "".join(ch if rng.random() > 0.03 else rng.choice("ACGT") for ch in contig[500:1500])
    gene = gene[:200] + gene[202:]
    gene = gene[:480] + "ACG" + gene[480:]
    gene = gene[:760] + gene[761:]
    return [contig], [gene, so.revcomp(gene)], params()


def _indels(rng, s, k):
    s = list(s)
    for _ in range(k):
        at = rng.randint(10, max(10, len(s) - 10))
        n = rng.randint(1, 6)
        if rng.random() < 0.5:
            del s[at:at + n]
        else:
            s[at:at] = [rng.choice("ACGT") for _ in range(n)]
    return "".join(s)


def medium(seed=13):
    """40 contigs of 300..2000 bases and 200 subjects: 190 homologs of 60..500 bases cut from
    them (both strands, 0..10 % substitutions, 0..4 indels of 1..6 bases, some unrelated), a
    repeat family of 70 copies, past max_occ = 64, and 10 subjects cut from it."""
    rng = random.Random(seed)
    unit = rnd(120, 8888)
    contigs = []
    for i in range(40):
        c = rnd(rng.randint(300, 2000), 3000 + i)
        if i < 35:                                       # one copy in each half
            for lo, hi in ((0, len(c) // 2 - 120), (len(c) // 2, len(c) - 120)):
                p = rng.randint(lo, hi)
                c = c[:p] + unit + c[p + 120:]
        contigs.append(c)
    subs = []
    for i in range(190):
        c = rng.choice(contigs)
        L = rng.randint(60, min(500, len(c)))
        p = rng.randint(0, len(c) - L)
        s = rnd(L, 7000 + i) if rng.random() < 0.1 else c[p:p + L]
        rate = rng.choice([0.0, 0.02, 0.05, 0.1])
        s = "".join(rng.choice("ACGTN") if rng.random() < rate else ch for ch in s)
        s = _indels(rng, s, rng.randint(0, 4))
        subs.append(so.revcomp(so.norm(s)) if rng.random() < 0.5 else s)
    subs += [unit, unit[10:100], so.revcomp(unit), rnd(30, 1) + unit[:60], _indels(rng, unit, 1),
             _indels(rng, unit, 2), so.revcomp(_indels(rng, unit, 1)), unit[:50] + unit[53:], unit[20:] + rnd(20, 2),
             unit[:60] + "A" + unit[60:]]
    return contigs, subs, params()
