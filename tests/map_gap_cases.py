"""Seeded inputs for the tests of the read mapper's single-gap rescue (tests/test_map_gap.py,
tests/test_gpu_map_gap.py).

Every hand-built batch is (contigs, reads1, reads2, params, G, expect).  `expect` states, pair
by pair, what the rule of DESIGN.md §11.1 gives: ("u",) aligned by the ungapped rule,
("g", d1, d2) aligned by the gapped pass with these gaps, ("x",) unaligned, ("o",) unaligned
with a hit-list overflow -- test_map_gap.py holds the oracles to that, so a batch checks what
its name says.
"""
import numpy as np

import map_cases as mc
import map_oracle as mo

S = 20


def no_runs_seq(rng, n):
    """Random bases, each different from the one before it."""
    out = [int(rng.integers(4))]
    for _ in range(n - 1):
        out.append((out[-1] + int(rng.integers(1, 4))) % 4)
    return bytes(b"ACGT"[c] for c in out)


def gap_read(contig, p, L, k, d, ins=None):
    """The + strand read of L bases that starts at contig[p] and, after k bases, lacks d
    contig bases (d > 0) or holds -d bases of its own (d < 0: `ins`, or bases that differ
    from both neighbours, so that the gap cannot slide)."""
    s = mo.norm(contig)
    if d >= 0:
        return s[p:p + k] + s[p + k + d:p + L + d]
    g = -d
    if ins is None:
        pick = next(b for b in b"ACGT" if b != s[p + k - 1] and b != s[p + k])
        ins = bytes([pick]) * g
    return s[p:p + k] + ins + s[p + k:p + L - g]


def gpair(contig, fp, L1, frag, L2, gap1=None, gap2=None, flip=False, sub1=(), sub2=()):
    """Mates of the fragment contig[fp : fp + frag] (contig bases); gapN = (k, d) of mate N
    with k along the contig; subN: substituted read indices, along the contig as well; flip:
    mate 1 is the reverse mate."""
    (k1, d1), (k2, d2) = gap1 or (0, 0), gap2 or (0, 0)
    if flip:
        plus = mc.mutate(gap_read(contig, fp, L2, k2, d2), sub2)
        minus = mc.mutate(gap_read(contig, fp + frag - L1 - d1, L1, k1, d1), sub1)
        return mo.revcomp(minus), plus
    plus = mc.mutate(gap_read(contig, fp, L1, k1, d1), sub1)
    minus = mc.mutate(gap_read(contig, fp + frag - L2 - d2, L2, k2, d2), sub2)
    return plus, mo.revcomp(minus)


def _batch(contigs, pairs, expect, G, **kw):
    return contigs, [p[0] for p in pairs], [p[1] for p in pairs], mo.params(**kw), G, expect


def gap_lengths():
    """An insertion and a deletion of 1 base and of G bases."""
    contig = mc.rand_seq(np.random.default_rng(201), 500)
    pairs, expect = [], []
    for d in (1, -1, 4, -4):
        pairs.append(gpair(contig, 40, 100, 300, 100, gap1=(50, d)))
        expect.append(("g", d, 0))
    pairs.append(gpair(contig, 40, 100, 300, 100))
    expect.append(("u",))
    return _batch([contig], pairs, expect, 4)


def gap_too_long():
    """A gap of G + 1 bases is not found."""
    contig = mc.rand_seq(np.random.default_rng(202), 500)
    pairs = [gpair(contig, 40, 100, 300, 100, gap1=(50, 3)), gpair(contig, 40, 100, 300, 100, gap1=(50, -3)),
             gpair(contig, 40, 100, 300, 100, gap1=(50, 2))]
    return _batch([contig], pairs, [("x",), ("x",), ("g", 2, 0)], 2)


def segment_edges():
    """Gaps at exactly k = S and k = L - S (- g), and one base nearer each end; max_mm 0, so
    that the gap cannot be moved inwards at the price of a mismatch."""
    contig = no_runs_seq(np.random.default_rng(203), 400)
    pairs, expect = [], []
    L = 100
    for k, d, ok in ((S, 1, True), (L - S, 1, True), (S, -2, True), (L - S - 2, -2, True),
                     (S - 1, 1, False), (L - S + 1, 1, False), (S - 1, -2, False), (L - S - 1, -2, False)):
        pairs.append(gpair(contig, 40, L, 300, L, gap1=(k, d)))
        expect.append(("g", d, 0) if ok else ("x",))
    return _batch([contig], pairs, expect, 2, max_mm=0)


def segment_edges_s12():
    """The same with S = 12 and reads of 40 bases, on the reverse mate."""
    contig = no_runs_seq(np.random.default_rng(204), 300)
    pairs, expect = [], []
    L = 40
    for k, d, ok in ((12, 1, True), (28, 1, True), (12, -1, True), (27, -1, True), (11, 1, False),
                     (29, 1, False), (11, -1, False), (28, -1, False)):
        pairs.append(gpair(contig, 30, 50, 220, L, gap2=(k, d)))
        expect.append(("g", 0, d) if ok else ("x",))
    return _batch([contig], pairs, expect, 1, S=12, max_mm=0)


def homopolymer():
    """A base missing from, or added to, a run of eight A: the least k, the run's start."""
    rng = np.random.default_rng(205)
    contig = mc.rand_seq(rng, 249) + b"C" + b"A" * 8 + b"G" + mc.rand_seq(rng, 241)
    # the + mate starts at 200: the run is its bases 50..57
    pairs = [gpair(contig, 200, 100, 280, 100, gap1=(54, 1)),
             (mo.revcomp(contig[380:480]), gap_read(contig, 200, 100, 54, -1, ins=b"A"))]
    return _batch([contig], pairs, [("g", 1, 0), ("g", 0, -1)], 2)


def seed_sides():
    """Reads of 60 bases (seeds at 0, 20, 40) with the gap at 30: the seed at 20 spans it.  A
    substitution in the seed at 0 leaves only the right segment seeded, one in the seed at
    40 only the left; with both, the alignment has two mismatches but no seed."""
    contig = mc.rand_seq(np.random.default_rng(206), 400)
    pairs, expect = [], []
    for d in (2, -2):
        for subs, ok in (((5,), True), ((45,), True), ((5, 45), False), ((), True)):
            pairs.append(gpair(contig, 50, 60, 250, 60, gap1=(30, d), sub1=subs))
            expect.append(("g", d, 0) if ok else ("x",))
            pairs.append(gpair(contig, 50, 60, 250, 60, gap2=(30, d), sub2=subs, flip=True))
            expect.append(("g", 0, d) if ok else ("x",))
    return _batch([contig], pairs, expect, 2)


def contig_ends():
    """Alignments that touch a contig's first or last base, at the ends of the store and
    between two contigs.  With an insertion, one of the two diagonals leaves the contig: it
    must still seed the alignment when the other segment's seeds are broken."""
    rng = np.random.default_rng(207)
    contigs = [mc.rand_seq(rng, n) for n in (300, 33, 260, 320)]
    pairs, expect = [], []
    for c in (0, 2, 3):
        n = len(contigs[c])
        for d in (2, -2, 1):
            # - mate ends on the last base: its right segment (seed at 40) is broken
            pairs.append(gpair(contigs[c], n - 200, 60, 200, 60, gap2=(30, d), sub2=(45,)))
            expect.append(("g", 0, d))
            # + mate starts on the first base: its left segment (seed at 0) is broken
            pairs.append(gpair(contigs[c], 0, 60, 200, 60, gap1=(30, d), sub1=(5,)))
            expect.append(("g", d, 0))
            pairs.append(gpair(contigs[c], 0, 60, n, 60, gap1=(25, d), gap2=(35, -d), flip=True))
            expect.append(("g", d, -d))
    # one base past either end: not an alignment
    m1, m2 = gpair(contigs[2], 0, 60, 200, 60, gap1=(30, -2))
    pairs.append((contigs[1][-1:] + m1[:-1], m2))
    expect.append(("x",))
    return _batch(contigs, pairs, expect, 2, max_insert=400)


def which_mate():
    """The gap on the reverse mate, on both mates, on mate 2 with mate 1 ungapped."""
    contig = mc.rand_seq(np.random.default_rng(208), 600)
    pairs, expect = [], []
    for flip in (False, True):
        pairs.append(gpair(contig, 100, 100, 350, 90, gap2=(40, 3), flip=flip))
        expect.append(("g", 0, 3))
        pairs.append(gpair(contig, 100, 100, 350, 90, gap1=(60, -3), flip=flip))
        expect.append(("g", -3, 0))
        pairs.append(gpair(contig, 100, 100, 350, 90, gap1=(30, 2), gap2=(55, -1), flip=flip, sub1=(90,)))
        expect.append(("g", 2, -1))
    return _batch([contig], pairs, expect, 3)


def ungapped_first():
    """A pair the ungapped rule aligns with two mismatches keeps that result although one
    deletion explains the read with nm = 1."""
    rng = np.random.default_rng(209)
    contig = mc.rand_seq(rng, 250) + b"A" * 20 + b"C" + b"A" * 30 + mc.rand_seq(rng, 200)
    # + mate from 200: bases 0..49 random, then the A run; one A of the run is missing
    pairs = [gpair(contig, 200, 100, 280, 100, gap1=(55, 1))]
    return _batch([contig], pairs, [("u",)], 2)


def gap_ties():
    """Equal nm, |d|, position and fragment: d = -1 and d = +1 both explain the + mate (its
    right segment has period 2), so the key is decided by d1, or by d2."""
    rng = np.random.default_rng(210)
    left = mc.rand_seq(rng, 140)
    if left[-1] == ord("C"):
        left = left[:-1] + b"G"
    contig = left + b"AC" * 20 + mc.rand_seq(rng, 220)
    plus = contig[100:140] + b"C" + b"AC" * 15
    minus = mo.revcomp(contig[250:330])
    return _batch([contig], [(plus, minus), (minus, plus)], [("g", -1, 0), ("g", 0, -1)], 1, max_mm=0)


def long_reads():
    """Reads of 511 and 512 bases: 16 seed slots cover the first 320 bases only."""
    contig = mc.rand_seq(np.random.default_rng(211), 900)
    pairs = [gpair(contig, 20, 511, 800, 60, gap1=(400, 1)),
             gpair(contig, 20, 512, 800, 60, gap1=(100, -1), flip=True),
             gpair(contig, 20, 60, 800, 512, gap2=(491, -1))]
    return _batch([contig], pairs, [("g", 1, 0), ("g", -1, 0), ("g", 0, -1)], 1, max_insert=900)


def widest():
    """G = 8 with S = 12 and max_occ = 64, on contigs that share a repeat."""
    rng = np.random.default_rng(212)
    rep = mc.rand_seq(rng, 60)
    contigs = [mc.rand_seq(rng, 150) + rep + mc.rand_seq(rng, 200 + 10 * i) for i in range(6)]
    pairs, expect = [], []
    for i, d in enumerate((8, -8, 5, -7)):
        pairs.append(gpair(contigs[i], 100, 100, 300, 100, gap1=(45, d), gap2=(60, -d if i < 2 else 0),
                           flip=bool(i & 1)))
        expect.append(("g", d, -d if i < 2 else 0))
    return _batch(contigs, pairs, expect, 8, S=12, max_occ=64)


def overflow():
    """A tandem repeat of period 3 (each 12-mer at most 64 times): every mate has more than
    256 hits over d = 0, +-3, +-6, and the insert bounds leave no ungapped pair."""
    rng = np.random.default_rng(213)
    tandem = b"ACG" * 66
    plain = mc.rand_seq(rng, 400)
    pairs = [(tandem[3:43], mo.revcomp(tandem[90:130])),
             gpair(plain, 20, 40, 330, 40, gap1=(20, 3))]
    return _batch([tandem, plain], pairs, [("o",), ("g", 3, 0)], 6, S=12, max_occ=64, min_insert=300,
                  max_insert=500)


HAND_BUILT = dict(gap_lengths=gap_lengths, gap_too_long=gap_too_long, segment_edges=segment_edges,
                  segment_edges_s12=segment_edges_s12, homopolymer=homopolymer, seed_sides=seed_sides,
                  contig_ends=contig_ends, which_mate=which_mate, ungapped_first=ungapped_first,
                  gap_ties=gap_ties, long_reads=long_reads, widest=widest, overflow=overflow)


def check_expect(results, expect):
    """Hold oracle (or kernel) result tuples to a batch's `expect`."""
    for i, (r, e) in enumerate(zip(results, expect)):
        r = tuple(int(v) for v in r)
        if e[0] == "u":
            ok = r[0] >= 0 and r[6:] == (0, 0, 0, 0, 0)
        elif e[0] == "g":
            ok = r[0] >= 0 and r[6:8] == e[1:] and r[10] == 1
        else:
            ok = r[:10] == mo.UNALIGNED + (0, 0, 0, 0) and r[10] == (2 if e[0] == "o" else 0)
        assert ok, "pair {}: {} is not {}".format(i, r, e)


def _indel(rng, read_len, gmax, margin):
    d = int(rng.integers(1, gmax + 1)) * (1 if rng.random() < 0.5 else -1)
    k = int(rng.integers(margin, read_len - margin - max(0, -d) + 1))
    return k, d


def medium(seed=17, n_contigs=20, n_pairs=600, G=3):
    """Contigs of 300..2,000 bases with a few planted repeats; 2 x 100 pairs with
    substitutions; two in five carry one indel of 1..G in one mate, and one in six a second
    indel in the other mate or a burst of substitutions."""
    rng = np.random.default_rng(seed)
    contigs = [bytearray(mc.rand_seq(rng, int(rng.integers(300, 2001)))) for _ in range(n_contigs)]
    for copies in (2, 3, 20):
        rep = mc.rand_seq(rng, 120)
        for _ in range(copies):
            c = contigs[int(rng.integers(n_contigs))]
            p = int(rng.integers(0, len(c) - 120))
            c[p:p + 120] = rep
    contigs = [bytes(c) for c in contigs]
    r1, r2 = [], []
    for i in range(n_pairs):
        c = contigs[int(rng.integers(n_contigs))]
        frag = min(int(rng.integers(150, 520)), len(c) - 10)
        fp = int(rng.integers(0, len(c) - frag - 8))
        gaps = [None, None]
        u = rng.random()
        if u < 0.55:
            gaps[int(rng.integers(2))] = _indel(rng, 100, G, 5)
            if u < 0.10:
                gaps = [_indel(rng, 100, G, 5), _indel(rng, 100, G, 5)]
        subs = [rng.integers(0, 100, int(rng.poisson(1.0))).tolist() for _ in range(2)]
        if 0.55 <= u < 0.72:
            subs[int(rng.integers(2))] = rng.choice(100, 7, replace=False).tolist()
        m1, m2 = gpair(c, fp, 100, frag, 100, gap1=gaps[0], gap2=gaps[1], flip=bool(i & 1),
                       sub1=subs[0], sub2=subs[1])
        r1.append(m1)
        r2.append(m2)
    return contigs, r1, r2, mo.params(), G


def planted(seed=19, n_contigs=8, length=1000, n_pairs=200, G=3):
    """Repeat-free contigs; every pair has one indel of 1..G in one mate, at least S + 5 bases
    from either end of the read, and no other error.  (contigs, reads1, reads2, params, G,
    truth): truth rows are (contig, pos1, pos2, strand1, d1, d2, k1, k2) with k the planted
    split (along the contig)."""
    rng = np.random.default_rng(seed)
    contigs = [mc.rand_seq(rng, length) for _ in range(n_contigs)]
    r1, r2, truth = [], [], []
    for i in range(n_pairs):
        c = int(rng.integers(n_contigs))
        frag = int(rng.integers(150, 451))
        fp = int(rng.integers(0, length - frag + 1))
        flip = bool(i % 3 == 0)
        gaps = [(0, 0), (0, 0)]
        gaps[i & 1] = _indel(rng, 100, G, S + 5)
        m1, m2 = gpair(contigs[c], fp, 100, frag, 100, gap1=gaps[0], gap2=gaps[1], flip=flip)
        r1.append(m1)
        r2.append(m2)
        (k1, d1), (k2, d2) = gaps
        if flip:
            row = (c, fp + frag - 100 - d1 + 1, fp + 1, 1, d1, d2, k1, k2)
        else:
            row = (c, fp + 1, fp + frag - 100 - d2 + 1, 0, d1, d2, k1, k2)
        truth.append(row)
    return contigs, r1, r2, mo.params(), G, truth
