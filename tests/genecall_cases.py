"""In-memory cases for the gene caller (wf_genecall, waafle_amd/csrc/wf_genecall.hip).

A case is one wf_genecall call: contig groups of hits (qstart, qend, strand, scov) and the
three thresholds.  Every passing hit carries the id of the component the builder put it
in, so the expected genes are known by construction: a component's gene runs from its
smallest start to its largest stop, takes the strand of its longest member (ties to "-")
and is listed in the order of its first member in (start, file position) order.
test_genecall_cases.py checks that against oracle.genecaller_oracle.overlap_intervals on
the CPU; test_gpu_genecall.py runs the same arrays through the C-ABI.

Families:
  S  sizes: the number of passing intervals crosses every LDS capacity of the kernel
     (64, 128 .. 4096), with rejected hits interleaved so that the compaction meets
     partial ballots in every 64-hit chunk; 4096 of 5000 passing; 4097 passing is refused.
  T  topology at 65, 1024 and 4096 intervals: a chain (one gene), the
     chain cut at every k-th link, reversed and shuffled file orders, one interval that
     contains the rest, a star, and chains joined only by weak overlaps.
  K  ties and thresholds: the stable sort, strand ties, ov/den exactly on --min-overlap,
     --min-overlap <= 0, --min-gene-length and --min-scov exactly met, qstart > qend.
  G  10 000 groups in one call, large and small alternating.

On "two interleaved chains with weak cross overlaps": on a line, an interval that lies
inside the span of a chain of overlapping intervals and is contained in none of them is
covered by the two chain members over its ends, so one of them overlaps at least half of
it; and an interval that starts after a weakly overlapping neighbour and strongly overlaps
the first one lies inside that neighbour.  Two chains that alternate in coordinate order
can therefore not stay apart at any threshold <= 1.  What the oracle's `elif score == 0:
break` (as opposed to a break on any non-edge) decides is built here instead: chains whose
ends overlap by a few bases (weak_links: they stay apart, given in alternating file
order), and weak_then_strong, where a weak neighbour sorts before a strong one and a scan
that stopped at the weak pair would lose the edge.
"""
import functools
import random

import numpy as np

from oracle import genecaller_oracle as gco

PASS, FAIL = 0.9, 0.1          # scov of kept and rejected hits at --min-scov 0.75
SIZES = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 4095, 4096]
TOPO_SIZES = [65, 1024, 4096]
CAP_MAX = 4096


class Case:
    """One wf_genecall call.  groups: lists of (qstart, qend, strand 0/1, scov, component
    id or None for a hit below --min-scov)."""

    def __init__(self, name, groups, min_overlap=0.1, min_gene_length=0.0, min_scov=0.75,
                 refused_group=None):
        self.name = name
        self.groups = groups
        self.min_overlap = min_overlap
        self.min_gene_length = min_gene_length
        self.min_scov = min_scov
        self.refused_group = refused_group        # wf_genecall must return WF_E_NOMEM for it

    def __repr__(self):
        return self.name

    def arrays(self):
        off = np.cumsum([0] + [len(g) for g in self.groups]).astype(np.int64)
        flat = [h for g in self.groups for h in g]
        col = lambda i, t: np.array([h[i] for h in flat], dtype=t)
        return off, col(0, np.int32), col(1, np.int32), col(2, np.int8), col(3, np.float64)

    def expected(self):
        """Per group: [(start, stop, strand char)] from the builder's components."""
        out = []
        for g in self.groups:
            comps = {}
            for pos, (qs, qe, st, scov, comp) in enumerate(g):
                if comp is None:
                    assert scov < self.min_scov
                    continue
                assert scov >= self.min_scov
                lo, hi = min(qs, qe), max(qs, qe)
                c = comps.setdefault(comp, [lo, hi, (0, ""), (lo, pos)])
                c[0], c[1] = min(c[0], lo), max(c[1], hi)
                c[2] = max(c[2], (hi - lo + 1, "-" if st else "+"))
                c[3] = min(c[3], (lo, pos))
            genes = sorted(comps.values(), key=lambda c: c[3])
            out.append([(c[0], c[1], c[2][1]) for c in genes
                        if c[1] - c[0] + 1 >= self.min_gene_length])
        return out

    def oracle(self):
        """Per group: the oracle's genes (its scov and length filters, call_genes :85-87)."""
        out = []
        for g in self.groups:
            ints = [(qs, qe, "-" if st else "+") for qs, qe, st, scov, _ in g
                    if scov >= self.min_scov]
            out.append([x for x in gco.overlap_intervals(ints, self.min_overlap)
                        if x[1] - x[0] + 1 >= self.min_gene_length])
        return out


def genes_of(case, n_genes, gs, ge, gst):
    """Result arrays of a call -> per group [(start, stop, strand char)]."""
    off = case.arrays()[0]
    return [[(int(gs[o + i]), int(ge[o + i]), "-" if gst[o + i] else "+")
             for i in range(int(k))] for o, k in zip(off[:-1].tolist(), n_genes.tolist())]


# ---------------------------------------------------------------------------
# building blocks
# ---------------------------------------------------------------------------

def clusters(n, rng, base=1):
    """n passing hits as chains of 1-5 intervals (300 long, step 100: 200/300 overlap)
    separated by 50 free bases; one member of each chain is one base longer, so the chain's
    strand is that member's.  Component ids are (base, chain number)."""
    hits, x, k = [], base, 0
    while len(hits) < n:
        size = min(rng.randint(1, 5), n - len(hits))
        longest = rng.randrange(size)
        for i in range(size):
            lo = x + 100 * i
            hi = lo + 299 + (1 if i == longest else 0)
            qs, qe = (lo, hi) if rng.random() < 0.5 else (hi, lo)
            hits.append((qs, qe, rng.randint(0, 1), PASS, (base, k)))
        x += 100 * (size - 1) + 301 + 50
        k += 1
    return hits, x


def with_rejects(hits, n_rej, rng, span):
    """Shuffle the passing hits and interleave n_rej hits below --min-scov at random file
    positions; the rejected hits are long, so a kept one would bridge chains."""
    hits = list(hits)
    rng.shuffle(hits)
    for _ in range(n_rej):
        lo = rng.randint(1, max(span, 2))
        rej = (lo, lo + rng.randint(200, 2000), rng.randint(0, 1), FAIL, None)
        hits.insert(rng.randint(0, len(hits)), rej)
    return hits


def sized_group(n, n_rej, seed):
    rng = random.Random(seed)
    hits, span = clusters(n, rng)
    return with_rejects(hits, n_rej, rng, span)


def chain(n, cut=None, weak=False, base=1):
    """Intervals of 150 at step 100: i overlaps only i +- 1 (50/150).  cut=k: every k-th
    link is broken, by 100 free bases or (weak) by an overlap of 5 bases, 5/150 < 0.1."""
    hits, x, comp = [], base, 0
    for i in range(n):
        if i and cut and i % cut == 0:
            x += 45 if weak else 150
            comp += 1
        hits.append((x, x + 149, 1 if i % 11 == 0 else 0, PASS, (base, comp)))
        x += 100
    return hits


def family_s():
    cases = [Case("S_pass{}".format(n), [sized_group(n, n // 7 + 3, 100 + n)]) for n in SIZES]
    rng = random.Random(5000)
    hits, span = clusters(CAP_MAX, rng)
    cases.append(Case("S_4096_of_5000", [with_rejects(hits, 5000 - CAP_MAX, rng, span)]))
    cases.append(Case("S_4097_refused", [sized_group(5, 2, 1), [], sized_group(CAP_MAX + 1, 600, 2),
                                         sized_group(7, 0, 3)], refused_group=2))
    return cases


def family_t():
    cases = []
    for n in TOPO_SIZES:
        rng = random.Random(n)
        c = chain(n)
        shuffled = list(c)
        rng.shuffle(shuffled)
        cut = chain(n, cut=7)
        rng.shuffle(cut)
        cases.append(Case("T_chain_{}".format(n), [c]))
        cases.append(Case("T_chain_cut7_{}".format(n), [chain(n, cut=7)]))
        cases.append(Case("T_chain_cut7_shuffled_{}".format(n), [cut]))
        cases.append(Case("T_chain_reversed_{}".format(n), [c[::-1]]))
        cases.append(Case("T_chain_shuffled_{}".format(n), [shuffled]))
        # one interval holds all the others (disjoint, 40 long): every pair with it scores 1.0
        inner = [(101 + 50 * i, 140 + 50 * i, i % 2, PASS, 0) for i in range(n - 1)]
        box = (1, 50 * n + 200, 1, PASS, 0)
        mixed = inner[:n // 2] + [box] + inner[n // 2:]
        cases.append(Case("T_container_{}".format(n), [mixed]))
        # star: the hub is not first in start order; one spoke overhangs each end
        hub = (500, 500 + 50 * n, 0, PASS, 0)
        spokes = [(510 + 50 * i, 540 + 50 * i, 1, PASS, 0) for i in range(n - 3)]
        left, right = (300, 560, 1, PASS, 0), (440 + 50 * n, 800 + 50 * n, 1, PASS, 0)
        star = spokes + [right, hub, left]
        rng.shuffle(star)
        cases.append(Case("T_star_{}".format(n), [star]))
        # chains joined by weak overlaps only: two chains in alternating file order, and many
        two = chain(n, cut=(n + 1) // 2, weak=True)
        half = (n + 1) // 2
        alt = [h for pair in zip(two[:half], two[half:] + [None]) for h in pair if h is not None]
        assert len(alt) == n
        cases.append(Case("T_weak_links_two_{}".format(n), [alt]))
        many = chain(n, cut=5, weak=True)
        rng.shuffle(many)
        cases.append(Case("T_weak_links_many_{}".format(n), [many]))
    # a weak neighbour sorts before a strong one: x-w 11/1000 and no edge, x-z 9/12, z in w
    x, w, z = (1, 1000, 0, PASS, 0), (990, 3000, 1, PASS, 0), (992, 1003, 0, PASS, 0)
    cases.append(Case("T_weak_then_strong", [[x, w, z], [z, w, x], [w, x, z]]))
    return cases


def family_k():
    cases = []
    # equal starts, no edges (containment scores exactly 1.0 < threshold): the output order
    # is the stable sort by start
    ties = [(100, 400, 0), (100, 250, 1), (100, 900, 1), (100, 250, 0), (50, 900, 0),
            (100, 100, 1), (50, 60, 1), (100, 400, 1)]
    orders = [ties, ties[::-1], ties[3:] + ties[:3], sorted(ties, key=lambda t: -t[1])]
    cases.append(Case("K_stable_sort", [[(a, b, s, PASS, i) for i, (a, b, s) in enumerate(o)]
                                        for o in orders], min_overlap=1.0000001))
    # strand of the longest member; equal longest lengths of both strands give "-"
    cases.append(Case("K_strand", [
        [(1, 300, 0, PASS, 0), (101, 400, 1, PASS, 0), (150, 200, 0, PASS, 0)],
        [(1, 300, 1, PASS, 0), (101, 400, 0, PASS, 0), (150, 200, 0, PASS, 0)],
        [(101, 400, 0, PASS, 0), (1, 300, 1, PASS, 0)],
        [(1, 300, 0, PASS, 0), (101, 350, 1, PASS, 0), (150, 200, 1, PASS, 0)],
        [(101, 350, 1, PASS, 0), (150, 200, 1, PASS, 0), (1, 300, 0, PASS, 0)],
        [(1, 300, 1, PASS, 0), (101, 350, 0, PASS, 0)],
    ]))
    # ov/den exactly the threshold as a double (one gene), then one base less (two genes)
    def duo(a, b, joined):
        return [(a[0], a[1], 0, PASS, 0), (b[0], b[1], 1, PASS, 0 if joined else 1)]
    cases.append(Case("K_overlap_at_0.1", [
        duo((1, 100), (91, 250), True), duo((1, 100), (92, 250), False),
        duo((1, 10), (10, 19), True), duo((1, 10), (11, 20), False),
        duo((1, 30), (28, 57), True), duo((1, 30), (29, 58), False),
        duo((28, 57), (1, 30), True), duo((29, 58), (1, 30), False),
    ], min_overlap=0.1))
    cases.append(Case("K_overlap_at_0.5", [
        duo((1, 2), (2, 3), True), duo((1, 2), (3, 4), False),
        duo((1, 100), (51, 200), True), duo((1, 100), (52, 200), False),
    ], min_overlap=0.5))
    cases.append(Case("K_overlap_at_1.0", [
        duo((1, 100), (20, 50), True), duo((1, 100), (20, 101), False),
        duo((1, 100), (1, 100), True), duo((1, 100), (1, 40), True), duo((1, 100), (2, 101), False),
    ], min_overlap=1.0))
    # --min-overlap <= 0: every pair is an edge, disjoint ones too
    rng = random.Random(77)
    scattered = [(a, a + rng.randint(10, 400), rng.randint(0, 1), PASS, 0)
                 for a in (rng.randint(1, 90000) for _ in range(300))]
    far = [(1, 50, 0, PASS, 0), (100000, 100200, 1, PASS, 0), (500, 520, 0, PASS, 0)]
    for t in (0.0, -0.5):
        cases.append(Case("K_min_overlap_{}".format(t), [scattered, far, far[:1], []],
                          min_overlap=t))
    # merged length exactly --min-gene-length and one less
    exact = [(1, 120, 0, PASS, 0), (81, 200, 1, PASS, 0)]
    short = [(1, 120, 0, PASS, 0), (81, 199, 1, PASS, 0)]
    long_ = [(1, 120, 0, PASS, 0), (81, 201, 1, PASS, 0)]
    both = exact + [(1001, 1199, 0, PASS, 1), (2001, 2200, 1, PASS, 2), (3001, 3201, 0, PASS, 3)]
    cases.append(Case("K_gene_length_200", [exact, short, long_, both], min_gene_length=200.0))
    cases.append(Case("K_gene_length_200.5", [exact, short, long_, both], min_gene_length=200.5))
    # scov exactly --min-scov is kept, the next double below is not
    below = float(np.nextafter(0.75, 0.0))
    cases.append(Case("K_scov_exact", [
        [(1, 300, 0, 0.75, 0), (1, 5000, 1, below, None), (1001, 1300, 1, 0.75, 1)],
        [(1, 5000, 1, below, None)],
        [(1, 300, 0, float(np.nextafter(0.75, 1.0)), 0), (250, 600, 1, 0.75, 0)],
    ]))
    # qstart > qend
    cases.append(Case("K_reversed_coordinates", [
        [(300, 1, 0, PASS, 0), (250, 600, 1, PASS, 0), (1200, 900, 1, PASS, 1)],
        [(600, 250, 1, PASS, 0), (1, 300, 0, PASS, 0)],
        [(5, 5, 0, PASS, 0), (6, 6, 1, PASS, 1), (5, 5, 1, PASS, 0)],
    ]))
    return cases


G_SIZES = [0, 1, 2, 5, 40, 64, 65, 300]


@functools.lru_cache(maxsize=None)
def family_g(n_groups=10000):
    """Many groups in one call: sizes from G_SIZES in a fixed shuffled order with large and
    small groups as neighbours, one group of 4096, empty groups and groups whose hits are
    all rejected.  Each group is sized_group(), so its genes are known."""
    rng = random.Random(31)
    groups = []
    for g in range(n_groups):
        if g == n_groups // 2:
            groups.append(sized_group(CAP_MAX, 0, 999))
        elif g % 2:
            groups.append(sized_group(rng.choice([0, 1, 2, 5]), rng.randint(0, 3), g))
        elif g % 50 == 0:                       # nothing passes
            groups.append(sized_group(0, rng.choice([1, 40, 65]), g))
        else:
            n = rng.choice(G_SIZES)
            groups.append(sized_group(n, rng.choice([0, 0, 3, n // 4]), g))
    # 350: a chain of one interval (300 or 301 long) is dropped, longer chains stay
    return Case("G_{}_groups".format(n_groups), groups, min_gene_length=350.0)


@functools.lru_cache(maxsize=None)
def all_cases():
    """Families S, T and K (G is family_g())."""
    return tuple(family_s() + family_t() + family_k())


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """The oracle's genes of a case, computed once per process."""
    if name.startswith("G_"):
        return family_g().oracle()
    return {c.name: c for c in all_cases()}[name].oracle()
