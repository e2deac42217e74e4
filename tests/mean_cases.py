"""Segment-mean cases at every locus length and kernel route, with a plain numpy reference.

Every call, crit and rank rests on one operation: the float64 mean of a locus's site array,
summed in numpy's order.  The device computes it along several routes chosen by the locus
length `n`, by numpy's leaf count `nl(n)` and by the number of attachments `na` of the
segment (closed forms, the leaf-table walk, the wave / lane / flat multi-attachment paths,
the staged leaf kernels).  This module builds contigs that sit on both sides of every such
change-over, as in-memory `HostBatch` objects (no text files, so a hit's score can be any
double), and computes what they must give with numpy alone: paint `np.zeros(n)` with
`np.maximum` over each hit's slice, exactly as the reference's contig model does, Python's
slice wrap included, then `np.mean`.  Nothing here restates device code.

Families (one contig is one case; a single-locus contig has crit == rank == the mean):
  A  one run at level 0: one species, one hit, every n in 1..8191 and the long EDGE lengths
  B  several attachments of one species on one locus, na across every routing threshold
  C  --min-overlap 0 painting of hits that lie wholly outside a long locus
  D  roll-up: sister species cover islands whose union alone passes -k1
  E  A (at the EDGE lengths), B and D contigs shuffled into one batch
  F  63 .. 200 clades that each explain the contig alone, per slice size of the wave kernels
"""
import functools
import os
import re

import numpy as np

from waafle_amd.inputs import HostBatch
from waafle_amd.taxonomy import TaxonomyTables

HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------------------
# lengths
# ---------------------------------------------------------------------------

def nl(n):
    """numpy's leaf count of one reduction buffer of n elements (pairwise_sum's split)."""
    if n <= 0:
        return 0
    if n <= 128:
        return 1
    h = n // 2
    h -= h % 8
    return nl(h) + nl(n - h)


EDGE = sorted({1, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 137, 255, 256, 257, 1031, 2047,
               2048, 2049,
               3848, 3849, 4096, 4097, 7688, 7689, 8190, 8191,
               8192, 8193, 8320, 16383, 16384, 16385, 20000,
               65535, 65536, 65537})
ALL = list(range(1, 8192))
NPY_BUF = 8192

# The routing thresholds these lengths straddle: one thread finishes a segment of <= 32
# leaves (kThreadLeaves), the wave paths take <= 64 leaves.  Leaf counts are not monotone
# in n; if the kernels' leaf gates change, these point to the lengths to update.
_NL = [nl(n) for n in range(NPY_BUF)]
assert min(n for n in range(NPY_BUF) if _NL[n] > 32) == 3849
assert min(n for n in range(NPY_BUF) if _NL[n] > 64) == 7689
assert _NL[8191] == 65


def multi_att0():
    """kMultiAtt0 of the wave kernels (the attachment count of their envelope buffer)."""
    path = os.path.join(os.path.dirname(HERE), "waafle_amd", "csrc", "wf_fast.hip")
    with open(path) as fh:
        m = re.search(r"constexpr\s+int\s+kMultiAtt0\s*=\s*(\d+)\s*;", fh.read())
    assert m, "kMultiAtt0 not found in wf_fast.hip"
    return int(m.group(1))


NA = sorted({2, 3, 4, 5, 16, 17, 64, 65, 66, 130, multi_att0(), multi_att0() + 1})
ROLL_K = (2, 5, 17, 65)

# ---------------------------------------------------------------------------
# taxonomy: species under genera under one family under r__Root
# ---------------------------------------------------------------------------

N_GENERA, N_SPECIES = 5, 70
EDGES = [("f__F", "r__Root")]
for _g in range(N_GENERA):
    EDGES.append(("g__G{}".format(_g), "f__F"))
    for _k in range(N_SPECIES):
        EDGES.append(("s__S{}_{:02d}".format(_g, _k), "g__G{}".format(_g)))
TAX = TaxonomyTables(EDGES)


def species(g, k):
    return "s__S{}_{:02d}".format(g, k)


FLAGS_ONE = ["-k1", "1e-6", "-k2", "1e-6", "--min-gene-length", "1"]
FLAGS_OVERLAP0 = FLAGS_ONE + ["--min-overlap", "0"]
FLAGS_ROLL = ["-k1", "0.9", "-k2", "0.9", "--weak-loci", "penalize", "--min-gene-length", "1"]


# ---------------------------------------------------------------------------
# contigs
# ---------------------------------------------------------------------------

class Contig:
    """loci: [(start, end)] 1-based inclusive; hits: [(locus index, qlo, qhi, species, score)]
    in file order.  `clade`: the expected clade1 name (None: not fixed); `iterations`: the expected count;
    `union`: the reported option's gene scores are the means of the union envelope of all
    hits (one species, or sisters rolled up into one clade), so `direct()` applies."""

    def __init__(self, name, meta, clade, iterations=1, union=True):
        self.name, self.meta, self.clade = name, meta, clade
        self.iterations, self.union = iterations, union
        self.loci, self.hits = [], []
        self.end = 0

    def add_locus(self, n, margin=0):
        """A locus of n sites with `margin` free sites before it; returns its index."""
        start = self.end + 32 + margin
        self.loci.append((start, start + n - 1))
        self.end = start + n - 1 + 32 + margin
        return len(self.loci) - 1

    def add_run(self, g, lo, hi, sp, score):
        """A hit over the sites [lo, hi) of locus g (lo may be < 0, hi > n: overhang)."""
        start = self.loci[g][0]
        assert start + lo >= 1 and hi > lo
        self.hits.append((g, start + lo, start + hi - 1, sp, float(score)))

    def n(self, g=0):
        return self.loci[g][1] - self.loci[g][0] + 1

    def site_arrays(self):
        """Per locus, the envelope of every hit: np.zeros painted with np.maximum over each
        hit's slice (the reference's ContigModel._paint, the slice's wrap included)."""
        arrays = [np.zeros(self.n(g)) for g in range(len(self.loci))]
        for g, qlo, qhi, _, score in self.hits:
            start, a = self.loci[g][0], arrays[g]
            first = max(0, qlo - start)
            last = min(len(a) - 1, qhi - start)
            a[first:last + 1] = np.maximum(a[first:last + 1], score)
        return arrays

    def direct(self):
        """(crit, rank) by numpy alone: min and mean of the per-locus np.mean."""
        means = np.array([np.mean(a) for a in self.site_arrays()])
        return np.min(means), np.mean(means)


def to_batch(contigs):
    """In-memory HostBatch of the contigs (scov 1, no annotation systems, '+' strands)."""
    N = len(contigs)
    hit_off = np.zeros(N + 1, dtype=np.int64)
    loc_off = np.zeros(N + 1, dtype=np.int64)
    np.cumsum([len(c.hits) for c in contigs], out=hit_off[1:])
    np.cumsum([len(c.loci) for c in contigs], out=loc_off[1:])
    hits = [h for c in contigs for h in c.hits]
    loci = [l for c in contigs for l in c.loci]
    H = len(hits)
    names = [c.name for c in contigs]
    assert len(set(names)) == N
    return HostBatch(
        contig_names=names, contig_lengths=np.array([c.end + 1 for c in contigs], dtype=np.int64),
        hit_off=hit_off, hit_qlo=np.array([h[1] for h in hits], dtype=np.int32),
        hit_qhi=np.array([h[2] for h in hits], dtype=np.int32),
        hit_taxon=np.array([TAX.index[h[3]] for h in hits], dtype=np.int32),
        hit_strand=np.zeros(H, dtype=np.int8),
        hit_score=np.array([h[4] for h in hits], dtype=np.float64),
        hit_scov=np.ones(H, dtype=np.float64), hit_sysmask=np.zeros(H, dtype=np.uint32),
        loc_off=loc_off, loc_start=np.array([l[0] for l in loci], dtype=np.int32),
        loc_end=np.array([l[1] for l in loci], dtype=np.int32),
        loc_strand=np.zeros(len(loci), dtype=np.int8),
        loc_codes=["{}:{}:+".format(a, b) for a, b in loci], systems=[],
        annot_value_ids=np.full((H, 1), -1, dtype=np.int32), annot_values=[[]],
        hit_row=np.arange(H, dtype=np.int64))


class CaseSet:
    """The contigs of one score call: batch, flags and the direct numpy values."""

    def __init__(self, key, contigs, flags):
        self.key, self.contigs, self.flags = key, contigs, list(flags)
        self.batch = to_batch(contigs)
        self.tax = TAX
        self.clade = np.array([-1 if c.clade is None else TAX.index[c.clade] for c in contigs],
                              dtype=np.int32)       # -1: whatever the oracle melds
        self.iterations = np.array([c.iterations for c in contigs])
        self.has_direct = np.array([c.union for c in contigs])
        self.single = np.array([len(c.loci) == 1 for c in contigs])
        self._direct = None

    @property
    def direct(self):
        """(crit, rank) float64 arrays, NaN where the contig has no direct value."""
        if self._direct is None:
            crit = np.full(len(self.contigs), np.nan)
            rank = np.full(len(self.contigs), np.nan)
            for i, c in enumerate(self.contigs):
                if c.union:
                    crit[i], rank[i] = c.direct()
            self._direct = (crit, rank)
        return self._direct

    def max_len(self):
        return max(c.n(g) for c in self.contigs for g in range(len(c.loci)))


def _score(rng, lo=0.5, hi=1.0):
    """A non-dyadic double in (lo, hi): the order of summation shows in the low bits."""
    return float(rng.uniform(lo, hi))


# ---------------------------------------------------------------------------
# A: one run at level 0
# ---------------------------------------------------------------------------

RUNS_A = ("whole", "prefix", "suffix", "tiny", "inner", "overhang")


def one_run_contigs(lengths, seed):
    """The six runs per length.  The run of 1-9 sites is built at every EDGE length and at
    every third other length: k <= 3 equal values have the same sum in any order of
    addition and k <= 9 mostly so, whatever the score, so this run tells summation orders
    apart for about a quarter of the lengths; built at every length it would hold family A
    below the 90 % discrimination that test_mean_cases.py demands of the family."""
    rng = np.random.default_rng(seed)
    edge = set(EDGE)
    out = []
    for n in lengths:
        for kind in RUNS_A:
            if kind == "tiny" and n % 3 and n not in edge:
                continue
            if kind == "whole":
                lo, hi = 0, n
            elif kind == "prefix":
                if n < 2:
                    continue
                lo, hi = 0, int(rng.integers(1, n))
            elif kind == "suffix":
                if n < 2:
                    continue
                lo, hi = int(rng.integers(1, n)), n
            elif kind == "tiny":                   # an interior run of 1-9 sites
                if n < 3:
                    continue
                w = min(int(rng.integers(1, 10)), n - 2)
                lo = int(rng.integers(1, n - w))
                hi = lo + w
            elif kind == "inner":
                if n < 3:
                    continue
                lo = int(rng.integers(1, n - 1))
                hi = int(rng.integers(lo + 1, n))
            else:                                  # overhangs both locus ends: clipped
                lo, hi = -int(rng.integers(1, 20)), n + int(rng.integers(1, 20))
            sp = species(int(rng.integers(N_GENERA)), int(rng.integers(N_SPECIES)))
            v = _score(rng)
            c = Contig("A{}_{}".format(n, kind), dict(family="A", n=n, kind=kind, lo=lo, hi=hi, v=v), sp)
            g = c.add_locus(n, margin=20)
            c.add_run(g, lo, hi, sp, v)
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def family_a():
    lengths = ALL + [n for n in EDGE if n >= NPY_BUF]
    return CaseSet("A", one_run_contigs(lengths, 1001), FLAGS_ONE)


@functools.lru_cache(maxsize=None)
def family_a_edge():
    return CaseSet("A_edge", one_run_contigs(EDGE, 1002), FLAGS_ONE)


# ---------------------------------------------------------------------------
# B: several attachments of one species on one locus
# ---------------------------------------------------------------------------

PATTERNS_B = ("staircase", "pyramid", "islands", "abutting", "whole_top", "whole_middle", "ties")


def _partial(rng, n):
    lo = int(rng.integers(0, n - 1))
    hi = int(rng.integers(lo + 1, n)) if lo > 0 else int(rng.integers(1, n))
    return lo, hi


def multi_runs(pattern, n, na, rng):
    """na runs (lo, hi, score) over a locus of n >= 128 sites, in file order."""
    runs = []
    if pattern == "staircase":                     # overlapping, rising scores, na distinct runs
        w = max(2, (2 * n) // (na + 1))
        sc = np.sort(rng.uniform(0.5, 1.0, na))
        for i in range(na):
            lo = (i * n) // (na + 1)
            runs.append((lo, min(n, lo + w), sc[i]))
    elif pattern == "pyramid":                     # nested, narrower is higher
        sc = np.sort(rng.uniform(0.5, 1.0, na))
        for i in range(na):
            lo = 1 + (i * (n // 2 - 1)) // na
            runs.append((lo, n - lo, sc[i]))
    elif pattern == "islands":                     # one-site gaps, one-site islands among them
        for i in range(na):
            a, b = (i * n) // na, ((i + 1) * n) // na
            a, b = min(a, n - 1), max(b, min(a, n - 1) + 1)
            if b - a >= 2:
                b -= 1                             # the gap
                if i % 3 == 1:
                    a = b - 1                      # a one-site island
            runs.append((a, b, _score(rng)))
    elif pattern == "abutting":
        for i in range(na):
            a = min((i * n) // na, n - 1)
            runs.append((a, max(((i + 1) * n) // na, a + 1), _score(rng)))
    elif pattern == "whole_top":                   # prunes to one run
        top = _score(rng, 0.9, 1.0)
        runs = [_partial(rng, n) + (_score(rng, 0.5, 0.9),) for _ in range(na - 1)]
        runs.insert(int(rng.integers(na)), (0, n, top))
    elif pattern == "whole_middle":                # survivors, then the whole-locus hit again
        mid = _score(rng, 0.7, 0.75)
        for i in range(na - 1):
            lohi = _partial(rng, n)
            runs.append(lohi + ((_score(rng, 0.75, 1.0) if i % 2 == 0 else _score(rng, 0.5, 0.7)),))
        runs.insert(int(rng.integers(na)), (0, n, mid))
    elif pattern == "ties":                        # a partial hit with the whole-locus score
        mid = _score(rng, 0.7, 0.75)
        runs = [_partial(rng, n) + (mid,)]
        for i in range(na - 2):
            lohi = _partial(rng, n)
            runs.append(lohi + ((mid, _score(rng, 0.75, 1.0), _score(rng, 0.5, 0.7))[i % 3],))
        order = rng.permutation(len(runs))
        runs = [runs[i] for i in order]
        runs.insert(int(rng.integers(na)), (0, n, mid))
    else:
        raise KeyError(pattern)
    assert len(runs) == na and all(0 <= lo < hi <= n for lo, hi, _ in runs)
    return runs


def multi_contigs(seed=2001):
    """Every (length, na), the patterns rotating: each pattern, na and length many times."""
    rng = np.random.default_rng(seed)
    out = []
    lengths = [n for n in EDGE if n >= 128]
    for li, n in enumerate(lengths):
        for ni, na in enumerate(NA):
            pattern = PATTERNS_B[(li + ni) % len(PATTERNS_B)]
            sp = species(int(rng.integers(N_GENERA)), int(rng.integers(N_SPECIES)))
            c = Contig("B{}_{}_{}".format(n, na, pattern),
                       dict(family="B", n=n, na=na, pattern=pattern), sp)
            g = c.add_locus(n)
            for lo, hi, v in multi_runs(pattern, n, na, rng):
                c.add_run(g, lo, hi, sp, v)
            out.append(c)
    return out


# ---------------------------------------------------------------------------
# C: --min-overlap 0 painting at long loci
# ---------------------------------------------------------------------------

def outside_contigs(seed=3001):
    """A hit wholly left of the locus by d sites (its slice [0 : 1 - d] wraps from the end,
    or is empty), or wholly right of it (empty), and one ordinary partial hit."""
    rng = np.random.default_rng(seed)
    out = []
    for n in [n for n in EDGE if n >= 3848]:
        for tag, d in (("l1", 1), ("l2", 2), ("lthird", n // 3), ("ln", n), ("ln5", n + 5),
                       ("right", None)):
            sp = species(int(rng.integers(N_GENERA)), int(rng.integers(N_SPECIES)))
            c = Contig("C{}_{}".format(n, tag), dict(family="C", n=n, kind=tag), sp)
            g = c.add_locus(n, margin=n + 64)
            w = int(rng.integers(1, 40))
            va, vb = _score(rng), _score(rng)
            if d is None:
                off = int(rng.integers(1, 30))
                c.add_run(g, n - 1 + off, n - 1 + off + w, sp, va)
            else:
                c.add_run(g, 1 - d - w, 1 - d, sp, va)       # last site: d before the locus
            lo, hi = _partial(rng, n)
            c.add_run(g, lo, hi, sp, vb)
            if int(rng.integers(2)):
                c.hits.reverse()
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def family_bc():
    """B and C in one batch: --min-overlap 0 changes nothing for hits inside their locus."""
    return CaseSet("BC", multi_contigs() + outside_contigs(), FLAGS_OVERLAP0)


# ---------------------------------------------------------------------------
# D: roll-up
# ---------------------------------------------------------------------------

def _islands(c, g, n, k, genera, rng):
    """k species each cover one island of locus g; neighbours overlap by up to 3 sites, the
    union covers the locus; every score is in (0.92, 1), so only the union reaches 0.9."""
    while True:
        cuts = [0] + sorted(rng.choice(np.arange(1, n), size=k - 1, replace=False).tolist()) + [n]
        los = [max(0, cuts[i] - int(rng.integers(0, 4))) for i in range(k)]
        cover = [0] * max(genera, k)               # per species, and per genus when several
        for i in range(k):
            cover[i if genera == 1 else i % genera] += cuts[i + 1] - los[i]
        if max(cover) <= 0.88 * n:                 # alone, none reaches 0.9 (scores < 1)
            break
    for i in range(k):
        c.add_run(g, los[i], cuts[i + 1], species(i % genera, i // genera), _score(rng, 0.92, 1.0))


def rollup_contigs(seed=4001, union=True):
    rng = np.random.default_rng(seed)
    out = []
    lengths = [n for n in EDGE if n >= 128]
    for n in lengths:
        for k in ROLL_K:
            for genera in (1, min(k, 3)):
                clade, its = ("g__G0", 2) if genera == 1 else ("f__F", 3)
                if not union:
                    clade, its = None, 1
                c = Contig("D{}_{}_{}".format(n, k, genera),
                           dict(family="D", n=n, k=k, genera=genera), clade, its, union)
                _islands(c, c.add_locus(n), n, k, genera, rng)
                out.append(c)
    # several such loci of different lengths in one contig: crit = min, rank = mean over loci
    groups = [(136, 3849, 8191), (129, 7688, 20000), (2049, 3848, 7689), (255, 4097, 8192),
              (136, 3849, 8191, 8192, 20000), (128, 1031, 4096, 8190, 16385),
              (257, 2048, 7689, 8193, 65537), (137, 3849, 7688, 8191, 65536)]
    for gi, lens in enumerate(groups):
        for k in ROLL_K:
            genera = 1 if (gi + k) % 2 else min(k, 3)
            clade, its = ("g__G0", 2) if genera == 1 else ("f__F", 3)
            if not union:
                clade, its = None, 1
            c = Contig("D{}x_{}_{}_{}".format(len(lens), gi, k, genera),
                       dict(family="D", n=lens, k=k, genera=genera), clade, its, union)
            for n in lens:
                _islands(c, c.add_locus(n), n, k, genera, rng)
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def family_d():
    return CaseSet("D", rollup_contigs(), FLAGS_ROLL)


# ---------------------------------------------------------------------------
# E: neighbours in one batch
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def family_e():
    """The one-run cases at the EDGE lengths between multi-attachment and island contigs, in
    one shuffled batch under family A's flags.  There every island species passes -k1 by
    itself, so an island contig is many one-run segments and reports its best species'
    mean, melded with the species within --range of it: the oracle gives its clade and
    values (no direct value)."""
    isl = rollup_contigs(seed=5003, union=False)
    contigs = one_run_contigs(EDGE, 5001) + multi_contigs(seed=5002) + isl
    for c in contigs:
        c.name = "E_" + c.name
    order = np.random.default_rng(5004).permutation(len(contigs))
    return CaseSet("E", [contigs[i] for i in order], FLAGS_ONE)


# ---------------------------------------------------------------------------
# F: more explain_one options than a wave has lanes
# ---------------------------------------------------------------------------

FLAGS_MELD_ALL = FLAGS_ONE + ["--range", "1.0"]
SLICES = (224, 256, 512)      # the wave kernels' slice sizes: chosen by the batch's max hits


@functools.lru_cache(maxsize=None)
def family_f(cap):
    """K species with one run each on every locus of a contig: K one-run segments per locus
    and K options for explain_one, all within --range 1.0 of the best, so the meld lists
    every option the kernel found.  K on both sides of 64 and 128; the batch's longest
    contig has more hits than the next smaller slice holds and no more than `cap`, so the
    wave kernels run it in their `cap`-attachment slice.  (Family E's batch found the case:
    in the 512 slice the options past the 64th were lost.)  The oracle gives the values."""
    below = max([0] + [c for c in SLICES if c < cap])
    out = []
    for K in (63, 64, 65, 66, 100, 128, 129, 200):
        for G in (1, 2, 3):
            if K * G > cap:
                continue
            c = Contig("F{}_{}_{}".format(cap, K, G), dict(family="F", k=K, loci=G), "f__F", 1, False)
            for g in range(G):
                gi = c.add_locus(300 + 100 * g)
                for i in range(K):
                    v = 0.6 + 0.001 * ((i * 37 + 11 * g) % 300) + 1e-7 * i
                    c.add_run(gi, i, i + 90 + (i % 7), species(i % N_GENERA, i // N_GENERA), v)
            out.append(c)
    cs = CaseSet("F{}".format(cap), out, FLAGS_MELD_ALL)
    assert below < cs.batch.max_hits <= cap
    return cs


# ---------------------------------------------------------------------------
# the oracle over a case set (computed once per process)
# ---------------------------------------------------------------------------

_ORACLE = {}


def oracle_for(cs):
    """The CPU oracle's Results for the case set's batch."""
    if cs.key not in _ORACLE:
        from oracle import orgscorer_oracle as orc
        from oracle_bridge import oracle_hits_from_batch, oracle_loci_from_batch, oracle_results
        from waafle_amd import cli
        params = orc.Params(**cli.param_dict(cli.parse_flags(cs.flags)))
        b = cs.batch
        contigs = orc.score_contigs(dict(zip(b.contig_names, b.contig_lengths.tolist())),
                                    oracle_loci_from_batch(b), oracle_hits_from_batch(b, cs.tax),
                                    orc.Taxonomy(EDGES), params)
        _ORACLE[cs.key] = oracle_results(contigs, b, cs.tax)
    return _ORACLE[cs.key]
