"""Contigs for explain_two on the compact table (sp_two, wf_sparse.h), built on mean_cases'
in-memory batches: 2-63 loci of 8 or 16 sites, 2-210 hits.  The kernel evaluates each
candidate pair once -- the whole wave on a pair when there are few, a lane per pair beyond
that, the first 64 kept in registers -- so the cases vary what that changes: the number of
candidate pairs (1 .. 100, at level 0 and among genera at level 1), the number of unmasked
loci and the gaps between them (numpy's summation branches), the selection (ties, the
--range edge, one or several options within it, equal and unequal synteny), and every
branch of the synteny and the LGT checks, each with one candidate pair and among twenty.
The oracle gives every expected value; `want` on a contig states what the case is meant to
be (tests/test_two_pair_cases.py checks it against a trace of the oracle's two_clade).

Thresholds (dyadic): -k1 0.5 -k2 0.75 (kmin = k_amb = the sister threshold = 0.5),
--range 0.0625.  A clade "on" a locus has one whole-locus hit there, so its gene score is the
hit's score.  A pair (a, b) is a candidate when every unmasked locus has one of them at or
above k2; no clade alone reaches k1 on every locus, so explain_one never answers first.
"""
import functools

import numpy as np

import env_cases as ec
import mean_cases as mc
from mean_cases import CaseSet, Contig, species
from env_cases import WideCaseSet, wide_species

FLAGS = ["-k1", "0.5", "-k2", "0.75", "--range", "0.0625", "--min-gene-length", "1"]
FLAGS_UNK = ["-k1", "0.75", "-k2", "0.5", "--range", "0.0625", "--min-gene-length", "1",
             "--weak-loci", "assign-unknown"]
STEP = 0.001
LGT, NO_LGT, NONE = "lgt", "no_lgt", "unclassified"

# (candidate pairs) -> (clades on locus 0, clades on locus 1)
GRID = {1: (1, 1), 2: (1, 2), 3: (1, 3), 7: (1, 7), 8: (2, 4), 9: (3, 3), 16: (1, 16),
        63: (7, 9), 64: (8, 8), 65: (5, 13), 100: (10, 10)}


def contig(name, want, **meta):
    """want: (roll-up level of the designed explain_two call, its candidate pairs, those
    within --range of the best, the contig's call)."""
    c = Contig(name, dict(family="two", want=want, **meta), None, union=False)
    return c


def whole(c, g, sp, score):
    c.add_run(g, 0, c.n(g), sp, score)


def _scores(rng, n, lo, hi):
    return [float(x) for x in rng.uniform(lo, hi, n)]


# ---------------------------------------------------------------------------
# the number of candidate pairs
# ---------------------------------------------------------------------------

def grid_cases():
    """na species of genus 0 on locus 0, nb of genus 1 on locus 1: na * nb candidate pairs.
    Half of the locus-1 species (rounded up) score 0.97 .. 1, the others 0.75 .. 0.8, the
    locus-0 ones 0.97 .. 1: ranks within 0.03 of the best for the first kind, at least 0.085
    below it for the second."""
    rng = np.random.default_rng(7001)
    out = []
    for n, (na, nb) in GRID.items():
        high = (nb + 1) // 2
        c = contig("grid_{}".format(n), (0, n, na * high, LGT), pairs=n)
        c.add_locus(8), c.add_locus(16)
        sa = _scores(rng, na, 0.97, 1.0)
        sb = _scores(rng, high, 0.97, 1.0) + _scores(rng, nb - high, 0.75, 0.8)
        order = rng.permutation(nb)
        for i in range(na):
            whole(c, 0, species(0, i), sa[i])
        for j in range(nb):
            whole(c, 1, species(1, j), sb[order[j]])
        out.append(c)
    return out


def grid_l1_cases(decided):
    """The same among genera: genus i < na has locus 0 whole by one species, genus na + j has
    locus 1 as two sister species' halves (each alone scores <= 0.5: no potential clade, so no
    pair at level 0), merged at level 1 into a segment of the mean of the two.  A hit of the
    last genus at 0.5625 keeps locus 1 unmasked at level 0.  Under the strict sister penalty
    every pair is rejected (the other genera, the last one among them, are sisters scoring on
    the pair's loci) and the family explains the contig at level 2; `decided`: the set's
    flags switch the penalty off and allow the LCA, so the melded pair is reported."""
    rng = np.random.default_rng(7002)
    out = []
    for n, (na, nb) in GRID.items():
        high = (nb + 1) // 2
        call = LGT if decided else NO_LGT
        c = contig("grid_l1_{}".format(n), (1, n, na * high, call), pairs=n)
        c.add_locus(8), c.add_locus(8)
        sa = _scores(rng, na, 0.97, 1.0)
        sb = _scores(rng, high, 0.97, 0.99) + _scores(rng, nb - high, 0.76, 0.8)
        order = rng.permutation(nb)
        for i in range(na):
            whole(c, 0, wide_species(i, 0), sa[i])
        for j in range(nb):
            m = sb[order[j]]
            ec.sisters(c, 1, na + j, m + 0.0078125, m - 0.0078125, sp=wide_species)
        whole(c, 1, wide_species(ec.WIDE_GENERA - 1, 0), 0.5625)
        out.append(c)
    return out


# ---------------------------------------------------------------------------
# the number of unmasked loci
# ---------------------------------------------------------------------------

GU = (2, 7, 8, 9, 15, 16, 17, 63)


def gu_cases():
    """Gu unmasked loci with a masked one (its only hit scores 0.25 < kmin) after every
    second of them while the contig stays within 63 loci.  Species B of genus 1 holds the
    unmasked loci u = 1 (mod 5), species A of genus 0 the others; on u = 3 (mod 7) the other
    of the two is present as well, below every threshold.  Scores are not dyadic, so the
    order of the rank's additions shows in its low bits.  `x10`: nine more species of genus
    1 on B's loci, all ten pairs within --range (scores 0.9 .. 1 on at most half the loci)."""
    rng = np.random.default_rng(7003)
    out = []
    for gu in GU:
        for many in (False, True):
            pairs = 10 if many else 1
            c = contig("gu_{}{}".format(gu, "_x10" if many else ""), (0, pairs, pairs, LGT), gu=gu)
            for u in range(gu):
                g = c.add_locus(8 if u % 2 else 16)
                a_owns = u % 5 != 1
                own = species(0, 0) if a_owns else species(1, 0)
                other = species(1, 0) if a_owns else species(0, 0)
                whole(c, g, own, float(rng.uniform(0.9, 1.0)))
                if u % 7 == 3:
                    whole(c, g, other, float(rng.uniform(0.1, 0.45)))
                if many and not a_owns:
                    for k in range(1, 10):
                        whole(c, g, species(1, k), float(rng.uniform(0.9, 1.0)))
                if u % 2 == 1 and u + 1 < gu and len(c.loci) + (gu - u - 1) < 63:
                    whole(c, c.add_locus(8), species(0, 0), 0.25)
            assert len(c.loci) <= 63 and len(c.hits) <= 224
            out.append(c)
    return out


# ---------------------------------------------------------------------------
# the selection
# ---------------------------------------------------------------------------

def selection_cases():
    out = []
    # equal ranks (dyadic scores): the later pair is the best (report-best shows which)
    c = contig("sel_tie", (0, 2, 2, LGT))
    c.add_locus(8), c.add_locus(8)
    whole(c, 0, species(0, 0), 0.875)
    whole(c, 1, species(1, 0), 0.875), whole(c, 1, species(1, 1), 0.875)
    out.append(c)
    # A on locus 0 at 1; B1 = (1, 1, 1) on loci 1-3 is the best; the second sums 0.25 less
    # (rank exactly --range below), the third one thousandth more or less than that
    for tag, last, near in (("on", None, 2), ("outside", (0.875, 0.875, 1.0 - 4 * STEP), 2),
                            ("inside", (0.875, 0.875 + 4 * STEP, 1.0), 3)):
        rows = [(1.0, 1.0, 1.0), (0.875, 0.875, 1.0)] + ([last] if last else [])
        c = contig("sel_range_" + tag, (0, len(rows), near, LGT))
        for _ in range(4):
            c.add_locus(8)
        whole(c, 0, species(0, 0), 1.0)
        for j, row in enumerate(rows):
            for g, s in enumerate(row):
                whole(c, 1 + g, species(1, j), s)
        out.append(c)
    # one option within --range (reported as is) ...
    c = contig("sel_one_near", (0, 3, 1, LGT))
    c.add_locus(8), c.add_locus(8)
    whole(c, 0, species(0, 0), 0.875)
    for j, s in enumerate((1.0, 0.8125, 0.75)):
        whole(c, 1, species(1, j), s)
    out.append(c)
    # ... and three with unequal synteny: (A, B1) "ABB", (A2, B1) and (A2, B2) "AAB": no meld,
    # the contig rolls up (the genera: G0 on loci 0-1, G1 on loci 1-2, '*' on a third of the
    # length: rejected; the family explains it)
    c = contig("sel_unequal", (0, 3, 3, NO_LGT))
    for _ in range(3):
        c.add_locus(8)
    whole(c, 0, species(0, 0), 0.9375)
    whole(c, 0, species(0, 1), 0.9375), whole(c, 1, species(0, 1), 0.9375)
    whole(c, 1, species(1, 0), 0.9375), whole(c, 2, species(1, 0), 0.9375)
    whole(c, 2, species(1, 1), 0.9375)
    out.append(c)
    return out


# ---------------------------------------------------------------------------
# the synteny and the LGT checks
# ---------------------------------------------------------------------------

def fillers(c, a_loci, b_loci):
    """Nineteen more candidate pairs, none within --range of a best pair that scores
    >= 0.984375 on every locus: nine species of genus 2 on `a_loci` and one of genus 3 on `b_loci`, at 0.75 ..
    0.76 (with the case's clades A on a_loci and B on b_loci: (A, H), 9 (F, B), 9 (F, H))."""
    for k in range(9):
        for g in a_loci:
            whole(c, g, species(2, k), 0.75 + k / 1024.0)
    for g in b_loci:
        whole(c, g, species(3, 0), 0.75)


def check_cases(leaves=False):
    """name -> contig, each built with one candidate pair (`_x1`) and among twenty
    (`_x20`).  A = s__S0_00 and B = s__S1_00 unless stated.  `leaves`: the set runs with
    --clade-leaves 2, which rejects every pair of species (one leaf each)."""
    A, B = species(0, 0), species(1, 0)
    out = []

    def case(tag, loci, hits, a_loci, b_loci, call, level=0):
        for many in (False, True):
            pairs = 20 if many else 1
            c = contig("chk_{}_x{}".format(tag, pairs), (level, pairs, 1, call), case=tag)
            for n in loci:
                c.add_locus(n)
            for g, sp, s in hits:
                whole(c, g, sp, s)
            if many:
                fillers(c, a_loci, b_loci)
            out.append(c)

    # "ABA": the direction is known (B>A), the sister check looks at the 'B' loci alone
    case("aba", (8, 8, 8), [(0, A, 1.0), (1, B, 1.0), (2, A, 0.984375)], (0, 2), (1,), LGT)
    # the first clade's loci come second: swapped
    case("swap", (8, 8), [(0, B, 1.0), (1, A, 0.984375)], (1,), (0,), LGT)
    # '*' (both at or above k_amb = 0.5) on 8 of 80 sites: exactly --ambiguous-fraction 0.1 ...
    star = [(0, A, 1.0), (0, B, 0.5), (1, A, 1.0), (2, A, 1.0), (3, B, 1.0),
            (4, B, 1.0), (5, B, 1.0)]
    case("star", (8, 16, 16, 16, 16, 8), star, (0, 1, 2), (3, 4, 5), LGT)
    # ... and on 16 of 88: exceeded, the pair is rejected and the family explains the contig
    case("star_over", (16, 16, 16, 16, 16, 8), star, (0, 1, 2), (3, 4, 5), NO_LGT)
    # B one thousandth below k_amb there: 'A'
    near = [(g, sp, 0.5 - STEP if (g, sp) == (0, B) else s) for g, sp, s in star]
    case("star_below", (16, 16, 16, 16, 16, 8), near, (0, 1, 2), (3, 4, 5), LGT)
    # a sister of A (s__S0_01) at the sister threshold on B's locus: rejected; just below: not
    case("sis_at", (8, 8), [(0, A, 1.0), (1, B, 1.0), (1, species(0, 1), 0.5)], (0,), (1,), NO_LGT)
    case("sis_below", (8, 8), [(0, A, 1.0), (1, B, 1.0), (1, species(0, 1), 0.5 - STEP)], (0,), (1,), LGT)
    # ... and a sister of B on A's locus, which counts while the direction is unknown ("AB")
    # and not once it is known ("ABA": only the recipient's loci are checked)
    case("sis_b_at", (8, 8), [(0, A, 1.0), (1, B, 1.0), (0, species(1, 1), 0.5)], (0,), (1,), NO_LGT)
    case("sis_b_dir", (8, 8, 8), [(0, A, 1.0), (1, B, 1.0), (2, A, 1.0), (0, species(1, 1), 0.5)],
         (0, 2), (1,), LGT)
    # the pair are sisters themselves (s__S0_00, s__S0_01): each is left out of the other's
    # sisters; a third species of the genus at the threshold on the second's locus counts
    S = species(0, 1)
    case("sibs", (8, 8), [(0, A, 1.0), (1, S, 1.0)], (0,), (1,), LGT)
    case("sibs_third", (8, 8), [(0, A, 1.0), (1, S, 1.0), (1, species(0, 2), 0.5)], (0,), (1,), NO_LGT)
    # two sisters at the threshold on the pair's other locus, one of them the pair's own
    # clade: (saturating counts: "at least two" minus the pair's clade is still one)
    case("sibs_two", (8, 8, 8), [(0, A, 1.0), (1, S, 1.0), (2, A, 1.0), (1, A, 0.5 - STEP),
                                 (1, species(0, 2), 0.5), (1, species(0, 3), 0.5)], (0, 2), (1,), NO_LGT)
    # --clade-genes 2 (its own set): one locus each is rejected, two each is not
    case("genes_1", (8, 8, 8), [(0, A, 1.0), (1, A, 1.0), (2, B, 1.0)], (0, 1), (2,), LGT)
    case("genes_2", (8, 8, 8, 8), [(0, A, 1.0), (1, A, 1.0), (2, B, 1.0), (3, B, 1.0)],
         (0, 1), (2, 3), LGT)
    return out


def unknown_cases():
    """--weak-loci assign-unknown, -k1 0.75 -k2 0.5: Unknown scores 1 - the best known score,
    1.0 on the locus without a hit.  A (0.875, none, 0.5) with Unknown (0.125, 1.0, 0.5):
    on the last locus both reach k_amb, and a pair with Unknown gets no '*'.  `x10`: nine
    species at 0.5 on A's loci, each a candidate pair with Unknown, ranks 0.125 below."""
    out = []
    for many in (False, True):
        pairs = 10 if many else 1
        c = contig("unknown_x{}".format(pairs), (0, pairs, 1, LGT))
        for _ in range(3):
            c.add_locus(8)
        whole(c, 0, species(0, 0), 0.875), whole(c, 2, species(0, 0), 0.5)
        if many:
            for k in range(9):
                whole(c, 0, species(2, k), 0.5), whole(c, 2, species(2, k), 0.5)
        out.append(c)
    return out


def _level0():
    return grid_cases() + gu_cases() + selection_cases() + check_cases()


# A flag set's effect on a contig's `want` (level, pairs, near, call): the cases' own `want`
# holds under FLAGS; the sets below restate it where their flag changes the outcome.
def _rewant(contigs, fn):
    for c in contigs:
        c.meta["want"] = fn(c, c.meta["want"])
    return contigs


def _sister_off(c, w):
    # nothing is rejected for a sister; sel_unequal's genera then pass as well ('*' is within
    # the ambiguous fraction?  no: 8 of 24 sites) -- its call stands
    flips = ("chk_sis_at", "chk_sis_b_at", "chk_sibs_third", "chk_sibs_two")
    return (w[0], w[1], w[2], LGT) if c.name.startswith(flips) else w


def _genes2(c, w):
    # both clades need two loci: of the designed contigs only these qualify
    ok = c.name.startswith(("chk_genes_2", "chk_star_x", "chk_star_below"))
    ok = ok or (c.name.startswith("gu_") and c.meta["gu"] >= 7)
    return (w[0], w[1], w[2], LGT if ok else NO_LGT)


@functools.lru_cache(maxsize=None)
def case_sets():
    """name -> CaseSet."""
    off = ["--sister-penalty", "off"]
    sets = [
        CaseSet("two_l0", _level0(), FLAGS),
        CaseSet("two_l0_best", _level0(), FLAGS + ["--disambiguate-two", "report-best"]),
        CaseSet("two_l0_sister_off", _rewant(selection_cases() + check_cases(), _sister_off), FLAGS + off),
        CaseSet("two_l0_genes2", _rewant(gu_cases() + check_cases(), _genes2), FLAGS + ["--clade-genes", "2"]),
        CaseSet("two_unknown", unknown_cases(), FLAGS_UNK),
        WideCaseSet("two_l1", grid_l1_cases(False), FLAGS),
        WideCaseSet("two_l1_off", grid_l1_cases(True), FLAGS + off + ["--allow-lca"]),
    ]
    return {cs.key: cs for cs in sets}


# --clade-leaves 2 rejects every pair of species, so the checks' contigs roll up and their
# genera (70 leaves each) decide at level 1: listed apart, with its own expectations.
@functools.lru_cache(maxsize=None)
def leaves_set():
    return CaseSet("two_l0_leaves2", check_cases(), FLAGS + ["--clade-leaves", "2"])


# ---------------------------------------------------------------------------
# the oracle's explain_two calls
# ---------------------------------------------------------------------------

def traced_oracle(cs):
    """contig name -> [(roll-up level, candidate pairs, pairs within --range of the best,
    whether the call returned an accepted explanation)] of the oracle's two_clade calls, and
    the oracle's Results."""
    from oracle import orgscorer_oracle as orc
    calls, level = {}, {}
    one0, two0 = orc.one_clade, orc.two_clade

    def one(C, tax):
        level[C.name] = level.get(C.name, -1) + 1
        return one0(C, tax)

    def two(C, tax):
        pool = [c for c in orc._ordered(C.clades) if max(C.genes[c]) >= C.p.k2]
        ranks = [r for r in (C.evaluate(a, b) for a in pool for b in pool if a < b) if r[0] >= C.p.k2]
        ranks = [r[1] for r in ranks]
        near = sum(1 for r in ranks if max(ranks) - r <= C.p.range)
        res = two0(C, tax)
        calls.setdefault(C.name, []).append((level[C.name], len(ranks), near, orc._ok(res)))
        return res

    orc.one_clade, orc.two_clade = one, two
    saved = mc._ORACLE.pop(cs.key, None)
    try:
        res = ec.oracle_for(cs)
    finally:
        orc.one_clade, orc.two_clade = one0, two0
        if saved is not None:
            mc._ORACLE[cs.key] = saved
    return calls, res
