"""Contigs for the first wave form's envelope-integral bounds and its explain_one from
intervals (wf_fast.hip), built on mean_cases' in-memory batches: 1-4 loci (one contig of
64), 2-70 hits (the > 64-option contigs: three hits per option), dyadic scores so that a
multi-run segment's numpy mean is *exactly* a threshold, and the same segment one
thousandth above and below it.  The oracle gives every expected value.

The bounds and the interval walk are compiled into the roll-up launches only, so every
decision that tests them is built twice: at the species level (level 0, `*_cases`), and
among genera (`*_l1_cases`), where the split segment's halves belong to two sister species.
There no species is an option (its half gives it a mean < k1 on that locus) and no pair of
species explains the contig, so the contig rolls up and the merged multi-run segment, the
ranks and the ties decide at level 1.  A hit of another genus at 0.5625 keeps the split
locus unmasked at level 0 (kmin = 0.5) without being an option or a potential clade.

Thresholds (all dyadic): set ONE  -k1 0.5  -k2 0.75 (kmin = k1 = 0.5), --range 0.125;
                         set KMIN -k1 0.75 -k2 0.5  (kmin = k2 = 0.5 < k1).
A "split" segment is one species with two hits over [0, 4) and [4, 8) of an 8-site locus:
scores a, b give the mean (a + b) / 2 exactly (8 sites, one numpy leaf: sums of dyadics).
"""
import functools

import mean_cases as mc
from mean_cases import CaseSet, Contig, species
from waafle_amd.taxonomy import TaxonomyTables

FLAGS_ONE = ["-k1", "0.5", "-k2", "0.75", "--range", "0.125", "--min-gene-length", "1"]
FLAGS_KMIN = ["-k1", "0.75", "-k2", "0.5", "--range", "0.125", "--min-gene-length", "1"]
STEP = 0.001                                       # one pident thousandth


def split(c, g, sp, a, b, n=8):
    """Two hits of one species: [0, n/2) at a and [n/2, n) at b -- a multi-run segment."""
    c.add_run(g, 0, n // 2, sp, a)
    c.add_run(g, n // 2, n, sp, b)


def sisters(c, g, genus, a, b, n=8, sp=species, first=0):
    """The split segment as two sister species of `genus`: a multi-run segment only once
    they merge at level 1."""
    c.add_run(g, 0, n // 2, sp(genus, first), a)
    c.add_run(g, n // 2, n, sp(genus, first + 1), b)


def at_threshold(tag, lo, hi, build):
    """The contig with the split segment's mean exactly at the threshold, and one
    thousandth below and above it."""
    out = []
    for name, d in (("at", 0.0), ("below", -STEP), ("above", STEP)):
        c = Contig("{}_{}".format(tag, name), dict(family="env", case=tag, side=name), None, union=False)
        build(c, lo + d, hi)
        out.append(c)
    return out


def k2_cases():
    """explain_two's potential-clade test: A (genus 0) holds locus 0 alone, B (genus 1) holds
    locus 1 with a split segment of mean exactly k2 = 0.75: the pair (A, B) exists iff B's
    mean reaches k2."""
    def build(c, a, b):
        c.add_locus(8), c.add_locus(8)
        c.add_run(0, 0, 8, species(0, 0), 0.875)
        split(c, 1, species(1, 0), a, b)
    return at_threshold("k2", 0.5, 1.0, build)


def k2_l1_cases():
    """The same among genera: genus 0 holds locus 0 alone, genus 1's two species merge on
    locus 1 into a segment of mean exactly k2: the pair (G0, G1) exists at level 1 iff the
    merged mean reaches k2; below it the family explains the contig at level 2."""
    def build(c, a, b):
        c.add_locus(8), c.add_locus(8)
        c.add_run(0, 0, 8, species(0, 0), 0.875)
        sisters(c, 1, 1, a, b)
    return at_threshold("k2_l1", 0.5, 1.0, build)


def k1_cases():
    """explain_one's crit test: A holds locus 0 whole and locus 1 with a split segment of mean
    exactly k1 = 0.5: A is an option iff that mean reaches k1 (another genus keeps the locus
    unmasked, so the comparison is crit's and not the mask's)."""
    def build(c, a, b):
        c.add_locus(8), c.add_locus(8)
        c.add_run(0, 0, 8, species(0, 0), 0.875)
        split(c, 1, species(0, 0), a, b)
        c.add_run(1, 0, 8, species(2, 3), 0.5625)  # keeps locus 1 unmasked (>= kmin) either way
    return at_threshold("k1", 0.25, 0.75, build)


def k1_l1_cases():
    """The same among genera: genus 0 has locus 0 whole and, merged from two species, a
    segment of mean exactly k1 on locus 1: it is the option at level 1 iff that mean
    reaches k1; below it the family is, at level 2."""
    def build(c, a, b):
        c.add_locus(8), c.add_locus(8)
        c.add_run(0, 0, 8, species(0, 0), 0.875)
        sisters(c, 1, 0, a, b)
        c.add_run(1, 0, 8, species(2, 3), 0.5625)  # keeps locus 1 unmasked at every level
    return at_threshold("k1_l1", 0.25, 0.75, build)


def kmin_cases():
    """The weak-locus mask (set KMIN, kmin = 0.5 < k1 = 0.75): locus 1's only known segment is
    a split one of mean exactly kmin: at or above it the locus is unmasked and A (0.5 < k1
    there) explains nothing alone; below it the locus is masked and A explains the rest."""
    def build(c, a, b):
        c.add_locus(8), c.add_locus(8), c.add_locus(16)
        c.add_run(0, 0, 8, species(0, 0), 0.875)
        split(c, 1, species(0, 0), a, b)
        c.add_run(2, 0, 16, species(0, 0), 0.9375)
        split(c, 2, species(0, 1), 0.875, 0.8125, n=16)
    return at_threshold("kmin", 0.25, 0.75, build)


def sibling_case():
    """Two sister species with half a locus each: no option at level 0, and at level 1 their
    hits merge into one multi-run segment that makes the genus the only option."""
    c = Contig("siblings", dict(family="env", case="siblings"), "g__G0", 2, union=False)
    c.add_locus(8), c.add_locus(8)
    c.add_run(0, 0, 8, species(0, 0), 0.875)
    c.add_run(1, 0, 4, species(0, 0), 0.875)
    c.add_run(1, 4, 8, species(0, 1), 0.9375)
    c.add_run(1, 0, 8, species(3, 0), 0.5625)      # another genus keeps locus 1 unmasked
    return [c]


FOUR_RANKS = dict(tie=(0.875, 0.875, 0.875, 0.875),
                  range=(0.75, 0.875, 0.75 + 2 * STEP, 0.75 - 2 * STEP),
                  range_top_last=(0.75 - 2 * STEP, 0.75, 0.75 + 2 * STEP, 0.875))


def four_clade_cases():
    """Four clades on both loci, each with a split segment on locus 1.  Ranks: all equal (the
    tie goes by clade id); the best and others exactly --range (0.125) below it, one
    thousandth inside and one thousandth outside."""
    out = []
    for tag, ranks in FOUR_RANKS.items():
        c = Contig("four_" + tag, dict(family="env", case="four", kind=tag), None, union=False)
        c.add_locus(8), c.add_locus(8)
        for i, r in enumerate(ranks):
            sp = species(i, 2 * i)
            c.add_run(0, 0, 8, sp, r)              # rank = (r + r) / 2 = r, exactly for dyadic r
            split(c, 1, sp, r, r)
        out.append(c)
    return out


def four_genus_cases():
    """The same ranks among four genera: each has locus 0 whole by one species and locus 1
    as a segment merged from that species and its sister, so the ties and the --range edges
    are decided at level 1, from ranks whose bounds overlap or touch."""
    out = []
    for tag, ranks in FOUR_RANKS.items():
        c = Contig("four_l1_" + tag, dict(family="env", case="four_l1", kind=tag), None, union=False)
        c.add_locus(8), c.add_locus(8)
        for i, r in enumerate(ranks):
            c.add_run(0, 0, 8, species(i, 2 * i), r)
            sisters(c, 1, i, r, r, first=2 * i)
        c.add_run(1, 0, 8, species(4, 0), 0.5625)  # keeps locus 1 unmasked at level 0
        out.append(c)
    return out


def many_option_cases():
    """66 and 70 clades that each explain the contig (a whole hit on locus 0, a split segment
    on locus 1), a third of them within --range of the best."""
    out = []
    for k in (66, 70):
        c = Contig("many_{}".format(k), dict(family="env", case="many", k=k), None, union=False)
        c.add_locus(8), c.add_locus(8)
        for i in range(k):
            sp = species(i % mc.N_GENERA, i // mc.N_GENERA)
            r = 0.5625 + ((i * 37) % 97) / 256.0
            c.add_run(0, 0, 8, sp, r)
            split(c, 1, sp, r, r - 0.03125)
        out.append(c)
    return out


# More than 64 options at a roll-up level need more than 64 genera: a taxonomy of its own,
# 72 genera of two species under one family.
WIDE_GENERA = 72
WIDE_EDGES = [("f__F", "r__Root")]
for _g in range(WIDE_GENERA):
    WIDE_EDGES.append(("g__W{:02d}".format(_g), "f__F"))
    for _k in range(2):
        WIDE_EDGES.append(("s__W{:02d}_{}".format(_g, _k), "g__W{:02d}".format(_g)))
WIDE_TAX = TaxonomyTables(WIDE_EDGES)


def wide_species(g, k):
    return "s__W{:02d}_{}".format(g, k)


def many_genus_cases():
    """66 and 70 genera that each explain the contig at level 1 only (locus 0 whole by one
    species, locus 1 merged from that species and its sister), a third of them within --range
    of the best: the interval walk drops most of them before explain_one lists the rest."""
    out = []
    for k in (66, 70):
        c = Contig("many_l1_{}".format(k), dict(family="env", case="many_l1", k=k), None, union=False)
        c.add_locus(8), c.add_locus(8)
        for i in range(k):
            r = 0.5625 + ((i * 37) % 97) / 256.0
            c.add_run(0, 0, 8, wide_species(i, 0), r)
            sisters(c, 1, i, r, r - 0.03125, sp=wide_species)
        c.add_run(1, 0, 8, wide_species(WIDE_GENERA - 1, 0), 0.5625)   # locus 1 unmasked at level 0
        out.append(c)
    return out


class WideCaseSet(CaseSet):
    """A case set over WIDE_TAX (mean_cases builds its batches over its module's taxonomy)."""
    edges = WIDE_EDGES

    def __init__(self, key, contigs, flags):
        saved = mc.TAX
        mc.TAX = WIDE_TAX
        try:
            CaseSet.__init__(self, key, contigs, flags)
        finally:
            mc.TAX = saved
        self.tax = WIDE_TAX


def oracle_for(cs):
    """mean_cases.oracle_for, over the case set's own taxonomy where it has one."""
    edges = getattr(cs, "edges", None)
    if edges is None:
        return mc.oracle_for(cs)
    saved = mc.EDGES
    mc.EDGES = edges
    try:
        return mc.oracle_for(cs)
    finally:
        mc.EDGES = saved


def loose_path_case():
    """One segment of 65 attachments (past kPruneMax: the loose bounds) next to a split
    competitor, on one locus."""
    c = Contig("loose65", dict(family="env", case="loose"), None, union=False)
    c.add_locus(200)
    for i in range(65):
        c.add_run(0, 3 * i, 3 * i + 5, species(0, 0), 0.5 + (i % 16) / 32.0)
    split(c, 0, species(1, 1), 0.75, 0.6875, n=200)
    return [c]


def locus_count_cases():
    """G = 1 (two species, split segments) and G = 64 (one species on every locus, split
    segments on three of them, a second species on six)."""
    one = Contig("G1", dict(family="env", case="G", G=1), None, union=False)
    one.add_locus(8)
    split(one, 0, species(0, 0), 0.75, 0.875)
    split(one, 0, species(0, 1), 0.875, 0.625)
    many = Contig("G64", dict(family="env", case="G", G=64), None, union=False)
    for g in range(64):
        many.add_locus(8)
        if g in (5, 33, 63):
            split(many, g, species(0, 0), 0.875, 0.75)
        else:
            many.add_run(g, 0, 8, species(0, 0), 0.875)
    for g in (0, 5, 63):
        many.add_run(g, 0, 8, species(1, 0), 0.9375)
    assert len(many.hits) == 70
    return [one, many]


def root_case():
    """Set KMIN: two species of two genera at 0.5625 .. 0.625 on both loci (split segments):
    every locus unmasked (>= kmin 0.5), no option at any level (k1 0.75), two potential
    clades whose pair the LGT checks reject at the species and the genus level (pair_evals 2,
    ppot_sum 4): unclassified at r__Root after four iterations."""
    c = Contig("to_root", dict(family="env", case="root"), None, 4, union=False)
    c.add_locus(8), c.add_locus(8)
    split(c, 0, species(0, 0), 0.5, 0.75)
    split(c, 1, species(0, 0), 0.75, 0.5)
    split(c, 0, species(1, 0), 0.5625, 0.5625)
    split(c, 1, species(1, 0), 0.5, 0.625)
    return [c]


def _one():
    return (k2_cases() + k2_l1_cases() + k1_cases() + k1_l1_cases() + sibling_case() +
            four_clade_cases() + four_genus_cases() + many_option_cases() + loose_path_case() +
            locus_count_cases())


def _kmin():
    return kmin_cases() + root_case()


@functools.lru_cache(maxsize=None)
def case_sets():
    """name -> CaseSet: the two threshold sets, and set ONE under the flags that keep the
    bound-derived unmasking off (penalize, assign-unknown) or change what attaches."""
    sets = [CaseSet("env_one", _one(), FLAGS_ONE), CaseSet("env_kmin", _kmin(), FLAGS_KMIN),
            WideCaseSet("env_wide", many_genus_cases(), FLAGS_ONE)]
    for tag, extra in (("penalize", ["--weak-loci", "penalize"]),
                       ("unknown", ["--weak-loci", "assign-unknown"]),
                       ("overlap0", ["--min-overlap", "0"])):
        sets.append(CaseSet("env_one_" + tag, _one(), FLAGS_ONE + extra))
        sets.append(WideCaseSet("env_wide_" + tag, many_genus_cases(), FLAGS_ONE + extra))
        sets.append(CaseSet("env_kmin_" + tag, _kmin(), FLAGS_KMIN + extra))
    return {cs.key: cs for cs in sets}
