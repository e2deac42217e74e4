"""In-memory cases for the junction kernels (k_jn_cover / k_jn_eval, wf_junctions.hip).

A case is one wf_junctions call: contig lengths, loci (start, end, strand) in GFF order and
concordant pairs (contig, mate-1 start/end, mate-2 start/end), plus --min-overlap-sites.
table() / pair_arrays() give the product's in-memory inputs; write_text() renders the same
case as FASTA, GFF and SAM for the judge, oracle.junctions_oracle (accumulate,
junction_rows, detailed_rows, unmodified; judge() runs them once per case and process).

Families:
  C  coverage edges: a pair ending on the last site, running past it, lying wholly past it,
     a mate at POS 0 (L = -1: Python's slice wraps), a whole-contig pair, contigs without
     pairs, a contig of length 0, 100 000 identical pairs, and 3000 contigs of lengths
     0..2999 (every sentinel slot at another offset of the device scan).
  L  locus geometry: 0/1/2 loci, a locus past the contig end, start 0, overlapping, touching,
     nested, equal starts, a repeated code, equal coordinates on both strands; and, in a
     call of its own, a locus with start > end (the kernel's early exit is off for the call).
  H  hit logic: overlap of exactly --min-overlap-sites and one less, a pair hitting loci j
     and j+2 only, mates hitting different loci, pairs left and right of all loci; at 25, 0, -3.
  W  wide hit sets: 64..300 loci at --min-overlap-sites 0, and at 25 two mates (one with an
     N-skip CIGAR) hitting small overlapping loci 70 positions apart.

The reference fixture set `edges` (tests/golden/make_junctions.py) is edges_case(): families
C, L, H and W's geometry in one file set (contigs of 65, 70 and 100 loci for W).  The
reference ran it without raising, the contig of length 0, the locus with start 0 and the
mate at POS 0 included, so none of those inputs is left out.  The locus with start > end is
not part of the set: it would switch the kernel's early exit off for the whole call, which
the set is meant to run; it stays in the oracle-judged case L_reversed.
"""
import functools
import os
import random
import tempfile
import warnings

import numpy as np

from oracle import junctions_oracle as jo
from waafle_amd import junctions


class JCase:
    """contigs: [(name, length, [(start, end, strand)])]; pairs: [(contig index, s1, e1, s2,
    e2)] or with two trailing CIGAR strings; expect: answers known by construction."""

    def __init__(self, name, contigs, pairs, min_sites=25, expect=None):
        self.name, self.contigs, self.min_sites = name, contigs, min_sites
        self.pairs = [tuple(p) + (None, None) if len(p) == 5 else tuple(p) for p in pairs]
        self.expect = expect or {}

    def __repr__(self):
        return self.name

    def names(self):
        return [c[0] for c in self.contigs]

    def gff_rows(self):
        return [[n, "case", "gene", str(a), str(b), ".", s, "0", "."]
                for n, _, loci in self.contigs for a, b, s in loci]

    def table(self):
        by = {}
        for row in self.gff_rows():
            by.setdefault(row[0], []).append(junctions.GffLocus(row))
        return junctions.JunctionTable(self.names(), [c[1] for c in self.contigs], by)

    def pair_arrays(self):
        col = lambda i: np.array([p[i] for p in self.pairs], dtype=np.int64)
        return (np.array([p[0] for p in self.pairs], dtype=np.int32), col(1), col(2), col(3),
                col(4), [])

    def write_text(self, d, base="case"):
        """(fna, gff, sam) paths of the case as text files."""
        fna, gff, sam = [os.path.join(str(d), base + e) for e in (".fna", ".gff", ".sam")]
        with open(fna, "w") as fh:
            for n, length, _ in self.contigs:
                fh.write(">{}\n".format(n) + ("A" * length + "\n" if length else ""))
        with open(gff, "w") as fh:
            fh.write("##gff-version 3\n")
            for row in self.gff_rows():
                fh.write("\t".join(row) + "\n")
        names = self.names()
        with open(sam, "w") as fh:
            fh.write("@HD\tVN:1.0\tSO:unsorted\n")
            for i, (c, s1, e1, s2, e2, g1, g2) in enumerate(self.pairs):
                for flag, s, e, cig in ((99, s1, e1, g1), (147, s2, e2, g2)):
                    cig = cig or "{}M".format(e - s + 1)
                    assert jo.cigar_length(cig) == e - s + 1
                    fh.write("\t".join(["r{}".format(i), str(flag), names[c], str(s), "42", cig,
                                        "=", "0", "0", "*", "*"]) + "\n")
        return fna, gff, sam


class Judged:
    """The oracle's answers for a case, in the table's layout."""


@functools.lru_cache(maxsize=None)
def judge(name):
    case = by_name()[name]
    table = case.table()
    res = Judged()
    with tempfile.TemporaryDirectory() as d:
        fna, gff, sam = case.write_text(d)
        _, coverage, _, hits = jo.accumulate(fna, gff, sam, case.min_sites)
        res.junction_rows = jo.junction_rows(fna, gff, sam, case.min_sites)
        with warnings.catch_warnings():              # np.mean / np.std of a contig of length 0
            warnings.simplefilter("ignore", RuntimeWarning)
            res.site_rows, res.gene_rows = jo.detailed_rows(fna, gff, sam, case.min_sites)
    names = case.names()
    res.coverage = np.concatenate([coverage[n] for n in names] + [np.zeros(0)]).astype(np.int64)
    res.by_contig = {n: coverage[n].astype(np.int64) for n in names}
    NL = len(table.loci)
    res.floats = np.full((4, NL), np.nan)
    res.is_junction = np.zeros(NL, bool)
    res.junction_hits = np.zeros(NL, np.int64)
    res.locus_hits = np.array([hits.get(names[c], {}).get((l.code, l.code), 0)
                               for c in range(len(names))
                               for l in table.loci[table.loc_off[c]:table.loc_off[c + 1]]] + [],
                              dtype=np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for c, n in enumerate(names):
                cov = coverage[n]
                for j in range(int(table.loc_off[c]), int(table.loc_off[c + 1]) - 1):
                    L1, L2 = table.loci[j], table.loci[j + 1]
                    gap = L2.start - L1.end - 1                     # evaluate_contig :292-316
                    c1 = np.mean(cov[L1.start - 1:L1.end])
                    c2 = np.mean(cov[L2.start - 1:L2.end])
                    cj = 0.0 if gap <= 0 else np.mean(cov[L1.end - 1:L2.start])
                    res.floats[:, j] = (c1, c2, cj, cj / (np.mean([c1, c2]) + 1e-6))
                    res.is_junction[j] = True
                    res.junction_hits[j] = hits.get(n, {}).get((L1.code, L2.code), 0)
    return res


# ---------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------

TWO = [(21, 120, "+"), (181, 280, "-")]


def coverage_contigs(prefix=""):
    """Family C's contigs and pairs (the contended and the scan cases are separate)."""
    contigs = [(prefix + n, 300, list(TWO)) for n in
               ("c0_end_exact", "c1_past_end", "c2_wholly_past", "c3_pos0", "c4_whole", "c5_nopairs")]
    contigs.append((prefix + "c6_empty", 0, []))
    contigs.append((prefix + "c7_nopairs_noloci", 50, []))
    pairs = [(0, 251, 280, 281, 300),
             (1, 250, 290, 280, 340),
             (2, 301, 330, 350, 400), (2, 30, 100, 150, 230),
             (3, 0, 29, 270, 300), (3, 0, 29, 100, 150), (3, 40, 90, 0, 9),
             (4, 1, 150, 151, 300),
             (6, 1, 10, 5, 20)]
    cov = {"c0_end_exact": [(250, 300, 1)], "c1_past_end": [(249, 300, 1)],
           "c2_wholly_past": [(29, 230, 1)], "c3_pos0": [(299, 300, 1)],
           "c4_whole": [(0, 300, 1)], "c5_nopairs": [], "c6_empty": [], "c7_nopairs_noloci": []}
    return contigs, pairs, {prefix + k: v for k, v in cov.items()}


def family_c():
    contigs, pairs, cov = coverage_contigs()
    cases = [JCase("C_coverage", contigs, pairs, expect=dict(
        cov=cov, junction_hits={("c2_wholly_past", 0): 1, ("c4_whole", 0): 1}))]
    cases.append(JCase("C_contended", [("hot", 200, [(41, 110, "+"), (131, 190, "-")]),
                                       ("cold", 200, [(41, 110, "+"), (131, 190, "-")])],
                       [(0, 50, 99, 120, 180)] * 100000,
                       expect=dict(cov={"hot": [(49, 180, 100000)], "cold": []},
                                   junction_hits={("hot", 0): 100000, ("cold", 0): 0})))
    # lengths 0..2999: one or two pairs and up to two loci per contig
    contigs, pairs, cov = [], [], {}
    for n in range(3000):
        name = "s{:04d}".format(n)
        loci = [(n // 8 + 1, n // 4, "+"), (n // 2, n - 2, "-")] if n >= 40 else []
        contigs.append((name, n, loci))
        cov[name] = []
        if n >= 10:
            a, b = (n * 7) % (n // 2) + 1, n - (n % 5)           # 1 <= a <= n/2 < b <= n
            over = 30 if n % 3 == 0 else 0                        # every third runs past the end
            mid = (a + b) // 2
            pairs.append((n, a, mid, mid + 1, b + over))
            cov[name] = [(a - 1, min(b + over, n), 1)]
    cases.append(JCase("C_scan_3000", contigs, pairs, expect=dict(cov=cov)))
    return cases


def random_pairs(c, length, k, rng):
    out = []
    for _ in range(k):
        a = rng.randint(1, length)
        l1, l2, ins = rng.randint(30, 100), rng.randint(30, 100), rng.randint(-20, 150)
        b = a + l1 + ins
        out.append((c, a, a + l1 - 1, b, b + l2 - 1))
    return out


def geometry_contigs(prefix=""):
    spec = [("l00_no_loci", []),
            ("l01_one_locus", [(100, 200, "+")]),
            ("l02_two_loci", [(100, 200, "+"), (260, 380, "-")]),
            ("l03_past_end", [(100, 200, "+"), (350, 450, "-")]),
            ("l04_start_zero", [(0, 80, "+"), (150, 250, "-")]),
            ("l05_overlapping", [(100, 200, "+"), (150, 250, "-")]),
            ("l06_touching", [(100, 200, "+"), (201, 300, "-")]),
            ("l07_gap_one", [(100, 200, "+"), (202, 300, "-")]),
            ("l08_nested", [(50, 350, "+"), (100, 150, "-"), (200, 220, "+")]),
            ("l09_equal_starts", [(100, 200, "+"), (100, 300, "-"), (100, 150, "+"), (90, 95, "-")]),
            ("l10_same_code_twice", [(100, 200, "+"), (250, 330, "-"), (100, 200, "+")]),
            ("l11_both_strands", [(100, 200, "+"), (100, 200, "-"), (300, 360, "+")]),
            ("l12_unsorted_gff", [(300, 380, "+"), (20, 90, "-"), (150, 260, "+")])]
    return [(prefix + n, 400, loci) for n, loci in spec]


def family_l():
    rng = random.Random(12)
    contigs = geometry_contigs()
    pairs = [p for c in range(len(contigs)) for p in random_pairs(c, 400, 14, rng)]
    cases = [JCase("L_geometry", contigs, pairs, expect=dict(
        nan=[("l04_start_zero", 0, 0)],                    # cov[-1:80] is empty on 400 sites
        zero_junction=[("l05_overlapping", 0), ("l06_touching", 0), ("l08_nested", 0),
                       ("l09_equal_starts", 1), ("l10_same_code_twice", 0)]))]
    rev = [("r0_reversed", 400, [(50, 120, "+"), (260, 200, "-"), (300, 380, "+")]),
           ("r1_forward", 400, [(100, 200, "+"), (260, 380, "-")]),
           ("r2_only_reversed", 400, [(300, 100, "-"), (350, 340, "+")])]
    rp = [p for c in range(3) for p in random_pairs(c, 400, 14, rng)]
    rp += [(1, 1, 40, 50, 90), (0, 210, 250, 390, 400), (2, 1, 60, 70, 99)]
    cases.append(JCase("L_reversed", rev, rp, expect=dict(
        nan=[("r0_reversed", 0, 1), ("r0_reversed", 0, 3), ("r0_reversed", 1, 0),
             ("r2_only_reversed", 0, 0), ("r2_only_reversed", 0, 1)])))
    return cases


def hit_contigs(prefix=""):
    abc = [(100, 199, "+"), (300, 399, "-"), (500, 599, "+")]
    contigs = [(prefix + "h0_exact", 700, abc), (prefix + "h1_one_less", 700, abc),
               (prefix + "h2_skip_middle", 700, abc), (prefix + "h3_two_mates", 700, abc),
               (prefix + "h4_left_right", 700, [(300, 399, "+"), (450, 549, "-")])]
    pairs = [(0, 175, 260, 650, 700), (0, 640, 690, 236, 324),        # 25 sites of A; of B
             (1, 176, 260, 650, 700), (1, 640, 690, 236, 323),        # 24
             (2, 100, 199, 500, 599), (2, 480, 560, 90, 160),
             (3, 120, 180, 320, 380), (3, 520, 580, 330, 390), (3, 150, 350, 360, 420),
             (4, 1, 50, 60, 120), (4, 600, 650, 660, 700), (4, 310, 380, 460, 530)]
    return contigs, pairs


def family_h():
    contigs, pairs = hit_contigs()
    at25 = dict(junction_hits={("h0_exact", 0): 0, ("h1_one_less", 0): 0, ("h2_skip_middle", 0): 0,
                               ("h2_skip_middle", 1): 0, ("h3_two_mates", 0): 2,
                               ("h3_two_mates", 1): 1, ("h4_left_right", 0): 1},
                locus_hits={("h0_exact", 0): 1, ("h0_exact", 1): 1, ("h1_one_less", 0): 0,
                            ("h1_one_less", 1): 0, ("h2_skip_middle", 0): 2,
                            ("h2_skip_middle", 1): 0, ("h2_skip_middle", 2): 2})
    every = dict(junction_hits={("h0_exact", 0): 2, ("h2_skip_middle", 1): 2,
                                ("h3_two_mates", 0): 3, ("h4_left_right", 0): 3},
                 locus_hits={("h1_one_less", 2): 2, ("h4_left_right", 1): 3})
    return [JCase("H_hits_25", contigs, pairs, 25, at25), JCase("H_hits_0", contigs, pairs, 0, every),
            JCase("H_hits_m3", contigs, pairs, -3, every)]


WIDE = [64, 65, 66, 130, 300]


def wide_contigs(sizes=WIDE, prefix=""):
    contigs, pairs = [], []
    for c, n in enumerate(sizes):
        loci = [(11 + 10 * i, 18 + 10 * i, "+-"[i % 2]) for i in range(n)]
        contigs.append(("{}w{:03d}_loci".format(prefix, n), 10 * n + 40, loci))
        pairs += [(c, 1, 8, 5 * n, 5 * n + 30), (c, 10 * n, 10 * n + 20, 10 * n - 60, 10 * n - 10),
                  (c, 3, 9, 2, 6)]
    return contigs, pairs


def nskip_contig(prefix=""):
    """100 loci of 30 sites, 5 apart; mates that hit loci 0-3 and 73-74 only, and one mate
    whose N-skip spans loci 0-86."""
    loci = [(1 + 5 * i, 30 + 5 * i, "+-"[i % 2]) for i in range(100)]
    pairs = [(0, 1, 40, 370, 399, "40M", "10M10N10M"),
             (0, 1, 460, 500, 540, "30M400N30M", "41M"),
             (0, 380, 420, 425, 470),                                  # first hit at locus 71
             (0, 330, 385, 5, 34, "20M16N20M", "30M")]
    return (prefix + "n100_nskip", 600, loci), pairs


def family_w():
    contigs, pairs = wide_contigs()
    want = {(c[0], j): 3 for c in contigs for j in range(len(c[2]) - 1)}
    cases = [JCase("W_wide_0", contigs, pairs, 0, dict(junction_hits=want))]
    contig, pairs = nskip_contig()
    cases.append(JCase("W_nskip_25", [contig], pairs, 25, dict(
        locus_hits={("n100_nskip", 0): 3, ("n100_nskip", 3): 2, ("n100_nskip", 40): 1,
                    ("n100_nskip", 72): 2, ("n100_nskip", 74): 2, ("n100_nskip", 99): 1})))
    return cases


def edges_case():
    """The `edges` set of the reference fixtures: every family's geometry in one call."""
    rng = random.Random(99)
    contigs, pairs = [], []

    def add(cs, ps):
        base = len(contigs)
        contigs.extend(cs)
        pairs.extend((p[0] + base,) + tuple(p[1:]) for p in ps)

    cs, ps, _ = coverage_contigs("e_")
    add(cs, ps)
    cs = geometry_contigs("e_")
    add(cs, [p for c in range(len(cs)) for p in random_pairs(c, 400, 6, rng)])
    add(*hit_contigs("e_"))
    add(*wide_contigs([65, 70], "e_"))
    c, ps = nskip_contig("e_")
    add([c], ps)
    return JCase("edges", contigs, pairs, 25)


@functools.lru_cache(maxsize=None)
def all_cases():
    return tuple(family_c() + family_l() + family_h() + family_w())


@functools.lru_cache(maxsize=None)
def by_name():
    d = {c.name: c for c in all_cases()}
    d["edges"] = edges_case()
    d["edges_0"] = JCase("edges_0", d["edges"].contigs, d["edges"].pairs, 0)
    return d
