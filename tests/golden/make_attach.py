"""Hit-to-locus attachment fixtures (build container only).

`attach_hits` / `score_hit` (waafle_orgscorer.py:359-392) filter the hits, attach them to
loci, paint each hit's site range and transfer annotations.  Every contig here is the
smallest shape that reaches one edge of that rule or one size at which the HIP kernels change
path.  Four input sets under attach_inputs/, committed gzipped (the counts below need some
6,000 rows; this script is their readable form, golden_cases.materialize unpacks them):

  attach      one annotation system: the triage's packed-key form, every wave slice, the
              counting kernel and the staged attach kernel
  attach7     seven systems (more than the packed key holds): the same annotation families
  attachhbm   one system, contigs of 256 and 257 loci     } more (locus, system) slots than the
  attachhbm7  seven systems, contigs of 36 and 37 loci    } staged kernel keeps on chip

The last two are sets of their own because one such contig sends its whole batch to the
staged kernels; inside `attach` it would keep every other contig off the wave kernels.

Contig families (loci are 200-300 sites: --min-gene-length stays at its default):
  b_*        hit/locus boundaries: the hit's last site on the locus's first and the reverse,
             each moved one site away, a hit containing a locus and one inside it, a hit over
             3 loci, over 26 and over 27 loci
  ovl_*      overlap fraction ov/den exactly 1/10 and 1/2 (den = 50 sites), one site more, one less
  lay_*      loci adjacent, sharing one site (start = prev_end), sharing two, nested, a GFF in
             descending order with one locus written end-first
  loci<n>    1, 63, 64, 65, 128, 129 loci (65 is also the first past 64 annotation slots)
  hits<n>    64, 65, 256, 257, 512, 513 hits
  att<n>     225, 257 (hits257) and 514 attachments: one past each wave slice
  strands    hit +/- against locus +/-/.
  scov_*     subject coverage 0.9, 0.899, 0.901
  ann        two hits at one best score on a locus (the later wins), a higher-scoring hit
             without annotation, a score at the annotation threshold and one just below

Scores: every hit gets its own percent identity, so all scores of a set are distinct, and
none is dyadic -- sums of site scores then do not collide and no rank ties.  Two exceptions,
both deliberate and both in `ann`: the pair sharing one score, and the hit at the annotation
threshold, which is min(k1, k2) = 0.5.  main() asserts both properties and `ties == []`.

Each case is run by make_golden.make_case (reference under two hash seeds and sorted clade
order).  Run:  python tests/golden/make_attach.py
"""
import gzip
import json
import os
import sys
from fractions import Fraction

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

INPUTS = os.path.join(HERE, "attach_inputs")
TAXONOMY = [("f__F", "r__Root"), ("g__A", "f__F"), ("g__B", "f__F")] + \
           [("s__{}{}".format(g, i), "g__" + g) for g in "AB" for i in (1, 2, 3)]
SPECIES = [c for c, _ in TAXONOMY[3:]]
FLAG_SETS = [[], ["--min-overlap", "0"], ["--min-overlap", "0.5"], ["--stranded"],
             ["--min-scov", "0.9"], ["--jump-taxonomy", "1"]]
SETS = {"attach": (1, FLAG_SETS), "attach7": (7, FLAG_SETS[:2]),
        "attachhbm": (1, FLAG_SETS[:2]), "attachhbm7": (7, FLAG_SETS[:2])}
TIE_PIDENT = 91111        # the two `ann` hits sharing one score (thousandths of a percent)
AT_THRESHOLD = 50000      # score 0.5 = the lenient annotation threshold


class Hit:
    def __init__(self, taxon, qs, qe, base, strand="plus", annot=True, slen=None, pident=None):
        self.taxon, self.qs, self.qe, self.base, self.strand = taxon, qs, qe, base, strand
        self.annot, self.slen, self.pident = annot, slen or qe - qs + 1, pident


class InputSet:
    def __init__(self, stem, n_sys):
        self.stem, self.n_sys = stem, n_sys
        self.contigs = {}               # name -> (loci [(start, end, strand)], hits)
        self.used = {TIE_PIDENT, AT_THRESHOLD - 1}

    def add(self, name, loci, hits):
        self.contigs[name] = (loci, hits)

    def pident(self, base):
        """The next unused percent identity at or above base, in thousandths, never dyadic."""
        t = int(round(base * 1000))
        while t in self.used or t % 3125 == 0:
            t += 1
        self.used.add(t)
        return t

    def annotations(self, k):
        if self.n_sys == 1:
            return "|KO=K{}".format(k)
        mask = (k * 37 + 1) & 127       # a varying subset of the systems; none when 0
        return "".join("|S{}=v{}_{}".format(s, s, k) for s in range(self.n_sys) if (mask >> s) & 1)

    def write(self, tmp):
        """The four plain files under tmp, for the reference; gzipped copies under INPUTS."""
        os.makedirs(INPUTS, exist_ok=True)
        stem = os.path.join(tmp, self.stem)
        with open(stem + ".taxonomy.tsv", "w") as fh:
            fh.writelines("{}\t{}\n".format(c, p) for c, p in TAXONOMY)
        lengths = {}
        for name, (loci, hits) in self.contigs.items():
            lengths[name] = 500 + max([max(l[:2]) for l in loci] + [h.qe for h in hits])
        with open(stem + ".fna", "w") as fh:
            for name in self.contigs:
                fh.write(">{}\n{}\n".format(name, "N" * lengths[name]))
        with open(stem + ".gff", "w") as fh:
            for name, (loci, _) in self.contigs.items():
                for s, e, strand in loci:
                    fh.write("{}\thand\tgene\t{}\t{}\t.\t{}\t0\t.\n".format(name, s, e, strand))
        scores, k = [], 0
        with open(stem + ".blastout", "w") as fh:
            for name, (_, hits) in self.contigs.items():
                for h in hits:
                    t = h.pident if h.pident is not None else self.pident(h.base)
                    n = h.qe - h.qs + 1
                    ss, se = (1, n) if h.strand == "plus" else (n, 1)
                    fh.write("{}\tH{}|{}{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}\t{}.{:03d}\t{}\t0\t0.0\t500\t{}\n".format(
                        name, k, h.taxon, self.annotations(k) if h.annot else "", lengths[name], h.slen, n,
                        h.qs, h.qe, ss, se, t // 1000, t % 1000, n, h.strand))
                    scores.append((n / float(h.slen)) * float("{}.{:03d}".format(t // 1000, t % 1000)) / 100.0)
                    k += 1
        # distinct and non-dyadic, but for the two deliberate exceptions
        plain = [s for s in scores if s not in (TIE_PIDENT / 1000.0 / 100.0, 0.5)]
        assert len(set(plain)) == len(plain), "equal scores in " + self.stem
        assert all(Fraction(s).denominator > 1 << 30 for s in plain), "a dyadic score in " + self.stem
        paths = [stem + e for e in (".fna", ".blastout", ".gff", ".taxonomy.tsv")]
        for p in paths:                 # (mtime 0: the same bytes from every run)
            with open(p, "rb") as src, open(os.path.join(INPUTS, os.path.basename(p) + ".gz"), "wb") as raw, \
                    gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as out:
                out.write(src.read())
        return paths


def row(n, first=1001, size=200, gap=10, strand="+"):
    """n loci of `size` sites, `gap` sites apart."""
    return [(first + (size + gap) * g, first + (size + gap) * g + size - 1, strand) for g in range(n)]


def full(taxon, locus, base, **kw):
    return Hit(taxon, min(locus[:2]), max(locus[:2]), base, **kw)


def owner(loci, skip=(), taxon="s__A1", base=88.0, **kw):
    """One whole-locus hit per locus: the clade the contig's answer rests on."""
    return [full(taxon, l, base, **kw) for g, l in enumerate(loci) if g not in skip]


def inside(loci, n, base=60.0):
    """n hits, each inside one locus, over every species and locus in turn."""
    out = []
    for k in range(n):
        l = loci[k % len(loci)]
        size = l[1] - l[0] + 1
        a = (k * 17) % (size - 60)
        out.append(Hit(SPECIES[k % 6], l[0] + a, l[0] + a + 40 + (k * 7) % 20, base + 5 * (k % 6)))
    return out


def bridging(loci, n, base=60.0):
    """n hits, each from the middle of one locus to the middle of the next: two attachments."""
    out = []
    for k in range(n):
        g = k % (len(loci) - 1)
        out.append(Hit(SPECIES[k % 6], loci[g][0] + 100, loci[g + 1][0] + 99, base + 5 * (k % 6)))
    return out


def by_start(hits):
    return sorted(hits, key=lambda h: (h.qs, h.qe))


def edge_contig(S, name, hit, loci=None):
    """Locus 0 carries only `hit`; the owner clade's whole-locus hit is on locus 1."""
    loci = loci or [(1001, 1300, "+"), (2001, 2300, "+")]
    S.add(name, loci, [hit] + owner(loci, skip=(0,)))


def annotation_contig(S):
    loci = row(4, size=300, gap=100)
    hits = [
        # locus 0: two hits at one best score, the later wins; then a lower one that must not
        full("s__A1", loci[0], 0, pident=TIE_PIDENT), full("s__A1", loci[0], 0, pident=TIE_PIDENT),
        full("s__A1", loci[0], 85.0),
        # locus 1: annotated, then a higher-scoring hit without annotation, then a lower annotated
        full("s__A1", loci[1], 90.0), full("s__A1", loci[1], 95.0, annot=False), full("s__A1", loci[1], 86.0),
        # locus 2: the only annotated hit scores exactly the threshold; locus 3: just below it
        full("s__A1", loci[2], 92.0, annot=False), full("s__B1", loci[2], 0, pident=AT_THRESHOLD),
        full("s__A1", loci[3], 93.0, annot=False), full("s__B1", loci[3], 0, pident=AT_THRESHOLD - 1),
    ]
    S.add("ann", loci, hits)


def count_contigs(S, loci_counts, hit_counts):
    for n in loci_counts:
        loci = row(n)
        # the owner, a second species on every third locus, a few hits over two loci
        hits = owner(loci) + [full("s__B1", l, 70.0) for l in loci[::3]] + bridging(loci[:6], min(5, n - 1))
        S.add("loci{}".format(n), loci, by_start(hits))
    for n in hit_counts:
        loci = row(8)
        S.add("hits{}".format(n), loci, by_start(owner(loci) + inside(loci, n - 8)))


def build_attach():
    S = InputSet("attach", 1)
    two = [(1001, 1300, "+"), (2001, 2300, "+")]
    edge_contig(S, "b_last_on_first", Hit("s__A1", 997, 1001, 88.0))
    edge_contig(S, "b_last_before_first", Hit("s__A1", 996, 1000, 88.0))
    edge_contig(S, "b_first_on_last", Hit("s__A1", 1300, 1304, 88.0))
    edge_contig(S, "b_first_after_last", Hit("s__A1", 1301, 1305, 88.0))
    edge_contig(S, "b_contains", Hit("s__A1", 901, 1400, 88.0))
    edge_contig(S, "b_inside", Hit("s__A1", 1101, 1200, 88.0))
    three = row(3, size=300, gap=100)
    S.add("b_over3", three, [Hit("s__A1", 1201, 1900, 88.0), full("s__B1", three[1], 70.0)])
    for n in (26, 27):
        loci = row(30)
        S.add("b_over{}".format(n), loci,
              by_start(owner(loci) + [Hit("s__A2", loci[1][0], loci[n][1], 80.0)]))
    # den = the hit's 50 sites; ov = the sites past the locus's first
    for tag, ov in (("10_below", 4), ("10_at", 5), ("10_above", 6), ("50_below", 24), ("50_at", 25),
                    ("50_above", 26)):
        edge_contig(S, "ovl_" + tag, Hit("s__A1", 951 + ov, 1000 + ov, 88.0))
    layouts = {
        "lay_adjacent": [(1001, 1300, "+"), (1301, 1600, "+"), (1601, 1900, "+")],
        "lay_touching": [(1001, 1300, "+"), (1300, 1600, "+"), (1601, 1900, "+")],
        "lay_overlap2": [(1001, 1300, "+"), (1299, 1600, "+"), (1601, 1900, "+")],
        "lay_nested": [(1001, 1900, "+"), (1201, 1500, "+"), (2001, 2300, "+")],
        "lay_descending": [(2001, 2300, "+"), (1600, 1301, "-"), (1001, 1300, "+")],
    }
    for name, loci in layouts.items():
        S.add(name, loci, owner(loci) + [Hit("s__B1", 1251, 1350, 70.0), Hit("s__B2", 1281, 1320, 75.0),
                                         Hit("s__A2", 1101, 2100, 80.0)])
    count_contigs(S, (1, 63, 64, 65, 128, 129), (64, 65, 256, 257, 512, 513))
    loci = row(5)
    S.add("att225", loci, by_start(owner(loci) + inside(loci, 220)))
    loci = row(8)
    S.add("att514", loci, by_start(bridging(loci, 257)))
    loci = [(1001, 1300, "+"), (1401, 1700, "-"), (1801, 2100, ".")]
    S.add("strands", loci, owner(loci) + owner(loci, taxon="s__B1", base=70.0, strand="minus"))
    for tag, n in (("at", 900), ("below", 899), ("above", 901)):
        edge_contig(S, "scov_" + tag, Hit("s__A1", 1001, 1000 + n, 88.0, slen=1000),
                    loci=[(1001, 2000, "+"), (2501, 2800, "+")])
    annotation_contig(S)
    return S


def build_attach7():
    S = InputSet("attach7", 7)
    annotation_contig(S)
    count_contigs(S, (9, 10), (65, 257, 513))
    three = row(3, size=300, gap=100)
    S.add("b_over3", three, [Hit("s__A1", 1201, 1900, 88.0), full("s__B1", three[1], 70.0)])
    loci = [(1001, 1300, "+"), (1300, 1600, "+"), (1601, 1900, "+")]
    S.add("lay_touching", loci, owner(loci) + [Hit("s__B1", 1251, 1350, 70.0)])
    loci = [(1001, 1300, "+"), (1401, 1700, "-"), (1801, 2100, ".")]
    S.add("strands", loci, owner(loci) + owner(loci, taxon="s__B1", base=70.0, strand="minus"))
    return S


def build_hbm(stem, n_sys, loci_counts):
    S = InputSet(stem, n_sys)
    count_contigs(S, loci_counts, ())
    annotation_contig(S)
    return S


def main():
    import tempfile
    sets = [build_attach(), build_attach7(), build_hbm("attachhbm", 1, (256, 257)),
            build_hbm("attachhbm7", 7, (36, 37))]
    with tempfile.TemporaryDirectory() as tmp:
        for S in sets:
            inputs = S.write(tmp)
            for flags in SETS[S.stem][1]:
                name = "{}_{}".format(S.stem, make_golden.flag_tag(flags))
                make_golden.make_case(name, inputs, flags, dict(kind="files", dir="attach_inputs", stem=S.stem, gz=True),
                                      tmp, dump_scores=True)
                with gzip.open(os.path.join(HERE, name + ".json.gz"), "rt") as fh:
                    assert json.load(fh)["ties"] == [], name


if __name__ == "__main__":
    main()
