"""Hand-built record sets for the record-to-hit rule, each with the hit_off it
must give written down, and the (matches, length) sweeps.  A case is the dict tests/hits_oracle.py
describes plus `hit_off`.  A record is (contig, subject, minus, qstart, qspan, sstart, sspan,
length, matches)."""
import numpy as np

COLUMNS = ("contig", "subject", "minus", "qstart", "qspan", "sstart", "sspan", "length", "matches")
EDGES = [("s__A", "g__G"), ("s__B", "g__G"), ("s__C", "g__H"), ("g__G", "f__F"), ("g__H", "f__F"),
         ("f__F", "r__Root")]
# subjects with 0, 1 and 6 annotation systems, and one with a seventh (UniProt, a .. f, g: bit 7,
# which the packed key does not hold)
SUBJECTS = [("g0|s__A", 400), ("g1|s__B|UniProt=P1", 300), ("g2|s__C|a=1|b=2|c=3|d=4|e=5|f=6", 1000),
            ("g3|s__A|UniProt=P1|a=9|b=8|c=7|d=6|e=5|f=4", 500), ("g4|s__D|g=1|a=2", 800)]


def make(qlen, records, hit_off, min_scov=0.75, subjects=SUBJECTS):
    cols = {f: [r[k] for r in records] for k, f in enumerate(COLUMNS)}
    return dict(contig_names=["ctg{}".format(c) for c in range(len(qlen))], qlen=list(qlen),
                subject_ids=[s for s, _ in subjects], slen=[n for _, n in subjects], edges=EDGES,
                min_scov=min_scov, cols=cols, hit_off=list(hit_off))


def empty():
    return make([500, 600], [], [0, 0, 0])


def one_record():
    return make([1000], [(0, 0, 0, 10, 400, 0, 400, 400, 390)], [0, 1])


def contigs_without_hits():
    """first, in the middle and last"""
    return make([900] * 5, [(1, 1, 0, 0, 300, 0, 300, 300, 300), (1, 2, 1, 100, 700, 20, 700, 700, 650),
                            (3, 0, 1, 400, 380, 10, 380, 380, 0)], [0, 0, 2, 2, 3, 3])


def one_contig_everything():
    """plus and minus rows, gapped records (qspan != sspan), matches 0 and matches = length, all
    five subjects (eight systems)"""
    return make([2000], [(0, 0, 0, 0, 400, 0, 400, 400, 400), (0, 1, 1, 450, 297, 2, 295, 299, 280),
                         (0, 2, 0, 800, 990, 5, 995, 1001, 903), (0, 3, 1, 100, 480, 12, 477, 483, 0),
                         (0, 4, 0, 1200, 790, 3, 793, 795, 795), (0, 1, 0, 1500, 250, 25, 250, 250, 249)], [0, 6])


def trims():
    """ltrim > 0 (the subject overhangs the contig's start), rtrim > 0, and both on a contig
    shorter than its subject"""
    return make([2000, 300], [(0, 0, 0, 10, 250, 100, 250, 250, 240), (1, 2, 0, 100, 200, 50, 200, 200, 150),
                              (1, 2, 1, 0, 300, 200, 300, 300, 299)], [0, 1, 3])


def scov_at_min(min_scov):
    """scov = 300 / 400 = 0.75 exactly, and the neighbours 299 / 400 and 301 / 400"""
    return make([2000], [(0, 0, 0, 500, 300, 50, 300, 300, 290), (0, 0, 1, 500, 299, 50, 299, 299, 290),
                         (0, 0, 0, 500, 301, 50, 301, 301, 290)], [0, 3], min_scov=min_scov)


SIZED_OFF = {63: [0, 31, 31, 32, 63], 64: [0, 32, 32, 33, 64], 65: [0, 32, 32, 33, 65],
             256: [0, 128, 128, 129, 256], 257: [0, 128, 128, 129, 257]}


def sized(n):
    """n records over four contigs: the first half in contig 0, none in 1, one in 2, the rest in 3"""
    recs = []
    for i in range(n):
        c = 0 if i < n // 2 else (2 if i == n // 2 else 3)
        length = 200 + i
        recs.append((c, i % 5, i % 2, 5 * i, length - i % 3, i % 7, length - (i + 1) % 3, length, length - i % 11))
    return make([5000] * 4, recs, SIZED_OFF[n])


HAND_BUILT = {
    "empty": empty, "one_record": one_record, "contigs_without_hits": contigs_without_hits,
    "one_contig_everything": one_contig_everything, "trims": trims,
    "scov_min_exact": lambda: scov_at_min(0.75),
    "scov_min_ulp_above": lambda: scov_at_min(float(np.nextafter(0.75, 1.0))),
    "scov_min_ulp_below": lambda: scov_at_min(float(np.nextafter(0.75, 0.0))),
}
HAND_BUILT.update({"sized_{}".format(n): (lambda n=n: sized(n)) for n in SIZED_OFF})


def sweep(lengths):
    """Every matches in 0 .. L for every L of `lengths`: one subject per L, three contigs."""
    lengths = [int(v) for v in lengths]
    L = np.concatenate([np.full(v + 1, v, np.int64) for v in lengths])
    m = np.concatenate([np.arange(v + 1, dtype=np.int64) for v in lengths])
    g = np.concatenate([np.full(v + 1, k, np.int64) for k, v in enumerate(lengths)])
    n = len(L)
    cols = dict(contig=(np.arange(n, dtype=np.int64) * 3) // n, subject=g, minus=m & 1, qstart=(m * 3) % 97,
                qspan=L, sstart=m % (L % 5 + 1), sspan=L, length=L, matches=m)
    subjects = [("w{}|s__{}|sys=v{}".format(v, "ABC"[v % 3], v % 7), v + v % 5) for v in lengths]
    case = make([250000] * 3, [], [], subjects=subjects)
    case["cols"] = cols
    case["hit_off"] = np.searchsorted(cols["contig"], np.arange(4), side="left").tolist()
    return case
