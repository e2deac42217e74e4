"""The gapped extension of the homology search without a GPU: the two CPU
forms of the rule against each other on the hand-built cases and the planted homolog, the
ordering and row writer of waafle_amd.search for gapped records against the oracle's, the
unchanged ungapped defaults, the row arithmetic on the reference's demo table, the bindings,
and the halving of a refused chunk."""
import ctypes as C
import gzip
import math
import os

import numpy as np
import pytest

import search_cases as sc
import search_gap_cases as gc
import search_gap_oracle as go
import search_oracle as so
from waafle_amd import lib, search

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", sorted(gc.HAND_BUILT))
def test_hand_built_cases_both_forms_agree(name):
    contigs, subjects, P, n = gc.HAND_BUILT[name]()
    a = go.search_gapped_cells(contigs, subjects, P)
    assert a == go.search_gapped_arrays(contigs, subjects, P)
    assert len(a) == n
    if name in gc.PINNED:
        assert [r[3:] for r in a] == [gc.PINNED[name]]
    for r in a:
        assert 2 * r[7] == r[4] + r[6] + r[9] and go.score2_of(r) >= 2 * P["min_score"]


def test_hand_built_cases_say_what_their_names_say():
    def recs(name):
        contigs, subjects, P, _ = gc.HAND_BUILT[name]()
        return go.search_gapped_cells(contigs, subjects, P), contigs, subjects
    for W in (1, 15, 31):                                    # bridged: W gap columns in one record
        assert [r[9] for r in recs("gap_w{}_bridged".format(W))[0]] == [W]
        assert [r[9] for r in recs("gap_w{}_plus_one".format(W))[0]] == [0, 0]
    (r,), _, subjects = recs("subject_ends")
    assert (r[5], r[6]) == (0, len(subjects[0]))
    (a, b), contigs, _ = recs("store_ends")
    assert a[3] == 0 and b[0] == 1 and b[3] + b[4] == len(contigs[1]) and a[9] == b[9] == 1
    (a, b), contigs, _ = recs("contig_junction")
    assert a[3] + a[4] == len(contigs[0]) and (b[0], b[3]) == (1, 0)
    assert [r[2] for r in recs("minus_strand")[0]] == [1]
    (r,), _, _ = recs("n_inside")
    assert r[7] - r[9] - r[8] == 2                           # the two N columns
    spans = sorted((r[6], r[9]) for r in recs("refill_lengths")[0])
    assert spans == [(L, 0) for L in (62, 63, 64, 65, 66, 126, 127, 128, 129, 130)]
    assert sorted((r[6], r[9]) for r in recs("refill_gaps")[0]) == sorted(
        [(L + 20, 1) for L in (62, 63, 64, 65, 66, 126, 127, 128, 129, 130)] * 2)
    assert [r[3] for r in recs("gene_twice")[0]] == [100, 350]


def test_planted_homolog():
    """The gene of DESIGN.md §12.5: every ungapped record covers less than 0.3 of the subject
    (the scorer's --min-scov 0.75 drops them all); the gapped rule gives one record that covers
    all of it, on either strand."""
    contigs, subjects, P = gc.planted()
    M = len(subjects[0])
    assert M == 1000
    ungapped = so.search_indexed(contigs, subjects, P)
    assert len(ungapped) == 8 and all(r[5] / M < 0.3 for r in ungapped)
    assert [r[3:6] for r in ungapped if r[2] == 0] == [(500, 0, 200), (698, 196, 282), (982, 483, 278), (1258, 758, 242)]
    a = go.search_gapped_cells(contigs, subjects, P)
    assert a == go.search_gapped_arrays(contigs, subjects, P)
    assert a == [(0, 0, 0, 500, 1000, 0, 1000, 1003, 971, 6), (0, 1, 1, 500, 1000, 0, 1000, 1003, 971, 6)]


def test_medium_set_has_what_the_gpu_test_needs():
    contigs, subjects, P = gc.medium()
    assert len(contigs) == 40 and len(subjects) == 200
    assert sum(c.count(subjects[190]) for c in contigs) == 70 > P["max_occ"]
    recs = go.search_gapped_arrays(contigs, subjects, P)
    assert len(recs) > 150 and {r[2] for r in recs} == {0, 1}
    assert max(r[9] for r in recs) >= 6 and sum(1 for r in recs if r[9] > 0) > 50


# ---------------------------------------------------------------------------
# ordering, --max-target-seqs, rows
# ---------------------------------------------------------------------------

def as_arrays(recs):
    cols = list(zip(*recs)) if recs else [()] * 10
    return {f: np.array(c, dt) for (f, dt), c in zip(search.GAP_RECORD_FIELDS, cols)}


HAND = [  # contig, subject, minus, qstart, qspan, sstart, sspan, length, matches, gaps
    (1, 0, 0, 10, 50, 0, 50, 50, 50, 0),         # score2 100
    (0, 2, 0, 5, 41, 0, 40, 41, 40, 1),          # 75
    (0, 1, 1, 7, 40, 3, 41, 41, 40, 1),          # 75: subject 1 before subject 2
    (0, 1, 0, 7, 40, 3, 41, 41, 40, 1),          # 75: plus before minus
    (0, 1, 0, 7, 41, 3, 40, 41, 40, 1),          # 75: qspan 41 after 40
    (0, 1, 0, 2, 41, 3, 40, 41, 40, 1),          # 75: qstart
    (0, 3, 0, 0, 100, 0, 100, 100, 100, 0),      # 200
    (0, 2, 0, 300, 30, 0, 30, 30, 30, 0),        # 60: subject 2's second row
    (0, 0, 0, 50, 38, 0, 38, 38, 38, 0),         # 76
]


def test_order_and_max_target_seqs():
    rec = as_arrays(HAND)
    assert search.score_of(rec).tolist() == [go.score2_of(r) for r in HAND] == [100, 75, 75, 75, 75, 75, 200, 60, 76]
    assert search.order_records(rec, 10000).tolist() == [6, 8, 5, 3, 4, 2, 1, 7, 0]
    # contig 0 ranks its subjects 3 (200), 0 (76), 1 (75), 2 (75)
    assert search.order_records(rec, 3).tolist() == [6, 8, 5, 3, 4, 2, 0]
    assert search.order_records(rec, 1).tolist() == [6, 0]
    assert search.order_records(as_arrays([]), 5).tolist() == []
    names, lens = ["c0", "c1"], [1000, 800]
    sids, slens = ["s0|t", "s1|t", "s2|t", "s3|t"], [60, 90, 70, 100]
    for limit in (10000, 3, 2, 1):
        got = search.format_rows(rec, search.order_records(rec, limit), names, lens, sids, slens, 320)
        assert got == go.rows(HAND, names, lens, sids, slens, 320, limit)
    assert search.format_rows(as_arrays([]), np.zeros(0, np.int64), names, lens, sids, slens, 320) == []


def test_row_format_with_a_half_unit_score():
    # 57 matches, 2 mismatches, 1 gap column: score2 = 114 - 8 - 5 = 101, score 50.5
    rec = as_arrays([(0, 0, 0, 10, 59, 4, 60, 60, 57, 1), (0, 0, 1, 100, 92, 4, 90, 92, 90, 2)])
    rows = search.format_rows(rec, np.array([1, 0]), ["ctg"], [500], ["gene|s__A|K=1"], [120], 1000)
    minus, plus = (r.split("\t") for r in rows)
    assert len(plus) == len(minus) == 15
    assert plus[:12] == ["ctg", "gene|s__A|K=1", "500", "120", "60", "11", "69", "5", "64", "95.000", "57", "1"]
    assert plus[13] == "%.1f" % ((1.28 * 50.5 - math.log(0.46)) / math.log(2)) == "94.4" and plus[14] == "plus"
    assert float(plus[12]) == pytest.approx(0.46 * 500 * 1000 * math.exp(-1.28 * 50.5), rel=1e-2)
    # minus: variant columns 4..93 are subject bases 116 down to 27; score2 = 180 - 10 = 170
    assert minus[4:12] == ["92", "101", "192", "116", "27", "97.826", "90", "2"] and minus[14] == "minus"
    assert minus[13] == str(int((1.28 * 85 - math.log(0.46)) / math.log(2))) == "158"


def test_without_gapped_nothing_changes():
    args = search.build_parser().parse_args(["c.fna", "genes.fna", "--searcher", "native"])
    assert (args.gapped, args.band, args.xdrop_gap) == (False, 15, 30)
    assert (args.seed_length, args.seed_stride, args.max_seed_hits, args.xdrop, args.min_score) == (21, 8, 64, 20, 28)
    assert search.RECORD_FIELDS == (("contig", np.int32), ("subject", np.int32), ("minus", np.uint8),
                                    ("qstart", np.int32), ("sstart", np.int32), ("length", np.int32),
                                    ("matches", np.int32))
    rec = {f: np.array(c, dt) for (f, dt), c in zip(search.RECORD_FIELDS, zip((0, 0, 0, 10, 4, 60, 57),
                                                                              (0, 0, 1, 100, 4, 90, 90)))}
    assert search.score_of(rec).tolist() == [51, 90]
    assert search.format_rows(rec, search.order_records(rec), ["ctg"], [500], ["gene|s__A|K=1"], [120], 1000) == [
        "ctg\tgene|s__A|K=1\t500\t120\t90\t101\t190\t116\t27\t100.000\t90\t0\t2.14e-45\t167\tminus",
        "ctg\tgene|s__A|K=1\t500\t120\t60\t11\t70\t5\t64\t95.000\t57\t0\t1.03e-23\t95.3\tplus"] == so.rows(
            [(0, 0, 0, 10, 4, 60, 57), (0, 0, 1, 100, 4, 90, 90)], ["ctg"], [500], ["gene|s__A|K=1"], [120], 1000)
    args = search.build_parser().parse_args(["c.fna", "genes.fna", "--searcher", "native", "--gapped", "--band", "7",
                                             "--xdrop-gap", "12"])
    assert (args.gapped, args.band, args.xdrop_gap) == (True, 7, 12)


def test_row_arithmetic_against_the_demo_table():
    """The 601 gapped rows of the reference's demo table (of 1416): 2 length = qspan + sspan +
    gaps on every one, so the row's columns are the record's fields.  The row bit score of the
    rule, from score = matches - 2 mismatches - 2.5 gaps, against the file's: equal on 254
    rows, lower on 222, higher on 125.  blastn's gapped alignments come from another
    algorithm and another gap cost; the difference is stated, not something to fix."""
    path = os.path.join(HERE, "golden", "demo_inputs", "demo_contigs.blastout.gz")
    rows = [l.rstrip("\n").split("\t") for l in gzip.open(path, "rt")]
    assert len(rows) == 1416
    rows = [r for r in rows if int(r[11]) > 0]
    assert len(rows) == 601
    equal = lower = higher = 0
    for r in rows:
        length, m, gaps = int(r[4]), int(r[10]), int(r[11])
        qspan, sspan = int(r[6]) - int(r[5]) + 1, abs(int(r[8]) - int(r[7])) + 1
        assert 2 * length == qspan + sspan + gaps, r
        rec = as_arrays([(0, 0, 0, 0, qspan, 0, sspan, length, m, gaps)])
        score = int(search.score_of(rec)[0]) / 2
        assert score == m - 2 * (length - gaps - m) - 2.5 * gaps
        text = search.bitscore_text(score)
        assert text == so.bitscore_text(score)
        equal += float(text) == float(r[13])
        lower += float(text) < float(r[13])
        higher += float(text) > float(r[13])
    assert (equal, lower, higher) == (254, 222, 125)


# ---------------------------------------------------------------------------
# bindings, the refused chunk
# ---------------------------------------------------------------------------

def test_bindings():
    assert C.sizeof(lib.WfSearchGapParams) == 16 and C.sizeof(lib.WfSearchGapResult) == 136
    res, args = lib.SIGNATURES["wf_search_gapped"]
    assert res is C.c_int and len(args) == 5
    assert args[3]._type_ is lib.WfSearchGapParams and args[4]._type_ is lib.WfSearchGapResult
    assert [f for f, _ in search.GAP_RECORD_FIELDS] == [f for f, _ in lib.WfSearchGapResult._fields_[2:12]]
    assert tuple(f for f, _ in search.GAP_RECORD_FIELDS) == go.FIELDS
    header = open(os.path.join(os.path.dirname(HERE), "include", "waafle_hip.h")).read()
    assert "int wf_search_gapped(wf_ctx* ctx" in header and "#define WF_ABI_VERSION 6 " in header


class Refusing:
    """A searcher that refuses chunks of more than `limit` bases."""

    def __init__(self, limit):
        self.limit, self.calls = limit, []

    def search_gapped(self, seq, off):
        self.calls.append(len(off) - 1)
        if off[-1] > self.limit:
            raise lib.WaafleHipError(lib.WF_E_TOOBIG, "too big")
        n = len(off) - 1
        out = {f: np.zeros(n, dt) for f, dt in search.GAP_RECORD_FIELDS}
        out["subject"] = np.arange(n, dtype=np.int32)
        out["sspan"] = np.diff(off).astype(np.int32)
        return out

    def search(self, seq, off):
        raise AssertionError("the gapped call was asked for")


def test_refused_gapped_chunk_is_halved():
    seq, off = sc.flat(["A" * 10, "C" * 30, "G" * 20, "T" * 5, "A" * 40])
    s = Refusing(45)
    out = search.search_chunk(s, seq, off, gapped=True)
    assert out["subject"].tolist() == [0, 1, 2, 3, 4] and out["sspan"].tolist() == [10, 30, 20, 5, 40]
    assert set(out) == {f for f, _ in search.GAP_RECORD_FIELDS}
    assert s.calls[0] == 5 and len(s.calls) > 1
    with pytest.raises(search.SearchError):
        search.search_chunk(Refusing(30), seq, off, gapped=True)
