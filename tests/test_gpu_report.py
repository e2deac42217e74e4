"""The reporting step of the native search on the GPU (wf_report.hip).

wf_search_report / wf_search_report_gapped in both forms (WF_OPT_SEARCH_REPORT 0 host, 1 device)
against the two CPU forms of tests/report_oracle.py: the hand-built cases of
tests/report_cases.py and seeded random sets in three shapes around the wave, block and launch
sizes; a large call between small ones; the refusals; the capacity protocol.  Then the four
search calls with the option at 1: the hand-built search cases against their oracles, the medium
sets however cut (FASTA and packed, with a low-complexity mask) and a case past one extend launch
and one gapped launch against the host form; and the two commands, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import report_cases as rc
import report_oracle as ro
import search_cases as sc
import search_dust_cases as sdc
import search_gap_cases as gc
import search_gap_oracle as go
import search_oracle as so
from test_gpu_search_db import make, run_ascii, run_packed
from test_gpu_search_gap import _sample
from waafle_amd import lib, makedb, search, workflow

pytestmark = pytest.mark.gpu

FIELDS = [f for f, _ in search.RECORD_FIELDS]
GAP_FIELDS = [f for f, _ in search.GAP_RECORD_FIELDS]
FORMS = ("host", "device")


class Ctx:
    def __init__(self):
        self.so, self.h = lib.load(), C.c_void_p()
        assert self.so.wf_init(0, C.byref(self.h)) == lib.WF_OK

    def form(self, where):
        assert self.so.wf_set_option(self.h, lib.OPT_SEARCH_REPORT, FORMS.index(where)) == lib.WF_OK
        return self

    def close(self):
        self.so.wf_free(self.h)


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def kw(P, **more):
    out = dict(seed_length=P["S"], seed_stride=P["T"], max_seed_hits=P["max_occ"], xdrop=P["X"],
               min_score=P["min_score"])
    if "W" in P:
        out.update(band=P["W"], xdrop_gap=P["Xg"])
    if "Wd" in P:
        out.update(dust_window=P["Wd"], dust_level=P["Lv"])
    out.update(more)
    return out


def rows(out, fields):
    return list(zip(*[out[f].tolist() for f in fields]))


def report(ctx, where, raw, min_score, gapped):
    """(records as they come, counters) of the tuples `raw` in the form `where`; the order is checked"""
    cols = ro.columns(raw, ro.ANCHOR if gapped else ro.HSP)
    out, stats = search.report_records(ctx.form(where), cols, min_score)
    got = rows(out, GAP_FIELDS if gapped else FIELDS)
    assert got == sorted(got, key=ro.sort_key if gapped else None), "the records come back in the defined order"
    for f, dt in (search.GAP_RECORD_FIELDS if gapped else search.RECORD_FIELDS):
        assert out[f].dtype == dt
    return got, stats


def check(ctx, raw, min_score, gapped, both_oracles=True):
    """both forms of the library against the CPU forms; returns the records"""
    if gapped:
        want, raw_alns = ro.alns_any(raw, min_score)
        if both_oracles:
            assert (want, raw_alns) == ro.alns_greedy(raw, min_score)
    else:
        want = ro.hsps_reach(raw, min_score)
        if both_oracles:
            assert want == ro.hsps_pairwise(raw, min_score)
    for where in FORMS:
        got, stats = report(ctx, where, raw, min_score, gapped)
        assert sorted(got) == want, where
        if gapped:
            assert (stats["anchors"], stats["raw_alignments"]) == (len(raw), raw_alns), where
            assert stats["seed_hits"] == stats["seeds_skipped"] == stats["raw_hsps"] == 0
        else:
            assert (stats["seed_hits"], stats["seeds_skipped"], stats["raw_hsps"]) == (0, 0, len(raw)), where
    return want


# ---- the stand-alone entries -------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(rc.UNGAPPED))
def test_ungapped_cases(ctx, name):
    raw, min_score, n = rc.UNGAPPED[name]()
    assert len(check(ctx, raw, min_score, False)) == n


@pytest.mark.parametrize("name", sorted(rc.GAPPED))
def test_gapped_cases(ctx, name):
    raw, min_score, n, _ = rc.GAPPED[name]()
    assert len(check(ctx, raw, min_score, True)) == n


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65537])
def test_random_sets(ctx, n):
    """three shapes: one group with everything, every element (nearly) its own group, groups of
    about 200"""
    for groups in (1, 10 * n, max(1, n // 200)):
        check(ctx, rc.random_hsps(n, n + groups, groups, span=48 if groups > 1 else 96), 20, False)
        check(ctx, rc.random_anchors(n, n + groups, groups), 20, True)


def big_columns(n, seed, gapped):
    """n raw elements as numpy columns (lists of tuples are slow at 2^20): about n / 150 groups"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, max(1, n // 150), n)
    cols = {"contig": k % 7, "subject": k // 7, "minus": k % 2}
    if not gapped:
        b = rng.integers(0, 120, n)
        e = b + rng.integers(1, 80, n)
        mism = (7 * b + 13 * e + k) % np.minimum(e - b + 1, 4)
        cols.update(delta=(k % 11) - 5, b=b, e=e, score=(e - b) - 3 * mism)
        return cols
    cols.update(i0=rng.integers(60, 120, n), j0=rng.integers(60, 120, n))
    for side in ("left", "right"):
        pairs, g_s, g_q = rng.integers(0, 60, n), rng.integers(0, 2, n), rng.integers(0, 3, n) // 2
        m = pairs - np.minimum(pairs, rng.integers(0, 3, n))
        cols.update({side + "_H": 6 * m - 4 * pairs - 5 * (g_s + g_q), side + "_p": pairs + g_s,
                     side + "_q": pairs + g_q, side + "_g": g_s + g_q})
    return cols


@pytest.fixture(scope="module")
def big():
    n = (1 << 20) + 1
    return {gapped: big_columns(n, 77 + gapped, gapped) for gapped in (False, True)}


@pytest.mark.parametrize("gapped", [False, True], ids=["ungapped", "gapped"])
def test_a_large_call_between_small_ones_on_one_context(big, gapped):
    """n = 2^20 + 1: the device form equals the host form; then 5, 4097 and 2^20 + 1 again on
    the same context, whose arrays only grow"""
    fields = GAP_FIELDS if gapped else FIELDS
    ctx = Ctx()
    try:
        host, host_stats = search.report_records(ctx.form("host"), big[gapped], 20)
        assert 1000 < len(host["contig"]) < (1 << 20)
        want = rows(host, fields)
        small = {n: rc.random_anchors(n, n, 3) if gapped else rc.random_hsps(n, n, 3) for n in (5, 4097)}
        ctx.form("device")
        for n in ((1 << 20) + 1, (1 << 20) + 1, 5, 4097, (1 << 20) + 1):
            if n in small:
                got, _ = report(ctx, "device", small[n], 20, gapped)
                assert sorted(got) == (ro.alns_any(small[n], 20)[0] if gapped else ro.hsps_reach(small[n], 20))
                continue
            dev, dev_stats = search.report_records(ctx, big[gapped], 20)
            assert rows(dev, fields) == want and dev_stats == host_stats
    finally:
        ctx.close()


def bad_inputs(gapped):
    """(what, raw with one bad element, min_score, n, null column)"""
    if gapped:
        raw = rc.random_anchors(40, 1, 2)
        names = ro.ANCHOR
        bad = [("contig < 0", "contig", -1), ("subject < 0", "subject", -1), ("minus > 1", "minus", 2),
               ("negative p", "left_p", -1), ("negative q", "right_q", -3), ("negative g", "left_g", -1),
               ("odd sum", "right_p", None), ("inexact matches", "left_H", None), ("matches above length", "right_H", 10 ** 6)]
    else:
        raw = rc.random_hsps(40, 1, 2)
        names = ro.HSP
        bad = [("contig < 0", "contig", -1), ("subject < 0", "subject", -1), ("minus > 1", "minus", 2),
               ("e <= b", "e", 0), ("b < 0", "b", -1), ("no multiple of 3", "score", None), ("score too high", "score", 10 ** 6),
               ("score too low", "score", -10 ** 6)]
    cols = ro.columns(raw, names)
    for what, field, value in bad:
        c = {f: list(v) for f, v in cols.items()}
        c[field][17] = c[field][17] + 1 if value is None else value
        yield what, c, 20, None, None
    yield "min_score < 1", cols, 0, None, None
    yield "n < 0", cols, 20, -1, None
    yield "n >= 2^31", cols, 20, 1 << 31, None
    yield "a null column", cols, 20, None, names[-1]


@pytest.mark.parametrize("where", FORMS)
@pytest.mark.parametrize("gapped", [False, True], ids=["ungapped", "gapped"])
def test_refusals_leave_the_outputs_and_the_context(ctx, gapped, where):
    fields = search.GAP_RECORD_FIELDS if gapped else search.RECORD_FIELDS
    ctx.form(where)
    good = ro.columns(rc.random_anchors(40, 1, 2) if gapped else rc.random_hsps(40, 1, 2), ro.ANCHOR if gapped else ro.HSP)
    want = search.report_records(ctx, good, 20)[0]
    for what, cols, min_score, n, null in bad_inputs(gapped):
        out = {f: np.full(64, 77, dt) for f, dt in fields}
        held = {f: np.ascontiguousarray(cols[f], dtype=dt) for f, dt in (search.ANCHOR_FIELDS if gapped else search.HSP_FIELDS)}
        ptrs = {f: None if f == null else lib.ptr(v) for f, v in held.items()}
        n = 40 if n is None else n
        if gapped:
            a = lib.WfReportAnchors(n=n, min_score=min_score, **ptrs)
            r = lib.WfSearchGapResult(capacity=64, n=-5, raw_alignments=-5, **{f: lib.ptr(out[f]) for f, _ in fields})
            rc_ = ctx.so.wf_search_report_gapped(ctx.h, C.byref(a), C.byref(r))
        else:
            a = lib.WfReportHsps(n=n, min_score=min_score, **ptrs)
            r = lib.WfSearchResult(capacity=64, n=-5, raw_hsps=-5, **{f: lib.ptr(out[f]) for f, _ in fields})
            rc_ = ctx.so.wf_search_report(ctx.h, C.byref(a), C.byref(r))
        assert rc_ == lib.WF_E_BADINPUT, what
        assert r.n == -5 and (r.raw_alignments if gapped else r.raw_hsps) == -5, what
        assert all((v == 77).all() for v in out.values()), what
        if len(cols["contig"]) == 40 and null is None and 0 < n < 1 << 31 and min_score >= 1:
            assert b" 17" in ctx.so.wf_last_error(ctx.h), what     # the first offending record is named
        again = search.report_records(ctx, good, 20)[0]            # still usable
        assert all((again[f] == want[f]).all() for f in want), what
    assert ctx.so.wf_set_option(ctx.h, lib.OPT_SEARCH_REPORT, 2) == lib.WF_E_BADINPUT
    assert ctx.so.wf_set_option(ctx.h, lib.OPT_SEARCH_REPORT, -1) == lib.WF_E_BADINPUT
    assert all((search.report_records(ctx, good, 20)[0][f] == want[f]).all() for f in want)


@pytest.mark.parametrize("where", FORMS)
@pytest.mark.parametrize("gapped", [False, True], ids=["ungapped", "gapped"])
def test_capacity_one_then_room(ctx, gapped, where):
    raw = rc.random_anchors(300, 9, 4) if gapped else rc.random_hsps(300, 9, 4)
    fields = GAP_FIELDS if gapped else FIELDS
    want = ro.alns_any(raw, 20)[0] if gapped else ro.hsps_reach(raw, 20)
    want = sorted(want, key=ro.sort_key) if gapped else want
    assert len(want) >= 3
    cols = ro.columns(raw, ro.ANCHOR if gapped else ro.HSP)
    ctx.form(where)
    code, full, out, _ = search.report_once(ctx, cols, 20, 1)
    assert code == lib.WF_E_NOMEM and full == len(want) and rows(out, fields) == want[:1]
    code, full, out, _ = search.report_once(ctx, cols, 20, len(want))
    assert code == lib.WF_OK and full == len(want) and rows(out, fields) == want
    code, full, out, _ = search.report_once(ctx, {f: [] for f in cols}, 20, 0)      # n = 0 is valid
    assert code == lib.WF_OK and full == 0


# ---- the four search calls with the option at 1 ------------------------------------------------

@pytest.mark.parametrize("name", sorted(sc.HAND_BUILT))
def test_search_cases_on_the_device_equal_both_oracles(name):
    contigs, subjects, P, n = sc.HAND_BUILT[name]()
    want = so.search_brute(contigs, subjects, P)
    assert want == so.search_indexed(contigs, subjects, P)
    stats = []
    for where in FORMS:
        with search.Searcher(*sc.flat(contigs), **kw(P, report_on=where)) as s:
            got = rows(s.search(*sc.flat(subjects)), FIELDS)
            stats.append(dict(s.stats))
        assert got == want and len(got) == n, where
    assert stats[0] == stats[1]


@pytest.mark.parametrize("name", sorted(gc.HAND_BUILT))
def test_gapped_search_cases_on_the_device_equal_both_oracles(name):
    contigs, subjects, P, n = gc.HAND_BUILT[name]()
    want = go.search_gapped_cells(contigs, subjects, P)
    assert want == go.search_gapped_arrays(contigs, subjects, P)
    stats = []
    for where in FORMS:
        with search.Searcher(*sc.flat(contigs), **kw(P, report_on=where)) as s:
            got = rows(s.search_gapped(*sc.flat(subjects)), GAP_FIELDS)
            stats.append(dict(s.stats))
        assert got == sorted(got, key=ro.sort_key) and sorted(got) == want and len(got) == n, where
    assert stats[0] == stats[1] and stats[0]["anchors"] == len(so.search_indexed(contigs, subjects, P))


def every_cut(s, subjects, db, gapped):
    """the records whole, in chunks of 7 and of 1, from ASCII and from the packed database, and
    the counters of it all"""
    s.stats = dict.fromkeys(s.stats, 0)
    got = [run(s, src, size, gapped) for run, src in ((run_ascii, subjects), (run_packed, db))
           for size in (len(subjects), 7, 1)]
    return got, dict(s.stats)


@pytest.mark.parametrize("dust", [False, True], ids=["plain", "dust"])
@pytest.mark.parametrize("gapped", [False, True], ids=["ungapped", "gapped"])
def test_medium_sets_however_cut_equal_the_host_form(tmp_path, gapped, dust):
    if dust:
        contigs, subjects, P = sdc.medium_low()
        P = sdc.gap_params() if gapped else P
    else:
        contigs, subjects, P = gc.medium() if gapped else sc.medium()
    db = make(tmp_path, subjects)
    got = {}
    for where in FORMS:
        with search.Searcher(*sc.flat(contigs), **kw(P, report_on=where, dust=dust)) as s:
            got[where] = every_cut(s, subjects, db, gapped)
    host, host_stats = got["host"]
    assert len(host[0]) > 100 and all(g == host[0] for g in host)
    assert got["device"][0] == host and got["device"][1] == host_stats
    if not dust:
        assert host[0] == (go.search_gapped_arrays if gapped else so.search_indexed)(contigs, subjects, P)


def test_past_one_extend_launch_and_one_gapped_launch():
    """max_seed_hits 1024: a 40-base motif 1,024 times in the contigs and 70 subjects that hold it,
    at stride 1: 20 seeds x 1,024 occurrences x 70 subjects, more than 2^20 seed hits in the one
    tile, and 70 x 1,024 > 2^16 records to anchor.  The device form equals the host form."""
    motif = sc.rnd(40, 4242)
    contigs = ["".join(sc.rnd(23, 9000 + 128 * c + k) + motif for k in range(128)) + sc.rnd(23, 8000 + c)
               for c in range(8)]
    subjects = [sc.rnd(10, 100 + g) + motif + sc.rnd(10, 200 + g) for g in range(70)]
    P = dict(S=21, T=1, max_occ=1024, X=20, min_score=28, W=15, Xg=30)
    got = {}
    for where in FORMS:
        with search.Searcher(*sc.flat(contigs), capacity=1 << 17, **kw(P, report_on=where)) as s:
            ungapped = s.search(*sc.flat(subjects))
            gapped = s.search_gapped(*sc.flat(subjects))
            got[where] = (rows(ungapped, FIELDS), rows(gapped, GAP_FIELDS), dict(s.stats))
    stats = got["host"][2]
    assert stats["seed_hits"] > 2 * (1 << 20) and stats["anchors"] > 1 << 16       # two calls: the ungapped twice
    assert len(got["host"][0]) == stats["anchors"] >= 70 * 1024
    assert got["device"] == got["host"]


def test_ungapped_search_untouched_by_a_device_form_gapped_call():
    contigs, subjects, P = gc.medium()
    with search.Searcher(*sc.flat(contigs), **kw(P, report_on="device")) as s:
        before = s.search(*sc.flat(subjects[:60]))
        assert len(s.search_gapped(*sc.flat(subjects[30:90]))["contig"]) > 0
        after = s.search(*sc.flat(subjects[:60]))
        lo, hi, nn = s.chunk_planes(sum(len(x) for x in subjects[:60]), 0)          # wf_search_chunk_planes works as before
        assert len(lo) == len(hi) == len(nn)
    assert len(before["contig"]) > 20
    for f in FIELDS:
        np.testing.assert_array_equal(before[f], after[f])


# ---- the command lines -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("report")
    contigs, subjects, paths = _sample(tmp)
    wfdb = str(tmp / "genes.wfdb")
    makedb.main([paths[4], "--out", wfdb])
    return paths, {"fasta": paths[4], "wfdb": wfdb}


@pytest.mark.parametrize("flags", [[], ["--gapped"], ["--gapped", "--order-on", "device"]],
                         ids=["plain", "gapped", "gapped_order_on_device"])
def test_search_report_on_device_writes_the_same_table(sample, tmp_path, flags):
    paths, dbs = sample
    tables = []
    for where in FORMS:
        out = str(tmp_path / (where + ".blastout"))
        search.main([paths[0], dbs["fasta"], "--searcher", "native", "--out", out, "--chunk-bases", "1200",
                     "--report-on", where] + flags)
        tables.append(open(out, "rb").read())
    assert tables[0] == tables[1] and tables[0].count(b"\n") >= 12


def test_workflow_report_on_device_writes_the_same_files(sample, tmp_path):
    paths, dbs = sample
    got = []
    for where in FORMS:
        d = tmp_path / where
        d.mkdir()
        table, calls = str(d / "w.blastout"), str(d / "w.gff")
        workflow.main([paths[0], dbs["wfdb"], paths[3], "--outdir", str(d), "--basename", "w", "--quiet",
                       "--write-blastout", table, "--write-gff", calls, "--report-on", where])
        files = {k: open(str(d / "w.{}.tsv".format(k)), "rb").read() for k in ("lgt", "no_lgt", "unclassified")}
        files.update(table=open(table, "rb").read(), calls=open(calls, "rb").read())
        got.append(files)
    assert got[0] == got[1]
    assert got[0]["table"].count(b"\n") >= 12 and got[0]["calls"].count(b"\n") >= 6
