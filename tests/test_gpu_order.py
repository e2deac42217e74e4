"""wf_order_records (csrc/wf_order.hip) on the GPU against both CPU forms of the
rule: search.order_records (A) and tests/order_oracle.py (B).  The order, the kept count and
each gathered column, on the hand-built cases, on seeded random sets at the sizes that cross a
lane, wave, block and grid boundary, on a real search's records, and through both command lines.

The routes of the device form, each met below (`route` says which a set takes, from the same
ranges the library derives it from):
  * the sort key is 1, 2, 3 or 4 words of 64 bits, by the ranges of the call's own fields;
  * the pairs are ranked only when the limit is below both the record count and the span of the
    subject values (otherwise no contig can hold more subjects than the limit).
There is no per-contig LDS route and so no LDS bound: a contig of any size goes the same way,
which the one-contig shapes check at every size."""
import ctypes as C

import numpy as np
import pytest

import order_cases as oc
import order_oracle as oo
import search_cases as sc
from test_gpu_search import _sample, kw
from waafle_amd import hits, lib, makedb, search, workflow

pytestmark = pytest.mark.gpu

SENTINEL = -7
COLS = search.ORDER_COLUMNS
SIZES = (63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65537)
BIG_N = 2 ** 20 + 1


class Ctx:
    def __init__(self):
        self.so, self.h = lib.load(), C.c_void_p()
        assert self.so.wf_init(0, C.byref(self.h)) == lib.WF_OK

    def close(self):
        self.so.wf_free(self.h)


@pytest.fixture(scope="module")
def ctx():
    c = Ctx()
    yield c
    c.close()


def route(rec, limit):
    """(key words, ranked) of a call, as wf_order_records plans it"""
    n = len(rec["contig"])
    if n == 0:
        return 0, False
    fields = [rec["contig"], search.score_of(rec), rec["subject"], rec["minus"], rec["qstart"], rec["sstart"]]
    fields += [rec["qspan"], rec["sspan"]] if "gaps" in rec else []
    bits = sum((int(a.max()) - int(a.min())).bit_length() for a in fields)
    span = int(rec["subject"].max()) - int(rec["subject"].min()) + 1
    return (bits + 63) // 64, limit < min(n, span)


def check(ctx, rec, limit, want=None, form_b=True):
    """the device call against form A (or `want`) and form B; returns the order"""
    a = search.order_records(rec, limit) if want is None else want
    if form_b:
        assert a.tolist() == oo.order(rec, limit)
    order, cols = search.order_records_device(ctx, rec, limit, gather=True)
    assert order.dtype == np.int64 and len(order) == len(a)
    assert np.array_equal(order, a)
    host = hits.record_columns(rec, a)
    for f, dt in COLS:
        assert cols[f].dtype == dt and np.array_equal(cols[f], host[f]), f
    assert np.array_equal(search.order_records_device(ctx, rec, limit), a)     # without gathering
    return order


@pytest.mark.parametrize("name", sorted(oc.HAND_BUILT))
def test_hand_built_cases_equal_both_forms(ctx, name):
    rec, limits = oc.HAND_BUILT[name]()
    for limit, n_kept in limits:
        assert len(check(ctx, rec, limit)) == n_kept, limit


def test_the_extreme_set_at_limit_one(ctx):
    rec, _ = oc.extreme()
    assert check(ctx, rec, 1).tolist() == oc.EXTREME_ORDER_AT_1


@pytest.mark.parametrize("kind", ["ungapped", "gapped"])
def test_the_input_order_does_not_matter(ctx, kind):
    rows = oc.distinct_records()
    for perm in (np.arange(len(rows)), np.arange(len(rows))[::-1], np.random.RandomState(3).permutation(len(rows))):
        rec = oc.permuted(oc.ungapped(rows), perm)
        for limit in (1, 2, 10000):
            check(ctx, oc.gapped_form(rec) if kind == "gapped" else rec, limit)


def shapes(n, seed, gapped):
    """name -> records: many tiny contigs; one contig with everything; contigs of about 200
    records with more subjects than the default limit."""
    return {"tiny": oc.random_set(seed, n, n // 3 + 1, 40, gapped),
            "one": oc.random_set(seed + 1, n, 1, 300, gapped),
            "families": oc.random_set(seed + 2, n, n // 200 + 1, 20000, gapped, spread=2)}


@pytest.mark.parametrize("n", SIZES)
def test_random_sets(ctx, n):
    seen = set()
    for gapped in (False, True):
        for name, rec in shapes(n, 1000 + n, gapped).items():
            for limit in (1, 3, 10000):
                seen.add(route(rec, limit)[1])
                order = check(ctx, rec, limit, form_b=n <= 4097 or limit == 3)
                assert limit < 10000 or len(order) == n     # no contig has 10000 subjects
    assert seen == {True, False}                             # ranked (limits 1, 3) and not (tiny at 10000)


def wide(seed, n, gapped, level):
    """Records whose fields take few values that lie far apart, so that the key needs 2 (level 0),
    3 or 4 words while pairs and records still tie."""
    rng = np.random.RandomState(seed)
    far = [2 ** 20, 2 ** 31 - 1][min(level, 1)]
    pick = lambda vals: np.array(vals, np.int64)[rng.randint(0, len(vals), n)]
    rec = dict(contig=pick([0, 1, far // 2, far]), subject=pick([0, 3, far - 1, far]), minus=rng.randint(0, 2, n),
               qstart=pick([0, 5, far // 3]), sstart=pick([0, 7, far]) if level else pick([0, 7]),
               length=pick([40, 2 ** 30 if level else 2 ** 12]), matches=pick([0, 30, 40]))
    if gapped:
        rec.update(qspan=pick([40, far]), sspan=pick([1, 39, far]), gaps=pick([0, 2]))
    fields = search.GAP_RECORD_FIELDS if gapped else search.RECORD_FIELDS
    return {f: rec[f].astype(dt) for f, dt in fields}


def test_every_key_width(ctx):
    seen = set()
    sets = [oc.random_set(1, 300, 5, 9), wide(2, 300, False, 0), wide(3, 300, False, 1), wide(4, 300, True, 1),
            wide(5, 4097, True, 1), wide(6, 257, True, 0)]
    for rec in sets:
        for limit in (1, 2, 10000):
            seen.add(route(rec, limit)[0])
            check(ctx, rec, limit)
    assert seen == {1, 2, 3, 4}


@pytest.fixture(scope="module")
def big():
    """2^20 + 1 gapped records in contigs of about 210, subjects from 30000 with heavy ties, at a
    limit that binds in every contig; both CPU forms once."""
    rec = oc.random_set(77, BIG_N, BIG_N // 210, 30000, True, spread=2)
    limit = 150
    a = search.order_records(rec, limit)
    assert a.tolist() == oo.order(rec, limit)
    assert route(rec, limit) == (1, True) and 0 < len(a) < BIG_N
    return rec, limit, a


def test_a_large_call_then_small_ones_on_one_context(ctx, big):
    rec, limit, a = big
    check(ctx, rec, limit, want=a, form_b=False)
    small = oc.random_set(8, 5, 2, 3)
    check(ctx, small, 1)
    mid = oc.random_set(9, 4097, 30, 50, True)
    first = check(ctx, mid, 3)
    assert np.array_equal(first, check(ctx, mid, 3))          # twice in a row
    check(ctx, rec, limit, want=a, form_b=False)              # and the large one again


# ---- refusals ---------------------------------------------------------------------------------

def raw_call(ctx, rec, limit, out, n=None, null_in=(), null_struct=None):
    held = {f: np.ascontiguousarray(a) for f, a in rec.items()}
    a = lib.WfOrderIn(n=len(held["contig"]) if n is None else n, max_target_seqs=limit,
                      **{f: lib.ptr(held[f]) if f in held and f not in null_in else None
                         for f, _ in search.GAP_RECORD_FIELDS})
    o = lib.WfOrderOut(n_kept=SENTINEL, **{f: lib.ptr(v) for f, v in out.items()})
    rc = ctx.so.wf_order_records(ctx.h, None if null_struct == "in" else C.byref(a),
                                 None if null_struct == "out" else C.byref(o))
    return rc, int(o.n_kept), ctx.so.wf_last_error(ctx.h).decode()


def changed(rec, field, at, value):
    out = {f: a.copy() for f, a in rec.items()}
    out[field][at] = value
    return out


def refusals():
    g = oc.random_set(21, 100, 4, 6, True)
    u = oc.random_set(22, 100, 4, 6, False)
    some = dict(u, qspan=g["qspan"])
    two = dict(u, qspan=g["qspan"], sspan=g["sspan"])
    return [("null records", u, {"null_struct": "in"}, None), ("null out", u, {"null_struct": "out"}, None),
            ("null contig column", u, {"null_in": ("contig",)}, None),
            ("null matches column", g, {"null_in": ("matches",)}, None),
            ("null order", u, {"no_order": True}, None),
            ("negative n", u, {"n": -1}, None), ("n of 2^31", u, {"n": 2 ** 31}, None),
            ("limit 0", u, {"limit": 0}, None), ("limit negative", g, {"limit": -5}, None),
            ("negative contig", changed(u, "contig", 37, -1), {}, "record 37"),
            ("negative subject", changed(g, "subject", 99, -2 ** 31), {}, "record 99"),
            ("minus above 1", changed(u, "minus", 0, 2), {}, "record 0"),
            ("first of two bad records", changed(changed(u, "minus", 60, 9), "contig", 12, -3), {}, "record 12"),
            ("only qspan", some, {}, None), ("qspan and sspan without gaps", two, {}, None),
            ("gaps alone", dict(u, gaps=g["gaps"]), {}, None)]


@pytest.mark.parametrize("what,rec,how,names", refusals(), ids=[r[0].replace(" ", "_") for r in refusals()])
def test_refusals_leave_the_outputs_and_the_context(ctx, what, rec, how, names):
    how = dict(how)
    n = len(rec["contig"])
    out = {"order": np.full(n, SENTINEL, np.int64)}
    out.update({f: np.full(n, 256 + SENTINEL, dt) for f, dt in COLS})
    before = {f: a.copy() for f, a in out.items()}
    if how.pop("no_order", False):
        del out["order"]
    rc, n_kept, msg = raw_call(ctx, rec, how.pop("limit", 3), out, **how)
    assert rc == lib.WF_E_BADINPUT, what
    assert n_kept == SENTINEL
    for f, a in out.items():
        assert np.array_equal(a, before[f]), f
    if names:
        assert names in msg and "record 60" not in msg       # the first offending record is named
    nxt = oc.random_set(23, 300, 7, 12, True)
    check(ctx, nxt, 2)


def test_empty_input(ctx):
    for rec in (oc.ungapped([]), oc.gapped([])):
        out = {"order": np.full(1, SENTINEL, np.int64)}
        rc, n_kept, _ = raw_call(ctx, rec, 1, out)
        assert rc == lib.WF_OK and n_kept == 0 and out["order"][0] == SENTINEL
        order, cols = search.order_records_device(ctx, rec, 10000, gather=True)
        assert len(order) == 0 and all(len(cols[f]) == 0 for f, _ in COLS)
    # null columns are fine without records
    a = lib.WfOrderIn(n=0, max_target_seqs=1)
    o = lib.WfOrderOut(n_kept=SENTINEL)
    assert ctx.so.wf_order_records(ctx.h, C.byref(a), C.byref(o)) == lib.WF_OK and o.n_kept == 0


# ---- a real search's records ------------------------------------------------------------------

@pytest.fixture(scope="module")
def medium_records():
    contigs, subjects, P = sc.medium()
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        plain = s.search(*sc.flat(subjects))
        gapped = s.search_gapped(*sc.flat(subjects))
    qlen = np.array([len(c) for c in contigs], np.int64)
    slen = np.array([len(g) for g in subjects], np.int64)
    return {"ungapped": plain, "gapped": gapped}, qlen, slen


@pytest.mark.parametrize("kind", ["ungapped", "gapped"])
def test_medium_search_records(ctx, medium_records, kind):
    recs, qlen, slen = medium_records
    rec = recs[kind]
    assert len(rec["contig"]) > 200
    kept = []
    taxon = (np.arange(len(slen)) % 11).astype(np.int32)
    sysmask = (np.arange(len(slen)) % 4).astype(np.uint32)
    for limit in (1, 3, 10000):
        order = check(ctx, rec, limit)
        kept.append(len(order))
        _, cols = search.order_records_device(ctx, rec, limit, gather=True)
        got = hits.hits_host(ctx.so, ctx.h, cols, qlen, slen, taxon, sysmask, 0.75)
        want = hits.hits_host(ctx.so, ctx.h, hits.record_columns(rec, search.order_records(rec, limit)), qlen, slen,
                              taxon, sysmask, 0.75)
        for f, _ in hits.HIT_FIELDS:
            assert got[f].tobytes() == want[f].tobytes(), f
    assert kept[0] < kept[1] < kept[2] == len(rec["contig"])


# ---- the command lines ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("order")
    contigs, subjects, paths = _sample(tmp)
    wfdb = str(tmp / "genes.wfdb")
    makedb.main([paths[4], "--out", wfdb])
    return paths, {"fasta": paths[4], "wfdb": wfdb}


@pytest.mark.parametrize("flags", [[], ["--gapped"], ["--max-target-seqs", "1"]], ids=["plain", "gapped", "limit_1"])
def test_search_order_on_device_writes_the_same_table(sample, tmp_path, flags):
    paths, dbs = sample
    tables = []
    for where in ("host", "device"):
        out = str(tmp_path / (where + ".blastout"))
        search.main([paths[0], dbs["fasta"], "--searcher", "native", "--out", out, "--chunk-bases", "1200",
                     "--order-on", where] + flags)
        tables.append(open(out, "rb").read())
    assert tables[0] == tables[1] and tables[0].count(b"\n") >= (3 if "--max-target-seqs" in flags else 12)


@pytest.mark.parametrize("form", ["fasta", "wfdb"])
def test_workflow_order_on_device_writes_the_same_files(sample, tmp_path, form):
    paths, dbs = sample
    got = []
    for where in ("host", "device"):
        d = tmp_path / where
        d.mkdir()
        table, calls = str(d / "w.blastout"), str(d / "w.gff")
        workflow.main([paths[0], dbs[form], paths[3], "--outdir", str(d), "--basename", "w", "--quiet",
                       "--write-blastout", table, "--write-gff", calls, "--order-on", where])
        files = {k: open(str(d / "w.{}.tsv".format(k)), "rb").read() for k in ("lgt", "no_lgt", "unclassified")}
        files.update(table=open(table, "rb").read(), calls=open(calls, "rb").read())
        got.append(files)
    assert got[0] == got[1]
    assert got[0]["table"].count(b"\n") >= 12 and got[0]["calls"].count(b"\n") >= 6
