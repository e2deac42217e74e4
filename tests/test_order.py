"""The rule of the table's order and --max-target-seqs pinned on the CPU:
search.order_records (form A) against the plain-Python form B of tests/order_oracle.py, on the
hand-built cases with their stated counts and on seeded random sets; and what the binding and
the command lines of the device form need without a GPU."""
import os

import numpy as np
import pytest

import order_cases as oc
import order_oracle as oo
from waafle_amd import hits, lib, search, workflow

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(oc.HAND_BUILT))
def test_hand_built_cases_both_forms(name):
    rec, limits = oc.HAND_BUILT[name]()
    for limit, n_kept in limits:
        a = search.order_records(rec, limit)
        assert a.dtype == np.int64
        assert a.tolist() == oo.order(rec, limit), (name, limit)
        assert len(a) == n_kept, (name, limit)
        cols = hits.record_columns(rec, a)
        assert {f: c.tolist() for f, c in cols.items()} == oo.columns(rec, a.tolist())


def test_the_extreme_set_at_limit_one():
    rec, _ = oc.extreme()
    assert search.order_records(rec, 1).tolist() == oc.EXTREME_ORDER_AT_1 == oo.order(rec, 1)
    assert oo.scores(rec) == [2 ** 30, -2 ** 31, 2 ** 30]
    assert search.score_of(rec).tolist() == oo.scores(rec)


def test_seeded_random_sets_both_forms():
    kept = total = 0
    for rec, limit in oc.small_random_sets():
        a = search.order_records(rec, limit).tolist()
        assert a == oo.order(rec, limit)
        kept, total = kept + len(a), total + len(rec["contig"])
    assert 0 < kept < total                                  # the limits dropped some, not all


@pytest.mark.parametrize("kind", ["ungapped", "gapped"])
def test_the_input_order_does_not_matter(kind):
    rows = oc.distinct_records()
    rng = np.random.RandomState(3)
    tables = []
    for perm in (np.arange(len(rows)), np.arange(len(rows))[::-1], rng.permutation(len(rows))):
        rec = oc.permuted(oc.ungapped(rows), perm)
        rec = oc.gapped_form(rec) if kind == "gapped" else rec
        for limit in (1, 2, 10000):
            a = search.order_records(rec, limit)
            assert a.tolist() == oo.order(rec, limit)
            tables.append((limit, [tuple(int(rec[f][i]) for f in rec) for i in a]))
    for limit in (1, 2, 10000):
        same = [t for k, t in tables if k == limit]
        assert same[0] == same[1] == same[2] and len(same[0]) > 0


def test_binding_and_header():
    header = open(os.path.join(REPO, "include", "waafle_hip.h")).read()
    assert "int wf_order_records(wf_ctx* ctx, const wf_order_in* in, wf_order_out* out);" in header
    assert "still 6 (additive): wf_order_records" in header and lib.ABI_VERSION == 6
    res, args = lib.SIGNATURES["wf_order_records"]
    assert len(args) == 3
    body = header.split("typedef struct wf_order_in {")[1].split("} wf_order_in;")[0]
    assert [f for f, _ in lib.WfOrderIn._fields_] == [
        ln.split(";")[0].split()[-1].lstrip("*") for ln in body.splitlines() if ";" in ln.split("/*")[0]]
    body = header.split("typedef struct wf_order_out {")[1].split("} wf_order_out;")[0]
    assert [f for f, _ in lib.WfOrderOut._fields_] == [
        ln.split(";")[0].split()[-1].lstrip("*") for ln in body.splitlines() if ";" in ln.split("/*")[0]]
    assert [f for f, _ in search.ORDER_COLUMNS] == [f for f, _ in hits.RECORD_COLUMNS]


def test_order_on_flag_of_both_commands():
    for ap in (search.build_parser(), workflow.build_parser()):
        group = next(g for g in ap._action_groups if g.title.startswith("native search"))
        act = next(a for a in group._group_actions if "--order-on" in a.option_strings)
        assert act.default == "host" and list(act.choices) == ["host", "device"]
    args = workflow.build_parser().parse_args(["c.fna", "g.wfdb", "t.tsv", "--order-on", "device"])
    assert args.order_on == "device"


def test_no_device_memory_falls_back_to_the_host():
    class NoRoom:
        so = h = None

    def refuse(ctx, rec, limit, gather=False):
        raise lib.WaafleHipError(lib.WF_E_NOMEM, "no device memory")

    rec, _ = oc.one_contig()
    said, real = [], search.order_records_device
    search.order_records_device = refuse
    try:
        order, cols = search.order_with(NoRoom(), rec, 2, "device", gather=True, say=lambda *a: said.append(a))
    finally:
        search.order_records_device = real
    assert order.tolist() == oo.order(rec, 2) and len(said) == 1 and "host" in said[0][0]
    assert {f: c.tolist() for f, c in cols.items()} == oo.columns(rec, order.tolist())
