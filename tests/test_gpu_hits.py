"""wf_hits_from_records (wf_hits.hip) on the GPU against the two CPU forms of DESIGN.md §13
(tests/hits_oracle.py): the nine arrays must be equal bit for bit, doubles compared as int64.
The hand-built cases in both residencies, every (matches, length) up to 1024 and every matches at
the lengths where the shortcuts fail, calls of different sizes in a row, every refusal, and the
device arrays handed straight to wf_genecall and wf_score against the host batch read from the
written table."""
import ctypes as C

import numpy as np
import pytest

import hits_cases as hc
import hits_oracle as ho
import search_cases as sc
import search_gap_cases as gc
from test_gpu_search import _sample
from waafle_amd import cli, engine, genecaller, hits, inputs, lib, output, search
from waafle_amd.taxonomy import TaxonomyTables, read_edges

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    so = lib.load()
    h = C.c_void_p()
    assert so.wf_init(0, C.byref(h)) == lib.WF_OK
    yield so, h
    so.wf_free(h)


def tables(case):
    """the product's own tables of a case: qlen, slen, taxon ids, sysmask"""
    used = np.unique(np.asarray(case["cols"]["subject"], np.int64))
    st = hits.subject_tables(case["subject_ids"], used)
    tax = TaxonomyTables(case["edges"], extra_names={t for t in st.taxa if t is not None})
    return case["qlen"], case["slen"], st.taxon_ids(tax), st.sysmask


def columns(case):
    return {f: np.asarray(case["cols"][f], dt) for f, dt in hits.RECORD_COLUMNS}


def run(ctx, case, resident):
    so, h = ctx
    cols, tabs = columns(case), tables(case)
    if not resident:
        return hits.hits_host(so, h, cols, *tabs, case["min_scov"])
    d = hits.hits_device(so, h, cols, *tabs, case["min_scov"], hits.hip_runtime(0))
    return hits.to_host(d, len(cols["contig"]), len(case["qlen"]))


@pytest.mark.parametrize("resident", [0, 1])
@pytest.mark.parametrize("name", sorted(hc.HAND_BUILT))
def test_hand_built_cases_equal_both_forms(ctx, name, resident):
    case = hc.HAND_BUILT[name]()
    got = run(ctx, case, resident)
    ho.assert_same(got, ho.form_a(case), name + " A")
    ho.assert_same(got, ho.form_b(case), name + " B")
    assert got["hit_off"].tolist() == case["hit_off"]


@pytest.mark.parametrize("lengths", [range(1, 1025), (1600, 8000, 16000, 40000, 200000)], ids=["to_1024", "long"])
def test_every_matches_value(ctx, lengths):
    case = hc.sweep(lengths)
    assert len(case["cols"]["length"]) == sum(v + 1 for v in lengths)
    a, b = ho.form_a(case), ho.form_b(case)
    ho.assert_same(a, b, "forms")
    ho.assert_same(run(ctx, case, 0), a, "host arrays")
    ho.assert_same(run(ctx, case, 1), b, "device arrays")


def test_calls_of_different_sizes_in_a_row(ctx):
    big, small = hc.sized(257), hc.trims()
    want_big, want_small = ho.form_b(big), ho.form_b(small)
    for resident in (0, 1):
        ho.assert_same(run(ctx, big, resident), want_big)
        ho.assert_same(run(ctx, big, resident), want_big)
        ho.assert_same(run(ctx, small, resident), want_small)
        ho.assert_same(run(ctx, hc.empty(), resident), ho.form_b(hc.empty()))
        ho.assert_same(run(ctx, big, resident), want_big)


def refusals():
    """(what, change of the good case's columns / tables / arguments) per WF_E_BADINPUT condition"""
    def col(f, i, v):
        return lambda cols, tabs: cols[f].__setitem__(i, v)

    def tab(k, i, v):
        return lambda cols, tabs: tabs[k].__setitem__(i, v)

    return [("contig above its table", col("contig", 2, 2)), ("contig negative", col("contig", 0, -1)),
            ("subject above its table", col("subject", 1, 5)), ("subject negative", col("subject", 1, -1)),
            ("contig column decreases", col("contig", 2, 0)), ("minus above 1", col("minus", 0, 2)),
            ("length 0", col("length", 0, 0)), ("length negative", col("length", 2, -5)),
            ("matches negative", col("matches", 1, -1)), ("matches above length", col("matches", 1, 201)),
            ("qspan 0", col("qspan", 0, 0)), ("sspan negative", col("sspan", 2, -1)),
            ("qlen 0", tab(0, 1, 0)), ("slen negative", tab(1, 0, -3)),
            ("denominator 0", col("sstart", 1, 1100)),     # ltrim = 1000 = slen
            ("qhi outside int32", col("qstart", 0, 2 ** 31 - 100)),
            ("taxon 2^24", tab(2, 2, 1 << 24)), ("taxon negative", tab(2, 0, -1))]


@pytest.mark.parametrize("what,change", refusals(), ids=[w.replace(" ", "_") for w, _ in refusals()])
def test_refusals_leave_the_outputs_and_the_context(ctx, what, change):
    so, h = ctx
    case = hc.trims()
    want = ho.form_b(case)
    cols = columns(case)
    tabs = [np.array(t).copy() for t in tables(case)]
    change(cols, tabs)
    n, N = len(cols["contig"]), len(tabs[0])
    out = {f: np.full(N + 1 if f == "hit_off" else n, 77, dt) for f, dt in hits.HIT_FIELDS}
    with pytest.raises(lib.WaafleHipError) as exc:
        hits.hits_host(so, h, cols, *tabs, case["min_scov"], out=out)
    assert exc.value.code == lib.WF_E_BADINPUT and exc.value.msg, what
    assert all((a == 77).all() for a in out.values()), what
    ho.assert_same(run(ctx, case, 0), want, "after " + what)


def test_null_arrays_and_empty_inputs(ctx):
    so, h = ctx
    case = hc.trims()
    cols, tabs = columns(case), [np.ascontiguousarray(t, dt) for t, dt in
                                 zip(tables(case), (np.int64, np.int64, np.int32, np.uint32))]
    n, N = 3, 2
    out = {f: np.full(N + 1 if f == "hit_off" else n, 77, dt) for f, dt in hits.HIT_FIELDS}
    held = [cols[f] for f, _ in hits.RECORD_COLUMNS]

    def call(rec_ptrs, tab_ptrs, out_ptrs, n=n):
        r = lib.WfHitRecords(n, *rec_ptrs)
        t = lib.WfHitTables(N, len(tabs[1]), *tab_ptrs, 0.75)
        o = lib.WfHitsOut(0, 0, *out_ptrs)
        return so.wf_hits_from_records(h, C.byref(r), C.byref(t), C.byref(o))

    recs, tp, op = [lib.ptr(a) for a in held], [lib.ptr(a) for a in tabs], [lib.ptr(out[f]) for f, _ in hits.HIT_FIELDS]
    for k in range(len(recs)):
        assert call(recs[:k] + [None] + recs[k + 1:], tp, op) == lib.WF_E_BADINPUT
    for k in range(len(tp)):
        assert call(recs, tp[:k] + [None] + tp[k + 1:], op) == lib.WF_E_BADINPUT
    for k in range(len(op)):
        assert call(recs, tp, op[:k] + [None] + op[k + 1:]) == lib.WF_E_BADINPUT
        assert so.wf_last_error(h)
    assert call(recs, tp, op, n=-1) == lib.WF_E_BADINPUT
    assert so.wf_hits_from_records(h, None, None, None) == lib.WF_E_BADINPUT
    assert all((a == 77).all() for a in out.values())
    # n = 0 needs hit_off alone, and n_contigs = 0 is valid too
    assert call([None] * 9, [None] * 4, op[:1] + [None] * 8, n=0) == lib.WF_OK
    assert out["hit_off"].tolist() == [0, 0, 0] and (out["hit_qlo"] == 77).all()
    r, t = lib.WfHitRecords(0), lib.WfHitTables(0, 0, None, None, None, None, 0.75)
    off = np.full(1, 77, np.int64)
    assert so.wf_hits_from_records(h, C.byref(r), C.byref(t), C.byref(lib.WfHitsOut(0, 0, lib.ptr(off)))) == lib.WF_OK
    assert off.tolist() == [0]
    assert call(recs, tp, op) == lib.WF_OK
    ho.assert_same(out, ho.form_b(case), "after the refusals")


# ---------------------------------------------------------------------------
# the device arrays straight into wf_genecall and wf_score
# ---------------------------------------------------------------------------

def _device_against_table(tmp_path, contigs, subjects, paths, gapped, flags=(), too_big=False):
    """The records of one search through the device arrays to gene calls and results, and the
    same through the written table: load_inputs, call_genes_arrays and engine.score.  too_big:
    the scorer takes the staged form with an attachment limit that holds one contig and not the
    batch, so the device call is refused (WF_E_TOOBIG) and score_device falls back to the host
    batch, which GpuScorer.score halves."""
    names, ids = [n for n, _ in contigs], [n for n, _ in subjects]
    with search.Searcher(*sc.flat([s for _, s in contigs])) as s:
        rec = (s.search_gapped if gapped else s.search)(*sc.flat([s for _, s in subjects]))
    order = search.order_records(rec)
    qlen, slen = [len(s) for _, s in contigs], [len(s) for _, s in subjects]
    with open(paths[1], "w") as fh:
        fh.write("".join(r + "\n" for r in search.format_rows(rec, order, names, qlen, ids, slen, sum(slen))))
    args = cli.parse_flags(list(flags))
    params = cli.param_dict(args)
    host, tax = inputs.load_inputs(*paths[:4], args.min_gene_length, warn=None)
    assert host.n_hits == len(order) >= 2
    cols = hits.record_columns(rec, order)
    st = hits.subject_tables(ids, np.unique(cols["subject"]))
    tax2 = TaxonomyTables(read_edges(paths[3]), extra_names={t for t in st.taxa if t is not None})
    assert tax2.names == tax.names
    limit = host.max_hits * host.max_loci                    # room for any one contig, not for all three
    scorer = engine.GpuScorer(0, mode="staged", options={lib.OPT_ATT_LIMIT: limit}) if too_big else engine.GpuScorer(0)
    host_calls, score = [], scorer.score
    scorer.score = lambda b, p: (host_calls.append(b.n_contigs), score(b, p))[1]
    try:
        scorer.set_taxonomy(tax2)
        d = hits.hits_device(scorer.lib, scorer.h, cols, qlen, slen, st.taxon_ids(tax2), st.sysmask, args.min_scov,
                             hits.hip_runtime(0))
        got = hits.to_host(d, len(order), len(names))
        for f, _ in hits.HIT_FIELDS[:-1]:
            assert (ho.bits(got[f]) == ho.bits(getattr(host, f))).all(), f
        assert (got["hit_key"] == engine.hit_keys(host, args.min_scov)).all()
        calls = hits.genecall_device(scorer.lib, scorer.h, d, len(names), len(order), args.min_overlap,
                                     args.min_scov, args.min_gene_length)
        want = genecaller.call_genes_arrays(host.hit_off, host.hit_qlo, host.hit_qhi, host.hit_strand, host.hit_scov,
                                            args.min_overlap, args.min_gene_length, args.min_scov)
        genes = hits.gene_lists(got["hit_off"], *calls)
        assert genes == hits.gene_lists(host.hit_off, *want) and sum(len(gl) for _, gl in genes) >= 1
        loci = inputs.read_loci(paths[2], {n: i for i, n in enumerate(names)}, args.min_gene_length, warn=None)
        batch = hits.make_batch(names, qlen, got["hit_off"], loci, st, cols["subject"])
        assert batch.loc_off.tolist() == host.loc_off.tolist() and batch.loc_start.tolist() == host.loc_start.tolist()
        res = hits.score_device(scorer, batch, d, params)
        assert (host_calls[:1] == [len(names)] and len(host_calls) >= 3) if too_big else not host_calls
    finally:
        scorer.close()
    ref = engine.score(host, tax, params)
    for f in ("call", "crit", "rank", "clade1", "clade2", "direction", "iterations", "synteny", "n_meld1", "n_meld2",
              "annot_hit", "status"):
        assert (ho.bits(getattr(res, f)) == ho.bits(getattr(ref, f))).all(), f
    assert output.render(batch, tax2, res) == output.render(host, tax, ref)
    return res


def test_device_arrays_into_genecall_and_score_sample(tmp_path):
    contigs, subjects, paths = _sample(tmp_path)
    res = _device_against_table(tmp_path, contigs, subjects, paths, gapped=False)
    assert (res.call != lib.CALL_UNCLASSIFIED).any()


def test_too_big_for_one_call_falls_back_to_the_host_batch(tmp_path):
    contigs, subjects, paths = _sample(tmp_path)
    _device_against_table(tmp_path, contigs, subjects, paths, gapped=False, too_big=True)


def test_device_arrays_into_genecall_and_score_planted_gapped(tmp_path):
    cs, ss, P = gc.planted()
    contigs = [("p{}".format(i), s) for i, s in enumerate(cs)]
    subjects = [("h{}|s__{}|UniProt=X{}".format(i, "AB"[i % 2], i), s) for i, s in enumerate(ss)]
    paths = [str(tmp_path / n) for n in ("p.fna", "p.blastout", "p.gff", "p.tsv")]
    with open(paths[0], "w") as fh:
        fh.write("".join(">{}\n{}\n".format(n, s) for n, s in contigs))
    with open(paths[2], "w") as fh:
        fh.write("\t".join(["p0", "x", "gene", "501", "1500", ".", "+", "0", "."]) + "\n")
    with open(paths[3], "w") as fh:
        fh.write("s__A\tg__G\ns__B\tg__G\ng__G\tr__Root\n")
    _device_against_table(tmp_path, contigs, subjects, paths, gapped=True)
