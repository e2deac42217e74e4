"""GPU parity: the HIP path (through the C-ABI) against the oracle and the goldens.

Bar: bit-exact for every integer/index/string field and for the float64 crit/rank
(the kernels follow numpy's summation order), TSV bytes identical to the reference
goldens except tie-flagged contigs (output must be one of the reference's outcomes).
"""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import golden_cases as gc
from oracle_bridge import (oracle_hits_from_batch, oracle_loci_from_batch, oracle_results,
                           run_oracle)
from oracle import orgscorer_oracle as orc
from waafle_amd import cli, engine, inputs, lib, output, synth

pytestmark = pytest.mark.gpu

CASES = gc.case_names()
FIELDS = ("call", "crit", "rank", "clade1", "clade2", "direction", "synteny", "n_meld1",
          "n_meld2", "annot_hit", "pair_evals", "ppot_sum", "iterations", "status")


FORMS = {
    # (default) explain_two and the roll-up levels in the first wave form's hand-over
    "level0": dict(mode="level0"),
    # the same without the level-0 triage (wf_triage.hip): the wave form runs every contig
    "notriage": dict(mode="level0", options={lib.OPT_TRIAGE: 0}),
    # a hand-over buffer of 96 entries: the contigs past it take the staged kernels; the
    # caller's packed hit_key (numpy) instead of the library's (k_pack_keys)
    "dumpcap": dict(mode="level0", options={lib.OPT_DUMP_CAP: 96}, host_keys=True),
    "waves": dict(mode="waves"),
    "staged": dict(mode="staged"),
    # every staged decision from the segment table (k_big_sparse, wf_sparse.h)
    "sparse": dict(mode="staged", options={lib.OPT_SPARSE_BIG: 2}),
    # a 4 KB dense arena: the > 63-loci decisions that outgrow it in an HBM slot (k_decide_big)
    "small_arena": dict(mode="staged", lds_bytes=4096),
}


@pytest.fixture(scope="module", params=list(FORMS))
def scorer(request):
    """Every execution form: the level-0 wave kernels with the staged kernels behind them
    (default), the wave kernels carrying the roll-up levels too, every contig through the
    staged kernels, and those with every decision in the segment-table form or in the
    dense HBM-slot form."""
    s = engine.GpuScorer(0, **FORMS[request.param])
    s.form = request.param
    yield s
    s.close()


# The oracle's results per case, computed once for all forms (the CPU oracle, not the GPU,
# is most of this module's time): case key -> Results
_ORACLE = {}


def oracle_for(key, paths, flags, batch, tax):
    if key not in _ORACLE:
        contigs, _ = run_oracle(paths, list(flags))
        _ORACLE[key] = oracle_results(contigs, batch, tax)
    return _ORACLE[key]


def gpu_score(scorer, batch, tax, flags):
    scorer.set_taxonomy(tax)
    return scorer.score(batch, cli.param_dict(cli.parse_flags(flags)))


def meld_sets(res, batch, c):
    base = 2 * int(batch.hit_off[c]) + 2 * c
    n1, n2 = int(res.n_meld1[c]), int(res.n_meld2[c])
    return (sorted(res.meld[base:base + n1].tolist()),
            sorted(res.meld[base + n1:base + n1 + n2].tolist()))


def assert_same_results(got, want, batch, skip=()):
    bad = []
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        if f in ("crit", "rank"):
            a, b = a.view(np.int64), b.view(np.int64)
        if f == "clade2":   # only meaningful for lgt rows
            a = np.where(got.call == 2, a, -1)
            b = np.where(want.call == 2, b, -1)
        if f in ("synteny",):
            keep = np.repeat(want.call != 0, np.diff(batch.loc_off))
            a, b = a[keep], b[keep]
        if f == "iterations":
            keep = want.call != 0
            a, b = a[keep], b[keep]
        diff = np.nonzero(a != b)[0]
        if len(diff):
            bad.append((f, diff[:5].tolist()))
    for c in range(batch.n_contigs):
        if c in skip:
            continue
        if meld_sets(got, batch, c) != meld_sets(want, batch, c):
            bad.append(("meld", c))
            break
    assert bad == []


def assert_matches_dump(fx, batch, res):
    """crit/rank bit-exact against the reference's own decision dump (float64 hex of the
    reported option, sorted-iteration run) -- no oracle involved."""
    bad = []
    for c, name in enumerate(batch.contig_names):
        if name in fx["ties"]:
            continue
        rec = fx["dump"].get(name, {})
        call = int(res.call[c])
        tag = {lib.CALL_NO_LGT: "one", lib.CALL_LGT: "two"}.get(call)
        if tag is None:
            if any(rec.get(t) and rec[t][0] for t in ("one", "two")):
                bad.append((name, "unclassified here, OK upstream"))
            continue
        want = rec.get(tag)
        got = [float(res.crit[c]).hex(), float(res.rank[c]).hex()]
        if want is None or not want[0] or want[1:3] != got:
            bad.append((name, tag, want, got))
    assert bad == []


@pytest.mark.parametrize("name", CASES)
def test_gpu_matches_goldens_and_oracle(name, scorer, tmp_path):
    fx = gc.load(name)
    paths = gc.materialize(fx, tmp_path)
    args = cli.parse_flags(fx["flags"])
    batch, tax = inputs.load_inputs(*paths, args.min_gene_length, warn=None)
    res = gpu_score(scorer, batch, tax, fx["flags"])
    rows = output.render(batch, tax, res)
    texts = {k: "\n".join(v) + "\n" for k, v in rows.items()}
    assert gc.compare_tsv(fx, texts) == []
    assert_matches_dump(fx, batch, res)
    if name in gc.HEAVY:       # cfg5 stress: the fixture is the only reference
        return
    want = oracle_for(("golden", name), paths, fx["flags"], batch, tax)
    assert_same_results(res, want, batch)


@pytest.mark.parametrize("name", gc.runaway_names())
def test_gpu_deep_taxonomy_and_runaway(name, scorer, tmp_path):
    """Roll-up depth past the 16-level lineage table and the > 100 iteration guard
    (orgscorer.py:566-583): the reference's TSVs, or WF_E_RUNAWAY on the contig the
    reference dies on, and the CLI's die message (make_deep.py fixtures)."""
    fx = gc.load_runaway(name)
    paths = gc.materialize(fx, tmp_path)
    batch, tax = inputs.load_inputs(*paths, 200.0, warn=None)
    if fx["returncode"] == 0:
        res = gpu_score(scorer, batch, tax, fx["flags"])
        rows = output.render(batch, tax, res)
        assert {k: "\n".join(v) + "\n" for k, v in rows.items()} == fx["tsv"]
        return
    with pytest.raises(lib.WaafleHipError) as exc:
        gpu_score(scorer, batch, tax, fx["flags"])
    assert exc.value.code == lib.WF_E_RUNAWAY
    assert batch.contig_names[int(exc.value.contigs[0])] in fx["stderr"]
    if scorer.form != "level0":   # the CLI runs the default form: once
        return
    cmd = [sys.executable, "-m", "waafle_amd.orgscorer"] + paths + \
          ["--outdir", str(tmp_path), "--quiet"] + fx["flags"]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                         cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert run.returncode == fx["returncode"]
    want = fx["stderr"].strip().splitlines()[-2:]        # the die: LETHAL ERROR + EXITING.
    assert want[0].startswith("LETHAL ERROR:")
    assert run.stderr.strip().splitlines()[-2:] == want


_SYNTH = {}


def synth_case(tmp_path, flags=(), **kw):
    """(batch, taxonomy, oracle results) of a synthetic case, built once for all forms."""
    key = (tuple(sorted(kw.items())), tuple(flags))
    if key not in _SYNTH:
        data = synth.generate(**kw)
        paths = synth.write_text(data, str(tmp_path), "s")
        args = cli.parse_flags(list(flags))
        batch, tax = inputs.load_inputs(*paths, args.min_gene_length, warn=None)
        contigs, _ = run_oracle(paths, list(flags))
        _SYNTH[key] = (batch, tax, oracle_results(contigs, batch, tax))
    return _SYNTH[key]


@pytest.mark.parametrize("kw,flags", [
    (dict(n=1500, genes=8, clades=200, seed=21), []),
    (dict(n=600, genes=12, clades=1000, seed=31), ["-k1", "0.9"]),
    (dict(n=800, genes=5, clades=12, seed=41, decoys=4, lgt_frac=0.4), []),
    (dict(n=800, genes=5, clades=12, seed=42, decoys=4, lgt_frac=0.4),
     ["--weak-loci", "assign-unknown", "--disambiguate-two", "report-best"]),
    (dict(n=500, genes=7, clades=40, seed=43, decoys=6, short_frac=0.3),
     ["--min-overlap", "0", "--jump-taxonomy", "2"]),
    (dict(n=2, genes=20, clades=2500, seed=5, stress=True), []),
])
def test_gpu_matches_oracle_synthetic(kw, flags, scorer, tmp_path):
    batch, tax, want = synth_case(tmp_path, flags, **kw)
    got = gpu_score(scorer, batch, tax, flags)
    assert_same_results(got, want, batch)


def test_long_locus_uses_numpy_buffered_sum(scorer, tmp_path):
    """A 20 kb gene: the site mean crosses numpy's 8192-element reduction buffer."""
    fna = tmp_path / "x.fna"
    fna.write_text(">big\n" + "N" * 30000 + "\n")
    (tmp_path / "x.gff").write_text("big\tx\tgene\t101\t20100\t.\t+\t0\t.\n"
                                    "big\tx\tgene\t20201\t29900\t.\t-\t0\t.\n")
    rows = []
    for i, (qs, qe, pid, tx) in enumerate([(101, 15000, "91.237", "s__A"),
                                          (9000, 20100, "88.001", "s__A"),
                                          (300, 20000, "79.999", "s__B"),
                                          (20201, 29900, "95.5", "s__A"),
                                          (20201, 28000, "99.1", "s__B")]):
        L = qe - qs + 1
        rows.append("big\tG{}|{}|KO=K{}\t30000\t{}\t{}\t{}\t{}\t1\t{}\t{}\t{}\t0\t0.0\t9\tplus"
                    .format(i, tx, i, L, L, qs, qe, L, pid, L))
    (tmp_path / "x.blastout").write_text("\n".join(rows) + "\n")
    (tmp_path / "x.tsv").write_text("s__A\tg__G\ns__B\tg__G\ng__G\tr__Root\n")
    paths = [str(tmp_path / f) for f in ("x.fna", "x.blastout", "x.gff", "x.tsv")]
    for flags in ([], ["-k1", "0.95", "-k2", "0.9"]):
        batch, tax = inputs.load_inputs(*paths, 200.0, warn=None)
        got = gpu_score(scorer, batch, tax, flags)
        assert_same_results(got, oracle_for(("long_locus",) + tuple(flags), paths, flags, batch, tax), batch)


def test_empty_and_degenerate_contigs(scorer, tmp_path):
    fna = tmp_path / "e.fna"
    fna.write_text(">nohits\nNNNN\n>noloci\nNNNNNNNN\n>ok\n" + "N" * 2000 + "\n")
    (tmp_path / "e.gff").write_text("nohits\tx\tgene\t1\t300\t.\t+\t0\t.\n"
                                    "ok\tx\tgene\t1\t400\t.\t+\t0\t.\n"
                                    "ok\tx\tgene\t20\t80\t.\t+\t0\t.\n")
    (tmp_path / "e.blastout").write_text(
        "noloci\tG|s__A\t8\t8\t8\t1\t8\t1\t8\t99.0\t8\t0\t0.0\t9\tplus\n"
        "ok\tG|s__A\t2000\t400\t400\t1\t400\t1\t400\t99.0\t8\t0\t0.0\t9\tplus\n"
        "ok\tG|s__B\t2000\t400\t10\t1\t10\t1\t10\t99.0\t8\t0\t0.0\t9\tplus\n")
    (tmp_path / "e.tsv").write_text("s__A\tr__Root\n")
    paths = [str(tmp_path / f) for f in ("e.fna", "e.blastout", "e.gff", "e.tsv")]
    for flags in ([], ["--weak-loci", "assign-unknown"], ["--weak-loci", "penalize"]):
        batch, tax = inputs.load_inputs(*paths, 200.0, warn=None)
        got = gpu_score(scorer, batch, tax, flags)
        assert_same_results(got, oracle_for(("degenerate",) + tuple(flags), paths, flags, batch, tax), batch)


def _decline_case(tmp_path):
    """One contig, 16 loci of 300 sites, 240 species each with one full-length hit on one
    locus, two species per genus on the 120 distinct locus pairs, every genus under one
    family.  Level 0: 240 potential clades (the whole table: sp_level), 16 one-locus classes,
    no pair covers the contig -> raised.  Level 1: 120 genera with 120 distinct two-locus
    masks, past sp_level's class table (96 of 128 slots) -> the wave levels decline the
    contig after a raise.  Level 2: the family covers every locus -> explain_one."""
    import itertools
    pairs = list(itertools.combinations(range(16), 2))
    starts = [1 + 350 * g for g in range(16)]
    clen = starts[-1] + 400
    (tmp_path / "d.fna").write_text(">dec\n" + "N" * clen + "\n")
    (tmp_path / "d.gff").write_text("".join("dec\tx\tgene\t{}\t{}\t.\t+\t0\t.\n".format(s, s + 299)
                                            for s in starts))
    rows, tax = [], ["f__F\tr__Root"]
    for j, (a, b) in enumerate(pairs):
        tax.append("g__G{}\tf__F".format(j))
        for k, g in enumerate((a, b)):
            sp = "s__S{}_{}".format(j, k)
            tax.append("{}\tg__G{}".format(sp, j))
            rows.append("dec\tH{}_{}|{}|KO=K1\t{}\t300\t300\t{}\t{}\t1\t300\t99.{:03d}\t300\t0\t0.0\t9\tplus"
                        .format(j, k, sp, clen, starts[g], starts[g] + 299, (7 * j + k) % 1000))
    (tmp_path / "d.blastout").write_text("\n".join(rows) + "\n")
    (tmp_path / "d.tsv").write_text("\n".join(tax) + "\n")
    return [str(tmp_path / f) for f in ("d.fna", "d.blastout", "d.gff", "d.tsv")]


def test_wave_levels_decline_after_a_raise(scorer, tmp_path):
    """A contig the wave levels decline at roll-up level 1 (sp_level's class
    table outgrown after the level-0 raise) is rescored from level 0 by the staged kernels:
    the records equal the oracle's, no contig is left pending, and in the default form the
    staged phases ran (the early return after the levels did not fire)."""
    paths = _decline_case(tmp_path)
    batch, tax = inputs.load_inputs(*paths, 200.0, warn=None)
    assert batch.n_contigs == 1 and int(batch.hit_off[1]) == 240 and int(batch.loc_off[1]) == 16
    want = oracle_for(("decline",), paths, [], batch, tax)
    assert int(want.iterations[0]) == 3 and int(want.call[0]) == lib.CALL_NO_LGT
    tm = lib.WfTiming()
    scorer.lib.wf_timing_enable(scorer.h, 1)
    try:
        got = gpu_score(scorer, batch, tax, [])
        assert scorer.lib.wf_timing_read(scorer.h, C.byref(tm)) == 0
    finally:
        scorer.lib.wf_timing_enable(scorer.h, 0)
    assert_same_results(got, want, batch)
    assert int(got.status[0]) == 0
    if scorer.form == "level0":
        ph = tm.phases()
        assert ph["rollup"][1] > 0 and ph["attach"][1] > 0, ph


def test_attach_fixture_reaches_the_staged_attach(tmp_path):
    """The default `attach` fixture (make_attach.py) in the default form: its 513-hit contig is
    past every wave slice, so the counting kernel sends it to the staged kernels and their
    attach phase runs; the records equal the oracle's."""
    fx = gc.load("attach_default")
    paths = gc.materialize(fx, tmp_path)
    batch, tax = inputs.load_inputs(*paths, 200.0, warn=None)
    assert int(np.diff(batch.hit_off).max()) == 513
    s = engine.GpuScorer(0, **FORMS["level0"])
    tm = lib.WfTiming()
    s.lib.wf_timing_enable(s.h, 1)
    try:
        got = gpu_score(s, batch, tax, fx["flags"])
        assert s.lib.wf_timing_read(s.h, C.byref(tm)) == 0
    finally:
        s.close()
    assert_same_results(got, oracle_for(("golden", "attach_default"), paths, fx["flags"], batch, tax), batch)
    ph = tm.phases()
    assert ph["attach"][1] > 0 and ph["segments"][1] > 0, ph


def test_full_size_cfg2_properties():
    """BASELINE config 2 at full size: deterministic, shard-invariant, LDS-budget
    invariant (forcing the HBM-workspace kernel), equal across every execution form, and
    equal to the oracle on a sample.  (Not per form: it builds every form itself.)"""
    data = synth.generate_config("cfg2")
    batch, tax = synth.to_batch(data)
    params = cli.param_dict(cli.parse_flags([]))
    scorer = engine.GpuScorer(0)
    scorer.set_taxonomy(tax)
    a = scorer.score(batch, params)
    b = scorer.score(batch, params)
    assert_same_results(a, b, batch)
    for kw in (dict(lds_bytes=8192),          # small decision arena: HBM decision slots
               dict(mode="staged", options={lib.OPT_SPARSE_BIG: 2}),   # segment-table form
               dict(lds_bytes=65536),         # large arena: every contig in LDS
               dict(mode="staged"), dict(mode="level0"), dict(mode="waves"),
               dict(options={lib.OPT_DUMP_CAP: 4096}),   # hand-over buffer overflow
               dict()):
        small = engine.GpuScorer(0, **kw)
        small.set_taxonomy(tax)
        c = small.score(batch, params)
        small.close()
        assert_same_results(a, c, batch)
    bounds = engine.shard_bounds(engine.contig_cost(batch), 4)
    parts = [scorer.score(batch.slice(x, y), params) for x, y in bounds]
    d = engine.Results.concat(parts, [int(batch.hit_off[x]) for x, _ in bounds])
    assert_same_results(a, d, batch)
    assert (a.call == 2).sum() > 0 and (a.call == 1).sum() > 0
    # oracle on a 300-contig sample (contigs are independent)
    sub = batch.slice(5000, 5300)
    opar = orc.Params(**params)
    otax = orc.Taxonomy(data.tax.edges)
    hits = oracle_hits_from_batch(sub, tax)
    loci = oracle_loci_from_batch(sub)
    lengths = dict(zip(sub.contig_names, sub.contig_lengths.tolist()))
    contigs = orc.score_contigs(lengths, loci, hits, otax, opar)
    want = oracle_results(contigs, sub, tax)
    got = scorer.score(sub, params)
    scorer.close()
    assert_same_results(got, want, sub)


def test_concurrent_contexts_share_a_device():
    """Two and three contexts on device 0, each scoring its shard from its own host thread
    at the same time (engine.score's device map), equal the one-context result field by
    field.  Each context drains only its own stream before replacing scratch buffers."""
    data = synth.generate(n=3000, genes=8, clades=200, seed=61)
    batch, tax = synth.to_batch(data)
    params = cli.param_dict(cli.parse_flags([]))
    want = engine.score(batch, tax, params, gpus=1)
    for n in (2, 3):
        got = engine.score(batch, tax, params, gpus=n, devices=[0] * n)
        assert_same_results(got, want, batch)
    # the same contexts re-used while another thread grows and shrinks its batch
    a, b = engine.GpuScorer(0), engine.GpuScorer(0)
    a.set_taxonomy(tax)
    b.set_taxonomy(tax)
    out, errs = {}, []

    def run(key, s, parts):
        try:
            out[key] = [s.score(batch.slice(x, y), params) for x, y in parts]
        except Exception as exc:      # re-raised below
            errs.append(exc)
    ta = threading.Thread(target=run, args=("a", a, [(0, 100), (0, 3000), (0, 50), (0, 3000)]))
    tb = threading.Thread(target=run, args=("b", b, [(0, 3000), (0, 10), (0, 3000)]))
    ta.start(); tb.start(); ta.join(); tb.join()
    a.close(); b.close()
    assert errs == []
    for res in (out["a"][1], out["a"][3], out["b"][0], out["b"][2]):
        assert_same_results(res, want, batch)


def test_many_contigs_device_scan_branch():
    """> 32K active contigs at level 0 takes the hipcub segment-offset scan instead of the
    one-workgroup scan: the whole batch must equal its shards (each below the threshold)
    and the oracle on a sample."""
    data = synth.generate(n=40000, genes=2, clades=30, seed=71, decoys=1, lgt_frac=0.2)
    batch, tax = synth.to_batch(data)
    params = cli.param_dict(cli.parse_flags([]))
    s = engine.GpuScorer(0, mode="staged")    # every contig reaches the staged level 0
    s.set_taxonomy(tax)
    whole = s.score(batch, params)
    parts = [s.score(batch.slice(x, x + 20000), params) for x in (0, 20000)]
    s.close()
    assert_same_results(whole, engine.Results.concat(parts, [0, int(batch.hit_off[20000])]), batch)
    sub = batch.slice(30000, 30400)
    otax = orc.Taxonomy(data.tax.edges)
    contigs = orc.score_contigs(dict(zip(sub.contig_names, sub.contig_lengths.tolist())),
                                oracle_loci_from_batch(sub), oracle_hits_from_batch(sub, tax),
                                otax, orc.Params(**params))
    got = engine.Results(**{f: getattr(whole, f) for f in engine.Results.__dataclass_fields__})
    got = _slice_results(got, batch, 30000, 30400)
    assert_same_results(got, oracle_results(contigs, sub, tax), sub)


def _slice_results(res, batch, a, b):
    h0, h1 = int(batch.hit_off[a]), int(batch.hit_off[b])
    l0, l1 = int(batch.loc_off[a]), int(batch.loc_off[b])
    nsys = len(batch.systems)
    out = {}
    for f in engine.Results.__dataclass_fields__:
        v = getattr(res, f)
        if f == "synteny":
            out[f] = v[l0:l1]
        elif f == "annot_hit":
            w = v[l0 * nsys:l1 * nsys]
            out[f] = np.where(w >= 0, w - h0, -1).astype(np.int32)
        elif f == "meld":
            out[f] = v[2 * h0 + 2 * a:2 * h1 + 2 * b]
        else:
            out[f] = v[a:b]
    return engine.Results(**out)
