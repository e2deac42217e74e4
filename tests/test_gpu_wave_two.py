"""explain_two hand-overs with no candidate pair settled in the first wave form
(WF_OPT_WAVE_TWO 2, the default) against the flow that hands every one over
(WF_OPT_WAVE_TWO 1: the compact table and k_dump_sparse<1>) and the staged kernels:
bit-equal records across the three forms, and equal to the oracle where stated.

The inputs are chosen for both kinds of hand-over and for the compact form's limits: the
ones with no candidate pair (raised or stopped by the wave itself) at level 0 and at the
roll-up levels, the ones with pairs (the table, as before), 64 potential clades (the
compact form's limit: 65 take the whole table), 63 loci (its limit: 64 leave the wave
forms), the deep-taxonomy and runaway fixtures, and a hand-over buffer that overflows."""
import collections

import pytest

import golden_cases as gc
from oracle import orgscorer_oracle as orc
from oracle_bridge import oracle_results, run_oracle
from test_gpu_parity import FIELDS, assert_same_results
from test_gpu_scale import FORM_FLAGS
from waafle_amd import cli, engine, inputs, lib, output, synth

pytestmark = pytest.mark.gpu

assert "pair_evals" in FIELDS and "ppot_sum" in FIELDS and "iterations" in FIELDS

FORMS = {
    "wave": dict(),                                            # WF_OPT_WAVE_TWO 2
    "table": dict(options={lib.OPT_WAVE_TWO: 1}),
    "staged": dict(mode="staged"),
}


@pytest.fixture(scope="module")
def scorers():
    ss = {k: engine.GpuScorer(0, **kw) for k, kw in FORMS.items()}
    yield ss
    for s in ss.values():
        s.close()


def score_forms(scorers, batch, tax, flags=()):
    params = cli.param_dict(cli.parse_flags(list(flags)))
    got = {}
    for k, s in scorers.items():
        s.set_taxonomy(tax)
        got[k] = s.score(batch, params)
    return got


def traced_oracle(paths, flags=()):
    """The oracle's contigs, and its explain_two calls as (contig, roll-up level, potential
    clades, whether some pair reaches k2)."""
    calls, level = [], collections.Counter()
    one0, two0 = orc.one_clade, orc.two_clade

    def one(C, tax):
        level[C.name] += 1
        return one0(C, tax)

    def two(C, tax):
        pool = [c for c in orc._ordered(C.clades) if max(C.genes[c]) >= C.p.k2]
        has = any(C.evaluate(a, b)[0] >= C.p.k2 for a in pool for b in pool if a < b)
        calls.append((C.name, level[C.name] - 1, len(pool), has))
        return two0(C, tax)

    orc.one_clade, orc.two_clade = one, two
    try:
        contigs, _ = run_oracle(paths, list(flags))
    finally:
        orc.one_clade, orc.two_clade = one0, two0
    return contigs, calls


def oracle_case(tmp, **kw):
    data = synth.generate(**kw)
    paths = synth.write_text(data, str(tmp), "s")
    batch, tax = inputs.load_inputs(*paths, 200.0, warn=None)
    contigs, calls = traced_oracle(paths)
    return batch, tax, oracle_results(contigs, batch, tax), calls


@pytest.fixture(scope="module")
def lgt_batch(tmp_path_factory):
    return oracle_case(tmp_path_factory.mktemp("lgt"), n=300, genes=10, clades=2000, seed=5, lgt_frac=1.0)


def test_lgt_heavy_matches_oracle(scorers, lgt_batch):
    """300 contigs that all carry a transfer: explain_two at every level, with and without a
    candidate pair, each form against the oracle."""
    batch, tax, want, calls = lgt_batch
    ends = collections.Counter(want.iterations.tolist())
    assert min(ends[2], ends[3], ends[4]) >= 5 and ends[5] >= 40, ends
    assert sum(1 for c in calls if not c[3] and c[1] == 0) >= 10      # nothing to decide, level 0
    assert sum(1 for c in calls if not c[3] and c[1] >= 1) >= 10      # ... and at the roll-up levels
    assert sum(1 for c in calls if c[3] and c[1] == 0) >= 10 and sum(1 for c in calls if c[3] and c[1] >= 1) >= 10
    got = score_forms(scorers, batch, tax)
    for form in FORMS:
        assert_same_results(got[form], want, batch)


@pytest.mark.parametrize("flags", FORM_FLAGS[1:], ids=[" ".join(f) for f in FORM_FLAGS[1:]])
def test_lgt_heavy_forms_agree(scorers, lgt_batch, flags):
    """The flag sets that move every threshold the pass-4 masks (the wave's pair test) and
    sp_two compare with: the three forms give the same records."""
    batch, tax, _, _ = lgt_batch
    got = score_forms(scorers, batch, tax, flags)
    assert_same_results(got["wave"], got["staged"], batch)
    assert_same_results(got["table"], got["staged"], batch)


@pytest.fixture(scope="module")
def pool_batch(tmp_path_factory):
    return oracle_case(tmp_path_factory.mktemp("pool"), n=8, genes=20, clades=72, seed=0, stress=True)


def test_potential_clade_limit(scorers, pool_batch):
    """63, 64 and 65 potential clades in one explain_two call: 64 is the most the compact form
    (one lane per potential clade) takes, 65 goes over as a whole table."""
    batch, tax, want, calls = pool_batch
    per = collections.defaultdict(list)
    for name, _, pool, _ in calls:
        per[name].append(pool)
    single = {v[0] for v in per.values() if len(v) == 1}
    assert {63, 64, 65} <= single, sorted(single)
    for c, name in enumerate(batch.contig_names):
        if len(per[name]) == 1 and per[name][0] >= 2:
            assert int(want.ppot_sum[c]) == per[name][0]
    got = score_forms(scorers, batch, tax)
    for form in FORMS:
        assert_same_results(got[form], want, batch)


@pytest.mark.parametrize("genes", [63, 64])
def test_locus_limit(scorers, tmp_path, genes):
    """63 loci: the most the compact form's locus masks hold (bit 63 flags r__Root); 64 loci
    leave the wave forms."""
    batch, tax, want, calls = oracle_case(tmp_path, n=6, genes=genes, clades=50, seed=7, lgt_frac=1.0, decoys=2)
    assert batch.max_hits <= 224                                        # (the first form's slice)
    assert any(c[3] for c in calls) and any(not c[3] for c in calls)
    assert any(c[1] >= 1 for c in calls)
    got = score_forms(scorers, batch, tax)
    for form in FORMS:
        assert_same_results(got[form], want, batch)


@pytest.mark.parametrize("name", gc.runaway_names())
def test_deep_taxonomy_and_runaway(scorers, name, tmp_path):
    """Roll-up past the 16-level lineage table and the > 100 iteration guard: every form gives
    the reference's TSVs, or WF_E_RUNAWAY on the contig the reference dies on."""
    fx = gc.load_runaway(name)
    paths = gc.materialize(fx, tmp_path)
    batch, tax = inputs.load_inputs(*paths, 200.0, warn=None)
    params = cli.param_dict(cli.parse_flags(fx["flags"]))
    for form, s in scorers.items():
        s.set_taxonomy(tax)
        if fx["returncode"] == 0:
            rows = output.render(batch, tax, s.score(batch, params))
            assert {k: "\n".join(v) + "\n" for k, v in rows.items()} == fx["tsv"], form
            continue
        with pytest.raises(lib.WaafleHipError) as exc:
            s.score(batch, params)
        assert exc.value.code == lib.WF_E_RUNAWAY, form
        assert batch.contig_names[int(exc.value.contigs[0])] in fx["stderr"], form


def test_hand_over_buffer_overflow(lgt_batch, pool_batch):
    """A 96-entry hand-over buffer in the default form: the tables past it (whole ones of the
    contigs with 65 or more potential clades, compact ones with candidate pairs) go to the
    staged kernels, and the pairless hand-overs need no table at all."""
    s = engine.GpuScorer(0, options={lib.OPT_DUMP_CAP: 96})
    try:
        for batch, tax, want, _ in (pool_batch, lgt_batch):
            s.set_taxonomy(tax)
            got = s.score(batch, cli.param_dict(cli.parse_flags([])))
            assert_same_results(got, want, batch)
    finally:
        s.close()


def test_option_values():
    s = engine.GpuScorer(0)
    try:
        for v in (1, 2):
            assert s.lib.wf_set_option(s.h, lib.OPT_WAVE_TWO, v) == lib.WF_OK
        for v in (0, 3):
            assert s.lib.wf_set_option(s.h, lib.OPT_WAVE_TWO, v) == lib.WF_E_BADINPUT
    finally:
        s.close()
