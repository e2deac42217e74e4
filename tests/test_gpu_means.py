"""GPU: the segment mean on every route, against numpy itself (mean_cases.py).

The float64 mean of a locus's site array is computed by closed forms (pw_const_sum /
pw_run_sum in the triage and in one_run_mean), by the leaf-table walk, by the wave kernels'
wave / lane / flat multi-attachment paths and by the staged leaf kernels; which one depends
on the locus length, its numpy leaf count and the segment's attachment count.  The cases
cross every change-over on purpose (3848/3849, 7688/7689, 8191/8192/8193, 65535/65536, and
4/5, 16/17, 32/33, 64/65 attachments at those lengths), in every execution form.  Family F
adds contigs with more explain_one options than a wave has lanes, which the mixed batch
showed the wave kernels losing.  Expected values are np.mean of explicitly painted arrays,
cross-checked against the oracle on the CPU by test_mean_cases.py; the bar is the int64 bit
pattern.

Thinned: family A's interior run of 1-9 sites is built at every EDGE length and at every
third other length (mean_cases.one_run_contigs says why); every other run is at every n.
"""
import ctypes as C

import numpy as np
import pytest

import mean_cases as mc
from test_gpu_parity import FORMS, assert_same_results, gpu_score
from waafle_amd import engine, lib

pytestmark = pytest.mark.gpu

# the eighth form: the comparison arm of explain_two's hand-over in the wave levels
MEAN_FORMS = dict(FORMS, wave_two=dict(mode="level0", options={lib.OPT_WAVE_TWO: 1}))


@pytest.fixture(scope="module", params=list(MEAN_FORMS))
def scorer(request):
    s = engine.GpuScorer(0, **MEAN_FORMS[request.param])
    s.form = request.param
    yield s
    s.close()


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def score_timed(scorer, cs):
    """(results, phase spans) of one score call over the case set."""
    tm = lib.WfTiming()
    scorer.lib.wf_timing_enable(scorer.h, 1)
    try:
        got = gpu_score(scorer, cs.batch, cs.tax, cs.flags)
        assert scorer.lib.wf_timing_read(scorer.h, C.byref(tm)) == 0
    finally:
        scorer.lib.wf_timing_enable(scorer.h, 0)
    return got, tm.phases()


def assert_handed_over(scorer, cs, phases):
    """The batch has loci of >= 8192 sites, which no wave form answers: in the default form
    the staged phases ran (the early return after the wave levels did not fire)."""
    assert cs.max_len() >= mc.NPY_BUF
    if scorer.form == "level0":
        assert phases["attach"][1] > 0 and phases["segments"][1] > 0, phases


def describe(c):
    m = dict(c.meta)
    if len(c.hits) == 1:
        m["v"] = c.hits[0][4]
    return m


def assert_direct(got, cs):
    """crit and rank equal the direct numpy values as bit patterns, wherever one exists."""
    crit, rank = cs.direct
    ok = cs.has_direct & (got.call == lib.CALL_NO_LGT)
    bad = np.nonzero(ok & ((bits(got.crit) != bits(crit)) | (bits(got.rank) != bits(rank))))[0]
    for i in bad[:8]:
        print(describe(cs.contigs[i]), "crit", float(got.crit[i]).hex(), float(crit[i]).hex(),
              "rank", float(got.rank[i]).hex(), float(rank[i]).hex())
    assert len(bad) == 0, "{} contigs differ from np.mean".format(len(bad))


def test_one_run_every_length(scorer):
    """Family A: one species, one hit; every n in 1..8191 and the long EDGE lengths, with the
    whole-locus, prefix, suffix, interior and overhanging runs at every n.  Thinned: the
    interior run of 1-9 sites, to every EDGE length and every third other length."""
    cs = mc.family_a()
    got, phases = score_timed(scorer, cs)
    want, _ = cs.direct
    wrong = ((got.call != lib.CALL_NO_LGT) | (got.status != 0) | (got.clade1 != cs.clade)
             | (bits(got.crit) != bits(want)) | (bits(got.rank) != bits(want)))
    bad = np.nonzero(wrong)[0]
    for i in bad[:8]:
        m = cs.contigs[i].meta
        print((m["n"], m["lo"], m["hi"], m["v"], float(got.crit[i]).hex(), float(want[i]).hex()),
              "call", int(got.call[i]), "status", int(got.status[i]), "rank", float(got.rank[i]).hex())
    assert len(bad) == 0, "{} of {} one-run contigs are wrong".format(len(bad), len(wrong))
    assert_handed_over(scorer, cs, phases)


def check_against_oracle(scorer, cs):
    got, phases = score_timed(scorer, cs)
    assert (got.status == 0).all()
    assert_direct(got, cs)
    assert_same_results(got, mc.oracle_for(cs), cs.batch)
    assert_handed_over(scorer, cs, phases)


def test_multi_attachment_routes(scorer):
    """Families B and C: 2 .. 130 attachments of one species on one locus in seven patterns
    (the prune against the whole-locus hit and its strict '>' among them), and hits outside
    a long locus painted by --min-overlap 0 through Python's slice wrap."""
    check_against_oracle(scorer, mc.family_bc())


def test_rollup_routes(scorer):
    """Family D: 2, 5, 17 and 65 sister species whose islands pass -k1 0.9 only as a union,
    at the genus (iteration 2) or the family (iteration 3); contigs of 3 and 5 such loci."""
    check_against_oracle(scorer, mc.family_d())


@pytest.mark.parametrize("cap", mc.SLICES)
def test_many_options(scorer, cap):
    """Family F: 63 .. 200 clades that each explain the contig alone, in a batch sized for each
    of the wave kernels' slices; --range 1.0 melds every option, so a lost one shows."""
    cs = mc.family_f(cap)
    got = gpu_score(scorer, cs.batch, cs.tax, cs.flags)
    want = mc.oracle_for(cs)
    assert got.n_meld1.tolist() == want.n_meld1.tolist()
    assert_same_results(got, want, cs.batch)


def test_mixed_batch(scorer):
    """Family E: one-run, multi-attachment and island contigs as neighbours in one batch."""
    check_against_oracle(scorer, mc.family_e())
