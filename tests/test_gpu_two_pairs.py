"""GPU: explain_two on the compact table (sp_two, wf_sparse.h), field by field against the
oracle, in every execution form the parity module runs and in the flow that hands every
explain_two contig over as a table (WF_OPT_WAVE_TWO 1).  The contigs (two_pair_cases.py)
vary what the kernel's one-evaluation-per-pair form depends on: 1 .. 100 candidate pairs at
level 0 and among genera at level 1 (the whole wave on each of a few pairs, a lane per pair
beyond that, the 64 pairs a wave keeps in registers), 2 .. 63 unmasked loci with masked ones
between them (numpy's summation branches; crit and rank are compared as bits), ties, ranks
exactly on, just inside and just outside --range, one and several options within it, and
every branch of the synteny and the LGT checks with one candidate pair and among twenty.
tests/test_two_pair_cases.py pins, without a GPU, that each contig is the case its name
says.  (Which of the kernel's two forms took a contig does not show in the records, and no
test here asserts it: the stamps build counts the wave-form calls, profiles/sp_two/.)"""
import pytest

import env_cases as ec
import two_pair_cases as tp
from test_gpu_parity import FORMS, assert_same_results, gpu_score
from waafle_amd import engine, lib

pytestmark = pytest.mark.gpu

ALL_FORMS = dict(FORMS, table=dict(options={lib.OPT_WAVE_TWO: 1}))
SETS = sorted(tp.case_sets()) + ["two_l0_leaves2"]


def case_set(key):
    return tp.leaves_set() if key == "two_l0_leaves2" else tp.case_sets()[key]


@pytest.fixture(scope="module", params=list(ALL_FORMS))
def scorer(request):
    s = engine.GpuScorer(0, **ALL_FORMS[request.param])
    s.form = request.param
    yield s
    s.close()


@pytest.mark.parametrize("key", SETS)
def test_two_pair_cases_match_oracle(scorer, key):
    cs = case_set(key)
    assert cs.batch.max_hits <= 224                     # (the first form's smallest slice)
    got = gpu_score(scorer, cs.batch, cs.tax, cs.flags)
    assert_same_results(got, ec.oracle_for(cs), cs.batch)
