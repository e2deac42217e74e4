"""GPU: the first wave form's envelope-integral bounds and explain_one from intervals
(wf_fast.hip), field by field against the oracle, in every execution form the parity module
runs.  The contigs (env_cases.py) put a multi-run segment's mean exactly on k2, k1 and kmin
and one thousandth to either side, so a decision taken from a bound inside its slack -- the
exact evaluation not engaging where it must -- shows as a wrong call, crit, rank, clade or
meld list; the neighbours' different outcomes show that the comparison is the one that
decides.  (Whether an exact evaluation was *skipped* where it may be does not show in the
records, and no test here asserts it: the stamps build's per-pass counts show it,
profiles/r08/stamps/.)  The other contigs: sister species that become an option only as
their genus' merged segment, four full clades with tied ranks and ranks exactly, just inside
and just outside --range, more than 64 full options, a 65-attachment segment (the
loose-bound path), G = 1 and G = 64, a contig that ends unclassified at r__Root
(pair_evals, ppot_sum), and all of them again under --weak-loci penalize / assign-unknown
and --min-overlap 0, where the bound-derived mask must stay off.

The bounds and the interval walk run in the roll-up launches only, so the k2 and k1
thresholds, the four clades and the > 64 options are each built twice: among species
(settled at level 0, by the code the roll-up launches share with it) and among genera whose
segments merge from two sister species (`*_l1_*`: no option and no pair at level 0, so the
mean on the threshold, the tie, the --range edges and the 66 / 70 options are decided at
level 1, where the walk drops clades and the sweep bounds the merged segments).
test_cases_are_what_they_claim pins the level each is settled at."""
import numpy as np
import pytest

import env_cases as ec
import mean_cases as mc
from test_gpu_parity import FORMS, assert_same_results, gpu_score
from waafle_amd import engine, lib

pytestmark = pytest.mark.gpu

SETS = ("env_one", "env_kmin", "env_one_penalize", "env_kmin_penalize", "env_one_unknown",
        "env_kmin_unknown", "env_one_overlap0", "env_kmin_overlap0",
        "env_wide", "env_wide_penalize", "env_wide_unknown", "env_wide_overlap0")


@pytest.fixture(scope="module", params=list(FORMS))
def scorer(request):
    s = engine.GpuScorer(0, **FORMS[request.param])
    s.form = request.param
    yield s
    s.close()


def by_name(cs, res):
    return {c.name: i for i, c in enumerate(cs.contigs)}, res


def test_cases_are_what_they_claim():
    """The oracle's outcomes of the designed contigs (default flags of each set): the
    thresholds decide as described, so the GPU comparison below tests those decisions."""
    cs = ec.case_sets()["env_one"]
    at, w = by_name(cs, ec.oracle_for(cs))
    name = lambda i: cs.tax.names[int(i)]
    for side in ("at", "above"):                        # mean >= k2: the pair; below: rolled up
        assert w.call[at["k2_" + side]] == lib.CALL_LGT and w.iterations[at["k2_" + side]] == 1
        assert w.call[at["k1_" + side]] == lib.CALL_NO_LGT and w.iterations[at["k1_" + side]] == 1
    assert w.crit[at["k2_at"]] == 0.75 and w.crit[at["k1_at"]] == 0.5
    assert w.call[at["k2_below"]] == lib.CALL_NO_LGT and w.iterations[at["k2_below"]] == 3
    assert w.call[at["k1_below"]] == lib.CALL_NO_LGT and w.iterations[at["k1_below"]] == 3
    # the same decisions among genera fall at level 1, in the roll-up launch
    for side in ("at", "above"):
        i, j = at["k2_l1_" + side], at["k1_l1_" + side]
        assert (w.call[i], w.iterations[i]) == (lib.CALL_LGT, 2)
        assert (w.call[j], w.iterations[j], name(w.clade1[j])) == (lib.CALL_NO_LGT, 2, "g__G0")
    assert w.crit[at["k2_l1_at"]] == 0.75 and w.crit[at["k1_l1_at"]] == 0.5
    for tag in ("k2_l1_below", "k1_l1_below"):
        i = at[tag]
        assert (w.call[i], w.iterations[i], name(w.clade1[i])) == (lib.CALL_NO_LGT, 3, "f__F")
    for tag, n in (("tie", 4), ("range", 3), ("range_top_last", 3)):
        i = at["four_l1_" + tag]
        assert (w.call[i], w.iterations[i], w.n_meld1[i]) == (lib.CALL_NO_LGT, 2, n)
        assert w.iterations[at["four_" + tag]] == 1
    i = at["siblings"]
    assert (w.call[i], w.iterations[i], name(w.clade1[i])) == (lib.CALL_NO_LGT, 2, "g__G0")
    assert w.n_meld1[at["four_tie"]] == 4
    assert w.n_meld1[at["four_range"]] == 3 and w.n_meld1[at["four_range_top_last"]] == 3
    assert 1 < w.n_meld1[at["many_66"]] < 66 and 1 < w.n_meld1[at["many_70"]] < 70
    cs = ec.case_sets()["env_wide"]
    at, w = by_name(cs, ec.oracle_for(cs))
    for k in (66, 70):                                  # k options at level 1, a third melded
        i = at["many_l1_{}".format(k)]
        assert (w.call[i], w.iterations[i]) == (lib.CALL_NO_LGT, 2)
        assert 1 < w.n_meld1[i] < k
    cs = ec.case_sets()["env_kmin"]
    at, w = by_name(cs, ec.oracle_for(cs))
    for side in ("at", "above"):                        # locus unmasked: nothing explains it
        assert w.call[at["kmin_" + side]] == 0 and w.iterations[at["kmin_" + side]] == 4
    assert w.call[at["kmin_below"]] == lib.CALL_NO_LGT and w.iterations[at["kmin_below"]] == 1
    i = at["to_root"]
    assert (w.call[i], w.iterations[i], w.pair_evals[i], w.ppot_sum[i]) == (0, 4, 2, 4)


@pytest.mark.parametrize("key", SETS)
def test_env_cases_match_oracle(scorer, key):
    cs = ec.case_sets()[key]
    sizes = np.diff(cs.batch.hit_off)
    assert cs.batch.max_hits <= 224                     # (the first form's smallest slice)
    assert sizes.min() >= 2
    got = gpu_score(scorer, cs.batch, cs.tax, cs.flags)
    assert_same_results(got, ec.oracle_for(cs), cs.batch)
