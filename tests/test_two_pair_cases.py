"""CPU: the contigs of two_pair_cases.py are what they claim.  A trace of the oracle's
two_clade gives, per contig, the roll-up level of each explain_two call, its candidate pairs
and how many lie within --range of the best; each case states these for the call it was
designed around, and the contig's final call.  So tests/test_gpu_two_pairs.py compares the
GPU with the oracle on the decisions its cases are named after."""
import pytest

import two_pair_cases as tp
from waafle_amd import lib

CALLS = {tp.LGT: lib.CALL_LGT, tp.NO_LGT: lib.CALL_NO_LGT, tp.NONE: 0}


def check_set(cs):
    calls, res = tp.traced_oracle(cs)
    for i, c in enumerate(cs.contigs):
        level, pairs, near, call = c.meta["want"]
        at = [t for t in calls.get(c.name, []) if t[0] == level]
        assert len(at) == 1, (cs.key, c.name, calls.get(c.name))
        assert at[0][1:3] == (pairs, near), (cs.key, c.name, at[0])
        assert int(res.call[i]) == CALLS[call], (cs.key, c.name, int(res.call[i]))
        if at[0][3]:                                   # decided by that call
            assert call == tp.LGT and int(res.iterations[i]) == level + 1, (cs.key, c.name)
        else:
            assert int(res.iterations[i]) > level + 1, (cs.key, c.name)
    return calls, res


@pytest.mark.parametrize("key", sorted(tp.case_sets()))
def test_cases_are_what_they_claim(key):
    check_set(tp.case_sets()[key])


def test_candidate_pair_counts_straddle_the_kernel_paths():
    """1 .. 100 pairs at level 0 and at level 1; 2 .. 63 unmasked loci with gaps."""
    for key, level in (("two_l0", 0), ("two_l1", 1), ("two_l1_off", 1)):
        cs = tp.case_sets()[key]
        got = {c.meta["want"][1] for c in cs.contigs if c.name.startswith("grid") and c.meta["want"][0] == level}
        assert got == {1, 2, 3, 7, 8, 9, 16, 63, 64, 65, 100}
    cs = tp.case_sets()["two_l0"]
    assert {c.meta["gu"] for c in cs.contigs if "gu" in c.meta} == {2, 7, 8, 9, 15, 16, 17, 63}
    for s in list(tp.case_sets().values()) + [tp.leaves_set()]:
        assert s.batch.max_hits <= 224 and max(len(c.loci) for c in s.contigs) <= 63


def test_ties_go_to_the_later_pair():
    cs = tp.case_sets()["two_l0_best"]
    _, res = tp.traced_oracle(cs)
    i = [c.name for c in cs.contigs].index("sel_tie")
    assert cs.tax.names[int(res.clade2[i])] == "s__S1_01"


def test_clade_leaves_moves_the_checks_to_the_genera():
    """--clade-leaves 2: every pair of species is rejected (one leaf each) whatever else holds,
    and the genera decide at level 1 with their own pairs."""
    cs = tp.leaves_set()
    calls, res = tp.traced_oracle(cs)
    for i, c in enumerate(cs.contigs):
        first = calls[c.name][0]
        assert first[0] == 0 and first[1] == c.meta["want"][1] and not first[3], (c.name, first)
        assert int(res.iterations[i]) >= 2
    assert sum(1 for i in range(len(cs.contigs)) if int(res.call[i]) == lib.CALL_LGT and
               int(res.iterations[i]) == 2) >= 6
