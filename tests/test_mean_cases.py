"""The conditions that keep tests/test_gpu_means.py honest, checked on the reference alone:
the case builders of mean_cases.py give what they intend (the oracle returns the intended
call, clade and iteration count, and for a single-locus contig a crit equal to the direct
numpy value bit for bit), and the scores tell numpy's summation order from a plain one."""
import numpy as np
import pytest

import mean_cases as mc
from waafle_amd import lib


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.int64)


def test_leaf_counts_at_the_routing_thresholds():
    assert mc.nl(1) == mc.nl(128) == 1 and mc.nl(129) == 2
    assert min(n for n in mc.ALL if mc.nl(n) > 32) == 3849
    assert min(n for n in mc.ALL if mc.nl(n) > 64) == 7689
    assert mc.nl(3848) == 32 and mc.nl(7688) == 64 and mc.nl(8191) == 65
    assert mc.multi_att0() in mc.NA and mc.multi_att0() + 1 in mc.NA


def test_family_a_covers_every_length():
    cs = mc.family_a()
    kinds = {}
    for c in cs.contigs:
        kinds.setdefault(c.meta["kind"], set()).add(c.meta["n"])
    want = set(mc.ALL) | {n for n in mc.EDGE if n >= mc.NPY_BUF}
    assert kinds["whole"] == want and kinds["overhang"] == want
    assert kinds["prefix"] == kinds["suffix"] == want - {1}
    assert kinds["inner"] == want - {1, 2}
    assert kinds["tiny"] == {n for n in want if n > 2 and (n in mc.EDGE or n % 3 == 0)}
    assert cs.max_len() == 65537


def test_family_b_covers_each_pattern_count_and_length():
    cs = mc.family_bc()
    seen = {"pattern": {}, "na": {}, "n": {}}
    for c in cs.contigs:
        if c.meta["family"] == "B":
            assert len(c.hits) == c.meta["na"]
            for k in seen:
                seen[k][c.meta[k]] = seen[k].get(c.meta[k], 0) + 1
    assert set(seen["pattern"]) == set(mc.PATTERNS_B) and min(seen["pattern"].values()) >= 3
    assert set(seen["na"]) == set(mc.NA) and min(seen["na"].values()) >= 3
    assert set(seen["n"]) == {n for n in mc.EDGE if n >= 128} and min(seen["n"].values()) >= 3
    # every (na, pattern) pair at a length on each side of 3848/3849, 7688/7689 and 8191/8192
    # is too many contigs; every na is at every length, which is what the routing reads


def test_outside_hits_wrap_as_python_slices():
    """Family C's left hit paints [0 : 1 - d]: nothing for d = 1 and d > n, all but the last
    site for d = 2, the first site for d = n."""
    for c in mc.family_bc().contigs:
        if c.meta["family"] != "C":
            continue
        n, kind = c.meta["n"], c.meta["kind"]
        lone = mc.Contig("x", {}, c.clade)
        lone.loci, lone.hits = c.loci, [h for h in c.hits if not (c.loci[0][0] <= h[2] and h[1] <= c.loci[0][1])]
        assert len(lone.hits) == 1 and len(c.hits) == 2
        painted = int(np.count_nonzero(lone.site_arrays()[0]))
        assert painted == {"l1": 0, "l2": n - 1, "lthird": n - n // 3 + 1, "ln": 1, "ln5": 0,
                           "right": 0}[kind]


@pytest.mark.parametrize("family", ["family_a_edge", "family_bc", "family_d", "family_e"])
def test_oracle_gives_the_intended_result(family):
    cs = getattr(mc, family)()
    got = mc.oracle_for(cs)
    names = np.array(cs.batch.contig_names)
    assert names[got.call != lib.CALL_NO_LGT].tolist() == []
    assert names[got.iterations != cs.iterations].tolist() == []
    fixed = cs.clade >= 0
    assert names[fixed & (got.clade1 != cs.clade)].tolist() == []
    crit, rank = cs.direct
    ok = cs.has_direct
    assert ok[cs.single & fixed].all()      # (family E's island contigs: the oracle alone)
    assert names[ok & (bits(got.crit) != bits(crit))].tolist() == []
    assert names[ok & (bits(got.rank) != bits(rank))].tolist() == []
    assert (bits(got.crit) == bits(got.rank))[cs.single].all()


@pytest.mark.parametrize("cap", mc.SLICES)
def test_many_option_contigs_meld_every_option(cap):
    cs = mc.family_f(cap)
    got = mc.oracle_for(cs)
    assert (got.call == lib.CALL_NO_LGT).all() and (got.iterations == 1).all()
    assert got.n_meld1.tolist() == [c.meta["k"] for c in cs.contigs]
    assert (got.clade1 == cs.clade).all()
    assert max(got.n_meld1) > 128 or cap == 224


def test_batches_reach_the_large_slices():
    """The wave kernels size their LDS slices by the batch's longest contig (224, 256 or 512
    attachments): the multi-attachment batch runs in the small one, the island batches in
    the large one."""
    assert mc.family_bc().batch.max_hits <= 224
    assert mc.family_d().batch.max_hits > 256 and mc.family_e().batch.max_hits > 256


def test_scores_tell_summation_orders_apart():
    """Among the family-A cases with n > 128, at least 90 % have an np.mean whose bits
    differ from the left-to-right sum's: a kernel that adds in another order fails them."""
    cs = mc.family_a()
    crit, _ = cs.direct
    total = differ = 0
    for i, c in enumerate(cs.contigs):
        n = c.meta["n"]
        if n <= 128:
            continue
        a = c.site_arrays()[0]
        total += 1
        differ += int(bits(crit[i]) != bits(np.cumsum(a)[-1] / n))
    assert total > 40000
    assert differ >= 0.9 * total, (differ, total)
