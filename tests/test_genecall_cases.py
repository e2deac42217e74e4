"""CPU: the gene-caller cases (genecall_cases.py) against the oracle and against the answers
their builders know by construction, so that a wrong builder cannot pass quietly on the GPU."""
import pytest

import genecall_cases as gcs

CASES = [c for c in gcs.all_cases() if c.refused_group is None]


def summary(genes):
    """Per group: gene count, first start, last stop, strands."""
    return [(len(g), g[0][0] if g else None, g[-1][1] if g else None, [x[2] for x in g])
            for g in genes]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_builder_answers_match_oracle(case):
    want, got = case.expected(), gcs.oracle_of(case.name)
    assert summary(got) == summary(want)
    assert got == want


def test_size_family_passes_the_sizes_it_names():
    seen = []
    for c in gcs.family_s():
        passing = [sum(1 for h in g if h[4] is not None) for g in c.groups]
        seen.append(max(passing))
        # rejected hits lie between passing ones in every 64-hit chunk that has any
        g = c.groups[passing.index(max(passing))]
        if max(passing) >= 63:
            chunks = [g[i:i + 64] for i in range(0, len(g), 64)]
            mixed = sum(1 for ch in chunks if 0 < sum(1 for h in ch if h[4] is None) < len(ch))
            assert mixed >= len(chunks) // 2, c.name
    assert seen == gcs.SIZES + [gcs.CAP_MAX, gcs.CAP_MAX + 1]
    big = {c.name: c for c in gcs.family_s()}["S_4096_of_5000"]
    assert len(big.groups[0]) == 5000


@pytest.mark.parametrize("n", gcs.TOPO_SIZES)
def test_topology_answers(n):
    by = {c.name: c.expected()[0] for c in gcs.family_t() if c.name.endswith("_{}".format(n))}
    last = 1 + 100 * (n - 1) + 149
    for name in ("T_chain_{}", "T_chain_reversed_{}", "T_chain_shuffled_{}"):
        assert by[name.format(n)] == [(1, last, "-")]
    pieces = -(-n // 7)
    assert len(by["T_chain_cut7_{}".format(n)]) == pieces
    assert by["T_chain_cut7_shuffled_{}".format(n)] == by["T_chain_cut7_{}".format(n)]
    assert {g[2] for g in by["T_chain_cut7_{}".format(n)]} == {"+", "-"}
    assert by["T_container_{}".format(n)] == [(1, 50 * n + 200, "-")]
    assert by["T_star_{}".format(n)] == [(300, 800 + 50 * n, "+")]
    assert len(by["T_weak_links_two_{}".format(n)]) == 2
    assert len(by["T_weak_links_many_{}".format(n)]) == -(-n // 5)


def test_weak_then_strong_is_one_gene():
    case = {c.name: c for c in gcs.family_t()}["T_weak_then_strong"]
    assert case.expected() == [[(1, 3000, "-")]] * 3


def test_tie_and_threshold_answers():
    by = {c.name: c.expected() for c in gcs.family_k()}
    # stable sort: equal starts keep their file order
    for genes, group in zip(by["K_stable_sort"], {c.name: c for c in gcs.family_k()}["K_stable_sort"].groups):
        assert len(genes) == len(group) == 8
        want = sorted(range(8), key=lambda i: (group[i][0], i))
        assert genes == [(group[i][0], group[i][1], "-" if group[i][2] else "+") for i in want]
    assert [g[0][2] for g in by["K_strand"]] == ["-", "-", "-", "+", "+", "-"]
    assert [len(g) for g in by["K_overlap_at_0.1"]] == [1, 2] * 4
    assert [len(g) for g in by["K_overlap_at_0.5"]] == [1, 2] * 2
    assert [len(g) for g in by["K_overlap_at_1.0"]] == [1, 2, 1, 1, 2]
    for t in ("0.0", "-0.5"):
        assert [len(g) for g in by["K_min_overlap_" + t]] == [1, 1, 1, 0]
        assert by["K_min_overlap_" + t][1] == [(1, 100200, "-")]
    assert [len(g) for g in by["K_gene_length_200"]] == [1, 0, 1, 3]
    assert [len(g) for g in by["K_gene_length_200.5"]] == [0, 0, 1, 1]
    assert by["K_scov_exact"] == [[(1, 300, "+"), (1001, 1300, "-")], [], [(1, 600, "-")]]
    assert by["K_reversed_coordinates"][0] == [(1, 600, "-"), (900, 1200, "-")]
    assert by["K_reversed_coordinates"][2] == [(5, 5, "-"), (6, 6, "-")]


def test_many_groups_batch():
    case = gcs.family_g()
    sizes = [sum(1 for h in g if h[4] is not None) for g in case.groups]
    assert len(case.groups) == 10000 and max(sizes) == gcs.CAP_MAX
    assert set(sizes) == set(gcs.G_SIZES) | {gcs.CAP_MAX}
    assert sum(1 for g in case.groups if not g) > 100                       # empty groups
    assert sum(1 for g, s in zip(case.groups, sizes) if g and s == 0) > 100  # all rejected
    want, got = case.expected(), gcs.oracle_of(case.name)
    assert summary(got) == summary(want)
    assert got == want
    # the length filter drops genes, and not all of them
    assert 0 < sum(len(g) for g in want) < sum(len({h[4] for h in g if h[4] is not None})
                                                 for g in case.groups)
