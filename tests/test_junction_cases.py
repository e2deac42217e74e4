"""CPU: the junction cases (junction_cases.py) against the oracle and against the answers
their builders know by construction; the product's host readers on the rendered text give
back the in-memory arrays the GPU test feeds to wf_junctions; and the host-side rebuild of
hit sets wider than pair_mask against the oracle's code sets."""
import numpy as np
import pytest

import junction_cases as jc
from oracle import junctions_oracle as jo
from waafle_amd import inputs, junctions

CASES = list(jc.all_cases())


def locus_index(case, table, contig, j):
    return int(table.loc_off[case.names().index(contig)]) + j


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_known_answers_match_oracle(case):
    got, table = jc.judge(case.name), case.table()
    for contig, runs in case.expect.get("cov", {}).items():
        want = np.zeros(dict((c[0], c[1]) for c in case.contigs)[contig], np.int64)
        for lo, hi, v in runs:
            want[lo:hi] += v
        assert np.array_equal(got.by_contig[contig], want), contig
    for (contig, j), n in case.expect.get("junction_hits", {}).items():
        k = locus_index(case, table, contig, j)
        assert got.is_junction[k] and got.junction_hits[k] == n, (contig, j)
    for (contig, j), n in case.expect.get("locus_hits", {}).items():
        assert got.locus_hits[locus_index(case, table, contig, j)] == n, (contig, j)
    for contig, j, field in case.expect.get("nan", []):
        assert np.isnan(got.floats[field, locus_index(case, table, contig, j)]), (contig, j, field)
    for contig, j in case.expect.get("zero_junction", []):
        k = locus_index(case, table, contig, j)
        assert got.floats[2, k] == 0.0 and got.floats[3, k] == 0.0, (contig, j)
    # the judge's text rows carry the same numbers
    assert len(got.junction_rows) == 1 + int(got.is_junction.sum())
    assert len(got.locus_hits) == len(table.loci)


@pytest.mark.parametrize("case", [c for c in CASES if c.name != "C_contended"], ids=repr)
def test_text_rendering_reads_back_as_the_arrays(case, tmp_path):
    fna, gff, sam = case.write_text(tmp_path)
    lengths = inputs.read_contig_lengths(fna)
    assert list(lengths.items()) == [(c[0], c[1]) for c in case.contigs]
    got = junctions.read_pairs(sam, {n: i for i, n in enumerate(lengths)})
    for a, b in zip(got[:5], case.pair_arrays()[:5]):
        assert np.array_equal(a, b)
    assert got[5] == []
    loci = junctions.read_contig_loci(gff)
    assert {k: [l.code for l in v] for k, v in loci.items()} == \
        {c[0]: ["{}:{}:{}".format(*l) for l in c[2]] for c in case.contigs if c[2]}
    assert len(list(jo.read_pairs(sam))) == len(case.pairs)


def test_geometry_the_families_promise():
    by = jc.by_name()
    t = by["L_reversed"].table()
    assert (t.loc_start > t.loc_end).any()
    for name in ("L_geometry", "H_hits_25", "W_wide_0", "W_nskip_25", "C_coverage"):
        t = by[name].table()
        assert (t.loc_start <= t.loc_end).all(), name
    assert [len(c[2]) for c in by["W_wide_0"].contigs] == jc.WIDE
    assert [c[1] for c in by["C_scan_3000"].contigs] == list(range(3000))
    assert len(by["C_contended"].pairs) == 100000
    g = {c[0]: c[2] for c in by["L_geometry"].contigs}
    t = by["L_geometry"].table()
    k = locus_index(by["L_geometry"], t, "l12_unsorted_gff", 0)
    assert [l.start for l in t.loci[k:k + 3]] == [20, 150, 300]
    k = locus_index(by["L_geometry"], t, "l09_equal_starts", 0)
    assert [l.code for l in t.loci[k:k + 4]] == ["90:95:-", "100:200:+", "100:300:-", "100:150:+"]
    assert g["l10_same_code_twice"][0] == g["l10_same_code_twice"][2]


def oracle_sets(case):
    """Per pair: the sorted locus indices whose code the oracle's find_hit_loci rule hits."""
    table = case.table()
    out = []
    for c, s1, e1, s2, e2, _, _ in case.pairs:
        out.append([k for k in range(int(table.loc_off[c]), int(table.loc_off[c + 1]))
                    if jo.calc_overlap(table.loci[k].start, table.loci[k].end, s1, e1) >= case.min_sites
                    or jo.calc_overlap(table.loci[k].start, table.loci[k].end, s2, e2) >= case.min_sites])
    return out


@pytest.mark.parametrize("name", ["W_wide_0", "W_nskip_25", "H_hits_25", "L_reversed", "edges_0"])
def test_wide_hits_rebuilds_what_the_mask_cannot_hold(name):
    """wide_hits (host) returns exactly the hits at locus first + 64 and later."""
    case = jc.by_name()[name]
    table, pairs, sets = case.table(), case.pair_arrays(), oracle_sets(case)
    first = np.array([s[0] if s else -1 for s in sets], dtype=np.int64)
    P, K = junctions.wide_hits(table, pairs, first, case.min_sites, chunk=2)
    got = sorted(zip(P.tolist(), K.tolist()))
    want = sorted((p, k) for p, s in enumerate(sets) for k in s if k >= s[0] + 64)
    assert got == want
    if name.startswith("W_") or name == "edges_0":
        assert len(want) > 0
    # and gene_hit_rows, given the device's outputs as the kernel defines them, is the judge's
    mask = np.array([sum(1 << (k - s[0]) for k in s if k - s[0] < 64) for s in sets] + [],
                    dtype=np.uint64)
    res = dict(pair_first=first, pair_mask=mask, wide_pair=P, wide_locus=K)
    assert junctions.gene_hit_rows(table, pairs, res) == jc.judge(name).gene_rows
