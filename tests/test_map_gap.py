"""Single-gap rescue of the read mapper, host side (no GPU): the two CPU oracles of the rule
agree and give what each hand-built batch states, G = 0 is the ungapped rule, the SAM writer
against junctions.read_pairs, the ctypes binding and the CLI option.  The kernel itself is
checked in tests/test_gpu_map_gap.py."""
import ctypes

import numpy as np
import pytest

import map_cases as mc
import map_gap_cases as gc
import map_gap_oracle as go
import map_oracle as mo
from waafle_amd import junctions, lib, mapper


@pytest.mark.parametrize("name", sorted(gc.HAND_BUILT))
def test_oracles_agree_on_hand_built_cases(name):
    contigs, r1, r2, P, G, expect = gc.HAND_BUILT[name]()
    brute = go.map_pairs_gapped_brute(contigs, r1, r2, P, G)
    assert go.map_pairs_gapped_indexed(contigs, r1, r2, P, G) == brute
    gc.check_expect(brute, expect)


@pytest.mark.parametrize("name", sorted(gc.HAND_BUILT) + sorted(mc.HAND_BUILT))
def test_max_gap_0_is_the_ungapped_rule(name):
    contigs, r1, r2, P = (gc.HAND_BUILT.get(name) or mc.HAND_BUILT[name])()[:4]
    want = [r + go.NO_GAP for r in mo.map_pairs_indexed(contigs, r1, r2, P)]
    assert go.map_pairs_gapped_indexed(contigs, r1, r2, P, 0) == want
    if max(len(r) for r in r1 + r2) <= 100:
        assert go.map_pairs_gapped_brute(contigs, r1, r2, P, 0) == want


def test_oracle_hand_checked_results():
    contigs, r1, r2, P, G, _ = gc.homopolymer()
    got = go.map_pairs_gapped_indexed(contigs, r1, r2, P, G)
    assert got[0] == (0, 201, 381, 0, 0, 0, 1, 0, 50, 0, 1)       # the run starts at read base 50
    assert got[1] == (0, 381, 201, 1, 0, 0, 0, -1, 0, 50, 1)
    contigs, r1, r2, P, G, _ = gc.gap_ties()
    got = go.map_pairs_gapped_indexed(contigs, r1, r2, P, G)
    assert got[0][6:] == (-1, 0, 40, 0, 1) and got[1][6:] == (0, -1, 0, 40, 1)
    contigs, r1, r2, P, G, _ = gc.ungapped_first()
    assert go.map_pairs_gapped_indexed(contigs, r1, r2, P, G)[0] == (0, 201, 381, 0, 2, 0, 0, 0, 0, 0, 0)
    contigs, r1, r2, P, G, _ = gc.gap_lengths()
    got = go.map_pairs_gapped_indexed(contigs, r1, r2, P, G)
    assert [g[6] for g in got] == [1, -1, 4, -4, 0] and [g[8] for g in got][1::2] == [50, 50]
    assert all(g[1] == 41 and g[4:6] == (0, 0) for g in got)
    # a deletion moves the - mate's start, an insertion does not move the + mate's
    assert [g[2] for g in got] == [241] * 5


def test_medium_set_holds_every_outcome():
    contigs, r1, r2, P, G = gc.medium()
    assert len(contigs) == 20 and len(r1) == 600
    flags = go.as_arrays(go.map_pairs_gapped_indexed(contigs, r1, r2, P, G))
    ungapped = np.mean((flags["contig"] >= 0) & (flags["flags"] == 0))
    rescued = np.mean(flags["flags"] == 1)
    unaligned = np.mean(flags["contig"] < 0)
    assert min(ungapped, rescued, unaligned) >= 0.10, (ungapped, rescued, unaligned)


def test_planted_contigs_have_unique_kmers():
    contigs, r1, _, P, G, truth = gc.planted()
    assert mc.unique_kmers(contigs, P["S"]) and len(truth) == len(r1) == 200
    assert all(abs(t[4]) + abs(t[5]) in range(1, G + 1) for t in truth)


# ---------------------------------------------------------------------------
# SAM writer
# ---------------------------------------------------------------------------

def gap_result():
    """A deletion and an insertion, each on mate 1 (+), on the reverse mate 2, and on a
    reverse mate 1; one ungapped and one unaligned pair."""
    return dict(contig=np.array([0, 0, 1, 1, 2, -1, 0], np.int32),
                pos1=np.array([5, 5, 40, 40, 300, 0, 7], np.int32),
                pos2=np.array([205, 205, 200, 200, 100, 0, 90], np.int32),
                strand1=np.array([0, 0, 0, 0, 1, 0, 0], np.uint8),
                mm1=np.array([0, 1, 0, 0, 2, 0, 3], np.uint8), mm2=np.array([2, 0, 0, 1, 0, 0, 0], np.uint8),
                d1=np.array([3, -2, 0, 0, -1, 0, 0], np.int8), d2=np.array([0, 0, 1, -8, 4, 0, 0], np.int8),
                k1=np.array([30, 61, 0, 0, 20, 0, 0], np.int16), k2=np.array([0, 0, 25, 50, 70, 0, 0], np.int16),
                flags=np.array([1, 1, 1, 1, 1, 0, 0], np.uint8))


def test_sam_round_trip_with_gaps_through_read_pairs(tmp_path):
    names = ["ctgA", "ctgB", "ctgC"]
    res = gap_result()
    len1 = np.array([100, 100, 100, 100, 151, 30, 60])
    len2 = np.array([90, 90, 100, 100, 151, 30, 60])
    qnames = ["q{}".format(i) for i in range(7)]
    lines = mapper.sam_header(names, [1000, 2000, 900]) + mapper.sam_records(qnames, len1, len2, res, names)
    recs = [l.split("\t") for l in lines if not l.startswith("@")]
    assert [r[5] for r in recs] == ["30M3D70M", "90M", "61M2I37M", "90M", "100M", "25M1D75M", "100M",
                                    "50M8I42M", "20M1I130M", "70M4D81M", "*", "*", "60M", "60M"]
    assert [r[11] for r in recs[:10]] == ["NM:i:3", "NM:i:2", "NM:i:3", "NM:i:0", "NM:i:0", "NM:i:1",
                                          "NM:i:0", "NM:i:9", "NM:i:3", "NM:i:4"]
    assert [r[1] for r in recs] == ["99", "147"] * 4 + ["83", "163", "77", "141", "99", "147"]
    # TLEN from the spans: mate 2 of pair 0 ends at 205 + 90, of pair 2 at 200 + 101, of pair 3
    # at 200 + 92; mate 1 of pair 4 (on -) ends at 300 + 150
    assert [r[8] for r in recs[:10]] == ["290", "-290", "290", "-290", "261", "-261", "252", "-252",
                                         "-350", "350"]
    for r in recs:                                        # the CIGAR consumes the whole read
        if r[5] != "*":
            ops = junctions._CIGAR_OP.findall(r[5])
            assert sum(int(n) for n, op in ops if op in "MI") in (100, 90, 151, 60)
    sam = tmp_path / "g.sam"
    sam.write_text("\n".join(lines) + "\n")
    got = junctions.read_pairs(str(sam), {n: i for i, n in enumerate(names)})
    want = mapper.pair_arrays(res, len1, len2)
    assert got[5] == []
    for g, w in zip(got[:5], want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert want[2].tolist() == [107, 102, 139, 139, 449, 66]       # p + L + d - 1
    assert want[4].tolist() == [294, 294, 300, 291, 254, 149]


def test_result_without_gap_fields_renders_as_before():
    res = {f: a for f, a in gap_result().items() if f in dict(mapper.RESULT_FIELDS)}
    recs = mapper.sam_records(["a"] * 7, [100] * 7, [100] * 7, res, ["x", "y", "z"])
    assert all(r.split("\t")[5] in ("100M", "*") for r in recs)
    assert recs[0].split("\t")[8] == "300" and recs[0].split("\t")[11] == "NM:i:0"
    assert mapper.pair_arrays(res, [100] * 7, [100] * 7)[2].tolist() == [104, 104, 139, 139, 399, 106]


# ---------------------------------------------------------------------------
# binding and CLI
# ---------------------------------------------------------------------------

def test_gapped_entry_point_is_bound():
    assert "wf_map_pairs_gapped" in lib.SIGNATURES
    so = lib.load()
    assert so.wf_abi_version() == 6
    assert ctypes.sizeof(lib.WfMapGapParams) == 16 and ctypes.sizeof(lib.WfMapGapResult) == 40
    assert lib.WfMapGapResult.flags.offset == 32
    assert ctypes.sizeof(lib.WfMapParams) == 32 and ctypes.sizeof(lib.WfMapResult) == 48   # unchanged
    # argument checks come before any device call
    assert so.wf_map_pairs_gapped(None, None, None, None, None, None) == lib.WF_E_BADINPUT
    assert [f for f, _ in mapper.GAP_FIELDS] == ["d1", "d2", "k1", "k2", "flags"]
    assert [np.dtype(t).itemsize for _, t in mapper.GAP_FIELDS] == [1, 1, 2, 2, 1]


def test_cli_max_gap_option():
    ap = junctions.build_parser()
    assert ap.parse_args(["c.fna", "g.gff"]).max_gap == 0
    a = ap.parse_args(["c.fna", "g.gff", "--mapper", "native", "--max-gap", "3"])
    assert a.max_gap == 3 and a.mapper == "native"
    group = next(g for g in ap._action_groups if g.title == "read mapper")
    assert "--max-gap" in [s for act in group._group_actions for s in act.option_strings]
    with pytest.raises(SystemExit):
        ap.parse_args(["c.fna", "g.gff", "--max-gap", "three"])
