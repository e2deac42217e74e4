"""wf_map_pairs_gapped (k_map_gap, wf_map.hip) on the GPU against the CPU oracles of the
single-gap rescue (tests/map_gap_oracle.py): every result field of every pair must be equal,
the six of wf_map_pairs and d1, d2, k1, k2, flags.  Hand-built edge batches, a seeded medium
set (whole, in chunks of 7 and of 1), device-resident reads, planted indels against their
origin, and `waafle_junctions --mapper native --max-gap` end to end."""
import ctypes as C
import gzip

import numpy as np
import pytest

import map_cases as mc
import map_gap_cases as gc
import map_gap_oracle as go
import map_oracle as mo
from oracle import junctions_oracle as jo
from waafle_amd import junctions, lib, mapper

pytestmark = pytest.mark.gpu

FIELDS = [f for f, _ in mapper.RESULT_FIELDS + mapper.GAP_FIELDS]


def kw(P, G):
    return dict(seed_length=P["S"], max_seed_hits=P["max_occ"], max_mismatches=P["max_mm"],
                min_insert=P["min_insert"], max_insert=P["max_insert"], max_gap=G)


def run(m, r1, r2):
    return m.map(*mc.flat(r1), *mc.flat(r2))


def assert_equal(got, want, what=""):
    want = go.as_arrays(want) if not isinstance(want, dict) else want
    for f in FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert got[f].dtype == want[f].dtype and len(bad) == 0, \
            "{} {}: pair {} got {} want {}".format(what, f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])


def rows(res):
    return list(zip(*(res[f].tolist() for f in FIELDS)))


@pytest.mark.parametrize("name", sorted(gc.HAND_BUILT))
def test_hand_built_cases_equal_both_oracles(name):
    contigs, r1, r2, P, G, expect = gc.HAND_BUILT[name]()
    want = go.map_pairs_gapped_indexed(contigs, r1, r2, P, G)
    if max(len(r) for r in r1 + r2) <= 100:              # (test_map_gap.py holds the long ones)
        assert want == go.map_pairs_gapped_brute(contigs, r1, r2, P, G)
    with mapper.Mapper(*mc.flat(contigs), **kw(P, G)) as m:
        got = run(m, r1, r2)
    assert_equal(got, want, name)
    gc.check_expect(rows(got), expect)


@pytest.mark.parametrize("name", ["gap_lengths", "contig_ends", "overflow"])
def test_max_gap_0_writes_the_ungapped_result_and_zeros(name):
    contigs, r1, r2, P, _, _ = gc.HAND_BUILT[name]()
    want = [r + go.NO_GAP for r in mo.map_pairs_indexed(contigs, r1, r2, P)]
    with mapper.Mapper(*mc.flat(contigs), **kw(P, 0)) as m:
        for gapped in (True, False):                     # wf_map_pairs_gapped, wf_map_pairs
            got = m.map(*mc.flat(r1), *mc.flat(r2), gapped=gapped)
            for f, dt in mapper.GAP_FIELDS:
                assert got[f].dtype == dt and not got[f].any()
            assert_equal(got, want, name)


def test_parameter_checks():
    contigs, r1, r2, P, G, _ = gc.gap_lengths()
    with pytest.raises(mapper.MapperError):
        mapper.Mapper(*mc.flat(contigs), **kw(P, 9))
    with mapper.Mapper(*mc.flat(contigs), **kw(P, G)) as m:
        for bad in (-1, 9):
            m.gap_params.max_gap = bad
            with pytest.raises(lib.WaafleHipError) as exc:
                run(m, r1, r2)
            assert exc.value.code == lib.WF_E_BADINPUT
        m.gap_params.max_gap = G
        empty = np.zeros(1, np.int64)
        none = m.map(np.zeros(0, np.uint8), empty, np.zeros(0, np.uint8), empty)
        assert len(none["flags"]) == 0
        seq, off = mc.flat(r1)
        rd = lib.WfMapReads(n_pairs=len(r1), seq1=lib.ptr(seq), off1=lib.ptr(off), seq2=lib.ptr(seq), off2=lib.ptr(off))
        out = {f: np.zeros(len(r1), dt) for f, dt in mapper.RESULT_FIELDS + mapper.GAP_FIELDS}
        r = lib.WfMapResult(**{f: lib.ptr(out[f]) for f, _ in mapper.RESULT_FIELDS})
        g = lib.WfMapGapResult(**{f: lib.ptr(out[f]) for f, _ in mapper.GAP_FIELDS})
        g.k2 = None
        call = m.so.wf_map_pairs_gapped
        assert call(m.h, C.byref(rd), C.byref(m.params), C.byref(m.gap_params), C.byref(r), C.byref(g)) == lib.WF_E_BADINPUT
        assert call(m.h, C.byref(rd), C.byref(m.params), None, C.byref(r), C.byref(g)) == lib.WF_E_BADINPUT
        assert call(m.h, C.byref(rd), C.byref(m.params), C.byref(m.gap_params), C.byref(r), None) == lib.WF_E_BADINPUT
        assert_equal(run(m, r1, r2), go.map_pairs_gapped_indexed(contigs, r1, r2, P, G))   # still usable
    so = lib.load()
    h = C.c_void_p()
    assert so.wf_init(0, C.byref(h)) == lib.WF_OK
    try:
        g = lib.WfMapGapResult(**{f: lib.ptr(out[f]) for f, _ in mapper.GAP_FIELDS})
        p = lib.WfMapParams(seed_len=20, max_occ=16, max_mm=4, min_insert=0, max_insert=500)
        gp = lib.WfMapGapParams(max_gap=2)
        assert so.wf_map_pairs_gapped(h, C.byref(rd), C.byref(p), C.byref(gp), C.byref(r), C.byref(g)) == lib.WF_E_STATE
    finally:
        so.wf_free(h)


def hip_runtime():
    """The HIP runtime libwaafle_hip.so is linked against (already loaded with it)."""
    lib.load()
    with open("/proc/self/maps") as fh:
        path = next(l.split()[-1] for l in fh if "libamdhip64" in l)
    return C.CDLL(path)


def test_device_resident_reads_equal_host_reads():
    contigs, r1, r2, P, G, _ = gc.which_mate()
    hip = hip_runtime()
    H2D, D2H = 1, 2
    held = []

    def alloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 16))) == 0
        held.append(p)
        return p

    with mapper.Mapper(*mc.flat(contigs), **kw(P, G)) as m:
        host = run(m, r1, r2)
        try:
            dev = []
            for a in mc.flat(r1) + mc.flat(r2):
                p = alloc(a.nbytes)
                assert hip.hipMemcpy(p, lib.ptr(a), C.c_size_t(a.nbytes), H2D) == 0
                dev.append(p)
            got = {f: np.full(len(r1), 9, dt) for f, dt in mapper.RESULT_FIELDS + mapper.GAP_FIELDS}
            out = {f: alloc(got[f].nbytes) for f in FIELDS}
            for f in FIELDS:                             # stale values the call must overwrite
                assert hip.hipMemcpy(out[f], lib.ptr(got[f]), C.c_size_t(got[f].nbytes), H2D) == 0
            m.map_device(len(r1), *dev, out)
            for f in FIELDS:
                assert hip.hipMemcpy(lib.ptr(got[f]), out[f], C.c_size_t(got[f].nbytes), D2H) == 0
            with pytest.raises(mapper.MapperError):      # max_gap > 0 needs the gap arrays
                m.map_device(len(r1), *dev, {f: out[f] for f, _ in mapper.RESULT_FIELDS})
        finally:
            for p in held:
                hip.hipFree(p)
    assert_equal(got, host)
    assert_equal(host, go.map_pairs_gapped_indexed(contigs, r1, r2, P, G))
    assert (host["flags"] == 1).all()


@pytest.fixture(scope="module")
def medium_case():
    contigs, r1, r2, P, G = gc.medium()
    want = go.as_arrays(go.map_pairs_gapped_indexed(contigs, r1, r2, P, G))
    for a in want.values():
        a.setflags(write=False)
    return contigs, r1, r2, P, G, want


def test_medium_random_set_equals_oracle(medium_case):
    contigs, r1, r2, P, G, want = medium_case
    assert len(contigs) == 20 and len(r1) == 600
    shares = (np.mean((want["contig"] >= 0) & (want["flags"] == 0)), np.mean(want["flags"] == 1),
              np.mean(want["contig"] < 0))
    assert min(shares) >= 0.10, shares                     # every outcome is well represented
    with mapper.Mapper(*mc.flat(contigs), **kw(P, G)) as m:
        assert_equal(run(m, r1, r2), want, "whole")
        assert_equal(run(m, r1, r2), want, "second run")
        for step in (7, 1):
            parts = [run(m, r1[i:i + step], r2[i:i + step]) for i in range(0, len(r1), step)]
            got = {f: np.concatenate([p[f] for p in parts]) for f in FIELDS}
            assert_equal(got, want, "chunks of {}".format(step))


def test_widest_gap_and_seed_limits(medium_case):
    """G = 8 with S = 12 and max_occ = 64: the candidate list and the task count at their
    largest."""
    contigs, r1, r2, _, _, _ = medium_case
    r1, r2 = r1[:150], r2[:150]
    P = mo.params(S=12, max_occ=64)
    want = go.map_pairs_gapped_indexed(contigs, r1, r2, P, 8)
    with mapper.Mapper(*mc.flat(contigs), **kw(P, 8)) as m:
        assert_equal(run(m, r1, r2), want)


def test_planted_indels_map_to_their_origin():
    contigs, r1, r2, P, G, truth = gc.planted()
    assert mc.unique_kmers(contigs, P["S"])
    with mapper.Mapper(*mc.flat(contigs), **kw(P, G)) as m:
        got = run(m, r1, r2)
    t = np.array(truth)
    for j, f in enumerate(("contig", "pos1", "pos2", "strand1", "d1", "d2")):
        assert np.array_equal(got[f].astype(np.int64), t[:, j]), f
    assert not got["mm1"].any() and not got["mm2"].any() and (got["flags"] == 1).all()
    assert (got["k1"] <= t[:, 6]).all() and (got["k2"] <= t[:, 7]).all()
    assert ((got["k1"] > 0) == (t[:, 4] != 0)).all() and ((got["k2"] > 0) == (t[:, 5] != 0)).all()
    assert_equal(got, go.map_pairs_gapped_indexed(contigs, r1, r2, P, G))


# ---------------------------------------------------------------------------
# end to end: waafle_junctions --mapper native --max-gap
# ---------------------------------------------------------------------------

def write_inputs(tmp, contigs, r1, r2, truth):
    names = ["ctg{}".format(i) for i in range(len(contigs))]
    fna, gff = str(tmp / "gap.fna"), str(tmp / "gap.gff")
    with open(fna, "w") as fh:
        for n, s in zip(names, contigs):
            fh.write(">{}\n{}\n".format(n, s.decode()))
    with open(gff, "w") as fh:
        fh.write("##gff-version 3\n")
        for n in names:
            for k, (a, b) in enumerate(((30, 280), (330, 600), (640, 960))):
                fh.write("\t".join([n, "x", "CDS", str(a), str(b), ".", "+-"[k & 1], "0", "ID={}_{}".format(n, k)]) + "\n")
    fq1, fq2 = str(tmp / "gap_1.fq"), str(tmp / "gap_2.fq.gz")
    with open(fq1, "w") as f1, gzip.open(fq2, "wt") as f2:
        for i, (a, b) in enumerate(zip(r1, r2)):
            f1.write("@read{}/1\n{}\n+\n{}\n".format(i, a.decode(), "I" * len(a)))
            f2.write("@read{}/2\n{}\n+\n{}\n".format(i, b.decode(), "I" * len(b)))
    sam = str(tmp / "truth.sam")
    with open(sam, "w") as fh:                          # the planted CIGARs
        for i, (c, p1, p2, _s, d1, d2, k1, k2) in enumerate(truth):
            for p, d, k in ((p1, d1, k1), (p2, d2, k2)):
                fh.write("\t".join(["read{}".format(i), "0", names[c], str(p), "42", mapper._cigar(100, d, k),
                                    "=", "0", "0", "*", "*"]) + "\n")
    return fna, gff, fq1, fq2, sam


def test_junctions_cli_max_gap_end_to_end(tmp_path):
    contigs, r1, r2, P, G, truth = gc.planted()
    fna, gff, fq1, fq2, truth_sam = write_inputs(tmp_path, contigs, r1, r2, truth)
    reads = ["--reads1", fq1, "--reads2", fq2, "--mapper", "native"]
    outs = []
    for k, extra in enumerate((reads + ["--max-gap", "3"], ["--sam", str(tmp_path / "tmp0" / "gap.sam")], reads)):
        out, tmp = tmp_path / "out{}".format(k), tmp_path / "tmp{}".format(k)
        out.mkdir()
        tmp.mkdir()
        junctions.main([fna, gff, "--outdir", str(out), "--tmpdir", str(tmp), "--write-detailed-output"] + extra)
        outs.append(out)
    for name in ("gap.junctions.tsv", "gap.gene_hits.tsv", "gap.site_hits.tsv.gz"):
        opener = gzip.open if name.endswith(".gz") else open
        with opener(str(outs[0] / name), "rb") as a, opener(str(outs[1] / name), "rb") as b:
            first = a.read()
            assert first == b.read() and len(first) > 100, name
    got = (outs[0] / "gap.junctions.tsv").read_text().splitlines()
    want = jo.junction_rows(fna, gff, truth_sam)
    assert got == want
    col = want[0].split("\t").index("JUNCTION_HITS")
    hits = lambda rows_: sum(int(r.split("\t")[col]) for r in rows_[1:])
    ungapped = (outs[2] / "gap.junctions.tsv").read_text().splitlines()
    assert hits(got) > 30 and hits(ungapped) < hits(got)
    cigars = [l.split("\t")[5] for l in (tmp_path / "tmp0" / "gap.sam").read_text().splitlines() if l[0] != "@"]
    assert sum("D" in c for c in cigars) > 20 and sum("I" in c for c in cigars) > 20
