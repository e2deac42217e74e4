"""wf_map_index / wf_map_pairs (wf_map.hip) on the GPU against the CPU oracles of the mapping
rule (tests/map_oracle.py): every result field of every pair must be equal.  Hand-built
edge batches against both oracles, a seeded medium set against the dictionary oracle (whole,
in chunks of 7 and of 1, twice, and after an index replacement), planted error-free pairs
against their origin, and `waafle_junctions --mapper native` end to end."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import map_cases as mc
import map_oracle as mo
from oracle import junctions_oracle as jo
from waafle_amd import junctions, lib, mapper

pytestmark = pytest.mark.gpu

FIELDS = [f for f, _ in mapper.RESULT_FIELDS]


def kw(P):
    return dict(seed_length=P["S"], max_seed_hits=P["max_occ"], max_mismatches=P["max_mm"],
                min_insert=P["min_insert"], max_insert=P["max_insert"])


def run(m, r1, r2):
    return m.map(*mc.flat(r1), *mc.flat(r2))


def assert_equal(got, want, what=""):
    want = mo.as_arrays(want) if not isinstance(want, dict) else want
    for f in FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert got[f].dtype == want[f].dtype and len(bad) == 0, \
            "{} {}: pair {} got {} want {}".format(what, f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])


@pytest.mark.parametrize("name", sorted(mc.HAND_BUILT))
def test_hand_built_cases_equal_both_oracles(name):
    contigs, r1, r2, P, aligned = mc.HAND_BUILT[name]()
    want = mo.map_pairs_brute(contigs, r1, r2, P)
    assert want == mo.map_pairs_indexed(contigs, r1, r2, P)
    with mapper.Mapper(*mc.flat(contigs), **kw(P)) as m:
        got = run(m, r1, r2)
    assert_equal(got, want, name)
    assert (got["contig"] >= 0).tolist() == aligned


def test_flags_of_both_orientations():
    contigs, r1, r2, P, _ = mc.orientation()
    with mapper.Mapper(*mc.flat(contigs), **kw(P)) as m:
        got = run(m, r1[:2], r2[:2])
    recs = mapper.sam_records(["a", "b"], [len(r) for r in r1[:2]], [len(r) for r in r2[:2]], got,
                              ["c0", "c1"])
    assert [r.split("\t")[1] for r in recs] == ["99", "147", "83", "163"]


def test_read_of_513_bases_is_refused_not_mapped():
    contigs, r1, r2, P, _ = mc.read_lengths()
    long1, long2 = mc.fr_pair(contigs[0], 30, 513, 563, 513)
    with mapper.Mapper(*mc.flat(contigs), **kw(P)) as m:
        for a, b in ((r1 + [long1], r2 + [long2]), (r1 + [long1], r2 + [r2[0]]), ([r1[0]], [long2])):
            with pytest.raises(lib.WaafleHipError) as exc:
                run(m, a, b)
            assert exc.value.code == lib.WF_E_BADINPUT
        assert_equal(run(m, r1, r2), mo.map_pairs_indexed(contigs, r1, r2, P))   # still usable


def test_parameter_checks():
    contigs, r1, r2, P, _ = mc.min_insert()
    with mapper.Mapper(*mc.flat(contigs), **kw(P)) as m:
        for field, value in (("seed_len", 24), ("max_occ", 8), ("max_mm", 33), ("seed_len", 11),
                             ("max_insert", 1)):
            p = lib.WfMapParams.from_buffer_copy(m.params)
            setattr(p, field, value)
            with pytest.raises(lib.WaafleHipError) as exc:
                m.map(*mc.flat(r1), *mc.flat(r2), params=p)
            assert exc.value.code == lib.WF_E_BADINPUT
        empty = np.zeros(1, np.int64)
        none = m.map(np.zeros(0, np.uint8), empty, np.zeros(0, np.uint8), empty)
        assert len(none["contig"]) == 0
    so = lib.load()
    h = C.c_void_p()
    assert so.wf_init(0, C.byref(h)) == lib.WF_OK
    try:
        seq, off = mc.flat(r1)
        rd = lib.WfMapReads(n_pairs=1, seq1=lib.ptr(seq), off1=lib.ptr(off), seq2=lib.ptr(seq), off2=lib.ptr(off))
        out = {f: np.zeros(1, dt) for f, dt in mapper.RESULT_FIELDS}
        r = lib.WfMapResult(**{f: lib.ptr(out[f]) for f in FIELDS})
        p = lib.WfMapParams(seed_len=20, max_occ=16, max_mm=4, min_insert=0, max_insert=500)
        assert so.wf_map_pairs(h, C.byref(rd), C.byref(p), C.byref(r)) == lib.WF_E_STATE
        big = np.array([0, (1 << 31)], np.int64)                   # refused before it is read
        c = lib.WfMapContigs(n_contigs=1, seq=lib.ptr(seq), off=lib.ptr(big))
        assert so.wf_map_index(h, C.byref(c), C.byref(p)) == lib.WF_E_TOOBIG
    finally:
        so.wf_free(h)


def hip_runtime():
    """The HIP runtime libwaafle_hip.so is linked against (already loaded with it)."""
    lib.load()
    with open("/proc/self/maps") as fh:
        path = next(l.split()[-1] for l in fh if "libamdhip64" in l)
    return C.CDLL(path)


def test_device_resident_reads_equal_host_reads():
    contigs, r1, r2, P, _ = mc.orientation()
    hip = hip_runtime()
    H2D, D2H = 1, 2
    held = []

    def alloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 16))) == 0
        held.append(p)
        return p

    with mapper.Mapper(*mc.flat(contigs), **kw(P)) as m:
        host = run(m, r1, r2)
        try:
            dev = []
            for a in mc.flat(r1) + mc.flat(r2):
                p = alloc(a.nbytes)
                assert hip.hipMemcpy(p, lib.ptr(a), C.c_size_t(a.nbytes), H2D) == 0
                dev.append(p)
            got = {f: np.full(len(r1), 9, dt) for f, dt in mapper.RESULT_FIELDS}
            out = {f: alloc(got[f].nbytes) for f in FIELDS}
            m.map_device(len(r1), *dev, out)
            for f in FIELDS:
                assert hip.hipMemcpy(lib.ptr(got[f]), out[f], C.c_size_t(got[f].nbytes), D2H) == 0
        finally:
            for p in held:
                hip.hipFree(p)
    assert_equal(got, host)
    assert_equal(host, mo.map_pairs_indexed(contigs, r1, r2, P))


@pytest.fixture(scope="module")
def medium_case():
    contigs, r1, r2, P = mc.medium()
    want = mo.as_arrays(mo.map_pairs_indexed(contigs, r1, r2, P))
    for a in want.values():
        a.setflags(write=False)
    return contigs, r1, r2, P, want


def test_medium_random_set_equals_oracle(medium_case):
    contigs, r1, r2, P, want = medium_case
    assert 40_000 < sum(len(c) for c in contigs) < 100_000 and len(r1) == 2000
    aligned = float(np.mean(want["contig"] >= 0))
    assert 0.3 < aligned < 0.98                           # both outcomes are well represented
    with mapper.Mapper(*mc.flat(contigs), **kw(P)) as m:
        assert_equal(run(m, r1, r2), want, "whole")
        assert_equal(run(m, r1, r2), want, "second run")
        for step in (7, 1):
            parts = [run(m, r1[i:i + step], r2[i:i + step]) for i in range(0, len(r1), step)]
            got = {f: np.concatenate([p[f] for p in parts]) for f in FIELDS}
            assert_equal(got, want, "chunks of {}".format(step))


@pytest.mark.parametrize("S,max_occ,max_mm", [(12, 64, 4), (32, 1, 8), (25, 5, 0), (31, 64, 32)])
def test_other_seed_lengths_and_limits(medium_case, S, max_occ, max_mm):
    """The ends of the parameter ranges: 24- and 64-bit keys, the candidate list at its
    largest (64 * 64 entries, more LDS than the default limit of a workgroup)."""
    contigs, r1, r2, _, _ = medium_case
    r1, r2 = r1[:400], r2[:400]
    P = mo.params(S=S, max_occ=max_occ, max_mm=max_mm)
    want = mo.map_pairs_indexed(contigs, r1, r2, P)
    with mapper.Mapper(*mc.flat(contigs), **kw(P)) as m:
        assert_equal(run(m, r1, r2), want)


def test_second_index_replaces_the_first(medium_case):
    contigs, r1, r2, P, want = medium_case
    other, o1, o2, _, truth = mc.planted()
    with mapper.Mapper(*mc.flat(contigs), **kw(P)) as m:
        assert_equal(run(m, r1[:200], r2[:200]), {f: want[f][:200] for f in FIELDS})
        m.index(*mc.flat(other))
        assert_equal(run(m, o1, o2), truth, "after re-index")
        assert (run(m, r1[:200], r2[:200])["contig"] == -1).all()
        m.index(*mc.flat(contigs))
        assert_equal(run(m, r1[:200], r2[:200]), {f: want[f][:200] for f in FIELDS})


def test_planted_error_free_pairs_map_to_their_origin():
    contigs, r1, r2, P, truth = mc.planted()
    assert mc.unique_kmers(contigs, P["S"])
    with mapper.Mapper(*mc.flat(contigs), **kw(P)) as m:
        got = run(m, r1, r2)
    assert_equal(got, truth)
    assert not got["mm1"].any() and not got["mm2"].any()


def test_empty_and_degenerate_contig_sets():
    reads = [b"ACGT" * 10], [b"ACGT" * 10]
    with mapper.Mapper(np.zeros(0, np.uint8), np.zeros(1, np.int64)) as m:
        assert run(m, *reads)["contig"].tolist() == [-1]
        m.index(*mc.flat([b"", b"ACGTACGTAC", b"N" * 70, b""]))     # no S-mer at all
        assert run(m, *reads)["contig"].tolist() == [-1]


# ---------------------------------------------------------------------------
# end to end: waafle_junctions --mapper native
# ---------------------------------------------------------------------------

def write_inputs(tmp, contigs, r1, r2, truth):
    names = ["ctg{}".format(i) for i in range(len(contigs))]
    fna, gff = str(tmp / "e2e.fna"), str(tmp / "e2e.gff")
    with open(fna, "w") as fh:
        for n, s in zip(names, contigs):
            s = s.decode()
            fh.write(">{} len={}\n".format(n, len(s)))
            fh.write("\n".join(s[i:i + 70] for i in range(0, len(s), 70)) + "\n")
    with open(gff, "w") as fh:
        fh.write("##gff-version 3\n")
        for n, s in zip(names, contigs):
            for k, (a, b) in enumerate(((30, 280), (330, 600), (640, 960))):
                fh.write("\t".join([n, "x", "CDS", str(a), str(b), ".", "+-"[k & 1], "0", "ID={}_{}".format(n, k)]) + "\n")
    fq1, fq2 = str(tmp / "e2e_1.fq"), str(tmp / "e2e_2.fq.gz")
    with open(fq1, "w") as f1, gzip.open(fq2, "wt") as f2:
        for i, (a, b) in enumerate(zip(r1, r2)):
            f1.write("@read{}/1\n{}\n+\n{}\n".format(i, a.decode(), "I" * len(a)))
            f2.write("@read{}/2 mate\n{}\n+\n{}\n".format(i, b.decode(), "I" * len(b)))
    sam = str(tmp / "truth.sam")
    with open(sam, "w") as fh:
        for i, (c, p1, p2, *_rest) in enumerate(truth):
            for p in (p1, p2):
                fh.write("\t".join(["read{}".format(i), "0", names[c], str(p), "42", "100M", "=", "0", "0",
                                    "*", "*"]) + "\n")
    return fna, gff, fq1, fq2, sam


def test_junctions_cli_native_mapper_end_to_end(tmp_path):
    contigs, r1, r2, P, truth = mc.planted()
    fna, gff, fq1, fq2, truth_sam = write_inputs(tmp_path, contigs, r1, r2, truth)
    outs = []
    for k, extra in enumerate((["--reads1", fq1, "--reads2", fq2, "--mapper", "native"],
                               ["--sam", str(tmp_path / "tmp0" / "e2e.sam")])):
        out, tmp = tmp_path / "out{}".format(k), tmp_path / "tmp{}".format(k)
        out.mkdir()
        tmp.mkdir()
        junctions.main([fna, gff, "--outdir", str(out), "--tmpdir", str(tmp), "--write-detailed-output"] + extra)
        outs.append(out)
    assert os.path.exists(str(tmp_path / "tmp0" / "e2e.sam"))
    for name in ("e2e.junctions.tsv", "e2e.gene_hits.tsv", "e2e.site_hits.tsv.gz"):
        opener = gzip.open if name.endswith(".gz") else open
        with opener(str(outs[0] / name), "rb") as a, opener(str(outs[1] / name), "rb") as b:
            first = a.read()
            assert first == b.read() and len(first) > 100, name
    rows = (outs[0] / "e2e.junctions.tsv").read_text().splitlines()
    want = jo.junction_rows(fna, gff, truth_sam)
    col = want[0].split("\t").index("JUNCTION_HITS")
    assert [r.split("\t")[col] for r in rows] == [r.split("\t")[col] for r in want]
    assert rows == want
    assert sum(int(r.split("\t")[col]) for r in rows[1:]) > 50
    # --resume: an existing SAM file is used, not mapped again
    sam0 = tmp_path / "tmp0" / "e2e.sam"
    kept = "\n".join(sam0.read_text().splitlines()[:-200]) + "\n"
    sam0.write_text(kept)
    out2 = tmp_path / "out2"
    out2.mkdir()
    junctions.main([fna, gff, "--outdir", str(out2), "--tmpdir", str(tmp_path / "tmp0"), "--reads1", fq1,
                    "--reads2", fq2, "--mapper", "native", "--resume"])
    assert sam0.read_text() == kept
    assert (out2 / "e2e.junctions.tsv").read_text() != (outs[0] / "e2e.junctions.tsv").read_text()
