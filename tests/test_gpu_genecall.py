"""GPU: wf_genecall through the C-ABI on the cases of genecall_cases.py, against the oracle
(oracle.genecaller_oracle.overlap_intervals with its scov and length filters).  Every
comparison is exact: gene count, starts, stops and strands of every group, in order."""
import ctypes as C

import numpy as np
import pytest

import genecall_cases as gcs
from waafle_amd import genecaller, lib

pytestmark = pytest.mark.gpu

CASES = [c for c in gcs.all_cases() if c.refused_group is None]


def hip_runtime():
    """The HIP runtime libwaafle_hip.so is linked against (already loaded with it)."""
    lib.load()
    with open("/proc/self/maps") as fh:
        path = next(l.split()[-1] for l in fh if "libamdhip64" in l)
    return C.CDLL(path)


def run(case):
    off, qs, qe, strand, scov = case.arrays()
    return genecaller.call_genes_arrays(off, qs, qe, strand, scov, case.min_overlap,
                                        case.min_gene_length, case.min_scov)


def assert_genes(case, got):
    want = gcs.oracle_of(case.name)
    bad = [g for g in range(len(want)) if got[g] != want[g]]
    for g in bad[:4]:
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(got[g], want[g])) if a != b][:3]
        print(case.name, "group", g, "genes", len(got[g]), "want", len(want[g]), "first diffs", diff)
    assert not bad, "{}: {} of {} groups differ from the oracle".format(case.name, len(bad), len(want))


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_matches_oracle(case):
    assert_genes(case, gcs.genes_of(case, *run(case)))


def test_more_than_4096_intervals_is_refused():
    """4097 passing intervals in group 2: WF_E_NOMEM naming the group, not a fault."""
    case = [c for c in gcs.all_cases() if c.refused_group is not None][0]
    with pytest.raises(lib.WaafleHipError) as exc:
        run(case)
    assert exc.value.code == lib.WF_E_NOMEM
    assert exc.value.msg == "contig group {} has more than 4096 intervals".format(case.refused_group)


def test_many_groups_host_and_device_resident():
    """Family G: 10 000 groups in one call (cap 4096, dozens of groups per block, LDS reused
    from a large group to a small one), with host arrays and again with device pointers."""
    case = gcs.family_g()
    host = run(case)
    assert_genes(case, gcs.genes_of(case, *host))
    off, qs, qe, strand, scov = case.arrays()
    G, NH = len(off) - 1, int(off[-1])
    so = lib.load()
    hip = hip_runtime()
    H2D, D2H = 1, 2
    held = []

    def alloc(nbytes):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(max(nbytes, 16))) == 0
        held.append(p)
        return p

    res = [np.full(G, -1, np.int32), np.full(NH, -1, np.int32), np.full(NH, -1, np.int32),
           np.full(NH, -1, np.int8)]
    h = C.c_void_p()
    assert so.wf_init(0, C.byref(h)) == lib.WF_OK
    try:
        dev = []
        for a in (off, qs, qe, strand, scov) + tuple(res):       # results start as -1
            p = alloc(a.nbytes)
            assert hip.hipMemcpy(p, lib.ptr(a), C.c_size_t(a.nbytes), H2D) == 0
            dev.append(p)
        b = lib.WfGcBatch(n_groups=G, device_resident=1, n_hits=NH, hit_off=dev[0], hit_qlo=dev[1],
                          hit_qhi=dev[2], hit_strand=dev[3], hit_scov=dev[4])
        prm = lib.WfGcParams(min_overlap=case.min_overlap, min_scov=case.min_scov,
                             min_gene_length=case.min_gene_length, stranded=0)
        r = lib.WfGcResult(n_genes=dev[5], gene_start=dev[6], gene_stop=dev[7], gene_strand=dev[8])
        rc = so.wf_genecall(h, C.byref(b), C.byref(prm), C.byref(r))
        assert rc == lib.WF_OK, so.wf_last_error(h).decode()
        assert hip.hipDeviceSynchronize() == 0
        for a, p in zip(res, dev[5:]):
            assert hip.hipMemcpy(lib.ptr(a), p, C.c_size_t(a.nbytes), D2H) == 0
    finally:
        so.wf_free(h)
        for p in held:
            hip.hipFree(p)
    assert np.array_equal(res[0], host[0])
    assert gcs.genes_of(case, *res) == gcs.genes_of(case, *host)
    # slots past a group's genes are not written
    used = np.zeros(NH, bool)
    for o, k in zip(off[:-1].tolist(), res[0].tolist()):
        used[o:o + k] = True
    assert (res[1][~used] == -1).all() and (res[2][~used] == -1).all() and (res[3][~used] == -1).all()
