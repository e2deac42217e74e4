"""Search records to the scorer's hit arrays, without the table.

`wf_hits_from_records` (csrc/wf_hits.hip) turns the search's records, in the table's order, into
the hit arrays `wf_genecall` and `wf_score` take, on the device, bit for bit what reading the
written table back would give.  This module binds it and holds the host side that the table's
readers otherwise do: the subjects' taxa and annotations parsed once per subject
(`subject_tables`), the loci made from the gene caller's arrays (`loci_from_genes`), the batch
object `output.render` reads (`HitsBatch`), and `wf_genecall` / `wf_score` on the device arrays.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import engine, inputs, lib as L

RECORD_COLUMNS = (("contig", np.int32), ("subject", np.int32), ("minus", np.uint8), ("qstart", np.int32),
                  ("qspan", np.int32), ("sstart", np.int32), ("sspan", np.int32), ("length", np.int32),
                  ("matches", np.int32))
HIT_FIELDS = (("hit_off", np.int64), ("hit_qlo", np.int32), ("hit_qhi", np.int32), ("hit_taxon", np.int32),
              ("hit_strand", np.int8), ("hit_score", np.float64), ("hit_scov", np.float64),
              ("hit_sysmask", np.uint32), ("hit_key", np.uint32))


def record_columns(rec, order=None):
    """The nine columns of wf_hit_records from the search's records (search.RECORD_FIELDS or
    GAP_RECORD_FIELDS), those of `order` in that order; an ungapped record has qspan = sspan =
    length."""
    pick = (lambda a: a) if order is None else (lambda a: a[order])
    out = {}
    for f, dt in RECORD_COLUMNS:
        src = rec[f] if f in rec else rec["length"]
        out[f] = np.ascontiguousarray(pick(np.asarray(src)), dtype=dt)
    return out


# ---------------------------------------------------------------------------
# the subjects
# ---------------------------------------------------------------------------

@dataclass
class SubjectTables:
    """Per subject (the rows of subjects not asked for stay empty): `taxa` the taxon name or
    None, `sysmask` the annotation systems present (bit s: systems[s]) and `value_ids`
    [n_subjects, max(1, systems)] the index of its value in `values[s]`, -1 absent."""
    taxa: list
    systems: list
    sysmask: np.ndarray
    value_ids: np.ndarray
    values: list = field(default_factory=list)

    def taxon_ids(self, tax):
        """int32 per subject: the id `tax` (TaxonomyTables) gives its taxon, -1 where none"""
        return np.array([-1 if t is None else tax.index[t] for t in self.taxa], dtype=np.int32)


def subject_tables(ids, used=None):
    """Taxon and annotations of the subjects `used` (indices into `ids`; default: all), each id
    parsed once, with the rules and error texts of inputs.split_sseqids; the systems are those
    of the subjects asked for, sorted, as the table's reader derives them from the hits."""
    n = len(ids)
    used = list(range(n)) if used is None else [int(g) for g in used]
    taxa_u, annots_u = inputs.split_sseqids([ids[g] for g in used])
    systems = sorted({s for d in annots_u if d for s in d})
    if len(systems) > 32:
        raise inputs.InputError("more than 32 annotation systems")
    bit = {s: b for b, s in enumerate(systems)}
    taxa = [None] * n
    sysmask = np.zeros(n, dtype=np.uint32)
    value_ids = np.full((n, max(1, len(systems))), -1, dtype=np.int32)
    values = [[] for _ in systems]
    index = [dict() for _ in systems]
    for g, t, d in zip(used, taxa_u, annots_u):
        taxa[g] = t
        m = 0
        for s, v in (d or {}).items():
            b = bit[s]
            m |= 1 << b
            vi = index[b].get(v)
            if vi is None:
                vi = index[b][v] = len(values[b])
                values[b].append(v)
            value_ids[g, b] = vi
        sysmask[g] = m
    return SubjectTables(taxa, systems, sysmask, value_ids, values)


# ---------------------------------------------------------------------------
# wf_hits_from_records
# ---------------------------------------------------------------------------

def _call(so, h, cols, qlen, slen, taxon, sysmask, min_scov, out_ptrs, device_resident):
    held = [np.ascontiguousarray(cols[f], dtype=dt) for f, dt in RECORD_COLUMNS]
    n = len(held[0])
    tabs = [np.ascontiguousarray(qlen, dtype=np.int64), np.ascontiguousarray(slen, dtype=np.int64),
            np.ascontiguousarray(taxon, dtype=np.int32), np.ascontiguousarray(sysmask, dtype=np.uint32)]
    if not (len(tabs[1]) == len(tabs[2]) == len(tabs[3])):
        raise ValueError("the subject tables differ in length")
    r = L.WfHitRecords(n, *[L.ptr(a) if n else None for a in held])
    t = L.WfHitTables(n_contigs=len(tabs[0]), n_subjects=len(tabs[1]), qlen=L.ptr(tabs[0]), slen=L.ptr(tabs[1]),
                      subject_taxon=L.ptr(tabs[2]), subject_sysmask=L.ptr(tabs[3]), min_scov=float(min_scov))
    o = L.WfHitsOut(device_resident=device_resident, **out_ptrs)
    rc = so.wf_hits_from_records(h, C.byref(r), C.byref(t), C.byref(o))
    if rc == L.WF_OK and device_resident:
        rc = so.wf_synchronize(h)            # the host columns above are read until here
    if rc != L.WF_OK:
        raise L.WaafleHipError(rc, so.wf_last_error(h).decode())


def hits_host(so, h, cols, qlen, slen, taxon, sysmask, min_scov, out=None):
    """wf_hits_from_records into host arrays ({field: array}, HIT_FIELDS); `out`: arrays to
    write into (they keep what they hold when the call is refused)."""
    n, N = len(cols["contig"]), len(qlen)
    if out is None:
        out = {f: np.zeros(N + 1 if f == "hit_off" else n, dt) for f, dt in HIT_FIELDS}
    _call(so, h, cols, qlen, slen, taxon, sysmask, min_scov, {f: L.ptr(out[f]) for f, _ in HIT_FIELDS}, 0)
    return out


class DeviceArray:
    """`count` items of `dtype` in device memory, allocated through the HIP runtime the library
    is linked against (no second runtime in the process); freed with `free` or with the object."""

    def __init__(self, hip, count, dtype, zero=False):
        self.hip, self.dtype, self.count = hip, np.dtype(dtype), int(count)
        self.nbytes = max(self.count, 1) * self.dtype.itemsize
        p = C.c_void_p()
        _hip_check(hip, hip.hipMalloc(C.byref(p), C.c_size_t(self.nbytes)), "hipMalloc")
        self.ptr = p
        if zero:
            _hip_check(hip, hip.hipMemset(p, 0, C.c_size_t(self.nbytes)), "hipMemset")

    @classmethod
    def of(cls, hip, a):
        """a host array's copy"""
        a = np.ascontiguousarray(a)
        d = cls(hip, len(a), a.dtype)
        if len(a):
            _hip_check(hip, hip.hipMemcpy(d.ptr, L.ptr(a), C.c_size_t(a.nbytes), 1), "hipMemcpy")
        return d

    def host(self, n=None):
        """the first n items (default: all) on the host; the caller has synchronised the
        stream that wrote them"""
        out = np.zeros(self.count if n is None else int(n), self.dtype)
        if len(out):
            _hip_check(self.hip, self.hip.hipMemcpy(L.ptr(out), self.ptr, C.c_size_t(out.nbytes), 2), "hipMemcpy")
        return out

    def free(self):
        if self.ptr:
            self.hip.hipFree(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _hip_check(hip, rc, what):
    if rc != 0:
        raise L.WaafleHipError(L.WF_E_HIP, "{} failed with HIP error {}".format(what, rc))


def hip_runtime(device=0):
    """The HIP runtime libwaafle_hip.so is linked against (loaded with it), with `device`
    current for this thread."""
    L.load()
    with open("/proc/self/maps") as fh:
        path = next((ln.split()[-1] for ln in fh if "libamdhip64" in ln), None)
    if path is None:
        raise ImportError("libwaafle_hip.so brought no HIP runtime with it")
    hip = C.CDLL(path)
    for fn in (hip.hipMalloc, hip.hipMemset, hip.hipMemcpy, hip.hipFree, hip.hipSetDevice, hip.hipDeviceSynchronize):
        fn.restype = C.c_int
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    _hip_check(hip, hip.hipSetDevice(int(device)), "hipSetDevice")
    return hip


def device_arrays(hip, n, n_contigs):
    """Uninitialised device arrays for HIT_FIELDS."""
    return {f: DeviceArray(hip, n_contigs + 1 if f == "hit_off" else n, dt) for f, dt in HIT_FIELDS}


def hits_device(so, h, cols, qlen, slen, taxon, sysmask, min_scov, hip, out=None):
    """wf_hits_from_records into device arrays ({field: DeviceArray}); returns after the
    context's stream has run."""
    if out is None:
        out = device_arrays(hip, len(cols["contig"]), len(qlen))
    _call(so, h, cols, qlen, slen, taxon, sysmask, min_scov, {f: out[f].ptr for f, _ in HIT_FIELDS}, 1)
    return out


def to_host(d, n, n_contigs):
    """{field: numpy array} of the device arrays of hits_device"""
    return {f: d[f].host(n_contigs + 1 if f == "hit_off" else n) for f, _ in HIT_FIELDS}


# ---------------------------------------------------------------------------
# gene calls and loci
# ---------------------------------------------------------------------------

def genecall_device(so, h, d, n_contigs, n_hits, min_overlap, min_scov, min_gene_length):
    """wf_genecall on the device hit arrays, one group per contig (a contig without hits is an
    empty group): (n_genes [n_contigs], gene_start, gene_stop, gene_strand [n_hits]) on the host."""
    hip = d["hit_off"].hip
    res = [DeviceArray(hip, n_contigs, np.int32, zero=True), DeviceArray(hip, n_hits, np.int32, zero=True),
           DeviceArray(hip, n_hits, np.int32, zero=True), DeviceArray(hip, n_hits, np.int8, zero=True)]
    _hip_check(hip, hip.hipDeviceSynchronize(), "hipDeviceSynchronize")      # the zeroing is done
    b = L.WfGcBatch(n_groups=n_contigs, device_resident=1, n_hits=n_hits, hit_off=d["hit_off"].ptr,
                    hit_qlo=d["hit_qlo"].ptr, hit_qhi=d["hit_qhi"].ptr, hit_strand=d["hit_strand"].ptr,
                    hit_scov=d["hit_scov"].ptr)
    prm = L.WfGcParams(min_overlap=min_overlap, min_scov=min_scov, min_gene_length=min_gene_length, stranded=0)
    r = L.WfGcResult(n_genes=res[0].ptr, gene_start=res[1].ptr, gene_stop=res[2].ptr, gene_strand=res[3].ptr)
    rc = so.wf_genecall(h, C.byref(b), C.byref(prm), C.byref(r))
    if rc == L.WF_OK:
        rc = so.wf_synchronize(h)
    if rc != L.WF_OK:
        raise L.WaafleHipError(rc, so.wf_last_error(h).decode())
    out = tuple(a.host() for a in res)
    for a in res:
        a.free()
    return out


def gene_lists(hit_off, n_genes, gene_start, gene_stop, gene_strand):
    """Per contig with hits, in contig order: (contig, [(start, stop, strand char), ...]), as
    genecaller.call_genes lists the groups of the table."""
    out = []
    for c in np.flatnonzero(np.diff(hit_off) > 0).tolist():
        o, k = int(hit_off[c]), int(n_genes[c])
        out.append((c, [(int(gene_start[o + i]), int(gene_stop[o + i]), "-" if gene_strand[o + i] else "+")
                        for i in range(k)]))
    return out


def loci_from_genes(genes, min_gene_length):
    """{contig: kept loci} as inputs.read_loci reads the GFF genecaller.write_gff writes of
    `genes` (gene_lists): a contig with a row is listed, and the length filter runs again."""
    return {c: [g for g in gl if abs(g[1] - g[0]) + 1 >= min_gene_length] for c, gl in genes if gl}


# ---------------------------------------------------------------------------
# the batch
# ---------------------------------------------------------------------------

@dataclass
class HitsBatch:
    """What output.render and the scoring call read of an inputs.HostBatch; the hit arrays
    themselves stay on the device."""
    contig_names: list
    contig_lengths: np.ndarray
    hit_off: np.ndarray
    loc_off: np.ndarray
    loc_start: np.ndarray
    loc_end: np.ndarray
    loc_strand: np.ndarray
    loc_codes: list
    systems: list
    annot_value_ids: np.ndarray
    annot_values: list
    loci_fields: object = None
    hit_group: object = None

    n_contigs = inputs.HostBatch.n_contigs
    n_hits = inputs.HostBatch.n_hits
    n_loci = inputs.HostBatch.n_loci
    max_hits = inputs.HostBatch.max_hits
    max_loci = inputs.HostBatch.max_loci


def make_batch(contig_names, contig_lengths, hit_off, loci, subjects, hit_subject):
    """loci: {contig: [(start, end, strand), ...]} (inputs.read_loci, loci_from_genes);
    subjects: SubjectTables; hit_subject: the records' subject column, in hit order."""
    N = len(contig_names)
    counts = np.array([len(loci.get(c, ())) for c in range(N)], dtype=np.int64)
    loc_off = np.zeros(N + 1, dtype=np.int64)
    np.cumsum(counts, out=loc_off[1:])
    flat = [r for c in range(N) for r in loci.get(c, ())]
    loc_start = np.array([r[0] for r in flat], dtype=np.int64)
    loc_end = np.array([r[1] for r in flat], dtype=np.int64)
    for arr, what in ((loc_start, "gff start"), (loc_end, "gff end")):
        if len(arr) and (arr.min() < -(2 ** 31) or arr.max() >= 2 ** 31):
            raise inputs.InputError("{} outside int32".format(what))
    return HitsBatch(
        contig_names=list(contig_names), contig_lengths=np.asarray(contig_lengths, dtype=np.int64),
        hit_off=np.asarray(hit_off, dtype=np.int64), loc_off=loc_off, loc_start=loc_start.astype(np.int32),
        loc_end=loc_end.astype(np.int32),
        loc_strand=np.array([inputs.STRAND_CODE.get(r[2], 2) for r in flat], dtype=np.int8),
        loc_codes=["{}:{}:{}".format(*r) for r in flat], systems=list(subjects.systems),
        annot_value_ids=subjects.value_ids[np.asarray(hit_subject, dtype=np.int64)],
        annot_values=subjects.values)


def host_batch(batch, d):
    """The inputs.HostBatch of a HitsBatch and its device hit arrays, copied to the host."""
    a = to_host(d, batch.n_hits, batch.n_contigs)
    hb = inputs.HostBatch(
        contig_names=batch.contig_names, contig_lengths=batch.contig_lengths, hit_off=batch.hit_off,
        hit_qlo=a["hit_qlo"], hit_qhi=a["hit_qhi"], hit_taxon=a["hit_taxon"], hit_strand=a["hit_strand"],
        hit_score=a["hit_score"], hit_scov=a["hit_scov"], hit_sysmask=a["hit_sysmask"], loc_off=batch.loc_off,
        loc_start=batch.loc_start, loc_end=batch.loc_end, loc_strand=batch.loc_strand, loc_codes=batch.loc_codes,
        systems=batch.systems, annot_value_ids=batch.annot_value_ids, annot_values=batch.annot_values)
    return hb


def score_device(scorer, batch, d, params):
    """wf_score (engine.GpuScorer `scorer`, its taxonomy set) on the device hit arrays `d` of
    `batch`, with their packed hit_key, which must have been made with params' min_scov.
    A batch one call refuses as too big (WF_E_TOOBIG) is copied to the host and scored in
    contig halves by GpuScorer.score.  Returns engine.Results on the host."""
    hip = d["hit_off"].hip
    N, NH, NL, S = batch.n_contigs, batch.n_hits, batch.n_loci, len(batch.systems)
    res = engine.Results.empty(N, NH, NL, S)
    loc = {f: DeviceArray.of(hip, getattr(batch, f)) for f in ("loc_off", "loc_start", "loc_end", "loc_strand")}
    # zeroed as engine.Results.empty: what a pass leaves unwritten reads the same every run
    out = {f: DeviceArray(hip, len(getattr(res, f)), getattr(res, f).dtype, zero=True) for f, _ in L.WfResult._fields_}
    _hip_check(hip, hip.hipDeviceSynchronize(), "hipDeviceSynchronize")
    bs = L.WfBatch(n_contigs=N, n_systems=S, n_hits=NH, n_loci=NL, max_hits=batch.max_hits, max_loci=batch.max_loci,
                   device_resident=1, _pad=0, **{f: d[f].ptr for f, _ in HIT_FIELDS},
                   **{f: a.ptr for f, a in loc.items()})
    ps = engine.params_struct(params)
    rs = L.WfResult(**{f: a.ptr for f, a in out.items()})
    try:
        rc = scorer.lib.wf_score(scorer.h, C.byref(bs), C.byref(ps), C.byref(rs))
        if rc == L.WF_E_TOOBIG:
            return scorer.score(host_batch(batch, d), params)
        if rc == L.WF_OK:
            rc = scorer.lib.wf_synchronize(scorer.h)
        if rc != L.WF_OK:
            raise L.WaafleHipError(rc, scorer.lib.wf_last_error(scorer.h).decode())
        for f, a in out.items():
            setattr(res, f, a.host())
    finally:
        for a in list(loc.values()) + list(out.values()):
            a.free()
    bad = np.nonzero(res.status)[0]
    if len(bad):                                     # as the host-resident call reports it
        c = int(bad[0])
        err = L.WaafleHipError(int(res.status[c]), "contig {} failed with status {}".format(c, int(res.status[c])))
        err.contigs, err.results = bad, res
        raise err
    return res
