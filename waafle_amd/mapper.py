"""Built-in paired-read mapper for `waafle_junctions --mapper native` (wf_map.hip).

A deterministic seed-and-verify ungapped mapper (DESIGN.md §11 states the rule): enough for
waafle_junctions, which only uses each mate's RNAME, POS and POS + cigar_length - 1.  It is
not a bowtie2 clone: no affine-gap alignments, no soft clipping, no MAPQ, no random
tie-breaks.  With max_gap > 0 the pairs left unaligned get a second pass in which each mate
may carry one insertion or deletion of at most max_gap bases (wf_map_pairs_gapped).

Host side (this module): the FASTA sequence reader, the paired FASTQ reader (4-line records,
plain or .gz, streamed in blocks), the calls into wf_map_index / wf_map_pairs and the SAM
writer (the record shape of `bowtie2 --no-mixed --no-discordant`).
"""
from __future__ import annotations

import ctypes as C
import gzip
import itertools

import numpy as np

from . import inputs, lib as L

DEFAULTS = dict(seed_length=20, max_seed_hits=16, max_mismatches=4, min_insert=0, max_insert=500)
MAX_READ = 512
CHUNK_PAIRS = 1 << 20


class MapperError(inputs.InputError):
    pass


def _open(path):
    return gzip.open(path, "rb") if str(path).endswith(".gz") else open(path, "rb")


# ---------------------------------------------------------------------------
# readers
# ---------------------------------------------------------------------------

def read_fasta(path):
    """(names, seq, off): the contigs' bases concatenated (uint8) and their int64 offsets.
    Names and lengths as inputs.read_contig_lengths; a repeated name is an error here."""
    names, chunks, sizes = [], [], []
    with _open(path) as fh:
        for line in fh:
            line = line.strip()
            if not line:
                raise MapperError("blank line in {} (upstream raises IndexError)".format(path))
            if line[:1] == b">":
                parts = line[1:].split()
                if not parts:
                    raise MapperError("empty FASTA header in {}".format(path))
                names.append(parts[0].decode())
                sizes.append(0)
            else:
                if not names:
                    raise MapperError("sequence before the first FASTA header in {}".format(path))
                chunks.append(line)
                sizes[-1] += len(line)
    if len(set(names)) != len(names):
        raise MapperError("repeated contig name in {}".format(path))
    seq = np.frombuffer(b"".join(chunks), dtype=np.uint8)
    off = np.zeros(len(names) + 1, np.int64)
    np.cumsum(sizes, out=off[1:])
    return names, seq, off


def _gather(buf, starts, lens):
    """buf[starts[i] : starts[i] + lens[i]] for every i, concatenated, and the offsets."""
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    idx = np.arange(int(off[-1]), dtype=np.int64) + np.repeat(starts - off[:-1], lens)
    return buf[idx], off


class FastqBlock:
    """Records of one block: names (bytes, offsets), bases (uint8, offsets)."""
    __slots__ = ("name", "name_off", "seq", "off")

    def __len__(self):
        return len(self.off) - 1

    def qname(self, i):
        return self.name[self.name_off[i]:self.name_off[i + 1]].tobytes().decode()


def parse_fastq_block(data, path="<fastq>"):
    """The 4-line records of `data` (bytes; whole records only)."""
    if not data.endswith(b"\n"):
        data += b"\n"
    buf = np.frombuffer(data, dtype=np.uint8)
    nl = np.flatnonzero(buf == 10)
    cut = len(nl) % 4                  # lines of an incomplete last record (judged last)
    start = np.concatenate([[0], nl[:-1] + 1]).astype(np.int64)[:len(nl) - cut]
    end = nl.astype(np.int64)[:len(nl) - cut]
    end = end - ((end > start) & (buf[np.maximum(end - 1, 0)] == 13))          # CRLF
    hs, he = start[0::4], end[0::4]
    ss, se = start[1::4], end[1::4]
    ps, pe = start[2::4], end[2::4]
    qs, qe = start[3::4], end[3::4]
    bad = (he <= hs) | (buf[np.minimum(hs, len(buf) - 1)] != ord("@")) | (pe <= ps) | \
        (buf[np.minimum(ps, len(buf) - 1)] != ord("+")) | ((se - ss) != (qe - qs))
    if bad.any():
        raise MapperError("{}: record {} of this block is not a 4-line FASTQ record (multi-line "
                          "records are not supported)".format(path, int(np.flatnonzero(bad)[0]) + 1))
    if cut:
        raise MapperError("{}: truncated FASTQ record at the end of the file".format(path))
    # QNAME: the header up to the first whitespace, without a trailing /1 or /2
    ws = np.flatnonzero((buf == 32) | (buf == 9))
    ne = he.copy()
    if len(ws):
        j = np.searchsorted(ws, hs)
        first = ws[np.minimum(j, len(ws) - 1)]
        ne = np.where((j < len(ws)) & (first < he), first, he)
    ns = hs + 1
    last = buf[np.maximum(ne - 1, 0)]
    mate_tag = (ne - ns >= 2) & (buf[np.maximum(ne - 2, 0)] == ord("/")) & \
        ((last == ord("1")) | (last == ord("2")))
    ne = ne - 2 * mate_tag
    blk = FastqBlock()
    blk.name, blk.name_off = _gather(buf, ns, ne - ns)
    blk.seq, blk.off = _gather(buf, ss, se - ss)
    return blk


def iter_fastq(path, chunk=CHUNK_PAIRS):
    """FastqBlocks of up to `chunk` records."""
    with _open(path) as fh:
        while True:
            lines = list(itertools.islice(fh, 4 * chunk))
            while lines and not lines[-1].strip():      # blank lines at the end of the file
                lines.pop()
            if not lines:
                return
            yield parse_fastq_block(b"".join(lines), path)


def iter_fastq_pairs(path1, path2, chunk=CHUNK_PAIRS):
    """(mate-1 block, mate-2 block) with equal record counts and equal names."""
    it1, it2 = iter_fastq(path1, chunk), iter_fastq(path2, chunk)
    done = 0
    for b1, b2 in itertools.zip_longest(it1, it2):
        if b1 is None or b2 is None or len(b1) != len(b2):
            raise MapperError("{} and {} hold different numbers of reads".format(path1, path2))
        same = np.array_equal(b1.name_off, b2.name_off) and np.array_equal(b1.name, b2.name)
        if not same:
            k = next(i for i in range(len(b1)) if b1.qname(i) != b2.qname(i))
            raise MapperError("mates {} of {} and {} differ in name: {} / {}".format(
                done + k + 1, path1, path2, b1.qname(k), b2.qname(k)))
        done += len(b1)
        yield b1, b2


# ---------------------------------------------------------------------------
# device calls
# ---------------------------------------------------------------------------

RESULT_FIELDS = (("contig", np.int32), ("pos1", np.int32), ("pos2", np.int32),
                 ("strand1", np.uint8), ("mm1", np.uint8), ("mm2", np.uint8))
# the gapped pass: d > 0 deletion, d < 0 insertion after the mate's first k bases (counted
# along the contig); flags bit 0: aligned by the gapped pass, bit 1: hit-list overflow
GAP_FIELDS = (("d1", np.int8), ("d2", np.int8), ("k1", np.int16), ("k2", np.int16), ("flags", np.uint8))
MAX_GAP = 8


class Mapper:
    """One context with the index of one contig set (wf_map_index); `map` runs wf_map_pairs
    or, with max_gap > 0, wf_map_pairs_gapped."""

    def __init__(self, seq, off, seed_length=20, max_seed_hits=16, max_mismatches=4, min_insert=0,
                 max_insert=500, device=0, max_gap=0):
        if not 0 <= int(max_gap) <= MAX_GAP:
            raise MapperError("max_gap {} outside 0..{}".format(max_gap, MAX_GAP))
        self.gap_params = L.WfMapGapParams(max_gap=int(max_gap))
        self.so = L.load()
        self.h = C.c_void_p()
        rc = self.so.wf_init(int(device), C.byref(self.h))
        if rc != L.WF_OK:
            self.h = None
            raise L.WaafleHipError(rc, "wf_init(device={}) failed".format(device))
        self.params = L.WfMapParams(seed_len=int(seed_length), max_occ=int(max_seed_hits),
                                    max_mm=int(max_mismatches), min_insert=int(min_insert),
                                    max_insert=int(max_insert))
        try:
            self.index(seq, off)
        except Exception:
            self.close()
            raise

    def _check(self, rc):
        if rc != L.WF_OK:
            raise L.WaafleHipError(rc, self.so.wf_last_error(self.h).decode())

    def index(self, seq, off):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        c = L.WfMapContigs(n_contigs=len(off) - 1, seq=L.ptr(seq), off=L.ptr(off))
        self._check(self.so.wf_map_index(self.h, C.byref(c), C.byref(self.params)))

    def map(self, seq1, off1, seq2, off2, params=None, gapped=None):
        """Result arrays (RESULT_FIELDS and GAP_FIELDS) for the pairs given as host arrays.
        gapped: call wf_map_pairs_gapped (default: when max_gap > 0; with max_gap 0 the gap
        fields are zeros either way, and wf_map_pairs spares their copies)."""
        seq1, seq2 = (np.ascontiguousarray(s, dtype=np.uint8) for s in (seq1, seq2))
        off1, off2 = (np.ascontiguousarray(o, dtype=np.int64) for o in (off1, off2))
        n = len(off1) - 1
        if len(off2) - 1 != n:
            raise MapperError("mate arrays of different lengths")
        out = {f: np.zeros(n, dt) for f, dt in RESULT_FIELDS + GAP_FIELDS}
        rd = L.WfMapReads(n_pairs=n, device_resident=0, seq1=L.ptr(seq1), off1=L.ptr(off1),
                          seq2=L.ptr(seq2), off2=L.ptr(off2))
        r = L.WfMapResult(**{f: L.ptr(out[f]) for f, _ in RESULT_FIELDS})
        if gapped is None:
            gapped = self.gap_params.max_gap != 0
        if gapped:
            g = L.WfMapGapResult(**{f: L.ptr(out[f]) for f, _ in GAP_FIELDS})
            self._check(self.so.wf_map_pairs_gapped(self.h, C.byref(rd), C.byref(params or self.params),
                                                    C.byref(self.gap_params), C.byref(r), C.byref(g)))
        else:
            self._check(self.so.wf_map_pairs(self.h, C.byref(rd), C.byref(params or self.params), C.byref(r)))
        return out

    def map_device(self, n_pairs, seq1, off1, seq2, off2, out):
        """Device-resident form: device addresses (ints, e.g. a tensor's data_ptr()) of the
        uint8 bases and int64 offsets on this context's device; `out` maps each of
        RESULT_FIELDS, and of GAP_FIELDS (which may be left out when max_gap is 0), to the
        address of its array.  Returns after the work is done."""
        rd = L.WfMapReads(n_pairs=int(n_pairs), device_resident=1, seq1=seq1, off1=off1, seq2=seq2,
                          off2=off2)
        r = L.WfMapResult(**{f: out[f] for f, _ in RESULT_FIELDS})
        if all(f in out for f, _ in GAP_FIELDS):
            g = L.WfMapGapResult(**{f: out[f] for f, _ in GAP_FIELDS})
            self._check(self.so.wf_map_pairs_gapped(self.h, C.byref(rd), C.byref(self.params),
                                                    C.byref(self.gap_params), C.byref(r), C.byref(g)))
        elif self.gap_params.max_gap:
            raise MapperError("max_gap > 0 needs the arrays of GAP_FIELDS in `out`")
        else:
            self._check(self.so.wf_map_pairs(self.h, C.byref(rd), C.byref(self.params), C.byref(r)))
        self._check(self.so.wf_synchronize(self.h))

    def close(self):
        if self.h is not None:
            self.so.wf_free(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---------------------------------------------------------------------------
# SAM
# ---------------------------------------------------------------------------

def sam_header(names, lengths):
    lines = ["@HD\tVN:1.0\tSO:unsorted"]
    lines += ["@SQ\tSN:{}\tLN:{}".format(n, int(l)) for n, l in zip(names, lengths)]
    lines.append("@PG\tID:waafle_amd.mapper\tPN:waafle_amd.mapper")
    return lines


def _cigar(length, d, k):
    if d > 0:
        return "{}M{}D{}M".format(k, d, length - k)
    if d < 0:
        return "{}M{}I{}M".format(k, -d, length - k + d)
    return "{}M".format(length)


def sam_records(qnames, len1, len2, res, contig_names):
    """Two records per pair: 99/147 (mate 1 on +) or 83/163 (mate 1 on -) with CIGAR <L>M and
    NM:i:<mm>, or 77/141 when the pair is unaligned.  With the gap fields in `res`, a mate
    with a gap has CIGAR <k>M<d>D<L-k>M or <k>M<g>I<L-k-g>M and NM:i:<mm + |d|>, and TLEN
    counts the contig bases the mates span (L + d each)."""
    out = []
    n = len(qnames)
    contig, pos1, pos2 = res["contig"].tolist(), res["pos1"].tolist(), res["pos2"].tolist()
    strand1, mm1, mm2 = res["strand1"].tolist(), res["mm1"].tolist(), res["mm2"].tolist()
    d1, d2, k1, k2 = (res[f].tolist() if f in res else [0] * n for f in ("d1", "d2", "k1", "k2"))
    for i, q in enumerate(qnames):
        c = contig[i]
        if c < 0:
            out.append("{}\t77\t*\t0\t0\t*\t*\t0\t0\t*\t*".format(q))
            out.append("{}\t141\t*\t0\t0\t*\t*\t0\t0\t*\t*".format(q))
            continue
        p1, p2, l1, l2 = pos1[i], pos2[i], int(len1[i]), int(len2[i])
        if strand1[i] == 0:
            f1, f2, frag = 99, 147, p2 + l2 + d2[i] - p1
            t1, t2 = frag, -frag
        else:
            f1, f2, frag = 83, 163, p1 + l1 + d1[i] - p2
            t1, t2 = -frag, frag
        name = contig_names[c]
        out.append("{}\t{}\t{}\t{}\t255\t{}\t=\t{}\t{}\t*\t*\tNM:i:{}".format(
            q, f1, name, p1, _cigar(l1, d1[i], k1[i]), p2, t1, mm1[i] + abs(d1[i])))
        out.append("{}\t{}\t{}\t{}\t255\t{}\t=\t{}\t{}\t*\t*\tNM:i:{}".format(
            q, f2, name, p2, _cigar(l2, d2[i], k2[i]), p1, t2, mm2[i] + abs(d2[i])))
    return out


def pair_arrays(res, len1, len2):
    """The aligned pairs as junctions.read_pairs returns them: (pair_contig, m1_start,
    m1_end, m2_start, m2_end); a mate with a gap d ends at p + L + d - 1."""
    keep = res["contig"] >= 0
    p1, p2 = res["pos1"][keep].astype(np.int64), res["pos2"][keep].astype(np.int64)
    l1, l2 = np.asarray(len1, np.int64)[keep], np.asarray(len2, np.int64)[keep]
    if "d1" in res:
        l1 = l1 + res["d1"][keep].astype(np.int64)
        l2 = l2 + res["d2"][keep].astype(np.int64)
    return res["contig"][keep].astype(np.int32), p1, p1 + l1 - 1, p2, p2 + l2 - 1


def map_pairs(contigs, reads1, reads2, sam_path=None, device=0, chunk=CHUNK_PAIRS, **params):
    """Map the FASTQ pair `reads1` / `reads2` against `contigs` = (names, seq, off) (as
    read_fasta returns), optionally writing the SAM file.  Returns (pair arrays of the
    aligned pairs, read pairs seen)."""
    names, seq, off = contigs
    parts = []
    total = 0
    fh = open(sam_path, "w") if sam_path else None
    try:
        if fh:
            fh.write("\n".join(sam_header(names, np.diff(off))) + "\n")
        with Mapper(seq, off, device=device, **params) as m:
            for b1, b2 in iter_fastq_pairs(reads1, reads2, chunk):
                len1, len2 = np.diff(b1.off), np.diff(b2.off)
                if max(len1.max(initial=0), len2.max(initial=0)) > MAX_READ:
                    raise MapperError("a read longer than {} bases".format(MAX_READ))
                res = m.map(b1.seq, b1.off, b2.seq, b2.off)
                parts.append(pair_arrays(res, len1, len2))
                total += len(b1)
                if fh:
                    qnames = [b1.qname(i) for i in range(len(b1))]
                    fh.write("\n".join(sam_records(qnames, len1, len2, res, names)) + "\n")
    finally:
        if fh:
            fh.close()
    if not parts:
        parts = [(np.zeros(0, np.int32),) + (np.zeros(0, np.int64),) * 4]
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(5)), total
