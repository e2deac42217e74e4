"""`waafle_search` drop-in CLI (waafle_search.py), with a built-in GPU search in place of blastn.

    python -m waafle_amd.search contigs.fna waafledb [--out --threads --blastn]
    python -m waafle_amd.search contigs.fna genes.fna --searcher native [--seed-length 21 ...]
    python -m waafle_amd.search contigs.fna genes.fna --searcher native --gapped [--band 15 --xdrop-gap 30]
    python -m waafle_amd.search contigs.fna genes.fna --searcher native --dust [--dust-out masked.tsv]
    python -m waafle_amd.makedb genes.fna --out genes.wfdb       (once per database)
    python -m waafle_amd.search contigs.fna genes.wfdb --searcher native [...]

`--searcher blastn` (the default) issues exactly the reference's blastn command.  `--searcher
native` runs the seed-and-extend search of wf_search.hip on one MI355X (DESIGN.md §12 states
the rule): the contigs are indexed once (wf_map_index), the database genes stream through in
chunks as subjects (wf_search), and the table is written in the reference's 15 columns.  It
is not a blastn clone.  Without `--gapped` it reports ungapped HSPs only, so a diverged
homolog with indels comes out as several HSPs with lower subject coverage than blastn would
report.  With `--gapped` (wf_search_gapped, wf_search_gap.hip) every ungapped
HSP is an anchor of a banded x-drop alignment with linear gap cost, and the table holds those
alignments: one row for such a homolog, when no gap on one side of an anchor is longer than
the band.  With `--dust` (wf_search_mask, wf_dust.hip) the contigs'
low-complexity stretches, by the published symmetric-DUST definition, give no seeds (a soft
mask: extensions run through them); blastn masks its query so by default, this search only
when asked, and agreement with NCBI dustmasker is not measured.

A database formatted once with `python -m waafle_amd.makedb` (a .wfdb file)
holds the genes as the bit planes the kernels use: the search maps the file and hands slices
of it to wf_search_packed / wf_search_gapped_packed, so no run parses the FASTA again and three
eighths of the bytes go to the device.  The table is the same either way.

Host side (this module): the streaming subject-FASTA reader, the reader of a packed database,
the calls into wf_search / wf_search_gapped and their packed forms, the ordering and
--max-target-seqs step (order_records; with `--order-on device` wf_order_records computes the
same on the GPU) and the row writer.
"""
from __future__ import annotations

import argparse
import ctypes as C
import gzip
import math
import os
import struct
import sys

import numpy as np

from . import inputs, lib as L, mapper

DEFAULTS = dict(seed_length=21, seed_stride=8, max_seed_hits=64, xdrop=20, min_score=28)
MAX_TARGET_SEQS = 10000          # utils.c_max_target_seqs
CHUNK_BASES = 1 << 28
LAMBDA, K = 1.28, 0.46           # bit score = (LAMBDA * score - ln K) / ln 2
BLAST_FORMAT = "6 qseqid sseqid qlen slen length qstart qend sstart send pident positive gaps evalue " \
               "bitscore sstrand"                            # utils.c_blast_format_string

RECORD_FIELDS = (("contig", np.int32), ("subject", np.int32), ("minus", np.uint8), ("qstart", np.int32),
                 ("sstart", np.int32), ("length", np.int32), ("matches", np.int32))
STAT_FIELDS = ("seed_hits", "seeds_skipped", "raw_hsps")
GAP_DEFAULTS = dict(band=15, xdrop_gap=30)
GAP_RECORD_FIELDS = (("contig", np.int32), ("subject", np.int32), ("minus", np.uint8), ("qstart", np.int32),
                     ("qspan", np.int32), ("sstart", np.int32), ("sspan", np.int32), ("length", np.int32),
                     ("matches", np.int32), ("gaps", np.int32))
GAP_STAT_FIELDS = STAT_FIELDS + ("anchors", "raw_alignments")
DUST_DEFAULTS = dict(dust_window=64, dust_level=20)
DUST_TILE = 448                  # kDustTile (csrc/wf_internal.h): starts one block of k_dust_mask emits


class SearchError(inputs.InputError):
    pass


# ---------------------------------------------------------------------------
# device calls
# ---------------------------------------------------------------------------

class Searcher:
    """One context with the index of one contig set; `search` runs wf_search on one chunk of
    subjects and returns its records (RECORD_FIELDS, subject indices within the chunk);
    `search_gapped` runs wf_search_gapped (GAP_RECORD_FIELDS).  dust: the index holds no S-mer
    with a low-complexity base (wf_search_mask after every indexing); the searcher owns its
    context, so no read mapper sees that index.  report_on "device": the reporting step of every
    search call (duplicates, containment or cover, min_score, the records' order) runs on the GPU
    (WF_OPT_SEARCH_REPORT); the records are the same."""

    def __init__(self, seq, off, seed_length=21, seed_stride=8, max_seed_hits=64, xdrop=20, min_score=28,
                 device=0, capacity=1 << 16, band=15, xdrop_gap=30, dust=False, dust_window=64, dust_level=20,
                 report_on="host"):
        if report_on not in ("host", "device"):
            raise SearchError("report_on is 'host' or 'device', not {!r}".format(report_on))
        self.params = L.WfSearchParams(seed_len=int(seed_length), stride=int(seed_stride),
                                       max_occ=int(max_seed_hits), xdrop=int(xdrop), min_score=int(min_score))
        self.gap_params = L.WfSearchGapParams(band=int(band), xdrop_gap=int(xdrop_gap))
        self.capacity = max(int(capacity), 1)
        self.stats = dict.fromkeys(GAP_STAT_FIELDS + ("masked_bases",), 0)
        self.dust = bool(dust)
        self.dust_params = L.WfDustParams(window=int(dust_window), level=int(dust_level))
        self.dust_stats = None
        self._mask = None
        # the index's own max_occ belongs to the read mapper and is not read by the search
        self.mapper = mapper.Mapper(seq, off, seed_length=int(seed_length), device=device)
        self.so, self.h = self.mapper.so, self.mapper.h
        self.report_on = report_on
        rc = self.so.wf_set_option(self.h, L.OPT_SEARCH_REPORT, int(report_on == "device"))
        if rc != L.WF_OK:
            msg = self.so.wf_last_error(self.h).decode()
            self.close()
            raise L.WaafleHipError(rc, msg)
        if self.dust:
            try:
                self.apply_mask(len(seq))
            except Exception:
                self.close()
                raise

    def index(self, seq, off):
        self.mapper.index(seq, off)
        self._mask, self.dust_stats, self.stats["masked_bases"] = None, None, 0
        if self.dust:
            self.apply_mask(len(seq))

    def apply_mask(self, total, params=None):
        """wf_search_mask on the `total` bases the context holds: the mask is kept for `mask`,
        the call's counters in `dust_stats`."""
        words = np.zeros((int(total) + 31) // 32, np.uint32)
        r = L.WfDustResult(mask=L.ptr(words))
        rc = self.so.wf_search_mask(self.mapper.h, C.byref(params or self.dust_params), C.byref(r))
        if rc != L.WF_OK:
            raise L.WaafleHipError(rc, self.so.wf_last_error(self.mapper.h).decode())
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[:int(total)].astype(bool)
        self._mask = bits
        self.dust_stats = dict(masked_bases=int(r.masked_bases), kmers_before=int(r.kmers_before),
                               kmers_after=int(r.kmers_after))
        self.stats["masked_bases"] = int(r.masked_bases)

    def mask(self):
        """One bool per store base (the contigs concatenated), or None without a mask."""
        return self._mask

    def search_once(self, seq, off, capacity, params=None):
        """(return code, full record count, records written): one wf_search call."""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        out = {f: np.zeros(capacity, dt) for f, dt in RECORD_FIELDS}
        sb = L.WfSearchSubjects(n_subjects=len(off) - 1, seq=L.ptr(seq), off=L.ptr(off))
        r = L.WfSearchResult(capacity=capacity, **{f: L.ptr(out[f]) for f, _ in RECORD_FIELDS})
        rc = self.so.wf_search(self.mapper.h, C.byref(sb), C.byref(params or self.params), C.byref(r))
        if rc == L.WF_OK:
            for f in STAT_FIELDS:
                self.stats[f] += getattr(r, f)
        n = int(r.n)
        return rc, n, {f: a[:min(n, capacity)] for f, a in out.items()}

    def search(self, seq, off, params=None):
        rc, n, out = self.search_once(seq, off, self.capacity, params)
        if rc == L.WF_E_NOMEM:                              # the call is repeatable with more room
            self.capacity = max(n, 2 * self.capacity)
            rc, n, out = self.search_once(seq, off, self.capacity, params)
        if rc != L.WF_OK:
            raise L.WaafleHipError(rc, self.so.wf_last_error(self.mapper.h).decode())
        return out

    def search_gapped_once(self, seq, off, capacity, params=None, gap_params=None):
        """(return code, full record count, records written): one wf_search_gapped call."""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=np.int64)
        out = {f: np.zeros(capacity, dt) for f, dt in GAP_RECORD_FIELDS}
        sb = L.WfSearchSubjects(n_subjects=len(off) - 1, seq=L.ptr(seq), off=L.ptr(off))
        r = L.WfSearchGapResult(capacity=capacity, **{f: L.ptr(out[f]) for f, _ in GAP_RECORD_FIELDS})
        rc = self.so.wf_search_gapped(self.mapper.h, C.byref(sb), C.byref(params or self.params),
                                      C.byref(gap_params or self.gap_params), C.byref(r))
        if rc == L.WF_OK:
            for f in GAP_STAT_FIELDS:
                self.stats[f] += getattr(r, f)
        n = int(r.n)
        return rc, n, {f: a[:min(n, capacity)] for f, a in out.items()}

    def search_gapped(self, seq, off, params=None, gap_params=None):
        rc, n, out = self.search_gapped_once(seq, off, self.capacity, params, gap_params)
        if rc == L.WF_E_NOMEM:                              # the call is repeatable with more room
            self.capacity = max(n, 2 * self.capacity)
            rc, n, out = self.search_gapped_once(seq, off, self.capacity, params, gap_params)
        if rc != L.WF_OK:
            raise L.WaafleHipError(rc, self.so.wf_last_error(self.mapper.h).decode())
        return out

    @staticmethod
    def _packed_subjects(chunk, off):
        return L.WfSearchPackedSubjects(n_subjects=len(off) - 1, off=L.ptr(off), lo=L.ptr(chunk.lo), hi=L.ptr(chunk.hi),
                                        nn=L.ptr(chunk.nn), n_words=len(chunk.lo), bit0=int(chunk.bit0))

    def search_packed_once(self, chunk, capacity, params=None):
        """(return code, full record count, records written): one wf_search_packed call on a
        chunk of a packed database (PackedChunk, or anything with off, bit0, lo, hi, nn)."""
        off = np.ascontiguousarray(chunk.off, dtype=np.int64)
        out = {f: np.zeros(capacity, dt) for f, dt in RECORD_FIELDS}
        sb = self._packed_subjects(chunk, off)
        r = L.WfSearchResult(capacity=capacity, **{f: L.ptr(out[f]) for f, _ in RECORD_FIELDS})
        rc = self.so.wf_search_packed(self.mapper.h, C.byref(sb), C.byref(params or self.params), C.byref(r))
        if rc == L.WF_OK:
            for f in STAT_FIELDS:
                self.stats[f] += getattr(r, f)
        n = int(r.n)
        return rc, n, {f: a[:min(n, capacity)] for f, a in out.items()}

    def search_packed(self, chunk, params=None):
        rc, n, out = self.search_packed_once(chunk, self.capacity, params)
        if rc == L.WF_E_NOMEM:                              # the call is repeatable with more room
            self.capacity = max(n, 2 * self.capacity)
            rc, n, out = self.search_packed_once(chunk, self.capacity, params)
        if rc != L.WF_OK:
            raise L.WaafleHipError(rc, self.so.wf_last_error(self.mapper.h).decode())
        return out

    def search_gapped_packed_once(self, chunk, capacity, params=None, gap_params=None):
        """(return code, full record count, records written): one wf_search_gapped_packed call."""
        off = np.ascontiguousarray(chunk.off, dtype=np.int64)
        out = {f: np.zeros(capacity, dt) for f, dt in GAP_RECORD_FIELDS}
        sb = self._packed_subjects(chunk, off)
        r = L.WfSearchGapResult(capacity=capacity, **{f: L.ptr(out[f]) for f, _ in GAP_RECORD_FIELDS})
        rc = self.so.wf_search_gapped_packed(self.mapper.h, C.byref(sb), C.byref(params or self.params),
                                             C.byref(gap_params or self.gap_params), C.byref(r))
        if rc == L.WF_OK:
            for f in GAP_STAT_FIELDS:
                self.stats[f] += getattr(r, f)
        n = int(r.n)
        return rc, n, {f: a[:min(n, capacity)] for f, a in out.items()}

    def search_gapped_packed(self, chunk, params=None, gap_params=None):
        rc, n, out = self.search_gapped_packed_once(chunk, self.capacity, params, gap_params)
        if rc == L.WF_E_NOMEM:                              # the call is repeatable with more room
            self.capacity = max(n, 2 * self.capacity)
            rc, n, out = self.search_gapped_packed_once(chunk, self.capacity, params, gap_params)
        if rc != L.WF_OK:
            raise L.WaafleHipError(rc, self.so.wf_last_error(self.mapper.h).decode())
        return out

    def chunk_planes(self, total, strand):
        """wf_search_chunk_planes: (lo, hi, nn) of the store that the last search call left on
        the device for its chunk of `total` bases, strand 0 or 1; (total + 31) // 32 + 2 words
        each.  A diagnostic."""
        words = (int(total) + 31) // 32 + 2
        lo, hi, nn = (np.zeros(words, np.uint32) for _ in range(3))
        rc = self.so.wf_search_chunk_planes(self.mapper.h, int(strand), L.ptr(lo), L.ptr(hi), L.ptr(nn), words)
        if rc != L.WF_OK:
            raise L.WaafleHipError(rc, self.so.wf_last_error(self.mapper.h).decode())
        return lo, hi, nn

    def close(self):
        self.mapper.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def search_chunk(searcher, seq, off=None, gapped=False):
    """`Searcher.search` (gapped: `Searcher.search_gapped`); a chunk that is refused as too big
    (WF_E_TOOBIG) is halved, down to one subject.  seq a PackedChunk (off is then its own): the
    packed calls, and the halves are cut from its database anew."""
    packed = isinstance(seq, PackedChunk)
    try:
        if packed:
            off = seq.off
            return searcher.search_gapped_packed(seq) if gapped else searcher.search_packed(seq)
        return searcher.search_gapped(seq, off) if gapped else searcher.search(seq, off)
    except L.WaafleHipError as exc:
        n = len(off) - 1
        if exc.code != L.WF_E_TOOBIG:
            raise
        if n <= 1:
            raise SearchError("a single subject is too big to search: {}".format(exc.msg))
    h = n // 2
    if packed:
        a = search_chunk(searcher, seq.db.chunk(seq.first, seq.first + h), None, gapped)
        b = search_chunk(searcher, seq.db.chunk(seq.first + h, seq.last), None, gapped)
    else:
        a = search_chunk(searcher, seq[:off[h]], off[:h + 1], gapped)
        b = search_chunk(searcher, seq[off[h]:], off[h:] - off[h], gapped)
    b["subject"] = b["subject"] + np.int32(h)
    return {f: np.concatenate([a[f], b[f]]) for f in a}


def mask_intervals(mask, off):
    """(contig, start, end) rows of the masked stretches, 0-based and half-open on the contig,
    in store order; a stretch that runs over a contig's end is split there."""
    rows = []
    mask = np.asarray(mask, bool)
    for c in range(len(off) - 1):
        m = np.concatenate([[False], mask[int(off[c]):int(off[c + 1])], [False]])
        edge = np.flatnonzero(m[1:] != m[:-1])
        rows += [(c, int(a), int(b)) for a, b in zip(edge[0::2], edge[1::2])]
    return rows


def format_mask_rows(rows, contig_names):
    """--dust-out: contig name, start, end (0-based, half-open), tab-separated."""
    return ["{}\t{}\t{}".format(contig_names[c], a, b) for c, a, b in rows]


# ---------------------------------------------------------------------------
# the subject FASTA
# ---------------------------------------------------------------------------

def _open(path):
    return gzip.open(path, "rb") if str(path).endswith(".gz") else open(path, "rb")


def subject_id(line):
    """The id of a header line (with its '>'): up to the first whitespace, a WAAFLE header."""
    words = line[1:].split()
    sid = words[0].decode() if words else ""
    if "|" not in sid:
        raise SearchError("bad subject id header: {} (a WAAFLE header is id|taxon|...)".format(sid))
    return sid


def headless_error(path):
    return SearchError("sequence before the first FASTA header in {}".format(path))


def iter_subject_chunks(path, chunk_bases=CHUNK_BASES):
    """(ids, seq, off) per chunk, in file order: whole subjects, at most `chunk_bases` bases
    together (a longer subject is a chunk of its own).  ids: the header up to the first
    whitespace, which must be a WAAFLE header (id|taxon|system=name...)."""
    ids, parts, sizes, held = [], [], [], 0

    def flush(n):
        """the first n subjects held"""
        nonlocal ids, parts, sizes, held
        off = np.zeros(n + 1, np.int64)
        np.cumsum(sizes[:n], out=off[1:])
        seq = np.frombuffer(b"".join(b"".join(p) for p in parts[:n]), dtype=np.uint8)
        out = (ids[:n], seq, off)
        ids, parts, sizes = ids[n:], parts[n:], sizes[n:]
        held = sum(sizes)
        return out

    with _open(path) as fh:
        for line in fh:
            line = line.strip()
            if not line:
                continue
            if line[:1] == b">":
                if len(ids) > 1 and held > chunk_bases:      # the last one complete does not fit
                    yield flush(len(ids) - 1)
                if len(ids) == 1 and held >= chunk_bases:
                    yield flush(1)
                ids.append(subject_id(line))
                parts.append([])
                sizes.append(0)
            else:
                if not ids:
                    raise headless_error(path)
                parts[-1].append(line)
                sizes[-1] += len(line)
                held += len(line)
    if len(ids) > 1 and held > chunk_bases:
        yield flush(len(ids) - 1)
    if ids:
        yield flush(len(ids))


# ---------------------------------------------------------------------------
# the packed database (.wfdb, written by waafle_amd.makedb)
# ---------------------------------------------------------------------------

DB_MAGIC = b"WAAFLEDB"
DB_VERSION = 1
DB_ALIGN = 64
DB_HEADER = struct.Struct("<8sIIqqqq")       # magic, version, 0, n_subjects, total, plane_words, id_bytes


def db_align(n):
    return -(-n // DB_ALIGN) * DB_ALIGN


def db_sections(n, words, id_bytes):
    """{section: (byte offset, items)} of a database of n subjects, and the file's length"""
    at, out = DB_ALIGN, {}
    for name, items, size in (("off", n + 1, 8), ("id_off", n + 1, 8), ("ids", id_bytes, 1), ("lo", words, 4),
                              ("hi", words, 4), ("nn", words, 4)):
        out[name] = (at, items)
        at = db_align(at + items * size)
    return out, at


def is_packed_db(path):
    try:
        with open(path, "rb") as fh:
            return fh.read(len(DB_MAGIC)) == DB_MAGIC
    except OSError:
        return False


class PackedChunk:
    """Subjects [first, last) of a PackedDb as the packed calls take them: `off` relative to
    the chunk, and `lo`, `hi`, `nn`, views into the file's map, in which base i of the chunk
    is bit (bit0 + i) & 31 of word (bit0 + i) >> 5."""

    def __init__(self, db, first, last):
        self.db, self.first, self.last = db, int(first), int(last)
        start = int(db.off[first])
        self.off = np.asarray(db.off[first:last + 1], np.int64) - start
        self.bit0 = start & 31
        w0, n_words = start >> 5, (self.bit0 + int(self.off[-1]) + 31) // 32
        self.lo, self.hi, self.nn = (p[w0:w0 + n_words] for p in (db.lo, db.hi, db.nn))


class _DbIds:
    """The ids of a PackedDb as a read-only sequence, decoded when asked for."""

    def __init__(self, id_off, blob):
        self.id_off, self.blob = id_off, blob

    def __len__(self):
        return len(self.id_off) - 1

    def __getitem__(self, g):
        if isinstance(g, slice):
            return [self[i] for i in range(*g.indices(len(self)))]
        if g < 0:
            g += len(self)
        if not 0 <= g < len(self):
            raise IndexError(g)
        return bytes(self.blob[int(self.id_off[g]):int(self.id_off[g + 1])]).decode()

    def __iter__(self):
        return (self[g] for g in range(len(self)))


class PackedDb:
    """A .wfdb file, memory-mapped read-only: `off` [n + 1], `lens`, `ids`, and the planes
    `lo`, `hi`, `nn`.  Opening it checks the header, every size against the file's length and
    the offsets; what fails is a SearchError."""

    def __init__(self, path):
        self.path = str(path)
        size = os.path.getsize(self.path)
        if size < DB_ALIGN:
            raise SearchError("{}: not a packed database ({} bytes)".format(path, size))
        with open(self.path, "rb") as fh:
            magic, version, _, n, total, words, id_bytes = DB_HEADER.unpack(fh.read(DB_HEADER.size))
        if magic != DB_MAGIC:
            raise SearchError("{}: not a packed database (bad magic)".format(path))
        if version != DB_VERSION:
            raise SearchError("{}: packed database version {} (this reader knows version {}): format it again "
                              "with `python -m waafle_amd.makedb`".format(path, version, DB_VERSION))
        if n < 0 or total < 0 or id_bytes < 0 or n >= 1 << 40 or id_bytes >= 1 << 50 or total >= 1 << 50 or \
                words != (total + 31) // 32 + 2:
            raise SearchError("{}: inconsistent header (subjects {}, bases {}, plane words {}, id bytes {})".format(
                path, n, total, words, id_bytes))
        sec, length = db_sections(n, words, id_bytes)
        if size != length:
            raise SearchError("{}: {} bytes, but its header describes {} (truncated or corrupt)".format(
                path, size, length))
        self.n_subjects, self.total, self.words = n, total, words
        mm = np.memmap(self.path, dtype=np.uint8, mode="r")

        def view(name, dtype):
            at, items = sec[name]
            return mm[at:at + items * np.dtype(dtype).itemsize].view(dtype)

        self.off, id_off = view("off", "<i8"), view("id_off", "<i8")
        for what, a, end in (("subject", self.off, total), ("id", id_off, id_bytes)):
            if a[0] != 0 or a[-1] != end or (n and bool((np.diff(a) < 0).any())):
                raise SearchError("{}: bad {} offsets (they must start at 0, not decrease and end at {})".format(
                    path, what, end))
        self.ids = _DbIds(id_off, view("ids", np.uint8))
        self.lens = np.diff(self.off)
        self.lo, self.hi, self.nn = view("lo", "<u4"), view("hi", "<u4"), view("nn", "<u4")

    def chunk(self, first, last):
        return PackedChunk(self, first, last)

    def chunks(self, chunk_bases=CHUNK_BASES):
        """PackedChunks in file order, cut where iter_subject_chunks cuts the FASTA: whole
        subjects, at most `chunk_bases` bases together; a subject of that many or more is a
        chunk of its own."""
        off, n, first = self.off, self.n_subjects, 0
        while first < n:
            if off[first + 1] - off[first] >= chunk_bases:
                last = first + 1
            else:                                            # the last subject that still fits: past first
                last = min(int(np.searchsorted(off, off[first] + chunk_bases, side="right")) - 1, n)
            yield self.chunk(first, last)
            first = last


# ---------------------------------------------------------------------------
# ordering and rows
# ---------------------------------------------------------------------------

def score_of(rec):
    """The raw score of ungapped records; of gapped ones (they have `gaps`) score2, the score
    in half units: 2 per match, -4 per mismatch, -5 per gap column."""
    m, length = rec["matches"].astype(np.int64), rec["length"].astype(np.int64)
    if "gaps" in rec:
        return 6 * m - 4 * length - rec["gaps"].astype(np.int64)
    return 3 * m - 2 * length


def order_records(rec, max_target_seqs=MAX_TARGET_SEQS):
    """Indices of the records to write, in the table's order: by contig; within a contig the
    subjects are ranked by (-best score, subject) and those past `max_target_seqs` lose their
    rows; the rest go by (-score, subject, minus, qstart, sstart), gapped records by (-score2,
    subject, minus, qstart, sstart, qspan, sspan)."""
    n = len(rec["contig"])
    if n == 0:
        return np.zeros(0, np.int64)
    score = score_of(rec)
    contig, subject = rec["contig"].astype(np.int64), rec["subject"].astype(np.int64)
    pair, inv = np.unique((contig << 32) | subject, return_inverse=True)
    best = np.full(len(pair), np.iinfo(np.int64).min)
    np.maximum.at(best, inv, score)
    pc, ps = pair >> 32, pair & 0xFFFFFFFF
    o = np.lexsort((ps, -best, pc))
    first = np.flatnonzero(np.concatenate([[True], pc[o][1:] != pc[o][:-1]]))
    run = np.repeat(first, np.diff(np.concatenate([first, [len(o)]])))
    keep_pair = np.zeros(len(pair), bool)
    keep_pair[o] = (np.arange(len(o)) - run) < max_target_seqs
    idx = np.flatnonzero(keep_pair[inv])
    spans = (rec["sspan"][idx], rec["qspan"][idx]) if "gaps" in rec else ()
    o2 = np.lexsort(spans + (rec["sstart"][idx], rec["qstart"][idx], rec["minus"][idx], subject[idx], -score[idx],
                             contig[idx]))
    return idx[o2]


ORDER_COLUMNS = (("contig", np.int32), ("subject", np.int32), ("minus", np.uint8), ("qstart", np.int32),
                 ("qspan", np.int32), ("sstart", np.int32), ("sspan", np.int32), ("length", np.int32),
                 ("matches", np.int32))                      # hits.RECORD_COLUMNS: those of wf_hit_records


def order_records_device(ctx, rec, max_target_seqs=MAX_TARGET_SEQS, gather=False, out=None):
    """order_records on the GPU (wf_order_records): the same indices.  `ctx`: an
    open Searcher, mapper.Mapper or engine.GpuScorer (anything with the library and a context
    handle).  gather: returns (order, columns), the columns what hits.record_columns(rec,
    order) gives.  out: {"order": int64 [n], column: [n] ...} to write into (a refused call
    leaves them as they are).  Raises lib.WaafleHipError; its code is lib.WF_E_NOMEM when the
    device has no room for the call (order_with falls back to the host then)."""
    so, h = getattr(ctx, "so", None) or ctx.lib, ctx.h
    gapped = "gaps" in rec
    fields = GAP_RECORD_FIELDS if gapped else RECORD_FIELDS
    held = {f: np.ascontiguousarray(rec[f], dtype=dt) for f, dt in fields}
    n = len(held["contig"])
    out = {} if out is None else out
    if "order" not in out:
        out["order"] = np.zeros(n, np.int64)
    if gather:
        for f, dt in ORDER_COLUMNS:
            out.setdefault(f, np.zeros(n, dt))
    a = L.WfOrderIn(n=n, max_target_seqs=int(max_target_seqs),
                    **{f: L.ptr(held[f]) if f in held else None for f, _ in GAP_RECORD_FIELDS})
    o = L.WfOrderOut(n_kept=-1, **{f: L.ptr(out[f]) for f in out})
    rc = so.wf_order_records(h, C.byref(a), C.byref(o))
    if rc != L.WF_OK:
        raise L.WaafleHipError(rc, so.wf_last_error(h).decode())
    k = int(o.n_kept)
    order = out["order"][:k]
    return (order, {f: out[f][:k] for f, _ in ORDER_COLUMNS}) if gather else order


HSP_FIELDS = (("contig", np.int32), ("subject", np.int32), ("minus", np.uint8), ("delta", np.int32),
              ("b", np.int32), ("e", np.int32), ("score", np.int32))
ANCHOR_FIELDS = (("contig", np.int32), ("subject", np.int32), ("minus", np.uint8), ("i0", np.int32),
                 ("j0", np.int32)) + tuple((side + "_" + f, np.int32) for side in ("left", "right") for f in "Hpqg")


def report_once(ctx, raw, min_score, capacity, out=None):
    """One wf_search_report call (raw: the HSP_FIELDS columns) or, when raw has "i0", one
    wf_search_report_gapped call (the ANCHOR_FIELDS columns), in the form the context's
    WF_OPT_SEARCH_REPORT selects.  `ctx` as for order_records_device.  Returns (return code, full
    record count, the records written, the call's counters); out: the arrays to write into."""
    so, h = getattr(ctx, "so", None) or ctx.lib, ctx.h
    gapped = "i0" in raw
    fields = GAP_RECORD_FIELDS if gapped else RECORD_FIELDS
    held = {f: np.ascontiguousarray(raw[f], dtype=dt) for f, dt in (ANCHOR_FIELDS if gapped else HSP_FIELDS)}
    out = {f: np.zeros(capacity, dt) for f, dt in fields} if out is None else out
    n = len(held["contig"])
    if gapped:
        a = L.WfReportAnchors(n=n, min_score=int(min_score), **{f: L.ptr(v) for f, v in held.items()})
        r = L.WfSearchGapResult(capacity=capacity, n=-1, **{f: L.ptr(out[f]) for f, _ in fields})
        rc = so.wf_search_report_gapped(h, C.byref(a), C.byref(r))
    else:
        a = L.WfReportHsps(n=n, min_score=int(min_score), **{f: L.ptr(v) for f, v in held.items()})
        r = L.WfSearchResult(capacity=capacity, n=-1, **{f: L.ptr(out[f]) for f, _ in fields})
        rc = so.wf_search_report(h, C.byref(a), C.byref(r))
    full = int(r.n)
    stats = {f: int(getattr(r, f)) for f in (GAP_STAT_FIELDS if gapped else STAT_FIELDS)}
    return rc, full, {f: out[f][:max(0, min(full, capacity))] for f, _ in fields}, stats


def report_records(ctx, raw, min_score):
    """The records of the raw HSPs (or anchors with their sides) `raw`: report_once with room for
    every one of them.  Raises lib.WaafleHipError.  Returns (records, counters)."""
    so, h = getattr(ctx, "so", None) or ctx.lib, ctx.h
    rc, _, out, stats = report_once(ctx, raw, min_score, max(len(raw["contig"]), 1))
    if rc != L.WF_OK:
        raise L.WaafleHipError(rc, so.wf_last_error(h).decode())
    return out, stats


def order_with(ctx, rec, max_target_seqs, order_on="host", gather=False, say=lambda *a: None):
    """The order of `rec` by the host function or, with order_on "device", on the GPU of the open
    context `ctx`; when the device has no room, one line through `say` and the host function.
    gather: (order, the nine columns of hits.record_columns)."""
    if order_on == "device":
        try:
            return order_records_device(ctx, rec, max_target_seqs, gather=gather)
        except L.WaafleHipError as exc:
            if exc.code != L.WF_E_NOMEM:
                raise
            say("  no device memory to order {:,} records: ordering on the host".format(len(rec["contig"])))
    order = order_records(rec, max_target_seqs)
    if not gather:
        return order
    from . import hits
    return order, hits.record_columns(rec, order)


def bitscore_text(score):
    bits = (LAMBDA * score - math.log(K)) / math.log(2)
    return str(int(bits)) if bits > 99.9 else "%.1f" % bits


def evalue(qlen, db_bases, score):
    """K qlen D exp(-LAMBDA score); infinite where exp overflows (a score below about -550, which
    no search reports: records made by hand)."""
    try:
        return K * qlen * db_bases * math.exp(-LAMBDA * score)
    except OverflowError:
        return math.inf


def format_rows(rec, order, contig_names, contig_lens, subject_ids, subject_lens, db_bases):
    """The 15 columns of utils.c_blast_fields, tab-separated, 1-based; a minus HSP has
    descending subject coordinates.  evalue = K qlen D exp(-LAMBDA score), D the database's
    bases: no length adjustment, not BLAST's effective-length value.  Gapped records: length
    counts the alignment's columns, the gaps column holds the gap columns and the score is
    score2 / 2, which may end in .5."""
    out = []
    if "gaps" in rec:
        cols = [rec[f][order].tolist() for f, _ in GAP_RECORD_FIELDS]
        for c, g, minus, qs, qn, ss, sn, length, m, gaps in zip(*cols):
            score, M, qlen = (6 * m - 4 * length - gaps) / 2, int(subject_lens[g]), int(contig_lens[c])
            s0, s1 = (M - ss, M - ss - sn + 1) if minus else (ss + 1, ss + sn)
            ev = evalue(qlen, db_bases, score)
            out.append("\t".join(str(v) for v in (
                contig_names[c], subject_ids[g], qlen, M, length, qs + 1, qs + qn, s0, s1,
                "%.3f" % (100.0 * m / length), m, gaps, "%.2e" % ev, bitscore_text(score),
                "minus" if minus else "plus")))
        return out
    cols = [rec[f][order].tolist() for f, _ in RECORD_FIELDS]
    for c, g, minus, qs, ss, length, m in zip(*cols):
        score, M, qlen = 3 * m - 2 * length, int(subject_lens[g]), int(contig_lens[c])
        s0, s1 = (M - ss, M - ss - length + 1) if minus else (ss + 1, ss + length)
        ev = evalue(qlen, db_bases, score)
        out.append("\t".join(str(v) for v in (
            contig_names[c], subject_ids[g], qlen, M, length, qs + 1, qs + length, s0, s1,
            "%.3f" % (100.0 * m / length), m, 0, "%.2e" % ev, bitscore_text(score),
            "minus" if minus else "plus")))
    return out


def search_files(query, db, out_path, device=0, chunk_bases=CHUNK_BASES, max_target_seqs=MAX_TARGET_SEQS,
                 say=lambda *a: None, gapped=False, band=15, xdrop_gap=30, dust=False, dust_window=64,
                 dust_level=20, dust_out=None, order_on="host", **params):
    """The native search of `db`, a genes' FASTA or a packed database (makedb: told by its
    magic), against the contigs `query`, written to `out_path`;
    gapped: the alignments of the gapped extension in place of the ungapped HSPs; dust: seeds
    from the contigs' unmasked S-mers only, and with dust_out the masked intervals written there;
    order_on "device": the table's order from wf_order_records in place of order_records;
    report_on "device" (passed on to the Searcher): each chunk's reporting step on the GPU.
    Returns the searcher's counters plus rows, subjects and database bases."""
    names, seq, off = mapper.read_fasta(query)
    rec, ids, lens, stats, order = search_ordered(
        names, seq, off, db, max_target_seqs, order_on=order_on, device=device, chunk_bases=chunk_bases, say=say,
        gapped=gapped, band=band, xdrop_gap=xdrop_gap, dust=dust, dust_window=dust_window, dust_level=dust_level,
        dust_out=dust_out, **params)
    rows = format_rows(rec, order, names, np.diff(off), ids, lens, int(lens.sum()))
    with open(out_path, "w") as fh:
        fh.write("".join(r + "\n" for r in rows))
    stats.update(rows=len(rows), subjects=len(ids), db_bases=int(lens.sum()))
    return stats


def search_records(names, seq, off, db, device=0, chunk_bases=CHUNK_BASES, say=lambda *a: None, gapped=False, band=15,
                   xdrop_gap=30, dust=False, dust_window=64, dust_level=20, dust_out=None, **params):
    """The search of search_files, up to its records: `db` chunk by chunk against the contigs
    (names, seq, off as mapper.read_fasta gives them).  Returns (records with database-wide
    subject numbers, in the order found; the subjects' ids; their lengths; the searcher's
    counters)."""
    with Searcher(seq, off, device=device, band=band, xdrop_gap=xdrop_gap, dust=dust, dust_window=dust_window,
                  dust_level=dust_level, **params) as s:
        return _records_of(s, names, seq, off, db, chunk_bases, say, gapped, dust, dust_out)


def search_ordered(names, seq, off, db, max_target_seqs=MAX_TARGET_SEQS, order_on="host", gather=False,
                   device=0, chunk_bases=CHUNK_BASES, say=lambda *a: None, gapped=False, band=15, xdrop_gap=30,
                   dust=False, dust_window=64, dust_level=20, dust_out=None, before_order=None, **params):
    """search_records and the table's order of its records (order_with), found while the
    searcher's context is still open: what search_records returns, then the order, or with
    gather (order, columns).  before_order: called between the two (a timer's lap)."""
    with Searcher(seq, off, device=device, band=band, xdrop_gap=xdrop_gap, dust=dust, dust_window=dust_window,
                  dust_level=dust_level, **params) as s:
        found = _records_of(s, names, seq, off, db, chunk_bases, say, gapped, dust, dust_out)
        if before_order:
            before_order()
        return found + (order_with(s, found[0], max_target_seqs, order_on, gather=gather, say=say),)


def _records_of(s, names, seq, off, db, chunk_bases, say, gapped, dust, dust_out):
    """search_records on the open Searcher `s`"""
    fields = GAP_RECORD_FIELDS if gapped else RECORD_FIELDS
    ids, lens, parts = [], [], []
    if dust:
        say("  {:,} of {:,} contig bases masked; {:,} of {:,} seeds kept".format(
            s.dust_stats["masked_bases"], len(seq), s.dust_stats["kmers_after"], s.dust_stats["kmers_before"]))
        if dust_out:
            with open(dust_out, "w") as fh:
                fh.write("".join(r + "\n" for r in format_mask_rows(mask_intervals(s.mask(), off), names)))
    pdb = PackedDb(db) if is_packed_db(db) else None
    for item in (pdb.chunks(chunk_bases) if pdb else iter_subject_chunks(db, chunk_bases)):
        if pdb:
            cid, coff = range(item.first, item.last), item.off
            rec = search_chunk(s, item, None, gapped)
        else:
            cid, cseq, coff = item
            rec = search_chunk(s, cseq, coff, gapped)
        rec["subject"] = rec["subject"] + np.int32(len(ids))
        parts.append(rec)
        ids += cid                                       # a packed database: its subjects' numbers
        lens.append(np.diff(coff))
        say("  {:,} subjects searched, {:,} records".format(len(ids), sum(len(p["contig"]) for p in parts)))
    stats = dict(s.stats)
    rec = {f: np.concatenate([p[f] for p in parts]) if parts else np.zeros(0, dt) for f, dt in fields}
    lens = np.concatenate(lens) if lens else np.zeros(0, np.int64)
    return rec, (pdb.ids if pdb else ids), lens, stats


# ---------------------------------------------------------------------------
# cli
# ---------------------------------------------------------------------------

def build_parser():
    ap = argparse.ArgumentParser(
        description="Step 1 in the WAAFLE pipeline: search a set of contigs against a WAAFLE database,\n"
                    "with blastn (the reference's command) or with the built-in GPU search (ungapped, or\n"
                    "with --gapped the banded gapped extension of its HSPs).",
        formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("query", help="contigs file (fasta format)")
    ap.add_argument("db", help="path to WAAFLE BLAST database; with --searcher native: the genes' FASTA\n"
                               "file (plain or .gz) with WAAFLE headers (id|taxon|system=name...), or the\n"
                               ".wfdb file that `python -m waafle_amd.makedb genes.fna --out genes.wfdb`\n"
                               "makes of it once: the genes as bit planes, which a search maps and sends\n"
                               "to the GPU as they are (no FASTA parsing per run, 3/8 of the bytes; the\n"
                               "same table).  The binary files of a BLAST database cannot be read: get\n"
                               "the FASTA with `blastdbcmd -db <db> -entry all`")
    ap.add_argument("--blastn", default="blastn", metavar="<path>", help="path to blastn binary\n[default: $PATH]")
    ap.add_argument("--threads", default="1", metavar="<int>",
                    help="number of CPU cores to use in blastn search\n[default: 1]")
    ap.add_argument("--out", default=None, metavar="<path>",
                    help="path for blast output file\n[default: <derived from input>]")
    ap.add_argument("--searcher", choices=["blastn", "native"], default="blastn",
                    help="blastn: run the reference's blastn command; native: the built-in\n"
                         "seed-and-extend search on the GPU (not a blastn clone; ungapped HSPs unless\n"
                         "--gapped is given)\n[default: blastn]")
    g = ap.add_argument_group("native search (defaults are choices, not measured optima)")
    g.add_argument("--seed-length", type=int, default=DEFAULTS["seed_length"], metavar="<12..32>")
    g.add_argument("--seed-stride", type=int, default=DEFAULTS["seed_stride"], metavar="<1..32>")
    g.add_argument("--max-seed-hits", type=int, default=DEFAULTS["max_seed_hits"], metavar="<1..1024>",
                   help="a seed with more occurrences in the contigs is unused")
    g.add_argument("--xdrop", type=int, default=DEFAULTS["xdrop"], metavar="<1..1000>")
    g.add_argument("--min-score", type=int, default=DEFAULTS["min_score"], metavar="<int>",
                   help="least raw score (match +1, mismatch -2) reported")
    g.add_argument("--max-target-seqs", type=int, default=MAX_TARGET_SEQS, metavar="<int>")
    g.add_argument("--order-on", choices=["host", "device"], default="host",
                   help="where the table's order and --max-target-seqs are computed: host (numpy) or\n"
                        "device (wf_order_records on the GPU; the same table)\n[default: host]")
    g.add_argument("--report-on", choices=["host", "device"], default="host",
                   help="where each chunk's reporting step (duplicates, contained or covered hits,\n"
                        "--min-score, the records' order) runs: host (C++) or device (the raw hits stay\n"
                        "on the GPU; the same table)\n[default: host]")
    g.add_argument("--chunk-bases", type=int, default=CHUNK_BASES, metavar="<int>",
                   help="subject bases per device call")
    g.add_argument("--gpu", type=int, default=0, metavar="<int>")
    g.add_argument("--gapped", action="store_true",
                   help="extend every ungapped HSP by a banded x-drop alignment with linear gap cost\n"
                        "(match +1, mismatch -2, gap column -2.5) and report those alignments\n[default: off]")
    g.add_argument("--band", type=int, default=GAP_DEFAULTS["band"], metavar="<1..31>",
                   help="--gapped: diagonals either way of the anchor's, per side")
    g.add_argument("--xdrop-gap", type=int, default=GAP_DEFAULTS["xdrop_gap"], metavar="<1..1000>",
                   help="--gapped: x-drop of the gapped extension, raw score")
    g.add_argument("--dust", action="store_true",
                   help="mask the contigs' low-complexity stretches (symmetric DUST, the published\n"
                        "definition; agreement with NCBI dustmasker is not measured): they give no\n"
                        "seeds, extensions still run through them.  blastn's default is on\n[default: off]")
    g.add_argument("--dust-window", type=int, default=DUST_DEFAULTS["dust_window"], metavar="<8..64>",
                   help="--dust: the longest interval scored, in bases")
    g.add_argument("--dust-level", type=int, default=DUST_DEFAULTS["dust_level"], metavar="<int>",
                   help="--dust: an interval is masked when its score exceeds level / 10")
    g.add_argument("--dust-out", default=None, metavar="<path>",
                   help="--dust: write the masked intervals there, one per line in FASTA order:\n"
                        "contig name, start, end (0-based, half-open)")
    return ap


def default_out(query):
    """utils.path2name / name2path: ./<file name up to its first dot>.blastout"""
    return os.path.join(".", os.path.split(query)[1].split(".")[0] + ".blastout")


def blastn_command(args):
    """waafle_search.py:94-112, the same string."""
    return " ".join(["{BLASTN}", "-query {QUERY}", "-db {DB}", "-out {OUTFILE}", "-max_target_seqs {MAXTAR}",
                     "-num_threads {THREADS}", "-outfmt '{FORMAT}'"]).format(
        QUERY=args.query, OUTFILE=args.out, BLASTN=args.blastn, DB=args.db, MAXTAR=MAX_TARGET_SEQS,
        THREADS=args.threads, FORMAT=BLAST_FORMAT)


def die(*args):
    inputs.say(*(["LETHAL ERROR:"] + list(args)))
    sys.exit("EXITING.")


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.out is None:
        args.out = default_out(args.query)
    if args.searcher == "blastn":
        command = blastn_command(args)
        inputs.say("Executing command:", command)
        os.system(command)
        inputs.say("Finished successfully.")
        return
    if args.max_target_seqs < 1 or args.chunk_bases < 1:
        die("--max-target-seqs and --chunk-bases must be positive")
    if args.dust_out and not args.dust:
        die("--dust-out needs --dust")
    try:
        stats = search_files(args.query, args.db, args.out, device=args.gpu, chunk_bases=args.chunk_bases,
                             max_target_seqs=args.max_target_seqs, say=inputs.say,
                             seed_length=args.seed_length, seed_stride=args.seed_stride,
                             max_seed_hits=args.max_seed_hits, xdrop=args.xdrop, min_score=args.min_score,
                             gapped=args.gapped, band=args.band, xdrop_gap=args.xdrop_gap, dust=args.dust,
                             dust_window=args.dust_window, dust_level=args.dust_level, dust_out=args.dust_out,
                             order_on=args.order_on, report_on=args.report_on)
    except (inputs.InputError, OSError, L.WaafleHipError) as exc:
        die(str(exc))
    inputs.say("Finished successfully ({:,} rows from {:,} subjects; {:,} seed hits).".format(
        stats["rows"], stats["subjects"], stats["seed_hits"]))


if __name__ == "__main__":
    main()
