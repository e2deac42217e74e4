"""Throughput of the built-in homology search (wf_map_index / wf_search / wf_search_gapped) on
one MI355X.

    python scripts/search_bench.py [--contigs 10000 --contig-length 5000 --db-bases 200000000
                                    --subject-length 1000 --homolog-share 0.01 --chunk-bases 67108864
                                    --indel-rate 0.003 --gapped --band 15 --xdrop-gap 30
                                    --low-complexity 2000 --dust --packed --report-on device
                                    --family 1000 --compare-report 3]
    python scripts/search_bench.py --files [--tmp-dir DIR]

Not bench.py (the flagship workload); the numbers go to DESIGN.md §12 and profiles/search/.
The workload is seeded: random contigs, and a database of random subjects of which a share
--homolog-share is cut from the contigs (either strand) with 0..10 % substitutions, that is
90..100 % identity; with --indel-rate r every planted homolog also gets Poisson(r x length)
indels of 1..6 bases, half insertions, half deletions (its length stays --subject-length: it
is cut longer and trimmed).  --gapped runs `Searcher.search_gapped` in place of
`Searcher.search`.  --low-complexity n writes n low-complexity stretches (homopolymers and
2..4-base repeats of 30..80 bases) over bases of the contigs and n over random subjects; --dust
masks the contigs (`wf_search_mask`) before the search and reports the mask's
counters and the wall of that call (mask kernel, index rebuild and the mask's copy to the
host).  The search parameters are the defaults (S 21, T 8, max_occ 64, X 20,
min_score 28).  --family n plants every gene n times: n database subjects cut from the same
place of the same contig, each with its own 0..2 % substitutions (a gene family present in n
species), so that one chunk carries 10^5 to 10^7 raw HSPs of which the reporting step keeps few.
--report-on device runs that step on the GPU (WF_OPT_SEARCH_REPORT).
--compare-report k measures both forms in one process: two searchers on the same contigs, one
warm-up pass over every chunk each, then k passes each, interleaved host, device, host, ...; a
pass's wall is the sum of its search calls, which return after a synchronisation; the records of
the two forms must be equal.  The GPU step runs in a child process under its own time limit
(--step-timeout); when it fails or runs out of time nothing more is started.

  search  `Searcher.search` on host-resident subjects in chunks of --chunk-bases (copies in
          and out and the host's de-duplication included), after one warm-up chunk of 2^20
          bases: wall per chunk, subject bases per second, the seed-hit, extended-HSP and record
          counts, the share of seed hits skipped by the predecessor shortcut, and the share of
          the planted homologs with at least one record, and with a record that covers at
          least 0.75 of the subject (the scorer's default --min-scov)

  --packed  the same chunks given as the bit planes of a packed database:
          the subjects are packed once, outside the timing, as `makedb` lays them out, and every
          chunk is `Searcher.search_packed` (`search_gapped_packed`) on slices of those planes;
          h2d_bytes_per_chunk is what either form copies to the device for the bases
  --files   the file leg: the workload written once as FASTA (60-column lines; the contigs too)
          and once as .wfdb (`makedb`, timed) under a temporary directory, then `search_files`
          on each, first with the database file's pages evicted (posix_fadvise DONTNEED after
          fsync: "cold", as far as the file system honours it), then again ("warm"); the two
          tables must be equal.  Walls include reading the contigs and indexing them.

Prints one JSON line.  For per-kernel times run the step under
`rocprofv3 --kernel-trace --stats -- python scripts/search_bench.py --step search ...`.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

ASCII = np.frombuffer(b"ACGT", dtype=np.uint8)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--contigs", type=int, default=10000)
    ap.add_argument("--contig-length", type=int, default=5000)
    ap.add_argument("--db-bases", type=int, default=200000000)
    ap.add_argument("--subject-length", type=int, default=1000)
    ap.add_argument("--homolog-share", type=float, default=0.01)
    ap.add_argument("--chunk-bases", type=int, default=1 << 26, help="subject bases per wf_search call")
    ap.add_argument("--indel-rate", type=float, default=0.0, help="indels per base of a planted homolog")
    ap.add_argument("--gapped", action="store_true", help="wf_search_gapped in place of wf_search")
    ap.add_argument("--band", type=int, default=15)
    ap.add_argument("--xdrop-gap", type=int, default=30)
    ap.add_argument("--low-complexity", type=int, default=0,
                    help="low-complexity stretches written over the contigs, and as many over random subjects")
    ap.add_argument("--dust", action="store_true", help="wf_search_mask on the contigs before the search")
    ap.add_argument("--report-on", choices=["host", "device"], default="host",
                    help="where each chunk's reporting step runs")
    ap.add_argument("--family", type=int, default=0, metavar="<copies>",
                    help="every planted gene in this many near-identical subjects (0: each planted once)")
    ap.add_argument("--compare-report", type=int, default=0, metavar="<runs>",
                    help="both forms of the reporting step in one process, interleaved, this many passes each")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--packed", action="store_true", help="the subjects as bit planes (wf_search_packed)")
    ap.add_argument("--files", action="store_true", help="the file leg: search_files on a FASTA and on its .wfdb")
    ap.add_argument("--tmp-dir", default=None, help="--files: where the temporary directory goes")
    ap.add_argument("--step", choices=["search", "files"], help="run the step in this process")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds for the GPU step")
    return ap.parse_args(argv)


def make_workload(a):
    """(contig codes, contig offsets, subject codes [n, L], homolog flags)."""
    rng = np.random.default_rng(a.seed)
    codes = rng.integers(0, 4, a.contigs * a.contig_length, dtype=np.uint8)
    off = np.arange(a.contigs + 1, dtype=np.int64) * a.contig_length
    L = a.subject_length
    n = a.db_bases // L
    subj = rng.integers(0, 4, (n, L), dtype=np.uint8)
    hom = np.flatnonzero(rng.random(n) < a.homolog_share)
    c = rng.integers(0, a.contigs, len(hom))
    p = rng.integers(0, a.contig_length - L + 1, len(hom))
    if a.family > 0:                                          # the members of a family share their gene's place
        first = np.arange(len(hom)) // a.family * a.family
        c, p = c[first], p[first]
    cut = codes[(off[c] + p)[:, None] + np.arange(L, dtype=np.int64)[None, :]]
    rate = rng.random(len(hom))[:, None] * (0.02 if a.family > 0 else 0.10)   # 90..100 % identity; a family 98..100 %
    sub = rng.random(cut.shape) < rate
    cut = (cut + sub * rng.integers(1, 4, cut.shape, dtype=np.uint8)).astype(np.uint8) & 3
    if a.indel_rate > 0:                                      # a stream of its own: rate 0 is the old workload
        rng2 = np.random.default_rng(a.seed + 1)
        for k in range(len(hom)):
            p0 = min(int(p[k]), a.contig_length - L - 64)     # room for what the deletions take
            row = list(cut[k] if p0 == p[k] else codes[off[c[k]] + p0:off[c[k]] + p0 + L])
            row += list(codes[off[c[k]] + p0 + L:off[c[k]] + p0 + L + 64])
            for _ in range(min(int(rng2.poisson(a.indel_rate * L)), 10)):
                at, m = int(rng2.integers(10, L - 10)), int(rng2.integers(1, 7))
                if rng2.random() < 0.5:
                    del row[at:at + m]
                else:
                    row[at:at] = rng2.integers(0, 4, m).tolist()
            cut[k] = np.array(row[:L], np.uint8)
    minus = rng.random(len(hom)) < 0.5
    cut[minus] = 3 - cut[minus][:, ::-1]
    subj[hom] = cut
    if a.low_complexity > 0:                                  # a stream of its own: 0 is the old workload
        rng3 = np.random.default_rng(a.seed + 2)
        rows = np.setdiff1d(np.arange(n), hom)
        for where in ("contigs", "subjects"):
            for _ in range(a.low_complexity):
                unit = rng3.integers(0, 4, int(rng3.integers(1, 5)), dtype=np.uint8)
                m = int(rng3.integers(30, 81))
                rep = np.tile(unit, m // len(unit) + 1)[:m]
                if where == "contigs":
                    at = off[int(rng3.integers(0, a.contigs))] + int(rng3.integers(0, a.contig_length - m + 1))
                    codes[at:at + m] = rep
                else:
                    at = int(rng3.integers(0, L - m + 1))
                    subj[rows[int(rng3.integers(0, len(rows)))], at:at + m] = rep
    return codes, off, subj, hom


def pack_subjects(subj):
    """[n, L] codes as a makedb would lay them out: (off, lo, hi, nn), a database in memory"""
    import types
    from waafle_amd import makedb
    n, L = subj.shape
    rows = max((1 << 25) // L // 32 * 32, 32)                 # whole words per piece
    parts = []
    for lo in range(0, n, rows):
        bases = ASCII[subj[lo:lo + rows]].reshape(-1)
        parts.append(makedb.pack_words(np.concatenate([bases, np.zeros(-len(bases) % 32, np.uint8)])))
    parts.append(makedb.pack_words(np.zeros(64, np.uint8)))  # the two padding words
    lo, hi, nn = (np.concatenate([p[k] for p in parts]) for k in range(3))
    return types.SimpleNamespace(off=np.arange(n + 1, dtype=np.int64) * L, lo=lo, hi=hi, nn=nn)


def step_search(a):
    from waafle_amd import search
    codes, off, subj, hom = make_workload(a)
    n, L = subj.shape
    per = max(a.chunk_bases // L, 1)
    db = pack_subjects(subj) if a.packed else None
    walls, records, found, span = [], 0, np.zeros(n, bool), np.zeros(n, np.int64)
    gap = dict(band=a.band, xdrop_gap=a.xdrop_gap) if a.gapped else {}
    dust = {}
    if a.compare_report > 0:
        return compare_report(a, search, codes, off, subj, per, db, gap)
    with search.Searcher(ASCII[codes], off, device=a.gpu, report_on=a.report_on, **gap) as s:
        if a.dust:
            t0 = time.perf_counter()
            s.apply_mask(len(codes))
            dust = dict(s.dust_stats, mask_call_s=time.perf_counter() - t0,
                        masked_fraction=s.dust_stats["masked_bases"] / max(len(codes), 1))
            t0 = time.perf_counter()
            s.apply_mask(len(codes))                          # again, with everything allocated
            dust["mask_call_again_s"] = time.perf_counter() - t0
        run = s.search_gapped if a.gapped else s.search
        run_packed = s.search_gapped_packed if a.gapped else s.search_packed
        w = min(n, max((1 << 20) // L, 1))
        if a.packed:                                          # warm-up chunk
            run_packed(search.PackedChunk(db, 0, w))
        else:
            run(ASCII[subj[:w]].reshape(-1), np.arange(w + 1, dtype=np.int64) * L)
        s.stats = dict.fromkeys(s.stats, 0)
        copied, raw_per_chunk, records_per_chunk = [], [], []
        for lo in range(0, n, per):
            hi = min(lo + per, n)
            if a.packed:
                chunk = search.PackedChunk(db, lo, hi)
                copied.append(12 * len(chunk.lo))
                t0 = time.perf_counter()
                rec = run_packed(chunk)
            else:
                seq = ASCII[subj[lo:hi]].reshape(-1)
                soff = np.arange(hi - lo + 1, dtype=np.int64) * L
                copied.append(len(seq))
                t0 = time.perf_counter()
                rec = run(seq, soff)
            walls.append(time.perf_counter() - t0)
            records += len(rec["contig"])
            found[rec["subject"].astype(np.int64) + lo] = True
            np.maximum.at(span, rec["subject"].astype(np.int64) + lo, rec["sspan" if a.gapped else "length"])
            raw_per_chunk.append(s.stats["raw_hsps"] - sum(raw_per_chunk))
            records_per_chunk.append(len(rec["contig"]))
        stats = dict(s.stats)
    total = sum(walls)
    return dict(search_s=total, chunk_s=walls, chunk_bases=per * L, subject_bases_per_s=n * L / total,
                subjects=n, homologs=int(len(hom)), homologs_found_fraction=float(found[hom].mean()) if len(hom) else 0.0,
                homologs_scov_075=int((span[hom] >= 0.75 * L).sum()), gapped=bool(a.gapped),
                packed=bool(a.packed), h2d_bytes_per_chunk=copied, report_on=a.report_on, family=a.family,
                raw_hsps_per_chunk=raw_per_chunk, records_per_chunk=records_per_chunk,
                anchors=stats.get("anchors", 0), raw_alignments=stats.get("raw_alignments", 0),
                other_subjects_with_records=int(found.sum() - found[hom].sum()), records=records,
                seed_hits=stats["seed_hits"], seeds_skipped=stats["seeds_skipped"], raw_hsps=stats["raw_hsps"],
                skipped_share=stats["seeds_skipped"] / max(stats["seed_hits"], 1), dust=dust,
                timing="host-resident subjects: copies in and out and the host's de-duplication included, "
                       "one warm-up chunk")


def compare_report(a, search, codes, off, subj, per, db, gap):
    """--compare-report: the two forms of the reporting step on the same chunks in one process"""
    n, L = subj.shape
    chunks = []
    for lo in range(0, n, per):
        hi = min(lo + per, n)
        chunks.append(search.PackedChunk(db, lo, hi) if a.packed else
                      (ASCII[subj[lo:hi]].reshape(-1), np.arange(hi - lo + 1, dtype=np.int64) * L))
    forms = ("host", "device")
    fields = [f for f, _ in (search.GAP_RECORD_FIELDS if a.gapped else search.RECORD_FIELDS)]
    searchers = {w: search.Searcher(ASCII[codes], off, device=a.gpu, report_on=w, dust=a.dust, **gap) for w in forms}
    walls = {w: [] for w in forms}
    chunk_walls = {w: [] for w in forms}
    out = {}
    try:
        def one_pass(w, keep):
            s = searchers[w]
            s.stats = dict.fromkeys(s.stats, 0)
            t, recs, raw, per_chunk = [], [], [], []
            for ch in chunks:
                before = s.stats["raw_hsps"]
                t0 = time.perf_counter()
                if a.packed:
                    rec = s.search_gapped_packed(ch) if a.gapped else s.search_packed(ch)
                else:
                    rec = s.search_gapped(*ch) if a.gapped else s.search(*ch)
                t.append(time.perf_counter() - t0)
                raw.append(s.stats["raw_hsps"] - before)
                per_chunk.append(len(rec["contig"]))
                if keep:
                    recs.append(rec)
            return t, recs, raw, per_chunk, dict(s.stats)

        kept = {}
        for w in forms:                                       # the warm-up pass; its records are compared
            _, kept[w], raw, per_chunk, stats = one_pass(w, True)
            out[w] = dict(raw_hsps_per_chunk=raw, records_per_chunk=per_chunk, stats=stats)
        equal = all((x[f] == y[f]).all() if len(x[f]) == len(y[f]) else False
                    for x, y in zip(kept["host"], kept["device"]) for f in fields)
        equal = equal and out["host"]["stats"] == out["device"]["stats"]
        kept.clear()
        for _ in range(a.compare_report):
            for w in forms:
                t = one_pass(w, False)[0]
                walls[w].append(sum(t))
                chunk_walls[w].append(t)
    finally:
        for s in searchers.values():
            s.close()
    return dict(compare_report=a.compare_report, gapped=bool(a.gapped), packed=bool(a.packed), family=a.family,
                chunks=len(chunks), chunk_bases=per * L, subjects=n, records_and_counters_equal=bool(equal),
                raw_hsps_per_chunk=out["host"]["raw_hsps_per_chunk"], records_per_chunk=out["host"]["records_per_chunk"],
                anchors=out["host"]["stats"].get("anchors", 0), seed_hits=out["host"]["stats"]["seed_hits"],
                pass_s=walls, chunk_s=chunk_walls,
                timing="each form: one warm-up pass over every chunk, then the passes of the two forms interleaved; "
                       "a pass is the sum of its search calls, host-resident subjects, each returning after a "
                       "synchronisation")


def evict(path):
    """Ask the kernel to drop the file's cached pages (they are clean after the fsync)."""
    fd = os.open(path, os.O_RDONLY)
    try:
        os.fsync(fd)
        os.posix_fadvise(fd, 0, 0, os.POSIX_FADV_DONTNEED)
    finally:
        os.close(fd)


def step_files(a):
    import shutil
    import tempfile
    from waafle_amd import makedb, search
    codes, off, subj, hom = make_workload(a)
    n, L = subj.shape
    d = tempfile.mkdtemp(prefix="search_bench_", dir=a.tmp_dir)
    out = dict(tmp_dir=d, subjects=n, db_bases=n * L)
    try:
        query, fasta, wfdb = (os.path.join(d, f) for f in ("contigs.fna", "genes.fna", "genes.wfdb"))

        def write_fasta(path, rows, name):
            with open(path, "wb") as fh:
                for i, row in enumerate(rows):
                    text = ASCII[row].tobytes()
                    fh.write(name(i) + b"\n".join(text[k:k + 60] for k in range(0, len(text), 60)) + b"\n")

        write_fasta(query, (codes[off[c]:off[c + 1]] for c in range(a.contigs)), lambda i: b">ctg%d\n" % i)
        t0 = time.perf_counter()
        write_fasta(fasta, subj, lambda i: b">g%d|s__S%d|UniProt=U%d\n" % (i, i % 97, i))
        out["write_fasta_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        makedb.make_db(fasta, wfdb)
        out["makedb_s"] = time.perf_counter() - t0
        out["fasta_bytes"], out["wfdb_bytes"] = os.path.getsize(fasta), os.path.getsize(wfdb)
        gap = dict(gapped=True, band=a.band, xdrop_gap=a.xdrop_gap) if a.gapped else {}
        t0 = time.perf_counter()
        search.mapper.read_fasta(query)
        out["read_contigs_s"] = time.perf_counter() - t0      # part of every wall below
        tables = {}
        for cache in ("cold", "warm"):
            for form, db in (("fasta", fasta), ("wfdb", wfdb)):
                if cache == "cold":
                    evict(db)
                table = os.path.join(d, form + ".blastout")
                t0 = time.perf_counter()
                st = search.search_files(query, db, table, device=a.gpu, chunk_bases=a.chunk_bases, dust=a.dust, **gap)
                out["search_files_{}_{}_s".format(form, cache)] = time.perf_counter() - t0
                out["rows"] = st["rows"]
                tables[form] = open(table, "rb").read()
            out["tables_equal_" + cache] = tables["fasta"] == tables["wfdb"]
    finally:
        shutil.rmtree(d, ignore_errors=True)
    out["cache"] = "cold: the database file's pages evicted by posix_fadvise(DONTNEED) after fsync, the contigs' " \
                   "file left cached; warm: the same call again"
    return out


def main(argv=None):
    a = parse(argv)
    if a.step:
        print("SEARCH_BENCH_STEP " + json.dumps(step_files(a) if a.step == "files" else step_search(a)))
        return 0
    out = dict(workload=dict(contigs=a.contigs, contig_length=a.contig_length, db_bases=a.db_bases,
                             subject_length=a.subject_length, homolog_share=a.homolog_share,
                             identity="90..100 %", indel_rate=a.indel_rate, seed=a.seed, gapped=a.gapped,
                             band=a.band, xdrop_gap=a.xdrop_gap, low_complexity=a.low_complexity, dust=a.dust,
                             packed=a.packed, files=a.files, report_on=a.report_on, family=a.family,
                             compare_report=a.compare_report,
                             params=dict(seed_length=21, seed_stride=8, max_seed_hits=64, xdrop=20, min_score=28)))
    passed = [x for x in (argv if argv is not None else sys.argv[1:])]
    cmd = [sys.executable, os.path.abspath(__file__), "--step", "files" if a.files else "search"] + passed
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, cwd=REPO)
    except subprocess.TimeoutExpired:
        print("the search step ran out of time ({} s); stopping".format(a.step_timeout), file=sys.stderr)
        return 2
    line = [l for l in r.stdout.splitlines() if l.startswith("SEARCH_BENCH_STEP ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stderr[-4000:])
        print("the search step failed (exit {}); stopping".format(r.returncode), file=sys.stderr)
        return 1
    out.update(json.loads(line[-1][len("SEARCH_BENCH_STEP "):]))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
