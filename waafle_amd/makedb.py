"""Format a gene database once for the native search (the `makeblastdb` step of waafle_search
--searcher native).

    python -m waafle_amd.makedb genes.fna[.gz] --out genes.wfdb [--chunk-bases N]

The genes' FASTA (WAAFLE headers, read by the rules of search.iter_subject_chunks) becomes one
.wfdb file: the subjects' offsets and ids, and the bases as the three bit
planes the search kernels use, laid out so that `search.PackedDb` maps the file and a search
hands slices of it to wf_search_packed as they are.  Runs on the host, with numpy, without a
GPU.  Bases as in the store (csrc/wf_mapstore.h base_code): lower case counts as upper case,
A C G T are 0 1 2 3, every other byte is an N.

Memory: `--chunk-bases` bases are held at a time (and at least one FASTA line); offsets, ids
and planes are spilled to part files beside the output as they are made and joined at the
end, so nothing grows with the database.  The file's bytes do not depend on `--chunk-bases`.
"""
from __future__ import annotations

import argparse
import os
import shutil
import sys
import time

import numpy as np

from . import inputs, search as S

CHUNK_BASES = 1 << 26
PARTS = ("off", "id_off", "ids", "lo", "hi", "nn")          # the file's sections, in order

CODE = np.full(256, 4, np.uint8)                             # base_code of csrc/wf_mapstore.h
for _i, _ch in enumerate(b"ACGT"):
    CODE[_ch] = CODE[_ch + 32] = _i


def pack_words(bases):
    """The planes (lo, hi, nn: little-endian uint32) of len(bases) bases, a multiple of 32:
    base i is bit i & 31 of word i >> 5; lo and hi are 0 under nn."""
    code = CODE[bases]
    return tuple(np.packbits(bits, bitorder="little").view("<u4")
                 for bits in (code & 1, (code >> 1) & 1, code >> 2))


def make_db(fasta, out_path, chunk_bases=CHUNK_BASES):
    """Write the packed database of the FASTA `fasta` to `out_path`; {subjects, bases, bytes}."""
    chunk_bases = max(int(chunk_bases), 1)
    paths = {p: "{}.part-{}".format(out_path, p) for p in PARTS}
    tmp = "{}.tmp".format(out_path)
    n = total = id_bytes = 0
    try:
        part = {p: open(paths[p], "wb") for p in PARTS}
        try:
            held, held_bases = [], 0                         # sequence lines not yet packed
            offs, id_offs = [0], [0]                         # offsets not yet written

            def flush(final):
                nonlocal held, held_bases, offs, id_offs
                bases = np.frombuffer(b"".join(held), dtype=np.uint8)
                if final:                                    # the last word's padding and two words more: all N
                    bases = np.concatenate([bases, np.zeros(-len(bases) % 32 + 64, np.uint8)])
                keep = len(bases) - len(bases) % 32          # whole words; the rest is carried over
                for p, words in zip(("lo", "hi", "nn"), pack_words(bases[:keep])):
                    part[p].write(words.tobytes())
                held = [bases[keep:].tobytes()] if keep < len(bases) else []
                held_bases = len(bases) - keep
                part["off"].write(np.asarray(offs, "<i8").tobytes())
                part["id_off"].write(np.asarray(id_offs, "<i8").tobytes())
                offs, id_offs = [], []

            with S._open(fasta) as fh:
                for line in fh:
                    line = line.strip()
                    if not line:
                        continue
                    if line[:1] == b">":
                        sid = S.subject_id(line).encode()
                        if n:                                # the previous subject ends here
                            offs.append(total)
                            id_offs.append(id_bytes)
                        part["ids"].write(sid)
                        id_bytes += len(sid)
                        n += 1
                    else:
                        if not n:
                            raise S.headless_error(fasta)
                        held.append(line)
                        held_bases += len(line)
                        total += len(line)
                    if held_bases >= chunk_bases + 32 or len(offs) >= chunk_bases:
                        flush(False)
            if n:
                offs.append(total)
                id_offs.append(id_bytes)
            flush(True)
        finally:
            for fh in part.values():
                fh.close()
        words = (total + 31) // 32 + 2
        sec, length = S.db_sections(n, words, id_bytes)
        with open(tmp, "wb") as out:
            out.write(S.DB_HEADER.pack(S.DB_MAGIC, S.DB_VERSION, 0, n, total, words, id_bytes))
            for p in PARTS:
                out.write(b"\0" * (sec[p][0] - out.tell()))
                with open(paths[p], "rb") as src:
                    shutil.copyfileobj(src, out, 1 << 24)
            out.write(b"\0" * (length - out.tell()))
        os.replace(tmp, out_path)
    finally:
        for p in list(paths.values()) + [tmp]:
            if os.path.exists(p):
                os.remove(p)
    return dict(subjects=n, bases=total, bytes=length)


def main(argv=None):
    ap = argparse.ArgumentParser(
        description="Format a WAAFLE gene FASTA once as a packed database (.wfdb) for\n"
                    "`python -m waafle_amd.search ... --searcher native`: a search then maps the file and\n"
                    "streams its bit planes to the GPU, without parsing the FASTA on every run.",
        formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("fasta", help="the genes' FASTA file (plain or .gz) with WAAFLE headers (id|taxon|...)")
    ap.add_argument("--out", required=True, metavar="<path>", help="the database file to write")
    ap.add_argument("--chunk-bases", type=int, default=CHUNK_BASES, metavar="<int>",
                    help="bases held in memory at a time; the file does not depend on it\n[default: 2^26]")
    args = ap.parse_args(argv)
    if args.chunk_bases < 1:
        sys.exit("--chunk-bases must be positive")
    t0 = time.perf_counter()
    try:
        st = make_db(args.fasta, args.out, args.chunk_bases)
    except (inputs.InputError, OSError) as exc:
        inputs.say("LETHAL ERROR:", str(exc))
        sys.exit("EXITING.")
    inputs.say("{}: {:,} subjects, {:,} bases, {:,} bytes in {:.1f} s".format(
        args.out, st["subjects"], st["bases"], st["bytes"], time.perf_counter() - t0))


if __name__ == "__main__":
    main()
