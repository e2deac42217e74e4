"""Throughput of the built-in read mapper (wf_map_index / wf_map_pairs) on one MI355X.

    python scripts/map_bench.py [--contigs 10000 --contig-length 5000 --pairs 2000000
                                 --read-length 150 --sub-rate 0.01 --indel-rate 0 --max-gap 0]

Not bench.py (the flagship workload); the numbers go to DESIGN.md §11 and profiles/.  The
workload is seeded: random contigs and error-carrying FR pairs drawn from them, half with
mate 1 on the reverse strand.  Each GPU step runs in a child process under its own time
limit (--step-timeout); after a step that fails or runs out of time nothing more is started.

  index   wf_map_index on the contigs (host bases in, index kept on the device): seconds
          per build, three builds
  map     wf_map_pairs on host-resident reads in chunks (copies in and out included):
          pairs per second after one warm-up chunk, the aligned fraction, and the fraction
          mapped back to the origin; with --max-gap, also the share of pairs the gapped pass
          receives (those the ungapped rule leaves unaligned) and the share it aligns

Prints one JSON line.  For per-kernel times run the map step under
`rocprofv3 --kernel-trace --stats -- python scripts/map_bench.py --step map ...`.
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
    ap.add_argument("--pairs", type=int, default=2000000)
    ap.add_argument("--read-length", type=int, default=150)
    ap.add_argument("--sub-rate", type=float, default=0.01)
    ap.add_argument("--indel-rate", type=float, default=0.0,
                    help="share of mates that carry one indel of 1..--indel-max bases")
    ap.add_argument("--indel-max", type=int, default=4)
    ap.add_argument("--max-gap", type=int, default=0, help="the mapper's max_gap (0: no gapped pass)")
    ap.add_argument("--insert", type=int, nargs=2, default=(200, 500), metavar=("MIN", "MAX"))
    ap.add_argument("--chunk", type=int, default=1 << 20, help="pairs per wf_map_pairs call")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--step", choices=["index", "map"], help="run one step in this process")
    ap.add_argument("--step-timeout", type=int, default=600, help="seconds per GPU step")
    return ap.parse_args(argv)


def make_contigs(a):
    rng = np.random.default_rng(a.seed)
    codes = rng.integers(0, 4, a.contigs * a.contig_length, dtype=np.uint8)
    off = np.arange(a.contigs + 1, dtype=np.int64) * a.contig_length
    return codes, off


def plant_indels(a, rng, codes, base, fwd, rev, fp, frag, pr):
    """One indel, at least 25 bases from either end of the read, in a share --indel-rate of
    the mates (before the substitutions).  A deletion in the reverse mate moves its start."""
    L = a.read_length
    for rows in (fwd, rev):
        for i in np.flatnonzero(rng.random(len(rows)) < a.indel_rate).tolist():
            g = int(rng.integers(1, a.indel_max + 1))
            d = -g if rng.random() < 0.5 else g
            k = int(rng.integers(25, L - 25 - g + 1))
            p = int(fp[i]) if rows is fwd else int(fp[i] + frag[i]) - L - d
            if p < 0 or p + L + d > a.contig_length:
                continue
            s0 = int(base[i]) + p
            if d < 0:
                plus = np.concatenate([codes[s0:s0 + k], rng.integers(0, 4, g, dtype=np.uint8),
                                       codes[s0 + k:s0 + L - g]])
            else:
                plus = np.concatenate([codes[s0:s0 + k], codes[s0 + k + d:s0 + L + d]])
            if rows is fwd:
                fwd[i] = plus
            else:
                rev[i] = 3 - plus[::-1]
                pr[i] = p + 1


def make_pairs(a, codes, off, block=1 << 17):
    """(mate-1 bases, mate-2 bases, offsets, truth): ASCII (pairs * L each)."""
    rng = np.random.default_rng(a.seed + 1)
    rng_indel = np.random.default_rng(a.seed + 2)          # the other draws stay as without indels
    L, n = a.read_length, a.pairs
    m1 = np.empty(n * L, np.uint8)
    m2 = np.empty(n * L, np.uint8)
    truth = np.empty((n, 4), np.int64)                      # contig, pos1, pos2, strand1
    col = np.arange(L, dtype=np.int64)[None, :]
    for lo in range(0, n, block):
        k = min(block, n - lo)
        c = rng.integers(0, a.contigs, k)
        frag = rng.integers(max(a.insert[0], L), min(a.insert[1], a.contig_length) + 1, k)
        fp = rng.integers(0, a.contig_length - frag + 1)
        fwd = codes[(off[c] + fp)[:, None] + col]
        rev = 3 - codes[(off[c] + fp + frag - L)[:, None] + col][:, ::-1]
        pf, pr = fp + 1, fp + frag - L + 1
        if a.indel_rate > 0:
            plant_indels(a, rng_indel, codes, off[c], fwd, rev, fp, frag, pr)
        for m in (fwd, rev):
            hit = rng.random(m.shape) < a.sub_rate
            m += (hit * rng.integers(1, 4, m.shape, dtype=np.uint8)).astype(np.uint8)
            m &= 3
        flip = (np.arange(lo, lo + k) & 1).astype(bool)    # odd pairs: mate 1 is the reverse mate
        first = np.where(flip[:, None], rev, fwd)
        second = np.where(flip[:, None], fwd, rev)
        m1[lo * L:(lo + k) * L] = ASCII[first].reshape(-1)
        m2[lo * L:(lo + k) * L] = ASCII[second].reshape(-1)
        truth[lo:lo + k] = np.stack([c, np.where(flip, pr, pf), np.where(flip, pf, pr), flip], axis=1)
    return m1, m2, np.arange(n + 1, dtype=np.int64) * L, truth


def step_index(a):
    from waafle_amd import mapper
    codes, off = make_contigs(a)
    seq = ASCII[codes]
    times = []
    with mapper.Mapper(seq[:off[1]], off[:2], device=a.gpu) as m:      # context and code objects warm
        for _ in range(3):
            t0 = time.perf_counter()
            m.index(seq, off)                                          # returns after the device is done
            times.append(time.perf_counter() - t0)
    return dict(index_build_s=min(times), index_build_s_all=times, bases=int(off[-1]))


def step_map(a):
    from waafle_amd import mapper
    codes, off = make_contigs(a)
    m1, m2, roff, truth = make_pairs(a, codes, off)
    L, n = a.read_length, a.pairs
    parts = []
    with mapper.Mapper(ASCII[codes], off, max_insert=max(500, a.insert[1]), device=a.gpu,
                       max_gap=a.max_gap) as m:
        w = min(a.chunk, n)
        m.map(m1[:w * L], roff[:w + 1], m2[:w * L], roff[:w + 1])      # warm-up chunk
        t0 = time.perf_counter()
        for lo in range(0, n, a.chunk):
            hi = min(lo + a.chunk, n)
            parts.append(m.map(m1[lo * L:hi * L], roff[lo:hi + 1] - roff[lo], m2[lo * L:hi * L],
                               roff[lo:hi + 1] - roff[lo]))
        dt = time.perf_counter() - t0
    res = {f: np.concatenate([p[f] for p in parts]) for f in parts[0]}
    right = (res["contig"] == truth[:, 0]) & (res["pos1"] == truth[:, 1]) & (res["pos2"] == truth[:, 2]) & \
        (res["strand1"] == truth[:, 3])
    ungapped = (res["contig"] >= 0) & (res["flags"] == 0)
    return dict(map_s=dt, pairs_per_s=n / dt, aligned_fraction=float(np.mean(res["contig"] >= 0)),
                at_origin_fraction=float(np.mean(right)), chunk=a.chunk, max_gap=a.max_gap,
                gapped_pass_receives_fraction=float(1.0 - np.mean(ungapped)) if a.max_gap else 0.0,
                gapped_pass_aligns_fraction=float(np.mean(res["flags"] == 1)),
                gapped_pass_overflow_fraction=float(np.mean(res["flags"] == 2)),
                timing="host-resident reads: copies in and out included, one warm-up chunk")


def main(argv=None):
    a = parse(argv)
    if a.step:
        print("MAP_BENCH_STEP " + json.dumps({"index": step_index, "map": step_map}[a.step](a)))
        return 0
    out = dict(workload=dict(contigs=a.contigs, contig_length=a.contig_length, pairs=a.pairs,
                             read_length=a.read_length, sub_rate=a.sub_rate, indel_rate=a.indel_rate,
                             indel_max=a.indel_max, max_gap=a.max_gap, insert=list(a.insert),
                             seed=a.seed, params=dict(seed_length=20, max_seed_hits=16, max_mismatches=4)))
    passed = [x for x in (argv if argv is not None else sys.argv[1:])]
    for step in ("index", "map"):
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + passed
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout, cwd=REPO)
        except subprocess.TimeoutExpired:
            print("step {} ran out of time ({} s); stopping".format(step, a.step_timeout), file=sys.stderr)
            return 2
        line = [l for l in r.stdout.splitlines() if l.startswith("MAP_BENCH_STEP ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stderr[-4000:])
            print("step {} failed (exit {}); stopping".format(step, r.returncode), file=sys.stderr)
            return 1
        out.update(json.loads(line[-1][len("MAP_BENCH_STEP "):]))
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
