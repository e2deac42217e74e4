"""Wall of the table's order and --max-target-seqs: the host form against the device form, on one
MI355X.

    python scripts/order_bench.py [--sizes 100000,1000000,10000000 --per-contig 210 --families 2000
                                   --family-size 64 --max-target-seqs 10000 --runs 3 --gapped
                                   --device-only --host-budget 240]

Not bench.py (the flagship workload); the numbers go to DESIGN.md §13.6 and profiles/order/.
The records are synthetic, seeded, shaped like the scorer's benchmark configuration cfg4: about
--per-contig records per contig; a contig draws a few gene families and its records' subjects
from those families' members (--family-size each), with identities that depend on the family
alone, so that many (contig, subject) pairs tie on their best score; a record's length and
matches take few values.  The input is in the order a search gives: by subject chunk, then contig.

Timed per size, in one process, interleaved, after one warm-up each, --runs times:

  host     search.order_records + hits.record_columns (numpy; unchanged by the device form)
  device   search.order_records_device with gathering: wf_order_records, the host pass that
           checks the records and plans the key, uploads, kernels and downloads included

The two must give the same order and columns.  A size whose host warm-up takes longer than
--host-budget seconds is not repeated on the host (its one wall is reported).  --device-only:
the device path alone, for a run under rocprofv3 --kernel-trace --stats.  One JSON line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from waafle_amd import hits, lib, search   # noqa: E402


def records(n, per_contig, families, family_size, gapped, seed):
    rng = np.random.RandomState(seed)
    n_contigs = max(1, n // per_contig)
    contig = rng.randint(0, n_contigs, n)
    fam_of_contig = rng.randint(0, families, (n_contigs, 4))
    fam = fam_of_contig[contig, rng.randint(0, 4, n)]
    subject = fam * family_size + rng.randint(0, family_size, n)
    length = 300 + 100 * (fam % 8)
    matches = length - (fam % 5) * 7 - 7 * rng.randint(0, 2, n)
    rec = dict(contig=contig, subject=subject, minus=rng.randint(0, 2, n), qstart=rng.randint(0, 5000, n),
               sstart=rng.randint(0, 200, n), length=length, matches=matches)
    if gapped:
        rec.update(qspan=length - rng.randint(0, 3, n), sspan=length - rng.randint(0, 3, n), gaps=rng.randint(0, 3, n))
    fields = search.GAP_RECORD_FIELDS if gapped else search.RECORD_FIELDS
    rec = {f: rec[f].astype(dt) for f, dt in fields}
    o = np.lexsort((rec["contig"], rec["subject"] // (family_size * 50)))     # chunk by chunk, by contig within
    return {f: a[o] for f, a in rec.items()}


class Ctx:
    def __init__(self, device):
        self.so, self.h = lib.load(), C.c_void_p()
        rc = self.so.wf_init(device, C.byref(self.h))
        if rc != lib.WF_OK:
            raise SystemExit("wf_init failed: no GPU, no measurement")


def host_form(rec, limit):
    order = search.order_records(rec, limit)
    return order, hits.record_columns(rec, order)


def wall(fn):
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--sizes", default="100000,1000000,10000000")
    ap.add_argument("--per-contig", type=int, default=210)
    ap.add_argument("--families", type=int, default=2000)
    ap.add_argument("--family-size", type=int, default=64)
    ap.add_argument("--max-target-seqs", type=int, default=search.MAX_TARGET_SEQS)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--gapped", action="store_true")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--host-budget", type=float, default=240.0)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args(argv)
    ctx = Ctx(args.gpu)
    limit = args.max_target_seqs
    result = dict(per_contig=args.per_contig, families=args.families, family_size=args.family_size,
                  max_target_seqs=limit, gapped=bool(args.gapped), runs=args.runs, sizes=[])
    for n in [int(s) for s in args.sizes.split(",")]:
        rec = records(n, args.per_contig, args.families, args.family_size, args.gapped, args.seed)
        device = lambda: search.order_records_device(ctx, rec, limit, gather=True)
        row = dict(n=n, host_s=[], device_s=[])
        w, (d_order, d_cols) = wall(device)                   # warm-up (the first call also allocates)
        row.update(device_warmup_s=w, kept=int(len(d_order)))
        print("n {:>11,}: device warm-up {:.3f} s".format(n, w), file=sys.stderr, flush=True)
        host_runs = 0
        if not args.device_only:
            w, (h_order, h_cols) = wall(lambda: host_form(rec, limit))
            row["host_warmup_s"] = w
            row["same"] = bool(np.array_equal(h_order, d_order) and
                               all(np.array_equal(h_cols[f], d_cols[f]) for f in h_cols))
            host_runs = args.runs if w <= args.host_budget else 0
        for k in range(args.runs):
            if k < host_runs:
                row["host_s"].append(wall(lambda: host_form(rec, limit))[0])
            row["device_s"].append(wall(device)[0])
        row["device_median_s"] = statistics.median(row["device_s"])
        if row["host_s"]:
            row["host_median_s"] = statistics.median(row["host_s"])
            row["host_over_device"] = row["host_median_s"] / row["device_median_s"]
        result["sizes"].append(row)
        print("n {:>11,}: {}".format(n, {k: v for k, v in row.items() if k.endswith("median_s") or k in ("same", "kept")}),
              file=sys.stderr, flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
