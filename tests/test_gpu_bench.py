"""bench.py as it is run for every change: a plain `--gpus 1 --steps K --warmup W` run carries
the main line alone (the other legs need --full), and --dump-outputs writes the records of
the last timed pass, which must be the records the scorer gives for the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 3000


def test_bench_plain_run_and_dumped_records(tmp_path):
    from waafle_amd import cli, engine, synth
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--contigs", str(N), "--dump-outputs", str(out)]
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "contigs/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert abs(d["value"] - N / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert d["calls"]["lgt"] + d["calls"]["no_lgt"] + d["calls"]["unclassified"] == N
    # the legs of --full are not run
    for key in ("weak", "strong_share_projection", "ops_roofline", "cpu_baseline", "k2_pair_evals_per_sec"):
        assert d[key] is None, key
    for key in ("k2", "pcie_inclusive", "cli_end_to_end"):
        assert key not in d, key
    assert "skipped" in d["roofline"]["valu"] and "skipped" in d["roofline"]["traffic_detail"]

    # the dumped records: the same seeded batch through the scorer
    batch, tax = synth.generate_batch("cfg4", 0, N, workers=1, n_total=N)
    res = engine.score(batch, tax, cli.param_dict(cli.parse_flags([])), gpus=1)
    z = {os.path.splitext(f)[0]: np.load(str(out / f)) for f in os.listdir(str(out))}
    assert all(a.dtype in (np.float32, np.float64) for a in z.values())
    assert sum(a.nbytes for a in z.values()) <= 64 << 20
    assert np.array_equal(z["contig"], np.arange(N))
    for f in ("call", "crit", "rank", "clade1", "clade2", "direction", "iterations", "n_meld1", "n_meld2",
              "pair_evals", "status", "need_bytes", "synteny", "annot_hit"):
        assert np.array_equal(z[f], getattr(res, f).astype(z[f].dtype), equal_nan=True), f
    assert np.array_equal(z["loc_off"], batch.loc_off)
    meld = [res.meld[2 * int(batch.hit_off[c]) + 2 * c:][:int(res.n_meld1[c]) + int(res.n_meld2[c])]
            for c in range(N)]
    assert np.array_equal(z["meld"], np.concatenate(meld))
    assert (res.call == 2).sum() > 0 and (res.call == 1).sum() > 0
