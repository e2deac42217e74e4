"""End-to-end wall of the one-command workflow against the three commands it stands for, on one
MI355X.

    python scripts/workflow_bench.py [--contigs 2000 --contig-length 5000 --db-bases 20000000
                                      --subject-length 1000 --homolog-share 0.2 --species 8 --runs 3
                                      --gapped --workdir DIR]

Not bench.py (the flagship workload); the numbers go to DESIGN.md §13 and profiles/workflow/.
The workload is that of scripts/search_bench.py (seeded random contigs; a database of random
subjects of which a share is cut from the contigs, either strand, 90..100 % identity) with a
taxonomy: --species species in two genera; a planted gene carries the species of its contig
(contig number modulo --species) four times in five and a random one otherwise, the other
subjects a random one, so that the scorer has single-clade contigs and candidate pairs to decide.
The database is written as FASTA and formatted once with makedb (outside the timing).

Timed, each as its own process, --runs times, interleaved:

  three   python -m waafle_amd.search --searcher native, then waafle_amd.genecaller, then
          waafle_amd.orgscorer: the wall of each command and their sum
  one     python -m waafle_amd.workflow: its wall, and its own phase split

Both on the same commit (the three commands are the parent's code).  The TSVs of the two must be
equal.  Every child runs under --step-timeout; after a failure nothing more is started.  With
--workdir the files stay there (for a run of the workflow under rocprofv3 --kernel-trace --stats).
Prints one JSON line.
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)

import search_bench as sb   # noqa: E402  (the workload generator)

KINDS = ("lgt", "no_lgt", "unclassified")


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("--contigs", type=int, default=2000)
    ap.add_argument("--contig-length", type=int, default=5000)
    ap.add_argument("--db-bases", type=int, default=20000000)
    ap.add_argument("--subject-length", type=int, default=1000)
    ap.add_argument("--homolog-share", type=float, default=0.2)
    ap.add_argument("--species", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--gapped", action="store_true")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--workdir", default=None, help="generate the files here and keep them")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds for each child process")
    return ap.parse_args(argv)


def write_workload(a, d):
    """contigs.fna, genes.fna, genes.wfdb and taxonomy.tsv under d; returns their paths and counts"""
    from waafle_amd import makedb
    gen = argparse.Namespace(contigs=a.contigs, contig_length=a.contig_length, db_bases=a.db_bases,
                             subject_length=a.subject_length, homolog_share=a.homolog_share, indel_rate=0.0,
                             low_complexity=0, seed=a.seed)
    codes, off, subj, hom = sb.make_workload(gen)
    # make_workload draws the homologs' contigs right after the subjects: the same stream again
    rng = np.random.default_rng(a.seed)
    rng.integers(0, 4, a.contigs * a.contig_length, dtype=np.uint8)
    n = a.db_bases // a.subject_length
    rng.integers(0, 4, (n, a.subject_length), dtype=np.uint8)
    assert np.array_equal(np.flatnonzero(rng.random(n) < a.homolog_share), hom)
    contig_of = rng.integers(0, a.contigs, len(hom))
    rng2 = np.random.default_rng(a.seed + 7)
    species = rng2.integers(0, a.species, n)
    own = rng2.random(len(hom)) < 0.8
    species[hom[own]] = contig_of[own] % a.species
    paths = {k: os.path.join(d, f) for k, f in (("contigs", "contigs.fna"), ("fasta", "genes.fna"),
                                                ("wfdb", "genes.wfdb"), ("taxonomy", "taxonomy.tsv"))}

    def write_fasta(path, rows, name):
        with open(path, "wb") as fh:
            for i, row in enumerate(rows):
                text = sb.ASCII[row].tobytes()
                fh.write(name(i) + b"\n".join(text[k:k + 60] for k in range(0, len(text), 60)) + b"\n")

    write_fasta(paths["contigs"], (codes[off[c]:off[c + 1]] for c in range(a.contigs)), lambda i: b">ctg%d\n" % i)
    write_fasta(paths["fasta"], subj, lambda i: b">g%d|s__S%d|UniProt=U%d\n" % (i, species[i], i))
    with open(paths["taxonomy"], "w") as fh:
        for k in range(a.species):
            fh.write("s__S{}\tg__G{}\n".format(k, k % 2))
        fh.write("g__G0\tf__F\ng__G1\tf__F\nf__F\tr__Root\n")
    makedb.make_db(paths["fasta"], paths["wfdb"])
    return paths, dict(subjects=n, homologs=int(len(hom)))


def child(cmd, timeout):
    """(wall seconds, stderr) of one command; raises when it fails or runs out of time"""
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-m"] + cmd, capture_output=True, text=True, timeout=timeout, cwd=REPO)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("{} failed (exit {}): {}".format(cmd[0], r.returncode, r.stderr[-1500:]))
    return wall, r.stderr


def tsvs(d, base):
    return {k: open(os.path.join(d, "{}.{}.tsv".format(base, k))).read() for k in KINDS}


def main(argv=None):
    a = parse(argv)
    d = a.workdir or tempfile.mkdtemp(prefix="workflow_bench_")
    os.makedirs(d, exist_ok=True)
    out = dict(workload=dict(contigs=a.contigs, contig_length=a.contig_length, db_bases=a.db_bases,
                             subject_length=a.subject_length, homolog_share=a.homolog_share, species=a.species,
                             identity="90..100 %", seed=a.seed, gapped=a.gapped, database="wfdb"), runs=[])
    try:
        paths, counts = write_workload(a, d)
        out["workload"].update(counts)
        mode = ["--gapped"] if a.gapped else []
        table, gff = os.path.join(d, "three.blastout"), os.path.join(d, "three.gff")
        for _ in range(a.runs):
            run = {}
            run["search_s"], err = child(["waafle_amd.search", paths["contigs"], paths["wfdb"], "--searcher", "native",
                                          "--out", table] + mode, a.step_timeout)
            out["records"] = int(re.search(r"\(([\d,]+) rows", err).group(1).replace(",", ""))
            run["genecaller_s"], _ = child(["waafle_amd.genecaller", table, "--gff", gff], a.step_timeout)
            run["orgscorer_s"], err = child(["waafle_amd.orgscorer", paths["contigs"], table, gff, paths["taxonomy"],
                                             "--outdir", d, "--basename", "three"], a.step_timeout)
            run["orgscorer_phases"] = [l for l in err.splitlines() if l.startswith("Finished")][-1]
            run["three_s"] = run["search_s"] + run["genecaller_s"] + run["orgscorer_s"]
            run["workflow_s"], err = child(["waafle_amd.workflow", paths["contigs"], paths["wfdb"], paths["taxonomy"],
                                            "--outdir", d, "--basename", "one"] + mode, a.step_timeout)
            run["workflow_phases"] = [l for l in err.splitlines() if l.startswith("Finished")][-1]
            run["tsvs_equal"] = tsvs(d, "three") == tsvs(d, "one")
            out["runs"].append(run)
        out["table_bytes"] = os.path.getsize(table)
        out["tsv_rows"] = {k: v.count("\n") - 1 for k, v in tsvs(d, "one").items()}
        for k in ("search_s", "genecaller_s", "orgscorer_s", "three_s", "workflow_s"):
            out["median_" + k] = float(np.median([r[k] for r in out["runs"]]))
    except (RuntimeError, subprocess.TimeoutExpired) as exc:
        print("a step failed; stopping: {}".format(exc), file=sys.stderr)
        print(json.dumps(out))
        return 1
    finally:
        if not a.workdir:
            shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
