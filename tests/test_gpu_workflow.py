"""`python -m waafle_amd.workflow` against the three commands it stands for, run one after another
(waafle_amd.search --searcher native, waafle_amd.genecaller, waafle_amd.orgscorer): the three
TSVs, and the optional table and gene calls, must be the same bytes.  On the sample of
tests/test_gpu_search.py, the database as FASTA and as .wfdb, plain, --gapped and --dust."""
import os
import subprocess
import sys

import pytest

import search_cases as sc
from oracle_bridge import oracle_results, run_oracle
from test_gpu_search import _sample
from waafle_amd import genecaller, inputs, makedb, orgscorer, output, search, workflow

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("lgt", "no_lgt", "unclassified")
MODES = {"plain": [], "gapped": ["--gapped"], "dust": ["--dust"]}


def tsvs(outdir, base):
    return {k: open(os.path.join(str(outdir), "{}.{}.tsv".format(base, k))).read() for k in KINDS}


def three_commands(paths, db, mode, outdir, gff=None):
    """search -> genecaller -> orgscorer through their mains; returns (TSVs, table, gene calls)"""
    table, calls = os.path.join(str(outdir), "t.blastout"), os.path.join(str(outdir), "t.gff")
    search.main([paths[0], db, "--searcher", "native", "--out", table, "--chunk-bases", "1200"] + MODES[mode])
    genecaller.main([table, "--gff", calls])
    orgscorer.main([paths[0], table, gff or calls, paths[3], "--outdir", str(outdir), "--basename", "t", "--quiet"])
    return tsvs(outdir, "t"), open(table).read(), open(calls).read()


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("workflow")
    contigs, subjects, paths = _sample(tmp)
    wfdb = str(tmp / "genes.wfdb")
    makedb.main([paths[4], "--out", wfdb])
    return tmp, contigs, subjects, paths, {"fasta": paths[4], "wfdb": wfdb}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("form", ["fasta", "wfdb"])
def test_workflow_equals_the_three_commands(sample, tmp_path, form, mode):
    tmp, contigs, subjects, paths, dbs = sample
    want, table, calls = three_commands(paths, dbs[form], mode, tmp_path)
    assert table.count("\n") >= 12 and calls.count("\n") >= 6
    out_table, out_calls = str(tmp_path / "w.blastout"), str(tmp_path / "w.gff")
    workflow.main([paths[0], dbs[form], paths[3], "--outdir", str(tmp_path), "--basename", "w", "--quiet",
                   "--chunk-bases", "1200", "--write-blastout", out_table, "--write-gff", out_calls] + MODES[mode])
    assert tsvs(tmp_path, "w") == want
    assert sum(t.count("\n") - 1 for t in want.values()) == 3
    assert open(out_table).read() == table
    assert open(out_calls).read() == calls


def test_workflow_with_user_gene_calls(sample, tmp_path):
    tmp, contigs, subjects, paths, dbs = sample
    want, table, _ = three_commands(paths, dbs["fasta"], "plain", tmp_path, gff=paths[2])
    workflow.main([paths[0], dbs["wfdb"], paths[3], "--gff", paths[2], "--outdir", str(tmp_path), "--basename", "w",
                   "--quiet"])
    got = tsvs(tmp_path, "w")
    assert got == want
    four = [paths[0], str(tmp_path / "t.blastout"), paths[2], paths[3]]
    batch, tax = inputs.load_inputs(*four, 200.0, warn=None)
    models, _ = run_oracle(four, [])
    rows = output.render(batch, tax, oracle_results(models, batch, tax))
    for kind in KINDS:
        assert got[kind] == "\n".join(rows[kind]) + "\n", kind
    assert len(rows["no_lgt"]) + len(rows["lgt"]) >= 3


def run_workflow(argv):
    return subprocess.run([sys.executable, "-m", "waafle_amd.workflow"] + argv, capture_output=True, text=True,
                          timeout=300, cwd=REPO)


def test_database_without_a_hit(sample, tmp_path):
    tmp, contigs, subjects, paths, dbs = sample
    db = str(tmp_path / "far.fna")
    with open(db, "w") as fh:
        fh.write("".join(">far{}|s__A|UniProt=F{}\n{}\n".format(k, k, sc.rnd(400, 900 + k)) for k in range(3)))
    run = run_workflow([paths[0], db, paths[3], "--outdir", str(tmp_path), "--basename", "w"])
    assert run.returncode == 0, run.stderr[-2000:]
    assert "Finished successfully" in run.stderr
    got = tsvs(tmp_path, "w")
    want, table, calls = three_commands(paths, db, "plain", tmp_path)
    assert table == "" and calls == ""
    assert got == want
    heads = {k: "\t".join(c.upper() for c in output.FORMATS[k]) + "\n" for k in KINDS}
    assert got["lgt"] == heads["lgt"] and got["no_lgt"] == heads["no_lgt"]
    # a contig without a hit is still a row of the unclassified file, as the scorer lists it
    assert got["unclassified"].startswith(heads["unclassified"]) and got["unclassified"].count("\n") == 1 + len(contigs)


def test_bad_subject_id_is_the_scorers_lethal_error(sample, tmp_path):
    tmp, contigs, subjects, paths, dbs = sample
    db = str(tmp_path / "bad.fna")
    with open(db, "w") as fh:
        fh.write("".join(">{}\n{}\n".format(n if k else "g00a|s__A|UniProt", s) for k, (n, s) in enumerate(subjects)))
    run = run_workflow([paths[0], db, paths[3], "--outdir", str(tmp_path), "--basename", "w"])
    assert run.returncode != 0 and run.stderr.rstrip().endswith("EXITING.")
    lethal = [l for l in run.stderr.splitlines() if l.startswith("LETHAL ERROR:")]
    table = str(tmp_path / "t.blastout")
    search.main([paths[0], db, "--searcher", "native", "--out", table])
    ref = subprocess.run([sys.executable, "-m", "waafle_amd.orgscorer", paths[0], table, paths[2], paths[3],
                          "--outdir", str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert ref.returncode != 0
    assert lethal and lethal == [l for l in ref.stderr.splitlines() if l.startswith("LETHAL ERROR:")]
    assert "bad annotation 'UniProt'" in lethal[0]
    assert not os.path.exists(str(tmp_path / "w.lgt.tsv"))
