"""GPU: wf_junctions through the C-ABI on the cases of junction_cases.py, against the oracle
(junction_cases.judge: oracle.junctions_oracle on the same case rendered as text).  Exact:
per-site coverage, junction and locus hit counts, the four float64 values of every junction
bit for bit (NaN matching NaN), and the gene-pair hit rows."""
import gzip

import numpy as np
import pytest

import junction_cases as jc
from waafle_amd import junctions

pytestmark = pytest.mark.gpu

FIELDS = ("coverage_gene1", "coverage_gene2", "coverage_junction", "ratio")


def bits(a):
    """float64 bit patterns, every NaN as one pattern."""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), np.int64(-1), a.view(np.int64))


@pytest.mark.parametrize("case", jc.all_cases(), ids=repr)
def test_case_matches_oracle(case):
    table, pairs, want = case.table(), case.pair_arrays(), jc.judge(case.name)
    res = junctions.score_junctions(table, pairs, case.min_sites, coverage=True, locus_hits=True,
                                    pair_sets=True)
    bad = np.nonzero(res["coverage"] != want.coverage)[0]
    assert len(bad) == 0, ("coverage", bad[:5], res["coverage"][bad[:5]], want.coverage[bad[:5]])
    j = want.is_junction
    for f, field in enumerate(FIELDS):
        bad = np.nonzero(bits(res[field][j]) != bits(want.floats[f][j]))[0]
        assert len(bad) == 0, (field, bad[:5], res[field][j][bad[:5]], want.floats[f][j][bad[:5]])
    assert np.array_equal(res["junction_hits"][j], want.junction_hits[j])
    assert np.array_equal(res["locus_hits"], want.locus_hits)
    assert junctions.gene_hit_rows(table, pairs, res) == want.gene_rows
    assert junctions.junction_rows(table, res) == want.junction_rows


def test_cli_detailed_output_on_a_70_locus_contig(tmp_path):
    """--write-detailed-output --min-overlap-sites 0 with more loci than pair_mask has bits:
    the three files are written and equal the oracle's text."""
    contigs, pairs = jc.wide_contigs([70])
    case = jc.JCase("cli70", contigs, pairs, 0)
    fna, gff, sam = case.write_text(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    junctions.main([fna, gff, "--sam", sam, "--outdir", str(out), "--basename", "case",
                    "--write-detailed-output", "--min-overlap-sites", "0"])
    from oracle import junctions_oracle as jo
    site, gene = jo.detailed_rows(fna, gff, sam, 0)
    text = lambda rows: "\n".join(rows) + "\n"
    assert (out / "case.junctions.tsv").read_text() == text(jo.junction_rows(fna, gff, sam, 0))
    assert (out / "case.gene_hits.tsv").read_text() == text(gene)
    with gzip.open(str(out / "case.site_hits.tsv.gz"), "rt") as fh:
        assert fh.read() == text(site)
    assert len(gene) == 1 + 70 * 71 // 2
