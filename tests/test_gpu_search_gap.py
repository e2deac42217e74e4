"""wf_search_gapped (wf_search_gap.hip) on the GPU against the two CPU forms of the gapped rule
(tests/search_gap_oracle.py): every field of every record must be equal.  The hand-built cases
against both forms and their stated record counts, a seeded medium set against the array form
(whole, in chunks of 7 and of 1, twice, and after an index replacement), wf_search around a
gapped call, the capacity protocol, the parameter checks, and `python -m waafle_amd.search
--searcher native --gapped` followed by `waafle_amd.orgscorer`."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import search_cases as sc
import search_gap_cases as gc
import search_gap_oracle as go
import search_oracle as so
from oracle_bridge import oracle_results, run_oracle
from waafle_amd import inputs, lib, output, search

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [f for f, _ in search.GAP_RECORD_FIELDS]
UNGAPPED = [f for f, _ in search.RECORD_FIELDS]


def kw(P):
    return dict(seed_length=P["S"], seed_stride=P["T"], max_seed_hits=P["max_occ"], xdrop=P["X"],
                min_score=P["min_score"], band=P["W"], xdrop_gap=P["Xg"])


def records(out, fields=FIELDS):
    return sorted(zip(*[out[f].tolist() for f in fields]))


def run_chunks(s, subjects, size):
    got = []
    for lo in range(0, len(subjects), size):
        out = s.search_gapped(*sc.flat(subjects[lo:lo + size]))
        out["subject"] = out["subject"] + np.int32(lo)
        got += records(out)
    return sorted(got)


def test_fields_are_the_oracles():
    assert tuple(FIELDS) == go.FIELDS


@pytest.mark.parametrize("name", sorted(gc.HAND_BUILT))
def test_hand_built_cases_equal_both_oracles(name):
    contigs, subjects, P, n = gc.HAND_BUILT[name]()
    want = go.search_gapped_cells(contigs, subjects, P)
    assert want == go.search_gapped_arrays(contigs, subjects, P)
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        out = s.search_gapped(*sc.flat(subjects))
        assert s.stats["anchors"] == len(so.search_indexed(contigs, subjects, P))
    got = list(zip(*[out[f].tolist() for f in FIELDS]))
    key = [(r[0], r[1], r[2], r[3], r[5], r[4], r[6], r[7], r[8], r[9]) for r in got]
    assert key == sorted(key), "the records come back in the defined order"
    assert sorted(got) == want
    assert len(got) == n
    for f, dt in search.GAP_RECORD_FIELDS:
        assert out[f].dtype == dt


def test_planted_homolog_is_one_record():
    contigs, subjects, P = gc.planted()
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        got = records(s.search_gapped(*sc.flat(subjects)))
        ungapped = s.search(*sc.flat(subjects))
    assert got == [(0, 0, 0, 500, 1000, 0, 1000, 1003, 971, 6), (0, 1, 1, 500, 1000, 0, 1000, 1003, 971, 6)]
    assert len(ungapped["length"]) == 8 and (ungapped["length"] / 1000.0 < 0.3).all()


@pytest.fixture(scope="module")
def medium():
    contigs, subjects, P = gc.medium()
    return contigs, subjects, P, go.search_gapped_arrays(contigs, subjects, P)


def test_medium_set_five_ways(medium):
    contigs, subjects, P, want = medium
    assert len(contigs) == 40 and len(subjects) == 200
    assert len(want) > 150 and sum(1 for r in want if r[9] > 0) > 50
    ungapped = so.search_indexed(contigs, subjects, P)
    other = [sc.rnd(500, 99)]
    with search.Searcher(*sc.flat(other), **kw(P)) as s:
        assert run_chunks(s, subjects[:20], 20) == go.search_gapped_arrays(other, subjects[:20], P)
        s.index(*sc.flat(contigs))                           # the index is replaced
        s.stats = dict.fromkeys(s.stats, 0)
        assert run_chunks(s, subjects, len(subjects)) == want
        assert s.stats["anchors"] == len(ungapped)
        assert 0 < s.stats["raw_alignments"] <= s.stats["anchors"]
        assert run_chunks(s, subjects, 7) == want
        assert run_chunks(s, subjects, 1) == want
        assert run_chunks(s, subjects, len(subjects)) == want   # twice over
        assert s.stats["anchors"] == 4 * len(ungapped)


def test_ungapped_search_untouched_by_a_gapped_call(medium):
    contigs, subjects, P, _ = medium
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        before = s.search(*sc.flat(subjects[:60]))
        assert len(s.search_gapped(*sc.flat(subjects[30:90]))["contig"]) > 0
        after = s.search(*sc.flat(subjects[:60]))
    assert len(before["contig"]) > 20
    for f in UNGAPPED:
        np.testing.assert_array_equal(before[f], after[f])


def test_capacity_one_then_room():
    contigs, subjects, P, n = gc.refill_gaps()
    want = go.search_gapped_cells(contigs, subjects, P)
    assert len(want) == n >= 3
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        rc, full, out = s.search_gapped_once(*sc.flat(subjects), 1)
        assert rc == lib.WF_E_NOMEM and full == n
        assert records(out) == want[:1]
        rc, full, out = s.search_gapped_once(*sc.flat(subjects), n)
        assert rc == lib.WF_OK and full == n and records(out) == want
        s.capacity = 1                                       # the wrapper grows on its own
        assert records(s.search_gapped(*sc.flat(subjects))) == want


def test_parameter_checks():
    contigs, subjects, P, _ = gc.minus_strand()
    seq, off = sc.flat(subjects)
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        for field, value in (("band", 0), ("band", 32), ("xdrop_gap", 0), ("xdrop_gap", 1001)):
            gp = lib.WfSearchGapParams.from_buffer_copy(s.gap_params)
            setattr(gp, field, value)
            with pytest.raises(lib.WaafleHipError) as exc:
                s.search_gapped(seq, off, gap_params=gp)
            assert exc.value.code == lib.WF_E_BADINPUT, (field, value)
        p = lib.WfSearchParams.from_buffer_copy(s.params)
        p.stride = 0
        with pytest.raises(lib.WaafleHipError) as exc:
            s.search_gapped(seq, off, params=p)
        assert exc.value.code == lib.WF_E_BADINPUT
        big = np.array([0, (1 << 30) + 1], np.int64)         # refused before it is read
        with pytest.raises(lib.WaafleHipError) as exc:
            s.search_gapped(seq, big)
        assert exc.value.code == lib.WF_E_TOOBIG
        assert len(s.search_gapped(seq, off)["contig"]) == 1   # still usable


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------

def _sample(tmp_path):
    """Three contigs of two genes each; the genes of species A as they are, those of species B
    with 3 % substitutions and two short indels each, one gene reverse-complemented; taxonomy
    and GFF to match."""
    rng = random.Random(4)
    contigs, subjects, gff = [], [], []
    for c in range(3):
        seq = sc.rnd(1500, 300 + c)
        contigs.append(("ctg{}".format(c), seq))
        for k, (a, b) in enumerate(((100, 600), (800, 1300))):
            gene = seq[a:b]
            other = "".join(ch if rng.random() > 0.03 else rng.choice("ACGT") for ch in gene)
            other = other[:150] + other[150 + rng.randint(1, 3):]
            other = other[:330] + sc.rnd(rng.randint(1, 3), 50 + 2 * c + k) + other[330:]
            if c == 1 and k == 1:
                gene = so.revcomp(gene)
            subjects.append(("g{}{}a|s__A|UniProt=U{}{}".format(c, k, c, k), gene))
            subjects.append(("g{}{}b|s__B|UniProt=U{}{}".format(c, k, c, k), other))
            gff.append("\t".join(["ctg{}".format(c), "x", "gene", str(a + 1), str(b), ".", "+", "0", "."]))
    paths = [str(tmp_path / n) for n in ("s.fna", "s.blastout", "s.gff", "s.tsv", "genes.fna")]
    with open(paths[0], "w") as fh:
        fh.write("".join(">{} sample\n{}\n".format(n, "\n".join(s[i:i + 70] for i in range(0, len(s), 70)))
                         for n, s in contigs))
    with open(paths[4], "w") as fh:
        fh.write("".join(">{} some words\n{}\n".format(n, "\n".join(s[i:i + 60] for i in range(0, len(s), 60)))
                         for n, s in subjects))
    with open(paths[2], "w") as fh:
        fh.write("\n".join(gff) + "\n")
    with open(paths[3], "w") as fh:
        fh.write("s__A\tg__G\ns__B\tg__G\ng__G\tr__Root\n")
    return contigs, subjects, paths


def _table(contigs, subjects, recs, rows):
    return "".join(r + "\n" for r in rows(
        recs, [n for n, _ in contigs], [len(s) for _, s in contigs], [n for n, _ in subjects],
        [len(s) for _, s in subjects], sum(len(s) for _, s in subjects)))


def test_gapped_search_then_orgscorer(tmp_path):
    contigs, subjects, paths = _sample(tmp_path)
    cs, ss = [s for _, s in contigs], [s for _, s in subjects]
    command = [sys.executable, "-m", "waafle_amd.search", paths[0], paths[4], "--searcher", "native", "--out",
               paths[1], "--chunk-bases", "1200"]
    run = subprocess.run(command, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert run.returncode == 0, run.stderr[-2000:]
    ungapped = so.search_indexed(cs, ss, so.DEFAULTS)
    assert open(paths[1]).read() == _table(contigs, subjects, ungapped, so.rows)
    run = subprocess.run(command + ["--gapped"], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert run.returncode == 0, run.stderr[-2000:]
    table = open(paths[1]).read()
    recs = go.search_gapped_cells(cs, ss, go.GAP_DEFAULTS)
    assert len(recs) == 12 < len(ungapped) and sum(1 for r in recs if r[9] > 0) == 6
    assert table == _table(contigs, subjects, recs, go.rows)
    batch, tax = inputs.load_inputs(*paths[:4], 200.0, warn=None)
    assert batch.n_hits == len(recs)
    run = subprocess.run([sys.executable, "-m", "waafle_amd.orgscorer"] + paths[:4] +
                         ["--outdir", str(tmp_path), "--basename", "s", "--quiet"], capture_output=True,
                         text=True, timeout=300, cwd=REPO)
    assert run.returncode == 0, run.stderr[-2000:]
    models, _ = run_oracle(paths[:4], [])
    rows = output.render(batch, tax, oracle_results(models, batch, tax))
    for kind in ("lgt", "no_lgt", "unclassified"):
        assert open(str(tmp_path / "s.{}.tsv".format(kind))).read() == "\n".join(rows[kind]) + "\n", kind
    assert len(rows["no_lgt"]) + len(rows["lgt"]) >= 1
