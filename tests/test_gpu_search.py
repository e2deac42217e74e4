"""wf_search (wf_search.hip) on the GPU against the CPU oracles of the search rule
(tests/search_oracle.py): every field of every record must be equal.  The hand-built cases
against both oracles and their stated record counts, a seeded medium set against the
dictionary oracle (whole, in chunks of 7 and of 1, twice, and after an index replacement),
the capacity protocol, the parameter checks, the mapper on the same context, and
`python -m waafle_amd.search --searcher native` followed by `waafle_amd.orgscorer`."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import map_cases as mc
import search_cases as sc
import search_oracle as so
from oracle_bridge import oracle_results, run_oracle
from waafle_amd import inputs, lib, mapper, output, search

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [f for f, _ in search.RECORD_FIELDS]


def kw(P):
    return dict(seed_length=P["S"], seed_stride=P["T"], max_seed_hits=P["max_occ"], xdrop=P["X"],
                min_score=P["min_score"])


def records(out):
    return sorted(zip(*[out[f].tolist() for f in FIELDS]))


def run_chunks(s, subjects, size):
    got = []
    for lo in range(0, len(subjects), size):
        out = s.search(*sc.flat(subjects[lo:lo + size]))
        out["subject"] = out["subject"] + np.int32(lo)
        got += records(out)
    return sorted(got)


@pytest.mark.parametrize("name", sorted(sc.HAND_BUILT))
def test_hand_built_cases_equal_both_oracles(name):
    contigs, subjects, P, n = sc.HAND_BUILT[name]()
    want = so.search_brute(contigs, subjects, P)
    assert want == so.search_indexed(contigs, subjects, P)
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        out = s.search(*sc.flat(subjects))
    got = list(zip(*[out[f].tolist() for f in FIELDS]))
    assert got == sorted(got), "the records come back in the defined order"
    assert got == want
    assert len(got) == n
    for f, dt in search.RECORD_FIELDS:
        assert out[f].dtype == dt


@pytest.fixture(scope="module")
def medium():
    contigs, subjects, P = sc.medium()
    return contigs, subjects, P, so.search_indexed(contigs, subjects, P)


def test_medium_set_five_ways(medium):
    contigs, subjects, P, want = medium
    assert len(want) > 200
    other = [sc.rnd(500, 99)]
    with search.Searcher(*sc.flat(other), **kw(P)) as s:
        assert run_chunks(s, subjects[:20], 20) == so.search_indexed(other, subjects[:20], P)
        s.index(*sc.flat(contigs))                           # the index is replaced
        assert run_chunks(s, subjects, len(subjects)) == want
        assert run_chunks(s, subjects, 7) == want
        assert run_chunks(s, subjects, 1) == want
        assert run_chunks(s, subjects, len(subjects)) == want   # twice over
        assert s.stats["seed_hits"] > 0 and s.stats["raw_hsps"] + s.stats["seeds_skipped"] == s.stats["seed_hits"]


def test_capacity_one_then_room():
    contigs, subjects, P, n = sc.run_28_all_phases()
    want = so.search_indexed(contigs, subjects, P)
    assert len(want) == n >= 3
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        rc, full, out = s.search_once(*sc.flat(subjects), 1)
        assert rc == lib.WF_E_NOMEM and full == n
        assert records(out) == want[:1]
        rc, full, out = s.search_once(*sc.flat(subjects), n)
        assert rc == lib.WF_OK and full == n and records(out) == want
        s.capacity = 1                                       # the wrapper grows on its own
        assert records(s.search(*sc.flat(subjects))) == want


def test_parameter_checks():
    contigs, subjects, P, _ = sc.minus_strand()
    seq, off = sc.flat(subjects)
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        for field, value in (("seed_len", 11), ("seed_len", 33), ("seed_len", 20), ("stride", 0), ("stride", 33),
                             ("max_occ", 0), ("max_occ", 1025), ("xdrop", 0), ("xdrop", 1001), ("min_score", 0)):
            p = lib.WfSearchParams.from_buffer_copy(s.params)
            setattr(p, field, value)
            with pytest.raises(lib.WaafleHipError) as exc:
                s.search(seq, off, params=p)
            assert exc.value.code == lib.WF_E_BADINPUT, (field, value)
        big = np.array([0, (1 << 30) + 1], np.int64)         # refused before it is read
        with pytest.raises(lib.WaafleHipError) as exc:
            s.search(seq, big)
        assert exc.value.code == lib.WF_E_TOOBIG
        assert len(s.search(seq, off)["contig"]) == 1        # still usable
    h = C.c_void_p()
    dll = lib.load()
    assert dll.wf_init(0, C.byref(h)) == lib.WF_OK
    try:
        sb = lib.WfSearchSubjects(n_subjects=1, seq=lib.ptr(seq), off=lib.ptr(off))
        out = {f: np.zeros(4, dt) for f, dt in search.RECORD_FIELDS}
        r = lib.WfSearchResult(capacity=4, **{f: lib.ptr(out[f]) for f in FIELDS})
        p = lib.WfSearchParams(seed_len=21, stride=8, max_occ=64, xdrop=20, min_score=28)
        assert dll.wf_search(h, C.byref(sb), C.byref(p), C.byref(r)) == lib.WF_E_STATE
    finally:
        dll.wf_free(h)


def test_mapper_untouched_by_a_search():
    contigs, r1, r2, P, _ = mc.orientation()
    with search.Searcher(*mc.flat(contigs), seed_length=P["S"]) as s:
        m = s.mapper
        params = lib.WfMapParams(seed_len=P["S"], max_occ=16, max_mm=P["max_mm"], min_insert=P["min_insert"],
                                 max_insert=P["max_insert"])
        before = m.map(*mc.flat(r1), *mc.flat(r2), params=params)
        assert (before["contig"] >= 0).any()
        found = s.search(*mc.flat([contigs[0][10:90]]))
        assert len(found["contig"]) >= 1
        after = m.map(*mc.flat(r1), *mc.flat(r2), params=params)
    for f in before:
        np.testing.assert_array_equal(before[f], after[f])


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------

def _sample(tmp_path):
    """Three contigs of two genes each; the genes of species A as they are, those of species B
    with 3 % substitutions, one gene reverse-complemented; taxonomy and GFF to match."""
    import random
    rng = random.Random(4)
    contigs, subjects, gff = [], [], []
    for c in range(3):
        seq = sc.rnd(1500, 300 + c)
        contigs.append(("ctg{}".format(c), seq))
        for k, (a, b) in enumerate(((100, 600), (800, 1300))):
            gene = seq[a:b]
            other = "".join(ch if rng.random() > 0.03 else rng.choice("ACGT") for ch in gene)
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


def test_native_search_then_orgscorer(tmp_path):
    contigs, subjects, paths = _sample(tmp_path)
    run = subprocess.run([sys.executable, "-m", "waafle_amd.search", paths[0], paths[4], "--searcher", "native",
                          "--out", paths[1], "--chunk-bases", "1200"], capture_output=True, text=True,
                         timeout=300, cwd=REPO)
    assert run.returncode == 0, run.stderr[-2000:]
    table = open(paths[1]).read()
    recs = so.search_indexed([s for _, s in contigs], [s for _, s in subjects], so.DEFAULTS)
    want = so.rows(recs, [n for n, _ in contigs], [len(s) for _, s in contigs], [n for n, _ in subjects],
                   [len(s) for _, s in subjects], sum(len(s) for _, s in subjects))
    assert len(want) >= 12
    assert table == "".join(r + "\n" for r in want)
    names = [l.split("\t")[0] for l in table.splitlines()]
    assert [n for i, n in enumerate(names) if i == 0 or names[i - 1] != n] == sorted(set(names))
    batch, tax = inputs.load_inputs(*paths[:4], 200.0, warn=None)
    assert batch.n_hits == len(want)
    run = subprocess.run([sys.executable, "-m", "waafle_amd.orgscorer"] + paths[:4] +
                         ["--outdir", str(tmp_path), "--basename", "s", "--quiet"], capture_output=True,
                         text=True, timeout=300, cwd=REPO)
    assert run.returncode == 0, run.stderr[-2000:]
    models, _ = run_oracle(paths[:4], [])
    rows = output.render(batch, tax, oracle_results(models, batch, tax))
    for kind in ("lgt", "no_lgt", "unclassified"):
        assert open(str(tmp_path / "s.{}.tsv".format(kind))).read() == "\n".join(rows[kind]) + "\n", kind
    assert len(rows["no_lgt"]) + len(rows["lgt"]) >= 1
