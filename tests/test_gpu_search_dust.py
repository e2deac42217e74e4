"""wf_search_mask (wf_dust.hip) on the GPU against the CPU oracles of DESIGN.md §12.6: the mask
base for base on every hand-built case and across the kernel's tile boundaries; the records
of wf_search and wf_search_gapped on a masked index against the masked-search oracles, on
every field; index replacement, the parameter checks, a mapper on another context, and
`python -m waafle_amd.search --searcher native --dust` followed by `waafle_amd.orgscorer`."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import dust_cases as dc
import dust_oracle as do
import map_cases as mc
import search_cases as sc
import search_dust_cases as sdc
import search_dust_oracle as sdo
import search_oracle as so
from oracle_bridge import oracle_results, run_oracle
from waafle_amd import inputs, lib, mapper, output, search

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [f for f, _ in search.RECORD_FIELDS]
GAP_FIELDS = [f for f, _ in search.GAP_RECORD_FIELDS]


def kw(P):
    out = dict(seed_length=P["S"], seed_stride=P["T"], max_seed_hits=P["max_occ"], xdrop=P["X"],
               min_score=P["min_score"], dust_window=P["Wd"], dust_level=P["Lv"])
    if "W" in P:
        out.update(band=P["W"], xdrop_gap=P["Xg"])
    return out


def records(out, fields=FIELDS):
    return sorted(zip(*[out[f].tolist() for f in fields]))


def run_chunks(s, subjects, size):
    got = []
    for lo in range(0, len(subjects), size):
        out = s.search(*sc.flat(subjects[lo:lo + size]))
        out["subject"] = out["subject"] + np.int32(lo)
        got += records(out)
    return sorted(got)


# ---------------------------------------------------------------------------
# the mask
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_mask_equals_both_oracles(name):
    contigs, Wd, Lv, masked, want = dc.expected(name)            # the two forms agree
    with search.Searcher(*sc.flat(contigs), dust=True, dust_window=Wd, dust_level=Lv) as s:
        got = s.mask()
        assert got.dtype == bool and got.shape == want.shape
        np.testing.assert_array_equal(got, want)
        assert s.stats["masked_bases"] == s.dust_stats["masked_bases"] == int(want.sum())
        if masked is not None:
            assert s.stats["masked_bases"] == masked
        assert s.dust_stats["kmers_after"] <= s.dust_stats["kmers_before"]
    with search.Searcher(*sc.flat(contigs)) as s:
        assert s.mask() is None and s.stats["masked_bases"] == 0


def test_mask_across_tile_boundaries():
    """One contig of three tiles per placement: the 40-base repeat starts 70 bases before to
    70 bases after the first tile boundary of its contig, then the same at the second.  Every
    contig starts on a tile boundary of the store."""
    tile = search.DUST_TILE
    back = sc.rnd(3 * tile, 31)
    rep = ("ACT" * 14)[:40]
    contigs = [back[:b + d] + rep + back[b + d + 40:] for b in (tile, 2 * tile) for d in range(-70, 71)]
    assert len(contigs) == 282 and all(len(c) == 3 * tile for c in contigs)
    want = do.mask_windows(contigs)
    assert want.reshape(282, -1)[:, tile - 70:2 * tile + 110].any(axis=1).all()     # each repeat is masked
    with search.Searcher(*sc.flat(contigs), dust=True) as s:
        got = s.mask()
    diff = np.flatnonzero(got != want)
    assert len(diff) == 0, "first difference at store base {} (contig {}, base {})".format(
        diff[0], diff[0] // (3 * tile), diff[0] % (3 * tile))


# ---------------------------------------------------------------------------
# records on a masked index
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(sdc.HAND_BUILT))
def test_records_equal_both_masked_oracles(name):
    contigs, subjects, P, n_plain, n_masked = sdc.HAND_BUILT[name]()
    want = sdo.search_brute(contigs, subjects, P)
    assert want == sdo.search_indexed(contigs, subjects, P) and len(want) == n_masked
    GP = sdc.gap_params(**P)
    want_gap = sdo.search_gapped_cells(contigs, subjects, GP)
    assert want_gap == sdo.search_gapped_arrays(contigs, subjects, GP, records=want)
    with search.Searcher(*sc.flat(contigs), dust=True, **kw(GP)) as s:
        assert records(s.search(*sc.flat(subjects))) == want
        assert records(s.search_gapped(*sc.flat(subjects)), GAP_FIELDS) == want_gap
    with search.Searcher(*sc.flat(contigs), **kw(GP)) as s:      # and without the mask, as before
        plain = records(s.search(*sc.flat(subjects)))
    assert plain == so.search_indexed(contigs, subjects, P)
    assert len(plain) >= 1 if n_plain is None else len(plain) == n_plain


def test_gapped_planted_gene_crosses_the_mask():
    contigs, subjects, P, _, n = sdc.planted_gapped()
    ungapped = sdo.search_indexed(contigs, subjects, P)
    want = sdo.search_gapped_arrays(contigs, subjects, P, records=ungapped)
    assert len(want) == n
    with search.Searcher(*sc.flat(contigs), dust=True, **kw(P)) as s:
        assert s.mask()[1000:1030].all()
        assert records(s.search(*sc.flat(subjects))) == ungapped
        assert records(s.search_gapped(*sc.flat(subjects)), GAP_FIELDS) == want


@pytest.fixture(scope="module")
def medium():
    contigs, subjects, P = sdc.medium_low()
    return contigs, subjects, P, sdo.search_indexed(contigs, subjects, P)


def test_medium_set_with_repeats(medium):
    contigs, subjects, P, want = medium
    assert want != so.search_indexed(contigs, subjects, P)       # the mask changes this set's records
    with search.Searcher(*sc.flat(contigs), dust=True, **kw(P)) as s:
        np.testing.assert_array_equal(s.mask(), do.mask_windows(contigs))
        assert 0 < s.dust_stats["kmers_after"] < s.dust_stats["kmers_before"]
        assert run_chunks(s, subjects, len(subjects)) == want
        assert run_chunks(s, subjects, 7) == want
        assert run_chunks(s, subjects, len(subjects)) == want    # twice over
        assert s.stats["raw_hsps"] + s.stats["seeds_skipped"] == s.stats["seed_hits"] > 0


def test_index_replacement(medium):
    contigs, subjects, P, want = medium
    subjects = subjects[:40]
    want = [r for r in want if r[1] < 40]
    other, _, _, _, _ = sdc.poly_a_against_poly_a()
    with search.Searcher(*sc.flat(contigs), dust=True, **kw(P)) as s:
        assert run_chunks(s, subjects, 40) == want
        s.mapper.index(*sc.flat(contigs))                        # wf_map_index alone: no mask again
        assert run_chunks(s, subjects, 40) == so.search_indexed(contigs, subjects, P)
        s.apply_mask(sum(len(c) for c in contigs))               # wf_search_mask again
        assert run_chunks(s, subjects, 40) == want
        s.index(*sc.flat(other))                                 # Searcher.index masks the new contigs
        np.testing.assert_array_equal(s.mask(), do.mask_windows(other))
        assert s.stats["masked_bases"] == 40
        _, subj, P2, _, _ = sdc.poly_a_against_poly_a()
        assert run_chunks(s, subj, 1) == []


def test_parameter_checks_and_no_index():
    contigs, _, _, _, _ = sdc.internal_poly_a()
    with search.Searcher(*sc.flat(contigs)) as s:
        for window, level in ((7, 20), (65, 20), (0, 20), (64, 0), (64, -5)):
            with pytest.raises(lib.WaafleHipError) as exc:
                s.apply_mask(len(contigs[0]), params=lib.WfDustParams(window=window, level=level))
            assert exc.value.code == lib.WF_E_BADINPUT, (window, level)
        assert s.mask() is None
        for window, level in ((8, 1), (64, 1 << 30)):            # the ends of the ranges are accepted
            s.apply_mask(len(contigs[0]), params=lib.WfDustParams(window=window, level=level))
            np.testing.assert_array_equal(s.mask(), do.mask_windows(contigs, window, level))
    h = C.c_void_p()
    dll = lib.load()
    assert dll.wf_init(0, C.byref(h)) == lib.WF_OK
    try:
        r = lib.WfDustResult()
        p = lib.WfDustParams(window=64, level=20)
        assert dll.wf_search_mask(h, C.byref(p), C.byref(r)) == lib.WF_E_STATE
    finally:
        dll.wf_free(h)


def test_mapper_on_another_context_is_untouched():
    contigs, r1, r2, P, _ = mc.orientation()
    with mapper.Mapper(*mc.flat(contigs), seed_length=P["S"]) as m:
        params = lib.WfMapParams(seed_len=P["S"], max_occ=16, max_mm=P["max_mm"], min_insert=P["min_insert"],
                                 max_insert=P["max_insert"])
        before = m.map(*mc.flat(r1), *mc.flat(r2), params=params)
        assert (before["contig"] >= 0).any()
        with search.Searcher(*mc.flat(list(contigs) + [b"A" * 60]), seed_length=P["S"], dust=True) as s:
            assert s.stats["masked_bases"] >= 60
            s.search(*mc.flat([contigs[0][10:90]]))
        after = m.map(*mc.flat(r1), *mc.flat(r2), params=params)
    for f in before:
        np.testing.assert_array_equal(before[f], after[f])


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------

def _sample(tmp_path):
    """Three contigs of two genes each (species A as they are, species B with 3 % substitutions);
    a poly-A x40 inside the first gene of contig 0 (the genes are cut after it is written), an
    (AC)x20 outside the genes of contig 2, and a junk subject that shares only a poly-A."""
    import random
    rng = random.Random(4)
    contigs, subjects, gff = [], [], []
    for c in range(3):
        seq = sc.rnd(1500, 400 + c)
        if c == 0:
            seq = seq[:300] + "A" * 40 + seq[340:]
        if c == 2:
            seq = seq[:650] + "AC" * 20 + seq[690:]
        contigs.append(("ctg{}".format(c), seq))
        for k, (a, b) in enumerate(((100, 600), (800, 1300))):
            gene = seq[a:b]
            other = "".join(ch if rng.random() > 0.03 else rng.choice("ACGT") for ch in gene)
            subjects.append(("g{}{}a|s__A|UniProt=U{}{}".format(c, k, c, k), gene))
            subjects.append(("g{}{}b|s__B|UniProt=U{}{}".format(c, k, c, k), other))
            gff.append("\t".join(["ctg{}".format(c), "x", "gene", str(a + 1), str(b), ".", "+", "0", "."]))
    subjects.append(("junk|s__B|UniProt=J", "C" + sc.rnd(99, 77) + "A" * 40 + sc.rnd(99, 78) + "C"))
    paths = [str(tmp_path / n) for n in ("s.fna", "s.blastout", "s.gff", "s.tsv", "genes.fna", "s.dust.tsv")]
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


def test_native_search_with_dust_then_orgscorer(tmp_path):
    contigs, subjects, paths = _sample(tmp_path)
    run = subprocess.run([sys.executable, "-m", "waafle_amd.search", paths[0], paths[4], "--searcher", "native",
                          "--dust", "--dust-out", paths[5], "--out", paths[1], "--chunk-bases", "1200"],
                         capture_output=True, text=True, timeout=300, cwd=REPO)
    assert run.returncode == 0, run.stderr[-2000:]
    cs, ss = [s for _, s in contigs], [s for _, s in subjects]
    names, lens = [n for n, _ in contigs], [len(s) for _, s in contigs]
    recs = sdo.search_indexed(cs, ss, sdo.DEFAULTS)
    plain = so.search_indexed(cs, ss, so.DEFAULTS)
    junk = len(subjects) - 1
    assert [r for r in plain if r[1] == junk] and not [r for r in recs if r[1] == junk]
    want = sdo.rows(recs, names, lens, [n for n, _ in subjects], [len(s) for s in ss], sum(len(s) for s in ss))
    assert len(want) >= 12
    assert open(paths[1]).read() == "".join(r + "\n" for r in want)
    mask = do.mask_windows(cs)
    rows = ["{}\t{}\t{}".format(names[c], a, b) for c, a, b in do.intervals(mask, lens)]
    assert any(r.startswith("ctg0\t") for r in rows) and any(r.startswith("ctg2\t") for r in rows)
    assert open(paths[5]).read() == "".join(r + "\n" for r in rows)
    batch, tax = inputs.load_inputs(*paths[:4], 200.0, warn=None)
    assert batch.n_hits == len(want)
    run = subprocess.run([sys.executable, "-m", "waafle_amd.orgscorer"] + paths[:4] +
                         ["--outdir", str(tmp_path), "--basename", "s", "--quiet"], capture_output=True,
                         text=True, timeout=300, cwd=REPO)
    assert run.returncode == 0, run.stderr[-2000:]
    models, _ = run_oracle(paths[:4], [])
    out = output.render(batch, tax, oracle_results(models, batch, tax))
    for kind in ("lgt", "no_lgt", "unclassified"):
        assert open(str(tmp_path / "s.{}.tsv".format(kind))).read() == "\n".join(out[kind]) + "\n", kind
    assert len(out["no_lgt"]) + len(out["lgt"]) >= 1
