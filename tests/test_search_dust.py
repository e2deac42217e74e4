"""The low-complexity mask and its place in the homology search, without a
GPU: the two mask oracles agree with each other and with the written counts on every
hand-built case; the two masked-search oracles agree on theirs, ungapped and gapped;
mask_intervals, the parser, the --dust-out rows and the binding."""
import os
import random
import re

import numpy as np
import pytest

import dust_cases as dc
import dust_oracle as do
import search_cases as sc
import search_dust_cases as sdc
import search_dust_oracle as sdo
import search_gap_oracle as go
import search_oracle as so
from waafle_amd import lib, search

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# the mask
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_mask_oracles_agree_on_hand_built_cases(name):
    contigs, Wd, Lv, masked, mask = dc.expected(name)            # asserts brute == windows
    assert len(mask) == sum(len(c) for c in contigs) and mask.dtype == bool
    if masked is not None:
        assert int(mask.sum()) == masked
    if name in dc.CHECKS:
        dc.CHECKS[name](mask)


def test_mask_facts_of_the_rule():
    def n(*contigs, **kw):
        a, b = do.mask_brute(list(contigs), **kw), do.mask_windows(list(contigs), **kw)
        assert (a == b).all()
        return int(a.sum())
    assert [n("A" * k) for k in range(3, 8)] == [0, 0, 0, 0, 7]
    assert n("A" * 130) == 130
    assert (n("AC" * 5), n("AC" * 6)) == (0, 12)
    assert n("A" * 7, "A" * 7) == 14 and do.intervals(do.mask_windows(["A" * 7, "A" * 7]), [7, 7]) == \
        [(0, 0, 7), (1, 0, 7)]
    # the parameters: a window of 8 bases holds 6 triplets, poly-A scores 3; level 30 is not passed
    assert n("A" * 20, Wd=8, Lv=20) == 20 and n("A" * 20, Wd=8, Lv=30) == 0
    assert n("A" * 6, Lv=19) == 6
    few = do.mask_windows([sc.rnd(5000, 3)])
    assert 0 < int(few.sum()) < 50                               # a fraction of a percent of random bases


def test_mask_oracles_agree_on_seeded_strings():
    units = ["AC", "AG", "ACG", "AAT", "ACGT", "AAAC"]
    for seed in range(20):
        r = random.Random(seed)
        parts = []
        for k in range(8):
            kind = r.randrange(4)
            parts.append([sc.rnd(r.randint(1, 30), seed * 7 + k), r.choice("ACGT") * r.randint(3, 40),
                          r.choice(units) * r.randint(2, 15), "N"][kind])
        s = "".join(parts)
        for Wd, Lv in ((64, 20), (8, 20), (16, 10), (63, 30)):
            assert (do.mask_brute([s], Wd, Lv) == do.mask_windows([s], Wd, Lv)).all(), (seed, Wd, Lv)


# ---------------------------------------------------------------------------
# the search with a mask
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(sdc.HAND_BUILT))
def test_masked_search_oracles_agree_on_hand_built_cases(name):
    contigs, subjects, P, n_plain, n_masked = sdc.HAND_BUILT[name]()
    plain = so.search_brute(contigs, subjects, P)
    masked = sdo.search_brute(contigs, subjects, P)
    assert masked == sdo.search_indexed(contigs, subjects, P)
    assert len(plain) >= 1 if n_plain is None else len(plain) == n_plain
    assert len(masked) == n_masked


def test_masked_cases_show_what_they_claim():
    contigs, subjects, P, _, _ = sdc.internal_poly_a()
    assert sdo.search_indexed(contigs, subjects, P) == so.search_indexed(contigs, subjects, P) == \
        [(0, 0, 0, 150, 0, 300, 300)]
    assert do.mask_windows(contigs)[290:310].all()               # the extension crossed the mask
    contigs, subjects, P, _, _ = sdc.trap()
    mask = do.mask_windows(contigs)
    assert mask[:25].all() and not mask[25:].any()               # the window of a = 24 on contig 0 is masked,
    assert contigs[1].count(contigs[0][24:45]) == 1              # its 21-mer is indexed through contig 1,
    assert sdo.search_indexed(contigs, subjects, P) == [(0, 0, 0, 0, 0, 70, 70)]    # and the HSP is whole
    contigs, subjects, P, _, _ = sdc.max_occ_interplay()
    assert [r[0] for r in sdo.search_indexed(contigs, subjects, P)] == [0, 1, 2]
    contigs, subjects, P, _, _ = sdc.no_low_complexity()
    assert not do.mask_windows(contigs).any()
    assert sdo.search_indexed(contigs, subjects, P) == so.search_indexed(contigs, subjects, P)


@pytest.mark.parametrize("S", [32, 12])
def test_straddle_cases_show_what_they_claim(S):
    contigs, subjects, P, _, _ = sdc._straddle(S)
    lo, hi = sdc.STRADDLE_MASK
    mask = do.mask_windows(contigs)
    assert (mask == do.mask_brute(contigs)).all()
    assert len(contigs) == 1 and len(contigs[0]) == 300 and P["S"] == S
    assert mask[lo:hi].all() and int(mask.sum()) == hi - lo      # the poly-A and nothing else
    q = lo - (S - 1)
    assert q & 31 != 0 and q >> 5 == (lo >> 5) - 1 and lo & 31 == 0
    assert not mask[q - 1:q - 1 + S].any()                       # the S-mer at q - 1 is unmasked,
    assert mask[q:q + S].tolist() == [False] * (S - 1) + [True]  # the one at q only in the next word
    assert subjects == [contigs[0][q - 1:q - 1 + S], contigs[0][q:q + S]]
    assert all(contigs[0].count(s) == 1 for s in subjects)
    assert so.search_indexed(contigs, subjects, P) == [(0, 0, 0, q - 1, 0, S, S), (0, 1, 0, q, 0, S, S)]
    assert sdo.search_indexed(contigs, subjects, P) == sdo.search_brute(contigs, subjects, P) == \
        [(0, 0, 0, q - 1, 0, S, S)]


def test_gapped_planted_gene_with_poly_a_is_one_alignment():
    contigs, subjects, P, n_plain, n_masked = sdc.planted_gapped()
    assert do.mask_windows(contigs)[1000:1030].all()
    cells = sdo.search_gapped_cells(contigs, subjects, P)
    assert cells == sdo.search_gapped_arrays(contigs, subjects, P)
    assert len(cells) == n_masked and sorted(r[1] for r in cells) == [0, 1]
    assert cells == go.search_gapped_arrays(contigs, subjects, P) and len(cells) == n_plain
    assert len(sdo.search_indexed(contigs, subjects, P)) < len(so.search_indexed(contigs, subjects, P))


# ---------------------------------------------------------------------------
# the host side
# ---------------------------------------------------------------------------

def test_mask_intervals():
    off = np.array([0, 5, 5, 12, 14], np.int64)
    mask = np.zeros(14, bool)
    mask[[0, 1, 3, 4, 5, 6, 11, 12, 13]] = True                  # [3, 7) runs over the end of contig 0
    rows = search.mask_intervals(mask, off)
    assert rows == [(0, 0, 2), (0, 3, 5), (2, 0, 2), (2, 6, 7), (3, 0, 2)]
    assert rows == do.intervals(mask, np.diff(off))
    assert search.mask_intervals(np.zeros(14, bool), off) == []
    assert search.mask_intervals(np.zeros(0, bool), np.zeros(1, np.int64)) == []
    assert search.format_mask_rows(rows[:2], ["a", "b", "c", "d"]) == ["a\t0\t2", "a\t3\t5"]


def test_parser_defaults_and_flags():
    ap = search.build_parser()
    a = ap.parse_args(["q.fna", "db.fna"])
    assert (a.dust, a.dust_window, a.dust_level, a.dust_out) == (False, 64, 20, None)
    a = ap.parse_args(["q.fna", "db.fna", "--searcher", "native", "--dust", "--dust-window", "32",
                       "--dust-level", "25", "--dust-out", "m.tsv"])
    assert (a.dust, a.dust_window, a.dust_level, a.dust_out) == (True, 32, 25, "m.tsv")
    assert "blastn's default is on" in ap.format_help()
    assert search.DUST_DEFAULTS == dict(dust_window=64, dust_level=20)
    with pytest.raises(SystemExit):                              # --dust-out alone is refused
        search.main(["q.fna", "db.fna", "--searcher", "native", "--dust-out", "m.tsv"])


def test_rows_of_masked_records_are_the_table_rows():
    contigs, subjects, P, _, _ = sdc.max_occ_interplay()
    recs = sdo.search_indexed(contigs, subjects, P)
    rec = {f: np.array([r[k] for r in recs], dt) for k, (f, dt) in enumerate(search.RECORD_FIELDS)}
    names, lens = ["c{}".format(i) for i in range(len(contigs))], [len(c) for c in contigs]
    got = search.format_rows(rec, search.order_records(rec), names, lens, ["u|s__A"], [len(subjects[0])],
                             len(subjects[0]))
    assert got == sdo.rows(recs, names, lens, ["u|s__A"], [len(subjects[0])], len(subjects[0]))
    assert len(got) == 3 and got[0].split("\t")[:2] == ["c0", "u|s__A"]


def test_binding_and_abi_version():
    assert lib.ABI_VERSION == 6
    header = open(os.path.join(REPO, "include", "waafle_hip.h")).read()
    assert re.search(r"#define WF_ABI_VERSION 6\b", header)
    assert "int wf_search_mask(wf_ctx* ctx, const wf_dust_params* params, wf_dust_result* out);" in header
    res, args = lib.SIGNATURES["wf_search_mask"]
    assert len(args) == 3
    assert [f[0] for f in lib.WfDustParams._fields_][:2] == ["window", "level"]
    assert [f[0] for f in lib.WfDustResult._fields_] == ["mask", "masked_bases", "kmers_before", "kmers_after"]
    import ctypes as C
    assert C.sizeof(lib.WfDustParams) == 16 and C.sizeof(lib.WfDustResult) == 32
    assert hasattr(lib.load(), "wf_search_mask")


def test_tile_constant_matches_the_kernel():
    text = open(os.path.join(REPO, "waafle_amd", "csrc", "wf_internal.h")).read()
    assert int(re.search(r"constexpr int kDustTile = (\d+);", text).group(1)) == search.DUST_TILE
