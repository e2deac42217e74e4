"""The record-to-hit rule of DESIGN.md §13 on the CPU: the two forms of tests/hits_oracle.py agree
on every hand-built case and on every matches value at the lengths where the shortcuts fail;
np.round is not the rule; and the host pieces of waafle_amd/hits.py (subjects parsed once, loci
from the gene caller's arrays) against the readers they stand in for."""
import numpy as np
import pytest

import hits_cases as hc
import hits_oracle as ho
from waafle_amd import genecaller, hits, inputs


@pytest.mark.parametrize("name", sorted(hc.HAND_BUILT))
def test_forms_agree_on_hand_built_cases(name):
    case = hc.HAND_BUILT[name]()
    a, b = ho.form_a(case), ho.form_b(case)
    ho.assert_same(a, b, name)
    assert a["hit_off"].tolist() == case["hit_off"]


def test_scov_at_min_flips_bit_24_only_one_ulp_above():
    keys = {n: ho.form_b(hc.HAND_BUILT[n]())["hit_key"] >> 24 & 1 for n in
            ("scov_min_exact", "scov_min_ulp_above", "scov_min_ulp_below")}
    assert keys["scov_min_exact"].tolist() == [1, 0, 1]
    assert keys["scov_min_ulp_above"].tolist() == [0, 0, 1]
    assert keys["scov_min_ulp_below"].tolist() == [1, 0, 1]


def test_seventh_system_is_in_the_mask_not_in_the_key():
    b = ho.form_b(hc.one_contig_everything())
    assert b["hit_sysmask"].tolist() == [0, 1, 0x7E, 0x7F, 0x82, 1]
    assert (b["hit_key"] >> 26).tolist() == [0, 1, 0x3E, 0x3F, 0x02, 1]


@pytest.fixture(scope="module")
def sweep():
    case = hc.sweep([64, 1600, 8000, 40000])
    return case, ho.form_a(case), ho.form_b(case)


def test_forms_agree_on_every_matches_value(sweep):
    case, a, b = sweep
    assert len(a["hit_score"]) == 65 + 1601 + 8001 + 40001
    ho.assert_same(a, b, "sweep")


def test_np_round_is_not_the_rule_at_8000(sweep):
    case, a, b = sweep
    sel = np.flatnonzero(np.asarray(case["cols"]["length"]) == 8000)
    m = np.asarray(case["cols"]["matches"])[sel]
    want = np.array([float("%.3f" % (100.0 * int(v) / 8000)) for v in m])
    got_b = np.array([ho.pident_b(int(v), 8000) for v in m])
    assert (want.view(np.int64) == got_b.view(np.int64)).all()
    shortcut = np.round(100.0 * m / 8000, 3)
    assert int((shortcut != want).sum()) > 1000
    assert float("%.3f" % (100.0 * 1 / 8000)) == 0.013 and ho.pident_b(1, 8000) == 0.013


def test_subject_tables_against_split_sseqids():
    ids = [s for s, _ in hc.SUBJECTS] + ["x|s__A|b=2|UniProt=Q"]
    t = hits.subject_tables(ids)
    taxa, annots = inputs.split_sseqids(ids)
    assert t.taxa == taxa
    assert t.systems == sorted({s for d in annots if d for s in d})
    for g, d in enumerate(annots):
        got = {t.systems[b]: t.values[b][t.value_ids[g, b]] for b in range(len(t.systems)) if t.value_ids[g, b] >= 0}
        assert got == (d or {})
        assert int(t.sysmask[g]) == sum(1 << t.systems.index(s) for s in (d or {}))
    # only the subjects asked for: their systems alone, the other rows empty
    t = hits.subject_tables(ids, [1, 0])
    assert t.systems == ["UniProt"] and t.taxa[:2] == ["s__A", "s__B"] and t.taxa[2:] == [None] * 4
    assert t.sysmask.tolist() == [0, 1, 0, 0, 0, 0] and t.value_ids.shape == (6, 1)
    t = hits.subject_tables(ids, [0])
    assert t.systems == [] and t.value_ids.shape == (6, 1) and (t.value_ids == -1).all()
    for bad in (["nobar"], ["g|s__A|UniProt"], ["g|s__A|a=b=c"]):
        with pytest.raises(inputs.InputError) as e1:
            inputs.split_sseqids(bad)
        with pytest.raises(inputs.InputError) as e2:
            hits.subject_tables(["g0|s__A"] + bad, [1])
        assert str(e1.value) == str(e2.value)
        hits.subject_tables(["g0|s__A"] + bad, [0])              # a subject without a row is not parsed
    with pytest.raises(inputs.InputError) as exc:
        hits.subject_tables(["g|s__A|" + "|".join("s{}=1".format(k) for k in range(33))])
    assert str(exc.value) == "more than 32 annotation systems"


def test_loci_against_write_gff_then_read_loci(tmp_path):
    names = ["c0", "c1", "c2", "c3", "c4"]
    hit_off = np.array([0, 3, 3, 5, 9, 10], np.int64)            # c1 has no hits
    n_genes = np.array([2, 0, 0, 3, 1], np.int32)                # c2 has hits and no gene
    gs = np.array([10, 500, -1, -1, -1, 1, 300, 900, -1, 40], np.int32)
    ge = np.array([260, 699, -1, -1, -1, 250, 1200, 1099, -1, 239], np.int32)
    gst = np.array([0, 1, 0, 0, 0, 1, 0, 1, 0, 0], np.int8)
    genes = hits.gene_lists(hit_off, n_genes, gs, ge, gst)
    assert [c for c, _ in genes] == [0, 2, 3, 4]
    assert genes[0][1] == [(10, 260, "+"), (500, 699, "-")] and genes[1][1] == []
    path = str(tmp_path / "g.gff")
    genecaller.write_gff(genecaller.GeneCalls([names[c] for c, _ in genes], [gl for _, gl in genes]), path)
    index = {n: i for i, n in enumerate(names)}
    for min_len in (200.0, 201.0, 250.5, 5000.0):                # the filter runs again
        want = inputs.read_loci(path, index, min_len, warn=None)
        assert hits.loci_from_genes(genes, min_len) == want
    assert sorted(inputs.read_loci(path, index, 5000.0, warn=None)) == [0, 3, 4]
    subjects = hits.subject_tables(["g|s__A|k=v", "h|s__B"])
    batch = hits.make_batch(names, [2000] * 5, hit_off, hits.loci_from_genes(genes, 200.0), subjects,
                            [0, 1, 0, 1, 1, 0, 0, 0, 1, 1])
    assert batch.loc_off.tolist() == [0, 2, 2, 2, 5, 6] and batch.n_loci == 6 and batch.max_loci == 3
    assert batch.loc_codes == ["10:260:+", "500:699:-", "1:250:-", "300:1200:+", "900:1099:-", "40:239:+"]
    assert batch.loc_strand.tolist() == [0, 1, 1, 0, 1, 0] and batch.n_hits == 10 and batch.max_hits == 4
    assert batch.annot_value_ids[:, 0].tolist() == [0, -1, 0, -1, -1, 0, 0, 0, -1, -1]
