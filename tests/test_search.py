"""The homology-search rule and the host side of waafle_amd.search, without a GPU: the two
oracles agree on every hand-built case (and give the stated record counts) and on a seeded
random set; the subject-FASTA chunk reader; the ordering and --max-target-seqs step; the row
format; the blastn command of --searcher blastn; and the bit-score formula against the
reference's own demo table."""
import gzip
import math
import os

import numpy as np
import pytest

import search_cases as sc
import search_oracle as so
from waafle_amd import search

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("name", sorted(sc.HAND_BUILT))
def test_oracles_agree_on_hand_built_cases(name):
    contigs, subjects, P, n = sc.HAND_BUILT[name]()
    brute = so.search_brute(contigs, subjects, P)
    assert brute == so.search_indexed(contigs, subjects, P)
    assert len(brute) == n


def test_hand_built_cases_show_what_they_claim():
    def recs(f):
        contigs, subjects, P, _ = f()
        return so.search_brute(contigs, subjects, P)
    assert recs(sc.clip_ends) == [(0, 0, 0, 0, 20, 60, 60), (1, 1, 0, 150, 0, 50, 50)]
    assert recs(sc.contig_junction) == [(0, 0, 0, 110, 0, 40, 40), (1, 0, 0, 0, 40, 40, 40)]
    assert recs(sc.minus_strand) == [(0, 0, 1, 50, 0, 80, 80)]
    assert [r[5:] for r in recs(sc.n_bases)] == [(100, 99), (100, 99)]
    assert [r[4:6] for r in recs(sc.ends_33)] == [(0, 54), (31, 54)]
    assert recs(sc.dip_exactly_x)[0][5:] == (120, 110)
    assert recs(sc.tie_shortest)[0][4:] == (0, 40, 40)
    assert recs(sc.contained)[0][4:] == (0, 103, 88)
    assert [r[4:6] for r in recs(sc.partial_overlap)] == [(0, 77), (37, 77)]
    assert recs(sc.degenerate) == [(2, 2, 0, 50, 0, 50, 50)]


def test_oracles_agree_on_a_random_set():
    for seed in (5, 6):
        contigs, subjects, P = sc.random_small(seed)
        brute = so.search_brute(contigs, subjects, P)
        assert brute == so.search_indexed(contigs, subjects, P)
        assert brute


def test_result_set_does_not_depend_on_the_chunks():
    contigs, subjects, P = sc.random_small(7)
    whole = so.search_indexed(contigs, subjects, P)
    parts = []
    for lo in range(0, len(subjects), 5):
        parts += [(r[0], r[1] + lo) + r[2:] for r in so.search_indexed(contigs, subjects[lo:lo + 5], P)]
    assert sorted(parts) == whole


def test_medium_set_repeat_family_is_past_max_occ():
    """The set the GPU tests use: the bare repeat unit has 70 copies > max_occ = 64, so none of
    its seeds is used and it has no record, while other subjects have hundreds."""
    contigs, subjects, P = sc.medium()
    unit = len(subjects) - 4
    assert sum(c.count(subjects[unit]) for c in contigs) == 70 > P["max_occ"]
    recs = so.search_indexed(contigs, subjects, P)
    assert len(recs) > 200 and not [r for r in recs if r[1] == unit]
    assert {r[2] for r in recs} == {0, 1}


# ---------------------------------------------------------------------------
# the chunk reader
# ---------------------------------------------------------------------------

SUBJECTS = [("g0|s__A|K=1", "ACGTACGTAC"), ("g1|s__B", "GGGGG"), ("g2|s__A", "T" * 23), ("g3|s__C", ""),
            ("g4|s__C", "CATCATCAT"), ("g5|s__A", "AC")]


def write_fasta(path, width=7, gz=False):
    text = "".join(">{} description words\n{}".format(n, "".join(s[i:i + width] + "\n" for i in range(0, len(s), width)))
                   for n, s in SUBJECTS)
    with (gzip.open if gz else open)(path, "wt") as fh:
        fh.write(text)


@pytest.mark.parametrize("gz", [False, True])
def test_chunk_reader_every_boundary(tmp_path, gz):
    path = str(tmp_path / ("db.fna.gz" if gz else "db.fna"))
    write_fasta(path, gz=gz)
    cuts = set()
    for limit in range(1, 60):
        ids, seqs = [], []
        n_before = 0
        for cid, seq, off in search.iter_subject_chunks(path, limit):
            assert len(cid) == len(off) - 1 >= 1 and off[0] == 0 and len(seq) == off[-1]
            assert off[-1] <= limit or len(cid) == 1          # a longer subject is alone
            ids += cid
            seqs += [seq[off[i]:off[i + 1]].tobytes().decode() for i in range(len(cid))]
            n_before += len(cid)
            cuts.add(n_before)
        assert list(zip(ids, seqs)) == SUBJECTS
    assert cuts == set(range(1, len(SUBJECTS) + 1))           # a boundary between any two subjects


def test_chunk_reader_refuses_a_header_without_bar(tmp_path):
    path = str(tmp_path / "bad.fna")
    with open(path, "w") as fh:
        fh.write(">g0|s__A\nACGT\n>plain_name\nACGT\n")
    with pytest.raises(search.SearchError, match="bad subject id header: plain_name"):
        list(search.iter_subject_chunks(path, 100))


# ---------------------------------------------------------------------------
# ordering, --max-target-seqs, rows
# ---------------------------------------------------------------------------

def as_arrays(recs):
    cols = list(zip(*recs)) if recs else [()] * 7
    return {f: np.array(c, dt) for (f, dt), c in zip(search.RECORD_FIELDS, cols)}


HAND = [  # contig, subject, minus, qstart, sstart, length, matches
    (1, 0, 0, 10, 0, 50, 50),      # score 50
    (0, 2, 0, 5, 0, 40, 38),       # 34
    (0, 1, 1, 7, 3, 40, 38),       # 34: subject 1 before subject 2
    (0, 1, 0, 7, 3, 40, 38),       # 34: plus before minus
    (0, 1, 0, 2, 3, 40, 38),       # 34: qstart
    (0, 3, 0, 0, 0, 100, 100),     # 100
    (0, 2, 0, 300, 0, 30, 30),     # 30: subject 2's second row
    (0, 0, 0, 50, 0, 31, 31),      # 31
]


def test_order_and_max_target_seqs():
    rec = as_arrays(HAND)
    assert search.order_records(rec, 10000).tolist() == [5, 4, 3, 2, 1, 7, 6, 0]
    # contig 0 ranks its subjects 3 (100), 1 (34), 2 (34), 0 (31)
    assert search.order_records(rec, 3).tolist() == [5, 4, 3, 2, 1, 6, 0]
    assert search.order_records(rec, 2).tolist() == [5, 4, 3, 2, 0]
    assert search.order_records(rec, 1).tolist() == [5, 0]
    assert search.order_records(as_arrays([]), 5).tolist() == []
    names, lens = ["c0", "c1"], [1000, 800]
    sids, slens = ["s0|t", "s1|t", "s2|t", "s3|t"], [60, 90, 70, 100]
    for limit in (10000, 3, 2, 1):
        got = search.format_rows(rec, search.order_records(rec, limit), names, lens, sids, slens, 320)
        assert got == so.rows(HAND, names, lens, sids, slens, 320, limit)


def test_row_format():
    rec = as_arrays([(0, 0, 0, 10, 4, 60, 57), (0, 0, 1, 100, 4, 90, 90)])
    rows = search.format_rows(rec, np.array([1, 0]), ["ctg"], [500], ["gene|s__A|K=1"], [120], 1000)
    minus, plus = (r.split("\t") for r in rows)
    assert len(plus) == len(minus) == 15
    # plus: subject columns 5..64 ascending; score 57 - 6 = 51
    assert plus[:12] == ["ctg", "gene|s__A|K=1", "500", "120", "60", "11", "70", "5", "64", "95.000", "57", "0"]
    assert plus[13] == "%.1f" % ((1.28 * 51 - math.log(0.46)) / math.log(2)) == "95.3" and plus[14] == "plus"
    # minus: variant columns 4..93 are subject bases 116 down to 27
    assert minus[5:9] == ["101", "190", "116", "27"] and minus[9] == "100.000" and minus[14] == "minus"
    assert minus[13] == "167"                                 # 167.33 bits: above 99.9, truncated
    assert float(plus[12]) == pytest.approx(0.46 * 500 * 1000 * math.exp(-1.28 * 51), rel=1e-2)
    assert search.bitscore_text(53) == "99.0" and search.bitscore_text(54) == "100"
    third = search.format_rows(as_arrays([(0, 0, 0, 0, 0, 30, 29)]), np.array([0]), ["c"], [50], ["g|t"], [30], 30)
    assert third[0].split("\t")[9] == "96.667"


def test_blastn_command_is_the_reference_command():
    args = search.build_parser().parse_args(["dir/my_contigs.v2.fna", "waafledb", "--threads", "4"])
    assert args.searcher == "blastn"
    assert search.default_out(args.query) == "./my_contigs.blastout"
    args.out = search.default_out(args.query)
    assert search.blastn_command(args) == (
        "blastn -query dir/my_contigs.v2.fna -db waafledb -out ./my_contigs.blastout -max_target_seqs 10000 "
        "-num_threads 4 -outfmt '6 qseqid sseqid qlen slen length qstart qend sstart send pident positive "
        "gaps evalue bitscore sstrand'")
    assert "blastdbcmd" in search.build_parser().format_help()


def test_bit_score_formula_against_the_demo_table():
    """The 815 ungapped rows of the reference's demo table: the formula never exceeds the
    file's bit score and equals it on at least 669 rows (BLAST's own raw score can be higher
    than match +1 / mismatch -2 of the whole row, never lower)."""
    path = os.path.join(HERE, "golden", "demo_inputs", "demo_contigs.blastout.gz")
    rows = [l.rstrip("\n").split("\t") for l in gzip.open(path, "rt")]
    rows = [r for r in rows if int(r[11]) == 0]
    assert len(rows) == 815
    equal = 0
    for r in rows:
        score = int(r[10]) - 2 * (int(r[4]) - int(r[10]))
        text = so.bitscore_text(score)
        assert text == search.bitscore_text(score)
        assert float(text) <= float(r[13]), r
        equal += text == r[13]
    assert equal >= 669
