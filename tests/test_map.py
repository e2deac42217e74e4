"""Built-in read mapper, host side (no GPU): the two CPU oracles of the mapping rule agree,
the FASTQ / FASTA readers, the SAM writer against junctions.read_pairs, the ctypes binding
and the CLI defaults.  The kernel itself is checked in tests/test_gpu_map.py."""
import ctypes
import gzip

import numpy as np
import pytest

import map_cases as mc
import map_oracle as mo
from waafle_amd import junctions, lib, mapper


@pytest.mark.parametrize("name", sorted(mc.HAND_BUILT))
def test_oracles_agree_on_hand_built_cases(name):
    contigs, r1, r2, P, aligned = mc.HAND_BUILT[name]()
    brute = mo.map_pairs_brute(contigs, r1, r2, P)
    assert mo.map_pairs_indexed(contigs, r1, r2, P) == brute
    assert [r[0] >= 0 for r in brute] == aligned


def test_oracle_hand_checked_results():
    contigs, r1, r2, P, _ = mc.orientation()
    got = mo.map_pairs_indexed(contigs, r1, r2, P)
    assert got[0] == (0, 61, 291, 0, 0, 0)              # mate 1 at 60, mate 2 ends at 380
    assert got[1] == (0, 281, 61, 1, 0, 0)
    contigs, r1, r2, P, _ = mc.repeats()
    got = mo.map_pairs_indexed(contigs, r1, r2, P)
    assert got[2][0] == 1                               # identical contigs 1 and 2: the lower
    assert got[3][:3] == (3, 66, 91)                    # tandem: lowest start, then shortest
    contigs, r1, r2, P, _ = mc.mismatches()
    got = mo.map_pairs_indexed(contigs, r1, r2, P)
    assert got[0][4:] == (4, 0) and got[1][4:] == (4, 4)
    contigs, r1, r2, P, _ = mc.n_and_case()
    assert [g[4] for g in mo.map_pairs_indexed(contigs, r1, r2, P)][:4] == [1, 0, 2, 2]


def test_oracles_agree_on_small_random_set():
    contigs, r1, r2, P = mc.medium(seed=3, n_contigs=3, n_pairs=12)
    contigs = [c[:260] for c in contigs]
    assert mo.map_pairs_indexed(contigs, r1, r2, P) == mo.map_pairs_brute(contigs, r1, r2, P)


def test_planted_contigs_have_unique_kmers():
    contigs, _, _, P, _ = mc.planted()
    assert mc.unique_kmers(contigs, P["S"])
    assert not mc.unique_kmers([b"ACGTACGTACGTACGTACGTACGTA"], 20)


# ---------------------------------------------------------------------------
# readers
# ---------------------------------------------------------------------------

FQ1 = "@r1/1 extra words\nACGT\n+\nIIII\n@r2/1\nGGNA\n+r2/1\n!!!!\n@pair3\tx\nTT\n+\nII\n"
FQ2 = "@r1/2\nTTTT\n+\nIIII\n@r2/2 z\nCC\n+\n!!\n@pair3\nAAAAA\n+\nIIIII\n"


def test_fastq_names_and_sequences(tmp_path):
    p1, p2 = tmp_path / "a_1.fq", tmp_path / "a_2.fq.gz"
    p1.write_text(FQ1)
    with gzip.open(str(p2), "wt") as fh:
        fh.write(FQ2.rstrip("\n"))                       # (no newline at the end of the file)
    for chunk in (1, 2, 100):
        blocks = list(mapper.iter_fastq_pairs(str(p1), str(p2), chunk=chunk))
        assert sum(len(b1) for b1, _ in blocks) == 3
        names = [b1.qname(i) for b1, _ in blocks for i in range(len(b1))]
        assert names == ["r1", "r2", "pair3"]
        s1 = [bytes(b1.seq[b1.off[i]:b1.off[i + 1]]) for b1, _ in blocks for i in range(len(b1))]
        s2 = [bytes(b2.seq[b2.off[i]:b2.off[i + 1]]) for _, b2 in blocks for i in range(len(b2))]
        assert s1 == [b"ACGT", b"GGNA", b"TT"] and s2 == [b"TTTT", b"CC", b"AAAAA"]


def test_fastq_crlf_and_trailing_blank_lines(tmp_path):
    p = tmp_path / "c.fq"
    p.write_bytes(FQ1.replace("\n", "\r\n").encode() + b"\r\n\n")
    (blk,) = list(mapper.iter_fastq(str(p)))
    assert [blk.qname(i) for i in range(3)] == ["r1", "r2", "pair3"]
    assert bytes(blk.seq) == b"ACGTGGNATT"


def test_fastq_truncated_and_multiline_records_are_refused(tmp_path):
    cut = tmp_path / "cut.fq"
    cut.write_text(FQ1[:FQ1.rindex("+")])                # the last record stops after its bases
    with pytest.raises(mapper.MapperError, match="truncated"):
        list(mapper.iter_fastq(str(cut)))
    short = tmp_path / "short.fq"
    short.write_text(FQ1[:-2] + "\n")                    # ... or has a short quality line
    with pytest.raises(mapper.MapperError):
        list(mapper.iter_fastq(str(short)))
    multi = tmp_path / "multi.fq"
    multi.write_text("@r1\nACGT\nACGT\n+\nIIII\nIIII\n@r2\nAC\n+\nII\n")
    with pytest.raises(mapper.MapperError, match="4-line"):
        list(mapper.iter_fastq(str(multi)))


def test_fastq_mate_names_must_agree(tmp_path):
    p1, p2 = tmp_path / "1.fq", tmp_path / "2.fq"
    p1.write_text(FQ1)
    p2.write_text(FQ2.replace("@r2/2", "@other/2"))
    with pytest.raises(mapper.MapperError, match="r2 / other"):
        list(mapper.iter_fastq_pairs(str(p1), str(p2)))
    p2.write_text(FQ2[:FQ2.index("@pair3")])
    with pytest.raises(mapper.MapperError, match="different numbers"):
        list(mapper.iter_fastq_pairs(str(p1), str(p2)))


def test_fasta_sequences_match_contig_lengths(tmp_path):
    from waafle_amd import inputs
    p = tmp_path / "c.fna"
    p.write_text(">c1 desc\nACGT\nacgtn\n>c2\nGG\n>empty\n>c3\nTTT\n")
    names, seq, off = mapper.read_fasta(str(p))
    assert names == ["c1", "c2", "empty", "c3"] and bytes(seq) == b"ACGTacgtnGGTTT"
    assert off.tolist() == [0, 9, 11, 11, 14]
    lengths = inputs.read_contig_lengths(str(p))
    assert list(lengths) == names and list(lengths.values()) == np.diff(off).tolist()
    p.write_text(">c1\nAC\n>c1\nGT\n")
    with pytest.raises(mapper.MapperError):
        mapper.read_fasta(str(p))


# ---------------------------------------------------------------------------
# SAM writer
# ---------------------------------------------------------------------------

def test_sam_round_trip_through_read_pairs(tmp_path):
    names = ["ctgA", "ctgB", "ctgC"]
    res = dict(contig=np.array([1, -1, 0, 2, -1], np.int32), pos1=np.array([5, 0, 300, 1, 0], np.int32),
               pos2=np.array([205, 0, 120, 1, 0], np.int32), strand1=np.array([0, 0, 1, 0, 0], np.uint8),
               mm1=np.array([0, 0, 3, 1, 0], np.uint8), mm2=np.array([2, 0, 0, 0, 0], np.uint8))
    len1 = np.array([100, 100, 151, 20, 30])
    len2 = np.array([90, 100, 151, 20, 19])
    qnames = ["q{}".format(i) for i in range(5)]
    lines = mapper.sam_header(names, [1000, 2000, 20]) + mapper.sam_records(qnames, len1, len2, res, names)
    sam = tmp_path / "x.sam"
    sam.write_text("\n".join(lines) + "\n")
    recs = [l.split("\t") for l in lines if not l.startswith("@")]
    assert len(recs) == 10 and all(len(r) >= 11 for r in recs)
    assert [r[1] for r in recs] == ["99", "147", "77", "141", "83", "163", "99", "147", "77", "141"]
    assert recs[0][3:9] == ["5", "255", "100M", "=", "205", "290"] and recs[0][11] == "NM:i:0"
    assert recs[1][3:9] == ["205", "255", "90M", "=", "5", "-290"] and recs[1][11] == "NM:i:2"
    assert recs[4][8] == "-331" and recs[5][8] == "331"
    assert recs[2][2] == "*" and recs[2][5] == "*"
    assert lines[0].startswith("@HD") and lines[2] == "@SQ\tSN:ctgB\tLN:2000"
    got = junctions.read_pairs(str(sam), {n: i for i, n in enumerate(names)})
    want = mapper.pair_arrays(res, len1, len2)
    assert got[5] == []
    for g, w in zip(got[:5], want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert got[0].tolist() == [1, 0, 2]                   # unaligned pairs yield nothing
    assert got[2].tolist() == [104, 450, 20] and got[4].tolist() == [294, 270, 20]


# ---------------------------------------------------------------------------
# binding and CLI
# ---------------------------------------------------------------------------

def test_map_entry_points_are_bound():
    assert {"wf_map_index", "wf_map_pairs"} <= set(lib.SIGNATURES)
    so = lib.load()
    assert so.wf_abi_version() == 6
    assert ctypes.sizeof(lib.WfMapParams) == 32 and lib.WfMapParams.min_insert.offset == 16
    assert ctypes.sizeof(lib.WfMapContigs) == 24 and ctypes.sizeof(lib.WfMapReads) == 48
    assert ctypes.sizeof(lib.WfMapResult) == 48
    # argument checks come before any device call
    assert so.wf_map_index(None, None, None) == lib.WF_E_BADINPUT
    assert so.wf_map_pairs(None, None, None, None) == lib.WF_E_BADINPUT


def test_cli_defaults_unchanged_and_mapper_options():
    ap = junctions.build_parser()
    a = ap.parse_args(["c.fna", "g.gff"])
    assert (a.mapper, a.seed_length, a.max_seed_hits, a.max_mismatches, a.min_insert, a.max_insert) == \
        ("bowtie2", 20, 16, 4, 0, 500)
    assert (a.min_overlap_sites, a.bowtie2, a.bowtie2_build, a.threads, a.resume, a.gpu, a.tmpdir,
            a.outdir, a.basename, a.write_detailed_output, a.sam, a.reads1, a.reads2) == \
        (25, "bowtie2", "bowtie2-build", 1, False, 0, ".", ".", None, False, None, None, None)
    assert mapper.DEFAULTS == dict(seed_length=20, max_seed_hits=16, max_mismatches=4, min_insert=0,
                                   max_insert=500)
    a = ap.parse_args(["c.fna", "g.gff", "--mapper", "native", "--seed-length", "24"])
    assert a.mapper == "native" and a.seed_length == 24
    with pytest.raises(SystemExit):
        ap.parse_args(["c.fna", "g.gff", "--mapper", "bwa"])
