"""The packed gene database (waafle_amd.makedb, search.PackedDb) on the host:
the file round-trips the FASTA by the store's base rules whatever the input's form and
`--chunk-bases`, a damaged file is refused on open, PackedDb.chunks cuts where the FASTA
reader cuts, and search_chunk halves a packed chunk that is too big.  No GPU."""
import gzip
import struct

import numpy as np
import pytest

from waafle_amd import lib, makedb, search

LENGTHS = (0, 1, 31, 32, 33, 64, 1000)
ALPHABET = "ACGTacgtNnRYKMSWBDHV-*"


def _subjects():
    rng = np.random.default_rng(5)
    out = []
    for i, n in enumerate(LENGTHS):
        letters = rng.choice(list(ALPHABET), n, p=[0.2] * 4 + [0.02] * 4 + [0.12 / 14] * 14)
        out.append(("gene{}|s__Sp{}|UniProt=U{}".format(i, i % 3, i), "".join(letters)))
    return out


def _fasta_text(subjects):
    """Multi-line records of varying width, blank lines, words after the id, and spaces."""
    text = ["\n"]
    for i, (sid, seq) in enumerate(subjects):
        width = (7, 60, 33)[i % 3]
        text.append(">{}  some words | more\n".format(sid))
        for a in range(0, len(seq), width):
            text.append("  {}  \n".format(seq[a:a + width]) if a == width else seq[a:a + width] + "\n")
            if a == 2 * width:
                text.append("\n   \n")
    return "".join(text)


def _expected(seq):
    return "".join(ch if ch in "ACGT" else "N" for ch in seq.upper())


def _bits(plane):
    return np.unpackbits(np.ascontiguousarray(plane).view(np.uint8), bitorder="little")


def _decode(lo, hi, nn, first, n):
    """bases [first, first + n) of three planes as text: independent of makedb.pack_words"""
    lo, hi, nn = (_bits(p)[first:first + n] for p in (lo, hi, nn))
    return "".join("N" if k else "ACGT"[a + 2 * b] for a, b, k in zip(lo.tolist(), hi.tolist(), nn.tolist()))


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("db")
    subjects = _subjects()
    fasta, db = str(d / "genes.fna"), str(d / "genes.wfdb")
    with open(fasta, "w") as fh:
        fh.write(_fasta_text(subjects))
    stats = makedb.make_db(fasta, db)
    return d, subjects, fasta, db, stats


def test_round_trip(built):
    _, subjects, _, path, stats = built
    db = search.PackedDb(path)
    total = sum(LENGTHS)
    assert stats["subjects"] == db.n_subjects == len(subjects) and stats["bases"] == db.total == total
    assert list(db.ids) == [sid for sid, _ in subjects] and db.ids[-1] == subjects[-1][0]
    assert db.lens.tolist() == list(LENGTHS)
    assert db.off.tolist() == np.concatenate([[0], np.cumsum(LENGTHS)]).tolist()
    words = (total + 31) // 32 + 2
    assert len(db.lo) == len(db.hi) == len(db.nn) == db.words == words
    assert _decode(db.lo, db.hi, db.nn, 0, total) == "".join(_expected(s) for _, s in subjects)
    assert "N" in _decode(db.lo, db.hi, db.nn, 0, total)
    assert _bits(db.nn)[total:].all() and len(_bits(db.nn)) == 32 * words            # the padding is N
    assert not (np.asarray(db.lo) & np.asarray(db.nn)).any() and not (np.asarray(db.hi) & np.asarray(db.nn)).any()
    import os
    assert os.path.getsize(path) == stats["bytes"] and stats["bytes"] % 64 == 0
    assert not [f for f in os.listdir(os.path.dirname(path)) if ".part-" in f or f.endswith(".tmp")]


def test_sections_are_64_byte_aligned(built):
    _, subjects, _, path, _ = built
    raw = open(path, "rb").read()
    magic, version, zero, n, total, words, id_bytes = struct.unpack_from("<8sIIqqqq", raw, 0)
    assert (magic, version, zero) == (search.DB_MAGIC, search.DB_VERSION, 0)
    sec, length = search.db_sections(n, words, id_bytes)
    assert length == len(raw) and all(at % 64 == 0 for at, _ in sec.values())
    assert np.frombuffer(raw, "<i8", n + 1, sec["off"][0]).tolist() == search.PackedDb(path).off.tolist()
    assert raw[sec["ids"][0]:sec["ids"][0] + id_bytes].decode() == "".join(sid for sid, _ in subjects)


def test_gz_and_chunk_bases_give_the_same_bytes(built, tmp_path):
    _, subjects, fasta, path, _ = built
    want = open(path, "rb").read()
    gz = str(tmp_path / "genes.fna.gz")
    with gzip.open(gz, "wb") as fh:
        fh.write(open(fasta, "rb").read())
    out = str(tmp_path / "other.wfdb")
    makedb.make_db(gz, out)
    assert open(out, "rb").read() == want
    for chunk_bases in (1, 33, 10 ** 9):
        makedb.make_db(fasta, out, chunk_bases=chunk_bases)
        assert open(out, "rb").read() == want, chunk_bases
    makedb.main([fasta, "--out", out, "--chunk-bases", "5"])                        # the command line
    assert open(out, "rb").read() == want


def test_empty_fasta_is_a_database_of_no_subjects(tmp_path):
    fasta, out = str(tmp_path / "e.fna"), str(tmp_path / "e.wfdb")
    open(fasta, "w").write("\n\n")
    assert makedb.make_db(fasta, out)["subjects"] == 0
    db = search.PackedDb(out)
    assert db.n_subjects == 0 and db.total == 0 and len(db.ids) == 0 and len(db.lens) == 0
    assert np.asarray(db.nn).tolist() == [0xFFFFFFFF] * 2 and not np.asarray(db.lo).any()
    assert list(db.chunks(100)) == []
    assert search.is_packed_db(out) and not search.is_packed_db(fasta)


@pytest.mark.parametrize("text, message", [
    (">noheaderbar words\nACGT\n", "bad subject id header: noheaderbar"),
    ("ACGT\n>a|b\nACGT\n", "sequence before the first FASTA header"),
    (">\nACGT\n", "bad subject id header"),
])
def test_rejected_fasta(tmp_path, text, message):
    fasta, out = str(tmp_path / "bad.fna"), str(tmp_path / "bad.wfdb")
    open(fasta, "w").write(text)
    with pytest.raises(search.SearchError) as exc:
        makedb.make_db(fasta, out)
    with pytest.raises(search.SearchError) as ref:                # the FASTA reader's own text
        list(search.iter_subject_chunks(fasta))
    assert message in str(exc.value) and str(exc.value) == str(ref.value)
    import os
    assert os.listdir(str(tmp_path)) == ["bad.fna"]                # nothing half-written is left


def _corrupt(raw, what):
    raw = bytearray(raw)
    n, total, words, id_bytes = struct.unpack_from("<qqqq", raw, 16)
    sec, _ = search.db_sections(n, words, id_bytes)
    at = sec["off"][0]
    if what == "magic":
        raw[0:8] = b"WAAFLEDX"
    elif what == "future version":
        struct.pack_into("<I", raw, 8, search.DB_VERSION + 1)
    elif what == "truncated":
        del raw[-64:]
    elif what == "shorter than a header":
        del raw[40:]
    elif what == "decreasing off":
        struct.pack_into("<q", raw, at + 8 * 3, 0)               # off[3] = 0 after off[2] = 1
    elif what == "off[0] != 0":
        struct.pack_into("<q", raw, at, 1)
    elif what == "off[n] != total":
        struct.pack_into("<q", raw, at + 8 * n, total + 1)
    elif what == "total disagrees with the planes":
        struct.pack_into("<q", raw, 24, total + 64)
    elif what == "n_subjects beyond the file":
        struct.pack_into("<q", raw, 16, n + (1 << 30))
    elif what == "negative n_subjects":
        struct.pack_into("<q", raw, 16, -1)
    return bytes(raw)


@pytest.mark.parametrize("what", ["magic", "future version", "truncated", "shorter than a header", "decreasing off",
                                  "off[0] != 0", "off[n] != total", "total disagrees with the planes",
                                  "n_subjects beyond the file", "negative n_subjects"])
def test_corrupt_database_is_refused_on_open(built, tmp_path, what):
    raw = open(built[3], "rb").read()
    bad = _corrupt(raw, what)
    assert bad != raw
    path = str(tmp_path / "bad.wfdb")
    open(path, "wb").write(bad)
    with pytest.raises(search.SearchError):
        search.PackedDb(path)


@pytest.mark.parametrize("chunk_bases", [1, 100, 10 ** 9])
def test_chunks_are_the_fasta_readers(built, chunk_bases):
    _, subjects, fasta, path, _ = built
    db = search.PackedDb(path)
    want = list(search.iter_subject_chunks(fasta, chunk_bases))
    got = list(db.chunks(chunk_bases))
    assert [(c.first, c.last) for c in got] == [(a, a + len(ids)) for a, ids in zip(
        np.concatenate([[0], np.cumsum([len(ids) for ids, _, _ in want])]).tolist(), [ids for ids, _, _ in want])]
    assert [c.first for c in got] + [db.n_subjects] == [0] + [c.last for c in got]     # each once, in order
    for c, (ids, seq, off) in zip(got, want):
        assert db.ids[c.first:c.last] == ids
        assert c.off.tolist() == off.tolist() and c.off.dtype == np.int64
        total = int(off[-1])
        assert 0 <= c.bit0 <= 31 and c.bit0 == int(db.off[c.first]) & 31
        assert len(c.lo) == len(c.hi) == len(c.nn) == (c.bit0 + total + 31) // 32
        assert _decode(c.lo, c.hi, c.nn, c.bit0, total) == _expected(seq.tobytes().decode())
        for view, plane in ((c.lo, db.lo), (c.hi, db.hi), (c.nn, db.nn)):
            assert total == 0 or np.shares_memory(view, plane)                         # views, not copies


class _TooBigAbove:
    """A searcher that refuses more than k subjects, or more than `bases` bases, per call and
    otherwise reports one record per subject: its index in the call and its length."""

    def __init__(self, k, bases=1 << 40):
        self.k, self.bases, self.calls = k, bases, []

    def _run(self, chunk):
        n = len(chunk.off) - 1
        if n > self.k or chunk.off[-1] > self.bases:
            raise lib.WaafleHipError(lib.WF_E_TOOBIG, "a chunk of {} bases".format(int(chunk.off[-1])))
        self.calls.append((chunk.first, chunk.last, chunk.bit0, len(chunk.lo)))
        return dict(subject=np.arange(n, dtype=np.int32), length=np.diff(chunk.off).astype(np.int32),
                    text=np.array([_decode(chunk.lo, chunk.hi, chunk.nn, chunk.bit0 + int(chunk.off[g]),
                                           int(chunk.off[g + 1] - chunk.off[g])) for g in range(n)], dtype=object))

    search_packed = search_gapped_packed = _run


@pytest.mark.parametrize("gapped", [False, True])
def test_search_chunk_halves_a_packed_chunk(built, gapped):
    _, subjects, _, path, _ = built
    db = search.PackedDb(path)
    whole = db.chunk(0, db.n_subjects)
    fake = _TooBigAbove(1)
    out = search.search_chunk(fake, whole, None, gapped)
    assert out["subject"].tolist() == list(range(len(LENGTHS)))                      # shifted back
    assert out["length"].tolist() == list(LENGTHS)
    assert out["text"].tolist() == [_expected(s) for _, s in subjects]               # bit0 and slices recomputed
    assert [(a, b) for a, b, _, _ in fake.calls] == [(g, g + 1) for g in range(len(LENGTHS))]
    assert [b0 for _, _, b0, _ in fake.calls] == [int(o) & 31 for o in db.off[:-1]]
    fake = _TooBigAbove(3)
    out = search.search_chunk(fake, whole, None, gapped)
    assert out["subject"].tolist() == list(range(len(LENGTHS))) and max(b - a for a, b, _, _ in fake.calls) <= 3
    with pytest.raises(search.SearchError) as exc:
        search.search_chunk(_TooBigAbove(7, bases=999), whole, None, gapped)
    assert "a single subject is too big" in str(exc.value)
    with pytest.raises(lib.WaafleHipError):                                          # other errors pass through
        class Broken(_TooBigAbove):
            def _run(self, chunk):
                raise lib.WaafleHipError(lib.WF_E_HIP, "x")
            search_packed = search_gapped_packed = _run
        search.search_chunk(Broken(1), whole, None, gapped)
