"""The packed database on the GPU (wf_search_packed, wf_search_gapped_packed, k_search_unpack;
DESIGN.md §12.7).  The store k_search_unpack leaves on the device must equal, word for word
and on both strands, the store k_map_pack leaves for the same chunk as ASCII, at every bit
offset of the chunk in the file and with real bases next to it; the records and counters of
the packed calls must equal those of the ASCII calls and of the CPU oracles on every
hand-built case, on the medium sets however they are cut, under the capacity protocol; the
new argument checks; and `python -m waafle_amd.search` gives the same bytes from a .wfdb as
from the FASTA it was made of."""
import ctypes as C
import os
import random
import subprocess
import sys
import types

import numpy as np
import pytest

import search_cases as sc
import search_dust_cases as sdc
import search_dust_oracle as sdo
import search_gap_cases as gc
import search_gap_oracle as go
import search_oracle as so
from waafle_amd import lib, makedb, search

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [f for f, _ in search.RECORD_FIELDS]
GAP_FIELDS = [f for f, _ in search.GAP_RECORD_FIELDS]


def kw(P):
    out = dict(seed_length=P["S"], seed_stride=P["T"], max_seed_hits=P["max_occ"], xdrop=P["X"],
               min_score=P["min_score"])
    if "W" in P:
        out.update(band=P["W"], xdrop_gap=P["Xg"])
    if "Wd" in P:
        out.update(dust_window=P["Wd"], dust_level=P["Lv"])
    return out


def records(out, fields=FIELDS):
    return sorted(zip(*[out[f].tolist() for f in fields]))


def make(tmp_path, subjects, name="genes"):
    """the PackedDb of the sequences `subjects`, through a FASTA file and makedb"""
    fasta, path = str(tmp_path / (name + ".fna")), str(tmp_path / (name + ".wfdb"))
    with open(fasta, "w") as fh:
        fh.write("".join(">s{}|t__T\n{}\n".format(i, s) for i, s in enumerate(subjects)))
    makedb.make_db(fasta, path)
    return search.PackedDb(path)


def reset(s):
    s.stats = dict.fromkeys(s.stats, 0)


def counters(s, names=search.GAP_STAT_FIELDS):
    return {f: s.stats[f] for f in names}


# ---------------------------------------------------------------------------
# the store, word for word
# ---------------------------------------------------------------------------

def letters(n, alphabet, seed):
    r = random.Random(seed)
    return "".join(r.choice(alphabet) for _ in range(n))


def both_stores(s, chunk, text):
    """The device's store of both strands after the packed call on `chunk`, and after the
    ASCII call on the same bases; a decoy of other bases is searched before each, so that a
    call that wrote nothing cannot pass."""
    total = len(text)
    decoy = sc.flat(["T" * total])
    s.search(*decoy)
    rec_p = s.search_packed(chunk)
    packed = [s.chunk_planes(total, strand) for strand in (0, 1)]
    s.search(*decoy)
    rec_a = s.search(*sc.flat([text]))
    ascii_ = [s.chunk_planes(total, strand) for strand in (0, 1)]
    assert records(rec_p) == records(rec_a)
    return packed, ascii_


def assert_same_store(packed, ascii_, total, what):
    words = (total + 31) // 32 + 2
    for strand in (0, 1):
        for plane, p, a in zip(("lo", "hi", "nn"), packed[strand], ascii_[strand]):
            assert len(p) == len(a) == words
            diff = np.flatnonzero(p != a)
            assert len(diff) == 0, "{}: strand {} plane {} word {}: {:#010x} for {:#010x}".format(
                what, strand, plane, diff[0], int(p[diff[0]]), int(a[diff[0]]))
        lo, hi, nn = packed[strand]
        assert not (lo & nn).any() and not (hi & nn).any()
        assert (nn[-2:] == 0xFFFFFFFF).all()                        # the two padding words


@pytest.fixture(scope="module")
def plane_searcher():
    contig = letters(300, "AC", 1)
    with search.Searcher(*sc.flat([contig]), seed_length=12, seed_stride=4, min_score=12) as s:
        yield s


@pytest.mark.parametrize("total", [31, 32, 33, 63, 64, 65, 97])
def test_store_equals_map_packs(plane_searcher, tmp_path, total):
    """The chunk is made of A and C, its neighbours in the file of G and T: a neighbour's bit
    that reaches the store shows as a base where k_map_pack has an N, or as a wrong base."""
    s = plane_searcher
    for bit0 in (0, 1, 31):
        for variant in ("plain", "n ends", "first subject", "last subject"):
            if variant == "first subject" and bit0:
                continue                                             # the file's first subject is at bit 0
            chunk = letters(total, "AC", 100 * total + bit0)
            if variant == "n ends":
                chunk = "N" + chunk[1:-1] + "R"
            before = [] if variant == "first subject" else [letters(32 + bit0, "GT", 7)]
            after = [] if variant == "last subject" else [letters(40, "GT", 8)]
            what = "total {} bit0 {} {}".format(total, bit0, variant)
            db = make(tmp_path, before + [chunk] + after, "t{}b{}{}".format(total, bit0, variant[0]))
            ch = db.chunk(len(before), len(before) + 1)
            assert ch.bit0 == bit0 and int(ch.off[-1]) == total, what
            assert_same_store(*both_stores(s, ch, chunk), total, what)


def test_dirty_planes_give_a_clean_store(plane_searcher, tmp_path):
    """lo and hi set under nn in the input (a file this reader's makedb never writes): the
    kernel clears them itself."""
    s = plane_searcher
    chunk = "NN" + letters(40, "AC", 3) + "NRY" + letters(30, "AC", 4) + "N"
    db = make(tmp_path, [letters(37, "GT", 5), chunk, letters(40, "GT", 6)])
    ch = db.chunk(1, 2)
    nn = np.array(ch.nn)
    assert nn.any()
    dirty = types.SimpleNamespace(off=ch.off, bit0=ch.bit0, lo=np.array(ch.lo) | nn, hi=np.array(ch.hi) | nn, nn=nn)
    assert ch.bit0 == 5 and ((dirty.lo & nn) != 0).any()
    assert_same_store(*both_stores(s, dirty, chunk), len(chunk), "dirty planes")


# ---------------------------------------------------------------------------
# records
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(sc.HAND_BUILT))
def test_hand_built_cases(name, tmp_path):
    contigs, subjects, P, n = sc.HAND_BUILT[name]()
    want = so.search_indexed(contigs, subjects, P)
    db = make(tmp_path, subjects)
    assert db.lens.tolist() == [len(x) for x in subjects]
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        out = s.search_packed(db.chunk(0, len(subjects)))
        got_counters = counters(s, search.STAT_FIELDS)
        reset(s)
        ascii_ = s.search(*sc.flat(subjects))
        assert got_counters == counters(s, search.STAT_FIELDS)
    got = list(zip(*[out[f].tolist() for f in FIELDS]))
    assert got == sorted(got), "the records come back in the defined order"
    assert got == want == records(ascii_) and len(got) == n
    for f, dt in search.RECORD_FIELDS:
        assert out[f].dtype == dt


@pytest.mark.parametrize("name", sorted(gc.HAND_BUILT))
def test_hand_built_gapped_cases(name, tmp_path):
    contigs, subjects, P, n = gc.HAND_BUILT[name]()
    want = go.search_gapped_arrays(contigs, subjects, P)
    db = make(tmp_path, subjects)
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        out = s.search_gapped_packed(db.chunk(0, len(subjects)))
        got_counters = counters(s)
        assert s.stats["anchors"] == len(so.search_indexed(contigs, subjects, P))
        reset(s)
        ascii_ = s.search_gapped(*sc.flat(subjects))
        assert got_counters == counters(s)
    assert records(out, GAP_FIELDS) == want == records(ascii_, GAP_FIELDS) and len(want) == n
    for f, dt in search.GAP_RECORD_FIELDS:
        assert out[f].dtype == dt


@pytest.mark.parametrize("name", sorted(sdc.HAND_BUILT))
def test_hand_built_dust_cases(name, tmp_path):
    contigs, subjects, P, _, n_masked = sdc.HAND_BUILT[name]()
    GP = sdc.gap_params(**P)
    want = sdo.search_indexed(contigs, subjects, P)
    want_gap = sdo.search_gapped_arrays(contigs, subjects, GP, records=want)
    assert len(want) == n_masked
    db = make(tmp_path, subjects)
    ch = db.chunk(0, len(subjects))
    with search.Searcher(*sc.flat(contigs), dust=True, **kw(GP)) as s:
        assert records(s.search_packed(ch)) == want
        assert records(s.search_gapped_packed(ch), GAP_FIELDS) == want_gap
        got_counters = counters(s)
        reset(s)
        assert records(s.search(*sc.flat(subjects))) == want
        assert records(s.search_gapped(*sc.flat(subjects)), GAP_FIELDS) == want_gap
        assert got_counters == counters(s)


def run_packed(s, db, size, gapped=False):
    got = []
    for lo in range(0, db.n_subjects, size):
        ch = db.chunk(lo, min(lo + size, db.n_subjects))
        out = s.search_gapped_packed(ch) if gapped else s.search_packed(ch)
        out["subject"] = out["subject"] + np.int32(lo)
        got += records(out, GAP_FIELDS if gapped else FIELDS)
    return sorted(got)


def run_ascii(s, subjects, size, gapped=False):
    got = []
    for lo in range(0, len(subjects), size):
        flat = sc.flat(subjects[lo:lo + size])
        out = s.search_gapped(*flat) if gapped else s.search(*flat)
        out["subject"] = out["subject"] + np.int32(lo)
        got += records(out, GAP_FIELDS if gapped else FIELDS)
    return sorted(got)


def test_medium_set_however_cut(tmp_path):
    contigs, subjects, P = sc.medium()
    want = so.search_indexed(contigs, subjects, P)
    assert len(want) > 200
    db = make(tmp_path, subjects)
    assert len({int(o) & 31 for o in db.off[:-1]}) == 32             # chunks of 1 walk through every bit0
    other = [sc.rnd(500, 99)]
    with search.Searcher(*sc.flat(other), **kw(P)) as s:
        assert run_packed(s, make(tmp_path, subjects[:20], "first20"), 20) == \
            so.search_indexed(other, subjects[:20], P)
        s.index(*sc.flat(contigs))                                   # the index is replaced
        reset(s)
        for _ in range(2):                                           # twice over
            assert run_packed(s, db, db.n_subjects) == want
            assert run_packed(s, db, 7) == want
            assert run_packed(s, db, 1) == want
        assert s.stats["seed_hits"] > 0 and s.stats["raw_hsps"] + s.stats["seeds_skipped"] == s.stats["seed_hits"]
        packed_hits = s.stats["seed_hits"]
        reset(s)
        assert run_ascii(s, subjects, 7) == want                     # ASCII after packed
        assert run_packed(s, db, 7) == want                          # packed after ASCII
        assert 6 * s.stats["seed_hits"] == 2 * packed_hits           # chunking and form leave the counters alone


def test_medium_gapped_set_however_cut(tmp_path):
    contigs, subjects, P = gc.medium()
    want = go.search_gapped_arrays(contigs, subjects, P)
    ungapped = so.search_indexed(contigs, subjects, P)
    assert len(want) > 150
    db = make(tmp_path, subjects)
    other = [sc.rnd(500, 99)]
    with search.Searcher(*sc.flat(other), **kw(P)) as s:
        assert run_packed(s, make(tmp_path, subjects[:20], "first20"), 20, True) == \
            go.search_gapped_arrays(other, subjects[:20], P)
        s.index(*sc.flat(contigs))                                   # the index is replaced
        reset(s)
        for _ in range(2):
            assert run_packed(s, db, db.n_subjects, True) == want
            assert run_packed(s, db, 7, True) == want
            assert run_packed(s, db, 1, True) == want
        assert s.stats["anchors"] == 6 * len(ungapped)
        assert run_ascii(s, subjects, 7, True) == want               # ASCII after packed
        assert run_packed(s, db, 7, True) == want                    # packed after ASCII
        assert run_packed(s, db, 7) == ungapped                      # and the ungapped call between gapped ones
        assert run_packed(s, db, db.n_subjects, True) == want


def test_search_chunk_halves_on_the_device(tmp_path, monkeypatch):
    """search_chunk on the device: a searcher whose packed call refuses more than 3 subjects
    gives the records of the whole chunk."""
    contigs, subjects, P = sc.medium()
    subjects = subjects[:40]
    want = so.search_indexed(contigs, subjects, P)
    db = make(tmp_path, subjects)
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        real = s.search_packed

        def refusing(chunk, params=None):
            if len(chunk.off) - 1 > 3:
                raise lib.WaafleHipError(lib.WF_E_TOOBIG, "more than 3 subjects")
            return real(chunk, params)

        monkeypatch.setattr(s, "search_packed", refusing)
        assert records(search.search_chunk(s, db.chunk(0, 40))) == want


# ---------------------------------------------------------------------------
# the capacity protocol and the checks
# ---------------------------------------------------------------------------

def test_capacity_one_then_room(tmp_path):
    contigs, subjects, P, n = sc.run_28_all_phases()
    want = so.search_indexed(contigs, subjects, P)
    assert len(want) == n >= 3
    ch = make(tmp_path, subjects).chunk(0, len(subjects))
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        rc, full, out = s.search_packed_once(ch, 1)
        assert rc == lib.WF_E_NOMEM and full == n
        assert records(out) == want[:1]
        rc, full, out = s.search_packed_once(ch, n)
        assert rc == lib.WF_OK and full == n and records(out) == want
        s.capacity = 1                                               # the wrapper grows on its own
        assert records(s.search_packed(ch)) == want


def test_capacity_one_then_room_gapped(tmp_path):
    contigs, subjects, P, n = gc.refill_gaps()
    want = go.search_gapped_arrays(contigs, subjects, P)
    assert len(want) == n >= 3
    ch = make(tmp_path, subjects).chunk(0, len(subjects))
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        rc, full, out = s.search_gapped_packed_once(ch, 1)
        assert rc == lib.WF_E_NOMEM and full == n
        assert records(out, GAP_FIELDS) == want[:1]
        s.capacity = 1
        assert records(s.search_gapped_packed(ch), GAP_FIELDS) == want


def _rc(s, gapped=False, **fields):
    """the status of one packed call whose subjects struct is given field by field"""
    sb = lib.WfSearchPackedSubjects(**fields)
    if gapped:
        out = {f: np.zeros(8, dt) for f, dt in search.GAP_RECORD_FIELDS}
        r = lib.WfSearchGapResult(capacity=8, **{f: lib.ptr(out[f]) for f in GAP_FIELDS})
        return s.so.wf_search_gapped_packed(s.h, C.byref(sb), C.byref(s.params), C.byref(s.gap_params), C.byref(r))
    out = {f: np.zeros(8, dt) for f, dt in search.RECORD_FIELDS}
    r = lib.WfSearchResult(capacity=8, **{f: lib.ptr(out[f]) for f in FIELDS})
    return s.so.wf_search_packed(s.h, C.byref(sb), C.byref(s.params), C.byref(r))


def test_argument_checks(tmp_path):
    contigs, subjects, P, _ = sc.minus_strand()
    db = make(tmp_path, [sc.rnd(37, 1)] + list(subjects))
    ch = db.chunk(1, 2)
    assert ch.bit0 == 5
    total, words = int(ch.off[-1]), len(ch.lo)
    good = dict(n_subjects=1, off=lib.ptr(ch.off), lo=lib.ptr(ch.lo), hi=lib.ptr(ch.hi), nn=lib.ptr(ch.nn),
                n_words=words, bit0=ch.bit0)
    with search.Searcher(*sc.flat(contigs), **kw(P)) as s:
        with pytest.raises(lib.WaafleHipError) as exc:               # nothing has been searched yet
            s.chunk_planes(total, 0)
        assert exc.value.code == lib.WF_E_STATE
        for gapped in (False, True):
            assert _rc(s, gapped, **good) == lib.WF_OK
            for change in (dict(bit0=-1), dict(bit0=32), dict(lo=None), dict(hi=None), dict(nn=None),
                           dict(n_words=words + 1), dict(n_words=words - 1), dict(n_words=0), dict(off=None),
                           dict(n_subjects=-1)):
                assert _rc(s, gapped, **dict(good, **change)) == lib.WF_E_BADINPUT, (gapped, change)
            p = lib.WfSearchParams.from_buffer_copy(s.params)        # the shared parameter checks
            p.stride = 0
            with pytest.raises(lib.WaafleHipError) as exc:
                s.search_gapped_packed(ch, params=p) if gapped else s.search_packed(ch, params=p)
            assert exc.value.code == lib.WF_E_BADINPUT
            # too big: refused before a plane is read (the three planes here are one word each)
            big = np.array([0, (1 << 30) + 1], np.int64)
            word = np.zeros(1, np.uint32)
            assert _rc(s, gapped, n_subjects=1, off=lib.ptr(big), lo=lib.ptr(word), hi=lib.ptr(word),
                       nn=lib.ptr(word), n_words=((1 << 30) + 1 + 31) // 32, bit0=0) == lib.WF_E_TOOBIG
            assert _rc(s, gapped, n_subjects=1, off=lib.ptr(big), lo=None, hi=None, nn=None, n_words=0,
                       bit0=0) == lib.WF_E_TOOBIG
        assert len(s.search_packed(ch)["contig"]) == 1               # still usable
        assert len(s.search_gapped_packed(ch)["contig"]) == 1
        lo, hi, nn = s.chunk_planes(total, 1)
        assert len(lo) == (total + 31) // 32 + 2
        for bad in (dict(strand=2), dict(strand=-1), dict(words=len(lo) + 1), dict(lo=None)):
            a = dict(dict(strand=0, lo=lib.ptr(lo), hi=lib.ptr(hi), nn=lib.ptr(nn), words=len(lo)), **bad)
            assert s.so.wf_search_chunk_planes(s.h, a["strand"], a["lo"], a["hi"], a["nn"], a["words"]) == \
                lib.WF_E_BADINPUT, bad
        s.search(*sc.flat(["ACGT"]))                                 # no seed slot: no chunk stays resident
        with pytest.raises(lib.WaafleHipError) as exc:
            s.chunk_planes(4, 0)
        assert exc.value.code == lib.WF_E_STATE
    h = C.c_void_p()
    dll = lib.load()
    assert dll.wf_init(0, C.byref(h)) == lib.WF_OK                   # a fresh context: no index, no chunk
    try:
        w = np.zeros(4, np.uint32)
        assert dll.wf_search_chunk_planes(h, 0, lib.ptr(w), lib.ptr(w), lib.ptr(w), 4) == lib.WF_E_STATE
        sb = lib.WfSearchPackedSubjects(**good)
        out = {f: np.zeros(4, dt) for f, dt in search.RECORD_FIELDS}
        r = lib.WfSearchResult(capacity=4, **{f: lib.ptr(out[f]) for f in FIELDS})
        p = lib.WfSearchParams(seed_len=21, stride=8, max_occ=64, xdrop=20, min_score=28)
        assert dll.wf_search_packed(h, C.byref(sb), C.byref(p), C.byref(r)) == lib.WF_E_STATE
    finally:
        dll.wf_free(h)


# ---------------------------------------------------------------------------
# the command line
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


@pytest.mark.parametrize("flags", [(), ("--gapped",), ("--dust", "--dust-out", "DUST")])
def test_cli_tables_are_byte_identical(tmp_path, flags):
    contigs, subjects, paths = _sample(tmp_path)
    wfdb = str(tmp_path / "genes.wfdb")
    run = subprocess.run([sys.executable, "-m", "waafle_amd.makedb", paths[4], "--out", wfdb], capture_output=True,
                         text=True, timeout=300, cwd=REPO)
    assert run.returncode == 0, run.stderr[-2000:]
    assert search.PackedDb(wfdb).n_subjects == len(subjects)
    tables = []
    for tag, db in (("fasta", paths[4]), ("wfdb", wfdb)):
        out = str(tmp_path / (tag + ".blastout"))
        extra = [str(tmp_path / (tag + ".dust.tsv")) if f == "DUST" else f for f in flags]
        run = subprocess.run([sys.executable, "-m", "waafle_amd.search", paths[0], db, "--searcher", "native",
                              "--out", out, "--chunk-bases", "1200"] + extra, capture_output=True, text=True,
                             timeout=300, cwd=REPO)
        assert run.returncode == 0, run.stderr[-2000:]
        tables.append(open(out, "rb").read())
        if "DUST" in flags:
            tables.append(open(str(tmp_path / (tag + ".dust.tsv")), "rb").read())
    half = len(tables) // 2
    assert tables[:half] == tables[half:]
    assert tables[0].count(b"\n") >= 12
    if not flags:                                                    # and they are the oracle's table
        recs = so.search_indexed([s for _, s in contigs], [s for _, s in subjects], so.DEFAULTS)
        want = so.rows(recs, [n for n, _ in contigs], [len(s) for _, s in contigs], [n for n, _ in subjects],
                       [len(s) for _, s in subjects], sum(len(s) for _, s in subjects))
        assert tables[0].decode() == "".join(r + "\n" for r in want)
