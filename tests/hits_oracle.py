"""Two independently written CPU forms of the record-to-hit rule.

Form A is the definition: the records are written as the table (search.format_rows) and read
back by the Python reader (inputs._load_python); no GPU and no native library takes part.
Form B is the arithmetic of §13 itself, with fractions.Fraction for the exact product of the
pident rounding: no fma and none of Form A's strings.

A case is a dict: contig_names, qlen, subject_ids, slen, edges [(child, parent)], min_scov and
cols {column: list} (the nine columns of wf_hit_records, sorted by contig)."""
import os
import tempfile
from fractions import Fraction

import numpy as np

from waafle_amd import inputs, lib, search

COLUMNS = ("contig", "subject", "minus", "qstart", "qspan", "sstart", "sspan", "length", "matches")
FIELDS = ("hit_off", "hit_qlo", "hit_qhi", "hit_taxon", "hit_strand", "hit_score", "hit_scov", "hit_sysmask",
          "hit_key")


def bits(a):
    """An array as integers: doubles as their int64 bit patterns."""
    a = np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_same(got, want, what=""):
    for f in FIELDS:
        g, w = np.asarray(got[f]), np.asarray(want[f])
        assert g.dtype == w.dtype, (what, f, g.dtype, w.dtype)
        assert g.shape == w.shape, (what, f, g.shape, w.shape)
        bad = np.flatnonzero(bits(g) != bits(w))
        assert len(bad) == 0, (what, f, len(bad), int(bad[0]), g[bad[0]], w[bad[0]])


def form_a(case):
    """{field: array} through the table and its Python reader."""
    cols = {f: np.asarray(case["cols"][f], np.int64) for f in COLUMNS}
    n = len(cols["contig"])
    ungapped = bool(np.all(cols["qspan"] == cols["length"]) and np.all(cols["sspan"] == cols["length"]))
    rec = {f: cols[f] for f in COLUMNS}
    if not ungapped:
        rec["gaps"] = np.zeros(n, np.int64)
    rows = search.format_rows(rec, np.arange(n), case["contig_names"], case["qlen"], case["subject_ids"],
                              case["slen"], int(sum(case["slen"])))
    with tempfile.TemporaryDirectory() as tmp:
        fna, table, gff = (os.path.join(tmp, x) for x in ("c.fna", "c.blastout", "c.gff"))
        with open(fna, "w") as fh:
            for name, length in zip(case["contig_names"], case["qlen"]):
                fh.write(">{}\n{}\n".format(name, "A" * int(length)))
        with open(table, "w") as fh:
            fh.write("".join(r + "\n" for r in rows))
        open(gff, "w").close()
        batch, tax = inputs._load_python(fna, table, gff, list(case["edges"]), 200.0, None)
    out = {f: getattr(batch, f) for f in FIELDS[:-1]}
    out["hit_key"] = lib.pack_hit_keys(batch.hit_taxon, batch.hit_strand, batch.hit_scov, batch.hit_sysmask,
                                       case["min_scov"])
    return out


def pident_b(matches, length):
    x = (100.0 * matches) / length
    return round(Fraction(x) * 1000) / 1000.0          # round(Fraction): nearest, ties to even


def form_b(case):
    """{field: array} by the arithmetic of §13."""
    c = {f: np.asarray(case["cols"][f], np.int64).tolist() for f in COLUMNS}
    n = len(c["contig"])
    used = sorted(set(c["subject"]))
    parts = {g: case["subject_ids"][g].split("|") for g in used}
    names = {"r__Root", "Unknown"} | {p[1] for p in parts.values()}
    for child, parent in case["edges"]:
        names |= {child, parent}
    rank = {nm: i for i, nm in enumerate(sorted(names))}
    systems = sorted({kv.split("=")[0] for p in parts.values() for kv in p[2:]})
    mask = {g: sum(1 << systems.index(kv.split("=")[0]) for kv in set(p[2:])) for g, p in parts.items()}
    out = {"hit_off": np.array([sum(1 for x in c["contig"] if x < k) for k in range(len(case["qlen"]) + 1)],
                               np.int64) if n < 5000 else
           np.searchsorted(np.asarray(c["contig"]), np.arange(len(case["qlen"]) + 1), side="left").astype(np.int64)}
    qlo, qhi, taxon, strand, score, scov_l, sysmask, key = ([] for _ in range(8))
    for i in range(n):
        g = c["subject"][i]
        qlen, slen = int(case["qlen"][c["contig"][i]]), int(case["slen"][g])
        q1 = c["qstart"][i] + 1
        s0, s1 = c["sstart"][i] + 1, c["sstart"][i] + c["sspan"][i]
        ltrim = max(0, s0 - q1)
        rtrim = max(0, slen - s0 - qlen + q1)
        scov = float(s1 - s0 + 1) / float(slen - ltrim - rtrim)
        pident = pident_b(c["matches"][i], c["length"][i])
        t, m, minus = rank[parts[g][1]], mask[g], int(c["minus"][i])
        qlo.append(q1)
        qhi.append(c["qstart"][i] + c["qspan"][i])
        taxon.append(t)
        strand.append(minus)
        scov_l.append(scov)
        score.append(scov * pident / 100.0)
        sysmask.append(m)
        key.append(t | (1 << 24 if scov >= case["min_scov"] else 0) | minus << 25 | (m & 63) << 26)
    out.update(hit_qlo=np.array(qlo, np.int32), hit_qhi=np.array(qhi, np.int32), hit_taxon=np.array(taxon, np.int32),
               hit_strand=np.array(strand, np.int8), hit_score=np.array(score, np.float64),
               hit_scov=np.array(scov_l, np.float64), hit_sysmask=np.array(sysmask, np.uint32),
               hit_key=np.array(key, np.uint32))
    return out
