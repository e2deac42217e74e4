"""CPU oracles of the homology-search rule, written from the rule's text.

Two independent forms:
  search_brute    every seed offset compared with every contig position by string comparison,
                  the extension walked column by column
  search_indexed  a dictionary of the contigs' S-mers, the extension from cumulative sums

Both return the sorted list of records (contig, subject, minus, qstart, sstart, length,
matches), all 0-based; sstart counts on the variant (the subject, or its reverse complement
when minus).  P: dict(S, T, max_occ, X, min_score).  `rows` renders the 15-column table.
"""
import math

import numpy as np

DEFAULTS = dict(S=21, T=8, max_occ=64, X=20, min_score=28)
LAMBDA, K = 1.28, 0.46
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def norm(s):
    return "".join(ch if ch in "ACGT" else "N" for ch in s.upper())


def revcomp(s):
    return "".join(_COMP[ch] for ch in reversed(s))


def _variants(subject):
    x = norm(subject)
    return ((0, x), (1, revcomp(x)))


def _report(hsps, P):
    """hsps: set of (minus, subject, contig, delta, b, e, matches) -> sorted records."""
    groups = {}
    for h in hsps:
        groups.setdefault(h[:4], set()).add(h[4:])
    out = []
    for (minus, g, c, delta), ivs in groups.items():
        for b, e, m in ivs:
            if any((b2, e2) != (b, e) and b2 <= b and e <= e2 for b2, e2, _ in ivs):
                continue
            length = e - b
            if m - 2 * (length - m) >= P["min_score"]:
                out.append((c, g, minus, b + delta, b, length, m))
    return sorted(out)


def _col(x, s, i, delta):
    return 1 if x[i] == s[i + delta] and x[i] != "N" else -2


def _extend_walk(x, s, delta, a, S, X):
    M, n = len(x), len(s)
    r = best = 0
    e = a + S
    i = a + S
    while i < M and i + delta < n:
        r += _col(x, s, i, delta)
        if r > best:
            best, e = r, i + 1
        if best - r > X:
            break
        i += 1
    r = best = 0
    b = a
    i = a - 1
    while i >= 0 and i + delta >= 0:
        r += _col(x, s, i, delta)
        if r > best:
            best, b = r, i
        if best - r > X:
            break
        i -= 1
    return b, e


def search_brute(contigs, subjects, P):
    S, T = P["S"], P["T"]
    cs = [norm(c) for c in contigs]
    hsps = set()
    for g, subj in enumerate(subjects):
        for minus, x in _variants(subj):
            for a in range(0, len(x) - S + 1, T):
                seed = x[a:a + S]
                if "N" in seed:
                    continue
                occ = [(c, q) for c, s in enumerate(cs) for q in range(len(s) - S + 1) if s[q:q + S] == seed]
                if not occ or len(occ) > P["max_occ"]:
                    continue
                for c, q in occ:
                    delta = q - a
                    b, e = _extend_walk(x, cs[c], delta, a, S, P["X"])
                    m = sum(1 for i in range(b, e) if _col(x, cs[c], i, delta) == 1)
                    hsps.add((minus, g, c, delta, b, e, m))
    return _report(hsps, P)


def _codes(s):
    """A0 C1 G2 T3 N4 as an int8 array."""
    lut = np.full(256, 4, np.int8)
    for k, ch in enumerate("ACGT"):
        lut[ord(ch)] = k
    return lut[np.frombuffer(s.encode(), np.uint8)]


def _side(sc, X):
    """Columns walked in order with scores sc: how many belong to the extension."""
    if len(sc) == 0:
        return 0
    r = np.cumsum(sc)
    best = np.maximum(np.maximum.accumulate(r), 0)
    stop = np.flatnonzero(best - r > X)
    upto = stop[0] + 1 if len(stop) else len(sc)
    r = r[:upto]
    top = r.max()
    return int(np.argmax(r)) + 1 if top > 0 else 0       # the first (shortest) of equal bests


def search_indexed(contigs, subjects, P):
    S, T, X = P["S"], P["T"], P["X"]
    cs = [norm(c) for c in contigs]
    cc = [_codes(c) for c in cs]
    table = {}
    for c, s in enumerate(cs):
        for q in range(len(s) - S + 1):
            w = s[q:q + S]
            if "N" not in w:
                table.setdefault(w, []).append((c, q))
    hsps = set()
    for g, subj in enumerate(subjects):
        for minus, x in _variants(subj):
            xc = _codes(x)
            M = len(x)
            for a in range(0, M - S + 1, T):
                occ = table.get(x[a:a + S], ())
                if len(occ) > P["max_occ"]:
                    continue
                for c, q in occ:
                    delta = q - a
                    lo, hi = max(0, -delta), min(M, len(cs[c]) - delta)
                    xs, ss = xc[lo:hi], cc[c][lo + delta:hi + delta]
                    sc = np.where((xs == ss) & (xs < 4), 1, -2).astype(np.int64)
                    e = a + S + _side(sc[a + S - lo:], X)
                    b = a - _side(sc[:a - lo][::-1], X)
                    m = int((sc[b - lo:e - lo] == 1).sum())
                    hsps.add((minus, g, c, delta, b, e, m))
    return _report(hsps, P)


# ---------------------------------------------------------------------------
# the 15-column table
# ---------------------------------------------------------------------------

def bitscore(score):
    return (LAMBDA * score - math.log(K)) / math.log(2)


def bitscore_text(score):
    bits = bitscore(score)
    return str(int(bits)) if bits > 99.9 else "%.1f" % bits


def rows(records, contig_names, contig_lens, subject_ids, subject_lens, db_bases, max_target_seqs=10000):
    """The table's lines: by contig; within a contig the subjects past --max-target-seqs (ranked
    by (-best score, subject)) lose their rows, the rest go by (-score, subject, minus, qstart,
    sstart)."""
    per = {}
    for c, g, minus, qs, ss, length, m in records:
        per.setdefault(c, []).append((-(m - 2 * (length - m)), g, minus, qs, ss, length, m))
    out = []
    for c in sorted(per):
        best = {}
        for r in per[c]:
            best[r[1]] = min(best.get(r[1], 0), r[0])
        keep = set(g for _, g in sorted((v, g) for g, v in best.items())[:max_target_seqs])
        for neg, g, minus, qs, ss, length, m in sorted(per[c]):
            if g not in keep:
                continue
            score, M = -neg, subject_lens[g]
            s0, s1 = (M - ss, M - ss - length + 1) if minus else (ss + 1, ss + length)
            ev = K * contig_lens[c] * db_bases * math.exp(-LAMBDA * score)
            out.append("\t".join(str(v) for v in (
                contig_names[c], subject_ids[g], contig_lens[c], M, length, qs + 1, qs + length, s0, s1,
                "%.3f" % (100.0 * m / length), m, 0, "%.2e" % ev, bitscore_text(score),
                "minus" if minus else "plus")))
    return out
