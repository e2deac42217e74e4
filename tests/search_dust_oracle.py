"""CPU oracles of the homology-search rule with a low-complexity mask (DESIGN.md §12.1 and
§12.5 as extended by §12.6), written from the rule's text: the index holds only the contigs'
S-mers whose S bases are all unmasked, max_occ counts those occurrences only, and everything
else (the extensions, which run through masked stretches, the report) is as without a mask.

Two independent forms, as in search_oracle:
  search_brute    every seed offset against every contig position by string comparison, an
                  occurrence dropped when the brute-force mask covers one of its bases
  search_indexed  a dictionary of the unmasked S-mers, by the array form of the mask
and for the gapped rule search_gapped_cells / search_gapped_arrays of search_gap_oracle, with
the masked records as anchors.

P: the rule's dict plus Wd and Lv (and W, Xg for the gapped forms).
"""
import numpy as np

import dust_oracle as do
import search_gap_oracle as go
import search_oracle as so

DEFAULTS = dict(so.DEFAULTS, **do.DEFAULTS)
GAP_DEFAULTS = dict(go.GAP_DEFAULTS, **do.DEFAULTS)


def _split(flat, contigs):
    out, base = [], 0
    for c in contigs:
        out.append(flat[base:base + len(c)])
        base += len(c)
    return out


def search_brute(contigs, subjects, P):
    S, T = P["S"], P["T"]
    cs = [so.norm(c) for c in contigs]
    masks = _split(do.mask_brute(contigs, P["Wd"], P["Lv"]), contigs)
    hsps = set()
    for g, subj in enumerate(subjects):
        for minus, x in so._variants(subj):
            for a in range(0, len(x) - S + 1, T):
                seed = x[a:a + S]
                if "N" in seed:
                    continue
                occ = [(c, q) for c, s in enumerate(cs) for q in range(len(s) - S + 1)
                       if s[q:q + S] == seed and not any(masks[c][k] for k in range(q, q + S))]
                if not occ or len(occ) > P["max_occ"]:
                    continue
                for c, q in occ:
                    delta = q - a
                    b, e = so._extend_walk(x, cs[c], delta, a, S, P["X"])
                    m = sum(1 for i in range(b, e) if so._col(x, cs[c], i, delta) == 1)
                    hsps.add((minus, g, c, delta, b, e, m))
    return so._report(hsps, P)


def search_indexed(contigs, subjects, P):
    S, T, X = P["S"], P["T"], P["X"]
    cs = [so.norm(c) for c in contigs]
    cc = [so._codes(c) for c in cs]
    masks = _split(do.mask_windows(contigs, P["Wd"], P["Lv"]), contigs)
    table = {}
    for c, s in enumerate(cs):
        covered = np.concatenate([[0], np.cumsum(masks[c])])     # masked bases before q
        for q in range(len(s) - S + 1):
            w = s[q:q + S]
            if "N" not in w and covered[q + S] == covered[q]:
                table.setdefault(w, []).append((c, q))
    hsps = set()
    for g, subj in enumerate(subjects):
        for minus, x in so._variants(subj):
            xc = so._codes(x)
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
                    e = a + S + so._side(sc[a + S - lo:], X)
                    b = a - so._side(sc[:a - lo][::-1], X)
                    m = int((sc[b - lo:e - lo] == 1).sum())
                    hsps.add((minus, g, c, delta, b, e, m))
    return so._report(hsps, P)


def rows(records, *args, **kw):
    return so.rows(records, *args, **kw)


# ---------------------------------------------------------------------------
# gapped: the masked records are the anchors
# ---------------------------------------------------------------------------

def anchors(records):
    """(contig, subject, minus, i0, j0) of every ungapped record."""
    out = []
    for c, g, minus, qs, ss, length, _ in records:
        i0 = ss + length // 2
        out.append((c, g, minus, i0, i0 + (qs - ss)))
    return out


def search_gapped_cells(contigs, subjects, P):
    cs = [so.norm(c) for c in contigs]
    var = [[so.norm(s), so.revcomp(so.norm(s))] for s in subjects]
    alns = set()
    for c, g, minus, i0, j0 in anchors(search_brute(contigs, subjects, P)):
        x, s = var[g][minus], cs[c]
        right = go.extend_cells(x[i0:], s[j0:], P["W"], P["Xg"])
        left = go.extend_cells(x[:i0][::-1], s[:j0][::-1], P["W"], P["Xg"])
        alns.add((minus, g, c) + go._alignment(i0, j0, left, right))
    return go._report_walk(alns, P)


def search_gapped_arrays(contigs, subjects, P, records=None):
    """records: the ungapped masked records when the caller has them already."""
    cc = [so._codes(so.norm(c)) for c in contigs]
    var = [[so._codes(so.norm(s)), so._codes(so.revcomp(so.norm(s)))] for s in subjects]
    anc = anchors(search_indexed(contigs, subjects, P) if records is None else records)
    right = go.extend_arrays([(var[g][minus][i0:], cc[c][j0:]) for c, g, minus, i0, j0 in anc], P["W"], P["Xg"])
    left = go.extend_arrays([(var[g][minus][:i0][::-1], cc[c][:j0][::-1]) for c, g, minus, i0, j0 in anc],
                            P["W"], P["Xg"])
    found = {}
    for (c, g, minus, i0, j0), (hr, pr, qr, nr, mr, gr), (hl, pl, ql, nl, ml, gl) in zip(anc, right, left):
        rec = (j0 - ql, ql + qr, i0 - pl, pl + pr, nl + nr, ml + mr, gl + gr)
        found.setdefault((c, g, minus), {})[rec] = hl + hr          # identical ones once
    out = []
    for key, recs in found.items():
        kept = []
        for r in sorted(recs, key=lambda r: (-recs[r],) + r):
            if any(k[0] <= r[0] and r[0] + r[1] <= k[0] + k[1] and k[2] <= r[2] and r[2] + r[3] <= k[2] + k[3]
                   for k in kept):
                continue
            kept.append(r)
            if recs[r] >= 2 * P["min_score"]:
                out.append(key + r)
    return sorted(out)
