"""CPU oracles of the gapped extension of the homology search, written from
the rule's text.  The anchors are the records of search_oracle.search_indexed.

Two independent forms:
  search_gapped_cells   scalar, over a dictionary of cells; every cell carries (H, g) and
                        length and matches come from the rule's closed forms
  search_gapped_arrays  numpy arrays per anti-diagonal (one slot per band diagonal, one row
                        per anchor, all anchors at once); the predecessor choices are kept and
                        length, matches and gaps come from an explicit traceback from the best
                        cell

Both return the sorted list of records (contig, subject, minus, qstart, qspan, sstart, sspan,
length, matches, gaps), all 0-based; sstart counts on the variant.  P: the ungapped rule's
dict plus W (band half-width) and Xg (gapped x-drop, raw score).  `rows` renders the table.
"""
import math

import numpy as np

import search_oracle as so

GAP_DEFAULTS = dict(so.DEFAULTS, W=15, Xg=30)
MATCH, MISMATCH, GAP = 2, -4, -5                 # half units
FIELDS = ("contig", "subject", "minus", "qstart", "qspan", "sstart", "sspan", "length", "matches", "gaps")


def score2_of(rec):
    """From a record: 2 per match, -4 per mismatch, -5 per gap column."""
    length, m, g = rec[7], rec[8], rec[9]
    return MATCH * m + MISMATCH * (length - g - m) + GAP * g


def anchors(contigs, subjects, P):
    """(contig, subject, minus, i0, j0) of every ungapped record, in the records' order."""
    out = []
    for c, g, minus, qs, ss, length, _ in so.search_indexed(contigs, subjects, P):
        i0 = ss + length // 2
        out.append((c, g, minus, i0, i0 + (qs - ss)))
    return out


# ---------------------------------------------------------------------------
# form 1: a dictionary of cells
# ---------------------------------------------------------------------------

def extend_cells(u, v, W, Xg):
    """(H, p, q, g) of the best live cell of the banded x-drop extension over u and v."""
    nu, nv = len(u), len(v)
    live = {(0, 0): (0, 0)}
    best = 0                                     # over the anti-diagonals before k
    res = (0, 0, 0, 0)
    empty = 0
    for k in range(1, nu + nv + 1):
        found = []
        for p in range(max(0, k - nv), min(nu, k) + 1):
            q = k - p
            if abs(q - p) > W:
                continue
            cands = []
            if (p - 1, q - 1) in live:
                h, g = live[(p - 1, q - 1)]
                same = u[p - 1] == v[q - 1] and u[p - 1] != "N"
                cands.append((h + (MATCH if same else MISMATCH), g))
            if (p - 1, q) in live:
                h, g = live[(p - 1, q)]
                cands.append((h + GAP, g + 1))
            if (p, q - 1) in live:
                h, g = live[(p, q - 1)]
                cands.append((h + GAP, g + 1))
            if not cands:
                continue
            top = max(h for h, _ in cands)
            h, g = next(c for c in cands if c[0] == top)     # the first of equal ones
            if best - h > 2 * Xg:
                continue
            found.append((p, q, h, g))
        for p, q, h, g in found:                 # p ascending
            live[(p, q)] = (h, g)
            if h > res[0]:
                res = (h, p, q, g)
        if found:
            best = max(best, max(f[2] for f in found))
            empty = 0
        else:
            empty += 1
            if empty == 2:
                break
    return res


def _alignment(i0, j0, left, right):
    (hl, pl, ql, gl), (hr, pr, qr, gr) = left, right
    sspan, qspan, gaps, score2 = pl + pr, ql + qr, gl + gr, hl + hr
    assert (sspan + qspan - gaps) % 2 == 0
    A = (sspan + qspan - gaps) // 2
    assert (score2 + 5 * gaps + 4 * A) % 6 == 0
    return (j0 - ql, qspan, i0 - pl, sspan, A + gaps, (score2 + 5 * gaps + 4 * A) // 6, gaps)


def _report_walk(alns, P):
    """alns: set of (minus, subject, contig, qstart, qspan, sstart, sspan, length, matches, gaps)."""
    groups = {}
    for a in alns:
        groups.setdefault(a[:3], set()).add(a[3:])
    out = []
    for (minus, g, c), rest in groups.items():
        kept = []
        for r in sorted(rest, key=lambda r: (-score2_of((0, 0, 0) + r),) + r):
            qs, qn, ss, sn = r[:4]
            if any(k[0] <= qs and qs + qn <= k[0] + k[1] and k[2] <= ss and ss + sn <= k[2] + k[3] for k in kept):
                continue
            kept.append(r)
        out += [(c, g, minus) + r for r in kept if score2_of((0, 0, 0) + r) >= 2 * P["min_score"]]
    return sorted(out)


def search_gapped_cells(contigs, subjects, P):
    cs = [so.norm(c) for c in contigs]
    var = [[so.norm(s), so.revcomp(so.norm(s))] for s in subjects]
    alns = set()
    for c, g, minus, i0, j0 in anchors(contigs, subjects, P):
        x, s = var[g][minus], cs[c]
        right = extend_cells(x[i0:], s[j0:], P["W"], P["Xg"])
        left = extend_cells(x[:i0][::-1], s[:j0][::-1], P["W"], P["Xg"])
        alns.add((minus, g, c) + _alignment(i0, j0, left, right))
    return _report_walk(alns, P)


# ---------------------------------------------------------------------------
# form 2: arrays per anti-diagonal, explicit traceback
# ---------------------------------------------------------------------------

_DEAD = -(1 << 40)


def extend_arrays(pairs, W, Xg):
    """pairs: (u, v) int8 code arrays (N = 4), all extended at once: one row per pair, one slot
    per band diagonal.  Per pair (H, p, q, columns, matches, gaps) of the best live cell, the
    last three counted along the traced path."""
    B = len(pairs)
    if B == 0:
        return []
    n = 2 * W + 3                                # slot d + W + 1; a dead slot at either edge
    d = np.arange(n) - W - 1
    inband = np.abs(d) <= W
    nu = np.array([len(u) for u, _ in pairs])
    nv = np.array([len(v) for _, v in pairs])
    U = np.full((B, nu.max() + 1), 5, np.int8)   # the padding matches nothing
    V = np.full((B, nv.max() + 1), 6, np.int8)
    for b, (u, v) in enumerate(pairs):
        U[b, :len(u)] = u
        V[b, :len(v)] = v
    dead = np.full((B, n), _DEAD, np.int64)
    h1 = dead.copy()                             # anti-diagonal k - 1
    h1[:, W + 1] = 0
    h2 = dead                                    # k - 2
    choice = [np.zeros((B, n), np.int8)]
    best = np.zeros(B, np.int64)
    top_h, top_k, top_slot = np.zeros(B, np.int64), np.zeros(B, np.int64), np.full(B, W + 1)
    for k in range(1, int((nu + nv).max()) + 1):
        p = (k - d) // 2
        q = k - p
        cell = inband & ((k - d) % 2 == 0) & (p >= 0) & (q >= 0)
        ok = cell[None, :] & (p[None, :] <= nu[:, None]) & (q[None, :] <= nv[:, None])
        uu = U[:, np.clip(p - 1, 0, U.shape[1] - 1)]
        vv = V[:, np.clip(q - 1, 0, V.shape[1] - 1)]
        cd = np.where(h2 > _DEAD, h2 + np.where((uu == vv) & (uu < 4), MATCH, MISMATCH), _DEAD)
        cu = dead.copy()                         # from (p - 1, q): the slot above
        cu[:, :-1] = np.where(h1[:, 1:] > _DEAD, h1[:, 1:] + GAP, _DEAD)
        cl = dead.copy()                         # from (p, q - 1): the slot below
        cl[:, 1:] = np.where(h1[:, :-1] > _DEAD, h1[:, :-1] + GAP, _DEAD)
        stack = np.stack([cd, cu, cl])
        ch = np.argmax(stack, axis=0)            # the first of equal ones
        h = np.take_along_axis(stack, ch[None], 0)[0]
        alive = ok & (h > _DEAD) & (best[:, None] - h <= 2 * Xg)
        hk = np.where(alive, h, _DEAD)
        choice.append(np.where(alive, ch + 1, 0).astype(np.int8))
        m = hk.max(axis=1)
        better = m > top_h                       # a later anti-diagonal must be greater
        # of equal cells of one anti-diagonal the smallest p, that is the greatest slot
        last = n - 1 - np.argmax((hk == m[:, None])[:, ::-1], axis=1)
        top_h, top_k, top_slot = np.where(better, m, top_h), np.where(better, k, top_k), np.where(better, last, top_slot)
        best = np.maximum(best, m)
        if not alive.any() and not (h1 > _DEAD).any():
            break
        h2, h1 = h1, hk
    out = []
    for b, (u, v) in enumerate(pairs):
        k, slot = int(top_k[b]), int(top_slot[b])
        pb, qb = (k - int(d[slot])) // 2, (k + int(d[slot])) // 2
        cols = matches = gaps = 0
        while k > 0:
            ch = int(choice[k][b, slot])
            assert ch in (1, 2, 3)
            pp, qq = (k - int(d[slot])) // 2, (k + int(d[slot])) // 2
            cols += 1
            if ch == 1:
                matches += int(u[pp - 1] == v[qq - 1] and u[pp - 1] < 4)
                k -= 2
            else:
                gaps += 1
                k -= 1
                slot += 1 if ch == 2 else -1
        assert slot == W + 1
        out.append((int(top_h[b]), pb, qb, cols, matches, gaps))
    return out


def search_gapped_arrays(contigs, subjects, P):
    cc = [so._codes(so.norm(c)) for c in contigs]
    var = [[so._codes(so.norm(s)), so._codes(so.revcomp(so.norm(s)))] for s in subjects]
    anc = anchors(contigs, subjects, P)
    right = extend_arrays([(var[g][minus][i0:], cc[c][j0:]) for c, g, minus, i0, j0 in anc], P["W"], P["Xg"])
    left = extend_arrays([(var[g][minus][:i0][::-1], cc[c][:j0][::-1]) for c, g, minus, i0, j0 in anc], P["W"], P["Xg"])
    found = {}
    for (c, g, minus, i0, j0), (hr, pr, qr, nr, mr, gr), (hl, pl, ql, nl, ml, gl) in zip(anc, right, left):
        rec = (j0 - ql, ql + qr, i0 - pl, pl + pr, nl + nr, ml + mr, gl + gr)
        assert score2_of((0, 0, 0) + rec) == hl + hr
        found.setdefault((c, g, minus), {})[rec] = hl + hr          # identical ones once
    out = []
    for key, recs in found.items():
        order = sorted(recs, key=lambda r: (-recs[r],) + r)
        q0 = np.array([r[0] for r in order])
        q1 = q0 + np.array([r[1] for r in order])
        s0 = np.array([r[2] for r in order])
        s1 = s0 + np.array([r[3] for r in order])
        kept = np.zeros(len(order), bool)
        for i, r in enumerate(order):
            kept[i] = not (kept[:i] & (q0[:i] <= q0[i]) & (q1[i] <= q1[:i]) & (s0[:i] <= s0[i]) &
                           (s1[i] <= s1[:i])).any()
            if kept[i] and recs[r] >= 2 * P["min_score"]:
                out.append(key + r)
    return sorted(out)


# ---------------------------------------------------------------------------
# the 15-column table
# ---------------------------------------------------------------------------

def rows(records, contig_names, contig_lens, subject_ids, subject_lens, db_bases, max_target_seqs=10000):
    """The table's lines: by contig; within a contig the subjects past --max-target-seqs (ranked
    by (-best score2, subject)) lose their rows, the rest go by (-score2, subject, minus, qstart,
    sstart, qspan, sspan)."""
    per = {}
    for r in records:
        c, g, minus, qs, qn, ss, sn, length, m, gaps = r
        per.setdefault(c, []).append((-score2_of(r), g, minus, qs, ss, qn, sn, length, m, gaps))
    out = []
    for c in sorted(per):
        best = {}
        for r in per[c]:
            best[r[1]] = min(best.get(r[1], 0), r[0])
        keep = set(g for _, g in sorted((v, g) for g, v in best.items())[:max_target_seqs])
        for neg, g, minus, qs, ss, qn, sn, length, m, gaps in sorted(per[c]):
            if g not in keep:
                continue
            score, M = -neg / 2, subject_lens[g]
            s0, s1 = (M - ss, M - ss - sn + 1) if minus else (ss + 1, ss + sn)
            ev = so.K * contig_lens[c] * db_bases * math.exp(-so.LAMBDA * score)
            out.append("\t".join(str(v) for v in (
                contig_names[c], subject_ids[g], contig_lens[c], M, length, qs + 1, qs + qn, s0, s1,
                "%.3f" % (100.0 * m / length), m, gaps, "%.2e" % ev, so.bitscore_text(score),
                "minus" if minus else "plus")))
    return out
