"""The reporting step of the native search (DESIGN.md §12.1 "Reporting", §12.5 "Reporting",
§12.8) on the CPU, twice per kind.

Ungapped.  A raw HSP is (contig, subject, minus, delta, b, e, score); its group is (subject,
minus, contig, delta).  Identical (b, e) in a group count once; an HSP is dropped iff another
of its group with a different interval contains it; containment first, then score >= min_score.
  hsps_pairwise  A, the definition: every pair of a group's distinct intervals is compared
  hsps_reach     B, the parallel form of wf_report.hip: sort by (group, b, -e); equal to the
                 predecessor = duplicate; contained iff the running maximum of
                 (group rank << 32 | e), read one position back, reaches e within the group
Two HSPs equal in (group, b, e) have equal scores (they cover the same bases); a set that breaks
this has no defined result and no test builds one.

Gapped.  A raw element is (contig, subject, minus, i0, j0, lH, lp, lq, lg, rH, rp, rq, rg): an
anchor and the two sides of its extension.  `alignment` is the closed form of §12.5.
  alns_greedy    A, the definition: per (subject, minus, contig) in the order (-score2, qstart,
                 sstart, qspan, sspan, length, matches, gaps), an alignment is dropped when a kept
                 earlier one covers both its intervals
  alns_any       B, the parallel form: ... when any earlier one covers them, each decided alone
Both return (records in the order of the output, raw_alignments)."""
import numpy as np

HSP = ("contig", "subject", "minus", "delta", "b", "e", "score")
ANCHOR = ("contig", "subject", "minus", "i0", "j0", "left_H", "left_p", "left_q", "left_g",
          "right_H", "right_p", "right_q", "right_g")


def columns(raw, names):
    """{name: list} of the tuples `raw`, for search.report_once"""
    return {f: [r[k] for r in raw] for k, f in enumerate(names)}


def hsp_record(c, g, minus, delta, b, e, score):
    length = e - b
    return (c, g, minus, b + delta, b, length, (score + 2 * length) // 3)


# ---------------------------------------------------------------------------
# ungapped
# ---------------------------------------------------------------------------

def hsps_pairwise(raw, min_score):
    groups = {}
    for c, g, minus, delta, b, e, score in set(raw):
        groups.setdefault((g, minus, c, delta), {})[(b, e)] = score
    out = []
    for (g, minus, c, delta), hs in groups.items():
        iv = np.array(sorted(hs), np.int64).reshape(-1, 2)
        b, e = iv[:, 0], iv[:, 1]
        for lo in range(0, len(iv), 2048):                   # x in [lo, lo + 2048) against every y
            xb, xe = b[lo:lo + 2048, None], e[lo:lo + 2048, None]
            inside = (b[None, :] <= xb) & (xe <= e[None, :]) & ((b[None, :] != xb) | (e[None, :] != xe))
            for k in np.flatnonzero(~inside.any(axis=1)):
                x = (int(b[lo + k]), int(e[lo + k]))
                if hs[x] >= min_score:
                    out.append(hsp_record(c, g, minus, delta, x[0], x[1], hs[x]))
    return sorted(out)


def hsps_reach(raw, min_score):
    if not raw:
        return []
    a = np.array(raw, np.int64).reshape(-1, 7)
    c, g, minus, delta, b, e, score = a.T
    sm = g << 1 | minus
    order = np.lexsort((-e, b, delta, c, sm))
    c, sm, delta, b, e, score = (x[order] for x in (c, sm, delta, b, e, score))
    same = np.zeros(len(a), bool)
    same[1:] = (sm[1:] == sm[:-1]) & (c[1:] == c[:-1]) & (delta[1:] == delta[:-1])
    dup = same.copy()
    dup[1:] &= (b[1:] == b[:-1]) & (e[1:] == e[:-1])
    rank = np.cumsum(~same)
    run = np.maximum.accumulate(rank << 32 | e)
    contained = np.zeros(len(a), bool)
    contained[1:] = run[:-1] >= (rank[1:] << 32 | e[1:])
    keep = ~dup & ~contained & (score >= min_score)
    return sorted(hsp_record(int(c[i]), int(sm[i]) >> 1, int(sm[i]) & 1, int(delta[i]), int(b[i]), int(e[i]),
                             int(score[i])) for i in np.flatnonzero(keep))


# ---------------------------------------------------------------------------
# gapped
# ---------------------------------------------------------------------------

def alignment(c, g, minus, i0, j0, lH, lp, lq, lg, rH, rp, rq, rg):
    """(sm, contig, score2, qstart, sstart, qspan, sspan, length, matches, gaps)"""
    qspan, sspan, gaps, score2 = lq + rq, lp + rp, lg + rg, lH + rH
    pairs = (sspan + qspan - gaps) // 2
    return (g << 1 | minus, c, score2, j0 - lq, i0 - lp, qspan, sspan, pairs + gaps,
            (score2 + 5 * gaps + 4 * pairs) // 6, gaps)


def _in_order(raw):
    alns = sorted({alignment(*r) for r in raw}, key=lambda x: (x[0], x[1], -x[2]) + x[3:])
    return alns


def _covers(y, x):
    return y[3] <= x[3] and x[3] + x[5] <= y[3] + y[5] and y[4] <= x[4] and x[4] + x[6] <= y[4] + y[6]


def _records(kept, min_score):
    return sorted((x[1], x[0] >> 1, x[0] & 1, x[3], x[5], x[4], x[6], x[7], x[8], x[9])
                  for x in kept if x[2] >= 2 * min_score)


def alns_greedy(raw, min_score):
    alns = _in_order(raw)
    kept, g0 = [], 0
    for i, x in enumerate(alns):
        if i == 0 or alns[i - 1][:2] != x[:2]:
            g0 = len(kept)
        if not any(_covers(y, x) for y in kept[g0:]):
            kept.append(x)
    return _records(kept, min_score), len(alns)


def alns_any(raw, min_score):
    alns = _in_order(raw)
    kept, g0 = [], 0
    for i, x in enumerate(alns):
        if i == 0 or alns[i - 1][:2] != x[:2]:
            g0 = i
        if not any(_covers(alns[k], x) for k in range(g0, i)):
            kept.append(x)
    return _records(kept, min_score), len(alns)


def sort_key(rec):
    """the order of wf_search_gapped's output: (contig, subject, minus, qstart, sstart, qspan, sspan, ...)"""
    return (rec[0], rec[1], rec[2], rec[3], rec[5], rec[4], rec[6], rec[7], rec[8], rec[9])
