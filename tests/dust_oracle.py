"""CPU oracles of the low-complexity mask (the symmetric-DUST definition of
Morgulis et al. 2006), written from the rule's text.

Two independent forms:
  mask_brute    by the definition: every interval of every run, its score as a Fraction,
                compared with the score of every one of its sub-intervals
  mask_windows  numpy: prefix counts of the 64 triplet kinds give the score numerator of every
                (start, length) at once; scores become exact integer ranks; the greatest score
                among an interval's sub-intervals is two running maxima (over the ends of one
                start, then over the starts of one end); an interval is perfect when it
                passes the threshold and its own rank equals that maximum

Both take the contigs as strings and return a bool array with one entry per store base (the
contigs concatenated).  Wd: window in bases, Lv: level (threshold Lv / 10).
"""
import functools
import math
from collections import Counter
from fractions import Fraction

import numpy as np

DEFAULTS = dict(Wd=64, Lv=20)


def norm(s):
    return "".join(ch if ch in "ACGT" else "N" for ch in s.upper())


# ---------------------------------------------------------------------------
# form 1: the definition
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def score(bases):
    """Score of the interval that covers `bases` (l = len - 2 triplets)."""
    l = len(bases) - 2
    if l < 2:
        return Fraction(0)
    kinds = Counter(bases[k:k + 3] for k in range(l))
    return Fraction(sum(c * (c - 1) // 2 for c in kinds.values()), l - 1)


@functools.lru_cache(maxsize=None)
def perfect(bases, Lv):
    """The interval's perfectness depends on its own bases only."""
    s = score(bases)
    if not s > Fraction(Lv, 10):
        return False
    n = len(bases)
    return not any(score(bases[a:b]) > s for a in range(n - 2) for b in range(a + 3, n + 1))


def runs(contig):
    """(start, end) of the maximal stretches of A/C/G/T of a normalised contig."""
    out, start = [], None
    for p, ch in enumerate(contig + "N"):
        if ch != "N" and start is None:
            start = p
        if ch == "N" and start is not None:
            out.append((start, p))
            start = None
    return out


def mask_brute(contigs, Wd=64, Lv=20):
    parts = []
    for contig in contigs:
        x = norm(contig)
        m = np.zeros(len(x), bool)
        for r0, r1 in runs(x):
            for i in range(r0, r1 - 2):
                for l in range(1, min(Wd - 2, r1 - 2 - i) + 1):
                    if perfect(x[i:i + l + 2], Lv):
                        m[i:i + l + 2] = True
        parts.append(m)
    return np.concatenate(parts) if parts else np.zeros(0, bool)


# ---------------------------------------------------------------------------
# form 2: arrays
# ---------------------------------------------------------------------------

_MAXL = 62                                       # triplets of the widest interval


@functools.lru_cache(maxsize=None)
def _ranks():
    """rank[r, d]: the place of r / d among all such fractions (equal fractions share it), so
    that integer comparison of ranks is exact comparison of scores.  d = 0 (l = 1) ranks as 0."""
    big = 1
    for d in range(1, _MAXL):
        big = big * d // math.gcd(big, d)
    rmax = _MAXL * (_MAXL - 1) // 2
    key = {(r, d): r * (big // d) for r in range(rmax + 1) for d in range(1, _MAXL)}
    place = {k: n for n, k in enumerate(sorted(set(key.values())))}
    rank = np.zeros((rmax + 1, _MAXL), np.int32)
    for (r, d), k in key.items():
        rank[r, d] = place[k]
    assert place[0] == 0
    return rank


def _mask_contig(x, Wd, Lv):
    n = len(x)
    m = np.zeros(n, bool)
    nt = n - 2
    if nt < 1:
        return m
    code = np.full(256, 4, np.int64)
    for k, ch in enumerate("ACGT"):
        code[ord(ch)] = k
    c = code[np.frombuffer(x.encode(), np.uint8)]
    isn = c == 4
    # len_run[p]: bases of the run from p on (0 at an N)
    nxt = np.where(isn, np.arange(n), n)
    nxt = np.minimum.accumulate(nxt[::-1])[::-1]
    len_run = nxt - np.arange(n)
    kind = np.where(isn[:-2] | isn[1:-1] | isn[2:], 64, c[:-2] * 16 + c[1:-1] * 4 + c[2:])
    P = np.zeros((nt + 1, 65), np.int32)
    P[np.arange(1, nt + 1), kind] = 1
    P = np.cumsum(P, axis=0, dtype=np.int32)
    L = min(Wd - 2, _MAXL)
    start = np.arange(nt)
    lmax = np.clip(len_run[:nt] - 2, 0, L)       # intervals of a start: l = 1 .. lmax
    # numer[i, l]: each further triplet adds the number of its kind among those before it
    numer = np.zeros((nt, L + 1), np.int64)
    for l in range(2, L + 1):
        ok = lmax >= l
        last = np.where(ok, start + l - 1, 0)
        k = kind[last]
        numer[:, l] = numer[:, l - 1] + np.where(ok, P[last, k] - P[start, k], 0)
    ls = np.arange(L + 1)
    valid = (ls[None, :] >= 1) & (ls[None, :] <= lmax[:, None])
    rank = np.where(valid, _ranks()[numer, np.maximum(ls - 1, 0)[None, :]], -1)
    # the greatest rank among intervals of start i that end at or before i + l
    by_start = np.maximum.accumulate(rank, axis=1)
    # ... re-indexed by the end e = i + l, e = 1 .. nt: by_end[e, l] belongs to start e - l
    e = np.arange(nt + 1)
    src = e[:, None] - ls[None, :]
    inside = (src >= 0) & (ls[None, :] >= 1)
    by_end = np.where(inside, by_start[np.clip(src, 0, nt - 1), ls[None, :]], -1)
    # over starts e - 1 down to e - l: for a valid interval (i, l) these all lie in its run
    inner = np.maximum.accumulate(by_end, axis=1)
    best = inner[np.clip(start[:, None] + ls[None, :], 0, nt), ls[None, :]]
    perfect = valid & (10 * numer > Lv * (ls[None, :] - 1)) & (rank == best)
    longest = np.where(perfect, ls[None, :], 0).max(axis=1)
    cover = np.zeros(n + 1, np.int64)
    hit = np.flatnonzero(longest > 0)
    np.add.at(cover, hit, 1)
    np.add.at(cover, hit + longest[hit] + 2, -1)
    return np.cumsum(cover)[:n] > 0


def mask_windows(contigs, Wd=64, Lv=20):
    parts = [_mask_contig(norm(c), Wd, Lv) for c in contigs]
    return np.concatenate(parts) if parts else np.zeros(0, bool)


def intervals(mask, lens):
    """(contig, start, end) of the masked stretches, 0-based half-open, split at contig ends."""
    out, base = [], 0
    for c, n in enumerate(lens):
        m = np.concatenate([[False], mask[base:base + n], [False]])
        d = np.flatnonzero(m[1:] != m[:-1])
        out += [(c, int(a), int(b)) for a, b in zip(d[0::2], d[1::2])]
        base += n
    return out
