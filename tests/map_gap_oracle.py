"""CPU oracles of the single-gap rescue of the read mapper ("gapped pass";
TEST INFRASTRUCTURE ONLY).

Two independent restatements of the rule k_map_gap (wf_map.hip) implements, on top of the
ungapped oracles of tests/map_oracle.py:

  map_pairs_gapped_brute    literal: every (contig, p, d, k) of every variant, mismatches and
                            seeds checked column by column.  Only the (p, d) without any
                            usable seed matching on either of their two diagonals are skipped
                            early: they cannot be seeded for any k (tiny inputs only)
  map_pairs_gapped_indexed  the dictionary index: diagonals from seed hits with the seed
                            offsets that hit them, mismatches by numpy prefix sums, the
                            seeded k as a boolean array

A result is (contig, pos1, pos2, strand1, mm1, mm2, d1, d2, k1, k2, flags); flags bit 0: the
pair was aligned by the gapped pass, bit 1: a mate had more than MAX_HITS hits in it.
"""
import numpy as np

import map_oracle as mo

MAX_HITS = 256
GAP_FIELDS = (("d1", np.int8), ("d2", np.int8), ("k1", np.int16), ("k2", np.int16), ("flags", np.uint8))
NO_GAP = (0, 0, 0, 0, 0)


def best_pair_gapped(hits1, hits2, L1, L2, P):
    """hits: [(contig, p, strand, d, k, mm)] of each mate -> the result of least key."""
    if len(set(h[:4] for h in hits1)) > MAX_HITS or len(set(h[:4] for h in hits2)) > MAX_HITS:
        return mo.UNALIGNED + (0, 0, 0, 0, 2)
    best = None
    for c1, p1, s1, d1, k1, m1 in hits1:
        for c2, p2, s2, d2, k2, m2 in hits2:
            if c1 != c2 or s1 == s2:
                continue
            if s1 == 0:
                fp, fe, rp, re_ = p1, p1 + L1 + d1, p2, p2 + L2 + d2
            else:
                fp, fe, rp, re_ = p2, p2 + L2 + d2, p1, p1 + L1 + d1
            if not (fp <= rp and fe <= re_):
                continue
            frag = re_ - fp
            if not P["min_insert"] <= frag <= P["max_insert"]:
                continue
            key = (m1 + abs(d1) + m2 + abs(d2), abs(d1) + abs(d2), c1, fp, frag, s1, d1, d2)
            if best is None or key < best[0]:
                best = (key, (c1, p1 + 1, p2 + 1, s1, m1, m2, d1, d2, k1, k2, 1))
    return best[1] if best else mo.UNALIGNED + NO_GAP


# ---------------------------------------------------------------------------
# literal brute force
# ---------------------------------------------------------------------------

def _columns(L, p, d, k):
    """(read index, contig index) of every aligned column."""
    if d == 0:
        return [(i, p + i) for i in range(L)]
    g = max(0, -d)
    return [(i, p + i) for i in range(k)] + [(i, p + i + d) for i in range(k + g, L)]


def _hits_gapped_brute(contigs, read, P, G):
    S, L = P["S"], len(read)
    hits = []
    for strand, x in ((0, read), (1, mo.revcomp(read))):
        usable = []
        for j in range(min(L // S, mo.MAX_SLOTS)):
            kmer = x[j * S:(j + 1) * S]
            if b"N" not in kmer and mo._occurrences(contigs, kmer) <= P["max_occ"]:
                usable.append(j * S)
        for c, s in enumerate(contigs):
            # diagonals q (read index i against s[q + i]) on which some usable seed matches
            diag = set(q for q in range(-L, len(s) + 1) for i in usable
                       if q + i >= 0 and s[q + i:q + i + S] == x[i:i + S])
            for d in range(-G, G + 1):
                g = max(0, -d)
                ks = [0] if d == 0 else range(S, L - S - g + 1)
                for p in range(0, len(s) - L - d + 1):
                    if p not in diag and p + d not in diag:
                        continue
                    best = None
                    for k in ks:
                        cols = dict(_columns(L, p, d, k))
                        mm = sum(1 for i, q in cols.items() if x[i] != s[q] or x[i] == ord("N"))
                        if mm > P["max_mm"]:
                            continue
                        seeded = False
                        for i0 in usable:
                            seg = range(i0, i0 + S)
                            inside = d == 0 or i0 + S <= k or i0 >= k + g
                            if inside and all(x[i] == s[cols[i]] for i in seg):
                                seeded = True
                        if seeded and (best is None or (mm, k) < best):
                            best = (mm, k)
                    if best is not None:
                        hits.append((c, p, strand, d, best[1], best[0]))
    return hits


def _gapped(ungapped, contigs, reads1, reads2, P, G, hits):
    out = []
    for u, r1, r2 in zip(ungapped, reads1, reads2):
        r1, r2 = mo.norm(r1), mo.norm(r2)
        if u[0] >= 0 or G == 0 or len(r1) < P["S"] or len(r2) < P["S"]:
            out.append(tuple(u) + NO_GAP)
        else:
            out.append(best_pair_gapped(hits(r1), hits(r2), len(r1), len(r2), P))
    return out


def map_pairs_gapped_brute(contigs, reads1, reads2, P, G):
    norm = [mo.norm(s) for s in contigs]
    return _gapped(mo.map_pairs_brute(contigs, reads1, reads2, P), contigs, reads1, reads2, P, G,
                   lambda r: _hits_gapped_brute(norm, r, P, G))


# ---------------------------------------------------------------------------
# dictionary index
# ---------------------------------------------------------------------------

def _hits_gapped_indexed(ix, read, P, G):
    S, L = ix.S, len(read)
    hits = []
    for strand, x in ((0, read), (1, mo.revcomp(read))):
        seeds = {}                                     # (contig, diagonal) -> seed offsets
        for j in range(min(L // S, mo.MAX_SLOTS)):
            occ = ix.table.get(x[j * S:(j + 1) * S], ())
            if 0 < len(occ) <= P["max_occ"]:
                for c, q in occ:
                    seeds.setdefault((c, q - j * S), []).append(j * S)
        todo = set()
        for c, q in seeds:
            for d in range(-G, G + 1):
                todo.add((c, q, d))                    # q is the left diagonal
                todo.add((c, q - d, d))                # ... the right one
        xa = np.frombuffer(x, dtype=np.uint8)
        xn = xa == ord("N")
        for c, p, d in sorted(todo):
            g = max(0, -d)
            n = len(ix.contigs[c])
            if p < 0 or p + L + d > n:
                continue

            def cum(q):                                # mismatches of read[:i] on diagonal q
                lo, hi = max(0, -q), min(L, n - q)
                bad = np.ones(L, bool)                 # columns outside the contig never count
                bad[lo:hi] = (xa[lo:hi] != ix.arr[c][q + lo:q + hi]) | xn[lo:hi] | ix.isn[c][q + lo:q + hi]
                return np.concatenate([[0], np.cumsum(bad)])

            left = cum(p)
            if d == 0:
                if int(left[L]) <= P["max_mm"]:
                    hits.append((c, p, strand, 0, 0, int(left[L])))
                continue
            ks = np.arange(S, L - S - g + 1)
            if len(ks) == 0:
                continue
            right = cum(p + d)
            mm = left[ks] + (right[L] - right[ks + g])
            seeded = np.zeros(len(ks), bool)
            for i0 in seeds.get((c, p), ()):
                seeded |= i0 + S <= ks
            for i0 in seeds.get((c, p + d), ()):
                seeded |= i0 >= ks + g
            ok = seeded & (mm <= P["max_mm"])
            if ok.any():
                k = int(ks[ok][np.argmin(mm[ok])])      # argmin: the first, so the least k
                hits.append((c, p, strand, d, k, int(mm[k - S])))
    return hits


def map_pairs_gapped_indexed(contigs, reads1, reads2, P, G, index=None):
    ix = index or mo.Index(contigs, P["S"])
    return _gapped(mo.map_pairs_indexed(contigs, reads1, reads2, P, index=ix), contigs, reads1, reads2, P, G,
                   lambda r: _hits_gapped_indexed(ix, r, P, G))


def as_arrays(results):
    """Result tuples -> the arrays wf_map_pairs_gapped writes."""
    a = np.array(results, dtype=np.int64).reshape(-1, 11)
    out = mo.as_arrays([r[:6] for r in results])
    for j, (f, dt) in enumerate(GAP_FIELDS):
        out[f] = a[:, 6 + j].astype(dt)
    return out
