"""CPU oracles of the paired-read mapping rule (TEST INFRASTRUCTURE ONLY).

Two independent restatements of the rule wf_map.hip implements, used by tests/test_map.py
(they must agree with each other) and tests/test_gpu_map.py (the kernel must equal them on
every field):

  map_pairs_brute    literal: slides every read variant over every position of every contig
                     and counts S-mer occurrences by scanning (tiny inputs only)
  map_pairs_indexed  a dictionary from S-mer to its positions, candidates from seed hits,
                     mismatches counted with numpy (the medium random case)

Contigs and reads are bytes.  A result is (contig, pos1, pos2, strand1, mm1, mm2) with
1-based positions and strand1 0 for mate 1 on +; UNALIGNED when no concordant pair exists.
"""
import numpy as np

UNALIGNED = (-1, 0, 0, 0, 0, 0)
MAX_SLOTS = 16
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_ACGT = frozenset(b"ACGT")


def params(S=20, max_occ=16, max_mm=4, min_insert=0, max_insert=500):
    return dict(S=S, max_occ=max_occ, max_mm=max_mm, min_insert=min_insert, max_insert=max_insert)


def norm(seq):
    """Upper case; every byte other than A, C, G, T becomes N."""
    return bytes(b if b in _ACGT else ord("N") for b in bytes(seq).upper())


def revcomp(x):
    return x.translate(_COMP)[::-1]            # x is normalised: N stays N


def best_pair(hits1, hits2, L1, L2, P):
    """hits: [(contig, p, strand, mm)] of each mate -> the result of least key."""
    best = None
    for c1, p1, s1, m1 in hits1:
        for c2, p2, s2, m2 in hits2:
            if c1 != c2 or s1 == s2:
                continue
            if s1 == 0:
                fp, Lf, rp, Lr = p1, L1, p2, L2
            else:
                fp, Lf, rp, Lr = p2, L2, p1, L1
            if not (fp <= rp and fp + Lf <= rp + Lr):
                continue
            frag = rp + Lr - fp
            if not P["min_insert"] <= frag <= P["max_insert"]:
                continue
            key = (m1 + m2, c1, fp, frag, s1)
            if best is None or key < best[0]:
                best = (key, (c1, p1 + 1, p2 + 1, s1, m1, m2))
    return best[1] if best else UNALIGNED


# ---------------------------------------------------------------------------
# literal brute force
# ---------------------------------------------------------------------------

def _occurrences(contigs, kmer):
    n = 0
    for s in contigs:
        for p in range(len(s) - len(kmer) + 1):
            if s[p:p + len(kmer)] == kmer:
                n += 1
    return n


def _hits_brute(contigs, read, P):
    S = P["S"]
    L = len(read)
    hits = []
    if L < S:
        return hits
    for strand, x in ((0, read), (1, revcomp(read))):
        usable = []
        for j in range(min(L // S, MAX_SLOTS)):
            kmer = x[j * S:(j + 1) * S]
            if b"N" not in kmer and _occurrences(contigs, kmer) <= P["max_occ"]:
                usable.append(j * S)
        for c, s in enumerate(contigs):
            for p in range(len(s) - L + 1):
                mm = sum(1 for i in range(L) if x[i] != s[p + i] or x[i] == ord("N"))
                if mm > P["max_mm"]:
                    continue
                if any(x[i:i + S] == s[p + i:p + i + S] for i in usable):
                    hits.append((c, p, strand, mm))
    return hits


def map_pairs_brute(contigs, reads1, reads2, P):
    contigs = [norm(s) for s in contigs]
    out = []
    for r1, r2 in zip(reads1, reads2):
        r1, r2 = norm(r1), norm(r2)
        out.append(best_pair(_hits_brute(contigs, r1, P), _hits_brute(contigs, r2, P),
                             len(r1), len(r2), P))
    return out


# ---------------------------------------------------------------------------
# dictionary index
# ---------------------------------------------------------------------------

class Index:
    def __init__(self, contigs, S):
        self.S = S
        self.contigs = [norm(s) for s in contigs]
        self.arr = [np.frombuffer(s, dtype=np.uint8) for s in self.contigs]
        self.isn = [a == ord("N") for a in self.arr]
        self.table = {}
        for c, s in enumerate(self.contigs):
            for p in range(len(s) - S + 1):
                kmer = s[p:p + S]
                if b"N" not in kmer:
                    self.table.setdefault(kmer, []).append((c, p))


def _hits_indexed(ix, read, P):
    S, L = ix.S, len(read)
    hits = []
    if L < S:
        return hits
    for strand, x in ((0, read), (1, revcomp(read))):
        cands = set()
        for j in range(min(L // S, MAX_SLOTS)):
            occ = ix.table.get(x[j * S:(j + 1) * S], ())
            if 0 < len(occ) <= P["max_occ"]:
                for c, q in occ:
                    p = q - j * S
                    if p >= 0 and p + L <= len(ix.contigs[c]):
                        cands.add((c, p))
        xa = np.frombuffer(x, dtype=np.uint8)
        xn = xa == ord("N")
        for c, p in cands:
            mm = int(np.count_nonzero((xa != ix.arr[c][p:p + L]) | xn | ix.isn[c][p:p + L]))
            if mm <= P["max_mm"]:
                hits.append((c, p, strand, mm))
    return hits


def map_pairs_indexed(contigs, reads1, reads2, P, index=None):
    ix = index or Index(contigs, P["S"])
    out = []
    for r1, r2 in zip(reads1, reads2):
        r1, r2 = norm(r1), norm(r2)
        out.append(best_pair(_hits_indexed(ix, r1, P), _hits_indexed(ix, r2, P), len(r1), len(r2), P))
    return out


def as_arrays(results):
    """Result tuples -> the arrays wf_map_pairs writes."""
    a = np.array(results, dtype=np.int64).reshape(-1, 6)
    return dict(contig=a[:, 0].astype(np.int32), pos1=a[:, 1].astype(np.int32),
                pos2=a[:, 2].astype(np.int32), strand1=a[:, 3].astype(np.uint8),
                mm1=a[:, 4].astype(np.uint8), mm2=a[:, 5].astype(np.uint8))
