"""Seeded inputs for the read-mapper tests (tests/test_map.py, tests/test_gpu_map.py).

Every hand-built batch is (contigs, reads1, reads2, params, aligned): `aligned` states, pair
by pair, whether the rule of DESIGN.md §11 aligns it -- test_map.py holds the oracles to
that, so a batch checks what its name says.
"""
import numpy as np

import map_oracle as mo

S = 20


def rand_seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))


def mutate(seq, positions):
    """Substitute the base at each position (A->C->G->T->A)."""
    b = bytearray(seq)
    nxt = dict(zip(b"ACGT", b"CGTA"))
    for p in positions:
        b[p] = nxt[b[p]]
    return bytes(b)


def fr_pair(contig, fp, L1, frag, L2, flip=False):
    """Mates of the fragment contig[fp : fp + frag]; flip: mate 1 is the reverse mate."""
    contig = mo.norm(contig)
    if flip:
        return mo.revcomp(contig[fp + frag - L1:fp + frag]), contig[fp:fp + L2]
    return contig[fp:fp + L1], mo.revcomp(contig[fp + frag - L2:fp + frag])


def _batch(contigs, pairs, aligned, **kw):
    return contigs, [p[0] for p in pairs], [p[1] for p in pairs], mo.params(**kw), aligned


def packing():
    rng = np.random.default_rng(101)
    lens = [31, 32, 33, 64, 65, S, 300]
    contigs = [rand_seq(rng, n) for n in lens]
    pairs, aligned = [], []
    for c in contigs[:5]:                      # mates at the first and last possible offset
        pairs.append(fr_pair(c, 0, S, len(c), S))
        aligned.append(True)
    pairs.append(fr_pair(contigs[5], 0, S, S, S))          # contig of exactly S bases
    aligned.append(True)
    good = fr_pair(contigs[6], 50, 30, 200, 30)
    # (the overrunning mate is the - mate, or starts before the + mate's contig: were it
    # accepted, the pair would be concordant)
    # the seed matches at offset 40 of the 65-base contig, the read ends one base past it
    pairs.append((contigs[4][20:60], mo.revcomp(contigs[4][40:65] + contigs[5][:1])))
    aligned.append(False)
    # the read matches the concatenated store exactly, across the boundary of contigs 3 / 4
    pairs.append((contigs[3][10:50], mo.revcomp(contigs[3][-22:] + contigs[4][:10])))
    aligned.append(False)
    # ... and one that starts five bases before its contig (seed slot 1 lies inside)
    pairs.append((contigs[5][-5:] + contigs[6][:40], good[1]))
    aligned.append(False)
    pairs.append(good)
    aligned.append(True)
    return _batch(contigs, pairs, aligned)


def read_lengths():
    rng = np.random.default_rng(102)
    contig = rand_seq(rng, 700)
    pairs, aligned = [], []
    for L in (S - 1, S, 2 * S - 1, 100, 151, 512):
        pairs.append(fr_pair(contig, 30, L, L + 50, L))
        aligned.append(L >= S)
    pairs.append(fr_pair(contig, 10, 100, 180, S - 1))     # one mate too short
    aligned.append(False)
    return _batch([contig], pairs, aligned, max_insert=600)


def mismatches():
    rng = np.random.default_rng(103)
    contig = rand_seq(rng, 600)
    pairs, aligned = [], []
    m1, m2 = fr_pair(contig, 40, 100, 300, 100)
    pairs.append((mutate(m1, [3, 25, 47, 69]), m2))        # max_mm, a mismatch in 4 of 5 seeds
    aligned.append(True)
    pairs.append((mutate(m1, [3, 25, 47, 69]), mutate(m2, [0, 39, 60, 99])))
    aligned.append(True)
    pairs.append((mutate(m1, [3, 4, 47, 69, 70]), m2))     # max_mm + 1, seeds left
    aligned.append(False)
    pairs.append((mutate(m1, [3, 25, 47, 69, 91]), m2))    # no seed left
    aligned.append(False)
    pairs.append(fr_pair(contig, 20, 100, 500, 100))       # fragment = max_insert
    aligned.append(True)
    pairs.append(fr_pair(contig, 20, 100, 501, 100))       # max_insert + 1
    aligned.append(False)
    return _batch([contig], pairs, aligned)


def min_insert():
    rng = np.random.default_rng(104)
    contig = rand_seq(rng, 500)
    pairs = [fr_pair(contig, 20, 100, 250, 100), fr_pair(contig, 20, 100, 300, 100)]
    return _batch([contig], pairs, [False, True], min_insert=300)


def orientation():
    rng = np.random.default_rng(105)
    a, b = rand_seq(rng, 500), rand_seq(rng, 400)
    pairs, aligned = [], []
    pairs.append(fr_pair(a, 60, 100, 320, 90))             # 99 / 147
    aligned.append(True)
    pairs.append(fr_pair(a, 60, 100, 320, 90, flip=True))  # 83 / 163
    aligned.append(True)
    pairs.append((a[60:160], a[280:380]))                  # FF
    aligned.append(False)
    pairs.append((a[100:200], mo.revcomp(a[50:150])))      # dovetail: the - mate starts first
    aligned.append(False)
    pairs.append((a[60:160], mo.revcomp(b[200:300])))      # different contigs
    aligned.append(False)
    pairs.append((a[100:150], mo.revcomp(a[100:200])))     # + mate contained, same start
    aligned.append(True)
    pairs.append((a[100:200], mo.revcomp(a[150:200])))     # - mate contained, same end
    aligned.append(True)
    pairs.append((a[100:200], mo.revcomp(a[120:170])))     # - mate ends before the + mate does
    aligned.append(False)
    return _batch([a, b], pairs, aligned)


def n_and_case():
    rng = np.random.default_rng(106)
    a = rand_seq(rng, 400)
    low = rand_seq(rng, 300).lower()
    withn = bytearray(rand_seq(rng, 400))
    withn[130] = ord("N")
    withn[135] = ord("n")
    withn = bytes(withn)
    pairs, aligned = [], []
    m1, m2 = fr_pair(a, 30, 100, 250, 100)
    pairs.append((m1[:50] + b"N" + m1[51:], m2.lower()))   # N in the read: one mismatch
    aligned.append(True)
    pairs.append(fr_pair(low, 20, 80, 200, 80))            # lower-case contig
    aligned.append(True)
    pairs.append(fr_pair(withn, 100, 100, 280, 100))       # contig N under mate 1 (N vs N too)
    aligned.append(True)
    m1, m2 = fr_pair(withn, 100, 100, 280, 100)
    pairs.append((m1.replace(b"N", b"A"), m2))
    aligned.append(True)
    pairs.append((b"N" * 100, m2))
    aligned.append(False)
    return _batch([a, low, withn], pairs, aligned)


def repeats():
    rng = np.random.default_rng(107)
    occ = 3
    ra, rb = rand_seq(rng, S), rand_seq(rng, S)
    parts, where = [rand_seq(rng, 100)], {}
    for name, rep, copies in (("a", ra, occ), ("b", rb, occ + 1)):
        for k in range(copies):
            where[name, k] = sum(len(p) for p in parts)
            parts += [rep, rand_seq(rng, 40)]
    parts.append(rand_seq(rng, 150))
    contig = b"".join(parts)
    pairs, aligned = [], []
    for name, ok in (("a", True), ("b", False)):           # 39 bases: the repeat is the only seed
        p = where[name, 1]
        pairs.append((contig[p:p + 39], mo.revcomp(contig[p + 60:p + 100])))
        aligned.append(ok)
    twin = rand_seq(rng, 300)
    pairs.append(fr_pair(twin, 10, 60, 200, 60))           # two identical contigs
    aligned.append(True)
    unit = rand_seq(rng, 50)
    tandem = rand_seq(rng, 60) + unit * occ + rand_seq(rng, 60)
    pairs.append((unit[5:45], mo.revcomp((unit * 2)[30:70])))
    aligned.append(True)
    return _batch([contig, twin, twin, tandem], pairs, aligned, max_occ=occ)


HAND_BUILT = dict(packing=packing, read_lengths=read_lengths, mismatches=mismatches,
                  min_insert=min_insert, orientation=orientation, n_and_case=n_and_case,
                  repeats=repeats)


def medium(seed=7, n_contigs=40, n_pairs=2000):
    """Contigs of 200..3,000 bases with planted repeats, N runs and lower case; 2 x 100 pairs
    with substitutions, fragments of 120..540 (some past max_insert), a few Ns in reads."""
    rng = np.random.default_rng(seed)
    contigs = [bytearray(rand_seq(rng, int(rng.integers(200, 3001)))) for _ in range(n_contigs)]
    for copies in (2, 3, 5, 12, 17, 25):                   # max_occ is 16
        rep = rand_seq(rng, 150)
        for _ in range(copies):
            c = contigs[int(rng.integers(n_contigs))]
            p = int(rng.integers(0, len(c) - 150))
            c[p:p + 150] = rep
    for _ in range(30):
        c = contigs[int(rng.integers(n_contigs))]
        n = int(rng.integers(1, 31))
        p = int(rng.integers(0, len(c) - n))
        c[p:p + n] = b"N" * n
    contigs = [bytes(c).lower() if i % 7 == 3 else bytes(c) for i, c in enumerate(contigs)]
    r1, r2 = [], []
    for i in range(n_pairs):
        c = mo.norm(contigs[int(rng.integers(n_contigs))])
        frag = int(rng.integers(120, 541))
        if len(c) < frag:
            frag = len(c)
        fp = int(rng.integers(0, len(c) - frag + 1))
        m1, m2 = fr_pair(c, fp, 100, frag, 100, flip=bool(i & 1))
        mates = []
        for m in (m1, m2):
            nsub = int(rng.poisson(1.5))
            m = mutate(m.replace(b"N", b"A"), rng.integers(0, 100, nsub).tolist())
            if rng.random() < 0.03:
                q = int(rng.integers(0, 100))
                m = m[:q] + b"N" + m[q + 1:]
            mates.append(m)
        r1.append(mates[0])
        r2.append(mates[1])
    return contigs, r1, r2, mo.params()


def planted(seed=11, n_contigs=10, length=1000, n_pairs=300):
    """Repeat-free contigs and error-free pairs with their origin: (contigs, reads1, reads2,
    params, truth)."""
    rng = np.random.default_rng(seed)
    contigs = [rand_seq(rng, length) for _ in range(n_contigs)]
    r1, r2, truth = [], [], []
    for i in range(n_pairs):
        c = int(rng.integers(n_contigs))
        frag = int(rng.integers(150, 451))
        fp = int(rng.integers(0, length - frag + 1))
        flip = bool(i % 3 == 0)
        m1, m2 = fr_pair(contigs[c], fp, 100, frag, 100, flip=flip)
        r1.append(m1)
        r2.append(m2)
        lo, hi = fp + 1, fp + frag - 100 + 1
        truth.append((c, hi, lo, 1, 0, 0) if flip else (c, lo, hi, 0, 0, 0))
    return contigs, r1, r2, mo.params(), truth


def unique_kmers(contigs, k):
    """True when no k-mer occurs twice over both strands of the contigs (a k-mer equal to
    its own reverse complement counts as twice)."""
    seen = set()
    for s in contigs:
        s = mo.norm(s)
        for strand in (s, mo.revcomp(s)):
            for p in range(len(s) - k + 1):
                kmer = strand[p:p + k]
                if kmer in seen:
                    return False
                seen.add(kmer)
    return True


def flat(seqs):
    """[bytes] -> (uint8 array, int64 offsets)."""
    off = np.zeros(len(seqs) + 1, np.int64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), off
