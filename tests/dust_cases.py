"""Hand-built cases of the low-complexity mask.  Every builder returns
(contigs, Wd, Lv, masked): `masked` is the number of masked bases the rule must give, written
down with the reasoning, or None where the case states a property instead (see `CHECKS`).
The tests compare both oracle forms with it, with each other and with the GPU.

At the defaults the threshold is 2.  A homopolymer of n bases is one triplet kind l = n - 2
times: r = l (l - 1) / 2, score l / 2, which grows with l, so the whole run is its own best
sub-interval; it exceeds 2 from l = 5, n = 7 on."""
import random

import dust_oracle as do


def rnd(n, seed):
    r = random.Random(seed)
    return "".join(r.choice("ACGT") for _ in range(n))


def _case(contigs, masked, Wd=64, Lv=20):
    return contigs, Wd, Lv, masked


def poly_a_6():
    """l = 4, score 2: not above the threshold."""
    return _case(["A" * 6], 0)


def poly_a_7():
    """l = 5, score 2.5."""
    return _case(["A" * 7], 7)


def poly_a_64():
    """Exactly one window."""
    return _case(["A" * 64], 64)


def poly_a_200():
    """Longer than the window: every 64-base stretch is perfect, their union is the run."""
    return _case(["A" * 200], 200)


def ac_5():
    """(AC)x5: 8 triplets, ACA and CAC four times each: r = 12, score 12 / 7 < 2."""
    return _case(["AC" * 5], 0)


def ac_6():
    """(AC)x6: 10 triplets, five of each kind: r = 20, score 20 / 9 > 2; its sub-intervals
    score less (l = 9: 16 / 8)."""
    return _case(["AC" * 6], 12)


def random_100():
    return _case([rnd(100, 101)], 0)


def n_splits_short_runs():
    """A x4, N, A x4: two runs of 4 bases; across the N it would be a run of 9."""
    return _case(["AAAANAAAA"], 0)


def n_after_seven():
    """A x7 (masked), N, A x6 (not)."""
    return _case(["A" * 7 + "N" + "A" * 6], 7)


def contig_end_splits_short_runs():
    """Two contigs of A x4, neighbours in the store without padding: 8 A's in a row there."""
    return _case(["AAAA", "AAAA"], 0)


def two_contigs_of_seven():
    """A x7 | A x7: both masked, as two intervals."""
    return _case(["A" * 7, "A" * 7], 14)


def lower_case():
    return _case(["a" * 9], 9)


def flanked_poly_a():
    """Random flanks, poly-A x30 between them.  The flank bases next to the run do not join
    it: count from the oracle, the flanks' ends checked in CHECKS."""
    return _case([rnd(60, 102) + "A" * 30 + rnd(60, 103)], None)


def run_at_store_end():
    """The last contig ends in A x12: the run ends exactly at the store's last base."""
    return _case([rnd(50, 104), rnd(45, 105) + "A" * 12], None)


def across_word_boundary():
    """A C-run at store positions 25..40, across the first 32-bit word boundary."""
    x = rnd(100, 106)
    return _case([x[:25] + "C" * 16 + x[41:]], None)


MIXED = (rnd(40, 107) + "A" * 25 + rnd(20, 108) + "AC" * 14 + rnd(15, 109) + "ACG" * 10 + "N" + "T" * 9 +
         rnd(30, 110) + "AAAC" * 8 + rnd(25, 111) + "G" * 70)[:300]
assert len(MIXED) == 300


def _mixed(Wd, Lv):
    def f():
        return _case([MIXED], None, Wd, Lv)
    f.__name__ = "mixed_w{}_l{}".format(Wd, Lv)
    return f


def empty_set():
    return _case([], 0)


def short_contigs():
    """Fewer than 3 bases: no triplet."""
    return _case(["AA", "", "A"], 0)


CASES = {f.__name__: f for f in [
    poly_a_6, poly_a_7, poly_a_64, poly_a_200, ac_5, ac_6, random_100, n_splits_short_runs, n_after_seven,
    contig_end_splits_short_runs, two_contigs_of_seven, lower_case, flanked_poly_a, run_at_store_end,
    across_word_boundary, empty_set, short_contigs] +
    [_mixed(Wd, Lv) for Wd in (8, 16, 63, 64) for Lv in (10, 20, 30)]}


def _flanks_unmasked(mask):
    assert not mask[:55].any() and not mask[95:].any()       # the flanks, but for the 5 bases
    assert mask[60:90].all()                                 # next to the run on either side


def _store_end(mask):
    assert mask[-12:].all() and not mask[:80].any()


def _word_boundary(mask):
    assert mask[25:41].all() and not mask[:20].any() and not mask[46:].any()


# properties of the cases without a written count, checked on every mask
CHECKS = {"flanked_poly_a": _flanks_unmasked, "run_at_store_end": _store_end,
          "across_word_boundary": _word_boundary}

_cache = {}


def expected(name):
    """(contigs, Wd, Lv, masked, mask): the mask by both oracle forms, which must agree;
    computed once per process."""
    if name not in _cache:
        contigs, Wd, Lv, masked = CASES[name]()
        a, b = do.mask_brute(contigs, Wd, Lv), do.mask_windows(contigs, Wd, Lv)
        assert (a == b).all(), name
        _cache[name] = (contigs, Wd, Lv, masked, a)
    return _cache[name]
