"""The envelope-integral bounds of the first wave form's pruning (wf_device.h: env_integral,
marker_lb; wf_fast.hip: scan_best), restated line by line in Python, in the device's
operation order, and checked against np.mean of the materialised site array -- numpy's
pairwise sum, the value the kernels reproduce bit for bit.

For a segment with 2..kPruneMax attachments the device keeps
    ub = min(best score * (1 + 1e-14), I * (1 + 2e-12))   in the not-evaluated marker, -1 - ub
      (numpy's rounded mean of n equal sites can exceed their value by an ulp: the cap carries it),
    lb = I * (1 - 2e-12)                    (the bound), and
    marker_lb(-1 - ub)                      (the lower bound the kernel re-derives from the marker)
with I the plain-double integral of the max-envelope over the locus length.

This checks the model: an edit to wf_device.h that is not mirrored here leaves it green.
The device code is checked by tests/test_gpu_env_bounds.py against the oracle."""
import random

import numpy as np
import pytest

SLACK = 2e-12
ATTACHMENTS = [2, 3, 4, 5, 6, 7, 8, 16, 64]
LENGTHS = [1, 7, 8, 9, 127, 128, 129, 1000, 8191]
KINDS = ["partial", "nested", "identical", "empty", "whole", "equal"]


def env_integral(atts, length):
    """Line-by-line restatement of wf_device.h env_integral: (I, the envelope's maximum)."""
    acc = 0.0
    best = 0.0
    p = 0
    while p < length:
        nx = length
        val = 0.0
        for lo, hi, s in atts:
            if lo >= hi:
                continue
            if lo <= p and p < hi:
                val = s if s > val else val
                nx = hi if hi < nx else nx
            elif lo > p:
                nx = lo if lo < nx else nx
        best = val if val > best else best
        acc += val * float(nx - p)
        p = nx
    return acc / float(length), best


def bounds(atts, length):
    """scan_best's upper bound and the lower bound."""
    integral, best = env_integral(atts, length)
    return integral * (1.0 - SLACK), min(best * (1.0 + 1e-14), integral * (1.0 + SLACK))


def marker_lb(v):
    """Line-by-line restatement of wf_device.h marker_lb."""
    ub = -1.0 - v
    lb = ub * (1.0 - 5e-12) - 4.5e-16 * (1.0 + ub)
    return lb if lb > 0.0 else 0.0


def site_mean(atts, length):
    site = np.zeros(length, dtype=np.float64)
    for lo, hi, s in atts:
        site[lo:hi] = np.maximum(site[lo:hi], s)
    return float(np.mean(site))


def score(rng):
    return rng.randrange(1, 1001) / 1000.0 * rng.randrange(50, 1001) / 1000.0


def make(kind, na, length, rng):
    def rand_range(a=0, b=length):
        lo = rng.randrange(a, b + 1)
        return lo, rng.randrange(lo, b + 1)

    if kind == "partial":
        return [rand_range() + (score(rng),) for _ in range(na)]
    if kind == "nested":
        lo, hi, out = 0, length, []
        for _ in range(na):
            out.append((lo, hi, score(rng)))
            lo, hi = rand_range(lo, hi)
        rng.shuffle(out)
        return out
    if kind == "identical":
        lo, hi = rand_range()
        return [(lo, hi, score(rng)) for _ in range(na)]
    if kind == "empty":                                   # lo == hi, among ordinary ranges
        out = [rand_range() + (score(rng),) for _ in range(na)]
        for i in rng.sample(range(na), max(1, na // 2)):
            lo = rng.randrange(0, length + 1)
            out[i] = (lo, lo, score(rng))
        return out
    if kind == "whole":                                   # whole-locus hits over partial ones
        out = [rand_range() + (score(rng),) for _ in range(na)]
        for i in rng.sample(range(na), max(1, na // 3)):
            out[i] = (0, length, score(rng))
        return out
    assert kind == "equal"
    s = score(rng)
    return [rand_range() + (s,) for _ in range(na)]


def all_empty(na, length, rng):
    return [(p, p, score(rng)) for p in (rng.randrange(0, length + 1) for _ in range(na))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("na", ATTACHMENTS)
def test_bounds_hold_and_are_tight(kind, na):
    rng = random.Random(1000 * na + KINDS.index(kind))
    for length in LENGTHS:
        cases = [make(kind, na, length, rng) for _ in range(6)]
        if kind == "empty":
            cases.append(all_empty(na, length, rng))
        for atts in cases:
            mean = site_mean(atts, length)
            lb, ub = bounds(atts, length)
            assert lb <= mean <= ub, (kind, na, length, atts, lb, mean, ub)
            assert ub - lb <= 1e-11 * mean, (kind, na, length, atts, lb, mean, ub)
            # the lower bound the kernel takes back out of the marker: below the mean, and
            # within 6e-12 relative + the marker's absolute rounding of the upper bound
            mlb = marker_lb(-1.0 - ub)
            assert mlb <= mean, (kind, na, length, atts, mlb, mean)
            assert ub - mlb <= 6e-12 * ub + 1e-15 * (1.0 + ub)


def test_one_attachment_marker_bound():
    """One attachment: ub = min(score, score * share * (1 + 2e-12)) (scan_best, as before: an
    upper bound up to numpy's rounding of a whole-locus run, which the 1e-12 slack of every
    threshold it is compared with covers); the marker's lower bound stays below the mean."""
    rng = random.Random(7)
    for length in LENGTHS:
        for _ in range(40):
            lo = rng.randrange(0, length + 1)
            hi = rng.choice([lo, length, rng.randrange(lo, length + 1)])
            s = score(rng)
            mean = site_mean([(lo, hi, s)], length)
            ub = min(s, s * (float(max(0, hi - lo)) / float(length)) * (1.0 + SLACK))
            assert mean <= ub * (1.0 + 1e-14)
            assert marker_lb(-1.0 - ub) <= mean


def test_integral_is_order_independent():
    """The sweep does not depend on the attachments' order beyond the last bits."""
    rng = random.Random(11)
    for _ in range(50):
        atts = make("partial", 8, 1000, rng)
        a, _ = env_integral(atts, 1000)
        rng.shuffle(atts)
        b, _ = env_integral(atts, 1000)
        assert a == b                                     # same runs, same order of sites
