"""Raw sets for the reporting step (tests/report_oracle.py states the rule): hand-built ones with
their record counts written down, and seeded random ones.

An ungapped case is (raw HSPs, min_score, records); an HSP is (contig, subject, minus, delta, b,
e, score) and `hsp` gives the score of `mism` mismatches.  A gapped case is (raw, min_score,
records, raw_alignments); `anchor` builds one element from its two sides, each (pairs, matches,
subject-only columns, contig-only columns)."""
import random


def hsp(b, e, mism=0, c=0, g=0, minus=0, delta=0):
    return (c, g, minus, delta, b, e, (e - b) - 3 * mism)


def u_empty():
    return [], 28, 0


def u_single():
    return [hsp(10, 50)], 28, 1


def u_duplicates_only():
    return [hsp(10, 50)] * 7, 28, 1


def u_nested_chain_of_five():
    # each contains the next: only the outermost stays
    return [hsp(20 + k, 100 - k) for k in (3, 0, 4, 1, 2)], 28, 1


def u_equal_b_different_e():
    # [10, 60) contains [10, 50) and [10, 40)
    return [hsp(10, 40), hsp(10, 60), hsp(10, 50)], 28, 1


def u_equal_e_different_b():
    return [hsp(30, 80), hsp(10, 80), hsp(20, 80)], 28, 1


def u_partial_overlaps_both_kept():
    return [hsp(10, 60), hsp(30, 90), hsp(61, 120)], 28, 3


def u_container_below_min_score_still_drops():
    # the container: 60 columns, 12 mismatches, score 24 < 28; the contained: 40 columns, score 40
    return [hsp(10, 70, mism=12), hsp(20, 60)], 28, 0


def u_min_score_edge():
    # scores 27, 28, 29 and (33 columns, 2 mismatches) 27 on four diagonals
    return [hsp(0, 27, delta=1), hsp(0, 28, delta=2), hsp(0, 29, delta=3), hsp(0, 33, mism=2, delta=4)], 28, 2


def u_negative_delta():
    # two groups below zero; within -7 one contains the other
    return [hsp(40, 90, delta=-7), hsp(50, 80, delta=-7), hsp(45, 95, delta=-30)], 28, 2


def u_same_interval_in_separate_groups():
    # diagonals 0 / 1, strands, contigs, then another subject: nine groups, and a contained one in the first
    raw = [hsp(10, 50, delta=d, minus=m, c=c) for d in (0, 1) for m in (0, 1) for c in (0, 1)]
    return raw + [hsp(10, 50, g=1), hsp(20, 40)], 28, 9


def u_group_of(n):
    """One group of n distinct intervals, staggered so that none contains another, with a
    contained one after every third, shuffled; a group of one on either side of it in the order."""
    raw = [hsp(2 * k, 2 * k + 40) for k in range(n)]
    raw += [hsp(2 * k + 1, 2 * k + 39) for k in range(0, n, 3)]
    random.Random(n).shuffle(raw)
    return raw + [hsp(0, 30, delta=-1), hsp(0, 30, delta=1)], 28, n + 2


def u_field_extremes(words):
    """Keys of 1, 2 and 3 words: the ranges of subject, contig, delta, b and e decide (key_words
    counts them)."""
    if words == 1:      # a few bits a field
        raw = [hsp(0, 60), hsp(5, 40), hsp(40, 100, c=1, g=1, minus=1, delta=9), hsp(41, 99, c=1, g=1, minus=1, delta=9)]
        return raw, 28, 2
    if words == 2:      # about 20 bits for subject, contig and delta, 9 for b and e
        raw = [hsp(0, 1000), hsp(1, 1000), hsp(500, 1500, c=10 ** 6 - 1, g=10 ** 6 - 1, minus=1, delta=-10 ** 6),
               hsp(500, 1499, c=10 ** 6 - 1, g=10 ** 6 - 1, minus=1, delta=-10 ** 6), hsp(500, 1500, delta=10 ** 6)]
        return raw, 28, 3
    big = 2 ** 31 - 1   # the int32 columns' ends; b and e up to 2^28
    far = 2 ** 28
    raw = [hsp(0, 100, delta=-2 ** 31), hsp(0, 100, c=big, g=2 ** 30 - 1, minus=1, delta=big - 100),
           hsp(far - 50, far, c=big, g=2 ** 30 - 1, minus=1, delta=0), hsp(far - 49, far, c=big, g=2 ** 30 - 1, minus=1),
           hsp(1, 99, delta=-2 ** 31), hsp(0, far, mism=7)]
    return raw, 28, 4


UNGAPPED = {
    "empty": u_empty, "single": u_single, "duplicates_only": u_duplicates_only,
    "nested_chain_of_five": u_nested_chain_of_five, "equal_b_different_e": u_equal_b_different_e,
    "equal_e_different_b": u_equal_e_different_b, "partial_overlaps_both_kept": u_partial_overlaps_both_kept,
    "container_below_min_score_still_drops": u_container_below_min_score_still_drops,
    "min_score_edge": u_min_score_edge, "negative_delta": u_negative_delta,
    "same_interval_in_separate_groups": u_same_interval_in_separate_groups,
}
for _n in (63, 64, 65, 255, 256, 257):
    UNGAPPED["group_of_{}".format(_n)] = lambda n=_n: u_group_of(n)
for _w in (1, 2, 3):
    UNGAPPED["field_extremes_{}_words".format(_w)] = lambda w=_w: u_field_extremes(w)


def side(pairs, matches=None, s_only=0, q_only=0):
    """(H, p, q, g) of one side: `pairs` aligned pairs of which `matches` match, and gap columns"""
    matches = pairs if matches is None else matches
    g = s_only + q_only
    return (6 * matches - 4 * pairs - 5 * g, pairs + s_only, pairs + q_only, g)


def anchor(i0, j0, left, right, c=0, g=0, minus=0):
    return (c, g, minus, i0, j0) + left + right


def aln(qstart, sstart, pairs, matches=None, s_only=0, q_only=0, **group):
    """an anchor at the alignment's start: its left side is empty"""
    return anchor(sstart, qstart, side(0), side(pairs, matches, s_only, q_only), **group)


def g_empty():
    return [], 28, 0, 0


def g_single():
    return [anchor(50, 150, side(40), side(40))], 28, 1, 1


def g_identical_from_four_anchors():
    # one alignment of subject [10, 110), contig [210, 310), reached from four anchors along it
    return [anchor(10 + k, 210 + k, side(k), side(100 - k)) for k in (20, 40, 60, 80)], 28, 1, 1


def g_coverer_itself_covered():
    # z covers y covers x, in score order z, y, x: y is dropped, and x all the same
    z = anchor(100, 300, side(100), side(100))
    y = anchor(100, 300, side(60), side(60))
    x = anchor(100, 300, side(30), side(30))
    return [x, y, z], 28, 1, 3


# Equal score2 (140), split by each later field of the order in turn.  A: contig [250, 350),
# subject [50, 150), 100 pairs of which 90 match.  (qspan, sspan, length) fix the pairs and the
# gaps, and score2 then fixes the matches: no two alignments differ first in matches or gaps.
_A = aln(250, 50, 100, 90)


def g_equal_score_split_by_qstart():
    # the other lies inside A and starts later on the contig: A is earlier and covers it
    return [aln(260, 60, 70), _A], 28, 1, 2


def g_equal_score_split_by_sstart():
    return [aln(250, 60, 70), _A], 28, 1, 2


def g_equal_score_split_by_qspan():
    # same starts, shorter on the contig: the other is earlier, so A, which covers it, is no kept
    # earlier one, and the other covers A not: both stay
    return [_A, aln(250, 50, 70)], 28, 2, 2


def g_equal_score_split_by_sspan():
    # contig [250, 350) as A, subject [50, 144): 94 pairs, 91 matches, 6 contig-only columns
    return [_A, aln(250, 50, 94, 91, q_only=6)], 28, 2, 2


def g_equal_score_split_by_length():
    # A's two intervals with one gap column either way: 99 pairs, 91 matches, length 101.  A is
    # earlier and covers it (cover is not strict)
    return [aln(250, 50, 99, 91, s_only=1, q_only=1), _A], 28, 1, 2


def g_twice_min_score_edge():
    # score2 55, 56, 57 on three contigs; 57 is the raw score 28.5
    return [aln(0, 0, 30, 30, q_only=1, c=0), aln(0, 0, 28, c=1), aln(0, 0, 31, 31, s_only=1, c=2)], 28, 2, 3


def g_half_score():
    # score2 201: 100.5
    return [aln(10, 20, 101, 101, q_only=1, minus=1)], 28, 1, 1


def g_separate_groups():
    # the same alignment on two strands, contigs and subjects, and a covered one in the first group
    raw = [aln(10, 20, 60, c=c, g=g, minus=m) for c in (0, 1) for g in (0, 1) for m in (0, 1)]
    return raw + [aln(15, 25, 40)], 28, 8, 9


def g_group_of(n):
    """One (subject, strand, contig) group of n alignments along a diagonal, none covering
    another, a covered one after every third, shuffled; one alignment in each neighbour group."""
    raw = [aln(3 * k, 3 * k, 50) for k in range(n)] + [aln(3 * k + 1, 3 * k + 1, 40) for k in range(0, n, 3)]
    random.Random(n).shuffle(raw)
    return raw + [aln(0, 0, 50, minus=1), aln(0, 0, 50, c=1)], 28, n + 2, n + (n + 2) // 3 + 2


def g_field_extremes(words):
    """Keys of 1 to 5 words (five: the int32 columns' ends); key_words counts them."""
    if words == 1:
        return [aln(0, 0, 40), aln(1, 1, 30), aln(2, 0, 40, c=1, g=1, minus=1)], 28, 2, 3
    if words < 5:
        m = {2: 10 ** 3, 3: 10 ** 6, 4: 6 * 10 ** 7}[words]
        raw = [aln(-m, -m, m, m - 5), aln(-m + 1, -m + 1, m - 2, m - 7), aln(m, m, 50, c=m, g=m, minus=1),
               aln(0, 0, m, m // 2, c=m, g=m, minus=1)]
        return raw, 28, 2, 4
    # two of negative score, one covered, two kept
    big, p = 2 ** 31 - 1, 2 ** 29
    raw = [aln(-2 ** 31, -2 ** 31, p, 0), aln(-2 ** 31 + 1, -2 ** 31 + 1, p - 2, 0),
           aln(0, 0, 2 * p - 2, 2 * p - 2, q_only=1, c=big, g=2 ** 30 - 1, minus=1),
           aln(2 ** 30 - 60, 2 ** 30 - 60, 50, c=big, g=2 ** 30 - 1, minus=1), aln(5, 5, 40)]
    return raw, 28, 2, 5


GAPPED = {
    "empty": g_empty, "single": g_single, "identical_from_four_anchors": g_identical_from_four_anchors,
    "coverer_itself_covered": g_coverer_itself_covered, "equal_score_split_by_qstart": g_equal_score_split_by_qstart,
    "equal_score_split_by_sstart": g_equal_score_split_by_sstart,
    "equal_score_split_by_qspan": g_equal_score_split_by_qspan,
    "equal_score_split_by_sspan": g_equal_score_split_by_sspan,
    "equal_score_split_by_length": g_equal_score_split_by_length, "twice_min_score_edge": g_twice_min_score_edge,
    "half_score": g_half_score, "separate_groups": g_separate_groups,
}
for _n in (63, 64, 65, 255, 256, 257):
    GAPPED["group_of_{}".format(_n)] = lambda n=_n: g_group_of(n)
for _w in (1, 2, 3, 4, 5):
    GAPPED["field_extremes_{}_words".format(_w)] = lambda w=_w: g_field_extremes(w)


def key_words(raw, gapped):
    """64-bit words of the first sort key the device form makes for `raw`: every field in the
    bits of its range in this set, as the stand-alone entry's pass over the input finds them"""
    import report_oracle as ro
    if gapped:
        rows = [ro.alignment(*r) for r in raw]
    else:
        rows = [(r[1] << 1 | r[2], r[0], r[3], r[4], r[5]) for r in raw]
    bits = sum((max(col) - min(col)).bit_length() for col in zip(*rows))
    return (bits + 63) // 64


# ---------------------------------------------------------------------------
# seeded random sets
# ---------------------------------------------------------------------------

def random_hsps(n, seed, groups, span=48):
    """n raw HSPs in `groups` groups, coordinates below `span`: most sets drop something.  The
    score is a function of (group, b, e), as it is for real HSPs."""
    rng = random.Random(seed)
    raw = []
    for _ in range(n):
        k = rng.randrange(groups)
        c, g, minus, delta = k % 3, (k // 3) % 5 + 5 * (k // 300), (k // 15) % 2, (k // 30) % 10 - 2
        b = rng.randrange(span - 1)
        e = rng.randrange(b + 1, span + 1)
        mism = (7 * b + 13 * e + k) % min(e - b + 1, 4)
        raw.append((c, g, minus, delta, b, e, (e - b) - 3 * mism))
    return raw


def random_anchors(n, seed, groups, span=40):
    rng = random.Random(seed)
    raw = []
    for _ in range(n):
        k = rng.randrange(groups)
        sides = []
        for _side in range(2):
            pairs = rng.randrange(span)
            s_only, q_only = rng.choice(((0, 0), (0, 0), (1, 0), (0, 1), (2, 1)))
            sides.append(side(pairs, pairs - rng.randrange(min(pairs + 1, 3)), s_only, q_only))
        raw.append(anchor(rng.randrange(span, 2 * span), rng.randrange(span, 2 * span), sides[0], sides[1],
                          c=k % 3, g=(k // 3) % 5 + 5 * (k // 30), minus=(k // 15) % 2))
    return raw
