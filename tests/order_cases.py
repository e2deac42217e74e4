"""Record sets for the table's order and --max-target-seqs, built by hand with
the number of kept records written down per limit, and the seeded random sets.

A case is (records, [(max_target_seqs, n_kept), ...]); records as search.order_records takes
them: {field: numpy array}, search.RECORD_FIELDS, or GAP_RECORD_FIELDS for the gapped kind.
An ungapped row is (contig, subject, minus, qstart, sstart, length, matches); its score is
3 matches - 2 length.  `gapped_form` gives the same rows as gapped records (qspan = sspan =
length, no gaps: twice the score, so the same order)."""
import numpy as np

from waafle_amd import search

BIG = 2 ** 31 - 1
LONG = 2 ** 30
NO_LIMIT = (10000, 2 ** 40)


def ungapped(rows):
    cols = list(zip(*rows)) if rows else [[] for _ in search.RECORD_FIELDS]
    return {f: np.array(c, dtype=dt) for (f, dt), c in zip(search.RECORD_FIELDS, cols)}


def gapped(rows):
    """rows: (contig, subject, minus, qstart, qspan, sstart, sspan, length, matches, gaps)"""
    cols = list(zip(*rows)) if rows else [[] for _ in search.GAP_RECORD_FIELDS]
    return {f: np.array(c, dtype=dt) for (f, dt), c in zip(search.GAP_RECORD_FIELDS, cols)}


def gapped_form(rec):
    out = {f: rec[f if f in rec else "length"].astype(dt) for f, dt in search.GAP_RECORD_FIELDS if f != "gaps"}
    out["gaps"] = np.zeros(len(rec["contig"]), np.int32)
    return {f: out[f] for f, _ in search.GAP_RECORD_FIELDS}


def permuted(rec, perm):
    return {f: a[np.asarray(perm, np.int64)] for f, a in rec.items()}


def empty():
    """No record."""
    return ungapped([]), [(1, 0), (10000, 0)]


def single():
    """One record."""
    return ungapped([(3, 4, 1, 5, 6, 40, 38)]), [(1, 1), (2 ** 40, 1)]


def one_contig():
    """One contig holds everything: subjects 5, 2, 9 with best scores 100, 80, 50 and two
    records each.  Limits 1, the subject count minus one, the count, and no limit."""
    rows = [(0, 5, 0, 0, 0, 100, 100), (0, 5, 0, 200, 0, 50, 50), (0, 2, 1, 10, 3, 80, 80), (0, 9, 0, 7, 7, 80, 70),
            (0, 2, 0, 90, 5, 30, 30), (0, 9, 1, 60, 1, 20, 20)]
    return ungapped(rows), [(1, 2), (2, 4), (3, 6), (10000, 6), (2 ** 40, 6)]


def own_contigs():
    """Every record its own contig, given in descending contig order: no limit can drop one."""
    rows = [(c, 7, 0, c, 2 * c, 30 + c, 30) for c in (4, 3, 2, 1, 0)]
    return ungapped(rows), [(1, 5), (10000, 5)]


def contigs_without_records():
    """Contigs 0, 1, 3, 4, 6, 7 have no record: before, between and after those of 2 and 5."""
    rows = [(5, 1, 0, 0, 0, 40, 40), (2, 8, 0, 0, 0, 40, 39), (5, 0, 0, 9, 9, 40, 36), (2, 8, 1, 50, 0, 33, 33),
            (2, 3, 0, 0, 0, 60, 60)]
    return ungapped(rows), [(1, 2), (2, 5), (10000, 5)]


def tied_best():
    """Subjects 7 and 3 tie on best (60) and subject 1 has 40: the ranks are 3, 7, 1.  At limit 1
    the tie straddles the cut and the lower subject stays; at 2 both tied ones stay."""
    rows = [(0, 7, 0, 0, 0, 60, 60), (0, 1, 0, 0, 0, 40, 40), (0, 3, 0, 5, 5, 60, 60), (0, 7, 0, 100, 0, 20, 20),
            (0, 3, 1, 70, 0, 25, 25), (0, 3, 0, 300, 0, 10, 10)]
    return ungapped(rows), [(1, 3), (2, 5), (3, 6), (10000, 6)]


def tied_best_in_every_contig():
    """Three contigs, each with two subjects tied on best and one behind; the lower subject wins:
    4, 4 and 5, with 1, 2 and 2 records."""
    rows = []
    for c, (a, b, z) in enumerate([(4, 9, 0), (9, 4, 2), (6, 5, 7)]):
        rows += [(c, a, 0, 0, 0, 50, 50), (c, b, 0, 0, 0, 50, 50), (c, z, 0, 0, 0, 50, 45), (c, b, 1, 9, 9, 20, 20)]
    return ungapped(rows), [(1, 5), (2, 9), (3, 12), (10000, 12)]


def later_keys():
    """Seven records of one contig with one score, split by subject, minus, qstart and sstart in
    turn, out of order in the input."""
    rows = [(0, 1, 0, 10, 11, 50, 50), (0, 2, 0, 10, 10, 50, 50), (0, 1, 1, 10, 10, 50, 50), (0, 1, 0, 10, 10, 50, 50),
            (0, 1, 0, 11, 10, 50, 50), (0, 1, 1, 9, 10, 50, 50), (0, 1, 0, 11, 9, 50, 50)]
    return ungapped(rows), [(1, 6), (2, 7), (10000, 7)]


def later_keys_gapped():
    """As later_keys, then split by qspan and by sspan alone (gapped records only)."""
    rows = [(0, 1, 0, 10, 52, 10, 51, 55, 50, 2), (0, 1, 0, 10, 51, 10, 52, 55, 50, 2),
            (0, 1, 0, 10, 51, 10, 51, 55, 50, 2), (0, 1, 0, 10, 52, 10, 50, 55, 50, 2),
            (0, 2, 0, 10, 50, 10, 50, 55, 50, 2), (0, 1, 1, 10, 50, 10, 50, 55, 50, 2),
            (0, 1, 0, 9, 60, 10, 60, 55, 50, 2), (0, 1, 0, 10, 50, 9, 60, 55, 50, 2)]
    return gapped(rows), [(1, 7), (2, 8), (10000, 8)]


def gaps_in_the_score():
    """Gapped records whose scores differ by their gap columns alone: 6 m - 4 length - gaps."""
    rows = [(0, 1, 0, 0, 50, 0, 50, 52, 50, 3), (0, 2, 0, 0, 50, 0, 50, 52, 50, 1), (0, 3, 0, 0, 50, 0, 50, 52, 50, 2),
            (1, 3, 0, 0, 50, 0, 50, 52, 50, 0)]
    return gapped(rows), [(1, 2), (2, 3), (3, 4), (10000, 4)]


def duplicates():
    """The same record four times among others, and a second one twice: the input position
    decides."""
    a, b = (1, 3, 0, 5, 5, 40, 40), (1, 2, 1, 0, 0, 40, 40)
    rows = [a, (0, 3, 0, 5, 5, 40, 40), a, b, (1, 3, 0, 5, 5, 41, 40), a, b, a]
    return ungapped(rows), [(1, 3), (2, 8), (10000, 8)]


def negative_scores():
    """matches 0: the scores are -2 length, and the shortest is the best."""
    rows = [(0, 4, 0, 0, 0, 50, 0), (0, 6, 0, 0, 0, 30, 0), (0, 4, 0, 9, 9, 20, 0), (0, 8, 0, 0, 0, 20, 0),
            (0, 9, 0, 0, 0, 25, 20), (1, 1, 0, 0, 0, 1000, 0)]
    return ungapped(rows), [(1, 2), (2, 4), (3, 5), (4, 6), (10000, 6)]


def extreme():
    """length 2^30 with matches 0 and with matches = length; contig and subject 2^31 - 1.  At
    limit 1 the order is [1, 2]: in contig 2^31 - 1 the subjects tie on best and 0 wins."""
    rows = [(BIG, BIG, 0, 0, 0, LONG, LONG), (0, 5, 0, 0, 0, LONG, 0), (BIG, 0, 0, 0, 0, LONG, LONG)]
    return ungapped(rows), [(1, 2), (2, 3), (2 ** 40, 3)]


EXTREME_ORDER_AT_1 = [1, 2]


def extreme_scores():
    """One contig with scores from -2^31 (matches 0) to 2^30 (all matches) at length 2^30, and
    short records between; int32 holds neither the scores' range nor 6 matches."""
    rows = [(7, 1, 0, 0, 0, LONG, 0), (7, 2, 0, 0, 0, LONG, LONG), (7, 3, 0, 0, 0, 40, 40), (7, 1, 1, 0, 0, 40, 0),
            (7, BIG, 1, BIG, BIG, LONG, LONG), (7, 3, 0, 0, 0, LONG, LONG - 1)]
    return ungapped(rows), [(1, 1), (2, 2), (3, 4), (4, 6), (10000, 6)]


UNGAPPED = dict(empty=empty, single=single, one_contig=one_contig, own_contigs=own_contigs,
                contigs_without_records=contigs_without_records, tied_best=tied_best,
                tied_best_in_every_contig=tied_best_in_every_contig, later_keys=later_keys, duplicates=duplicates,
                negative_scores=negative_scores, extreme=extreme, extreme_scores=extreme_scores)
GAPPED_ONLY = dict(later_keys_gapped=later_keys_gapped, gaps_in_the_score=gaps_in_the_score)


def _as_gapped(fn):
    def case():
        rec, limits = fn()
        return gapped_form(rec), limits
    case.__doc__ = fn.__doc__
    return case


HAND_BUILT = dict(UNGAPPED)
HAND_BUILT.update({name + "_gapped_form": _as_gapped(fn) for name, fn in UNGAPPED.items()})
HAND_BUILT.update(GAPPED_ONLY)


def distinct_records():
    """40 records without two equal in every key, in sorted order (a list of rows), over 4 contigs
    and 6 subjects with many score ties: the same table whatever the input order."""
    rng = np.random.RandomState(5)
    rows = set()
    while len(rows) < 40:
        rows.add((int(rng.randint(4)), int(rng.randint(6)), int(rng.randint(2)), int(rng.randint(3)),
                  int(rng.randint(3)), 40, int(rng.randint(38, 41))))
    return sorted(rows)


# ---- seeded random sets -----------------------------------------------------------------------

def random_set(seed, n, n_contigs, n_subjects, gapped_kind=False, spread=3):
    """n records with heavy ties: contigs and subjects uniform, lengths and matches from `spread`
    values each, starts from `spread`, so pairs tie on best and records on every key."""
    rng = np.random.RandomState(seed)
    rec = dict(contig=rng.randint(0, n_contigs, n), subject=rng.randint(0, n_subjects, n),
               minus=rng.randint(0, 2, n), qstart=rng.randint(0, spread, n), sstart=rng.randint(0, spread, n),
               length=40 + rng.randint(0, spread, n), matches=36 + rng.randint(0, spread, n))
    if gapped_kind:
        rec.update(qspan=rec["length"] - rng.randint(0, spread, n), sspan=rec["length"] - rng.randint(0, spread, n),
                   gaps=rng.randint(0, spread, n))
    fields = search.GAP_RECORD_FIELDS if gapped_kind else search.RECORD_FIELDS
    return {f: rec[f].astype(dt) for f, dt in fields}


def small_random_sets(count=200, seed=1234):
    """(records, limit): `count` sets of 0..300 records, both kinds, at limits 1, 2, 3, 10000 and
    2^40 in turn."""
    rng = np.random.RandomState(seed)
    for k in range(count):
        n = int(rng.randint(0, 301))
        rec = random_set(int(rng.randint(1 << 30)), n, int(rng.randint(1, 6)), int(rng.randint(1, 9)), k % 2 == 1,
                         spread=int(rng.randint(1, 4)))
        yield rec, (1, 2, 3, 10000, 2 ** 40)[k % 5]
