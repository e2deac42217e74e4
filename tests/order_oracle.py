"""The table's order and --max-target-seqs in plain Python: form B of the rule
that search.order_records (form A, numpy) defines.  No numpy sort: a dict for each pair's best
score, a per-contig `sorted` of (-best, subject), and `sorted` over tuple keys that end in the
input position."""

COLUMNS = ("contig", "subject", "minus", "qstart", "qspan", "sstart", "sspan", "length", "matches")


def _ints(a):
    return a.tolist() if hasattr(a, "tolist") else [int(v) for v in a]


def scores(rec):
    """Python ints: 3 matches - 2 length, or for gapped records 6 matches - 4 length - gaps."""
    m, length = _ints(rec["matches"]), _ints(rec["length"])
    if "gaps" in rec:
        return [6 * a - 4 * b - g for a, b, g in zip(m, length, _ints(rec["gaps"]))]
    return [3 * a - 2 * b for a, b in zip(m, length)]


def order(rec, max_target_seqs):
    """The input indices of the kept records, in the table's order (a list of ints)."""
    contig, subject, score = _ints(rec["contig"]), _ints(rec["subject"]), scores(rec)
    best = {}
    for pair, s in zip(zip(contig, subject), score):
        if pair not in best or s > best[pair]:
            best[pair] = s
    by_contig = {}
    for (c, g), b in best.items():
        by_contig.setdefault(c, []).append((-b, g))
    kept = set()
    for c, pairs in by_contig.items():
        for rank, (_, g) in enumerate(sorted(pairs)):
            if rank < max_target_seqs:
                kept.add((c, g))
    later = [_ints(rec[f]) for f in ("minus", "qstart", "sstart")]
    if "gaps" in rec:
        later += [_ints(rec["qspan"]), _ints(rec["sspan"])]
    keys = []
    for i, (c, g, s) in enumerate(zip(contig, subject, score)):
        if (c, g) in kept:
            keys.append((c, -s, g) + tuple(col[i] for col in later) + (i,))
    return [k[-1] for k in sorted(keys)]


def columns(rec, idx):
    """The nine wf_hit_records columns of the records `idx`, as lists (an ungapped record has
    qspan = sspan = length)."""
    src = {f: _ints(rec[f] if f in rec else rec["length"]) for f in COLUMNS}
    return {f: [src[f][i] for i in idx] for f in COLUMNS}
