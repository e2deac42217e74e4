"""The WAAFLE pipeline in one command: contigs, a gene database and a taxonomy to the three TSVs.

    python -m waafle_amd.workflow contigs.fna genes.wfdb|genes.fna taxonomy.tsv [flags]

The native search (waafle_amd.search --searcher native), the gene caller (waafle_amd.genecaller)
and the scorer (waafle_amd.orgscorer) with no text file between them: the search's records go
through `wf_hits_from_records` to the hit arrays on the device, and `wf_genecall`
and `wf_score` read those.  The three TSVs are byte for byte those of the three commands run one
after another with the same flags.  `--gff` takes user-supplied gene calls in place of the gene
caller; `--write-blastout` and `--write-gff` also write the files the first two commands would,
through their writers (for inspection: they cost what those writers cost).  `--order-on device`
puts the records in the table's order, applies `--max-target-seqs` and gathers their columns on
the GPU as well (`wf_order_records`); the files are the same.

One GPU (`--gpu`); no `--write-details`, no blastn searcher.  A contig name that occurs twice in
the FASTA is an error here, as for the native search.
"""
import argparse
import sys
import time

import numpy as np

from . import cli, engine, genecaller, hits, inputs, lib, mapper, output, search
from .taxonomy import TaxonomyTables, read_edges

SEARCH_SKIP = {"query", "db", "blastn", "threads", "out", "searcher", "help"}
SCORER_SKIP = {"contigs", "blastout", "gff", "taxonomy", "write_details", "gpus", "help"}


def _adopt(parser, source, skip):
    """Every argument of `source` (a parser) but those whose dest is in `skip`, in its groups:
    names, types, defaults and help are those of the command they come from."""
    for grp in source._action_groups:
        acts = [a for a in grp._group_actions if a.dest not in skip]
        if acts:
            g = parser.add_argument_group(grp.title, grp.description)
            for a in acts:
                g._add_action(a)


def build_parser():
    ap = argparse.ArgumentParser(
        description="WAAFLE in one command on the GPU: native search, gene calls and contig scoring,\n"
                    "with no text file between the steps.",
        formatter_class=argparse.RawTextHelpFormatter)
    ap.add_argument("contigs", help="contigs file (fasta format)")
    ap.add_argument("db", help="the genes: a .wfdb file (python -m waafle_amd.makedb) or a FASTA file\n"
                               "with WAAFLE headers (id|taxon|system=name...)")
    ap.add_argument("taxonomy", help="taxonomy file of the gene database")
    ap.add_argument("--gff", default=None, metavar="<path>",
                    help="user-supplied gene calls for <contigs> (.gff), in place of the gene caller")
    ap.add_argument("--write-blastout", default=None, metavar="<path>",
                    help="also write the table `waafle_amd.search` would write")
    ap.add_argument("--write-gff", default=None, metavar="<path>",
                    help="also write the gene calls `waafle_amd.genecaller` would write")
    _adopt(ap, search.build_parser(), SEARCH_SKIP)
    _adopt(ap, cli.build_parser(), SCORER_SKIP)
    return ap


def die(*args):
    inputs.say(*(["LETHAL ERROR:"] + list(args)))
    sys.exit("EXITING.")


def run(args, say):
    """The flow of DESIGN.md §13; returns the phase walls in seconds."""
    walls, t = {}, time.time()

    def lap(name):
        nonlocal t
        walls[name] = time.time() - t
        t = time.time()

    edges = read_edges(args.taxonomy)
    names, seq, off = mapper.read_fasta(args.contigs)
    qlen = np.diff(off)
    gapped = bool(args.gapped)
    found = dict(
        device=args.gpu, chunk_bases=args.chunk_bases, say=say, gapped=gapped,
        band=args.band, xdrop_gap=args.xdrop_gap, dust=args.dust, dust_window=args.dust_window,
        dust_level=args.dust_level, dust_out=args.dust_out, seed_length=args.seed_length,
        seed_stride=args.seed_stride, max_seed_hits=args.max_seed_hits, xdrop=args.xdrop, min_score=args.min_score,
        report_on=args.report_on)
    if args.order_on == "device":
        # wf_order_records with gathering, on the searcher's context before it closes
        rec, ids, lens, stats, (order, cols) = search.search_ordered(
            names, seq, off, args.db, args.max_target_seqs, order_on="device", gather=True,
            before_order=lambda: lap("search"), **found)
    else:
        rec, ids, lens, stats = search.search_records(names, seq, off, args.db, **found)
        lap("search")
        order = search.order_records(rec, args.max_target_seqs)
        cols = hits.record_columns(rec, order)
    lap("order")
    if args.write_blastout:
        rows = search.format_rows(rec, order, names, qlen, ids, lens, int(lens.sum()))
        with open(args.write_blastout, "w") as fh:
            fh.write("".join(r + "\n" for r in rows))
        lap("write_blastout")
    n, N = len(order), len(names)
    subjects = hits.subject_tables(ids, np.unique(cols["subject"]))
    tax = TaxonomyTables(edges, extra_names={t for t in subjects.taxa if t is not None})
    say("Analyzing {:,} contigs ({:,} hits from {:,} subjects).".format(N, n, len(ids)))
    params = cli.param_dict(args)
    scorer = engine.GpuScorer(args.gpu)
    d = {}
    try:
        scorer.set_taxonomy(tax)
        d = hits.hits_device(scorer.lib, scorer.h, cols, qlen, lens, subjects.taxon_ids(tax), subjects.sysmask,
                             args.min_scov, hits.hip_runtime(args.gpu))
        hit_off = d["hit_off"].host()
        lap("hits")
        genes = None
        if args.gff is None or args.write_gff:
            genes = hits.gene_lists(hit_off, *hits.genecall_device(
                scorer.lib, scorer.h, d, N, n, args.min_overlap, args.min_scov, args.min_gene_length))
            if args.write_gff:
                genecaller.write_gff(genecaller.GeneCalls([names[c] for c, _ in genes], [gl for _, gl in genes]),
                                     args.write_gff)
        if args.gff is None:
            loci = hits.loci_from_genes(genes, args.min_gene_length)
        else:
            loci = inputs.read_loci(args.gff, {nm: i for i, nm in enumerate(names)}, args.min_gene_length,
                                    warn=inputs.say)
        batch = hits.make_batch(names, qlen, hit_off, loci, subjects, cols["subject"])
        lap("genes")
        res = hits.score_device(scorer, batch, d, params)
        lap("score")
    finally:
        for a in d.values():
            a.free()
        scorer.close()
    say("Initializing outputs.")
    output.write(output.render(batch, tax, res), args.outdir, args.basename)
    lap("write")
    return walls, batch, stats


def main(argv=None):
    args = build_parser().parse_args(argv)
    say = (lambda *a: None) if args.quiet else inputs.say
    if args.max_target_seqs < 1 or args.chunk_bases < 1:
        die("--max-target-seqs and --chunk-bases must be positive")
    if args.dust_out and not args.dust:
        die("--dust-out needs --dust")
    if args.basename is None:
        args.basename = inputs.basename_of(args.contigs)
    try:
        walls, batch, _ = run(args, say)
    except lib.WaafleHipError as exc:
        if exc.code == lib.WF_E_RUNAWAY and len(getattr(exc, "contigs", ())):
            die("  Warning: Runaway taxonomic recursion for",
                mapper.read_fasta(args.contigs)[0][int(exc.contigs[0])])
        die(str(exc))
    except (inputs.InputError, ValueError, OSError) as exc:
        die(str(exc))
    say("Finished successfully ({:,} contigs, {:,} hits, {:,} loci; {}).".format(
        batch.n_contigs, batch.n_hits, batch.n_loci,
        ", ".join("{} {:.3f}s".format(k, v) for k, v in walls.items())))


if __name__ == "__main__":
    main()
