/*
 * waafle_hip.h -- C-ABI of libwaafle_hip.so, the MI355X (gfx950) implementation of the
 * waafle_orgscorer contig-scoring hot path.
 *
 * The reference (menickname/waafle v0.1.0, pure Python + numpy) has no FFI; its
 * in-process seam is the per-contig loop of `waafle/waafle_orgscorer.py:943-960`
 * (attach_hits -> update_gene_scores -> [jump_taxonomy] -> evaluate_contig).  One
 * wf_score() call replaces that loop for a whole batch of contigs.  The host side
 * (Python, ctypes) parses the four input files, interns taxa, packs the flat arrays
 * below and renders the three TSVs from the result records.
 *
 * Conventions: plain pointers + sizes, no ownership transfer (every buffer is owned by
 * the caller and only borrowed for the duration of the call), 0 = success and a
 * negative WF_E_* code otherwise with the message in wf_last_error(ctx), no exceptions
 * and no exit() inside the library.  One wf_ctx per device; distinct contexts may be
 * used from different host threads concurrently; a context is not re-entrant.
 */
#ifndef WAAFLE_HIP_H
#define WAAFLE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WF_ABI_VERSION 6   /* 4: WF_OPT_SPARSE_BIG 0/1 retired, WF_PHASE_ROLLUP, WF_OPT_WAVE_TWO / _DUMP_CAP;
                                 5: WF_OPT_TRIAGE, WF_PHASE_TRIAGE;
                                 6: wf_batch.hit_key (packed hit record), wf_pack_hit_keys;
                                    WF_OPT_WAVE_TWO 0 (the round-3 hand-over flow) retired;
                                    still 6 (additive): wf_map_index, wf_map_pairs;
                                    still 6 (additive): wf_map_pairs_gapped;
                                    still 6 (additive): wf_search, wf_search_gapped;
                                    still 6 (additive): wf_search_mask;
                                    still 6 (additive): wf_search_packed, wf_search_gapped_packed,
                                                        wf_search_chunk_planes;
                                    still 6 (additive): wf_hits_from_records;
                                    still 6 (additive): wf_order_records;
                                    still 6 (additive): WF_OPT_SEARCH_REPORT, wf_search_report,
                                                        wf_search_report_gapped */

enum wf_status {
  WF_OK = 0,
  WF_E_BADINPUT = -1,  /* malformed arguments (sizes, null pointers, limits) */
  WF_E_HIP = -2,       /* a HIP runtime call failed */
  WF_E_RUNAWAY = -3,   /* > 100 roll-up iterations: orgscorer.py:580-581 */
  WF_E_NOMEM = -4,     /* per-contig workspace too small (see wf_result.need_bytes) */
  WF_E_STATE = -5,     /* call order (e.g. wf_score before wf_set_taxonomy) */
  WF_E_EMPTYMASK = -6, /* every locus masked at a roll-up level (np.min of empty) */
  WF_E_TOOBIG = -7     /* the hit-locus attachments the staged kernels would hold in HBM
                          (the contigs the wave forms hand them; every contig in
                          WF_MODE_STAGED) exceed one call's limit (WF_OPT_ATT_LIMIT, at
                          most 2^31 - 1): score the batch in parts */
};

enum wf_call { WF_CALL_UNCLASSIFIED = 0, WF_CALL_NO_LGT = 1, WF_CALL_LGT = 2 };

/* Execution form of wf_score (the results are identical).
 * WF_MODE_LEVEL0 (default): per-contig wave kernels carry level 0 in LDS (explain_one in
 *   the wave; explain_two from the segment table it hands over, k_dump_sparse), and every
 *   roll-up level is one more launch of the same wave form over the contigs the level before
 *   raised.  Only contigs that exceed a wave's LDS slice (attachments,
 *   loci, leaf tables) or the hand-over tables continue in the second wave form and then
 *   the staged kernels.
 * WF_MODE_WAVES: the second (FULL) wave form carries explain_two and the roll-up levels in
 *   its LDS slice.
 * WF_MODE_STAGED: every contig through the staged kernels (one kernel per phase over all
 *   contigs: attachments, per-contig sort, segment means, decisions; one pass per level).
 * The ABI-1 WF_MODE_FUSED form (1) stays retired; wf_set_mode rejects it. */
enum wf_mode { WF_MODE_STAGED = 0, WF_MODE_LEVEL0 = 2, WF_MODE_WAVES = 3 };

/* Context options (wf_set_option); every one leaves the results unchanged.
 * WF_OPT_SPARSE_BIG: the decision form of the staged kernels for contigs of <= 63 loci.
 *   3 (default): explain_one by one wave per contig (k_one), and every contig it leaves
 *   open (explain_two, more segments than its LDS holds, --weak-loci assign-unknown) takes
 *   the decision straight from the segment table, one wave per contig (k_big_sparse);
 *   2: every staged decision in the segment-table form (a test setting: it exercises that
 *   form on every input).  The dense matrix decision remains for > 63 loci and for a table
 *   the segment-table form declines (its class or pair tables outgrown).  The values 0 and 1
 *   (dense decisions for <= 63 loci) are retired: WF_E_BADINPUT.
 * WF_OPT_ATT_LIMIT: hit-locus attachments the staged kernels accept in one wf_score call
 *   (default and maximum 2^31 - 1; more -> WF_E_TOOBIG and the call's records are not
 *   valid: score the batch in parts).  The wave forms hold a contig's attachments in LDS.
 * WF_OPT_WAVE_TWO (WF_MODE_LEVEL0): the first wave form also prepares explain_two (up to 64
 *   potential clades, <= 63 loci) and carries the roll-up levels, one pass per level over
 *   the contigs still open; the rest goes to the segment-table decision (k_dump_sparse).
 *   2 (default): a contig whose potential clades form no candidate pair is raised or stopped
 *   by the wave itself, with no table; the others hand a compact table to k_dump_sparse.
 *   1: every such contig hands its compact table over (a test setting, and the same-build
 *   comparison arm).  0 (every explain_two contig to the whole-table decision and the roll-up
 *   levels in the staged kernels: the round-3 flow) is retired: WF_E_BADINPUT.
 * WF_OPT_DUMP_CAP: segment-table entries of the wave form's hand-over buffer (default
 *   max(32 * contigs, 65536)); contigs past it go to the staged kernels (a test setting).
 * WF_OPT_TRIAGE (WF_MODE_LEVEL0 / _WAVES): 1 (default) a level-0 triage kernel first decides
 *   the contigs explain_one settles from the clades present on every locus (one-run gene
 *   scores), without the wave form's sort and segment table; the wave form runs the rest.
 *   0: the wave form runs every contig (a test setting: it exercises that path on every
 *   input).
 * WF_OPT_SEARCH_REPORT: where the reporting step of the four search calls and of
 *   wf_search_report / wf_search_report_gapped runs: 0 (default) on the host,
 *   1 on the device; the same records, counters and statuses either way.
 */
enum wf_option { WF_OPT_SPARSE_BIG = 1, WF_OPT_ATT_LIMIT = 2, WF_OPT_WAVE_TWO = 3, WF_OPT_DUMP_CAP = 4,
                 WF_OPT_TRIAGE = 5, WF_OPT_SEARCH_REPORT = 6 };

typedef struct wf_ctx wf_ctx;

/* Interned taxonomy.  Ids are the ranks of all names (taxonomy file names, hit taxa,
 * "r__Root", "Unknown") in Python code-point order, so `clade1 < clade2`
 * (orgscorer.py:608) is an integer compare.  Replaces utils.py:374-447. */
typedef struct wf_taxonomy {
  int32_t n;                  /* number of names */
  const int32_t* parent;      /* [n] Taxonomy.get_parent (utils.py:386-387) */
  const int32_t* depth;       /* [n] len(Taxonomy.get_lineage) - 1 (utils.py:392-399) */
  const int32_t* sib_parent;  /* [n] parent the name is listed under as a child in the
                                 taxonomy file (children map, utils.py:382), or -1 */
  const int64_t* leaf_count;  /* [n] Taxonomy.get_leaf_count (utils.py:436-447) */
  int32_t root;               /* id of "r__Root" (utils.py:368) */
  int32_t unknown;            /* id of "Unknown" (utils.py:367) */
} wf_taxonomy;

/* orgscorer.py:135-303 + genecaller.py:81-101 (enums in the choice order shown). */
typedef struct wf_params {
  double k1;                  /* -k1 / --one-clade-threshold */
  double k2;                  /* -k2 / --two-clade-threshold */
  double range;               /* --range */
  double min_overlap;         /* --min-overlap */
  double min_scov;            /* --min-scov */
  double ambiguous_fraction;  /* --ambiguous-fraction */
  int32_t disambiguate_one;   /* 0 report-best, 1 meld */
  int32_t disambiguate_two;   /* 0 report-best, 1 jump, 2 meld */
  int32_t jump_taxonomy;      /* 0 = off (None) */
  int32_t allow_lca;          /* --allow-lca */
  int32_t ambiguous_threshold;/* 0 off, 1 lenient, 2 strict */
  int32_t sister_penalty;     /* 0 off, 1 lenient, 2 strict */
  int32_t clade_genes;        /* -1 = off (None) */
  int32_t clade_leaves;       /* -1 = off (None) */
  int32_t weak_loci;          /* 0 ignore, 1 penalize, 2 assign-unknown */
  int32_t annotation_threshold; /* 0 off, 1 lenient, 2 strict */
  int32_t stranded;           /* --stranded */
} wf_params;

/* A batch of contigs in CSR form.  Contig c owns hits [hit_off[c], hit_off[c+1]) in
 * blastout file order (utils.py:255-270) and loci [loc_off[c], loc_off[c+1]) -- the
 * loci that passed --min-gene-length, in GFF order (orgscorer.py:348-352). */
typedef struct wf_batch {
  int32_t n_contigs;
  int32_t n_systems;          /* annotation systems (<= 32); bit s of hit_sysmask */
  int64_t n_hits;
  int64_t n_loci;
  int32_t max_hits;           /* max hits of one contig (workspace sizing) */
  int32_t max_loci;           /* max loci of one contig */
  int32_t device_resident;    /* 1: all pointers (batch and result) are device memory
                                 and wf_score only enqueues on the context stream;
                                 0: host memory, wf_score copies and synchronises */
  int32_t _pad;
  const int64_t* hit_off;     /* [n_contigs+1] */
  const int32_t* hit_qlo;     /* [n_hits] min(qstart, qend)  (utils.py:173-174) */
  const int32_t* hit_qhi;     /* [n_hits] max(qstart, qend) */
  const int32_t* hit_taxon;   /* [n_hits] taxon id = sseqid.split("|")[1] (utils.py:234-235) */
  const int8_t*  hit_strand;  /* [n_hits] 0 '+', 1 '-' (sstrand, utils.py:214) */
  const double*  hit_score;   /* [n_hits] waafle_score (utils.py:229) */
  const double*  hit_scov;    /* [n_hits] scov_modified (utils.py:227) */
  const uint32_t* hit_sysmask;/* [n_hits] annotation systems present (utils.py:237-241) */
  const int64_t* loc_off;     /* [n_contigs+1] */
  const int32_t* loc_start;   /* [n_loci] GFF start */
  const int32_t* loc_end;     /* [n_loci] GFF end */
  const int8_t*  loc_strand;  /* [n_loci] 0 '+', 1 '-', 2 anything else */
  /* Optional (NULL: the library packs it on the device, one extra pass over the hits): the
     hit's filter fields packed in one word, wf_pack_hit_keys' layout -- bits 0-23 hit_taxon,
     bit 24 hit_scov >= params.min_scov (the attach_hits filter, orgscorer.py:363-364: it
     must be packed with the min_scov of the wf_score call it is passed to), bit 25
     hit_strand '-', bits 26-31 hit_sysmask & 63 (systems 0-5; also when n_systems is 0, from
     the library's own packer too).  The level-0 triage, the
     kernel of most contigs, then reads 20 bytes per hit (qlo, qhi, key, score) instead of
     32.  The other arrays stay required (the other kernels read them). */
  const uint32_t* hit_key;    /* [n_hits] */
} wf_batch;

/* Per-contig results (caller-allocated, same residency as the batch). */
typedef struct wf_result {
  int8_t*  call;              /* [n] wf_call: routing of orgscorer.py:838-890 */
  double*  crit;              /* [n] min (max) score of the reported option */
  double*  rank;              /* [n] avg (max) score of the reported option */
  int32_t* clade1;            /* [n] reported clade / clade_A (after melding) */
  int32_t* clade2;            /* [n] clade_B (lgt only) */
  int8_t*  direction;         /* [n] 0 "A?B", 1 "B>A" */
  int16_t* iterations;        /* [n] roll-up iterations performed (1 = none) */
  uint8_t* synteny;           /* [n_loci] synteny characters, CSR by loc_off */
  int32_t* n_meld1;           /* [n] melded clades for clade1 (tails), 0 = none */
  int32_t* n_meld2;           /* [n] melded clades for clade2 */
  int32_t* meld;              /* [2*n_hits + 2*n]; contig c writes its meld1 ids then its
                                 meld2 ids from 2*hit_off[c] + 2*c */
  int32_t* annot_hit;         /* [n_loci * n_systems] batch hit index whose annotation
                                 the locus keeps (orgscorer.py:384-392), or -1 */
  int64_t* pair_evals;        /* [n] sum of P_pot*(P_pot-1)/2 over explain_two calls */
  int32_t* status;            /* [n] 0 or a WF_E_* code for this contig */
  int64_t* need_bytes;        /* [n] workspace bytes asked for when status == WF_E_NOMEM */
  int64_t* ppot_sum;          /* [n] optional (NULL: not reported): sum of P_pot over the
                                 explain_two calls that evaluate pairs (P_pot >= 2), one per
                                 roll-up level -- the per-call sizes behind pair_evals, for
                                 SURVEY 8(d)'s B_k2 = sum P_pot * G * 8 (ABI 6) */
} wf_result;

/* Pass timing accumulated while enabled: HIP events recorded on the context stream
 * around every kernel of each wf_score pass. */
enum wf_phase {
  WF_PHASE_WAVES = 0,         /* wave kernels: level 0, explain_one / explain_two in LDS */
  WF_PHASE_ATTACH = 1,        /* staged: attachment counts, offsets, attachments */
  WF_PHASE_SEGMENTS = 2,      /* staged, per level: sort, segments, exact segment means */
  WF_PHASE_DECIDE = 3,        /* staged, per level: k_one + k_decide (LDS arena) */
  WF_PHASE_BIG = 4,           /* staged, per level: k_big_sparse + k_decide_big */
  WF_PHASE_HANDOVER = 5,      /* level 0 of the contigs the wave kernels hand over with
                                 their segment tables (k_dump_sparse) */
  WF_PHASE_ROLLUP = 6,        /* roll-up levels 1, 2, ... in the first wave form (with their
                                 hand-overs), WF_OPT_WAVE_TWO 1 or 2 */
  WF_PHASE_TRIAGE = 7,        /* the level-0 triage kernel and the list of contigs it hands
                                 on (WF_OPT_TRIAGE 1); WF_PHASE_WAVES is then the first wave
                                 form's launch over that list */
  WF_N_PHASES = 8
};
typedef struct wf_timing {
  double pass_ms;             /* sum over timed passes */
  int64_t passes;             /* number of wf_score calls timed */
  double phase_ms[WF_N_PHASES];       /* per wf_phase, summed over timed passes */
  int64_t phase_spans[WF_N_PHASES];   /* timed spans (one per phase and level) */
} wf_timing;

/* ---- waafle_genecaller (waafle_genecaller.py:107-233) -------------------------------
 * Gene calls from one blastout: per contig group (a run of consecutive rows with the same
 * qseqid, utils.py:255-270), hits with scov_modified >= min_scov become intervals, the
 * connected components of overlapping intervals (calc_overlap >= min_overlap) are merged
 * (min start, max stop, strand of the longest member, ties to '-'), and merged genes of
 * length >= min_gene_length are returned in component order.  Replaces the per-contig
 * hits2ints / overlap_intervals / merge_inodes calls of the reference's main loop. */
typedef struct wf_gc_batch {
  int32_t n_groups;           /* contig groups, blastout order */
  int32_t device_resident;    /* 1: device pointers (enqueue only); 0: host arrays */
  int64_t n_hits;
  const int64_t* hit_off;     /* [n_groups + 1] hit range of each group */
  const int32_t* hit_qlo;     /* [n_hits] qstart / qend, either order */
  const int32_t* hit_qhi;
  const int8_t* hit_strand;   /* 0 '+', 1 '-' (sstrand "minus", utils.py:214) */
  const double* hit_scov;     /* scov_modified (utils.py:227) */
} wf_gc_batch;

typedef struct wf_gc_params {
  double min_overlap;         /* --min-overlap, default 0.1 */
  double min_scov;            /* --min-scov, default 0.75 */
  double min_gene_length;     /* --min-gene-length, default 200 */
  int32_t stranded;           /* accepted, no effect: dead upstream (genecaller.py:212-215) */
  int32_t _pad;
} wf_gc_params;

typedef struct wf_gc_result { /* same residency as the batch */
  int32_t* n_genes;           /* [n_groups] */
  int32_t* gene_start;        /* [n_hits]: group g's genes at [hit_off[g], hit_off[g] + n_genes[g]) */
  int32_t* gene_stop;
  int8_t*  gene_strand;       /* 0 '+', 1 '-' */
} wf_gc_result;

int wf_genecall(wf_ctx* ctx, const wf_gc_batch* batch, const wf_gc_params* params, wf_gc_result* out);

/* ---- waafle_junctions (waafle_junctions.py:252-316, 414-451) ---------------------------
 * Read-pair support of gene-gene junctions.  For every concordant pair (two consecutive
 * aligned SAM records with the same QNAME and RNAME, concordant_hits :252-275) the pair's
 * span [min(coords) - 1, max(coords) - 1] adds 1 to the contig's per-site coverage
 * (:432-436), and every locus overlapping either mate by >= min_overlap_sites sites
 * (find_hit_loci :277-286) is hit.  For each pair of start-adjacent loci (j, j+1) of a
 * contig (evaluate_contig :292-316): junction_hits = pairs hitting both, coverage_gene1/2 =
 * mean coverage over each locus, coverage_junction = mean over [end(j) - 1, start(j+1))
 * (0 when the loci touch or overlap), ratio = junction / (mean of the two genes + 1e-6).
 * Slices follow Python's rules on the contig's coverage array; an empty slice gives NaN
 * (np.mean of nothing).  Replaces the SAM loop of the reference's main() and its
 * evaluate_contig calls. */
typedef struct wf_jn_batch {
  int32_t n_contigs;
  int32_t device_resident;    /* 1: device pointers (enqueue only); 0: host arrays */
  int64_t n_pairs;
  int64_t n_loci;
  const int64_t* contig_length; /* [n_contigs] FASTA lengths (read_contig_lengths) */
  const int64_t* loc_off;     /* [n_contigs + 1] loci of each contig, sorted by start (stable) */
  const int64_t* loc_start;   /* [n_loci] GFF start */
  const int64_t* loc_end;     /* [n_loci] GFF end */
  const int32_t* pair_contig; /* [n_pairs] contig of both mates */
  const int64_t* m1_start;    /* [n_pairs] mate 1: POS, POS + cigar_length - 1 (utils.py:524-539) */
  const int64_t* m1_end;
  const int64_t* m2_start;    /* mate 2 */
  const int64_t* m2_end;
} wf_jn_batch;

typedef struct wf_jn_params {
  int64_t min_overlap_sites;  /* --min-overlap-sites, default 25 */
} wf_jn_params;

typedef struct wf_jn_result {   /* same residency as the batch */
  int32_t* junction_hits;     /* [n_loci] at j: junction (j, j+1) of j's contig */
  double* coverage_gene1;     /* [n_loci] */
  double* coverage_gene2;
  double* coverage_junction;
  double* ratio;
  int32_t* locus_hits;        /* [n_loci] pairs hitting locus j, or NULL */
  int64_t* coverage;          /* [sum(contig_length)] per-site coverage, contig-major, or NULL */
  int64_t* pair_first;        /* [n_pairs] first hit locus of each pair (-1: none), or NULL */
  uint64_t* pair_mask;        /* [n_pairs] bit i: locus pair_first + i hit (the pair's code
                                 set, :277-286).  The mask ends at locus pair_first + 63: a
                                 pair may hit later loci of its contig too (always, at
                                 min_overlap_sites <= 0); junction_hits and locus_hits
                                 count those, and a caller that needs the whole set tests
                                 loci pair_first + 64 .. loc_off[contig + 1] - 1 against the
                                 two mates itself (waafle_amd/junctions.py: wide_hits) */
} wf_jn_result;

int wf_junctions(wf_ctx* ctx, const wf_jn_batch* batch, const wf_jn_params* params, wf_jn_result* out);

/* ---- paired-read mapper (the read input of waafle_junctions, in place of bowtie2) -------
 * A deterministic seed-and-verify ungapped mapper; DESIGN.md §11 states the rule in full.
 * Bases are upper-cased and every byte other than A, C, G, T is N, which mismatches
 * everything.  wf_map_index keeps, in the context, the contigs as two bit planes plus an N
 * plane and the sorted (S-mer, position) index of every forward-strand S-mer that lies in one
 * contig and holds no N; a second call replaces the first index.  wf_map_pairs maps read
 * pairs against it: each mate as given (+) and reverse-complemented (-), seeds at offsets
 * 0, S, 2S, ... (at most 16), seeds with more than max_occ occurrences unused, ungapped
 * alignments inside one contig with at most max_mm mismatches, and of the concordant pairs
 * (same contig, opposite strands, no dovetail, min_insert <= fragment <= max_insert) the
 * one with the least (mm1 + mm2, contig, + mate's position, fragment, mate-1 strand).
 * No gaps, no clipping, no MAPQ: reads with indels stay unaligned (but see
 * wf_map_pairs_gapped below). */
typedef struct wf_map_params {
  int32_t seed_len;           /* S, 12..32 (default 20) */
  int32_t max_occ;            /* 1..64 (default 16) */
  int32_t max_mm;             /* 0..32 mismatches per mate (default 4) */
  int32_t _pad;
  int64_t min_insert;         /* fragment length bounds (defaults 0, 500) */
  int64_t max_insert;
} wf_map_params;

typedef struct wf_map_contigs { /* host memory */
  int32_t n_contigs;
  int32_t _pad;
  const char* seq;            /* [off[n_contigs]] the contigs' ASCII bases, concatenated */
  const int64_t* off;         /* [n_contigs + 1] off[0] = 0; off[n_contigs] < 2^31 - 1024,
                                 else WF_E_TOOBIG */
} wf_map_contigs;

typedef struct wf_map_reads {
  int64_t n_pairs;            /* < 2^31 per call */
  int32_t device_resident;    /* 1: device pointers (reads and result); 0: host arrays.  The
                                 offsets are read back and checked either way, so the call
                                 synchronises */
  int32_t _pad;
  const char* seq1;           /* mate 1: ASCII bases, concatenated */
  const int64_t* off1;        /* [n_pairs + 1]; a read longer than 512: WF_E_BADINPUT */
  const char* seq2;           /* mate 2 */
  const int64_t* off2;
} wf_map_reads;

typedef struct wf_map_result {  /* [n_pairs] each, same residency as the reads */
  int32_t* contig;            /* contig index, -1: unaligned (the other fields are then 0) */
  int32_t* pos1;              /* 1-based leftmost contig position of mate 1 */
  int32_t* pos2;              /* ... of mate 2 */
  uint8_t* strand1;           /* 0: mate 1 on +, mate 2 on -; 1: the reverse */
  uint8_t* mm1;               /* mismatches of mate 1 */
  uint8_t* mm2;
} wf_map_result;

/* params: seed_len and max_occ (the other fields are not read) */
int wf_map_index(wf_ctx* ctx, const wf_map_contigs* contigs, const wf_map_params* params);
/* params: seed_len and max_occ must equal the index's (WF_E_BADINPUT); WF_E_STATE before
   wf_map_index */
int wf_map_pairs(wf_ctx* ctx, const wf_map_reads* reads, const wf_map_params* params, wf_map_result* out);

/* Single-gap rescue ("gapped pass").  wf_map_pairs_gapped is wf_map_pairs
 * followed, for max_gap > 0, by a second pass over the pairs it left unaligned whose mates
 * are both at least seed_len long: each mate may then carry one deletion (d > 0: d contig
 * bases the read lacks) or one insertion (d < 0: -d read bases) of at most max_gap bases
 * after its first k bases (k counted along the contig's + strand), both segments at least
 * seed_len long.  Pairs that wf_map_pairs aligns keep exactly its result.  mm1 / mm2 stay
 * mismatch counts; a mate spans L + d contig bases. */
typedef struct wf_map_gap_params {
  int32_t max_gap;            /* 0..8 (default 0: no gapped pass) */
  int32_t _pad[3];
} wf_map_gap_params;

typedef struct wf_map_gap_result { /* [n_pairs] each, same residency as the reads */
  int8_t* d1;                 /* gap of mate 1: > 0 deletion, < 0 insertion, 0 none */
  int8_t* d2;
  int16_t* k1;                /* bases of mate 1's variant before its gap (0 when d1 = 0) */
  int16_t* k2;
  uint8_t* flags;             /* bit 0: aligned by the gapped pass; bit 1: a mate had more
                                 than 256 hits in the gapped pass (the pair stays unaligned) */
} wf_map_gap_result;

/* As wf_map_pairs, plus gap_params->max_gap outside 0..8: WF_E_BADINPUT.  With max_gap 0 it
   writes what wf_map_pairs writes and zeros in gap_out.  Returns after the work is done. */
int wf_map_pairs_gapped(wf_ctx* ctx, const wf_map_reads* reads, const wf_map_params* params,
                        const wf_map_gap_params* gap_params, wf_map_result* out, wf_map_gap_result* gap_out);

/* ---- homology search (waafle_search without blastn) --------------------------------------
 * Ungapped seed-and-extend of database genes (subjects) against the contigs wf_map_index
 * holds; DESIGN.md §12 states the rule in full.  Not a blastn clone: wf_search reports ungapped
 * HSPs only (wf_search_gapped below extends them by a banded gapped alignment).
 * Bases as in the mapper.  Each subject is searched as given (plus) and reverse-complemented
 * (minus).  Seeds of seed_len bases at subject offsets 0, stride, 2 stride, ...; a seed with
 * an N, or with more than max_occ occurrences in the index, is unused (the index's own
 * max_occ is not read).  Every seed hit is extended on its diagonal to both sides, match +1,
 * mismatch -2, until the running score has dropped more than xdrop below its best, and never
 * past an end of its contig or subject.  Per (variant, contig, diagonal) identical HSPs count
 * once and an HSP strictly contained in another is dropped; those with score >= min_score
 * are reported.  The subjects of a call are one chunk; the result set of a database does not
 * depend on how it is cut into chunks. */
typedef struct wf_search_params {
  int32_t seed_len;           /* S, 12..32, must equal the index's (default 21) */
  int32_t stride;             /* T, 1..32 (default 8) */
  int32_t max_occ;            /* 1..1024 (default 64) */
  int32_t xdrop;              /* X, 1..1000 (default 20) */
  int32_t min_score;          /* >= 1 (default 28) */
  int32_t _pad[3];
} wf_search_params;

typedef struct wf_search_subjects { /* host memory */
  int64_t n_subjects;         /* < 2^31 */
  const char* seq;            /* [off[n_subjects]] ASCII bases, concatenated */
  const int64_t* off;         /* [n_subjects + 1] off[0] = 0; off[n_subjects] <= 2^30, else
                                 WF_E_TOOBIG */
} wf_search_subjects;

typedef struct wf_search_result { /* caller-owned host arrays of `capacity` records, 0-based */
  int64_t capacity;
  int64_t n;                  /* out: records found (may exceed capacity, see wf_search) */
  int32_t* contig;            /* contig index */
  int32_t* subject;           /* subject index within the call */
  uint8_t* minus;             /* 0: the subject as given, 1: reverse-complemented */
  int32_t* qstart;            /* first contig base of the HSP */
  int32_t* sstart;            /* first base of the HSP on the variant (plus: the subject, minus:
                                 its reverse complement) */
  int32_t* length;
  int32_t* matches;
  int64_t seed_hits;          /* out, diagnostics: seed hits of the call, those skipped because */
  int64_t seeds_skipped;      /*   their predecessor on the diagonal gives the same HSP, and    */
  int64_t raw_hsps;           /*   the HSPs extended, before de-duplication                     */
} wf_search_result;

/* Records sorted by (contig, subject, minus, qstart, sstart, length).  WF_E_STATE before
   wf_map_index; WF_E_BADINPUT for a parameter out of range or a seed_len other than the
   index's; WF_E_TOOBIG for more than 2^31 - 1 seed hits in the call.  With more than
   `capacity` records the first `capacity` are written, n is the full count and the call
   returns WF_E_NOMEM: repeat it with more room.  Returns after the work is done. */
int wf_search(wf_ctx* ctx, const wf_search_subjects* subjects, const wf_search_params* params,
              wf_search_result* out);

/* Gapped extension.  wf_search_gapped is wf_search followed by a banded
 * x-drop alignment from every record: the record's midpoint (variant position i0 = sstart +
 * length / 2, the contig position on its diagonal) is an anchor, extended to the right and to
 * the left on its own, over anti-diagonals, within `band` diagonals of the anchor's on each
 * side, until every cell has dropped more than xdrop_gap below the best so far; never past an
 * end of its contig or subject.  Scores in half units: match +2, mismatch -4, every gap
 * column -5 (linear: megablast's +1 / -2 with open 0, extend 2.5).  Per (subject, strand,
 * contig) identical alignments count once and, in score order, one whose contig and subject
 * intervals a kept one covers is dropped; those with score2 >= 2 min_score are reported.
 * score2 = 6 matches - 4 (length - gaps) - 5 gaps.  Not a blastn clone: linear gaps only, no
 * greedy or affine alignment, no traceback-based trimming; a gap longer than `band` on one
 * side of the anchor is not bridged, and a homolog with no ungapped record is not found. */
typedef struct wf_search_gap_params {
  int32_t band;               /* W, 1..31 (default 15) */
  int32_t xdrop_gap;          /* Xg, raw score, 1..1000 (default 30) */
  int32_t _pad[2];
} wf_search_gap_params;

typedef struct wf_search_gap_result { /* caller-owned host arrays of `capacity` records, 0-based */
  int64_t capacity;
  int64_t n;                  /* out: records found (may exceed capacity) */
  int32_t* contig;
  int32_t* subject;           /* subject index within the call */
  uint8_t* minus;
  int32_t* qstart;            /* contig interval [qstart, qstart + qspan) */
  int32_t* qspan;
  int32_t* sstart;            /* variant interval [sstart, sstart + sspan) */
  int32_t* sspan;
  int32_t* length;            /* alignment columns: aligned pairs + gaps */
  int32_t* matches;
  int32_t* gaps;              /* gap columns */
  int64_t seed_hits;          /* out, diagnostics: as in wf_search_result, and               */
  int64_t seeds_skipped;
  int64_t raw_hsps;
  int64_t anchors;            /*   the ungapped records extended,                            */
  int64_t raw_alignments;     /*   the distinct alignments they gave, before the covered go */
} wf_search_gap_result;

/* Records sorted by (contig, subject, minus, qstart, sstart, qspan, sspan, length, matches,
   gaps).  Statuses as wf_search, plus WF_E_BADINPUT for band outside 1..31 or xdrop_gap outside
   1..1000; the same WF_E_NOMEM-and-repeat protocol.  wf_search on the same context is
   unaffected.  Returns after the work is done. */
int wf_search_gapped(wf_ctx* ctx, const wf_search_subjects* subjects, const wf_search_params* params,
                     const wf_search_gap_params* gap_params, wf_search_gap_result* out);

/* Subjects as the bit planes of a packed database (python -m waafle_amd.makedb, DESIGN.md
 * §12.7): the chunk's bases lie bit-contiguously in three planes, starting at bit `bit0` of
 * their first word, so a slice of a memory-mapped .wfdb file is passed as it is.  A base's code
 * (A0 C1 G2 T3) is its lo bit + 2 x its hi bit; a set nn bit makes it an N whatever lo and hi
 * hold there.  The bits before bit0 and from bit0 + off[n_subjects] on belong to the file's
 * neighbouring subjects and are not searched.  No ASCII is uploaded and nothing is parsed. */
typedef struct wf_search_packed_subjects { /* host memory; may be a read-only file mapping */
  int64_t n_subjects;         /* < 2^31 */
  const int64_t* off;         /* [n_subjects + 1] chunk-relative, off[0] = 0; off[n_subjects] <= 2^30,
                                 else WF_E_TOOBIG */
  const uint32_t* lo;         /* base i of the chunk: bit (bit0 + i) & 31 of word (bit0 + i) >> 5 */
  const uint32_t* hi;
  const uint32_t* nn;
  int64_t n_words;            /* (bit0 + off[n_subjects] + 31) / 32; no word outside [0, n_words) is read */
  int32_t bit0;               /* 0..31 */
  int32_t _pad;
} wf_search_packed_subjects;

/* wf_search / wf_search_gapped on such subjects: the same records, counters, statuses and
   WF_E_NOMEM-and-repeat protocol.  Also WF_E_BADINPUT for bit0 outside 0..31, null planes with
   off[n_subjects] > 0, or an n_words other than (bit0 + off[n_subjects] + 31) / 32; WF_E_TOOBIG
   (more than 2^30 bases) is returned before the planes are looked at. */
int wf_search_packed(wf_ctx* ctx, const wf_search_packed_subjects* subjects, const wf_search_params* params,
                     wf_search_result* out);
int wf_search_gapped_packed(wf_ctx* ctx, const wf_search_packed_subjects* subjects, const wf_search_params* params,
                            const wf_search_gap_params* gap_params, wf_search_gap_result* out);

/* Diagnostic: the device's store of the chunk that the context's last search call (any of the
   four) left resident, copied out: strand 0 the chunk as given, 1 its reverse complement, each
   as planes of words = (off[n_subjects] + 31) / 32 + 2 words, the padding N.  A call that found
   no seed slot (no subject as long as a seed, no index entries) leaves none.  WF_E_STATE when no
   chunk is resident; WF_E_BADINPUT for another strand, null arrays or another `words`. */
int wf_search_chunk_planes(wf_ctx* ctx, int strand, uint32_t* lo, uint32_t* hi, uint32_t* nn, int64_t words);

/* The reporting step on its own (DESIGN.md §12.1 "Reporting", §12.5 "Reporting", §12.8), in the
 * form WF_OPT_SEARCH_REPORT selects; no index is needed.  wf_search_report: raw HSPs, [b, e) on the
 * variant at diagonal delta (contig position - variant position) with score = matches - 2
 * mismatches, to the records wf_search gives for them; out->raw_hsps = n, the other counters 0.
 * wf_search_report_gapped: anchors (i0 on the variant, j0 contig-local) with the two sides of
 * their gapped extension (H in half units, p variant bases, q contig bases, g gap columns) to
 * the records wf_search_gapped gives; out->anchors = n and out->raw_alignments are set. */
typedef struct wf_report_hsps {   /* host memory, [n] each */
  int64_t n;                      /* < 2^31 */
  int32_t min_score;              /* >= 1 */
  int32_t _pad;
  const int32_t* contig;          /* >= 0 */
  const int32_t* subject;         /* >= 0, < 2^30 */
  const uint8_t* minus;           /* 0 / 1 */
  const int32_t* delta;
  const int32_t* b;               /* >= 0 */
  const int32_t* e;               /* > b */
  const int32_t* score;           /* score + 2 (e - b) = 3 matches, 0 <= matches <= e - b */
} wf_report_hsps;

typedef struct wf_report_anchors { /* host memory, [n] each */
  int64_t n;                      /* < 2^31 */
  int32_t min_score;              /* >= 1 */
  int32_t _pad;
  const int32_t* contig;
  const int32_t* subject;
  const uint8_t* minus;
  const int32_t* i0;
  const int32_t* j0;
  const int32_t* left_H;  const int32_t* left_p;  const int32_t* left_q;  const int32_t* left_g;
  const int32_t* right_H; const int32_t* right_p; const int32_t* right_q; const int32_t* right_g;
} wf_report_anchors;

/* Both: the capacity / n / WF_E_NOMEM-and-repeat protocol and the order of the search calls.
   n = 0 is valid.  WF_E_BADINPUT, checked on the host before anything is uploaded, so nothing is
   written: a null struct, a null column with n > 0 or a null result array with capacity > 0, n
   outside [0, 2^31), a negative capacity, min_score < 1; and, named by its first record in
   wf_last_error: contig or subject < 0 (subject >= 2^30), minus above 1; ungapped: b < 0, e <= b,
   score + 2 (e - b) no multiple of 3 or outside 0 .. 3 (e - b), b + delta outside int32; gapped: a negative p, q or g,
   sspan + qspan - gaps odd, (score2 + 5 gaps + 4 pairs) / 6 inexact or outside 0 .. length, a field of
   the alignment outside int32.  Two HSPs equal in (subject, minus, contig, delta, b, e) cover the same
   bases and must have the same score: which score survives is otherwise undefined.
   Returns after the work is done. */
int wf_search_report(wf_ctx* ctx, const wf_report_hsps* hsps, wf_search_result* out);
int wf_search_report_gapped(wf_ctx* ctx, const wf_report_anchors* anchors, wf_search_gap_result* out);

/* Low-complexity masking.  wf_search_mask computes the symmetric-DUST mask
 * (Morgulis et al. 2006, the published definition) of the contigs the context holds and
 * rebuilds the index, at the seed length it has, without the S-mers that hold a masked base:
 * a soft mask, as blastn applies to its query by default.  Masked stretches then give no
 * seeds, and max_occ counts the remaining occurrences only; the extensions of wf_search and
 * wf_search_gapped read the bases as before and run through masked stretches, and the N plane
 * is unchanged.  A run is a maximal stretch of A/C/G/T inside one contig; an interval of l
 * triplets (l + 2 <= window bases) of one run scores r / (l - 1), r the sum of c (c - 1) / 2
 * over the counts c of the 64 triplet kinds (0 for l = 1); it is perfect when 10 r >
 * level (l - 1) and no sub-interval scores strictly more; a base is masked iff a perfect
 * interval covers it.  Not a dustmasker clone: agreement with NCBI dustmasker is not measured.
 * The mask lasts until the next wf_map_index on the context, which builds an unmasked index
 * again; calling wf_search_mask again replaces the mask.  wf_map_pairs on the same context
 * sees the masked index too: give the read mapper a context of its own. */
typedef struct wf_dust_params {
  int32_t window;             /* Wd, 8..64 bases (default 64) */
  int32_t level;              /* Lv >= 1; the score threshold is Lv / 10 (default 20) */
  int32_t _pad[2];
} wf_dust_params;

typedef struct wf_dust_result {
  uint32_t* mask;             /* null, or caller-owned host memory of (total + 31) / 32 words,
                                 total = the contigs' bases: bit p & 31 of word p >> 5 is set
                                 iff store position p (contigs concatenated) is masked */
  int64_t masked_bases;       /* out */
  int64_t kmers_before;       /* out: S-mers of the index without a mask, */
  int64_t kmers_after;        /*   and of the index as it is now         */
} wf_dust_result;

/* WF_E_STATE before wf_map_index; WF_E_BADINPUT for window outside 8..64 or level < 1.
   Returns after the work is done. */
int wf_search_mask(wf_ctx* ctx, const wf_dust_params* params, wf_dust_result* out);

/* ---- search records -> hit arrays ---------------------------------------
 * The hit arrays of wf_batch / wf_gc_batch from the search's records, without the table: bit
 * for bit what inputs.load_inputs gives for the table search.format_rows writes of the same
 * records.  The records come in the table's order (search.order_records), so sorted by contig;
 * an ungapped record (wf_search_result) has qspan = sspan = length.  Per record:
 *   hit_qlo = qstart + 1, hit_qhi = qstart + qspan; s0 = sstart + 1, s1 = sstart + sspan (on
 *   either strand: a minus row's subject coordinates mirror back to these);
 *   ltrim = max(0, s0 - hit_qlo), rtrim = max(0, slen - s0 - qlen + hit_qlo);
 *   hit_scov = (double)(s1 - s0 + 1) / (double)(slen - ltrim - rtrim);
 *   pident = n / 1000.0, n the integer nearest to x * 1000 exactly, ties to even, for the double
 *   x = (100.0 * matches) / length: the value of the text "%.3f" % x;
 *   hit_score = hit_scov * pident / 100.0 (two roundings); hit_taxon and hit_sysmask gathered by
 *   subject; hit_strand = minus; hit_key as wf_pack_hit_keys packs it for min_scov;
 *   hit_off[c] = records with contig < c. */
typedef struct wf_hit_records {   /* host memory, [n] each */
  int64_t n;                      /* < 2^31 */
  const int32_t* contig;          /* not decreasing */
  const int32_t* subject;         /* index into the subject tables */
  const uint8_t* minus;           /* 0 / 1 */
  const int32_t* qstart;          /* 0-based first contig base */
  const int32_t* qspan;
  const int32_t* sstart;          /* 0-based, on the variant */
  const int32_t* sspan;
  const int32_t* length;          /* alignment columns */
  const int32_t* matches;
} wf_hit_records;

typedef struct wf_hit_tables {    /* host memory */
  int32_t n_contigs;
  int32_t n_subjects;
  const int64_t* qlen;            /* [n_contigs] contig lengths */
  const int64_t* slen;            /* [n_subjects] subject lengths */
  const int32_t* subject_taxon;   /* [n_subjects] interned taxon id, 0 .. 2^24 - 1 */
  const uint32_t* subject_sysmask;/* [n_subjects] annotation systems present */
  double min_scov;                /* read for bit 24 of hit_key only */
} wf_hit_tables;

typedef struct wf_hits_out {      /* the arrays wf_batch and wf_gc_batch take */
  int32_t device_resident;        /* 1: device pointers, the call only enqueues on the context
                                     stream (the records and tables must stay valid until
                                     wf_synchronize, or a later synchronising call, returns);
                                     0: host arrays, copied out and synchronised */
  int32_t _pad;
  int64_t* hit_off;               /* [n_contigs + 1] */
  int32_t* hit_qlo;               /* [n] each from here */
  int32_t* hit_qhi;
  int32_t* hit_taxon;
  int8_t* hit_strand;
  double* hit_score;
  double* hit_scov;
  uint32_t* hit_sysmask;
  uint32_t* hit_key;
} wf_hits_out;

/* WF_E_BADINPUT, checked on the host before anything is launched or written, so the outputs are
   untouched: a null struct, a null hit_off, a null record or output array with n > 0 or a null
   table a record needs, n or a table size negative, n >= 2^31; and, named by its first record in
   wf_last_error: a contig or subject outside its table, a contig column that decreases, minus
   above 1, length <= 0, matches < 0 or > length, qspan or sspan <= 0, qlen or slen <= 0 (of a
   contig or subject some record names), a denominator slen - ltrim - rtrim <= 0, hit_qlo or
   hit_qhi outside int32, a taxon outside 24 bits.  n = 0 and n_contigs = 0 are valid (hit_off is
   still written). */
int wf_hits_from_records(wf_ctx* ctx, const wf_hit_records* records, const wf_hit_tables* tables,
                         wf_hits_out* out);

/* ---- the table's order and --max-target-seqs (search.order_records) -------
 * Which of the search's records the table holds, and in which order.  The score, in 64 bits, is
 * 3 matches - 2 length for ungapped records (qspan, sspan and gaps all null) and
 * 6 matches - 4 length - gaps for gapped ones.  best of a (contig, subject) pair: the greatest
 * score of its records.  Within a contig the pairs are ranked by (-best, subject), and the pairs
 * of rank >= max_target_seqs lose their records.  The others go by (contig, -score, subject,
 * minus, qstart, sstart), gapped records then by (qspan, sspan); records equal in all of these by
 * their position in the input.  order[k] is the input index of the k-th record of the table. */
typedef struct wf_order_in {      /* host memory, [n] each; the records in any order */
  int64_t n;                      /* < 2^31 */
  int64_t max_target_seqs;        /* >= 1 */
  const int32_t* contig;          /* >= 0 */
  const int32_t* subject;         /* >= 0 */
  const uint8_t* minus;           /* 0 / 1 */
  const int32_t* qstart;
  const int32_t* sstart;
  const int32_t* length;
  const int32_t* matches;
  const int32_t* qspan;           /* these three: all null (ungapped) or all given (gapped) */
  const int32_t* sspan;
  const int32_t* gaps;
} wf_order_in;

typedef struct wf_order_out {     /* host memory */
  int64_t n_kept;                 /* written by the call */
  int64_t* order;                 /* room for n; [0, n_kept) written */
  /* the columns of wf_hit_records gathered in that order (an ungapped record has qspan = sspan =
     length): each null (not wanted) or room for n, [0, n_kept) written */
  int32_t* contig;
  int32_t* subject;
  uint8_t* minus;
  int32_t* qstart;
  int32_t* qspan;
  int32_t* sstart;
  int32_t* sspan;
  int32_t* length;
  int32_t* matches;
} wf_order_out;

/* Returns after the work is done.  n = 0 is valid (n_kept = 0).  WF_E_BADINPUT, checked on the
   host before anything is uploaded or launched, so nothing is written: a null struct, a null
   record column or a null order with n > 0, n < 0 or >= 2^31, max_target_seqs < 1, only some of
   qspan / sspan / gaps given; and, named by its first record in wf_last_error: a contig or
   subject < 0, minus above 1.  WF_E_NOMEM, also with nothing written, when device memory cannot
   be had: the call holds 25 bytes per record of input (37 gapped), 8 per 64 bits of sort key
   (the fields' ranges in this call decide: 8 to 32), 68 of sort and ranking arrays and, with any
   column asked for, 33 of gathered columns: at most 170 bytes per record, plus the radix sort's
   scratch.  The arrays stay with the context and are reused by later calls of any size. */
int wf_order_records(wf_ctx* ctx, const wf_order_in* in, wf_order_out* out);

/* ---- --write-details (orgscorer.py:766-812, 931-937) --------------------------------
 * With details on, the next wf_score (staged mode) also records, for every roll-up level,
 * the contigs it evaluated and each (contig, clade, locus) segment of that level: its gene
 * score (Contig.update_gene_scores :394-406, the exact numpy mean) and its gene spans
 * (make_gene_spans_field :770-789: first and last 1-based site of every nonzero run longer
 * than one site).  The caller renders the reference's rows from them (clades per contig
 * and level, 'Unknown' = 1 - max for --weak-loci assign-unknown).  Replaces the
 * write_details(details, contig, iteration) calls of evaluate_contig (:566-583).
 * Arrays stay valid until the next wf_score or wf_free.  Synchronous; a diagnostic path. */
typedef struct wf_details {
  int64_t n_evals;            /* evaluated (contig, level) pairs, level-major */
  const int32_t* eval_contig;
  const int32_t* eval_level;
  int64_t n_segs;             /* segment records, level-major */
  const int32_t* seg_level;
  const int32_t* seg_contig;
  const int32_t* seg_clade;   /* taxonomy id at that level */
  const int32_t* seg_locus;   /* index among the contig's kept loci */
  const double* seg_mean;     /* gene score */
  const int32_t* seg_nspan;   /* runs listed; -1: the site array is all zero (upstream raises) */
  const int64_t* span_off;    /* [n_segs + 1] first run of each segment */
  const int32_t* spans;       /* [2 * span_off[n_segs]] (first, last) 1-based site pairs */
} wf_details;

int wf_details_enable(wf_ctx* ctx, int on);
int wf_details_read(wf_ctx* ctx, wf_details* out);

int wf_abi_version(void);
int wf_device_count(int* count);
int wf_init(int device, wf_ctx** out);
void wf_free(wf_ctx* ctx);
const char* wf_last_error(const wf_ctx* ctx);
int wf_set_stream(wf_ctx* ctx, void* hip_stream);     /* NULL = the context's own stream */
int wf_set_lds_bytes(wf_ctx* ctx, int64_t bytes);     /* decision arena per workgroup (LDS) */
int wf_set_mode(wf_ctx* ctx, int mode);               /* WF_MODE_LEVEL0 (default), _WAVES or _STAGED */
int wf_set_option(wf_ctx* ctx, int option, int64_t value);   /* wf_option */
int wf_set_taxonomy(wf_ctx* ctx, const wf_taxonomy* tax);
int wf_score(wf_ctx* ctx, const wf_batch* batch, const wf_params* params, wf_result* out);
/* wf_batch.hit_key from the separate arrays (host memory, any thread, no context):
   out[i] = taxon[i] | (scov[i] >= min_scov) << 24 | (strand[i] == 1) << 25
            | (sysmask[i] & 63) << 26.
   WF_E_BADINPUT for a taxon id outside [0, 2^24) or a strand other than 0 / 1. */
int wf_pack_hit_keys(int64_t n_hits, const int32_t* taxon, const int8_t* strand, const double* scov,
                     const uint32_t* sysmask, double min_scov, uint32_t* out);
int wf_synchronize(wf_ctx* ctx);
int wf_timing_enable(wf_ctx* ctx, int on);             /* also resets the counters */
int wf_timing_read(wf_ctx* ctx, wf_timing* out);       /* synchronises first */

#ifdef __cplusplus
}
#endif
#endif /* WAAFLE_HIP_H */
