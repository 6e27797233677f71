/*
 * pyrodigal_amd.h -- C-ABI of the MI355X-native Prodigal gene-finding core.
 *
 * Plain C linkage, plain pointers and sizes, no exceptions cross this boundary.
 * Every entry point returns 0 on success or a negative PGA_E* code; the message
 * for the last failure on a context is available through pga_last_error().
 * All "ref:" citations are relative to /root/reference/src/pyrodigal.
 *
 * Two levels, both replacing reference plug points:
 *
 *  1. scorer level  -- pga_score_connections(): whole-array drop-in for
 *     ConnectionScorer.index() + score_connections()  (ref: lib.pyx:1126-1237,
 *     1336-1357; _connection.h:386-408; impl/generic.h:13-49).
 *  2. finder level  -- pga_find_genes_batch(): whole-batch drop-in for
 *     GeneFinder.find_genes() in meta or single mode  (ref: lib.pyx:5281-5469).
 */
#ifndef PYRODIGAL_AMD_H
#define PYRODIGAL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGA_OK          0
#define PGA_EINVAL     (-1)   /* bad argument (maps to ValueError)  */
#define PGA_ENOMEM     (-2)   /* host or device allocation failed (MemoryError) */
#define PGA_EDEVICE    (-3)   /* HIP runtime error (RuntimeError) */
#define PGA_ENODEVICE  (-4)   /* no gfx950 device visible (RuntimeError) */

typedef struct pga_ctx pga_ctx;

/* Byte layout of the reference's `struct _training` (ref: prodigal/training.pxd:3-14),
 * 558 392 bytes; TrainingInfo.dump() files can be passed as-is. */
typedef struct pga_training {
    double  gc;
    int32_t trans_table;
    int32_t _pad0;
    double  st_wt;
    double  bias[3];
    double  type_wt[3];
    int32_t uses_sd;
    int32_t _pad1;
    double  rbs_wt[28];
    double  ups_comp[32][4];
    double  mot_wt[4][4][4096];
    double  no_mot;
    double  gene_dc[4096];
} pga_training;

/* pga_params.want_nodes = PGA_NODES_DEVICE: the winners' node arrays stay in device memory, owned by the context, until the next
 * call on it that runs the finder (pga_find_genes*, pga_nodes_stage, pga_train*) or loads models; nothing of them is copied back. */
#define PGA_NODES_DEVICE 2

/* GeneFinder constructor options (ref: lib.pyx:5102-5115). */
typedef struct pga_params {
    int32_t closed;         /* default 0  */
    int32_t min_gene;       /* default 90 */
    int32_t min_edge_gene;  /* default 60 */
    int32_t max_overlap;    /* default 60 */
    int32_t meta;           /* 1: meta mode over all loaded models; 0: single mode with model 0 */
    int32_t want_nodes;     /* 1: also return the winning model's full node arrays; PGA_NODES_DEVICE (2): keep them on the device
                             * only, for pga_render_genes (PGA_RENDER_SCO), with pga_result.nodes NULL; 0: neither */
    int32_t mask;           /* 1: no gene may run across a masked region (runs of unknown bases), default 0 */
    int32_t min_mask;       /* shortest run of unknown bases that is masked, default 50 (ref: lib.pyx:5102-5115, 699-713) */
} pga_params;

/* One predicted gene (ref: lib.pxd:274-278 `_gene` + the start/stop node fields Gene reads,
 * lib.pyx:2644-2830). Coordinates are 1-based inclusive like the reference. */
typedef struct pga_gene {
    int32_t contig;        /* index into the batch */
    int32_t begin, end;
    int32_t start_ndx, stop_ndx;
    int8_t  strand;
    uint8_t partial_begin, partial_end;
    uint8_t start_type;    /* 0 ATG, 1 GTG, 2 TTG, 3 Edge */
    uint8_t rbs[2];
    uint8_t mot_len, mot_spacer;
    int32_t mot_ndx;
    float   gc_cont;
    double  cscore, sscore, rscore, uscore, tscore, mot_score;
} pga_gene;

/* Node arrays of one contig for its winning model (SoA; ref: src/Prodigal/node.h:40-76). */
typedef struct pga_nodes {
    int32_t  n;
    int32_t *ndx, *stop_val, *traceb, *tracef, *star_ptr /* [n][3] */;
    uint8_t *type, *edge, *elim, *rbs /* [n][2] */;
    int8_t  *strand, *ov_mark;
    float   *gc_cont;
    double  *cscore, *sscore, *rscore, *uscore, *tscore, *score, *mot_score;
    int32_t *mot_ndx;
    uint8_t *mot_len, *mot_spacer, *mot_spacendx;
} pga_nodes;

typedef struct pga_contig_result {
    int32_t model;        /* winning model index, -1 if none (ref: lib.pyx:5317-5396) */
    int32_t n_nodes;
    int64_t gene_begin;   /* genes[gene_begin .. gene_begin + n_genes) */
    int32_t n_genes;
    int32_t n_unknown;    /* bases that are not A, C, G or T (ref: lib.pyx:664-697) */
    double  gc;
    double  score;        /* nodes[ipath].score of the winning DP pass */
} pga_contig_result;

typedef struct pga_result {
    int32_t            n_contigs;
    int64_t            n_genes;
    pga_contig_result* contigs;
    pga_gene*          genes;
    pga_nodes*         nodes;     /* NULL unless want_nodes */
    double             t_total_ms, t_dp_ms;   /* device time of the whole batch / of the DP kernel */
    int64_t            node_passes;           /* sum over (contig, model) DP passes of node count */
    int32_t            n_chains;              /* number of (contig, model) DP passes */
    int32_t            _pad;
    /* masked regions when params.mask or a mask source of the batch (pga_batch_set_regions / _set_mask_case) is set, else NULL:
     * the union of the sources, contig i owns masks[2*k], masks[2*k+1] = [begin, end)
     * for k in [mask_off[i], mask_off[i+1])   (ref: lib.pyx:699-713, `Sequence.masks`) */
    int32_t*           mask_off;
    int32_t*           masks;
} pga_result;

/* ---- context ---------------------------------------------------------- */
int         pga_create(int device, pga_ctx** out);
void        pga_destroy(pga_ctx*);
const char* pga_last_error(const pga_ctx*);
int         pga_device_info(const pga_ctx*, char* name, int name_len, int* cus, int64_t* hbm_bytes);
/* How the connection scoring of the last pga_find_genes / pga_find_genes_batch / pga_score_connections call on this
 * context ran (diagnostics; no counterpart in the reference, whose dynamic programme is one serial loop):
 *   out[0] chains that were cut into segments (0: every chain was walked serially)   out[1] segments
 *   out[2..4] nodes whose speculative result the verification rounds 1..3 rejected
 *   out[5] chains that were walked serially in the end because they never verified clean
 *   out[6] 1 when the wave-batch scorer ran from a step schedule   out[7] 64-node batches whose schedule did not fit its
 *          buffer (> 0: the launch was repeated by the kernel that works the lane masks out per chain) */
int         pga_dp_stats(const pga_ctx*, int32_t out[8]);
/* Device time (HIP events on the context's stream, milliseconds) of the connection scoring of the last pga_find_genes /
 * pga_find_genes_batch call on this context, by part (diagnostics; the reference's counterpart of all three is ConnectionScorer.index +
 * score_connections, src/pyrodigal/lib.pyx:1126-1176, 1205-1237):
 *   out[0] the connection-scoring launch(es) themselves (= pga_result.t_dp_ms; both launches when a schedule miss repeated the launch)
 *   out[1] the topology kernels of every translation-table group (windows, near-zone starts, candidate links)
 *   out[2] the step-schedule kernels of every group   out[3] reserved (0) */
int         pga_dp_timings(const pga_ctx*, double out[4]);
/* How the node extraction of the last pga_find_genes / pga_find_genes_batch / pga_nodes_stage call on this context ran (diagnostics):
 *   out[0] extraction passes (1; 2 when a tile of the batch did not fit the half-density staging, or its pool of stop values, and the batch was extracted again)
 *   out[1] reserved (0) */
int         pga_extract_stats(const pga_ctx*, int32_t out[2]);
/* How a connection-scoring launch over chains of these node counts would be cut (host arithmetic only, no device needed;
 * the PGA_DP_SEG* environment variables of INTEGRATION.md apply):
 *   out[0] chains cut into segments   out[1] segments   out[2] nodes of the longest sub-chain (segment + warm-up)
 *   out[3] scratch elements behind the real chains in every per-node array */
int         pga_dp_plan_summary(int32_t n_chains, const int32_t* nodes_per_chain, int64_t out[4]);
/* The order in which the wave-batch connection scorer starts the chains of a launch: longest first by walk batches of 64 nodes,
 * launch order among equals (host arithmetic only).  order[k] = index of the chain started k-th. */
int         pga_dp_start_order(int32_t n_chains, const int32_t* nodes_per_chain, int32_t* order);
/* ... and that order made XCD-aware (workgroup b runs on XCD b % 8): chains with the same key -- a contig under one translation
 * table, i.e. the same topology arrays -- all go to one XCD, the one with the fewest nodes so far; out[8 k + x] is the k-th chain of
 * XCD x, -1 where a queue has ended.  Returns the entries written (a multiple of 8) or a negative PGA_E* code. */
int64_t     pga_dp_xcd_order(int32_t n_chains, const int32_t* order, const int32_t* nodes_per_chain, const int32_t* key_of_chain,
                             int32_t n_keys, int32_t* out, int64_t out_cap);
/* How the ORF walks of the coding score (LDS-table form) of one translation-table group are cut into tasks (host arithmetic only):
 * contig i has nodes_per_contig[i] nodes and is scored for models_per_contig[i] models whose table columns start at
 * first_column[i] (columns of a contig are neighbours; every four of them are one walk).
 *   out[0] tasks   out[1] entries (pieces of contigs)   out[2] nodes of the largest task   out[3] nodes over all tasks
 *   out[4] 1 if the tasks of higher columns come first; returns PGA_EINVAL when the LDS form does not apply */
int         pga_cs_task_summary(int32_t n_contigs, const int32_t* nodes_per_contig, const int32_t* first_column,
                                const int32_t* models_per_contig, int32_t task_nodes, int64_t out[5]);

/* ---- models (MetagenomicBins / TrainingInfo, ref: lib.pyx:4888-5069, 3898-3953) ---- */
int pga_set_models(pga_ctx*, const pga_training* const* models, int n_models);

/* ---- scorer level ------------------------------------------------------ */
/* Whole-array connection scoring of one sorted node list (the gene prediction pass, final = 1).
 * Inputs are the node fields _score_connections reads; outputs are the fields it writes.  Scores must be finite: equal values
 * and exact zeros are decided as the reference decides them, NaN and infinities are outside the contract. */
int pga_score_connections(pga_ctx*, int32_t n,
                          const int32_t* ndx, const int32_t* stop_val,
                          const uint8_t* type, const int8_t* strand,
                          const double* cscore, const double* sscore,
                          const double* rscore, const double* uscore,
                          const int32_t* star_ptr /* [n][3] */,
                          double st_wt, int final /* must be 1: see pga_score_connections_training for the training pass */,
                          double* score, int32_t* traceb, int8_t* ov_mark,
                          int32_t* max_index /* _find_max_index, may be NULL */,
                          double* kernel_ms /* may be NULL */);

/* The training pass of the same scorer (final = 0 in the reference, _connection.h:94-367): a connection is worth its length
 * times bias . gc_score of one of its nodes.  gc_score is the [n][3] array of the nodes after Prodigal's record_gc_bias
 * (call site lib.pyx:5261), bias = TrainingInfo.bias, star_ptr as left by _record_overlapping_starts(flag = 0). */
int pga_score_connections_training(pga_ctx*, int32_t n,
                                   const int32_t* ndx, const int32_t* stop_val,
                                   const uint8_t* type, const int8_t* strand,
                                   const double* gc_score /* [n][3] */, const double* bias /* [3] */,
                                   const int32_t* star_ptr /* [n][3] */, double st_wt,
                                   double* score, int32_t* traceb, int8_t* ov_mark,
                                   int32_t* max_index /* may be NULL */, double* kernel_ms /* may be NULL */);

/* ---- finder level ------------------------------------------------------ */
/* `seqs[c]` points at `lens[c]` ASCII nucleotides (any case, non-ACGT = unknown).
 * One call = GeneFinder.find_genes() on every contig of the batch (ref: lib.pyx:5400-5469). */
int  pga_find_genes_batch(pga_ctx*, int32_t n_contigs, const char* const* seqs, const int64_t* lens,
                          const pga_params*, pga_result** out);
void pga_result_free(pga_result*);

/* The same in two steps, for callers that keep a batch resident in HBM (repeated passes over the
 * same contigs with different options/models, benchmarking without the PCIe upload):
 * pga_batch_create packs and uploads the contigs once, pga_find_genes runs the whole path on it.
 * A context runs ONE pga_find_genes / pga_find_genes_batch at a time; pga_batch_create / pga_batch_create_packed / pga_batch_free may be
 * called from another thread while it does (the upload has a stream, a pinned staging area and a worker pool of its own: the next batch
 * of a context can be on its way while the current one is worked on), one upload at a time per context. */
typedef struct pga_batch pga_batch;
int  pga_batch_create(pga_ctx*, int32_t n_contigs, const char* const* seqs, const int64_t* lens, pga_batch** out);
/* The same from contigs that already lie back to back in one host buffer (offs[i + 1] == offs[i] + lens[i]), ideally pinned
 * (pga_fasta_next_packed): no host-side packing, one DMA of the whole batch.  The buffer may be reused when the call returns. */
int  pga_batch_create_packed(pga_ctx*, int32_t n_contigs, const char* packed, const int64_t* offs, const int64_t* lens, pga_batch** out);
/* The same from sequences that already lie in DEVICE memory (the samples of a generative model, the output of a GPU assembler or of a
 * torch preprocessing step): one packing kernel on the device, no copy to the host and back.
 *   Letters.  Letter j of contig i is f(e), where e is element elem_off[i] + j of d_data.  With elem_bytes == 1, e is read as an
 *     unsigned byte; with elem_bytes == 4 or 8, as a signed little-endian integer.  With alphabet == NULL, which is allowed only for
 *     elem_bytes == 1, f(e) = e: the bytes are the letters, as with host input.  Otherwise f(e) = alphabet[e] for 0 <= e < n_alphabet
 *     (n_alphabet <= 256); every other value gives 'N', negative ones included.  Every alphabet entry must be an ASCII letter; lower
 *     case is allowed and keeps its meaning for pga_batch_set_mask_case.
 *   Source ranges.  The ranges of different contigs may overlap, repeat, or come in any order.  Nothing outside
 *     [elem_off[i], elem_off[i] + lens[i]) is read: the padding of a padded row is never read.
 *   Validation.  All of it happens on the host, before anything is allocated or launched; a failure returns PGA_EINVAL with a
 *     pga_last_error that names the contig where one is concerned.  elem_bytes must be 1, 4 or 8.  alphabet may be NULL only with
 *     elem_bytes == 1, and must hold only letters.  0 <= elem_off[i] and elem_off[i] + lens[i] <= n_elems.  The length limits are
 *     those of pga_batch_create: a contig of at most 0x7fff0000 bases, a batch below 2^31 bases.  hipPointerGetAttributes must say
 *     that d_data is device memory of the context's device: a host pointer is refused here, it is never dereferenced on the device.
 *   Ordering.  The call records an event on producer_stream.  The context's upload stream is non-blocking, so it does not order itself
 *     after the null stream on its own: the call makes it wait for that event, runs the pack there and synchronises that stream before
 *     it returns, as the other two pga_batch_create* calls do.  On return the source may be overwritten or freed.  The concurrency
 *     rule is that of pga_batch_create: one upload at a time per context, and it may run beside a pga_find_genes of the same context.
 *   The batch cannot be told apart from one that pga_batch_create made from the same letters: every pga_batch_set_*,
 *     pga_batch_replicate, pga_batch_trim_terminal_repeats, pga_find_genes*, pga_train*, pga_translate_genes and pga_render_genes
 *     takes it unchanged. */
int  pga_batch_create_device(pga_ctx*, int32_t n_contigs,
        const void* d_data, int64_t n_elems, int32_t elem_bytes,          /* device memory of the context's device */
        const int64_t* elem_off, const int64_t* lens,                     /* HOST arrays, n entries each */
        const uint8_t* alphabet, int32_t n_alphabet,                      /* HOST, or NULL, 0 */
        void* producer_stream,                                            /* hipStream_t, NULL = the null stream */
        pga_batch** out);
/* The packed letters of a resident batch (of any origin), one device-to-host copy on the upload stream, synchronised. */
int  pga_batch_read(pga_ctx*, const pga_batch*, int32_t contig, char* out /* HOST, lens[contig] bytes; contig = -1: the whole batch, total bytes */);
void pga_batch_free(pga_batch*);
/* More mask sources, attached to the resident batch: every call that takes the batch (pga_find_genes*, pga_nodes_stage, pga_train*,
 * pga_find_coding_bases) honours them, with params.mask on or off, and pga_batch_replicate carries them to its copies.  A region from
 * any source takes part in the mask test exactly as a masked run of N at the same coordinates would; its bases keep their identity
 * for everything else (GC content, model choice, scores, the printed sequence).  The extraction sees the UNION of all sources per
 * contig -- sorted, disjoint, touching intervals joined -- built on the device, and pga_result.masks reports that union.
 *   pga_batch_set_regions    contig i owns the intervals iv[2 k], iv[2 k + 1] = [begin, end), 0-based, for k in [off[i], off[i + 1]);
 *                            any order, overlaps and duplicates allowed, no minimum length.  0 <= begin < end <= length is checked:
 *                            PGA_EINVAL names the sequence and the interval.  NULL, NULL detaches them.
 *   pga_batch_set_mask_case  1: runs of lower-case letters of at least params.min_mask positions (or that reach the end of their
 *                            sequence) are masked, by the rule of the runs of unknown bases; the letters still read as their bases.
 * Not to be called while a call on the batch runs. */
int  pga_batch_set_regions(pga_batch*, const int32_t* off /* n + 1 */, const int32_t* iv /* 2 per interval */);
int  pga_batch_set_mask_case(pga_batch*, int lower_case);
/* Topology, one more attribute of the resident batch: circular[i] != 0 marks contig i a circle that the record cuts open at an
 * arbitrary base (NULL: every contig is linear again).  pga_find_genes and pga_find_genes_models then call a flagged contig of L
 * bases in two passes, the linear contigs of the batch exactly as without flags, in one call and in batch order:
 *   1. the ordinary call on the record; only the positions its genes cover are used;
 *   2. cut = pga_circular_cut of those genes: the middle of the widest uncovered stretch in the record's middle half;
 *   3. the ordinary call, with closed = 1, on the contig rotated to start at base cut (0-based): R = S[cut:] + S[:cut];
 *   4. a gene begin_R..end_R of R is reported with begin = (begin_R - 1 + cut) % L + 1 and end = begin + (end_R - begin_R): always
 *      1 <= begin <= L, and end > L exactly for a gene across the origin, which ends at base end - L.  Genes are ordered by begin,
 *      partial_begin = partial_end = 0, every other field is pass 3's; node arrays (want_nodes) and start_ndx / stop_ndx are those of
 *      R, in R's coordinates.
 * Mask sources follow the letters (runs are found on R; the caller's regions are rotated and split at the cut); pga_result.masks
 * stays in the record's coordinates.  pga_translate_genes and pga_render_genes read positions beyond L of a flagged contig at p - L;
 * the `# Sequence Data:` line of a flagged contig ends `;topology=circular`.  PGA_RENDER_SCO and PGA_RENDER_GBK refuse a batch
 * with flags (PGA_EINVAL): nodes live in R's coordinates, and GenBank locations across the origin are the host writer's.
 * pga_batch_replicate carries the flags; training, pga_nodes_stage and pga_find_coding_bases ignore them.
 * Not to be called while a call on the batch runs. */
int  pga_batch_set_circular(pga_batch*, const uint8_t* circular /* n flags, or NULL */);
/* The cut of every contig of the last pga_find_genes / pga_find_genes_models call on the context: out[i] for i < n, -1 for a linear
 * contig (and for every contig when the batch carried no flag). */
int  pga_circular_cuts(const pga_ctx*, int32_t n, int32_t* out);
/* Direct terminal repeats: a circular contig that its assembler wrote out with the first bases once more at the end.  For a contig S of
 * L letters, W = min(max_length, L / 2); match = the largest r with min_length <= r <= W such that S[j] and S[L - r + j] are the same
 * base for every 0 <= j < r (either case; a letter that is not A, C, G or T matches nothing), 0 when there is none.  With c the count
 * of the most frequent base of S[0 : match], the repeat is low-complexity when 100 c > max_base_percent * match; trim = match, or 0 for
 * a low-complexity repeat (a shorter match is not tried; max_base_percent = 100 turns the filter off).
 *   pga_batch_terminal_repeats       detects only, on the device, and leaves the batch as it is: search[i] != 0 (NULL: every contig)
 *                                    has contig i searched, match_out[i] / trim_out[i] are 0 for the others; 8 n bytes come back.
 *                                    PGA_EINVAL unless 1 <= min_length <= max_length <= 1048576 and 25 <= max_base_percent <= 100.
 *   pga_batch_trim_terminal_repeats  a new batch whose contig i is S[0 : len - trim[i]], copied device to device, flagged circular where
 *                                    trim[i] > 0 or `src` says so; mask_case and the set labels are copied, the caller's regions are
 *                                    clipped to the new length (empty ones dropped).  *out = NULL, and nothing is copied, when every
 *                                    trim[i] is 0.  trim[i] < 0 or 2 trim[i] > len is PGA_EINVAL naming the contig.
 * pga_find_genes on the new batch is the circular call of the trimmed contigs.  Both are calls on the context like pga_find_genes: one
 * at a time.  pga_terminal_repeat_chunk: the letters of each window the detection hashes per step (for tests that straddle it). */
int  pga_batch_terminal_repeats(pga_ctx*, const pga_batch*, const uint8_t* search /* n flags, or NULL */, int32_t min_length,
                                int32_t max_length, int32_t max_base_percent, int32_t* match_out /* n */, int32_t* trim_out /* n */);
int  pga_batch_trim_terminal_repeats(pga_ctx*, const pga_batch* src, const int32_t* trim /* n */, pga_batch** out);
int  pga_terminal_repeat_chunk(void);
/* Contig sets, one more attribute of the resident batch (meta mode): set_of_contig[i] >= 0 labels contig i as a member of that set of
 * contigs known to be one organism (the bins of a binner, the contigs of a draft genome, the segments of a virus); -1 leaves it on its
 * own.  Labels need not be dense, and the members of a set need not be adjacent in the batch.  NULL clears the labels.
 * pga_find_genes with params->meta = 1 then chooses ONE model per set:
 *   1. the GC window of every member is that of gc_A = (sum of the members' G+C counts) / (sum of their lengths), 0.0 for an empty
 *      set; every member is scored under every model of that window, in model order (contigs[i].gc stays the member's own);
 *   2. a member contributes under model m iff it has nodes and a path there, and contributes that path's score;
 *   3. S_m is the sum of the contributions under m, added as doubles in batch order; the set's model W is the one with the largest
 *      S_m among those with S_m > -100.0, the lowest index among equals;
 *   4. a member that contributed under W gets exactly the result of a contig whose winner is W (genes, node arrays, translation
 *      table); any other member, and every member of a set without W, has no genes and model -1.
 * A set of one contig, labelled or not, is the ordinary meta-mode call, bit for bit; a batch without labels runs the ordinary code.
 * Refused with PGA_EINVAL: labels below -1; a labelled batch with params->meta = 0 (pga_find_genes); a batch that carries both labels
 * and circular flags (pass 2 of a circular call holds only the circular members, so a set's sums would change their meaning).
 * pga_batch_replicate carries the labels; pga_find_genes_models, training, pga_nodes_stage and pga_find_coding_bases ignore them.
 * Not to be called while a call on the batch runs. */
int  pga_batch_set_sets(pga_batch*, const int32_t* set_of_contig /* n entries, or NULL */);
/* The choice of the last pga_find_genes call on the context, when its batch carried labels: per contig i < n the model W of its set
 * (-1: none) and S_W (NaN: none).  -1 / NaN for every contig after a call without labels. */
int  pga_set_choice(const pga_ctx*, int32_t n, int32_t* model, double* score);
/* The contributions behind that choice: out[i * n_models + m] is the path score of contig i under model m, NaN where it did not
 * contribute (m outside its set's window, no nodes, no path) and everywhere after a call without labels. */
int  pga_model_scores(const pga_ctx*, int32_t n_contigs, int32_t n_models, double* out);
/* Step 2 above (host arithmetic only): genes begin[k]..end[k], 1-based inclusive, either strand, any order, on a contig of L bases.
 * A gap is a maximal run of positions no gene covers, [gb, ge) 0-based, mid = (gb + ge) / 2.  Among the gaps with
 * L / 4 <= mid < L - L / 4 (all gaps if there is none) the widest wins, then the smallest |mid - L / 2|, then the lowest mid;
 * returns its mid, L / 2 when there is no gap, or a negative PGA_E* code. */
int  pga_circular_cut(int32_t L, int32_t n, const int32_t* begin, const int32_t* end);
int  pga_find_genes(pga_ctx*, const pga_batch*, const pga_params*, pga_result** out);
/* Single mode, contig i called with loaded model model_of_contig[i] (an index into the pga_set_models set): every contig's result
 * is identical to pga_find_genes with that one model loaded -- its nodes extracted under that model's translation table, its genes,
 * node arrays (want_nodes), contigs[i].model = model_of_contig[i] and score.  params->meta must be 0; PGA_EINVAL for an index
 * outside [0, n_models).  Many genomes under their own models in one call (ref: the per-genome loop of benches/run_single). */
int  pga_find_genes_models(pga_ctx*, const pga_batch*, const pga_params*, const int32_t* model_of_contig, pga_result** out);
/* A new batch whose entry i is a copy of contig contig_of_entry[i] of the resident batch `src` (of the same context), copied device
 * to device: the same genome under K models in one call needs one upload, not K.  Entries may repeat contigs and come in any order;
 * they do not share letters. */
int  pga_batch_replicate(pga_ctx*, const pga_batch* src, int32_t n, const int32_t* contig_of_entry, pga_batch** out);
/* What pga_find_genes_models runs, reduced on the device to three numbers per contig: coding_bases[i] = the positions of contig i
 * (1 .. length) that lie in [begin, end] of at least one of its genes, either strand, overlaps counted once; n_genes[i] and score[i]
 * as pga_contig_result reports them.  The gene records stay on the device (a bitmap of the batch's bases, a popcount per contig);
 * params->want_nodes is ignored (no node arrays are kept).  The coding density of a genome under a model is the sum of its contigs'
 * coding_bases over the sum of their lengths: the measure that tells translation table 4 from 11. */
int  pga_find_coding_bases(pga_ctx*, const pga_batch*, const pga_params*, const int32_t* model_of_contig, int64_t* coding_bases,
                           int32_t* n_genes, double* score);

/* ---- stage level --------------------------------------------------------- */
/* The node arrays as the reference's Nodes methods leave them, one pga_nodes per contig of the batch
 * (pga_result.nodes; no genes).  Later stages include the earlier ones and use model 0 of the context;
 * `params.meta` then selects the is_meta behaviour of Nodes.score, `translation_table` is only read
 * by PGA_STAGE_EXTRACT. */
#define PGA_STAGE_EXTRACT 1   /* Nodes.extract() + Nodes.sort()             (ref: lib.pyx:2501-2541, 2489-2493) */
#define PGA_STAGE_SCORE   2   /* + Nodes.reset_scores() + Nodes.score()     (ref: lib.pyx:2543-2595)            */
#define PGA_STAGE_OVERLAP 3   /* + _record_overlapping_starts(flag = 1)      (ref: lib.pyx:2279-2329, 5302)      */
#define PGA_STAGE_SEQUENCE 4  /* Sequence.__init__ only: gc, n_unknown and masks per contig, no nodes (ref: lib.pyx:664-713) */
int pga_nodes_stage(pga_ctx*, const pga_batch*, const pga_params*, int stage, int translation_table, pga_result** out);

/* ---- translation -------------------------------------------------------------- */
/* Protein translations of gene records, computed on the device from a resident batch: one thread per codon
 * (ref: lib.pyx:2932-3047 `Gene.translate`, 770-789 `Sequence._amino`, _translation.h:4-42 the genetic codes).
 *   genes[g]         records of a pga_result of THIS batch (contig, begin, end, strand, partial flags are read)
 *   table_of_contig  translation table of every contig of the batch (what the winning model was trained with, or the caller's
 *                    choice); one of the NCBI tables the reference knows (1-6, 9-16, 21-26, 29, 30, 32, 33)
 *   unknown_residue  the letter of a codon with an unknown base ('X' in the reference)
 *   include_stop     0: a complete gene loses its final `*`
 *   strict           0: a codon with one unknown base in second or third position reads the residue all four completions agree on
 *   offsets[g]       first letter of gene g in `out`: offsets[g + 1] - offsets[g] must be (end - begin + 1) / 3, minus 1 for a
 *                    gene whose stop is not at an edge when include_stop == 0; offsets[n_genes] letters are written to `out`
 * As in the reference the first codon of a gene that does not start at an edge reads M when it is a start codon of the table,
 * and a stop codon of the table reads `*`. */
int pga_translate_genes(pga_ctx*, const pga_batch*, int64_t n_genes, const pga_gene* genes, const int32_t* table_of_contig,
                        int unknown_residue, int include_stop, int strict, const int64_t* offsets, char* out);

/* The same proteins left on the device as token ids, in the consumer's layout, in the consumer's device tensor (a protein language
 * model, an embedding search or a classifier in the same process): nothing of them comes to the host.
 *   Residues.  For gene g, the residues are exactly what pga_translate_genes yields for that record under table_of_contig,
 *     include_stop, strict and unknown_residue: M at a non-edge start codon, `*` at a stop, a gene across the origin of a circular
 *     contig reading on at base 1.  n_g is their number.
 *   Vocabulary.  vocab[128], int64 ids indexed by the 7-bit residue letter.  The caller builds it complete: every letter the kernel
 *     can emit under the chosen options -- the 20 amino acids, `*` when include_stop, and the unknown_residue letter -- has an id, its
 *     own or the caller's id for unknown.  The kernel does a plain look-up and never meets an unmapped letter.
 *   Tokens of gene g.  [bos] if given, then vocab[r] for the first R_g residues, then [eos] if given.  With s the number of special
 *     tokens (0 to 2), R_g = n_g without max_length (max_length == 0), otherwise R_g = min(n_g, max_length - s); max_length must be at
 *     least s + 1.  len_g = s + R_g; a gene with no residues has len_g = s.
 *   Layouts.  PGA_TOKENS_RAGGED: gene g is out[off[g] .. off[g + 1]), off the exclusive scan of len (the consumer's cu_seqlens);
 *     elements at or beyond off[G] are not written.  PGA_TOKENS_PADDED: out is G rows of stride S = row_stride >= W = row_width >=
 *     max(len_g) elements; row g holds its tokens, then pad, up to W: every one of the G x W elements is written, elements W .. S of a
 *     row are not touched.
 *   Elements.  uint8, int32 or int64 (elem_bytes 1, 4, 8).  Every id (vocabulary, bos, eos, pad) must fit the element type: 0 .. 255,
 *     the int32 range, any int64.  d_out need only be element-aligned.
 *   Sizes.  len and off are computed on the host from the gene coordinates; len_out[g] = len_g.  Nothing about sizes comes back from
 *     the device.
 *   Validation.  Everything is checked on the host before anything is allocated or launched; a failure returns PGA_EINVAL and
 *     pga_last_error names the gene or field: element width, id ranges, max_length, W against the longest gene, n_out_elems against
 *     the layout (off[G], or (G - 1) S + W), gene records inside their contig (the checks of pga_translate_genes), table validity,
 *     the alignment of d_out, and hipPointerGetAttributes calling d_out device memory of the context's device: a host pointer is
 *     refused there and never reaches a kernel.
 *   Ordering.  d_out may be a fresh block from a caching allocator that earlier work on the caller's stream still uses.  The call
 *     records an event on `stream`, makes the context's upload stream wait for it, runs the kernel there and synchronises before it
 *     returns (the discipline of pga_batch_create_device).  On return the tensor is complete for any stream.  The concurrency rule is
 *     that of pga_batch_create: one such call or upload at a time per context, and it may run beside a pga_find_genes of the context.
 * Gene records come from the host, as for pga_translate_genes: any subset or reordering of a result's records may be passed. */
#define PGA_TOKENS_RAGGED 0
#define PGA_TOKENS_PADDED 1
#define PGA_TOKEN_NONE    INT64_MIN   /* bos / eos: no such token */
typedef struct pga_token_opts {
    int32_t elem_bytes;         /* 1, 4 or 8 */
    int32_t layout;             /* PGA_TOKENS_RAGGED or PGA_TOKENS_PADDED */
    int64_t row_width;          /* W, padded layout (ignored for ragged) */
    int64_t row_stride;         /* S, padded layout (ignored for ragged) */
    int32_t include_stop, strict;
    int32_t unknown_residue;    /* a single ASCII character, 'X' in the reference */
    int32_t _pad;
    int64_t max_length;         /* 0: no limit */
    int64_t vocab[128];
    int64_t bos, eos;           /* PGA_TOKEN_NONE: none */
    int64_t pad;                /* padded layout */
} pga_token_opts;
int pga_translate_genes_tokens(pga_ctx*, const pga_batch*, int64_t n_genes, const pga_gene* genes, const int32_t* table_of_contig,
                               const pga_token_opts*, void* d_out /* device memory of the context's device */, int64_t n_out_elems,
                               void* stream /* hipStream_t, NULL = the null stream */, int64_t* len_out /* [n_genes], host */);

/* The annotation of every base of a resident batch, left on the device as a tensor in the shape of the input: token-classification
 * targets, codon-phase supervision, loss masks, GC3 or intergenic statistics in the same process.  The letters of the batch are not
 * read; nothing comes to the host.
 *   Raw byte.  Take contig i of a resident batch with length L_i.  This is the length the batch holds, so for a record trimmed by
 *     trim_terminal_repeats it is the trimmed length.  Take position p in [0, L_i).
 *     A gene record of contig i has 1-based inclusive [b, e], with 1 <= b <= L_i and 3 <= e - b + 1 <= L_i.  e > L_i is allowed only
 *     on a contig flagged circular.  The record covers p through q = p + 1 or q = p + 1 + L_i, whichever lies in [b, e].  At most one
 *     of the two does.
 *     A covering record contributes:
 *       0x01 / 0x02 / 0x04   forward gene (strand == 1): codon position (q - b) % 3 = 0 / 1 / 2
 *       0x08 / 0x10 / 0x20   reverse gene: codon position (e - q) % 3 = 0 / 1 / 2, counted in the gene's own reading direction
 *       0x40 (start codon)   forward: q <= b + 2 and partial_begin == 0.  Reverse: q >= e - 2 and partial_end == 0
 *       0x80 (stop codon)    forward: q >= e - 2 and partial_end == 0.  Reverse: q <= b + 2 and partial_begin == 0
 *     The partial flags are in sequence orientation, as translate_tokens.inl already notes.
 *     raw[p] is the OR over all covering records, and 0 without one.  The rule is a union, so it does not depend on the order of the
 *     records.  Same-strand overlaps land in different bits because they are in different frames.  A start or stop codon that
 *     straddles the origin of a circle is handled by q.
 *   Classes.  class_map[256] holds int64 ids, built complete by the host layer.  The element for p is class_map[raw[p]].  The kernel
 *     does a plain look-up.
 *   Layouts.  Padded (PGA_TOKENS_PADDED): B rows of stride S >= W >= max(L_i).  Row i holds its L_i elements, then pad up to W.  All
 *     B x W elements are written.  Elements W .. S of a row are not touched.  Ragged (PGA_TOKENS_RAGGED): contig i is
 *     out[off[i] .. off[i + 1]), with off the exclusive scan of L_i.  Nothing at or beyond off[B] is written.
 *     Elements are uint8, int32 or int64.  Every id and pad must fit the element type.  d_out need only be element-aligned.
 *     len_out[i] = L_i.  Nothing about sizes comes back from the device.
 *   Validation.  Everything is checked on the host before anything is allocated or launched.  A failure returns PGA_EINVAL, and
 *     pga_last_error names the record or field.  The checks are: element width; id ranges; W against the longest contig; n_out_elems
 *     against the layout (off[B], or (B - 1) S + W); every record inside its contig, with a whole number of codons, and e > L_i only
 *     where the contig is flagged circular; the alignment of d_out; and hipPointerGetAttributes calling d_out device memory of the
 *     context's device.
 *   Ordering and concurrency.  Those of pga_translate_genes_tokens exactly: the call records an event on `stream`, runs on the
 *     context's upload stream behind it, one such call or upload at a time per context, and synchronises before it returns.
 * Gene records come from the host.  Any subset or order of a result's records may be passed. */
typedef struct pga_label_opts {
    int32_t elem_bytes;         /* 1, 4 or 8 */
    int32_t layout;             /* PGA_TOKENS_RAGGED or PGA_TOKENS_PADDED */
    int64_t row_width;          /* W, padded layout (ignored for ragged) */
    int64_t row_stride;         /* S, padded layout (ignored for ragged) */
    int64_t class_map[256];     /* the id of every raw byte */
    int64_t pad;                /* padded layout */
} pga_label_opts;
int pga_label_bases(pga_ctx*, const pga_batch*, int64_t n_genes, const pga_gene* genes, const pga_label_opts*,
                    void* d_out /* device memory of the context's device */, int64_t n_out_elems,
                    void* stream /* hipStream_t, NULL = the null stream */, int64_t* len_out /* [contigs of the batch], host */);

/* The nucleotides of every gene and of the region around it, in the gene's own reading direction, left on the device as token ids,
 * one row per gene record: coding sequences as codon tokens, fixed start contexts, upstream and downstream flanks for a model in the
 * same process.  Only the letters the windows name are read; nothing comes to the host.
 *   Positions.  Gene record g lies on contig i.  L is the length the batch holds for that contig.  It is the trimmed length after
 *     trim_terminal_repeats, as for pga_label_bases.  The record is [b, e], 1-based and inclusive, n = e - b + 1, with a strand.
 *     The gene's reading axis gives offset t (any integer) the position q(t) = b + t on the forward strand and q(t) = e - t on the
 *     reverse strand.  Two anchors are defined: start = 0 and end = n, one past the gene's last base in reading direction.
 *     A window is from = (anchor, delta) to to = (anchor, delta).  It covers offsets t_lo = anchor_from + delta_from up to but
 *     excluding t_hi = anchor_to + delta_to.  Its m_g = max(0, t_hi - t_lo) bases are read in reading direction.  An empty or
 *     inverted window on a short gene is a row without bases.  It is not an error.
 *     Examples: (start, 0) .. (end, 0) is the gene as -d prints it.  (start, -60) .. (start, +30) is a fixed 90-base start context.
 *     (end, 0) .. (end, +50) is the downstream region.
 *   Base class.  On a contig flagged circular, q is taken modulo L: ((q - 1) mod L) + 1, floor modulo.  It is defined for any q, so a
 *     flank longer than the contig goes round more than once.  On a linear contig, q < 1 or q > L is the class outside.  Otherwise
 *     the letter reads A, C, G, T in either case.  Anything else reads N.  This is exactly the reading of Gene.sequence().  A reverse
 *     gene's letter is complemented: A and T swap, C and G swap, N stays N.
 *   Units.  PGA_WINDOW_BASES: one token per base.  ids[0..3] = A, C, G, T.  ids[4] = N.  ids[5] = outside.
 *     PGA_WINDOW_CODONS: both deltas must be multiples of 3.  Token j covers offsets t_lo + 3j .. t_lo + 3j + 2.  The id is
 *     ids[16 c0 + 4 c1 + c2], with A, C, G, T = 0, 1, 2, 3.  This is the public ACGT order.  It is not the internal digit order.
 *     A codon that touches outside gets ids[65].  Otherwise a codon with an N gets ids[64].  m_g is a multiple of 3, because records
 *     are whole codons.
 *   Tokens of a row, layouts, elements.  These follow pga_translate_genes_tokens exactly, with u_g = m_g (bases) or m_g / 3 (codons)
 *     in the place of the residues n_g: [bos] if given, the ids of the first R_g units, [eos] if given; max_length cuts on the far
 *     side, and eos survives the cut.  The layout is ragged or padded with W, S and pad.  Elements W .. S of a row are untouched.
 *     Elements are uint8, int32 or int64.  d_out need only be element-aligned.  len_out[g] is computed on the host.
 *   Validation.  Everything is checked on the host, before anything is allocated or launched.  A failure returns PGA_EINVAL, and
 *     pga_last_error names the gene or field.  The checks are: element width and id ranges; unit and anchors; |delta| <= 2^30; deltas
 *     that are multiples of 3 for codons; max_length; the record checks of pga_label_bases (every record inside its contig, whole
 *     codons, and e > L only on a circle); W against the longest row; n_out_elems against the layout; the alignment of d_out; and the
 *     device-pointer query on it.
 *   Ordering and concurrency.  Those of pga_translate_genes_tokens.
 * Gene records come from the host, in any subset or order. */
#define PGA_WINDOW_BASES  0
#define PGA_WINDOW_CODONS 1
#define PGA_WINDOW_START  0     /* anchor: offset 0, the gene's first base in reading direction */
#define PGA_WINDOW_END    1     /* anchor: offset n, one past the gene's last base in reading direction */
typedef struct pga_window_opts {
    int32_t elem_bytes;         /* 1, 4 or 8 */
    int32_t layout;             /* PGA_TOKENS_RAGGED or PGA_TOKENS_PADDED */
    int64_t row_width;          /* W, padded layout (ignored for ragged) */
    int64_t row_stride;         /* S, padded layout (ignored for ragged) */
    int32_t unit;               /* PGA_WINDOW_BASES or PGA_WINDOW_CODONS */
    int32_t from_anchor, to_anchor;   /* PGA_WINDOW_START or PGA_WINDOW_END */
    int32_t _pad;
    int64_t from_delta, to_delta;
    int64_t max_length;         /* 0: no limit */
    int64_t ids[66];            /* bases: [0..5] are read.  Codons: all 66 */
    int64_t bos, eos;           /* PGA_TOKEN_NONE: none */
    int64_t pad;                /* padded layout */
} pga_window_opts;
int pga_gene_windows(pga_ctx*, const pga_batch*, int64_t n_genes, const pga_gene* genes, const pga_window_opts*,
                     void* d_out /* device memory of the context's device */, int64_t n_out_elems,
                     void* stream /* hipStream_t, NULL = the null stream */, int64_t* len_out /* [n_genes], host */);

/* The k-mers of every contig, or of every gene record, counted into integer vectors on the device, one row per contig or per gene:
 * tetranucleotide frequencies for binning, codon usage, in-frame dicodon counts, amino-acid composition for a model in the same
 * process.  Only the letters the rows name are read; nothing comes to the host.
 *   Letters and codes.  A letter reads A, C, G, T in either case; anything else reads N.  This is the reading of pga_gene_windows.
 *     The code of a k-mer c0 c1 .. c(k-1) is sum c_j * 4^(k-1-j) with A, C, G, T = 0, 1, 2, 3.  This is the public ACGT order, first
 *     base most significant.  GeneWindows uses the same order for codons (16 c0 + 4 c1 + c2).  A window that holds an N is not
 *     counted.  1 <= k <= 6.
 *   Rows.  L is the length the batch holds for a contig.  After trim_terminal_repeats it is the trimmed length.  There are three
 *     kinds of row.
 *     PGA_COUNT_CONTIG: one row per contig, forward strand as stored.  step must be 1.  A linear contig has window starts
 *       p = 0 .. L-k (none if L < k).  A contig flagged circular has p = 0 .. L-1.  Base j of a window is read at (p + j) mod L.  If
 *       L < k there are no windows.
 *     PGA_COUNT_GENE: one row per gene record [b, e], n = e - b + 1.  The gene is read in its own direction: complemented on the
 *       reverse strand, and wrapped modulo L on a circle when e > L.  This is exactly the axis q(t) of pga_gene_windows.  Window
 *       starts are t = 0, step, 2*step, .. while t + k <= n.  Windows lie wholly inside the gene.  step is 1 or 3.  k = 3, step = 3
 *       is codon usage, including the start and stop codon the record holds.  k = 6, step = 3 is in-frame dicodons.  Records come
 *       from the host, in any subset or order.  The record checks are those of pga_label_bases.
 *     PGA_COUNT_CONTIG_GENES: one row per contig.  It is the sum of the PGA_COUNT_GENE rows of the records given on that contig, and
 *       zero where there are none.  It uses the same kernel, with the contig's row as destination.
 *   Bins.  The caller passes bin_of_code: 4^k int32 entries in [-1, n_bins).  -1 means the window is not counted.  n_bins <= 4096.
 *     The identity table gives the plain counts.
 *   Output.  d_out holds int32, [R, S] row-major with S = row_stride >= n_bins.  Elements 0 .. n_bins-1 of every row are set to the
 *     counts.  Whatever the tensor held before does not matter.  Elements n_bins .. S-1 are untouched.  d_out need only be 4-byte
 *     aligned.  win_out[r] (host, int64) is the number of window positions of row r, whether counted or not.  It is host arithmetic.
 *   Validation.  Everything is checked on the host before anything is allocated or launched.  A failure returns PGA_EINVAL and
 *     pga_last_error names the field or gene.  The checks are: k, step and the row kind; the table's range; S and n_out_elems; the
 *     record checks of pga_label_bases; a row whose window positions exceed INT32_MAX; the alignment of d_out and the device-pointer
 *     query on it.
 *   Ordering and concurrency.  Those of pga_translate_genes_tokens.  The result depends on the arguments alone.
 * pga_kmer_counts_chunk: the window starts of one piece of work (for tests that straddle it). */
#define PGA_COUNT_CONTIG       0
#define PGA_COUNT_GENE         1
#define PGA_COUNT_CONTIG_GENES 2
typedef struct pga_count_opts {
    int32_t rows;                 /* PGA_COUNT_CONTIG / PGA_COUNT_GENE / PGA_COUNT_CONTIG_GENES */
    int32_t k, step, n_bins;
    int64_t row_stride;           /* S */
    const int32_t* bin_of_code;   /* host, 4^k entries */
} pga_count_opts;
int pga_count_kmers(pga_ctx*, const pga_batch*, int64_t n_genes, const pga_gene* genes /* ignored for PGA_COUNT_CONTIG */,
                    const pga_count_opts*, void* d_out /* device memory of the context's device */, int64_t n_out_elems,
                    void* stream /* hipStream_t, NULL = the null stream */,
                    int64_t* win_out /* [R]: n_genes for PGA_COUNT_GENE, else the contigs of the batch; host */);
int pga_kmer_counts_chunk(void);

/* Every candidate start site of a gene record's ORF, with its scores under the winning model, left on the device as three tensors:
 * positives and hard negatives for a translation-initiation-site model, the input of a re-ranker of the starts or of a start-correction
 * step in the same process.  Nothing but 8 bytes per gene comes to the host.
 *   The record.  Gene record g lies on contig i of the batch whose result the context has on record.  On record means: the last finder
 *     call on the context kept its node arena on the device, with want_nodes 1 or PGA_NODES_DEVICE.  This is exactly the condition
 *     PGA_RENDER_SCO has.
 *   Candidates.  Let x = start_ndx be the record's start node within that contig's node arrays.  The candidates of g are all nodes of
 *     contig i that satisfy three conditions: the node is not a stop node (type != 3); strand == strand[x]; stop_val == stop_val[x].
 *   Row order.  Rows run in reading direction, outermost (longest ORF) first: ascending ndx on the forward strand, descending ndx on the
 *     reverse strand.
 *   Row data.  n_g >= 1 is the number of candidates in the row.  chosen_g is the index of node x within the row.
 *   Values per candidate node y.  These are the values pga_result.nodes reports with want_nodes = 1: in single mode the *_dp fields, in
 *     meta mode the fresh re-score, as write_scores prints them.
 *       position = ndx[y] + 1.  This is the begin the gene would have with this start on the forward strand, and the end on the reverse
 *         strand.
 *       type = edge[y] ? 3 : type[y] & 3.  The codes are 0 ATG, 1 GTG, 2 TTG, 3 Edge.
 *       scores: F columns in the caller's order, drawn from PGA_START_TOTAL (cscore + sscore, added in double), PGA_START_CSCORE,
 *         _SSCORE, _RSCORE, _USCORE, _TSCORE, and PGA_START_GC_CONT.  A float32 tensor holds the double value rounded once to nearest.
 *   Two calls.  The row lengths are sizes the host cannot compute from the gene records, so the call is split.
 *     pga_start_plan_create validates the records, puts the arena in sorted order (the order of the start-score file), finds every
 *     gene's group, and brings home count_out[g] = n_g and chosen_out[g] = chosen_g.  The plan holds the device memory the second step
 *     needs: a block the context keeps and hands to the next plan once this one is freed, so a steady run of create / write / free
 *     allocates nothing.  The plan remembers which recorded result it belongs to.
 *     pga_start_plan_write writes the three tensors.  It returns PGA_EINVAL if a later finder call, stage call, training or model load
 *     has replaced the recorded result.  A plan may be written more than once, with other options.
 *     pga_start_plan_nodes brings home, for every candidate in ragged order, its index in the contig's node arrays (4 bytes per
 *     candidate): the start_ndx a gene record of that candidate has.  It reads the plan alone, so it works after the recorded result
 *     has been replaced.
 *     pga_start_plan_free gives the block back.  pga_destroy orphans the plans that still live: such a plan can only be freed.
 *   Layouts.  PGA_TOKENS_RAGGED: positions [T], types [T] and scores [T, F], with T = sum n_g; gene g owns candidates off[g] ..
 *     off[g + 1], off the exclusive scan of n_g.  Nothing at or beyond T is written.  PGA_TOKENS_PADDED: [G, W], [G, W] and [G, W, F]
 *     with a row stride S >= W >= max n_g, counted in candidates for all three tensors.  All G x W candidates are written: values
 *     first, then index_pad (positions, types) and score_pad (every column).  Candidates W .. S of a row are untouched.
 *   Elements.  positions and types are int32 or int64 (index_bytes 4 or 8), scores float32 or float64 (score_bytes 4 or 8).  The
 *     outputs need only be element-aligned.
 *   Refusals.  PGA_EINVAL, with pga_last_error naming the gene or field.  pga_start_plan_create, on the host before anything is
 *     launched: no node arena on record for this batch (the test the score renderer applies); a batch with a contig flagged circular
 *     or trimmed by trim_terminal_repeats (the nodes of a circle live in the rotated contig's coordinates); a record that names no
 *     contig of the batch; start_ndx or stop_ndx outside the contig's nodes.  Three checks read the arena, which lies on the device,
 *     so the look-up kernel makes them and reports with the counts, before any tensor is touched: a start_ndx node that is a stop
 *     node; a strand that differs from the record's; ndx + 1 that differs from the record's begin (forward) or end (reverse).
 *     pga_start_plan_write, on the host before anything is launched: element widths; pads that do not fit the element type; an
 *     unknown or repeated field; W below the longest row; the sizes against the layout; the alignment of the outputs; and the
 *     device-pointer query on every output.
 *   Ordering and concurrency.  pga_start_plan_write follows pga_translate_genes_tokens: it waits for what `stream` holds, and on return
 *     the tensors are complete for any stream.  pga_start_plan_create runs on the context's own stream and shares the renderer's
 *     scratch, so it follows pga_render_genes.  No call that runs the finder may run on the context between the two.
 *   The result depends on the arguments alone.
 * Gene records come from the host, in any subset or order.  They need not be genes the finder called: any start node of the record's
 * contig makes a valid record. */
#define PGA_START_TOTAL   0
#define PGA_START_CSCORE  1
#define PGA_START_SSCORE  2
#define PGA_START_RSCORE  3
#define PGA_START_USCORE  4
#define PGA_START_TSCORE  5
#define PGA_START_GC_CONT 6
typedef struct pga_start_opts {
    int32_t index_bytes;        /* 4 or 8: positions and types */
    int32_t score_bytes;        /* 4 or 8: float32 or float64 */
    int32_t layout;             /* PGA_TOKENS_RAGGED or PGA_TOKENS_PADDED */
    int32_t n_fields;           /* F, 1 .. 7 */
    int64_t row_width;          /* W in candidates, padded layout (ignored for ragged) */
    int64_t row_stride;         /* S in candidates, padded layout (ignored for ragged) */
    int32_t fields[7];          /* PGA_START_*: the first n_fields are read, none twice */
    int32_t _pad;
    int64_t index_pad;          /* padded layout: positions and types behind a row's candidates */
    double  score_pad;          /* padded layout: every score column behind a row's candidates */
} pga_start_opts;
typedef struct pga_start_plan pga_start_plan;
int  pga_start_plan_create(pga_ctx*, const pga_batch*, int64_t n_genes, const pga_gene* genes, pga_start_plan** plan,
                           int32_t* count_out /* [n_genes], host */, int32_t* chosen_out /* [n_genes], host */);
int  pga_start_plan_write(pga_ctx*, const pga_start_plan*, const pga_start_opts*, void* d_positions, void* d_types, void* d_scores,
                          int64_t n_positions, int64_t n_types, int64_t n_scores /* elements of each */,
                          void* stream /* hipStream_t, NULL = the null stream */);
int  pga_start_plan_nodes(pga_ctx*, const pga_start_plan*, int32_t* node_out /* [n_out >= T], host */, int64_t n_out);
void pga_start_plan_free(pga_ctx* /* unused: the plan knows its context */, pga_start_plan*);
/* `bytes` of device memory of the context's device to the host (what DeviceStarts.records() reads positions with): waits for what
 * `stream` holds first.  PGA_EINVAL when the runtime does not call d_src device memory.  The context may be NULL -- a result that
 * outlives the call that made it reads its tensor this way: the pointer then names its device, and no message is kept. */
int  pga_device_read(pga_ctx*, const void* d_src, int64_t bytes, void* dst, void* stream /* hipStream_t, NULL = the null stream */);

/* Gene records with the same predicted protein (or the same nucleotides), grouped on the device, exactly: which records are copies of
 * each other, one representative of every group, and a portable digest of every record's string.  What a caller that embeds, searches
 * or catalogues the proteins does first -- drop the copies -- without a letter coming to the host.
 *   Strings.  With unit = PGA_GROUP_PROTEIN the string of gene g is exactly the residue letters that pga_translate_genes yields for that
 *     record under table_of_contig, include_stop, strict and unknown_residue: M at a non-edge start codon, * at a stop, a gene across
 *     the origin of a circular contig reads on at base 1, and a gene with no residues has the empty string.  With unit =
 *     PGA_GROUP_GENE the string is all end - begin + 1 bases of the record in reading direction, in the reading of pga_gene_windows:
 *     A, C, G, T in either case give the upper-case letter, anything else gives N, the reverse strand is complemented, and a record
 *     wraps at the origin of a circle.  table_of_contig, include_stop, strict and unknown_residue are not read for this unit.
 *   Groups.  Genes g and h are in one group exactly when their strings are equal byte for byte.  A group's representative is its member
 *     with the smallest index in the array of records passed (any subset or reordering is allowed, as for pga_translate_genes_tokens).
 *     Groups are numbered 0 .. U - 1 in increasing order of their representatives, which is the order of first appearance.
 *   Digest.  A property of the string alone, so results of different calls, batches and processes can be merged with it.  M = 2^61 - 1,
 *     b0 = 0x0123456789ABCDEF, b1 = 0x1BADB002C0FFEE11.  h = 1; for every byte r of the string in order, h = (h * b + r) mod M.
 *     digest[g] = (h under b0, h under b1), two non-negative int64.  The empty string has (1, 1).  Equal digests are NOT the rule: they
 *     only drive the grouping, and every pair that is merged has had its strings compared byte for byte.
 *   Outputs.  All int64 device memory of the context's device, 8-byte aligned; any of d_representative, d_size and d_digest may be NULL.
 *       d_group          [G], required       the group of gene g
 *       d_representative [capacity >= G]     first U elements: the gene index of each group's representative
 *       d_size           [capacity >= G]     first U elements: the members of each group
 *       d_digest         [G, 2]              the digest of every gene's string
 *       n_groups         host                U -- the one size that comes back from the device
 *     Elements beyond U of d_representative and d_size, and everything outside the named elements, are not touched.
 *   Refusals.  PGA_EINVAL, pga_last_error naming the gene or field, all on the host before anything is allocated or launched: unit and
 *     unknown_residue; G above INT32_MAX; capacity below G with d_representative or d_size given; the record and table checks of
 *     pga_translate_genes; a NULL d_group; a pointer that is not 8-byte aligned; and the device-pointer query on every pointer given.
 *   Ordering and concurrency.  As pga_translate_genes_tokens: the call waits for what `stream` holds, works on the context's upload
 *     stream, and on return the tensors are complete for any stream.  One such call at a time per context; a steady run allocates
 *     nothing.
 *   The result depends on the arguments alone: integers throughout.
 * PGA_PROTEIN_GROUPS_KEY_BITS = k (1 .. 61) in the environment, read per call, makes the GROUPING sort on the low k bits of digest
 * word 0 alone and skip the comparison of lengths and of word 1 in front of the comparison of the strings: collisions abound and the
 * strings alone decide (tests and measurements).  The exported digests are unchanged.  pga_protein_groups_stats: {verification
 * rounds, pairs whose strings differed} of the context's last pga_group_proteins call. */
#define PGA_GROUP_PROTEIN 0
#define PGA_GROUP_GENE    1
typedef struct pga_group_opts {
    int32_t unit;               /* PGA_GROUP_PROTEIN or PGA_GROUP_GENE */
    int32_t include_stop;       /* as in pga_translate_genes */
    int32_t strict;
    int32_t unknown_residue;    /* a single ASCII character, e.g. 'X' */
} pga_group_opts;
int  pga_group_proteins(pga_ctx*, const pga_batch*, int64_t n_genes, const pga_gene* genes, const int32_t* table_of_contig,
                        const pga_group_opts*, int64_t* d_group, int64_t* d_representative, int64_t* d_size, int64_t* d_digest,
                        int64_t capacity, void* stream /* hipStream_t, NULL = the null stream */, int64_t* n_groups /* host */);
int  pga_protein_groups_stats(pga_ctx*, int64_t out[2]);

/* Bottom-s MinHash sketches of the gene records' strings, on the device: a fixed [G, size] int64 tensor from which the resemblance and
 * containment of any two proteins can be estimated, and whose sort yields candidate pairs -- the step behind pga_group_proteins for
 * proteins that differ in a few residues, a start codon or a truncation.  Defined by the string alone, so sketches of different
 * calls, batches and processes can be compared.
 *   Strings.  The string of gene record g is exactly that of pga_group_proteins.  unit = PGA_SKETCH_PROTEIN: the residues
 *     pga_translate_genes yields under table_of_contig, include_stop, strict and unknown_residue.  unit = PGA_SKETCH_GENE: all bases in
 *     reading direction, in the reading of pga_gene_windows.  Circular contigs wrap.  Any subset or reordering of a result's records
 *     may be passed.
 *   Letter codes.  Protein: a 128-entry byte table `classes` maps a letter to a class 0..254, or to 255 ("skip").  The default table
 *     (what the Python layer fills in) is the identity with classes[unknown_residue] = 255; a caller-given table (a reduced alphabet)
 *     decides alone.  A letter at or above 128 is skipped.  8 bits per letter, 1 <= k <= 8.  Gene: A, C, G, T map to 0..3 and N is
 *     skipped.  2 bits per letter, 1 <= k <= 32.  `classes` is not read.
 *   Windows.  Window j (0 <= j <= n - k) of a string S of n letters is valid when none of its k letters is skipped.  Its key is
 *     x = sum_i code(S[j + i]) << (bits * (k - 1 - i)), an unsigned 64-bit number.  windows[g] is the number of valid windows.  It is
 *     0 when n < k.
 *   Hash.  All arithmetic is mod 2^64:
 *       z = x + (seed + 1) * 0x9E3779B97F4A7C15
 *       z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
 *       z = (z ^ (z >> 27)) * 0x94D049BB133111EB
 *       z ^= z >> 31
 *       hash = z >> 1, a non-negative int64.
 *     seed is a uint32.  x = 0, seed = 0 gives z = 0xE220A8397B1DCDAF (the first output of splitmix64 from state 0) and
 *     hash = 0x7110541CBD8EE6D7.
 *   Sketch.  H_g is the set of distinct hashes of the valid windows of g.  count[g] = min(size, |H_g|).  sketch[g, 0 .. count[g])
 *     holds the count[g] smallest elements of H_g in ascending order.  sketch[g, count[g] .. size) is INT64_MAX.  count says which
 *     entries are real.  A genuine hash that equals INT64_MAX is not special-cased.  1 <= size <= 64.
 *   Pairs (pga_sketch_pairs).  For a pair (a, b): A and B are the real entries of the two rows.  U is their sorted distinct union.
 *     m = min(size, |U|).  union[p] = m.  shared[p] is the number of the m smallest elements of U that lie in both A and B.  This is
 *     the Mash estimator: resemblance is about shared / m, and it is 0 / 0 for two empty rows.  A pair with an index outside
 *     0 .. G - 1 gets shared = union = -1, and nothing is read for it.
 *   Outputs.  All int64 device memory of the context's device, 8-byte aligned.  d_sketch [G, size], d_count [G], d_windows [G] or NULL;
 *     d_shared [P], d_union [P].  Nothing outside the named elements is touched.  pga_sketch_pairs reads d_sketch [G, size], d_count
 *     [G] and d_pairs [P, 2] as a call of pga_sketch_proteins with the same size left them.
 *   Refusals.  PGA_EINVAL, pga_last_error naming the gene or field, all on the host before anything is allocated or launched: unit, k
 *     and size out of range; unknown_residue; G above INT32_MAX; a NULL d_sketch or d_count (d_pairs, d_shared, d_union); a pointer
 *     that is not 8-byte aligned; the device-pointer query on every pointer given; and the record and table checks of
 *     pga_translate_genes.  G = 0 and P = 0 return PGA_OK without a launch.
 *   Ordering and concurrency.  As pga_translate_genes_tokens: the call waits for what `stream` holds, works on the context's upload
 *     stream, and on return the tensors are complete for any stream.  One such call at a time per context; the records and the class
 *     table go through the upload lease, and a steady run allocates nothing.
 *   The result depends on the arguments alone: integers throughout.
 * pga_sketch_passes: the hashes behind a record's first 64 windows that passed the threshold of the record's sketch -- the insertions
 * tried, duplicates included -- in the context's last pga_sketch_proteins call, when the library was built with
 * -DPGA_SKETCH_COUNT_PASSES (measurements); -1 otherwise. */
#define PGA_SKETCH_PROTEIN 0
#define PGA_SKETCH_GENE    1
typedef struct pga_sketch_opts {
    int32_t unit;               /* PGA_SKETCH_PROTEIN or PGA_SKETCH_GENE */
    int32_t k;                  /* letters per window */
    int32_t size;               /* s: the hashes kept per record */
    uint32_t seed;
    int32_t include_stop;       /* as in pga_translate_genes */
    int32_t strict;
    int32_t unknown_residue;    /* a single ASCII character, e.g. 'X' */
    int32_t _pad;
    uint8_t classes[128];       /* protein unit: the class of every letter, 255 = skip */
} pga_sketch_opts;
int  pga_sketch_proteins(pga_ctx*, const pga_batch*, int64_t n_genes, const pga_gene* genes, const int32_t* table_of_contig,
                         const pga_sketch_opts*, int64_t* d_sketch /* [G, size] */, int64_t* d_count /* [G] */,
                         int64_t* d_windows /* [G] or NULL */, void* stream /* hipStream_t, NULL = the null stream */);
int  pga_sketch_pairs(pga_ctx*, const int64_t* d_sketch, const int64_t* d_count, int64_t n_genes, int32_t size,
                      const int64_t* d_pairs /* [P, 2] */, int64_t n_pairs, int64_t* d_shared, int64_t* d_union, void* stream);
int  pga_sketch_passes(pga_ctx*, int64_t* out);

/* Near-identical proteins clustered on the device from their sketches: which pairs of sketch rows are worth comparing, which of them
 * pass a resemblance threshold, and the connected components of those -- the step behind pga_sketch_proteins for a caller that drops
 * near-copies before embedding or searching.  It takes sketch tensors, not a batch: the rows of different calls, batches and
 * processes can be concatenated and clustered together.  Candidate generation is linear in the input, as in linclust.
 *   Inputs.  sketch [G, size] and count [G], as pga_sketch_proteins leaves them (a count outside 0 .. size is read as the nearest of
 *     the two, as pga_sketch_pairs reads it).  weight [G] (int64), or NULL, which means all weights are equal.  Options: size (1..64),
 *     probes (1..size), num, den (1 <= num <= den <= 2^20), min_union (0..size).
 *   1. Probes.  Record g probes with sketch[g, j] for j < min(probes, count[g]).  Padding behind count[g] is never a probe.  Two
 *      records with count = 0 are never joined.  A genuine hash equal to INT64_MAX inside the counted entries is a probe like any
 *      other.
 *   2. Buckets.  The bucket of hash h is every record that probes with h.  Its centre is the member of greatest weight; on a tie, the
 *      smallest index.
 *   3. Candidates.  For each bucket and each member g other than its centre c, the unordered pair (min(c, g), max(c, g)).  The
 *      candidate set is the distinct such pairs.  It holds at most G * probes pairs.
 *   4. Acceptance.  Take (shared, m) as pga_sketch_pairs defines them for the pair.  The pair is an edge exactly when
 *      m >= max(min_union, 1) and shared * den >= num * m.
 *   5. Edges.  The accepted pairs in ascending (a, b) order, a < b, each once, with their shared and m.  n_edges is the true count.
 *   6. Clusters.  The connected components of the graph on 0 .. G - 1 with those edges.  Clusters are numbered 0 .. U - 1 in
 *      increasing order of their smallest member.  cluster[g] is that number.  representative[u] is the member of greatest weight,
 *      smallest index on a tie.  size[u] is its number of members.
 *   Two limits.  Single linkage chains: a is joined to c through b although a and c are far apart.  It is meant for high thresholds.
 *     A pair whose common hashes all lie beyond the first `probes` entries of either row is not proposed.  The edges are exported so
 *     that a caller can apply a linkage of their own.
 *   Outputs.  All int64 device memory of the context's device, 8-byte aligned.
 *       d_cluster        [G], required           the cluster of record g
 *       d_representative [capacity >= G], NULL   first U elements: each cluster's representative
 *       d_size           [capacity >= G], NULL   first U elements: the members of each cluster
 *       d_edges          [edge_capacity, 2]      the first min(edge_capacity, n_edges) edges, (a, b) each
 *       d_edge_shared    [edge_capacity]         their shared
 *       d_edge_union     [edge_capacity]         their m
 *       n_clusters, n_edges   host               U, and the true number of edges whatever edge_capacity is
 *     d_representative and d_size may be NULL; the three edge arrays may be NULL all together.  Nothing outside the named elements
 *     is touched.
 *   Refusals.  PGA_EINVAL, pga_last_error naming the field, all on the host before anything is allocated or launched: an option out
 *     of range; G above INT32_MAX, or G * probes above INT32_MAX; capacity below G with d_representative or d_size given; a negative
 *     edge_capacity; a NULL d_sketch, d_count, d_cluster, options or count pointer; edge arrays given only in part; a pointer that is
 *     not 8-byte aligned; and the device-pointer query on every pointer given.  G = 0 returns PGA_OK with both counts 0 and no launch.
 *   Ordering and concurrency.  As pga_group_proteins: the call waits for what `stream` holds, works on the context's upload stream,
 *     and on return the tensors are complete for any stream.  One such call at a time per context.  The work arrays -- 44 bytes per
 *     probe slot, 32 per record -- are a block the context keeps and grows: a steady run allocates nothing, and the result does not
 *     depend on what earlier calls left there.
 *   The result depends on the arguments alone: integers throughout, and every atomic is a max, a min, an add or a compare-and-swap
 *     whose outcome does not depend on the order of arrival.
 * pga_cluster_stats: {probes, distinct candidates, edges, clusters} of the context's last pga_cluster_sketches call. */
typedef struct pga_cluster_opts {
    int32_t size;               /* s of the sketches */
    int32_t probes;             /* leading entries of a row that propose pairs */
    int32_t num, den;           /* the threshold: shared / m >= num / den */
    int32_t min_union;          /* the least m of an edge */
    int32_t _pad;
} pga_cluster_opts;
int  pga_cluster_sketches(pga_ctx*, const int64_t* d_sketch, const int64_t* d_count, const int64_t* d_weight /* or NULL */, int64_t n,
                          const pga_cluster_opts*, int64_t* d_cluster /* [n], required */, int64_t* d_representative, int64_t* d_size,
                          int64_t capacity, int64_t* d_edges /* [edge_capacity, 2] */, int64_t* d_edge_shared, int64_t* d_edge_union,
                          int64_t edge_capacity, void* stream /* hipStream_t, NULL = the null stream */, int64_t* n_clusters /* host */,
                          int64_t* n_edges /* host */);
int  pga_cluster_stats(pga_ctx*, int64_t out[4]);

/* Edges verified against the proteins themselves: an exact, integer, banded edit distance for pairs of token rows, a threshold on
 * it, and the connected components of a caller's edge list -- the step behind pga_cluster_sketches for a caller who wants to know
 * that two proteins are 90 % identical, not that their sketches say so.  The rows are tokens from anywhere: the tokens of
 * pga_translate_genes_tokens or pga_gene_windows in either layout, or several calls' tensors joined.
 *   Inputs (pga_align_pairs).  d_tokens: device memory of n_elems elements of elem_bytes 1, 4 or 8; it need only be element-aligned.
 *     row_begin [G] and row_len [G]: host int64 arrays, row g is tokens[row_begin[g] .. row_begin[g] + row_len[g]).  d_pairs [P, 2]:
 *     int64, device -- in practice the edges of pga_cluster_sketches.  Options: max_distance (0 .. 255), num, den
 *     (1 <= num <= den <= 2^20).
 *   Outputs.  d_distance [P]: int64, required.  d_pass [P]: int64, or NULL.  Nothing outside the named elements is touched.
 *   For pair p = (a, b):
 *   1. If a or b lies outside 0 .. G - 1: distance = -1 and pass = 0.  This is the convention of pga_sketch_pairs; nothing is read for
 *      such a pair.
 *   2. Otherwise let ed be the unit-cost Levenshtein distance of the two rows.  Elements are compared for equality over all their
 *      bits.  bos, eos and pad are elements like any other.  a == b gives 0, and two empty rows give 0.
 *   3. distance = min(ed, max_distance + 1).  The value max_distance + 1 means "more than max_distance".  The band is an implementation
 *      detail and not part of the rule.  By Ukkonen's argument, a DP confined to diagonals |j - i| <= max_distance finds every distance
 *      <= max_distance exactly.  |len_a - len_b| > max_distance decides a pair without a DP.
 *   4. pass = 1 exactly when distance <= max_distance and distance * den <= (den - num) * max(len_a, len_b).  That is identity over
 *      the longer row, 1 - ed / longer >= num / den, in integers.  The result depends on the arguments alone.
 *   Refusals.  PGA_EINVAL, pga_last_error naming the row or field, all on the host before anything is allocated or launched:
 *     elem_bytes; max_distance, num, den; G or P above INT32_MAX; a row that does not lie inside 0 .. n_elems, or whose length is
 *     outside 0 .. 2^30; a NULL d_pairs or d_distance (d_tokens where a row has an element); a pointer that is not aligned to its
 *     elements; and the device-pointer query on every pointer given.  P = 0 returns PGA_OK without a launch.
 *   Ordering and concurrency.  As pga_sketch_pairs: the call waits for what `stream` holds, works on the context's upload stream, and
 *     on return the tensors are complete for any stream.  One such call at a time per context; row_begin and row_len go through the
 *     upload lease, and a steady run allocates nothing.
 * pga_align_stats: {pairs, pairs decided without a DP, pairs that ran the DP, pairs that passed} of the context's last
 * pga_align_pairs call.
 *
 * pga_cluster_edges: the connected components of a caller's edge list -- the edges of pga_cluster_sketches filtered by any rule,
 * d_pass of pga_align_pairs among them.
 *   Inputs.  d_edges [E, 2]: int64.  d_keep [E]: int64 or NULL; nonzero means use the edge, NULL means use all.  n: the number of
 *     records.  d_weight [n]: int64 or NULL, which means all weights are equal.
 *   Outputs.  d_cluster [n], required.  d_representative and d_size: optional, with capacity >= n.  *n_clusters.  *n_used: the kept
 *     edges with both indices in 0 .. n - 1.
 *   A kept edge with an index out of range is ignored and not counted.  a == b is counted and joins nothing.
 *   Clusters.  The connected components of the graph on 0 .. n - 1 with the used edges.  Clusters are numbered 0 .. U - 1 in
 *     increasing order of their smallest member.  cluster[g] is that number.  representative[u] is the member of greatest weight,
 *     smallest index on a tie.  size[u] is its number of members.
 *   Refusals.  PGA_EINVAL, all on the host before anything is allocated or launched: n or E negative or above INT32_MAX; capacity
 *     below n with d_representative or d_size given; a NULL d_cluster or count pointer (d_edges where E > 0); a pointer that is not
 *     8-byte aligned; and the device-pointer query on every pointer given.  n = 0 returns PGA_OK with both counts 0 and no launch.
 *   Ordering, concurrency and work memory: those of pga_cluster_sketches, whose block of the context it shares (32 bytes per
 *     record).  The result depends on the arguments alone. */
typedef struct pga_align_opts {
    int32_t elem_bytes;         /* 1, 4 or 8 */
    int32_t max_distance;       /* 0 .. 255 */
    int32_t num, den;           /* the threshold: 1 - distance / longer >= num / den */
} pga_align_opts;
int  pga_align_pairs(pga_ctx*, const void* d_tokens, int64_t n_elems, const int64_t* row_begin /* host [G] */,
                     const int64_t* row_len /* host [G] */, int64_t n_rows, const int64_t* d_pairs /* [P, 2] */, int64_t n_pairs,
                     const pga_align_opts*, int64_t* d_distance /* [P] */, int64_t* d_pass /* [P] or NULL */,
                     void* stream /* hipStream_t, NULL = the null stream */);
int  pga_align_stats(pga_ctx*, int64_t out[4]);
int  pga_cluster_edges(pga_ctx*, const int64_t* d_edges /* [E, 2] */, const int64_t* d_keep /* [E] or NULL */, int64_t n_edges,
                       int64_t n, const int64_t* d_weight /* [n] or NULL */, int64_t* d_cluster /* [n], required */,
                       int64_t* d_representative, int64_t* d_size, int64_t capacity, void* stream, int64_t* n_clusters /* host */,
                       int64_t* n_used /* host */);

/* ---- text output ------------------------------------------------------------------ */
/* GFF, protein FASTA, gene FASTA, GenBank and the start-score file of gene records, rendered on the device from a resident
 * batch: byte for byte what the host writers Genes.write_gff / write_translations / write_genes / write_genbank / write_scores
 * emit, contig after contig (ref: lib.pyx:3405-3894).
 * A length pass, an exclusive scan and a write pass per format; one text arena per format, copied back once.
 * PGA_RENDER_SCO reads the node arrays the last finder call on the context kept on the device (want_nodes 1 or
 * PGA_NODES_DEVICE) for exactly this result (`contigs`) and batch; PGA_EINVAL otherwise. */
#define PGA_RENDER_GFF 1
#define PGA_RENDER_FAA 2
#define PGA_RENDER_FNA 4
#define PGA_RENDER_GBK 8
#define PGA_RENDER_SCO 16
typedef struct pga_render_opts {
    int32_t     formats;            /* PGA_RENDER_* bits */
    int32_t     meta;               /* run_type=Metagenomic (1) or Single (0) in the GFF header */
    int64_t     first_seqnum;       /* seqnum of contig 0 (the reference counts sequences from 1) */
    const char* source;             /* GFF column 2, e.g. "pyrodigal_amd_v0.1.0" (tool name + version separator + version) */
    const char* version;            /* GFF header "version=", e.g. "pyrodigal_amd.v0.1.0" */
    const char* const* model_desc;  /* [n_models] the model="..." of the GFF header ("Ab initio" in single mode) */
    int32_t     gff_header, gff_include_translation_table, gff_full_id;
    int32_t     faa_width, faa_translation_table /* 0: the contig's model's */, faa_include_stop, faa_strict, faa_full_id;
    int32_t     fna_width, fna_full_id;
    double      fallback_margin;    /* a line whose confidence lies this close to a %.2f rounding midpoint is left to the host
                                     * (the device exp may differ from the host's by an ulp); 1e-9 */
    /* GenBank (write_genbank): LOCUS division ("BCT"), date as "%d-%b-%y" upper case ("16-OCT-26"), the version in
     * /inference="ab initio prediction:pyrodigal_amd:<version>", translation table (0: the contig's model's), strict translation */
    const char* gbk_division;
    const char* gbk_date;
    const char* gbk_version;
    int32_t     gbk_translation_table, gbk_strict;
    /* start-score file (write_scores): the three header lines of every contig */
    int32_t     sco_header;
    int32_t     _pad1;
} pga_render_opts;
typedef struct pga_text {
    char*    data;          /* `size` bytes in pinned host memory the CONTEXT owns (kept and grown across calls): valid until the
                             * next pga_render_genes on the context or its pga_destroy -- copy it out before either */
    int64_t  size;
    int64_t* contig_off;    /* [n_contigs + 1]: contig i is data[contig_off[i] .. contig_off[i + 1]) */
    int64_t  n_fallback;    /* lines the caller renders itself and splices in (device text in their place is a best guess) */
    int64_t* fallback;      /* [3 * n_fallback]: gene index, first byte, end byte of each such line */
} pga_text;
typedef struct pga_render_result {
    int32_t  n_contigs;
    int32_t  _pad;
    pga_text text[5];       /* GFF, protein FASTA, gene FASTA, GenBank, start scores (PGA_RENDER_* bit order); data == NULL for a
                             * format that was not asked for */
    double   t_kernels_ms[5];  /* device time of each format's length pass, scan and write pass (scores: and the row sort) */
} pga_render_result;
/*   contigs[i]          the result's contig records of THIS batch (gene_begin / n_genes; genes of contig i in order)
 *   genes               the result's gene records
 *   model_of_contig[i]  the loaded model (pga_set_models index) that called contig i: 0 in single mode, contigs[i].model in
 *                       meta mode, the caller's index on the model-per-contig path; -1 only for a contig without genes
 *                       (and then not with PGA_RENDER_GFF or PGA_RENDER_SCO: their headers need a model -- Prodigal reports
 *                       bin 5 for it)
 *   ids / id_off        sequence ids: contig i is ids[id_off[i] .. id_off[i + 1]) */
int  pga_render_genes(pga_ctx*, const pga_batch*, const pga_contig_result* contigs, int64_t n_genes, const pga_gene* genes,
                      const int32_t* model_of_contig, const char* ids, const int64_t* id_off, const pga_render_opts* opts,
                      pga_render_result** out);
void pga_render_free(pga_render_result*);
/* The records of a batch need not be consecutive records of their file (contig sets are packed into device calls set by set):
 * while seqnum (n entries) is attached to the context, pga_render_genes on a batch of n contigs prints seqnum[i] for contig i in
 * place of opts->first_seqnum + i.  NULL detaches it. */
int  pga_render_seqnums(pga_ctx*, int32_t n, const int64_t* seqnum /* n entries, or NULL */);

/* ---- training --------------------------------------------------------------- */
/* Single-genome training (ref: lib.pyx:5236-5279 `GeneFinder._train`): `batch` holds exactly ONE sequence (several
 * training sequences are joined by the caller with the reference's TTAATTAATTAA spacer, lib.pyx:5510-5532); closed,
 * min_gene, min_edge_gene, max_overlap and mask come from `params`.  On success `*out` is the complete TrainingInfo.
 * `upto` = 0 trains completely; 1 / 2 / 3 stop after the GC frame bias / the hexamer statistics / the Shine-Dalgarno
 * start training (partial structs, for validation). */
int pga_train(pga_ctx*, const pga_batch*, const pga_params*, int translation_table, double start_weight, int force_nonsd,
              int upto, pga_training* out);
/* Many genomes at once: sequence g of the batch is genome g (its contigs already joined with TTAATTAATTAA by the caller), trained
 * with translation_table[g], start_weight[g], force_nonsd[g]; closed / min_gene / min_edge_gene / max_overlap / mask from params.
 * out[g] is byte-identical to pga_train of that genome alone; status[g] is PGA_OK or the code pga_train would return (PGA_EINVAL: no
 * node).  `upto` as in pga_train.  One device pass per stage or training round for all genomes; at most 4 distinct tables per call
 * (PGA_EINVAL).  The context's loaded model set is left as it was. */
int pga_train_batch(pga_ctx*, const pga_batch*, const pga_params*, const int32_t* translation_table, const double* start_weight,
                    const int32_t* force_nonsd, int upto, pga_training* out, int32_t* status);

/* ---- FASTA ingest (host side) ---------------------------------------------- */
/* Multi-record FASTA, plain or gzip, read in batches ready for pga_find_genes_batch / pga_batch_create
 * (ref: src/pyrodigal/tests/fasta.py:59-86 `parse`, src/pyrodigal/cli.py:32-61).  headers[i] is the header line
 * without '>' (id = first word, description = the rest); seqs[i] holds lens[i] letters with every blank
 * removed, not NUL-terminated.  The arrays are valid until the next call on the same reader; a batch ends
 * after max_records records or once max_bases bases are exceeded (0 = no limit); *n_records == 0 at end of file. */
typedef struct pga_fasta pga_fasta;
/* plain files are mapped and parsed by several threads; gzip files are inflated with zlib on one thread; a file in another
 * compression format is rejected (PGA_EINVAL): decompress it into pga_fasta_open_callback.  A mapped file must not be truncated by
 * another process while it is read: the kernel answers a read behind the new end with SIGBUS, which no return code can stand for
 * (feed files that may shrink through pga_fasta_open_callback and read() instead). */
int         pga_fasta_open(const char* path, pga_fasta** out);
/* The same reader over a byte stream the caller produces: read(user, buf, cap) fills up to cap bytes and returns their number,
 * 0 at the end of the stream, negative on failure (ref: tests/fasta.py:16-57 `zopen` -- the reference sniffs bz2 / xz / lz4 / zstd
 * and decompresses with Python modules; the Python layer here hands those decompressors in through this entry point). */
typedef int64_t (*pga_fasta_read_fn)(void* user, char* buf, int64_t cap);
int         pga_fasta_open_callback(pga_fasta_read_fn read, void* user, pga_fasta** out);
int         pga_fasta_next(pga_fasta*, int64_t max_bases, int32_t max_records, int32_t* n_records,
                           const char* const** headers, const char* const** seqs, const int64_t** lens);
const char* pga_fasta_error(const pga_fasta*);
void        pga_fasta_close(pga_fasta*);
/* The pinned staging arenas of closed readers wait in a process-wide pool for the next reader (at most eight arenas and 512 MB,
 * allocated hipHostMallocPortable, so a reader on any device can take them); this gives them back to the system. */
void        pga_fasta_release_spare(void);
/* Device and pinned buffers of destroyed contexts wait in a process-wide cache for the next context (at most PGA_CACHE_GB, default
 * 16 GB, of device memory and 2 GB of pinned memory; 0 turns the cache off); this gives them back to the system. */
void        pga_release_cached(void);
/* The same records with their sequences packed back to back in PINNED host memory (hipHostMalloc): `*packed` holds the
 * letters of the batch, record i at offs[i], lens[i] long, offs[i + 1] == offs[i] + lens[i].  The reader owns `n_arenas`
 * staging arenas (2 .. 8, fixed at the first call) and fills them in turn: the LETTERS of a call (`*packed`) stay valid until
 * that arena comes up again, i.e. for the next n_arenas - 1 calls -- batch k can be on its way to the device
 * (pga_batch_create_packed) while batch k + 1 is being parsed (ref: the reader the reference's CLI feeds its thread pool
 * with, cli.py:287-302).  `headers`, `offs` and `lens` belong to the reader and are only valid until the NEXT call: copy them
 * (or hand them to pga_batch_create_packed, which copies) before asking for the next batch. */
int         pga_fasta_next_packed(pga_fasta*, int64_t max_bases, int32_t max_records, int32_t n_arenas, int32_t* n_records,
                                  const char* const** headers, const char** packed, const int64_t** offs, const int64_t** lens);

/* ---- test support ----
 * Makes memory that an earlier call left behind visible to a test: a call's result depends on its arguments only, so nothing a
 * call reads may come from a buffer that this call did not write.  Waits for the context's streams, then fills the whole capacity
 * (slack included) of every workspace buffer of the context whose elements are floating point, device and pinned, with `byte`
 * (0 .. 255); while it is on, every block such a buffer newly acquires -- from the runtime or from the cache of destroyed contexts --
 * gets the same fill before it is used, so do the floating-point buffers of pga_score_connections*, and the letters' allocation of
 * a batch is filled with 'N'.  Buffers of integers are left alone: a pattern read as an index would be a wild address.  byte = -1
 * switches it off (the state of a new context).  out (optional): buffers and bytes filled by this call.  0xFF is NaN in both
 * widths, 0x7F a huge positive and 0xFE a huge negative number.  Not for production use: every fill synchronises the device. */
int         pga_debug_poison(pga_ctx*, int byte, int64_t out[2]);

#ifdef __cplusplus
}
#endif
#endif
