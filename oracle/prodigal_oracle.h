/*
 * prodigal_oracle.h -- CPU restatement of the pyrodigal / Prodigal gene-finding
 * path.  TEST INFRASTRUCTURE ONLY.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library; the product (pyrodigal_amd/, include/) never links,
 * imports or calls it.
 *
 * Every function cites the reference location it restates (paths relative to
 * /root/reference).  The vendored Prodigal C sources are absent from the
 * reference checkout (vendor/Prodigal is an un-vendored submodule pinned at
 * hyattpd/Prodigal v2.6.3+c1e2d36), so helpers that live only there
 * (eliminate_bad_genes, reset_node_scores, compare_nodes, record_gc_bias,
 * determine_sd_usage, build_coverage_map) restate the published v2.6.3
 * algorithm and are pinned through the reference's own golden fixtures
 * (tests/golden/, see tests/test_oracle_golden.py).
 */
#ifndef PRODIGAL_ORACLE_H
#define PRODIGAL_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* src/pyrodigal/prodigal/training.pxd:3-14 -- byte layout of the reference's
 * `struct _training` (558 392 bytes), so its TrainingInfo dumps load as-is. */
typedef struct po_training {
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
} po_training;

/* Same information as src/Prodigal/node.h:40-76 (own field order). */
typedef struct po_node {
    double  cscore, uscore, tscore, rscore, sscore, score;
    double  gc_score[3];
    double  mot_score;
    float   gc_cont;
    int32_t star_ptr[3];
    int32_t traceb, tracef, ndx, stop_val;
    int32_t mot_ndx;
    int8_t  ov_mark, strand;
    uint8_t rbs[2];
    uint8_t edge, elim, gc_bias, type;
    uint8_t mot_len, mot_spacer, mot_spacendx, _pad;
} po_node;

/* src/pyrodigal/lib.pxd:274-278 */
typedef struct po_gene {
    int32_t begin, end, start_ndx, stop_ndx;
} po_gene;

typedef struct po_params {
    int32_t closed;
    int32_t min_gene;
    int32_t min_edge_gene;
    int32_t max_overlap;
} po_params;

typedef struct po_ctx po_ctx;

po_ctx*  po_new(const char* ascii, int64_t len, int mask, int mask_size);
int      po_masks(const po_ctx* c, int32_t* out, int cap);
void     po_free(po_ctx*);

int      po_slen(const po_ctx*);
double   po_gc(const po_ctx*);
int      po_unknown(const po_ctx*);
const uint8_t* po_digits(const po_ctx*);

int      po_node_size(void);
int      po_num_nodes(const po_ctx*);
po_node* po_nodes(po_ctx*);
int      po_num_genes(const po_ctx*);
po_gene* po_genes(po_ctx*);

/* individual stages (mirror Nodes.extract/sort/score, ConnectionScorer...) */
int  po_extract(po_ctx*, int tt, const po_params*);
void po_sort(po_ctx*);
void po_reset_scores(po_ctx*);
void po_score_nodes(po_ctx*, const po_training*, int closed, int is_meta);
void po_overlapping_starts(po_ctx*, const po_training*, int flag, int max_overlap);
int  po_dprog(po_ctx*, const po_training*, int final, int use_filter);
void po_record_gc_bias(po_ctx*, po_training*);   /* training: GC frame plot + frame bias of every start */
void po_dprog_raw(po_ctx*, const po_training*, int final);   /* connection loop only, no fix-ups */
int  po_find_max_index(po_ctx*);
void po_eliminate_bad_genes(po_ctx*, int ipath, const po_training*);
int  po_extract_genes(po_ctx*, int ipath);
void po_tweak_final_starts(po_ctx*, const po_training*, int max_overlap);

/* whole-path drivers (GeneFinder._find_genes_single/_meta/_train) */
int  po_find_genes_single(po_ctx*, const po_training*, const po_params*);
int  po_find_genes_meta(po_ctx*, const po_training* const* bins, int nbins, const po_params*);
/* the same for n sequences on a pool of threads sharing the models (bench.py's all-core CPU baseline); returns the genes found */
int64_t po_find_genes_meta_pool(const char* const* seqs, const int64_t* lens, int n, const po_training* const* bins, int nbins,
                                const po_params* p, int threads);
int  po_train(po_ctx*, po_training* out, const po_params*, int force_nonsd,
              double start_weight, int tt);
int  po_train_upto(po_ctx*, po_training* out, const po_params*, int force_nonsd,
              double start_weight, int tt, int upto);

/* How often the tie rules of the connection scoring decided something in the last calls on this context (counters only: no result
 * depends on them).  With `v` the value a candidate connection offers (source score + connection score):
 *   TIES          v == the target's score and the target already had a connection: `>=` lets the later source replace it
 *                 (ref: _connection.h:135/197 and their siblings)
 *   ZERO_JOINS    v == the target's score and the target had none: a sum of exactly 0.0 still connects
 *   FRAME_TIES    triple overlap: a frame's value == the best so far while a frame is chosen: strict `>` keeps the earlier frame
 *   BEST_END_TIES po_find_max_index: further gene ends whose score equals the best (ref: lib.pyx:1239-1251, the largest index wins)
 *   OVL_TIES      po_overlapping_starts(flag = 1): a later candidate's value == the best so far (strict `>` keeps the earlier one)
 *   JOINS         connections made or replaced in all
 * TIES, ZERO_JOINS, FRAME_TIES and JOINS are cleared by po_dprog_raw, OVL_TIES by po_overlapping_starts; BEST_END_TIES is set by
 * every po_find_max_index. */
enum { PO_EV_TIES = 0, PO_EV_ZERO_JOINS, PO_EV_FRAME_TIES, PO_EV_BEST_END_TIES, PO_EV_OVL_TIES, PO_EV_JOINS, PO_EV_COUNT };
void   po_dp_events(const po_ctx*, int64_t out[PO_EV_COUNT]);

/* How often each integer comparison of the connection scoring and of po_overlapping_starts was evaluated with lhs - rhs equal to
 * -1, 0 and +1 (out[id][0..2]) in the last calls on this context: which inputs decide a rule AT its threshold.  Counters only.
 *   FS_FB / RB_RS / FS_RS      `left(+2) >= right(-2)` of forward stop -> forward start, reverse start -> reverse stop, forward stop ->
 *                              reverse stop (ref: _connection.h:94-140, 270-367)
 *   FB_FS / RS_RB              `stop_val >= ndx` / `stop_val <= ndx` of the gene connections
 *   FS_FS / RS_RS              the same of the operon rules; *_STAR: [0] star_ptr of the frame was -1, [2] it was not
 *   FS_RB_APART / _OVLP / _HALF / _BND   the four tests of forward stop -> reverse start, in the reference's order
 *   TRI_OVLP0 / _OVLP200 / _N3 / _TRACEB the tests of a frame of the triple overlap; TRI_NO_TRACEB [1]: the source had no traceb;
 *                              TRI_BEST: sign of (candidate - best so far), [0] below, [1] equal, [2] above (strict `>` takes it)
 *   ARTIFACT [1]               a never-reached forward stop or reverse start was refused as a source
 *   IGM_ADJ2 / IGM_ADJ1        `a.ndx + 2 == b.ndx` / `a.ndx == b.ndx + 1`; IGM_FAR `dist > 180`; IGM_OVL `a.ndx + 2 strand >= b.ndx`;
 *                              IGM_OPER `dist <= 60` and IGM_QUARTER `dist < 15` without overlap, *_OVL with it (dist <= 180 only)
 *   OVL_F_* / OVL_R_*          forward / reverse stop of po_overlapping_starts: _SKIP `ndx > s.ndx + 2` (`< s.ndx - 2`) on starts of the
 *                              strand, _MAXOV the break, _STOPVAL `stop_val <= s.ndx` (`>=`); OVL_EDGE_STOP [1]: an edge stop, which
 *                              takes none; OVL_BEST: sign of (candidate - best so far) from the second kept candidate on
 * The entries before PO_EDGE_OVL_FIRST are cleared by po_dprog_raw, the others by po_overlapping_starts (whose igm_same calls count
 * into IGM_* as well: read them after po_dprog_raw for the sum of the two only if no clear lies between). */
enum { PO_EDGE_FS_FB = 0, PO_EDGE_RB_RS, PO_EDGE_FS_RS, PO_EDGE_FB_FS, PO_EDGE_RS_RB, PO_EDGE_FS_FS, PO_EDGE_FS_FS_STAR, PO_EDGE_RS_RS,
       PO_EDGE_RS_RS_STAR, PO_EDGE_FS_RB_APART, PO_EDGE_FS_RB_OVLP, PO_EDGE_FS_RB_HALF, PO_EDGE_FS_RB_BND, PO_EDGE_TRI_OVLP0,
       PO_EDGE_TRI_OVLP200, PO_EDGE_TRI_N3, PO_EDGE_TRI_TRACEB, PO_EDGE_TRI_NO_TRACEB, PO_EDGE_TRI_BEST, PO_EDGE_ARTIFACT,
       PO_EDGE_IGM_ADJ2, PO_EDGE_IGM_ADJ1, PO_EDGE_IGM_FAR, PO_EDGE_IGM_OVL, PO_EDGE_IGM_OPER, PO_EDGE_IGM_OPER_OVL,
       PO_EDGE_IGM_QUARTER, PO_EDGE_IGM_QUARTER_OVL,
       PO_EDGE_OVL_FIRST, PO_EDGE_OVL_F_SKIP = PO_EDGE_OVL_FIRST, PO_EDGE_OVL_F_MAXOV, PO_EDGE_OVL_F_STOPVAL, PO_EDGE_OVL_R_SKIP,
       PO_EDGE_OVL_R_MAXOV, PO_EDGE_OVL_R_STOPVAL, PO_EDGE_OVL_EDGE_STOP, PO_EDGE_OVL_BEST, PO_EDGE_COUNT };
void   po_dp_edges(const po_ctx*, int64_t out[PO_EDGE_COUNT][3]);

/* First candidate source of target i in po_dprog_raw (ref: lib.pyx:1221-1233); *walked: the giant-ORF walk ran, *landed: the node it
 * ended on (0 where no node has the position looked for), else the node 500 back.  -1 for an index out of range. */
int    po_dp_window(const po_ctx*, int i, int* walked, int* landed);

double po_last_path_score(const po_ctx*);  /* nodes[ipath].score of last winning DP */
int    po_last_ipath(const po_ctx*);

#ifdef __cplusplus
}
#endif
#endif
