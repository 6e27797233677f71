// Device-side data layout of the finder pipeline (see DESIGN.md "Data layout in HBM").
#pragma once
#include "pga_internal.h"

// One 3072-position tile of one contig (forward coordinates; every position of a contig of three bases or more lies in one) for the extraction kernels.
#define PGA_STAGE_SLACK 8     // extra staging slots of every tile under GroupArrays::st_half
struct TileDesc {
    int32_t contig;
    int32_t start;
};

// Per translation-table group: per-position scratch of the extraction and the node topology
// (fields that do not depend on the model), indexed by global node number.
struct GroupArrays {
    // per position (whole batch)
    uint8_t* df;                             // the digit of the position (bits 0-2) | 16 = a forward node has its ndx here | 32 = a reverse node has
                                             // (written densely by the tile that owns the position): all an ORF walk reads of a position is one byte
    // the index of a position's first node (the forward one when both strands have one there: the reverse node then is the next, ref:
    // lib.pyx:2489-2493) is a COUNT: c16[192 tile + g] = index of the first node at or after position 16 g of the tile (k_place_nodes; a
    // contig's tiles are consecutive from tile0[contig], so that is entry position >> 4 of the contig), and the sixteen bytes of df from
    // there on carry the node flags of the positions in between.  (Until the end of round 6 an int32 per POSITION: 500 MB per group and
    // call, written four bytes at a time wherever a node sat -- most of what k_place_nodes moved.)
    int32_t* c16; const int32_t* tile0 = nullptr;
    // staging: the nodes of the tile that starts at global position g, packed in order from slot 2 g (two slots per position: every
    // position can hold a node on either strand) -- or, st_half = s > 0, from slot g >> s with room for one node per 2^s positions
    // of the tile (s = 1 in production: sequence has a node every 25 positions or so, periodic worst cases reach one in two); a
    // tile that does not fit says so in bit 0 of *st_overflow and the caller extracts again with the full staging (bit 1: a tile's
    // pool of stop values ran out, see pga_launch_extract)
    int32_t* st_ndx; int32_t* st_sv;         // ndx, stop_val
    uint8_t* st_info;                        // type | edge << 2 | reverse << 3
    int32_t st_half = 0; int32_t* st_overflow = nullptr;
    int32_t* stop_list;                      // the stop nodes of the group in node order (node indices); contig c owns [sbase[c], sbase[c + 1])
    int32_t* start_list = nullptr;           // the other nodes of the group in node order (k_place_nodes; nullptr: not wanted): the start scorer's work list
    uint32_t* ovl_topo;                      // per entry of stop_list: which of its first 16 neighbours can be overlapping starts (k_ovl_topo)
    int32_t* srank = nullptr;                // per node, written for stop nodes only: its rank among the stop nodes of its contig (k_ovl_topo):
                                             // the k-th stop of a chain owns extras record ChainDesc::soff + k of the wave-batch scorer
    // per node, in (contig, ndx, strand) order
    int32_t* ndx; int32_t* stop_val; uint8_t* type; int8_t* strand; uint8_t* edge0; float* gc_cont;
    int32_t* contig_of = nullptr;            // the node's contig (k_place_nodes): kernels over nodes read it instead of searching the contigs' first nodes
};

// Per (contig, model) chain node fields (SoA over all chains of the batch).
struct ChainArrays {
    double* cscore; double* sscore; double* rscore; double* uscore; double* tscore; double* mot_score;
    double* cscore_raw;    // the coding score as the ORF walk leaves it (k_coding_score); `cscore` is what Nodes._score makes of it
    int32_t* star_ptr;     // [n][3]
    int32_t* mot_ndx;
    uint8_t* rbs;          // [n][2]
    uint8_t* edge;         // edge flag after Nodes._score's conversion
    uint8_t* mot_len; uint8_t* mot_spacer; uint8_t* mot_spacendx;
    double* cs_sink = nullptr;   // as many doubles as the largest contig has nodes: where the ORF walks of k_coding_score_quads store the sums of
                                 // table columns a contig has no model for (unconditional stores instead of a divergent branch per column)
};

// Host-computed per-model constants of the node scorer (libm log/pow stay on the host).
struct ModelScoreConst {
    double lfac_min, lfac_max;          // ref: lib.pyx:2146-2147
    double lfac_tab[1001];              // log((1-p^n)/p^n) - lfac_min for n = 0..1000 codons (ref: lib.pyx:2209-2210)
};

// Masked regions (ref: lib.pyx:699-713): per contig a sorted run of [begin, end) intervals.
struct MaskList {
    const int32_t* off;     // [n_contigs + 1] into iv, or nullptr when masking is off
    const int2* iv;         // begin, end (contig coordinates)
};
struct MaskRun { int32_t contig, begin, end, _pad; };

struct ScoreParams {
    int32_t closed, is_meta, max_overlap, n_models;       // n_models: entries of the model array the chains index
    double* cs_out;          // or nullptr: cscore + sscore of every node, indexed like the chain arrays (what the wave-batch connection scorer reads)
    uint8_t* conv_flag;      // per contig (of the group being scored), or nullptr: set when the contig holds a start node that the
                             // reference turns into an edge node while scoring (lib.pyx:2424-2434) -- only such contigs are scored
                             // differently by the first and by a later model of a run
    unsigned long long* prof = nullptr;   // PGA_SS_PROFILE=1: wave-cycles per phase of k_score_starts / k_score_starts_mm (16 slots), or nullptr
    int32_t models_per_pass = 512;        // k_score_starts walks a workgroup's models in sets of this many (<= 512; PGA_SS_MODELS_PER_PASS: tests)
    int32_t lean_stops = 0;               // 1: of a stop node's per-chain fields only `edge` is written (round 6).  A stop node carries no start
                                          // scores (reset_node_scores: zeros); the wave-batch connection scorer, the overlapping-start search and the
                                          // device tail read a stop node's `edge` and nothing else of them, so the path proper -- no node arrays asked
                                          // for -- leaves the other twelve fields unwritten: 66 bytes per (stop node, model) pair, 0.6 GB per 125 Mbp call
};

void pga_launch_digitize(const char* d_seq, uint8_t* d_dig, int64_t total, const ContigDesc* d_ct, int n_contigs,
                         int32_t* d_gc, int32_t* d_unk, hipStream_t st);
// GC-or-unknown bases before every 16th position of the batch (d_p16: total / 16 + 2 entries); scratch of pga_gc_blocks(total) + 1 entries each
int64_t pga_gc_blocks(int64_t total);
void pga_launch_gc_prefix(const uint8_t* d_dig, int64_t total, int32_t* d_block_sum, int32_t* d_block_off, int32_t* d_p16, hipStream_t st);
// nodes of one translation-table group: staged per tile, counted (d_tile_count[n_tiles], d_tile_off[n_tiles + 1]), first node of
// every contig in d_cbase[n_contigs + 1]; d_tile0[c] = first tile of contig c (n_contigs + 1 entries).  pga_launch_place moves the
// staged nodes to ga.ndx .. ga.edge0 once those are allocated.
void pga_launch_extract(const uint8_t* d_dig, int64_t total, const ContigDesc* d_ct, int n_contigs, int tt,
                        const pga_params& p, const GroupArrays& ga, const TileDesc* d_tiles, int n_tiles, const int32_t* d_tile0,
                        int32_t* d_tile_first, int32_t* d_tile_last, int32_t* d_tile_count, int32_t* d_tile_off, int32_t* d_cbase,
                        int32_t* d_tile_scount, int32_t* d_tile_soff, int32_t* d_sbase /* the same three for stop nodes only */,
                        MaskList masks, hipStream_t st,
                        const uint8_t* d_enabled = nullptr /* per contig: extract it in this group?  nullptr = every contig */,
                        int ex_c = 4 /* stop values a thread lists per strand, 1 .. 4; 0: a value for every position (k_extract_tile<false>) */,
                        int ex_pool = 128 /* entries of the workgroup's pool for what the lists do not hold, 0 .. 128; a tile that needs
                                             more raises bit 1 of *ga.st_overflow (bit 0: the half-density staging did not fit) */);
void pga_launch_place(const ContigDesc* d_ct, const TileDesc* d_tiles, int n_tiles, const int32_t* d_tile_off, const int32_t* d_tile_soff,
                      const GroupArrays& ga, hipStream_t st);
// (chain, start) items of the model-major start scoring: tiles of `tile` (Knobs::ss_mm_tile) items of one model each
int32_t pga_mm_tiles(const ChainDesc* h_chains, int n_chains, const int32_t* h_cbase, const int32_t* h_sbase, int n_models, int tile, std::vector<int64_t>& scratch);
size_t pga_mm_scratch_bytes(int n_models, int n_chains);
constexpr size_t PGA_SS_REC_BYTES = 32, PGA_SS_MMCHAIN_BYTES = 32, PGA_SS_MMTILE_BYTES = 16;
// per (group, contig): is any model of the group inside the contig's GC window?  (meta mode)
void pga_launch_group_enable(const ContigDesc* d_ct, int n_contigs, const int32_t* d_gc_count, const double* d_model_gc,
                             const int32_t* d_model_group, int n_models, int n_groups, uint8_t* d_enabled, hipStream_t st);
// the same flags from the GC window of the contig's SET: d_set_of[i] in [0, n_contigs), d_pool: 2 * n_contigs entries of
// scratch that hold every set's pooled G+C count and length afterwards
void pga_launch_group_enable_sets(const ContigDesc* d_ct, int n_contigs, const int32_t* d_gc_count, const int32_t* d_set_of, int32_t* d_pool,
                                  const double* d_model_gc, const int32_t* d_model_group, int n_models, int n_groups, uint8_t* d_enabled,
                                  hipStream_t st);
// runs of unknown bases of at least min_mask positions, unordered, at most `cap` of them; *d_count is reset first
void pga_launch_find_masks(const uint8_t* d_dig, const ContigDesc* d_ct, int n_contigs, const TileDesc* d_tiles, int n_tiles, int min_mask,
                           MaskRun* d_runs, int32_t* d_count, int cap, hipStream_t st);
// The union of the mask sources of a call, built on the device (DESIGN.md "Region masks"): runs of unknown bases (d_dig) and / or of
// lower-case letters (d_seq) of at least min_mask positions, and the caller's intervals (d_regions, any order, overlaps allowed), come
// out as MaskList{d_moff, d_miv}: per contig sorted, disjoint, touching intervals joined, at most `cap` in all.
//   d_bits    2 * pga_mask_words(total) words (cleared here)      d_counts  4 * (pga_mask_waves(total) + 1) ints
int64_t pga_mask_words(int64_t total);
int64_t pga_mask_waves(int64_t total);
void pga_launch_mask_union(const uint8_t* d_dig, const char* d_seq, int64_t total, const ContigDesc* d_ct, int n_contigs, const TileDesc* d_tiles,
                           int n_tiles, int unknown_runs, int lower_case_runs, int min_mask, const MaskRun* d_regions, int n_regions,
                           uint32_t* d_bits, int32_t* d_counts, int32_t* d_moff, int2* d_miv, int cap, hipStream_t st);
int pga_extract_tile_size();
void pga_launch_orf_gc(const ContigDesc* d_ct, int n_contigs, const uint8_t* d_dig, const int32_t* d_p16, const GroupArrays& ga,
                       int n_nodes_total, const int32_t* d_node_contig_base, hipStream_t st);
// ---- node scoring of one translation-table group: three launchers, every choice of form made by the caller (FindCall::score_groups,
//      rescore_winners in finder.hip; DESIGN.md "Run-time knobs").  Each takes the group's chains plus what only it reads.
struct ScoreGroup {
    const ChainDesc* d_chains = nullptr; int n_chains = 0; int64_t node_begin = 0, total = 0;      // the chains of the launch, contiguous in `off` from node_begin, and their nodes
    const ChainDesc* d_all_chains = nullptr; const int2* d_contig_chains = nullptr;                // per contig of the group: first chain (an index into d_all_chains), count
    const int32_t* d_node_contig_base = nullptr; int n_contigs = 0; int group_nodes = 0;
    const uint8_t* d_dig = nullptr; const ContigDesc* d_ct = nullptr; const GroupArrays* ga = nullptr; const ChainArrays* ca = nullptr;
    const pga_training* d_models = nullptr; hipStream_t st = nullptr;
};
// (the argument structs are built from the group and filled by name: a field that moves cannot change what a caller passes)
struct CodingScoreLaunch : ScoreGroup {
    explicit CodingScoreLaunch(const ScoreGroup& g) : ScoreGroup(g) {}
    // lds_tasks: ORF walks from hexamer tables in LDS (k_coding_score_quads over the tasks of pga_cs_tasks); global_memory: k_coding_score
    enum Form { lds_tasks, global_memory } form = global_memory;
    const ModelScoreConst* d_msc = nullptr;
    const double* d_gil = nullptr; int il_stride = 0; const int32_t* d_rank = nullptr;      // hexamer tables of the group's models, interleaved: [4096][il_stride]; model -> column
    const void* d_cs_tasks = nullptr; int n_cs_tasks = 0; const void* d_cs_entries = nullptr;
    int cs_wave = 0, qclasses = 0; bool profile = false;                                    // Knobs::cs_wave, cs_qclasses, cs_profile
};
struct StartScoreLaunch : ScoreGroup {
    explicit StartScoreLaunch(const ScoreGroup& g) : ScoreGroup(g) {}
    // model_major: a per-start prologue and a model-major pass over (chain, start) items (k_start_prologue, k_mm_*, k_score_starts_mm,
    // k_clear_stops); listed_loop: the model loop of k_score_starts over ga->start_list (its workgroups clear the fields of the stop nodes
    // between their start nodes at the end); all_nodes: the same kernel with a thread per node
    enum Form { model_major, listed_loop, all_nodes } form = all_nodes;
    ScoreParams sp{}; const unsigned* d_sd_lut = nullptr;
    int32_t n_starts = 0, n_stops = 0; const int32_t* sbase = nullptr;      // entries of ga->start_list / ga->stop_list; per contig: first entry of ga->stop_list (n_contigs + 1)
    // model_major: the context's buffers, sized by the caller
    void* mm_rec = nullptr;                      // SsStartRec per start node of the group (n_starts)
    void* mm_chain = nullptr;                    // SsMmChain per chain of the launch (n_chains)
    void* mm_tile = nullptr;                     // SsMmTile per tile (mm_tiles)
    void* mm_scratch = nullptr;                  // pga_mm_scratch_bytes(n_models, n_chains)
    int32_t mm_tiles = 0; int mm_tile_items = 0; // pga_mm_tiles(.., mm_tile_items, ..): the one value sizes the tiles and launches them
    bool profile = false;                        // Knobs::ss_profile
};
struct OverlapLaunch : ScoreGroup {
    explicit OverlapLaunch(const ScoreGroup& g) : ScoreGroup(g) {}
    // stop_pairs: over (chain, stop node) pairs (k_ovl_topo, k_ovl_stops); every_node: k_overlapping_starts (the re-score)
    enum Form { stop_pairs, every_node } form = every_node;
    const ModelConst* d_mc = nullptr; int32_t max_overlap = 0;
    const int32_t* sbase = nullptr; int64_t soff_begin = 0, n_pairs = 0; int32_t n_stops = 0;      // ChainDesc::soff of the launch's first chain; (chain, stop) pairs of its chains
    // the wave-batch scorer's 64-byte extras of every stop node, built in the same pass (ext nullptr: not wanted), from cs_out = cscore + sscore
    const int32_t* topo_q2 = nullptr; void* ext = nullptr; const double* cs_out = nullptr;
    // star_ptr of the nodes that are no stop nodes is -1: the launcher fills the chains' range first -- unless nobody will read it
    // (the wave-batch scorer takes the extras, the tail asks for stop nodes only, the caller does not want the node arrays)
    bool fill_star_ptr = true;
    // per workgroup of k_ovl_stops (256 pairs from soff_begin on): the chain of its first pair, relative to the launch's first chain
    // (the caller's plan; nullptr, Knobs::ovl_search: the workgroup searches)
    const int32_t* blk_chain = nullptr;
};
void pga_launch_coding_score(const CodingScoreLaunch& a);
// false, and nothing launched: the form the caller chose lacks its list or its buffers
bool pga_launch_start_scores(const StartScoreLaunch& a);
void pga_launch_overlapping_starts(const OverlapLaunch& a);
// host: the tasks of the LDS form of the coding score for one group (pipeline.hip); false = models are not neighbours in the table
bool pga_cs_tasks(const int2* h_cc, int n_contigs, const ChainDesc* h_chains, const int32_t* h_cbase, const int32_t* model_rank, int task_nodes,
                  std::vector<int32_t>& tasks, std::vector<int32_t>& entries);
// the RBS search tabulated: 1920 words, filled once per context (see sd_hits in pipeline.hip)
void pga_launch_sd_lut(unsigned* d_lut, hipStream_t st);
