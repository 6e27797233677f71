// The run-time knobs: every PGA_* environment variable the library honours, parsed here and nowhere else.  No HIP header:
// tests/knobs_shim.cpp builds this file with a host compiler.  The table of INTEGRATION.md ("Run-time knobs and diagnostics") is a
// rendering of the comments below.
//
// When a knob is read (DESIGN.md "Run-time knobs"): a public entry point calls read_knobs() once, at its entry, and hands the values
// down by value or const reference -- a knob is read once per call, whatever the number of phases that honour it.  The fields marked
// "once per process" are taken from process_knobs() instead, which reads the environment the first time anybody asks -- in practice
// in the first pga_create, which asks for `mallopt`: all five are the environment as it was then; the field
// marked "at destruction" is read when a context is destroyed.  Nothing here is mutable after it was read.
//
// The parse rules are the ones each knob has always had, odd ones included; they are not meant to be uniform.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

namespace pga_knobs {

// ---- the parse helpers ------------------------------------------------------------------------------------------------
inline bool present(const char* name) { return getenv(name) != nullptr; }                       // set, to anything (the empty string too)
inline bool is_zero(const char* name) { const char* e = getenv(name); return e && atoi(e) == 0; }   // set to 0 -- or to anything atoi reads as 0
// atoi of the value, or `dflt` when unset (nonempty: also when set to the empty string -- the knobs of the segment plan)
inline int int_or(const char* name, const int dflt, const bool nonempty = false) {
    const char* e = getenv(name);
    return e && (!nonempty || *e) ? atoi(e) : dflt;
}
inline int in_range_or(const int v, const int lo, const int hi, const int dflt) { return v >= lo && v <= hi ? v : dflt; }   // out of range: the default, not the nearest end

struct Knobs {
    enum Tail { par, device, host };
    enum DpKernel { by_shape, wave, tree1, tree3, scan, other };

    // ---- the call as a whole
    bool timing;                // PGA_TIMING              unset | set: stage times of the call on stderr, one line per call
    bool fault_contig_len_set;  // PGA_FAULT_CONTIG_LEN    unset | a length (atol): a finder call that carries a contig of exactly this many bases fails
    long fault_contig_len;      //                         (tests of the host layer's error paths)
    bool pageable_results;      // PGA_PAGEABLE_RESULTS    unset | set: gene records of a large result go to pageable memory, not to a pinned block
    // ---- once per process / at destruction
    int cache_gb;               // PGA_CACHE_GB            16 | >= 0 (negative: 0): GB of device memory (pinned: at most 2 GB of it) that buffers of
                                //                         destroyed contexts may hold for the next context; 0: no cache.  Once per process.
    bool upload_turns;          // PGA_UPLOAD_TURNS        1 | 0: the contexts of a process upload their batches all at once, not in turn.  Once per process.
    bool mallopt;               // PGA_MALLOPT             1 | 0: glibc's mmap and trim thresholds are left alone.  Once per process (first pga_create).
    int dp_seg_height;          // PGA_DP_SEG_HEIGHT       4 | 2 .. 24 (else 4): segmented path: height from which a node of the claimed traceb forest
                                //                         belongs to the serially walked spine.  Once per process.
    int dpw_occ;                // PGA_DPW_OCC             6 | 4 .. 6 (else 6): wavefronts per SIMD the wave-batch connection scorer is compiled for.  Once per process.
    bool print_buffers;         // PGA_PRINT_BUFFERS       unset | set: a context lists its device buffers by size on stderr.  At destruction.
    // ---- FASTA reader (read when a file is opened)
    bool fasta_no_mmap;         // PGA_FASTA_NO_MMAP       unset | set: plain files go through the line-by-line stream reader
    int fasta_threads;          // PGA_FASTA_THREADS       0 = cores / 4, at most 16 | a count (below 1: 1): threads of the mapped reader
    // ---- extraction
    bool stage_full;            // PGA_STAGE_FULL          unset | set: two staging slots per position from the start; the context keeps that (sticky)
    bool stage_shift_set;       // PGA_STAGE_SHIFT         1 | 1 .. 8 (clamped): one staging slot per 2^shift positions (5: ordinary sequence overflows --
    int stage_shift;            //                         tests of the second pass).  While it is set, an overflow leaves the context as it was.
    int extract_c;              // PGA_EXTRACT_C           4 | 0 .. 4 (clamped): stop values a thread of k_extract_tile lists per strand; 0: a value per position
    int extract_pool;           // PGA_EXTRACT_POOL        128 | 0 .. 128 (clamped): entries of the workgroup's pool for what the lists do not hold
    // ---- coding score
    bool cs_lds;                // PGA_CS_LDS              1 | 0: per-lane table gathers (k_coding_score) instead of the LDS-table kernel
    int cs_task_nodes;          // PGA_CS_TASK_NODES       5120 | 256 .. 8192 (else 5120): nodes per task of the LDS-table kernel
    int cs_wave;                // PGA_CS_WAVE             2048 | >= 64 (else 2048): ORFs longer than this many codons take a whole wavefront
    int cs_qclasses;            // PGA_CS_QCLASSES         3 | 4 (anything else: 3): ORFs of 193 .. 256 codons walk four to a wavefront as well
    bool cs_profile;            // PGA_CS_PROFILE          unset | set: wave-cycles per phase of k_coding_score_quads on stderr (synchronises)
    // ---- start scores, overlapping starts
    bool ss_starts_only;        // PGA_SS_STARTS_ONLY      1 | 0: the start scorer of the path proper keeps a thread per node, not per listed start node
    bool ss_mm;                 // PGA_SS_MM               1 | 0: the listed start scoring runs the model loop of k_score_starts, not the model-major pass
    int ss_mm_tile;             // PGA_SS_MM_TILE          1024 | 256, 512, 1024 (else 1024): (chain, start) items per workgroup of k_score_starts_mm
    int ss_models_per_pass;     // PGA_SS_MODELS_PER_PASS  512 | 1 .. 512 (else 512): models a workgroup of k_score_starts walks per pass (tests)
    bool ss_full_stops;         // PGA_SS_FULL_STOPS       unset | set: every per-chain field of a stop node is written also where nobody reads them
    bool ss_profile;            // PGA_SS_PROFILE          unset | set: wave-cycles per phase of the start scorer on stderr, one line per launch (synchronises)
    bool ovl_search;            // PGA_OVL_SEARCH          unset | set: a workgroup of k_ovl_stops searches the chain of its first pair instead of reading the plan
    // ---- connection scoring: which kernel
    bool dp_kernel_set;         // PGA_DP_KERNEL           by launch shape | wave, tree1, tree3, scan.  Odd, and kept: set to ANYTHING (the empty string
    DpKernel dp_kernel;         //                         too) turns the segmented path off; a word that is none of the four (`other`) also keeps the
                                //                         wave-batch kernel from many-chain launches; the empty string does not.
    int dp_waves;               // PGA_DP_WAVES            0 = by launch shape | 1, 4, 16 (else by shape): wavefronts per chain of the `scan` kernels
    bool dp_profile;            // PGA_DP_PROFILE          unset | set: cycles per phase of the connection-scoring kernel on stderr (synchronises)
    // ---- connection scoring: the segmented path (an empty string counts as unset for SEG, SEG_MIN, SEG_WARM, SEG_LEN, SEG_SLOTS, SEG_WSLOTS)
    bool dp_seg;                // PGA_DP_SEG              1 | 0: always the serial walk
    int dp_seg_min;             // PGA_DP_SEG_MIN          16384 | >= 256 (below: 256): shortest chain (nodes) that is cut
    int dp_seg_warm;            // PGA_DP_SEG_WARM         4096 | >= 64 (below: 64): nodes walked ahead of a segment from the empty state
    bool dp_seg_len_set;        // PGA_DP_SEG_LEN          by the slots below | > 0: segment length in nodes (rounded up to 64)
    int dp_seg_len;
    int dp_seg_slots;           // PGA_DP_SEG_SLOTS        256 | a count: workgroups of the chain kernel at once; four are held back and at least 64 stay (default 252)
    int dp_seg_wslots;          // PGA_DP_SEG_WSLOTS       4096 | >= 64 (below: 64): segments at once when the wave-batch kernel walks them
    bool dp_seg_wave_set;       // PGA_DP_SEG_WAVE         by size | 1 / 0: the wave-batch kernel always / never walks the segments (tests)
    bool dp_seg_wave;
    int64_t dp_seg_wave_min;    // PGA_DP_SEG_WAVE_MIN     2500000 | nodes (atoll) in chains of PGA_DP_SEG_MIN or more from which it does
    bool dp_seg_readback;       // PGA_DP_SEG_READBACK     1 | 0: the verification rounds behind the first are gated launches, not issued after a read-back
    bool dp_seg_debug;          // PGA_DP_SEG_DEBUG        unset | set: segments / rejected nodes / spine sizes of the call on stderr
    // ---- connection scoring: the wave-batch scorer
    bool dp_no_order;           // PGA_DP_NO_ORDER         unset | set: chains start in launch order, not longest first
    bool dp_xcd;                // PGA_DP_XCD              1 | 0: the start order is not made XCD-aware
    bool dpw_sched;             // PGA_DPW_SCHED           1 | 0: every launch by k_dpw_dyn, which works the lane masks out itself (cross-check)
    bool dpw_sched_miss;        // PGA_DPW_SCHED_MISS      unset | non-zero: every batch reports that its lists did not fit (tests of the fallback)
    bool dpw_sched_debug;       // PGA_DPW_SCHED_DEBUG     unset | set: batches missed per group on stderr
    bool dpw_topo_walk;         // PGA_DPW_TOPO_WALK       unset | non-zero: the topology pass finds a forward stop's successors by walking the nodes (cross-check)
    bool dpw_topo_lds;          // PGA_DPW_TOPO_LDS        1 | 0: the per-node topology kernel on global memory also where the contigs fit the LDS form
    // ---- winners and tail
    Tail tail;                  // PGA_TAIL                par | host, device (any other word: par): the host-thread tail / one device thread per contig
    bool full_gather;           // PGA_FULL_GATHER         unset | set: the winners' final-pass node fields are gathered even when nobody asked for node arrays
    bool gather_all_dp;         // PGA_GATHER_ALL_DP       unset | set: the tail works on gathered copies of all the DP pass's fields (cross-check)
    bool tp_steps;              // PGA_TP_STEPS            unset | set: the many-launch traceback tail also for short chains (cross-check)
    bool tp_jump8;              // PGA_TP_JUMP8            1 | 0: pointer jumping by doubling only, not eight hops per launch
    bool tp_extract_one;        // PGA_TP_EXTRACT_ONE      unset | set: genomes take one workgroup per contig (k_tp_extract), not the chunked pair
    bool tweak_slots;           // PGA_TWEAK_SLOTS         unset | set: many-contig batches take k_tail_tweak over slots, not the packed kernel
    // ---- device-tensor calls
    int kmer_direct;            // PGA_KMER_COUNTS_FORM    by shape | words found anywhere in the value (strstr): `direct` (wins) or `lds`, and
    int kmer_per_wave;          //                         `wave` (wins) or `group`; a pair such as lds-wave sets both.  Fields: -1 by shape, 0, 1.
    int protein_groups_key_bits;    // PGA_PROTEIN_GROUPS_KEY_BITS  61 | 1 .. 61 (strtol, the whole string): the grouping sorts on the low k bits; anything
                                    //                         else (0 in this field) makes pga_group_proteins refuse the call
};

inline Knobs read_knobs() {
    Knobs k{};
    k.timing = present("PGA_TIMING");
    k.fault_contig_len_set = present("PGA_FAULT_CONTIG_LEN");
    k.fault_contig_len = k.fault_contig_len_set ? atol(getenv("PGA_FAULT_CONTIG_LEN")) : 0;
    k.pageable_results = present("PGA_PAGEABLE_RESULTS");
    k.cache_gb = std::max(0, int_or("PGA_CACHE_GB", 16));
    k.upload_turns = !is_zero("PGA_UPLOAD_TURNS");
    k.mallopt = !is_zero("PGA_MALLOPT");
    k.dp_seg_height = in_range_or(int_or("PGA_DP_SEG_HEIGHT", 4), 2, 24, 4);
    k.dpw_occ = in_range_or(int_or("PGA_DPW_OCC", 6), 4, 6, 6);
    k.print_buffers = present("PGA_PRINT_BUFFERS");
    k.fasta_no_mmap = present("PGA_FASTA_NO_MMAP");
    k.fasta_threads = present("PGA_FASTA_THREADS") ? std::max(1, int_or("PGA_FASTA_THREADS", 1)) : 0;
    k.stage_full = present("PGA_STAGE_FULL");
    k.stage_shift_set = present("PGA_STAGE_SHIFT");
    k.stage_shift = std::max(1, std::min(8, int_or("PGA_STAGE_SHIFT", 1)));
    k.extract_c = std::max(0, std::min(4, int_or("PGA_EXTRACT_C", 4)));
    k.extract_pool = std::max(0, std::min(128, int_or("PGA_EXTRACT_POOL", 128)));
    k.cs_lds = !is_zero("PGA_CS_LDS");
    k.cs_task_nodes = in_range_or(int_or("PGA_CS_TASK_NODES", 5120), 256, 8192, 5120);
    k.cs_wave = int_or("PGA_CS_WAVE", 2048) >= 64 ? int_or("PGA_CS_WAVE", 2048) : 2048;
    k.cs_qclasses = int_or("PGA_CS_QCLASSES", 3) == 4 ? 4 : 3;
    k.cs_profile = present("PGA_CS_PROFILE");
    k.ss_starts_only = !is_zero("PGA_SS_STARTS_ONLY");
    k.ss_mm = !is_zero("PGA_SS_MM");
    { const int v = int_or("PGA_SS_MM_TILE", 0); k.ss_mm_tile = v == 256 || v == 512 || v == 1024 ? v : 1024; }
    k.ss_models_per_pass = in_range_or(int_or("PGA_SS_MODELS_PER_PASS", 512), 1, 512, 512);
    k.ss_full_stops = present("PGA_SS_FULL_STOPS");
    k.ss_profile = present("PGA_SS_PROFILE");
    k.ovl_search = present("PGA_OVL_SEARCH");
    {
        const char* e = getenv("PGA_DP_KERNEL");
        k.dp_kernel_set = e != nullptr;
        k.dp_kernel = !e || !*e ? Knobs::by_shape : !strcmp(e, "wave") ? Knobs::wave : !strcmp(e, "tree1") ? Knobs::tree1 : !strcmp(e, "tree3") ? Knobs::tree3 :
                      !strcmp(e, "scan") ? Knobs::scan : Knobs::other;
    }
    { const int v = int_or("PGA_DP_WAVES", 0); k.dp_waves = v == 1 || v == 4 || v == 16 ? v : 0; }
    k.dp_profile = present("PGA_DP_PROFILE");
    k.dp_seg = int_or("PGA_DP_SEG", 1, true) != 0;
    k.dp_seg_min = std::max(256, int_or("PGA_DP_SEG_MIN", 16384, true));
    k.dp_seg_warm = std::max(64, int_or("PGA_DP_SEG_WARM", 4096, true));
    k.dp_seg_len = int_or("PGA_DP_SEG_LEN", 0, true);
    k.dp_seg_len_set = k.dp_seg_len > 0;
    k.dp_seg_slots = std::max(64, int_or("PGA_DP_SEG_SLOTS", 256, true) - 4);
    k.dp_seg_wslots = std::max(64, int_or("PGA_DP_SEG_WSLOTS", 4096, true));
    k.dp_seg_wave_set = present("PGA_DP_SEG_WAVE");
    k.dp_seg_wave = int_or("PGA_DP_SEG_WAVE", 0) != 0;
    { const char* e = getenv("PGA_DP_SEG_WAVE_MIN"); k.dp_seg_wave_min = e ? atoll(e) : 2500000ll; }
    k.dp_seg_readback = !is_zero("PGA_DP_SEG_READBACK");
    k.dp_seg_debug = present("PGA_DP_SEG_DEBUG");
    k.dp_no_order = present("PGA_DP_NO_ORDER");
    k.dp_xcd = !is_zero("PGA_DP_XCD");
    k.dpw_sched = !is_zero("PGA_DPW_SCHED");
    k.dpw_sched_miss = int_or("PGA_DPW_SCHED_MISS", 0) != 0;
    k.dpw_sched_debug = present("PGA_DPW_SCHED_DEBUG");
    k.dpw_topo_walk = int_or("PGA_DPW_TOPO_WALK", 0) != 0;
    k.dpw_topo_lds = !is_zero("PGA_DPW_TOPO_LDS");
    {
        const char* e = getenv("PGA_TAIL");
        k.tail = e && !strcmp(e, "host") ? Knobs::host : e && !strcmp(e, "device") ? Knobs::device : Knobs::par;
    }
    k.full_gather = present("PGA_FULL_GATHER");
    k.gather_all_dp = present("PGA_GATHER_ALL_DP");
    k.tp_steps = present("PGA_TP_STEPS");
    k.tp_jump8 = !is_zero("PGA_TP_JUMP8");
    k.tp_extract_one = present("PGA_TP_EXTRACT_ONE");
    k.tweak_slots = present("PGA_TWEAK_SLOTS");
    k.kmer_direct = k.kmer_per_wave = -1;
    if (const char* e = getenv("PGA_KMER_COUNTS_FORM")) {
        if (strstr(e, "direct")) k.kmer_direct = 1; else if (strstr(e, "lds")) k.kmer_direct = 0;
        if (strstr(e, "wave")) k.kmer_per_wave = 1; else if (strstr(e, "group")) k.kmer_per_wave = 0;
    }
    k.protein_groups_key_bits = 61;
    if (const char* e = getenv("PGA_PROTEIN_GROUPS_KEY_BITS")) {
        char* end = nullptr;
        const long v = strtol(e, &end, 10);
        k.protein_groups_key_bits = end == e || *end || v < 1 || v > 61 ? 0 : (int)v;
    }
    return k;
}

// the once-per-process fields (cache_gb, upload_turns, mallopt, dp_seg_height, dpw_occ) are read from here and only from here
inline const Knobs& process_knobs() {
    static const Knobs k = read_knobs();
    return k;
}

}  // namespace pga_knobs
using pga_knobs::Knobs;
using pga_knobs::read_knobs;
