// Finder-level entry point: whole-batch drop-in for GeneFinder.find_genes() in meta or single
// mode (ref: lib.pyx:5281-5469).  Host orchestration only; every per-base / per-node stage runs in
// the HIP kernels of pipeline.hip and dp.hip.  The tail of the reference's _dynamic_programming
// (traceback untangling), eliminate_bad_genes, Genes._extract and Genes._tweak_final_starts runs on
// the device as well (the kernels of tail.inl over the rules of tail_rules.h); the same rules, compiled
// for the host too, remain as a cross-check (PGA_TAIL=host: one contig per worker thread over the winning
// models' nodes brought home).
#include "pga_internal.h"
#include "pipeline.h"
#include "dpw_core.h"
#include "dev_common.h"
#include "find_plan.h"
#include "tail_rules.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <type_traits>
#include <unordered_map>

namespace {

struct Buf { void* p = nullptr; size_t cap = 0; bool fp = false; /* element type is floating point (pga_debug_poison) */ };

}  // namespace

// Device arrays of the last stage-level run (single contig), kept for the training driver, which continues from them.
struct LastRun {
    const uint8_t* d_dig = nullptr;
    GroupArrays ga{};
    ChainArrays ca{};
    int n_nodes = 0;
    int len = 0;
};
// Host threads that stay around between calls (the per-contig tail work is short: starting threads for it every call
// would cost more than the work).  run(fn, k): fn runs on the caller and on k - 1 pool threads, returns when all are done.
class WorkerPool {
public:
    ~WorkerPool() {
        { std::lock_guard<std::mutex> g(mu_); stop_ = true; gen_++; }
        cv_.notify_all();
        for (auto& t : th_) t.join();
    }
    void run(const std::function<void()>& fn, int k) {
        k = std::max(1, k);
        {
            std::lock_guard<std::mutex> g(mu_);
            while ((int)th_.size() < k - 1) th_.emplace_back([this, id = (int)th_.size()] { loop(id); });
            job_ = &fn; want_ = k - 1; left_ = k - 1; gen_++;
        }
        if (k > 1) cv_.notify_all();
        fn();
        std::unique_lock<std::mutex> g(mu_);
        done_.wait(g, [this] { return left_ == 0; });
        job_ = nullptr;
    }
private:
    void loop(const int id) {
        unsigned long long seen = 0;
        for (;;) {
            const std::function<void()>* job = nullptr;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return gen_ != seen; });
                seen = gen_;
                if (stop_) return;
                if (id < want_) job = job_;
            }
            if (!job) continue;
            (*job)();
            { std::lock_guard<std::mutex> g(mu_); if (--left_ == 0) done_.notify_all(); }
        }
    }
    std::mutex mu_; std::condition_variable cv_, done_;
    std::vector<std::thread> th_;
    const std::function<void()>* job_ = nullptr;
    int want_ = 0, left_ = 0; unsigned long long gen_ = 0; bool stop_ = false;
};

struct FinderState {
    bool stage_full = false;        // a batch of this context did not fit the half-density staging of the extraction: full staging from then on
    LastRun last;
    WorkerPool pool;
    std::map<std::string, Buf> dev, pin;
    std::vector<int> model_group;   // model -> translation-table group
    std::vector<int> group_tt;
    ModelScoreConst* d_msc = nullptr;
    double* d_model_gc = nullptr;   // GC of every loaded model, and its translation-table group: which groups a contig needs
    int32_t* d_model_grp = nullptr;
    // the hexamer tables (gene_dc) of each group's models interleaved: d_gil + gil_off[g], [4096][gil_stride[g]]; d_model_rank[m] = column
    double* d_gil = nullptr; int32_t* d_model_rank = nullptr;
    std::vector<size_t> gil_off; std::vector<int> gil_stride; std::vector<int32_t> model_rank;
    unsigned* d_sd_lut = nullptr;   // RBS search table (pga_launch_sd_lut), filled when the context's finder state is created
    std::mutex spare_mu; void* spare_p = nullptr; size_t spare_cap = 0;   // the letters' allocation of the last batch that was freed
    // Round 6: an upload (pga_batch_create) may run BESIDE a call of the same context -- a caller that keeps the next batch on its way
    // while the current one is being worked on: double buffering of H2D against the kernels.  So the upload has a stream, a pinned
    // staging area and a worker pool of its own and touches nothing else of the context; one upload at a time per context (up_mu).
    std::mutex up_mu; WorkerPool up_pool; hipStream_t up_stream = nullptr; void* up_pin = nullptr; size_t up_pin_cap = 0;
    hipEvent_t up_ev = nullptr;        // pga_batch_create_device: where the producer's stream stood when the call came
    void* up_dev = nullptr; size_t up_dev_cap = 0;   // pga_translate_genes_tokens: the device copy of its tables, kept and grown across calls
    hipEvent_t e_start = nullptr, e_stop = nullptr, e_dp0[4] = {}, e_dp1[4] = {};
    hipEvent_t e_aux[20] = {};      // around the topology / schedule launches of each group (pga_dp_timings), and the first of two connection-scoring launches
};

namespace {

struct StageTimer {
    bool on; std::chrono::steady_clock::time_point t0, tbegin; const char* names[32]; double ms[32]; int n = 0;
    explicit StageTimer(const bool on_) : on(on_), t0(std::chrono::steady_clock::now()), tbegin(t0) {}
    void mark(const char* name) {
        if (!on || n >= 32) return;
        auto t1 = std::chrono::steady_clock::now();
        names[n] = name; ms[n++] = std::chrono::duration<double, std::milli>(t1 - t0).count(); t0 = t1;
    }
    ~StageTimer() {
        if (!on) return;
        fprintf(stderr, "[pga timing]");
        for (int i = 0; i < n; i++) fprintf(stderr, " %s=%.2fms", names[i], ms[i]);
        fprintf(stderr, " | total=%.2fms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tbegin).count());
    }
};

#define HT(ctx, expr) do { int rc__ = pga_hip_try_(ctx, (expr), #expr); if (rc__ != PGA_OK) return rc__; } while (0)

// Buffers of destroyed contexts wait in a process-wide cache for the next context: a caller that makes a context per file pays the
// 120 allocations of a context (50 ms, and as much again to free them) once.  Blocks enter the cache only when their context is
// released, after its stream has drained; the cache is bounded (PGA_CACHE_GB, default 16 GB of device and 2 GB of pinned memory)
// and pga_release_cached() empties it.
struct CachedBlock { void* p; size_t cap; int dev; };
static std::mutex g_cache_mu;
static std::vector<CachedBlock> g_cache[2];          // 0: device, 1: pinned
static size_t g_cached[2] = {0, 0};
static size_t cache_limit(int kind) {
    const size_t gb = (size_t)pga_knobs::process_knobs().cache_gb;
    return kind == 0 ? gb << 30 : std::min<size_t>(gb << 30, (size_t)2 << 30);
}
static void* cache_take(int kind, int dev, size_t want, size_t* cap, size_t roomy = 2) {
    std::lock_guard<std::mutex> g(g_cache_mu);
    std::vector<CachedBlock>& v = g_cache[kind];
    int best = -1;
    for (int k = 0; k < (int)v.size(); k++)
        if (v[k].dev == dev && v[k].cap >= want && v[k].cap <= roomy * want + ((size_t)1 << 20) && (best < 0 || v[k].cap < v[best].cap)) best = k;
    if (best < 0) return nullptr;
    void* p = v[best].p; *cap = v[best].cap;
    g_cached[kind] -= v[best].cap;
    v.erase(v.begin() + best);
    return p;
}
static bool cache_put(int kind, int dev, void* p, size_t cap) {
    std::lock_guard<std::mutex> g(g_cache_mu);
    if (g_cached[kind] + cap > cache_limit(kind) || g_cache[kind].size() >= 4096) return false;
    g_cache[kind].push_back(CachedBlock{p, cap, dev});
    g_cached[kind] += cap;
    return true;
}
// a pinned block of a freed result: always taken -- when the cache is full the oldest pinned result blocks go back to the runtime first
// (a workload with results of another size would otherwise pay hipHostMalloc / hipHostFree on every call: round 6, seen as 7 ms steps of a
// 4 ms workload behind a job that had filled the cache)
static void cache_put_result(void* p, size_t cap) {
    std::vector<void*> drop;
    {
        std::lock_guard<std::mutex> g(g_cache_mu);
        std::vector<CachedBlock>& v = g_cache[1];
        for (size_t k = 0; k < v.size() && (g_cached[1] + cap > cache_limit(1) || v.size() >= 4096); ) {
            if (v[k].dev != -1) { k++; continue; }
            drop.push_back(v[k].p); g_cached[1] -= v[k].cap; v.erase(v.begin() + (long)k);
        }
        if (g_cached[1] + cap <= cache_limit(1) && v.size() < 4096) { v.push_back(CachedBlock{p, cap, -1}); g_cached[1] += cap; p = nullptr; }
    }
    for (void* q : drop) (void)hipHostFree(q);
    if (p != nullptr) (void)hipHostFree(p);
}
// Test support: see include/pyrodigal_amd.h.  Only buffers of floating-point elements are filled: a pattern read as an index would be a
// wild address, and a stale read has to show as a wrong answer, not as a fault.
extern "C" int pga_debug_poison(pga_ctx* c, int byte, int64_t out[2]) {
    if (out) out[0] = out[1] = 0;
    if (!c || byte < -1 || byte > 255) { if (c) c->err = "pga_debug_poison: byte must be 0..255, or -1"; return PGA_EINVAL; }
    HT(c, hipSetDevice(c->device));
    HT(c, hipDeviceSynchronize());              // every stream of the context: the call's, the upload's
    c->poison = byte;
    if (byte < 0 || !c->finder) return PGA_OK;
    FinderState* f = c->finder;
    int64_t nb = 0, bytes = 0;
    for (auto& kv : f->dev) if (kv.second.p && kv.second.fp) { HT(c, hipMemset(kv.second.p, byte, kv.second.cap)); nb++; bytes += (int64_t)kv.second.cap; }
    for (auto& kv : f->pin) if (kv.second.p && kv.second.fp) { memset(kv.second.p, byte, kv.second.cap); nb++; bytes += (int64_t)kv.second.cap; }
    {
        std::lock_guard<std::mutex> g(f->spare_mu);
        if (f->spare_p) { HT(c, hipMemset(f->spare_p, 'N', f->spare_cap)); nb++; bytes += (int64_t)f->spare_cap; }
    }
    HT(c, hipDeviceSynchronize());
    if (out) { out[0] = nb; out[1] = bytes; }
    return PGA_OK;
}

extern "C" void pga_release_cached(void) {
    std::lock_guard<std::mutex> g(g_cache_mu);
    for (auto& b : g_cache[0]) hipFree(b.p);
    for (auto& b : g_cache[1]) hipHostFree(b.p);
    g_cache[0].clear(); g_cache[1].clear(); g_cached[0] = g_cached[1] = 0;
}
// An allocation that fails while blocks are parked here (a cached block only serves requests of about its own size) gets a second
// try after the parked blocks of that kind have gone back to the runtime.
template <class Alloc>
static hipError_t alloc_or_evict(int kind, Alloc alloc) {
    hipError_t e = alloc();
    if (e != hipErrorOutOfMemory) return e;
    (void)hipGetLastError();                          // the failed attempt is not this call's error
    bool had;
    {
        std::lock_guard<std::mutex> g(g_cache_mu);
        had = !g_cache[kind].empty();
        for (auto& b : g_cache[kind]) { if (kind == 0) hipFree(b.p); else hipHostFree(b.p); }
        g_cache[kind].clear(); g_cached[kind] = 0;
    }
    return had ? alloc() : e;
}

// Test support (pga_debug_poison): a block that a float buffer has just acquired -- from the runtime or from the cache, never written by
// this context -- is filled with the context's poison byte.
static int poison_fill(pga_ctx* c, void* p, size_t cap, int byte, bool pinned) {
    if (pinned) { memset(p, byte, cap); return PGA_OK; }
    HT(c, hipMemset(p, byte, cap));
    HT(c, hipDeviceSynchronize());
    return PGA_OK;
}

int ensure_dev(pga_ctx* c, const char* name, size_t bytes, void** out, bool fp = false) {
    Buf& b = c->finder->dev[name];
    if (b.cap < bytes || !b.p) {
        if (b.p) { hipFree(b.p); b.p = nullptr; b.cap = 0; }     // (not to the cache: kernels of this call may still read it; hipFree waits)
        // room to grow: the calls of a job are about the same size, so the big buffers get a sixteenth on top, the small ones a quarter
        size_t want = bytes + (bytes >= ((size_t)64 << 20) ? bytes / 16 : bytes / 4) + 256;
        b.p = cache_take(0, c->device, want, &want);
        if (!b.p) HT(c, alloc_or_evict(0, [&] { return hipMalloc(&b.p, want); }));
        b.cap = want; b.fp = fp;
        if (c->poison >= 0 && fp) { const int rc = poison_fill(c, b.p, b.cap, c->poison, false); if (rc) return rc; }
    }
    *out = b.p;
    return PGA_OK;
}
int ensure_pin(pga_ctx* c, const char* name, size_t bytes, void** out, bool fp = false) {
    Buf& b = c->finder->pin[name];
    if (b.cap < bytes || !b.p) {
        if (b.p) { hipHostFree(b.p); b.p = nullptr; b.cap = 0; }
        size_t want = bytes + bytes / 4 + 256;
        b.p = cache_take(1, c->device, want, &want);
        if (!b.p) HT(c, alloc_or_evict(1, [&] { return hipHostMalloc(&b.p, want, hipHostMallocDefault); }));
        b.cap = want; b.fp = fp;
        if (c->poison >= 0 && fp) { const int rc = poison_fill(c, b.p, b.cap, c->poison, true); if (rc) return rc; }
    }
    *out = b.p;
    return PGA_OK;
}
#define DEVBUF(var, type, name, count) type* var; DEVSET(var, type, name, count)
#define DEVSET(var, type, name, count) { void* p__; int rc__ = ensure_dev(c, name, sizeof(type) * (size_t)(count) + 64, &p__, std::is_floating_point<type>::value); if (rc__) return rc__; var = (type*)p__; }
#define PINSET(var, type, name, count) { void* p__; int rc__ = ensure_pin(c, name, sizeof(type) * (size_t)(count) + 64, &p__, std::is_floating_point<type>::value); if (rc__) return rc__; var = (type*)p__; }
#define PINBUF(var, type, name, count) type* var; PINSET(var, type, name, count)

// ---- tail on host threads (PGA_TAIL=host): the rules are tail_rules.h's, here is only how long paths and gene lists are split ----
// eliminate_bad_genes on several threads: path positions are independent in either loop (elim_add_terms); the second loop reads
// the finished scores.
void eliminate_bad_genes_mt(const NodeView& v, const int32_t* path, int cnt, double st_wt, WorkerPool& pool, int threads) {
    if (cnt < 4096 || threads <= 1) { eliminate_bad_genes(v, path, cnt, st_wt); return; }
    std::atomic<int> next(cnt - 1);
    bool marking = false;
    const std::function<void()> work = [&]() {          // 512 path positions at a time, from the head
        const int lo = marking ? 1 : 0;                  // a pair is path[q], path[q - 1]
        for (;;) {
            const int hi = next.fetch_sub(512);
            if (hi < lo) break;
            for (int q = hi; q > hi - 512 && q >= lo; q--) {
                if (marking) elim_mark_pair(v, path, q); else elim_add_terms(v, path, cnt, q, st_wt);
            }
        }
    };
    pool.run(work, threads);
    next.store(cnt - 1); marking = true;
    pool.run(work, threads);
}

// In-order semantics of the reference loop, evaluated in parallel when a contig has many genes: every
// gene is first tweaked against its ORIGINAL neighbours; a gene whose predecessor did change is then
// redone in order against the predecessor's final record (tweaks are rare, so few are redone).
void tweak_final_starts(const NodeView& v, std::vector<GeneRec>& g, double w, int maxov, int inner_threads = 1, WorkerPool* pool = nullptr) {
    const int ng = (int)g.size();
    if (inner_threads <= 1 || ng < 2048 || pool == nullptr) {
        for (int i = 0; i < ng; i++) tweak_one(v, i > 0 ? &g[i - 1] : nullptr, g[i], i < ng - 1 ? &g[i + 1] : nullptr, w, maxov);
        return;
    }
    const std::vector<GeneRec> orig(g);
    std::atomic<int> next(0);
    auto work = [&]() {
        for (;;) {
            const int i0 = next.fetch_add(256);
            if (i0 >= ng) break;
            for (int i = i0; i < std::min(ng, i0 + 256); i++)
                tweak_one(v, i > 0 ? &orig[i - 1] : nullptr, g[i], i < ng - 1 ? &orig[i + 1] : nullptr, w, maxov);
        }
    };
    pool->run(work, inner_threads);
    for (int i = 1; i < ng; i++) {
        if (g[i - 1].start_ndx == orig[i - 1].start_ndx) continue;       // predecessor unchanged: the parallel result stands
        g[i] = orig[i];
        tweak_one(v, &g[i - 1], g[i], i < ng - 1 ? &orig[i + 1] : nullptr, w, maxov);
    }
}

// ---- tail kernels (tail.inl): what they are handed --------------------------------------------------------------------------------------
struct OutArrays;
struct TailDesc {          // one per contig
    int64_t out_off;       // first node of the contig's winning chain in the gathered arrays
    int64_t gene_off;      // first slot of the contig's gene records (capacity n / 2 + 2)
    int32_t n;             // nodes (0: no winning model)
    int32_t mx;            // _find_max_index of the winning pass
    double  st_wt;
    // where the winner's final-pass node fields and its topology sit in the arrays the scorers wrote (k_emit_genes reads the
    // two nodes of a gene from there when the winners were gathered without them)
    int64_t fin_off, topo_off;
    int32_t group, _pad;
    int64_t dp_off;        // the winning pass's chain offset (what the connection scoring saw)
};
// ---- gather kernel: pack the winning chains' node fields contiguously for one D2H per field ----
struct WinDesc {
    int64_t out_off;     // first output node
    int64_t dp_off;      // chain offset of the pass that won (scores as seen by the DP)
    int64_t fin_off;     // chain offset of the fresh re-score (== dp_off when the winner was `first`)
    int64_t topo_off;
    int32_t n;
    int32_t _pad;
};
struct GcPtrs { const float* p[4]; };      // GroupArrays::gc_cont of every translation-table group
struct OutArrays {
    int32_t* ndx; int32_t* stop_val; uint8_t* type; int8_t* strand; float* gc_cont;
    uint8_t* edge_dp; double* cscore_dp; double* sscore_dp; double* rscore_dp; double* uscore_dp; double* tscore_dp;
    int32_t* star_ptr; int32_t* traceb; int8_t* ov_mark; double* score;
    uint8_t* edge; double* cscore; double* sscore; double* rscore; double* uscore; double* tscore; double* mot_score;
    int32_t* mot_ndx; uint8_t* rbs; uint8_t* mot_len; uint8_t* mot_spacer; uint8_t* mot_spacendx;
    // direct != 0 (nobody reads the node arrays after the call): only the fields the tail WRITES -- sscore_dp, traceb, ov_mark -- are
    // gathered; what it only reads stays where the scorers left it: the topology of the contig's group at TailDesc::topo_off, the
    // DP pass's node fields and scores at TailDesc::dp_off
    int32_t direct;
    const int32_t* g_ndx[4]; const int32_t* g_stop_val[4]; const uint8_t* g_type[4]; const int8_t* g_strand[4];
    const uint8_t* c_edge; const double* c_cscore; const double* c_rscore; const double* c_uscore; const double* c_tscore;
    const int32_t* c_star_ptr; const double* d_score;
};

__global__ void __launch_bounds__(256)
k_gather_winners(const WinDesc* __restrict__ wd, int n_win, int64_t out_begin, int64_t total, GroupArrays ga, ChainArrays ca,
                 DpBuffers dp, OutArrays o, const int lean /* 1: only what the device tail walks */) {
    __shared__ int s_w0;
    const int64_t blk0 = out_begin + (int64_t)blockIdx.x * blockDim.x;
    const int64_t g = blk0 + threadIdx.x;
    int lo = block_search_le([&](const int k) { return wd[k].out_off; }, n_win, blk0, &s_w0);      // one search per workgroup, then a short walk per thread
    if (g >= out_begin + total) return;
    while (lo + 1 < n_win && wd[lo + 1].out_off <= g) lo++;
    const WinDesc w = wd[lo];
    const int i = (int)(g - w.out_off);
    const int64_t t = w.topo_off + i, a = w.dp_off + i, f = w.fin_off + i;
    if (o.direct) { o.sscore_dp[g] = ca.sscore[a]; o.traceb[g] = dp.traceb[a]; o.ov_mark[g] = dp.ov_mark[a]; return; }
    o.ndx[g] = ga.ndx[t]; o.stop_val[g] = ga.stop_val[t]; o.type[g] = ga.type[t]; o.strand[g] = ga.strand[t];
    o.edge_dp[g] = ca.edge[a]; o.cscore_dp[g] = ca.cscore[a]; o.sscore_dp[g] = ca.sscore[a]; o.rscore_dp[g] = ca.rscore[a];
    o.uscore_dp[g] = ca.uscore[a]; o.tscore_dp[g] = ca.tscore[a];
    o.star_ptr[3 * g] = ca.star_ptr[3 * a]; o.star_ptr[3 * g + 1] = ca.star_ptr[3 * a + 1]; o.star_ptr[3 * g + 2] = ca.star_ptr[3 * a + 2];
    o.traceb[g] = dp.traceb[a]; o.ov_mark[g] = dp.ov_mark[a]; o.score[g] = dp.score[a];
    // the final-pass fields: fourteen of the thirty per node.  Only the two nodes of a gene are ever looked at unless the caller
    // wants the node arrays, and k_emit_genes can fetch those from where the scorer left them
    if (lean) return;
    o.gc_cont[g] = ga.gc_cont[t];
    o.edge[g] = ca.edge[f]; o.cscore[g] = ca.cscore[f]; o.sscore[g] = ca.sscore[f]; o.rscore[g] = ca.rscore[f];
    o.uscore[g] = ca.uscore[f]; o.tscore[g] = ca.tscore[f]; o.mot_score[g] = ca.mot_score[f]; o.mot_ndx[g] = ca.mot_ndx[f];
    o.rbs[2 * g] = ca.rbs[2 * f]; o.rbs[2 * g + 1] = ca.rbs[2 * f + 1];
    o.mot_len[g] = ca.mot_len[f]; o.mot_spacer[g] = ca.mot_spacer[f]; o.mot_spacendx[g] = ca.mot_spacendx[f];
}

// Final-pass fields of the two nodes of every gene (start, stop), fetched after the host tail so that
// the full per-node arrays of the re-score need not cross PCIe unless the caller asks for nodes.
struct GeneNodeAttr {
    double cscore, sscore, rscore, uscore, tscore, mot_score;
    float gc_cont; int32_t mot_ndx;
    uint8_t edge, rbs[2], mot_len, mot_spacer, _pad[3];
};

// Coding bases (pga_find_coding_bases): the positions [begin, end] of every gene record, clipped to its contig, set in a bitmap of
// one bit per base of the batch (bit ct[contig].base + position - 1).  A wavefront per gene, its lanes over the 32-bit words the
// gene touches; neighbouring genes and contigs share words, hence the atomic OR.
__global__ void __launch_bounds__(256)
k_cover_genes(const pga_gene* __restrict__ genes, int64_t n_genes, const ContigDesc* __restrict__ ct, int n_contigs, uint32_t* __restrict__ bits) {
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (g >= n_genes) return;
    const int c = genes[g].contig;
    if (c < 0 || c >= n_contigs) return;
    const int32_t b = max(genes[g].begin, 1), e = min(genes[g].end, ct[c].len);
    if (b > e) return;
    const int64_t b0 = ct[c].base + b - 1, b1 = ct[c].base + e - 1;     // inclusive bit range
    const int64_t w0 = b0 >> 5, w1 = b1 >> 5;
    for (int64_t w = w0 + lane; w <= w1; w += 64) {
        uint32_t m = 0xffffffffu;
        if (w == w0) m &= 0xffffffffu << (b0 & 31);
        if (w == w1) m &= 0xffffffffu >> (31 - (b1 & 31));
        atomicOr(&bits[w], m);
    }
}

// A workgroup per contig: the set bits of [base, base + len).
__global__ void __launch_bounds__(256)
k_count_cover(const uint32_t* __restrict__ bits, const ContigDesc* __restrict__ ct, int64_t* __restrict__ coding) {
    __shared__ int64_t part[4];
    const int c = blockIdx.x;
    const int64_t lo = ct[c].base, len = ct[c].len;
    int64_t n = 0;
    if (len > 0) {
        const int64_t hi = lo + len - 1, w0 = lo >> 5, w1 = hi >> 5;
        for (int64_t w = w0 + threadIdx.x; w <= w1; w += blockDim.x) {
            uint32_t m = bits[w];
            if (w == w0) m &= 0xffffffffu << (lo & 31);
            if (w == w1) m &= 0xffffffffu >> (31 - (hi & 31));
            n += __popc(m);
        }
    }
    for (int d = 32; d > 0; d >>= 1) n += __shfl_down(n, d, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) coding[c] = part[0] + part[1] + part[2] + part[3];
}

#include "tail.inl"

struct ResultOwner {
    pga_result pub;
    std::vector<pga_contig_result> contigs;
    std::vector<pga_gene> genes;
    // Round 6: the gene records of a large result land in PINNED memory that the result owns (from the process-wide cache of pinned
    // blocks, back to it when the result is freed): the read-back of 16 MB per 125 Mbp call is one DMA to where the records stay, where
    // a std::vector meant a value-initialised allocation (page faults) and a copy staged through the runtime's own pinned buffers,
    // 0.8 .. 4 ms of a 9 ms call.
    pga_gene* pin_genes = nullptr; size_t pin_cap = 0, pin_n = 0;
    std::vector<pga_nodes> nodes;
    std::vector<int32_t> mask_off, masks;
    bool has_masks = false;            // a mask source was set: the lists are reported (empty ones too)
    std::vector<void*> blocks;
    ~ResultOwner() {
        for (void* b : blocks) free(b);
        if (pin_genes != nullptr) cache_put_result(pin_genes, pin_cap);
    }
    // room for n gene records; pinned when the result is large enough for it to matter
    pga_gene* gene_records(const size_t n, const bool pageable /* Knobs::pageable_results */) {
        const size_t bytes = n * sizeof(pga_gene);
        if (bytes < ((size_t)256 << 10) || pageable) { genes.resize(n); return genes.data(); }
        size_t cap = 0;
        void* p = cache_take(1, -1, bytes, &cap, 8);         // (a block up to eight times the size will do: results vary, pinned allocations cost milliseconds)
        if (p == nullptr) {
            cap = (bytes + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1);
            if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); genes.resize(n); return genes.data(); }
        }
        pin_genes = (pga_gene*)p; pin_cap = cap; pin_n = n;
        return pin_genes;
    }
};

// one zeroed block per contig for the SoA node arrays of a result
int alloc_nodes(ResultOwner* R, pga_nodes& N, const int n) {
    memset(&N, 0, sizeof N);
    N.n = n;
    const size_t bytes = (size_t)n * (4 * 8 + 10 + 4 + 8 * 7) + 8 * 32;   // 8 int32, 10 bytes, 1 float, 7 doubles per node + padding
    char* blk = (char*)calloc(1, bytes);
    if (!blk) return PGA_ENOMEM;
    R->blocks.push_back(blk);
    char* q = blk;
    auto take = [&](size_t b) { char* r = q; q += (b + 7) & ~(size_t)7; return (void*)r; };
    N.ndx = (int32_t*)take(4 * n); N.stop_val = (int32_t*)take(4 * n); N.traceb = (int32_t*)take(4 * n); N.tracef = (int32_t*)take(4 * n);
    N.star_ptr = (int32_t*)take(12 * n); N.mot_ndx = (int32_t*)take(4 * n);
    N.type = (uint8_t*)take(n); N.edge = (uint8_t*)take(n); N.elim = (uint8_t*)take(n); N.rbs = (uint8_t*)take(2 * n);
    N.strand = (int8_t*)take(n); N.ov_mark = (int8_t*)take(n); N.mot_len = (uint8_t*)take(n); N.mot_spacer = (uint8_t*)take(n); N.mot_spacendx = (uint8_t*)take(n);
    N.gc_cont = (float*)take(4 * n);
    N.cscore = (double*)take(8 * n); N.sscore = (double*)take(8 * n); N.rscore = (double*)take(8 * n); N.uscore = (double*)take(8 * n);
    N.tscore = (double*)take(8 * n); N.score = (double*)take(8 * n); N.mot_score = (double*)take(8 * n);
    return PGA_OK;
}

void fill_model_score_const(ModelScoreConst* m, const pga_training* t) {   // ref: lib.pyx:2136-2147, 2209-2210
    double no_stop;
    if (t->trans_table != 11) {
        no_stop = ((1 - t->gc) * (1 - t->gc) * t->gc) / 8.0;
        no_stop += ((1 - t->gc) * (1 - t->gc) * (1 - t->gc)) / 8.0;
    } else {
        no_stop = ((1 - t->gc) * (1 - t->gc) * t->gc) / 4.0;
        no_stop += ((1 - t->gc) * (1 - t->gc) * (1 - t->gc)) / 8.0;
    }
    no_stop = 1 - no_stop;
    m->lfac_max = log((1 - pow(no_stop, 1000.0)) / pow(no_stop, 1000.0));
    m->lfac_min = log((1 - pow(no_stop, 80)) / pow(no_stop, 80));
    for (int n = 0; n <= 1000; n++) {
        const double tmp = pow(no_stop, (double)n);
        m->lfac_tab[n] = log((1 - tmp) / tmp) - m->lfac_min;
    }
}

}  // namespace

void pga_finder_release(pga_ctx* c) {
    if (!c->finder) return;
    if (read_knobs().print_buffers) {
        // diagnostics: what this context held on the device, largest first
        std::vector<std::pair<size_t, std::string>> v; size_t tot = 0;
        for (auto& kv : c->finder->dev) if (kv.second.p) { v.push_back({kv.second.cap, kv.first}); tot += kv.second.cap; }
        std::sort(v.begin(), v.end(), [](const std::pair<size_t, std::string>& a, const std::pair<size_t, std::string>& b) { return a.first > b.first; });
        fprintf(stderr, "[pga] context buffers: %.2f GB in %zu allocations\n", tot / 1e9, v.size());
        for (size_t k = 0; k < v.size() && k < 48; k++) fprintf(stderr, "[pga]   %-22s %9.1f MB\n", v[k].second.c_str(), v[k].first / 1e6);
    }
    if (c->stream) (void)hipStreamSynchronize(c->stream);        // nothing of this context still reads what goes to the cache
    for (auto& kv : c->finder->dev) if (kv.second.p && !cache_put(0, c->device, kv.second.p, kv.second.cap)) hipFree(kv.second.p);
    for (auto& kv : c->finder->pin) if (kv.second.p && !cache_put(1, c->device, kv.second.p, kv.second.cap)) hipHostFree(kv.second.p);
    if (c->finder->d_msc) hipFree(c->finder->d_msc);
    if (c->finder->d_model_gc) hipFree(c->finder->d_model_gc);
    if (c->finder->d_model_grp) hipFree(c->finder->d_model_grp);
    if (c->finder->d_gil) hipFree(c->finder->d_gil);
    if (c->finder->d_model_rank) hipFree(c->finder->d_model_rank);
    if (c->finder->d_sd_lut) hipFree(c->finder->d_sd_lut);
    if (c->finder->spare_p) hipFree(c->finder->spare_p);
    if (c->finder->up_stream) { (void)hipStreamSynchronize(c->finder->up_stream); (void)hipStreamDestroy(c->finder->up_stream); }
    if (c->finder->up_pin && !cache_put(1, c->device, c->finder->up_pin, c->finder->up_pin_cap)) hipHostFree(c->finder->up_pin);
    if (c->finder->up_ev) hipEventDestroy(c->finder->up_ev);
    if (c->finder->up_dev) hipFree(c->finder->up_dev);
    if (c->finder->e_start) hipEventDestroy(c->finder->e_start);
    if (c->finder->e_stop) hipEventDestroy(c->finder->e_stop);
    for (int i = 0; i < 4; i++) { if (c->finder->e_dp0[i]) hipEventDestroy(c->finder->e_dp0[i]); if (c->finder->e_dp1[i]) hipEventDestroy(c->finder->e_dp1[i]); }
    for (int i = 0; i < 20; i++) if (c->finder->e_aux[i]) hipEventDestroy(c->finder->e_aux[i]);
    delete c->finder;
    c->finder = nullptr;
}

int pga_finder_models_changed(pga_ctx* c) {
    if (!c->finder) {
        c->finder = new (std::nothrow) FinderState();
        if (!c->finder) return PGA_ENOMEM;
        HT(c, hipEventCreate(&c->finder->e_start)); HT(c, hipEventCreate(&c->finder->e_stop));
        for (int i = 0; i < 4; i++) { HT(c, hipEventCreate(&c->finder->e_dp0[i])); HT(c, hipEventCreate(&c->finder->e_dp1[i])); }
        for (int i = 0; i < 20; i++) HT(c, hipEventCreate(&c->finder->e_aux[i]));
        HT(c, hipMalloc((void**)&c->finder->d_sd_lut, sizeof(unsigned) * 1920));
        pga_launch_sd_lut(c->finder->d_sd_lut, c->stream);
        HT(c, hipStreamSynchronize(c->stream));
    }
    FinderState* f = c->finder;
    f->model_group.clear(); f->group_tt.clear();
    if (f->d_msc) { hipFree(f->d_msc); f->d_msc = nullptr; }
    if (f->d_model_gc) { hipFree(f->d_model_gc); f->d_model_gc = nullptr; }
    if (f->d_model_grp) { hipFree(f->d_model_grp); f->d_model_grp = nullptr; }
    if (f->d_gil) { hipFree(f->d_gil); f->d_gil = nullptr; }
    if (f->d_model_rank) { hipFree(f->d_model_rank); f->d_model_rank = nullptr; }
    f->gil_off.clear(); f->gil_stride.clear();
    const int nm = c->n_models;
    if (nm == 0) return PGA_OK;
    std::vector<ModelScoreConst> msc(nm);
    for (int m = 0; m < nm; m++) {
        const int tt = c->models[m].trans_table;
        int g = -1;
        for (size_t k = 0; k < f->group_tt.size(); k++) if (f->group_tt[k] == tt) g = (int)k;
        if (g < 0) { g = (int)f->group_tt.size(); f->group_tt.push_back(tt); }
        f->model_group.push_back(g);
        fill_model_score_const(&msc[m], &c->models[m]);
    }
    if (f->group_tt.size() > 4) { c->err = "pga_set_models: more than 4 distinct translation tables"; return PGA_EINVAL; }
    HT(c, hipMalloc((void**)&f->d_msc, sizeof(ModelScoreConst) * nm));
    HT(c, hipMemcpy(f->d_msc, msc.data(), sizeof(ModelScoreConst) * nm, hipMemcpyHostToDevice));
    std::vector<double> mgc(nm);
    for (int m = 0; m < nm; m++) mgc[m] = c->models[m].gc;
    HT(c, hipMalloc((void**)&f->d_model_gc, sizeof(double) * nm));
    HT(c, hipMalloc((void**)&f->d_model_grp, sizeof(int32_t) * nm));
    HT(c, hipMemcpy(f->d_model_gc, mgc.data(), sizeof(double) * nm, hipMemcpyHostToDevice));
    HT(c, hipMemcpy(f->d_model_grp, f->model_group.data(), sizeof(int32_t) * nm, hipMemcpyHostToDevice));
    {
        const int ng = (int)f->group_tt.size();
        std::vector<int32_t> rank(nm, 0), count(ng, 0);
        for (int m = 0; m < nm; m++) rank[m] = count[f->model_group[m]]++;
        size_t total_il = 0;
        for (int g = 0; g < ng; g++) { f->gil_stride.push_back((count[g] + 1) & ~1); f->gil_off.push_back(total_il); total_il += (size_t)4096 * f->gil_stride[g]; }
        std::vector<double> il(total_il + 8, 0.0);               // a pair load at the last column of the last row stays inside
        for (int m = 0; m < nm; m++) {
            const int g = f->model_group[m];
            for (int h = 0; h < 4096; h++) il[f->gil_off[g] + (size_t)h * f->gil_stride[g] + rank[m]] = c->models[m].gene_dc[h];
        }
        HT(c, hipMalloc((void**)&f->d_gil, sizeof(double) * il.size()));
        HT(c, hipMalloc((void**)&f->d_model_rank, sizeof(int32_t) * nm));
        HT(c, hipMemcpy(f->d_gil, il.data(), sizeof(double) * il.size(), hipMemcpyHostToDevice));
        HT(c, hipMemcpy(f->d_model_rank, rank.data(), sizeof(int32_t) * nm, hipMemcpyHostToDevice));
        f->model_rank = rank;
    }
    return PGA_OK;
}

struct pga_batch {
    pga_ctx* ctx;
    int32_t n;
    int64_t total;
    std::vector<ContigDesc> ct;   // n + 1 entries
    char* d_seq;                  // packed ASCII, resident in HBM
    size_t d_seq_cap = 0;         // bytes of that allocation (it goes back to the context's spare slot)
    TileDesc* d_tiles;            // extraction tiles of every contig (behind the letters, in their allocation)
    int32_t* d_tile0;             // first tile of every contig, n + 1 entries (behind d_tiles)
    int32_t n_tiles;
    // mask sources attached to the batch (pga_batch_set_regions / pga_batch_set_mask_case): every call on the batch honours them
    int mask_case = 0;                // 1: runs of lower-case letters are masked like runs of unknown bases
    std::vector<int32_t> reg_off;     // the caller's intervals: contig i owns regions[reg_off[i] .. reg_off[i + 1]); empty: none attached
    std::vector<MaskRun> regions;     // (contig, begin, end) as given: any order, overlaps allowed
    MaskRun* d_regions = nullptr;     // their device copy
    // topology (pga_batch_set_circular): one flag per contig, empty: every contig is linear
    std::vector<uint8_t> circular;
    // contig sets (pga_batch_set_sets): the caller's label per contig, -1: on its own; empty: no labels
    std::vector<int32_t> sets;
};

// Tiles of a batch: every position of a contig of at least three bases lies in one tile.  Host vectors for one upload.
static void batch_tiles(const pga_batch* b, std::vector<TileDesc>& tiles, std::vector<int32_t>& tile0) {
    const int TS = pga_extract_tile_size();
    tile0.resize((size_t)b->n + 1);
    for (int i = 0; i < b->n; i++) {
        tile0[i] = (int32_t)tiles.size();
        const int64_t L = b->ct[i].len;
        if (L >= 3) for (int64_t s0 = 0; s0 < L; s0 += TS) tiles.push_back(TileDesc{i, (int32_t)s0});
    }
    tile0[b->n] = (int32_t)tiles.size();
}
// the tile list and the per-contig first-tile table live behind the letters, in the same device allocation (`at`, 256-byte aligned)
static size_t batch_tiles_bytes(const std::vector<TileDesc>& tiles, const std::vector<int32_t>& tile0) {
    return sizeof(TileDesc) * tiles.size() + sizeof(int32_t) * tile0.size() + 64 + 256;
}
static hipError_t batch_upload_tiles(pga_batch* b, char* at, const std::vector<TileDesc>& tiles, const std::vector<int32_t>& tile0, hipStream_t st) {
    b->n_tiles = (int32_t)tiles.size();
    const size_t tb = sizeof(TileDesc) * tiles.size(), zb = sizeof(int32_t) * tile0.size();
    b->d_tiles = (TileDesc*)(((uintptr_t)at + 255) & ~(uintptr_t)255);
    b->d_tile0 = (int32_t*)((char*)b->d_tiles + tb);
    hipError_t e = hipSuccess;
    if (tb) e = hipMemcpyAsync(b->d_tiles, tiles.data(), tb, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(b->d_tile0, tile0.data(), zb, hipMemcpyHostToDevice, st);
    return e;
}

extern "C" int pga_dp_start_order(int32_t n_chains, const int32_t* nodes_per_chain, int32_t* order) {
    if (n_chains < 0 || (n_chains > 0 && (!nodes_per_chain || !order))) return PGA_EINVAL;
    // counting sort on walk batches (nodes / 64), most first; stable, so equals keep the launch order
    int maxb = 0;
    for (int k = 0; k < n_chains; k++) maxb = std::max(maxb, std::max(nodes_per_chain[k], 0) >> 6);
    std::vector<int32_t> first((size_t)maxb + 2, 0);
    for (int k = 0; k < n_chains; k++) first[(size_t)(maxb - (std::max(nodes_per_chain[k], 0) >> 6)) + 1]++;
    for (int b = 0; b <= maxb; b++) first[(size_t)b + 1] += first[(size_t)b];
    for (int k = 0; k < n_chains; k++) order[(size_t)first[(size_t)(maxb - (std::max(nodes_per_chain[k], 0) >> 6))]++] = k;
    return PGA_OK;
}

// The start order made XCD-aware: workgroup b runs on XCD b % 8, and chains that share a key (a contig under one translation table:
// the same topology arrays) should meet in one XCD's L2.  `order` is a start order (pga_dp_start_order); every key goes to the XCD
// with the fewest nodes so far, in that order; out[8 k + x] = k-th chain of XCD x, -1 where a queue has ended.  Returns the number
// of entries written (a multiple of 8, at most 8 * n_chains), or a negative error code.
extern "C" int64_t pga_dp_xcd_order(int32_t n_chains, const int32_t* order, const int32_t* nodes_per_chain, const int32_t* key_of_chain, int32_t n_keys,
                                    int32_t* out, int64_t out_cap) {
    if (n_chains < 0 || n_keys < 0 || (n_chains > 0 && (!order || !nodes_per_chain || !key_of_chain || !out))) return -(int64_t)PGA_EINVAL;
    std::vector<int32_t> queue[8];
    int64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<int8_t> xcd_of((size_t)n_keys, (int8_t)-1);
    for (int p = 0; p < n_chains; p++) {
        const int c = order[p];
        if (c < 0 || c >= n_chains || key_of_chain[c] < 0 || key_of_chain[c] >= n_keys) return -(int64_t)PGA_EINVAL;
        int8_t& x = xcd_of[(size_t)key_of_chain[c]];
        if (x < 0) { int best = 0; for (int q = 1; q < 8; q++) if (load[q] < load[best]) best = q; x = (int8_t)best; }
        queue[x].push_back(c);
        load[x] += std::max(nodes_per_chain[c], 0);
    }
    size_t longest = 0;
    for (int q = 0; q < 8; q++) longest = std::max(longest, queue[q].size());
    if ((int64_t)(longest * 8) > out_cap) return -(int64_t)PGA_EINVAL;
    for (size_t k = 0; k < longest * 8; k++) out[k] = -1;
    for (int q = 0; q < 8; q++) for (size_t k = 0; k < queue[q].size(); k++) out[k * 8 + (size_t)q] = queue[q][k];
    return (int64_t)(longest * 8);
}

extern "C" int pga_cs_task_summary(int32_t n_contigs, const int32_t* nodes_per_contig, const int32_t* first_column,
                                   const int32_t* models_per_contig, int32_t task_nodes, int64_t out[5]) {
    if (n_contigs < 0 || !out || (n_contigs > 0 && (!nodes_per_contig || !first_column || !models_per_contig)) || task_nodes < 1) return PGA_EINVAL;
    // the inputs in the shape pga_cs_tasks plans from: one chain per (contig, model), columns = model ranks
    std::vector<int2> cc((size_t)n_contigs); std::vector<ChainDesc> chains; std::vector<int32_t> cbase((size_t)n_contigs + 1, 0), rank;
    int max_col = 0;
    for (int i = 0; i < n_contigs; i++) max_col = std::max(max_col, first_column[i] + std::max(models_per_contig[i], 0));
    rank.resize((size_t)max_col + 1);
    for (int m = 0; m <= max_col; m++) rank[(size_t)m] = m;
    for (int i = 0; i < n_contigs; i++) {
        cbase[(size_t)i + 1] = cbase[(size_t)i] + std::max(nodes_per_contig[i], 0);
        cc[(size_t)i] = make_int2((int)chains.size(), std::max(models_per_contig[i], 0));
        for (int m = 0; m < models_per_contig[i]; m++) { ChainDesc ch{}; ch.model = first_column[i] + m; ch.contig = i; ch.n = nodes_per_contig[i]; chains.push_back(ch); }
    }
    std::vector<int32_t> tasks, entries;
    if (!pga_cs_tasks(cc.data(), n_contigs, chains.data(), cbase.data(), rank.data(), task_nodes, tasks, entries)) return PGA_EINVAL;
    const size_t nt = tasks.size() / 4, ne = entries.size() / 4;
    int64_t biggest = 0, total = 0; bool falling = true;
    for (size_t t = 0; t < nt; t++) {
        int64_t nodes = 0;
        for (int e = 0; e < tasks[4 * t + 2]; e++) nodes += entries[4 * (size_t)(tasks[4 * t + 1] + e) + 3];
        biggest = std::max(biggest, nodes); total += nodes;
        if (t > 0 && tasks[4 * t] > tasks[4 * (t - 1)]) falling = false;
    }
    out[0] = (int64_t)nt; out[1] = (int64_t)ne; out[2] = biggest; out[3] = total; out[4] = falling ? 1 : 0;
    return PGA_OK;
}

// The letters of a batch live in one device allocation.  hipMalloc / hipFree per call cost a device-wide synchronisation each
// (hipFree waits for every stream of the device, i.e. for the other contexts' kernels), so a context keeps the allocation of the
// last batch it freed and hands it to the next one that fits.
// (pga_debug_poison: the letters are bytes, not floats -- 'N', so that the padding behind the last contig is defined and harmless)
static hipError_t batch_poison(char* p, size_t cap) {
    const hipError_t e = hipMemset(p, 'N', cap);
    return e == hipSuccess ? hipDeviceSynchronize() : e;
}
static hipError_t batch_take_dev(pga_ctx* c, size_t bytes, char** out, size_t* cap) {
    FinderState* f = c->finder;
    {
        std::lock_guard<std::mutex> g(f->spare_mu);
        if (f->spare_p && f->spare_cap >= bytes && f->spare_cap <= 2 * bytes + (64u << 20)) {
            *out = (char*)f->spare_p; *cap = f->spare_cap; f->spare_p = nullptr; f->spare_cap = 0;
            return c->poison >= 0 ? batch_poison(*out, *cap) : hipSuccess;
        }
    }
    const size_t want = bytes + bytes / 8 + 256;
    *cap = want;
    const hipError_t e = hipMalloc((void**)out, want);
    return (e == hipSuccess && c->poison >= 0) ? batch_poison(*out, *cap) : e;
}
static void batch_give_dev(pga_ctx* c, char* p, size_t cap) {
    if (!p) return;
    FinderState* f = c->finder;
    void* drop = p;
    if (f) {
        std::lock_guard<std::mutex> g(f->spare_mu);
        if (!f->spare_p || f->spare_cap < cap) { drop = f->spare_p; f->spare_p = p; f->spare_cap = cap; }
    }
    if (drop) hipFree(drop);
}

// the upload's own stream and pinned staging area (FinderState::up_*; the caller holds up_mu)
static int upload_resources(pga_ctx* c, size_t pin_bytes, hipStream_t* st, char** pin) {
    FinderState* f = c->finder;
    if (!f->up_stream) HT(c, hipStreamCreateWithFlags(&f->up_stream, hipStreamNonBlocking));
    *st = f->up_stream;
    if (pin_bytes > 0 && (f->up_pin_cap < pin_bytes || !f->up_pin)) {
        if (f->up_pin) { hipHostFree(f->up_pin); f->up_pin = nullptr; f->up_pin_cap = 0; }
        size_t want = pin_bytes + pin_bytes / 4 + 256;
        f->up_pin = cache_take(1, c->device, want, &want);
        if (!f->up_pin) HT(c, alloc_or_evict(1, [&] { return hipHostMalloc(&f->up_pin, want, hipHostMallocDefault); }));
        f->up_pin_cap = want;
    }
    if (pin) *pin = (char*)f->up_pin;
    return PGA_OK;
}

// What translate.hip needs of the upload path (pga_translate_genes_tokens): the upload's stream and event, `bytes` of its pinned staging
// area and as many of a device block that the context keeps and grows across calls.  up_mu is held from _take (when it returns PGA_OK)
// to _give: one upload or token call at a time per context.
struct pga_upload_lease { hipStream_t st; hipEvent_t ev; char* pin; char* dev; };
static int upload_lease_fill(pga_ctx* c, size_t bytes, pga_upload_lease* out) {
    FinderState* f = c->finder;
    { const int rc = upload_resources(c, bytes, &out->st, &out->pin); if (rc) return rc; }
    if (!f->up_ev) HT(c, hipEventCreateWithFlags(&f->up_ev, hipEventDisableTiming));
    out->ev = f->up_ev;
    if (f->up_dev_cap < bytes) {
        // (every call on this stream ends with a synchronise: nothing still reads the old block)
        if (f->up_dev) { (void)hipFree(f->up_dev); f->up_dev = nullptr; f->up_dev_cap = 0; }
        const size_t want = bytes + bytes / 4 + 256;
        HT(c, alloc_or_evict(0, [&] { return hipMalloc(&f->up_dev, want); }));
        f->up_dev_cap = want;
    }
    out->dev = (char*)f->up_dev;
    return PGA_OK;
}
int pga_upload_lease_take(pga_ctx* c, size_t bytes, pga_upload_lease* out) {
    if (!c->finder) { const int rc = pga_finder_models_changed(c); if (rc) return rc; }
    c->finder->up_mu.lock();
    const int rc = upload_lease_fill(c, bytes, out);
    if (rc) c->finder->up_mu.unlock();
    return rc;
}
void pga_upload_lease_give(pga_ctx* c) { c->finder->up_mu.unlock(); }

extern "C" int pga_batch_create(pga_ctx* c, int32_t n_contigs, const char* const* seqs, const int64_t* lens, pga_batch** out) {
    if (out) *out = nullptr;
    if (!c || !out || n_contigs < 0 || (n_contigs > 0 && (!seqs || !lens))) { if (c) c->err = "pga_batch_create: bad arguments"; return PGA_EINVAL; }
    if (!c->finder) { int rc = pga_finder_models_changed(c); if (rc) return rc; }
    HT(c, hipSetDevice(c->device));
    pga_batch* b = new (std::nothrow) pga_batch();
    if (!b) return PGA_ENOMEM;
    b->ctx = c; b->n = n_contigs; b->d_seq = nullptr; b->d_tiles = nullptr; b->d_tile0 = nullptr; b->n_tiles = 0; b->ct.resize((size_t)n_contigs + 1);
    int64_t total = 0;
    for (int i = 0; i < n_contigs; i++) {
        if (lens[i] < 0 || lens[i] > 0x7fff0000LL || (lens[i] > 0 && !seqs[i])) { delete b; c->err = "pga_batch_create: bad contig length"; return PGA_EINVAL; }
        b->ct[i].base = total; b->ct[i].len = (int32_t)lens[i]; b->ct[i]._pad = 0;
        total += lens[i];
    }
    b->ct[n_contigs].base = total; b->ct[n_contigs].len = 0; b->ct[n_contigs]._pad = 0;
    b->total = total;
    if (total >= 0x7fffffffLL) { delete b; c->err = "pga_batch_create: batch larger than 2^31 bases; split it"; return PGA_EINVAL; }
    if (total > 0) {
        std::lock_guard<std::mutex> up(c->finder->up_mu);          // one upload at a time per context; a call of the context may run beside it
        hipStream_t st = nullptr; char* h_seq = nullptr;
        { const int rc = upload_resources(c, (size_t)total + 16, &st, &h_seq); if (rc) { delete b; return rc; } }
        std::vector<TileDesc> tiles; std::vector<int32_t> tile0;
        batch_tiles(b, tiles, tile0);
        if (batch_take_dev(c, (size_t)total + 16 + batch_tiles_bytes(tiles, tile0), &b->d_seq, &b->d_seq_cap) != hipSuccess) { delete b; c->err = "pga_batch_create: hipMalloc failed"; return PGA_ENOMEM; }
        // Packing is a host memcpy per contig and the upload a DMA from the pinned copy: the contigs are cut into slices of about
        // 8 MB, a few host threads pack slices, and each slice goes on its way to the device as soon as it is packed -- the DMA of
        // slice k runs under the packing of the slices after it (it was: one thread packing everything, then one DMA, 12 + 3 ms
        // per 125 Mbp).
        std::vector<int> cut{0};
        { int64_t acc = 0; for (int i = 0; i < n_contigs; i++) { acc += lens[i]; if (acc >= (8 << 20)) { cut.push_back(i + 1); acc = 0; } } }
        if (cut.back() != n_contigs) cut.push_back(n_contigs);
        const int n_slices = (int)cut.size() - 1;
        std::atomic<int> next{0};
        std::atomic<int> first_err{(int)hipSuccess};
        const int dev = c->device;
        char* d_seq = b->d_seq;
        const ContigDesc* ct = b->ct.data();
        std::mutex issue_mu;
        auto work = [&]() {
            (void)hipSetDevice(dev);
            for (;;) {
                const int k = next.fetch_add(1);
                if (k >= n_slices) return;
                for (int i = cut[k]; i < cut[k + 1]; i++) if (lens[i] > 0) memcpy(h_seq + ct[i].base, seqs[i], (size_t)lens[i]);
                const int64_t lo = ct[cut[k]].base, hi = ct[cut[k + 1]].base;
                if (hi > lo) {
                    std::lock_guard<std::mutex> g(issue_mu);
                    const hipError_t e = hipMemcpyAsync(d_seq + lo, h_seq + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, st);
                    if (e != hipSuccess) { int z = (int)hipSuccess; first_err.compare_exchange_strong(z, (int)e); }
                }
            }
        };
        const int threads = n_slices >= 2 ? std::min(n_slices, 6) : 1;
        hipError_t e;
        {
            // One upload at a time per process: several contexts that start their calls together (a job dealt to eight contexts) would
            // otherwise share the host's memory bandwidth and the PCIe link eight ways, every batch would arrive late, and the device
            // would idle until the first one is complete.  In turn, the first batch is on the device after one eighth of that time and
            // the uploads of the others run under its kernels.  (PGA_UPLOAD_TURNS=0: no turns.)
            static std::mutex upload_turns[64];        // one per device: only contexts that share a link take turns
            const bool turns = pga_knobs::process_knobs().upload_turns;
            std::unique_lock<std::mutex> turn(upload_turns[c->device & 63], std::defer_lock);
            if (turns && total >= (8 << 20)) turn.lock();
            if (threads == 1) work(); else c->finder->up_pool.run(work, threads);
            e = (hipError_t)first_err.load();
            if (e == hipSuccess) e = batch_upload_tiles(b, b->d_seq + total + 16, tiles, tile0, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
        if (e != hipSuccess) { batch_give_dev(c, b->d_seq, b->d_seq_cap); delete b; return pga_hip_try_(c, e, "upload of the batch"); }
    }
    *out = b;
    return PGA_OK;
}

extern "C" int pga_batch_create_packed(pga_ctx* c, int32_t n_contigs, const char* packed, const int64_t* offs, const int64_t* lens, pga_batch** out) {
    if (out) *out = nullptr;
    if (!c || !out || n_contigs < 0 || (n_contigs > 0 && (!packed || !offs || !lens))) { if (c) c->err = "pga_batch_create_packed: bad arguments"; return PGA_EINVAL; }
    for (int i = 0; i < n_contigs; i++) {
        if (lens[i] < 0 || lens[i] > 0x7fff0000LL || offs[i] != offs[0] + (i ? offs[i - 1] - offs[0] + lens[i - 1] : 0)) {
            c->err = "pga_batch_create_packed: contigs must lie back to back"; return PGA_EINVAL;
        }
    }
    if (!c->finder) { int rc = pga_finder_models_changed(c); if (rc) return rc; }
    HT(c, hipSetDevice(c->device));
    pga_batch* b = new (std::nothrow) pga_batch();
    if (!b) return PGA_ENOMEM;
    b->ctx = c; b->n = n_contigs; b->d_seq = nullptr; b->d_tiles = nullptr; b->d_tile0 = nullptr; b->n_tiles = 0; b->ct.resize((size_t)n_contigs + 1);
    int64_t total = 0;
    for (int i = 0; i < n_contigs; i++) { b->ct[i].base = total; b->ct[i].len = (int32_t)lens[i]; b->ct[i]._pad = 0; total += lens[i]; }
    b->ct[n_contigs].base = total; b->ct[n_contigs].len = 0; b->ct[n_contigs]._pad = 0;
    b->total = total;
    if (total >= 0x7fffffffLL) { delete b; c->err = "pga_batch_create_packed: batch larger than 2^31 bases; split it"; return PGA_EINVAL; }
    if (total > 0) {
        std::vector<TileDesc> tiles; std::vector<int32_t> tile0;
        batch_tiles(b, tiles, tile0);
        if (batch_take_dev(c, (size_t)total + 16 + batch_tiles_bytes(tiles, tile0), &b->d_seq, &b->d_seq_cap) != hipSuccess) { delete b; c->err = "pga_batch_create_packed: hipMalloc failed"; return PGA_ENOMEM; }
        // the letters go straight from the caller's (pinned) buffer: one DMA, overlapped with the tile list's host work
        std::lock_guard<std::mutex> up(c->finder->up_mu);
        hipStream_t st = nullptr;
        { const int rc = upload_resources(c, 0, &st, nullptr); if (rc) { batch_give_dev(c, b->d_seq, b->d_seq_cap); delete b; return rc; } }
        hipError_t e = hipMemcpyAsync(b->d_seq, packed + offs[0], (size_t)total, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = batch_upload_tiles(b, b->d_seq + total + 16, tiles, tile0, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { batch_give_dev(c, b->d_seq, b->d_seq_cap); delete b; return pga_hip_try_(c, e, "upload of the packed batch"); }
    }
    *out = b;
    return PGA_OK;
}

// what translate.hip needs of a batch
struct pga_batch_view { pga_ctx* ctx; int32_t n; int64_t total; const ContigDesc* ct; const char* d_seq; const uint8_t* circular /* or nullptr: all linear */; };
pga_batch_view pga_batch_peek(const pga_batch* b) { return pga_batch_view{b->ctx, b->n, b->total, b->ct.data(), b->d_seq, b->circular.empty() ? nullptr : b->circular.data()}; }

extern "C" void pga_batch_free(pga_batch* b) {
    if (!b) return;
    if (b->d_seq) { hipSetDevice(b->ctx->device); batch_give_dev(b->ctx, b->d_seq, b->d_seq_cap); }
    if (b->d_regions) { hipSetDevice(b->ctx->device); hipFree(b->d_regions); }
    delete b;
}

// the intervals of a batch, already checked, go to the device (or leave it: none)
static int batch_upload_regions(pga_ctx* c, pga_batch* b) {
    HT(c, hipSetDevice(c->device));
    if (b->d_regions) { HT(c, hipFree(b->d_regions)); b->d_regions = nullptr; }
    if (b->regions.empty()) return PGA_OK;
    HT(c, hipMalloc((void**)&b->d_regions, sizeof(MaskRun) * b->regions.size()));
    HT(c, hipMemcpy(b->d_regions, b->regions.data(), sizeof(MaskRun) * b->regions.size(), hipMemcpyHostToDevice));
    return PGA_OK;
}

extern "C" int pga_batch_set_regions(pga_batch* b, const int32_t* off, const int32_t* iv) {
    if (!b) return PGA_EINVAL;
    pga_ctx* c = b->ctx;
    if ((off == nullptr) != (iv == nullptr)) { c->err = "pga_batch_set_regions: offsets and intervals go together"; return PGA_EINVAL; }
    std::vector<int32_t> reg_off; std::vector<MaskRun> regions;
    if (off) {
        for (int i = 0; i < b->n; i++) {
            if (off[i] < 0 || off[i + 1] < off[i]) { c->err = "pga_batch_set_regions: offsets must not decrease"; return PGA_EINVAL; }
            for (int32_t k = off[i]; k < off[i + 1]; k++) {
                const int32_t begin = iv[2 * (size_t)k], end = iv[2 * (size_t)k + 1];
                if (!(0 <= begin && begin < end && end <= b->ct[i].len)) {          // 0 <= begin < end <= len
                    c->err = "pga_batch_set_regions: sequence " + std::to_string(i) + ": interval [" + std::to_string(begin) + ", " + std::to_string(end) +
                             ") is not a non-empty part of [0, " + std::to_string(b->ct[i].len) + ")";
                    return PGA_EINVAL;
                }
                regions.push_back(MaskRun{i, begin, end, 0});
            }
        }
        if (!regions.empty()) { reg_off.resize((size_t)b->n + 1); for (int i = 0; i <= b->n; i++) reg_off[i] = off[i] - off[0]; }
    }
    b->reg_off.swap(reg_off); b->regions.swap(regions);
    return batch_upload_regions(c, b);
}

extern "C" int pga_batch_set_mask_case(pga_batch* b, int lower_case) {
    if (!b) return PGA_EINVAL;
    b->mask_case = lower_case != 0;
    return PGA_OK;
}

extern "C" int pga_find_genes_batch(pga_ctx* c, int32_t n_contigs, const char* const* seqs, const int64_t* lens,
                                    const pga_params* pp, pga_result** out) {
    if (out) *out = nullptr;
    pga_batch* b = nullptr;
    int rc = pga_batch_create(c, n_contigs, seqs, lens, &b);
    if (rc != PGA_OK) return rc;
    rc = pga_find_genes(c, b, pp, out);
    pga_batch_free(b);
    return rc;
}

extern "C" void pga_result_free(pga_result* r) {
    if (r) delete reinterpret_cast<ResultOwner*>(r);
}

// hand the result over to the caller
static int publish(ResultOwner* R, ResultOwner*& guarded, const pga_params& P, pga_result** out) {
    R->pub.contigs = R->contigs.data();
    R->pub.genes = R->pin_genes != nullptr ? R->pin_genes : R->genes.data();
    R->pub.n_genes = (int64_t)(R->pin_genes != nullptr ? R->pin_n : R->genes.size());
    R->pub.nodes = !R->nodes.empty() ? R->nodes.data() : nullptr;
    R->pub.mask_off = R->has_masks ? R->mask_off.data() : nullptr;
    R->pub.masks = R->has_masks ? R->masks.data() : nullptr;
    guarded = nullptr;
    *out = &R->pub;
    return PGA_OK;
}

// the merged mask list of a call for pga_result.masks: its offsets have arrived with the stream's last synchronisation, the intervals
// are fetched now that their number is known (the kernels that read them are already queued or done)
static int fetch_mask_union(pga_ctx* c, ResultOwner* R, const int32_t* h_moff, const int2* d_iv, int n_contigs) {
    R->mask_off.assign(h_moff, h_moff + n_contigs + 1);
    const size_t n = (size_t)std::max(h_moff[n_contigs], 0);
    R->masks.resize(2 * n);
    if (n > 0) HT(c, hipMemcpy(R->masks.data(), d_iv, sizeof(int2) * n, hipMemcpyDeviceToHost));
    return PGA_OK;
}

// where a pass of a circular call (circular.inl) leaves its gene records on the device: find_impl's `keep`
struct GeneKeep { const char* buf; pga_gene* d_genes = nullptr; int64_t n_genes = 0; };
namespace {

// a per-group device buffer: `base` with the group's number behind it
int group_dev(pga_ctx* c, const char* base, const int g, const size_t bytes, void** out, const bool fp = false) {
    char nm[32];
    snprintf(nm, sizeof nm, "%s%d", base, g);
    return ensure_dev(c, nm, bytes, out, fp);
}
#define GROUPBUF(dst, ptr_type, base, bytes, fp) { void* p__; int rc__ = group_dev(c, base, g, bytes, &p__, fp); if (rc__) return rc__; dst = (ptr_type)p__; }
#define GBUF(field, type, count) GROUPBUF(ga[g].field, type*, #field, sizeof(type) * (size_t)(count) + 64, std::is_floating_point<type>::value)

struct TailBufs;
// the per-tile counts and offsets of one group's extraction (nodes, stop nodes)
struct GroupTiles { int32_t* count; int32_t* off; int32_t* scount; int32_t* soff; };

// The state of one finder call: what more than one phase of find_impl reads.  The phases are its member functions, called in order;
// what only one phase needs is a local of that phase.  The vectors that uploads on the stream read live here, so they outlive it.
struct FindCall : pga_plan::ChainPlan, pga_plan::RescorePlan, pga_plan::GatherPlan<WinDesc> {
    // ---- inputs and mode flags (check_call)
    Knobs kn{};             // the run-time knobs as the entry point read them: one reading for every phase
    pga_ctx* c = nullptr; FinderState* f = nullptr; hipStream_t st = nullptr;
    const pga_batch* batch = nullptr; pga_params P{};
    int stage = 0, tt_override = 0;
    const int32_t* model_of_contig = nullptr; const int32_t* tt_of_contig = nullptr; int64_t* coding = nullptr; GeneKeep* keep = nullptr;
    bool meta_run = false, use_sets = false, per_contig = false, multi = false, mask_union = false;
    int NC = 0, NM = 0, NG = 0, NS = 0; int64_t total = 0;
    std::vector<int> cgrp, gtt;             // a translation-table group per contig, the table of every group (multi)
    std::vector<int32_t> set_of;            // contig sets: dense ids
    ResultOwner* R = nullptr;               // the call's until publish_result hands it over
    StageTimer* tm = nullptr;
    // ---- sequence, masks, extraction: device views and what the extraction read back
    uint8_t* d_dig = nullptr; ContigDesc* d_ct = nullptr; int32_t* d_p16 = nullptr;
    int32_t* d_xa = nullptr; int32_t* h_xa = nullptr; size_t xa_words = 0;
    int32_t* d_cnt = nullptr; int32_t* h_cnt = nullptr; int32_t* d_cbase = nullptr; int32_t* h_cbase = nullptr;
    int32_t* d_sbase = nullptr; int32_t* h_sbase = nullptr; uint8_t* d_enabled = nullptr; uint8_t* h_enabled = nullptr;
    int32_t* d_tile_first = nullptr; int32_t* d_tile_last = nullptr; GroupTiles d_tile{};
    GroupArrays ga[4];
    MaskList masks{nullptr, nullptr}; int32_t* h_moff = nullptr; const int2* d_union_iv = nullptr;
    int64_t group_nodes[4] = {0, 0, 0, 0};
    // ---- the plan of the connection scoring (the chains themselves: ChainPlan)
    int NCH = 0;
    bool use_wave = false, seg_wave = false, wave_prep = false, use_sched = false, segmented = false, lean_gather = false, direct_gather = false;
    DpSegPlan seg_plan; DpSegDev seg_dev{}; int64_t dp_slots = 0;
    std::vector<int32_t> h_bbase, dp_order;
    int max_batches[4] = {0, 0, 0, 0};
    ChainArrays ca{}; DpBuffers dp{}; DpwGroupPtrs wgroups{}; DpwBuffers wbuf{};
    double* h_maxscore = nullptr; int32_t* h_maxidx = nullptr; int32_t* h_ipath = nullptr; uint32_t* h_scur = nullptr;
    // ---- the call plan on the device (upload_plan) and its pinned mirror
    std::vector<int64_t> ovl_blk0;
    uint8_t* d_conv = nullptr; uint8_t* h_conv = nullptr; int2* d_cc = nullptr; int2* h_cc = nullptr; int32_t* d_bbase = nullptr;
    int32_t* d_dp_order = nullptr; ChainDesc* d_chains = nullptr; const int32_t* d_ovl_blk = nullptr;
    // ---- scoring
    std::vector<int32_t> cs_tk[4], cs_en[4];    // alive until the stream is synchronized
    ScoreParams sp{};
    // ---- winners (their plans: RescorePlan, GatherPlan), the gathered arena and its pinned mirror, the tail
    std::vector<int> win_chain;
    OutArrays o{}, h{}; size_t arena_dp = 0, arena_all = 0; int max_n = 0;      // max_n: nodes of the longest winner
    std::vector<int32_t> tracef; std::vector<uint8_t> elim;
    std::vector<TailDesc> tdv; std::vector<TpSeg> segs;

    ~FindCall() { delete R; }

    // group g's node and stop-node offsets per contig (NC + 1 entries), on the host and on the device
    const int32_t* h_cb(const int g) const { return h_cbase + (size_t)g * (NC + 1); }
    const int32_t* h_sb(const int g) const { return h_sbase + (size_t)g * (NC + 1); }
    int32_t* d_cb(const int g) const { return d_cbase + (size_t)g * (NC + 1); }
    int32_t* d_sb(const int g) const { return d_sbase + (size_t)g * (NC + 1); }
    int contig_nodes(const int g, const int i) const { return h_cb(g)[i + 1] - h_cb(g)[i]; }
    int group_stops(const int g) const { return h_sb(g)[NC]; }
    GroupTiles tiles(const int g) const {
        const size_t at = (size_t)g * (batch->n_tiles + 1);
        return GroupTiles{d_tile.count + at, d_tile.off + at, d_tile.scount + at, d_tile.soff + at};
    }
    // what the three scoring launchers share for `n_chains` chains of group g (pipeline.h)
    ScoreGroup score_group(const int g, const ChainDesc* d_first, const int n_chains, const int64_t node_begin, const int64_t n_nodes, const int2* d_contig_chains) const {
        ScoreGroup s;
        s.d_chains = d_first; s.n_chains = n_chains; s.node_begin = node_begin; s.total = n_nodes;
        s.d_all_chains = d_chains; s.d_contig_chains = d_contig_chains; s.d_node_contig_base = d_cb(g); s.n_contigs = NC; s.group_nodes = (int)group_nodes[g];
        s.d_dig = d_dig; s.d_ct = d_ct; s.ga = &ga[g]; s.ca = &ca; s.d_models = (const pga_training*)c->d_models_raw; s.st = st;
        return s;
    }
    // does group g have chains, and nodes in them?
    bool group_has_work(const int g) const { return g_c0[g + 1] > g_c0[g] && g_n0[g + 1] > g_n0[g]; }

    void contig_counts() {      // the contigs' GC content and unknown bases into the result
        for (int i = 0; i < NC; i++) { R->contigs[i].gc = batch->ct[i].len > 0 ? (double)h_cnt[i] / (double)batch->ct[i].len : 0.0; R->contigs[i].n_unknown = h_cnt[NC + i]; }
    }
    int sync() { HT(c, hipGetLastError()); HT(c, hipStreamSynchronize(st)); return PGA_OK; }      // what the launches left, then the stream
    int stop_clock() {       // the call's device time: e_start (run_sequence_and_masks) to here, waited for
        HT(c, hipEventRecord(f->e_stop, st));
        if (const int rc = sync()) return rc;
        float ms = 0; HT(c, hipEventElapsedTime(&ms, f->e_start, f->e_stop)); R->pub.t_total_ms = ms;
        return PGA_OK;
    }
    int publish_result(pga_result** out) { ResultOwner* const r = R; return publish(r, R, P, out); }

    // the phases, in the order find_impl calls them
    int check_call(const Knobs& kn_, pga_ctx* c_, const pga_batch* batch_, const pga_params* pp, pga_result** out);
    int run_sequence_and_masks(); int return_sequence_stage(pga_result** out); int run_extract(); int place_nodes(); int plan_chains();
    int plan_connection_scoring(); int prepare_wave(int64_t dp_cap); void order_starts(); int upload_plan(); int score_groups();
    int return_stage_nodes(pga_result** out); int score_connections(); void pick_winners(); int rescore_winners(); int gather_winners();
    int64_t contig_results(const int32_t* n_genes, int64_t* gene_begin);
    int run_host_tail(); int run_device_tail(bool par_tail); int launch_tail_paths(const TailBufs& t); int launch_tail_tweaks(TailBufs& t);
    int copy_out_nodes(); void keep_device_nodes();
};

// the argument checks, the translation-table groups, the dense set ids, the result
int FindCall::check_call(const Knobs& kn_, pga_ctx* c_, const pga_batch* batch_, const pga_params* pp, pga_result** out) {
    kn = kn_; c = c_; batch = batch_;
    if (out) *out = nullptr;
    if (c) c->dev_nodes.clear();        // this call reuses the arena the last one kept on the device
    if (!c || !out || !pp || !batch || batch->ctx != c) {
        if (c) c->err = "pga_find_genes: bad arguments";
        return PGA_EINVAL;
    }
    if (!c->finder) { int rc0 = pga_finder_models_changed(c); if (rc0) return rc0; }
    meta_run = pp->meta && stage == 0;
    use_sets = meta_run && !batch->sets.empty();      // one GC window and one model per set of contigs
    per_contig = model_of_contig != nullptr && !pp->meta && stage != PGA_STAGE_EXTRACT && stage != PGA_STAGE_SEQUENCE;
    const bool per_contig_tt = tt_of_contig != nullptr && stage == PGA_STAGE_EXTRACT;
    // meta mode over an empty bin collection is legal and finds nothing (ref: tests/test_gene_finder.py:316-324)
    if (c->n_models <= 0 && !meta_run && stage != PGA_STAGE_EXTRACT && stage != PGA_STAGE_SEQUENCE) { c->err = "pga_find_genes: no model loaded (call pga_set_models first)"; return PGA_EINVAL; }
    P = *pp;
    // the caller's intervals and runs of lower-case letters (pga_batch_set_regions / _set_mask_case) join the runs of unknown bases
    mask_union = batch->mask_case != 0 || !batch->regions.empty();
    if ((P.mask || batch->mask_case) && P.min_mask < 0) { c->err = "pga_find_genes: min_mask must be positive"; return PGA_EINVAL; }   // ref: lib.pyx:5175-5176
    if (!P.closed && P.min_edge_gene > 0 && P.min_edge_gene < 4) {
        // with open ends and min_edge_gene <= 3 the reference emits a start node AND the virtual edge stop node at the same
        // position and strand; the per-position node layout of this path holds one of them.  Nobody calls genes of one codon.
        c->err = "pga_find_genes: min_edge_gene below 4 is not supported with open ends";
        return PGA_EINVAL;
    }
    if (P.min_gene <= 0 || P.min_edge_gene <= 0 || P.max_overlap < 0 || P.max_overlap > P.min_gene) {
        c->err = "pga_find_genes: invalid min_gene / min_edge_gene / max_overlap";   // ref: lib.pyx:5169-5181
        return PGA_EINVAL;
    }
    HT(c, hipSetDevice(c->device));
    f = c->finder;
    st = c->stream;
    NC = batch->n;
    // a translation-table group per contig (per_contig: its model's group; per_contig_tt: a group per distinct table of the call)
    multi = per_contig || per_contig_tt;
    if (per_contig) {
        gtt = f->group_tt;
        for (int i = 0; i < NC; i++) cgrp.push_back(f->model_group[model_of_contig[i]]);
    } else if (per_contig_tt) {
        for (int i = 0; i < NC; i++) {
            int g = (int)(std::find(gtt.begin(), gtt.end(), tt_of_contig[i]) - gtt.begin());
            if (g == (int)gtt.size()) gtt.push_back(tt_of_contig[i]);
            cgrp.push_back(g);
        }
    }
    NM = c->n_models; NG = meta_run ? (int)f->group_tt.size() : (multi ? std::max(1, (int)gtt.size()) : 1);
    if (NG > 4) { c->err = "pga_find_genes: more than 4 distinct translation tables loaded"; return PGA_EINVAL; }
    if (kn.fault_contig_len_set) {
        // diagnostics: a call that carries a contig of exactly this many bases fails (the host layer's error paths under test)
        const long fl = kn.fault_contig_len;
        for (int i = 0; i < NC; i++) if ((long)batch->ct[i].len == fl) { c->err = "pga_find_genes: fault injected by PGA_FAULT_CONTIG_LEN"; return PGA_EDEVICE; }
    }
    if (use_sets) {
        NS = pga_plan::dense_set_ids(batch->sets.data(), NC, set_of);
        c->set_model.assign((size_t)NC, -1);
        c->set_score.assign((size_t)NC, std::numeric_limits<double>::quiet_NaN());
        c->model_scores.assign((size_t)NC * (size_t)NM, std::numeric_limits<double>::quiet_NaN());
        c->model_scores_nm = NM;
    }
    R = new (std::nothrow) ResultOwner();
    if (!R) return PGA_ENOMEM;
    R->contigs.assign(NC, pga_contig_result{-1, 0, 0, 0, 0, 0.0, 0.0});
    R->mask_off.assign(NC + 1, 0);
    R->has_masks = P.mask || mask_union;
    memset(&R->pub, 0, sizeof R->pub);
    R->pub.n_contigs = NC;
    total = batch->total;
    return PGA_OK;
}

// digitize, the GC prefix, and both mask paths
int FindCall::run_sequence_and_masks() {
    const char* d_seq = batch->d_seq;
    DEVSET(d_dig, uint8_t, "d_dig", total + 16);
    DEVSET(d_ct, ContigDesc, "d_ct", NC + 1);
    // What the host reads back after the extraction -- the staging-overflow flag, the contigs' GC / unknown counts, the node and stop-node
    // offsets of every group, the groups a contig is extracted under -- sits in ONE device allocation and ONE pinned one with the same
    // layout: one read-back instead of five, one memset instead of two (round 6: a lone 20 kbp call was 56 launches, 31 of them the
    // runtime's own copy and fill kernels).  Word 0 is the overflow flag.
    const size_t xa_cnt = 4, xa_cbase = xa_cnt + 2 * (size_t)NC, xa_sbase = xa_cbase + (size_t)NG * (NC + 1), xa_en = xa_sbase + (size_t)NG * (NC + 1);
    xa_words = xa_en + ((size_t)NG * NC + 3) / 4 + 1;
    DEVSET(d_xa, int32_t, "d_extract_info", xa_words);
    PINSET(h_xa, int32_t, "h_extract_info", xa_words);
    d_cnt = d_xa + xa_cnt; h_cnt = h_xa + xa_cnt;
    const int64_t gc_blocks = pga_gc_blocks(total);
    DEVSET(d_p16, int32_t, "d_gc_p16", total / 16 + 2);
    DEVBUF(d_gc_bsum, int32_t, "d_gc_bsum", gc_blocks + 1);
    DEVBUF(d_gc_boff, int32_t, "d_gc_boff", gc_blocks + 1);
    d_cbase = d_xa + xa_cbase; h_cbase = h_xa + xa_cbase;
    DEVSET(d_tile_first, int32_t, "d_tile_first", (size_t)6 * batch->n_tiles);
    DEVSET(d_tile_last, int32_t, "d_tile_last", (size_t)6 * batch->n_tiles);
    DEVSET(d_tile.count, int32_t, "d_tile_count", (size_t)NG * (batch->n_tiles + 1));
    DEVSET(d_tile.off, int32_t, "d_tile_off", (size_t)NG * (batch->n_tiles + 1));
    DEVSET(d_tile.scount, int32_t, "d_tile_scount", (size_t)NG * (batch->n_tiles + 1));
    DEVSET(d_tile.soff, int32_t, "d_tile_soff", (size_t)NG * (batch->n_tiles + 1));
    d_sbase = d_xa + xa_sbase; h_sbase = h_xa + xa_sbase;
    d_enabled = (uint8_t*)(d_xa + xa_en); h_enabled = (uint8_t*)(h_xa + xa_en);

    for (int g = 0; g < NG; g++) {
        GBUF(df, uint8_t, total + 16)
        GBUF(c16, int32_t, (size_t)batch->n_tiles * 192 + 2)
        ga[g].tile0 = batch->d_tile0;
        ga[g].ndx = nullptr; ga[g].stop_val = nullptr; ga[g].type = nullptr; ga[g].strand = nullptr; ga[g].edge0 = nullptr; ga[g].gc_cont = nullptr;
    }

    HT(c, hipEventRecord(f->e_start, st));
    HT(c, hipMemcpyAsync(d_ct, batch->ct.data(), sizeof(ContigDesc) * (NC + 1), hipMemcpyHostToDevice, st));
    HT(c, hipMemsetAsync(d_xa, 0, sizeof(int32_t) * xa_cbase, st));          // the overflow flag and the counts
    pga_launch_digitize(d_seq, d_dig, total, d_ct, NC, d_cnt, d_cnt + NC, st);
    pga_launch_gc_prefix(d_dig, total, d_gc_bsum, d_gc_boff, d_p16, st);
    if (mask_union) {
        // Several sources: their union per contig is built on the device (pga_launch_mask_union) and the extraction is launched behind
        // it without a word from the host.  The list comes back for pga_result.masks with the extraction's own read-back.
        const int64_t per_source = total / std::max(1, P.min_mask) + NC + 1;       // qualifying runs of one kind
        const int64_t most = std::min<int64_t>((P.mask ? per_source : 0) + (batch->mask_case ? per_source : 0) + (int64_t)batch->regions.size(),
                                               total / 2 + NC + 1);               // disjoint runs that do not touch
        const int cap = (int)std::min<int64_t>(most, (int64_t)1 << 28);
        DEVBUF(d_bits, uint32_t, "d_mask_bits", 2 * pga_mask_words(total) + 2);
        DEVBUF(d_mcounts, int32_t, "d_mask_counts", 4 * (pga_mask_waves(total) + 1));
        DEVBUF(d_moff, int32_t, "d_mask_off", NC + 2);
        DEVBUF(d_miv, int2, "d_mask_iv", cap + 1);
        PINBUF(h_moff_, int32_t, "h_mask_off", NC + 2);
        pga_launch_mask_union(d_dig, d_seq, total, d_ct, NC, batch->d_tiles, batch->n_tiles, P.mask, batch->mask_case, P.min_mask, batch->d_regions,
                              (int)batch->regions.size(), d_bits, d_mcounts, d_moff, d_miv, cap, st);
        HT(c, hipMemcpyAsync(h_moff_, d_moff, sizeof(int32_t) * (NC + 1), hipMemcpyDeviceToHost, st));
        h_moff = h_moff_; d_union_iv = d_miv;
        masks = MaskList{d_moff, d_miv};
    } else if (P.mask) {
        // masked regions: found on the device, ordered on the host (a handful of intervals)
        const int cap = (int)std::min<int64_t>(total / std::max(1, P.min_mask) + NC + 1, (int64_t)1 << 28);
        DEVBUF(d_runs, MaskRun, "d_mask_runs", cap + 1);
        DEVBUF(d_nruns, int32_t, "d_mask_count", 4);
        DEVBUF(d_moff, int32_t, "d_mask_off", NC + 2);
        DEVBUF(d_miv, int2, "d_mask_iv", cap + 1);
        pga_launch_find_masks(d_dig, d_ct, NC, batch->d_tiles, batch->n_tiles, P.min_mask, d_runs, d_nruns, cap, st);
        int32_t nruns = 0;
        HT(c, hipMemcpyAsync(&nruns, d_nruns, 4, hipMemcpyDeviceToHost, st));
        HT(c, hipStreamSynchronize(st));
        nruns = std::min(nruns, cap);
        std::vector<MaskRun> runs((size_t)nruns);
        if (nruns > 0) HT(c, hipMemcpy(runs.data(), d_runs, sizeof(MaskRun) * nruns, hipMemcpyDeviceToHost));
        std::sort(runs.begin(), runs.end(), [](const MaskRun& a, const MaskRun& b) { return a.contig != b.contig ? a.contig < b.contig : a.begin < b.begin; });
        std::vector<int32_t> moff(NC + 1, 0);
        std::vector<int2> miv((size_t)nruns + 1);
        for (int k = 0; k < nruns; k++) { moff[runs[k].contig + 1]++; miv[k] = make_int2(runs[k].begin, runs[k].end); }
        for (int i = 0; i < NC; i++) moff[i + 1] += moff[i];
        R->mask_off = moff;
        R->masks.resize(2 * (size_t)nruns);
        for (int k = 0; k < nruns; k++) { R->masks[2 * k] = runs[k].begin; R->masks[2 * k + 1] = runs[k].end; }
        HT(c, hipMemcpy(d_moff, moff.data(), sizeof(int32_t) * (NC + 1), hipMemcpyHostToDevice));
        if (nruns > 0) HT(c, hipMemcpy(d_miv, miv.data(), sizeof(int2) * nruns, hipMemcpyHostToDevice));
        masks = MaskList{d_moff, d_miv};
    }
    return PGA_OK;
}

// PGA_STAGE_SEQUENCE: the contigs' GC and unknown counts (and the masks), and stop
int FindCall::return_sequence_stage(pga_result** out) {
    HT(c, hipMemcpyAsync(h_cnt, d_cnt, sizeof(int32_t) * 2 * (size_t)NC, hipMemcpyDeviceToHost, st));
    if (const int rc = sync()) return rc;
    contig_counts();
    if (h_moff) { const int rc = fetch_mask_union(c, R, h_moff, d_union_iv, NC); if (rc) return rc; }
    return publish_result(out);
}

// the group-enable launch and the extraction loop with its staging and pool retries
int FindCall::run_extract() {
    // meta mode: a contig is extracted under a translation table only if a model with that table lies in its GC window
    // (contig sets: in its SET's window -- the labels go up, two integers per set are summed on the device)
    if (meta_run && NM > 0 && use_sets) {
        DEVBUF(d_set_of, int32_t, "d_set_of", 3 * (size_t)NC + 1);      // the dense ids, then the pooled (G+C count, length) pairs
        HT(c, hipMemcpyAsync(d_set_of, set_of.data(), sizeof(int32_t) * (size_t)NC, hipMemcpyHostToDevice, st));
        pga_launch_group_enable_sets(d_ct, NC, d_cnt, d_set_of, d_set_of + NC, f->d_model_gc, f->d_model_grp, NM, NG, d_enabled, st);
    } else if (meta_run && NM > 0) {
        pga_launch_group_enable(d_ct, NC, d_cnt, f->d_model_gc, f->d_model_grp, NM, NG, d_enabled, st);
    }
    // per-contig models: a contig is extracted under its own model's translation table only
    if (multi) {
        for (int g = 0; g < NG; g++) for (int i = 0; i < NC; i++) h_enabled[(size_t)g * NC + i] = cgrp[i] == g;
        HT(c, hipMemcpyAsync(d_enabled, h_enabled, (size_t)NG * NC, hipMemcpyHostToDevice, st));
    }
    // Staging of the extraction: one slot per two positions of a tile (sequence has a node every 25 positions or so; the full
    // two-slots-per-position staging was half of a context's memory).  A tile that does not fit raises a flag, the batch is then
    // extracted again with full staging, and the context keeps that (PGA_STAGE_FULL=1: from the start).
    if (kn.stage_full) f->stage_full = true;
    bool stage_full = f->stage_full;
    // Stop values of the extraction: a thread of k_extract_tile lists up to four per strand in LDS and a pool of the workgroup takes the
    // rest; a tile that exhausts the pool (a full tile of (GT)n) raises bit 1 of the flag and the batch is extracted again with a
    // value for every position.  That choice is the batch's, the context does not keep it.  (PGA_EXTRACT_C=1 .. 4 / PGA_EXTRACT_POOL=
    // 0 .. 128: fewer list slots / pool entries, so that the tests reach the pool and the second pass on small inputs; PGA_EXTRACT_C=0:
    // a value for every position from the start)
    int ex_c = kn.extract_c;
    const int ex_pool = kn.extract_pool;
    int32_t* const d_st_overflow = d_xa; const int32_t* const h_st_overflow = h_xa;
    c->extract_passes = 0;
    for (;;) {
        const bool half = !stage_full;
        // (PGA_STAGE_SHIFT=5: one slot per 32 positions, so that ordinary sequence overflows and the tests see the second pass)
        const int shift = half ? kn.stage_shift : 0;
        const int64_t st_slots = half ? (total >> shift) + (int64_t)PGA_STAGE_SLACK * batch->n_tiles + 8 : 2 * total + 2;
        for (int g = 0; g < NG; g++) {
            GBUF(st_ndx, int32_t, st_slots) GBUF(st_sv, int32_t, st_slots) GBUF(st_info, uint8_t, st_slots)
            ga[g].st_half = shift; ga[g].st_overflow = d_st_overflow;
        }
        if (c->extract_passes > 0) HT(c, hipMemsetAsync(d_st_overflow, 0, sizeof(int32_t), st));      // (the first pass: cleared with the counts)
        for (int g = 0; g < NG; g++) {
            const int tt = meta_run ? f->group_tt[g] : multi ? gtt[g] : (stage == PGA_STAGE_EXTRACT ? tt_override : c->models[0].trans_table);
            const GroupTiles t = tiles(g);
            pga_launch_extract(d_dig, total, d_ct, NC, tt, P, ga[g], batch->d_tiles, batch->n_tiles, batch->d_tile0, d_tile_first, d_tile_last,
                               t.count, t.off, d_cb(g), t.scount, t.soff, d_sb(g),
                               masks, st, ((meta_run && NM > 0) || multi) ? d_enabled + (size_t)g * NC : nullptr, ex_c, ex_pool);
        }
        HT(c, hipMemcpyAsync(h_xa, d_xa, sizeof(int32_t) * xa_words, hipMemcpyDeviceToHost, st));      // flag, counts, offsets, enabled groups
        if (const int rc = sync()) return rc;
        c->extract_passes++;
        const bool staging_overflow = half && (h_st_overflow[0] & 1), pool_exhausted = ex_c > 0 && (h_st_overflow[0] & 2);
        if (!staging_overflow && !pool_exhausted) break;
        if (pool_exhausted) ex_c = 0;
        if (staging_overflow) {
            stage_full = true;
            if (!kn.stage_shift_set) f->stage_full = true;       // (the test knob leaves the context as it was)
        }
    }
    if (h_moff) { const int rc = fetch_mask_union(c, R, h_moff, d_union_iv, NC); if (rc) return rc; }
    return PGA_OK;
}

// ---- topology buffers; the nodes go to their places and get their GC content while the host plans the chains: neither kernel
//      reads anything of the plan (round 6: the device sat idle through the 0.7 ms of planning of a 6 250-contig call)
int FindCall::place_nodes() {
    for (int g = 0; g < NG; g++) {
        group_nodes[g] = h_cb(g)[NC];
        const int64_t n = group_nodes[g] + 1;
        GBUF(ndx, int32_t, n) GBUF(stop_val, int32_t, n) GBUF(type, uint8_t, n) GBUF(strand, int8_t, n) GBUF(edge0, uint8_t, n) GBUF(gc_cont, float, n) GBUF(contig_of, int32_t, n)
        GBUF(stop_list, int32_t, (int64_t)group_stops(g) + 1)
        GBUF(start_list, int32_t, group_nodes[g] - (int64_t)group_stops(g) + 1)
        GBUF(ovl_topo, uint32_t, (int64_t)group_stops(g) + 1)
        GBUF(srank, int32_t, n + 4)
    }
    for (int g = 0; g < NG; g++) {
        pga_launch_place(d_ct, batch->d_tiles, batch->n_tiles, tiles(g).off, tiles(g).soff, ga[g], st);
        pga_launch_orf_gc(d_ct, NC, d_dig, d_p16, ga[g], (int)group_nodes[g], d_cb(g), st);
    }
    return PGA_OK;
}

// ---- plan the (contig, model) chains (ref: lib.pyx:5335-5362; the arithmetic: find_plan.h) ------------------------
int FindCall::plan_chains() {
    std::vector<double> mgc((size_t)NM); std::vector<int> mtt((size_t)NM);     // the models are 558 KB apart: keep what the loop reads together
    for (int m = 0; m < NM; m++) { mgc[m] = c->models[m].gc; mtt[m] = c->models[m].trans_table; }
    contig_counts();
    const pga_plan::ChainPlanIn in{NC, NM, NG, meta_run, batch->ct.data(), h_cnt, h_cbase, h_sbase, h_enabled, mgc.data(), mtt.data(), f->model_group.data(),
                                   per_contig ? model_of_contig : nullptr, multi ? cgrp.data() : nullptr, use_sets ? set_of.data() : nullptr, NS};
    if (!pga_plan::plan_chains(in, *this)) { c->err = "pga_find_genes: host and device disagree on a GC window"; return PGA_EDEVICE; }
    NCH = (int)chains.size();
    R->pub.node_passes = tot_chain_nodes;
    R->pub.n_chains = NCH;
    return PGA_OK;
}

// the wave / segmented / schedule decisions, the chain, DP and wave buffers, the early topology launches, the start order
int FindCall::plan_connection_scoring() {
    // space for the fresh re-scores of winners that were not `first` (at most one per contig)
    int64_t max_rescore = 0;
    if (meta_run) for (int g = 0; g < NG; g++) max_rescore += h_cb(g)[NC];   // loose bound: every node once per group
    const int64_t chain_cap = tot_chain_nodes + max_rescore + 64;

    // ---- chain buffers ---------------------------------------------------------------------
    {
        DEVBUF(a0, double, "ca_cscore", chain_cap) DEVBUF(a1, double, "ca_sscore", chain_cap) DEVBUF(a2, double, "ca_rscore", chain_cap)
        DEVBUF(a3, double, "ca_uscore", chain_cap) DEVBUF(a4, double, "ca_tscore", chain_cap) DEVBUF(a5, double, "ca_mot_score", chain_cap)
        DEVBUF(a6, int32_t, "ca_star_ptr", 3 * chain_cap) DEVBUF(a7, int32_t, "ca_mot_ndx", chain_cap) DEVBUF(a8, uint8_t, "ca_rbs", 2 * chain_cap)
        DEVBUF(a9, uint8_t, "ca_edge", chain_cap) DEVBUF(a10, uint8_t, "ca_mot_len", chain_cap) DEVBUF(a11, uint8_t, "ca_mot_spacer", chain_cap)
        DEVBUF(a12, uint8_t, "ca_mot_spacendx", chain_cap)
        int64_t max_contig_nodes = 0;
        for (int g = 0; g < NG; g++) for (int i = 0; i < NC; i++) max_contig_nodes = std::max<int64_t>(max_contig_nodes, contig_nodes(g, i));
        DEVBUF(a13, double, "ca_cscore_raw", chain_cap + max_contig_nodes + 64)
        ca = ChainArrays{a0, a1, a2, a3, a4, a5, a13, a6, a7, a8, a9, a10, a11, a12, a13 + chain_cap};
    }
    // few long chains: their walks are cut into segments that run side by side (dp.hip "segmented chains": seg_plan)
    // many chains: one wavefront each, records and far-field structures of dp_wave.hip
    use_wave = stage == 0 && pga_dp_use_wave(kn, NCH);
    // Round 6 -- few LONG chains whose segments the wave-batch kernel walks (dp.hip, launch_dp_segmented): a wavefront per segment, 4096
    // segments at once where the chain kernel's workgroup per compute unit allows 252.  Every segment pays the same 4096-node warm-up and
    // a wavefront walks a node more slowly than the sixteen of a chain-kernel workgroup, so this pays where the chains are long enough --
    // from PGA_DP_SEG_WAVE_MIN (2.5 M) nodes in chains of 16 k nodes or more; PGA_DP_SEG_WAVE=1 / 0: always / never (tests).
    seg_wave = false;
    if (stage == 0 && !use_wave && kn.dpw_sched && !kn.dp_kernel_set) {
        int64_t cand = 0;
        for (int k = 0; k < NCH; k++) if (chains[(size_t)k].n >= kn.dp_seg_min) cand += chains[(size_t)k].n;
        seg_wave = kn.dp_seg_wave_set ? kn.dp_seg_wave : cand >= kn.dp_seg_wave_min;
    }
    // what the wave-batch kernel reads -- topology, step schedule, cs, extras -- is made for its own launches and for such segments
    wave_prep = use_wave || seg_wave;
    // the step schedule of the wave-batch scorer: one header per 64-node batch of every contig of a group (dpw_core.h)
    use_sched = wave_prep && kn.dpw_sched;
    if (use_sched) {
        h_bbase.resize((size_t)NG * (NC + 1));
        for (int g = 0; g < NG; g++) {
            int32_t* bb = h_bbase.data() + (size_t)g * (NC + 1);
            bb[0] = 0;
            for (int i = 0; i < NC; i++) bb[i + 1] = bb[i] + ((contig_nodes(g, i) + 63) >> 6);
        }
        for (ChainDesc& ch : chains) ch.sched_b0 = h_bbase[(size_t)ch.group * (NC + 1) + ch.contig];
    }
    if (use_sched) for (int g = 0; g < NG; g++) for (int i = 0; i < NC; i++)
        max_batches[g] = std::max(max_batches[g], h_bbase[(size_t)g * (NC + 1) + i + 1] - h_bbase[(size_t)g * (NC + 1) + i]);
    segmented = stage == 0 && !use_wave && pga_dp_plan(kn, chains.data(), NCH, tot_chain_nodes, seg_plan, seg_wave);
    if (seg_wave && !segmented) { seg_wave = false; wave_prep = use_wave; use_sched = false; h_bbase.clear(); }       // (nothing to cut after all)
    // lean: the tail runs on the device and nobody asked for node arrays, so only what the tail writes is gathered; direct: it
    // also reads the winners' node fields where the scorers left them.  (One definition: the scorers skip the star_ptr fill under
    // exactly the condition under which the tail never looks at it.)
    lean_gather = !P.want_nodes && kn.tail != Knobs::host && !kn.full_gather;
    direct_gather = lean_gather && !kn.gather_all_dp;
    const int64_t dp_cap = tot_chain_nodes + seg_plan.extra + 1;
    dp_slots = NCH + (int64_t)seg_plan.segs.size() + 1;
    // records and far-field arrays of the tree / chain kernels (sub-chains walked by the wave-batch kernel need none of their own)
    const int64_t tree_cap = use_wave ? 1 : (seg_wave ? tot_chain_nodes + 1 : dp_cap);
    {
        DEVBUF(b0, DpSrc, "dp_src", tree_cap) DEVBUF(b1, DpTgt, "dp_tgt", tree_cap)
        DEVBUF(b2, double, "dp_score", dp_cap) DEVBUF(b3, int32_t, "dp_traceb", dp_cap)
        DEVBUF(b4, int32_t, "dp_tbn", dp_cap) DEVBUF(b5, int8_t, "dp_ov", dp_cap)
        // (what the host reads back of a chain -- best gene end, its score, the path's start -- in one allocation: one read-back)
        DEVBUF(b7, double, "dp_chain_results", 2 * dp_slots + 2)
        int32_t* const b6 = (int32_t*)(b7 + dp_slots); int32_t* const b8 = b6 + dp_slots;
        DEVBUF(b9, double, "dp_A", tree_cap) DEVBUF(b10, double, "dp_V0", tree_cap) DEVBUF(b11, double, "dp_V1", tree_cap)
        DEVBUF(b12, double, "dp_V2", tree_cap) DEVBUF(b13, double, "dp_hv", tree_cap) DEVBUF(b14, int32_t, "dp_hi", tree_cap)
        dp = DpBuffers{b0, b1, b2, b3, b4, b5, b6, b7, b8, b9, {b10, b11, b12}, b13, b14, nullptr};
    }
    if (wave_prep) { const int rc = prepare_wave(dp_cap); if (rc) return rc; }
    if (segmented) {
        DEVBUF(seg_arena, char, "dp_seg_arena", pga_dp_seg_bytes(seg_plan, NCH, tot_chain_nodes));
        HT(c, pga_dp_seg_bind(seg_plan, NCH, tot_chain_nodes, seg_arena, st, &seg_dev));
        if (seg_wave) { seg_dev.wave_groups = &wgroups; seg_dev.wave_buf = &wbuf; }
    }
    order_starts();
    PINSET(h_maxscore, double, "h_chain_results", 2 * dp_slots + 2);
    h_maxidx = (int32_t*)(h_maxscore + dp_slots); h_ipath = h_maxidx + dp_slots;
    PINSET(h_scur, uint32_t, "h_dpw_scur", 16);
    return PGA_OK;
}

// the buffers of the wave-batch scorer and the topology of every group
int FindCall::prepare_wave(const int64_t dp_cap) {
    for (int g = 0; g < NG; g++) {
        const int64_t n = group_nodes[g] + 1;
#define WBUF(field, type) GROUPBUF(wgroups.g[g].field, type*, "dpw_" #field, sizeof(type) * (size_t)n + 64, std::is_floating_point<type>::value)
        WBUF(kf, uint8_t) WBUF(lo, int32_t) WBUF(q1, int32_t) WBUF(q2, int32_t)
#undef WBUF
        wgroups.g[g].ndx = ga[g].ndx; wgroups.g[g].stop_val = ga[g].stop_val; wgroups.g[g].srank = ga[g].srank;
        if (use_sched) {
            // headers: one per batch; lists: DPW_SCHED_STRIDE 32-byte slots per batch (what does not fit is counted and the launch
            // falls back to k_dpw_dyn)
            const int64_t nbat = h_bbase[(size_t)g * (NC + 1) + NC];
            GROUPBUF(wgroups.g[g].shdr, DpwSchedHdr*, "dpw_shdr", sizeof(DpwSchedHdr) * (size_t)(nbat + 1), false)
            GROUPBUF(wgroups.g[g].sent, uint4*, "dpw_sent", sizeof(DpwSlot) * (size_t)DPW_SCHED_STRIDE * (size_t)(nbat + 1) + 256, false)
            GROUPBUF(wgroups.g[g].scur, uint32_t*, "dpw_scur", 64, false)
        }
    }
    DEVBUF(w0, double, "dpw_cs", dp_cap + 2) DEVBUF(w1, DpwExt, "dpw_ext", tot_chain_stops + 4)      /* one extras record per (chain, stop node) pair */ DEVBUF(w2, double, "dpw_sfxv", dp_cap) DEVBUF(w3, int32_t, "dpw_sfxi", dp_cap)
    wbuf = DpwBuffers{w0, w1, w2, w3};
    // the topology of every group now: it reads the placed nodes and nothing of the plan, and runs under the rest of the planning
    // (start order, the copy of the plan, the coding-score tasks)
    for (int g = 0; g < NG; g++) {
        if (!group_has_work(g) || stage == PGA_STAGE_EXTRACT) continue;
        int max_nodes_g = 0;
        for (int i = 0; i < NC; i++) max_nodes_g = std::max(max_nodes_g, contig_nodes(g, i));
        if (g < 4) HT(c, hipEventRecord(f->e_aux[4 * g], st));
        pga_launch_dpw_topo(kn, wgroups.g[g], ga[g].type, ga[g].strand, d_cb(g), NC, (int)group_nodes[g], st, max_nodes_g);
        if (g < 4) HT(c, hipEventRecord(f->e_aux[4 * g + 1], st));
    }
    return PGA_OK;
}

// start order of the wave-batch scorer: longest chains first (counting sort on nodes / 64 = walk batches)
void FindCall::order_starts() {
    if (!(use_wave && NCH > 1 && !kn.dp_no_order)) return;
    std::vector<int32_t> lens((size_t)NCH);
    for (int k = 0; k < NCH; k++) lens[(size_t)k] = chains[k].n;
    dp_order.resize((size_t)NCH);
    pga_dp_start_order(NCH, lens.data(), dp_order.data());
    // Workgroups go to the eight XCDs in turn (b % 8), each with an L2 of its own, and the chains of a contig (one per model of
    // the same translation table) read the same topology arrays.  So every (contig, table) goes to ONE XCD -- the one with
    // the fewest nodes so far, in start order -- and workgroup 8 k + x takes the k-th chain of XCD x's queue; queues that end
    // early are filled up with -1 (the workgroup returns at once).  PGA_DP_XCD=0: the order as it is.
    // Only where the premise holds -- a device of eight XCDs (an MI355X in its default SPX mode; a partitioned one reports fewer) --
    // and where the queues come out even: a handful of keys, or one contig far longer than the rest, would leave XCDs idle
    // behind one long queue, and the plain longest-first order is the better one then.
    static std::atomic<int> xcc_of[64];      // per device: 0 = not asked yet
    int n_xcc = xcc_of[c->device & 63].load();
    if (n_xcc == 0) {
        int v = 0;
        n_xcc = (hipDeviceGetAttribute(&v, hipDeviceAttributeNumberOfXccs, c->device) == hipSuccess && v > 0) ? v : 8;
        xcc_of[c->device & 63].store(n_xcc);
    }
    if (kn.dp_xcd && NCH >= 64 && n_xcc == 8) {
        std::vector<int32_t> key((size_t)NCH), by_xcd((size_t)NCH * 8);
        for (int k = 0; k < NCH; k++) key[(size_t)k] = chains[(size_t)k].group * NC + chains[(size_t)k].contig;
        const int64_t nb = pga_dp_xcd_order(NCH, dp_order.data(), lens.data(), key.data(), NC * NG, by_xcd.data(), (int64_t)by_xcd.size());
        int64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0}, sum = 0, heaviest = 0;
        for (int64_t k = 0; k < nb; k++) if (by_xcd[(size_t)k] >= 0) { load[k & 7] += lens[(size_t)by_xcd[(size_t)k]]; sum += lens[(size_t)by_xcd[(size_t)k]]; }
        for (int q = 0; q < 8; q++) heaviest = std::max(heaviest, load[q]);
        if (nb > 0 && heaviest * 8 <= sum + sum * 3 / 10) { by_xcd.resize((size_t)nb); dp_order.swap(by_xcd); }       // within 1.3 x the mean
    }
}

// The plan of the call goes to the device in ONE copy (round 6; it was four copies and a memset): the cleared flags "scoring turned a
// start node into an edge node", per group and contig the run of chains scored on it, the batches before each contig (step
// schedule), the start order of the connection scoring, the chains -- one pinned staging area, one device area, the same layout.
// (Behind the chains the device area has room for the re-score chains of the winners, which are uploaded later.)
int FindCall::upload_plan() {
    // the workgroups of k_ovl_stops take 256 (chain, stop node) pairs each: the chain of a workgroup's first pair, relative to its group's
    // first chain, comes with the plan (a search on the device was three dependent loads in front of everything the workgroup does)
    ovl_blk0.assign((size_t)NG + 1, 0);
    for (int g = 0; g < NG; g++) ovl_blk0[(size_t)g + 1] = ovl_blk0[(size_t)g] + (g_s0[g + 1] - g_s0[g] + 255) / 256;
    const size_t pa_conv = 0, pa_cc = (((size_t)NG * NC + 1) + 7) & ~(size_t)7, pa_bb = pa_cc + sizeof(int2) * (size_t)2 * NG * NC,
                 pa_ord = pa_bb + ((sizeof(int32_t) * (h_bbase.size() + 1) + 7) & ~(size_t)7),
                 pa_blk = pa_ord + ((sizeof(int32_t) * (dp_order.size() + 1) + 7) & ~(size_t)7),
                 pa_ch = pa_blk + ((sizeof(int32_t) * ((size_t)ovl_blk0[NG] + 1) + 7) & ~(size_t)7), pa_copy = pa_ch + sizeof(ChainDesc) * (size_t)NCH;
    DEVBUF(d_plan, char, "d_call_plan", pa_copy + sizeof(ChainDesc) * ((size_t)NC + 2));
    PINBUF(h_plan, char, "h_call_plan", pa_copy + 64);
    d_conv = (uint8_t*)(d_plan + pa_conv);
    d_cc = (int2*)(d_plan + pa_cc); h_cc = (int2*)(h_plan + pa_cc);
    d_bbase = use_sched ? (int32_t*)(d_plan + pa_bb) : nullptr;
    if (!dp_order.empty()) d_dp_order = (int32_t*)(d_plan + pa_ord);
    d_chains = (ChainDesc*)(d_plan + pa_ch);
    memset(h_plan + pa_conv, 0, pa_cc);
    // per group and contig: the contiguous run of chains (models) scored on that contig
    for (size_t k = 0; k < (size_t)2 * NG * NC; k++) h_cc[k] = make_int2(0, 0);
    for (int k = 0; k < NCH; k++) {
        const int g = chains[k].group;
        int2& e = h_cc[(size_t)g * NC + chains[k].contig];
        if (e.y == 0) e.x = k;
        e.y++;
    }
    if (use_sched && !h_bbase.empty()) memcpy(h_plan + pa_bb, h_bbase.data(), sizeof(int32_t) * h_bbase.size());
    if (!dp_order.empty()) memcpy(h_plan + pa_ord, dp_order.data(), sizeof(int32_t) * dp_order.size());
    if (NCH > 0) memcpy(h_plan + pa_ch, chains.data(), sizeof(ChainDesc) * (size_t)NCH);
    d_ovl_blk = (const int32_t*)(d_plan + pa_blk);
    int32_t* const h_blk = (int32_t*)(h_plan + pa_blk);
    for (int g = 0; g < NG; g++) {
        int k = g_c0[g];
        const int64_t nb = ovl_blk0[(size_t)g + 1] - ovl_blk0[(size_t)g];
        for (int64_t b = 0; b < nb; b++) {
            const int64_t p0 = g_s0[g] + 256 * b;
            while (k + 1 < g_c0[g + 1] && chains[(size_t)k + 1].soff <= p0) k++;
            h_blk[ovl_blk0[(size_t)g] + b] = k - g_c0[g];
        }
    }
    HT(c, hipMemcpyAsync(d_plan, h_plan, pa_copy, hipMemcpyHostToDevice, st));
    return PGA_OK;
}

// node scoring of every group that has work; the wave-batch scorer's schedule, or the chain kernels' records, behind it
int FindCall::score_groups() {
    sp = ScoreParams{P.closed, P.meta, P.max_overlap, NM, nullptr, nullptr};
    sp.models_per_pass = kn.ss_models_per_pass;
    PINSET(h_conv, uint8_t, "h_conv_flag", (size_t)NG * NC + 1);
    for (int g = 0; g < NG; g++) {
        const int nch = g_c0[g + 1] - g_c0[g];
        const int64_t nn = g_n0[g + 1] - g_n0[g];
        if (!group_has_work(g) || stage == PGA_STAGE_EXTRACT) continue;
        // the ORF walks of the coding score run from hexamer tables in LDS, contigs bucketed by the four table columns they need
        // (PGA_CS_LDS=0: the global-memory form)
        const void* d_cs_tasks = nullptr; const void* d_cs_entries = nullptr; int n_cs_tasks = 0;
        // kn.cs_task_nodes: several tasks per CU and launch (swept again at the end of round 6, one box: 4096 629 us per launch, 4864 581, 5120 586, 5376 584, 5632 600, 6144 592)
        // (single mode as well: one table column, a genome is cut into tasks of that many nodes)
        // (the global-memory form walks every ORF on one lane through the texture path: a launch takes as long as its longest ORF,
        //  a few hundred microseconds on high-GC sequence whatever its size -- so small launches take the LDS form as well)
        if (kn.cs_lds && !f->gil_stride.empty()) {
            std::vector<int32_t>& tk = cs_tk[g]; std::vector<int32_t>& en = cs_en[g];     // alive until the stream is synchronized
            if (pga_cs_tasks(h_cc + (size_t)g * NC, NC, chains.data(), h_cb(g), f->model_rank.data(), kn.cs_task_nodes, tk, en) && !tk.empty()) {
                void* p1; void* p2;
                GROUPBUF(p1, void*, "cs_tasks", tk.size() * 4 + 64, false)
                GROUPBUF(p2, void*, "cs_entries", en.size() * 4 + 64, false)
                HT(c, hipMemcpyAsync(p1, tk.data(), tk.size() * 4, hipMemcpyHostToDevice, st));
                HT(c, hipMemcpyAsync(p2, en.data(), en.size() * 4, hipMemcpyHostToDevice, st));
                d_cs_tasks = p1; d_cs_entries = p2; n_cs_tasks = (int)(tk.size() / 4);
            }
        }
        sp.conv_flag = meta_run ? d_conv + (size_t)g * NC : nullptr;
        const ScoreGroup grp = score_group(g, d_chains + g_c0[g], nch, g_n0[g], nn, d_cc + (size_t)g * NC);
        const int32_t n_stops = group_stops(g), n_starts = (int32_t)(group_nodes[g] - n_stops);
        // (the path proper; a stage-level call returns the node arrays after any stage, so there every node keeps its thread)
        const bool starts_only = stage == 0 && kn.ss_starts_only;
        StartScoreLaunch ss(grp);
        ss.form = starts_only ? StartScoreLaunch::listed_loop : StartScoreLaunch::all_nodes;
        ss.d_sd_lut = f->d_sd_lut; ss.n_starts = n_starts; ss.n_stops = n_stops; ss.sbase = d_sb(g);
        ss.mm_tile_items = kn.ss_mm_tile; ss.profile = kn.ss_profile;
        // the model-major start scoring: its records, chains and tiles live in the context (PGA_SS_MM=0: the model loop).  With one
        // model loaded the model loop has nothing to walk (one staging, one barrier per workgroup) and stays: on a 200 Mbp genome the
        // two kernels took 2 ms more (k_mm_place writes a chain's thousands of tiles from one thread)
        if (starts_only && n_starts > 0 && NM > 1 && kn.ss_mm) {
            std::vector<int64_t> mm_items;
            ss.mm_tiles = pga_mm_tiles(chains.data() + g_c0[g], nch, h_cb(g), h_sb(g), NM, kn.ss_mm_tile, mm_items);
            GROUPBUF(ss.mm_rec, void*, "ss_rec", PGA_SS_REC_BYTES * (size_t)n_starts + 64, false)
            GROUPBUF(ss.mm_chain, void*, "ss_mmchain", PGA_SS_MMCHAIN_BYTES * (size_t)nch + 64, false)
            GROUPBUF(ss.mm_tile, void*, "ss_mmtile", PGA_SS_MMTILE_BYTES * (size_t)ss.mm_tiles + 64, false)
            GROUPBUF(ss.mm_scratch, void*, "ss_mmscratch", pga_mm_scratch_bytes(NM, nch), false)
            if (ss.mm_tiles > 0) ss.form = StartScoreLaunch::model_major;      // (no start node in any chain's contig: nothing to tile)
        }
        // overlapping starts over (chain, stop node) pairs; for the wave-batch scorer the same pass builds the stops' extras and
        // the start scorer leaves cscore + sscore, so its per-chain preparation is done when scoring is
        OverlapLaunch ov(grp);
        ov.form = OverlapLaunch::stop_pairs; ov.d_mc = c->d_model_const; ov.max_overlap = sp.max_overlap;
        ov.sbase = d_sb(g); ov.soff_begin = g_s0[g]; ov.n_pairs = g_s0[g + 1] - g_s0[g]; ov.n_stops = n_stops;
        ov.blk_chain = kn.ovl_search ? nullptr : d_ovl_blk + ovl_blk0[(size_t)g];
        sp.cs_out = nullptr;
        if (wave_prep) {
            ov.topo_q2 = wgroups.g[g].q2; ov.ext = wbuf.ext; ov.cs_out = sp.cs_out = wbuf.cs;
            if (use_wave) {
                // (direct mode: the tail reads star_ptr only at the stop nodes, which k_ovl_stops always writes)
                ov.fill_star_ptr = !(stage == 0 && direct_gather);
                // (the path proper, node arrays not asked for: a stop node's zero scores are read by nobody -- ScoreParams::lean_stops)
                sp.lean_stops = (stage == 0 && direct_gather && starts_only && !kn.ss_full_stops) ? 1 : 0;
            }       // (segments walked by the wave-batch kernel: the re-scoring and verifying kernels read the node arrays in full)
        }
        ss.sp = sp;       // (final for this group; the member keeps cs_out and lean_stops for the re-score of the winners)
        const bool gil = meta_run || per_contig || n_cs_tasks > 0;
        CodingScoreLaunch cs(grp);
        cs.form = n_cs_tasks > 0 ? CodingScoreLaunch::lds_tasks : CodingScoreLaunch::global_memory;
        cs.d_msc = f->d_msc; cs.d_gil = gil ? f->d_gil + f->gil_off[g] : nullptr; cs.il_stride = gil ? f->gil_stride[g] : 0; cs.d_rank = f->d_model_rank;
        cs.d_cs_tasks = d_cs_tasks; cs.n_cs_tasks = n_cs_tasks; cs.d_cs_entries = d_cs_entries;
        cs.cs_wave = kn.cs_wave; cs.qclasses = kn.cs_qclasses; cs.profile = kn.cs_profile;
        pga_launch_coding_score(cs);
        if (!pga_launch_start_scores(ss)) { c->err = "pga_find_genes: the start scoring was planned in a form whose buffers are missing"; return PGA_EDEVICE; }
        pga_launch_overlapping_starts(ov);
        if (wave_prep && use_sched) {
            // (behind the scoring launches: the schedule's headers carry the stop nodes' ranks, which k_ovl_topo writes there)
            if (g < 4) HT(c, hipEventRecord(f->e_aux[4 * g + 2], st));
            pga_launch_dpw_sched(kn, wgroups.g[g], d_cb(g), d_bbase + (size_t)g * (NC + 1), NC, max_batches[g], st);
            if (g < 4) HT(c, hipEventRecord(f->e_aux[4 * g + 3], st));
            HT(c, hipMemcpyAsync(h_scur + 2 * g, wgroups.g[g].scur, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        }
        NodeArrays na{ga[g].ndx, ga[g].stop_val, ga[g].type, ga[g].strand, ca.cscore, ca.sscore, ca.rscore, ca.uscore, ca.star_ptr};
        if (!use_wave && stage == 0) pga_launch_dp_prepare(d_chains + g_c0[g], nch, g_n0[g], nn, na, c->d_model_const, dp, st);
    }
    return PGA_OK;
}

// what both copy-outs of node arrays (the stage-level one, the winners') fill alike; every source points at the contig's first node
void copy_node_topology(pga_nodes& N, const int n, const int32_t* ndx, const int32_t* stop_val, const uint8_t* type, const int8_t* strand, const uint8_t* edge) {
    memcpy(N.ndx, ndx, 4 * (size_t)n); memcpy(N.stop_val, stop_val, 4 * (size_t)n);
    memcpy(N.type, type, n); memcpy(N.strand, strand, n); memcpy(N.edge, edge, n);
}
void copy_node_scores(pga_nodes& N, const int n, const double* const src64[6] /* cscore, sscore, rscore, uscore, tscore, mot_score */, const int32_t* mot_ndx,
                      const uint8_t* rbs, const uint8_t* mot_len, const uint8_t* mot_spacer, const uint8_t* mot_spacendx, const float* gc_cont) {
    double* const dst64[6] = {N.cscore, N.sscore, N.rscore, N.uscore, N.tscore, N.mot_score};
    for (int q = 0; q < 6; q++) memcpy(dst64[q], src64[q], 8 * (size_t)n);
    memcpy(N.mot_ndx, mot_ndx, 4 * (size_t)n); memcpy(N.rbs, rbs, 2 * (size_t)n); memcpy(N.mot_len, mot_len, n);
    memcpy(N.mot_spacer, mot_spacer, n); memcpy(N.mot_spacendx, mot_spacendx, n); memcpy(N.gc_cont, gc_cont, 4 * (size_t)n);
}
void reset_dp_fields(pga_nodes& N, const int n) { for (int j = 0; j < n; j++) { N.traceb[j] = -1; N.tracef[j] = -1; N.ov_mark[j] = -1; } }    // ref: reset_node_scores

// ---- stage-level call: bring the node arrays home as they are now and stop ---------------
int FindCall::return_stage_nodes(pga_result** out) {
    const int64_t nn = tot_chain_nodes;          // every group's nodes; a contig's chain sits at the same offset in both layouts
    PINBUF(hs_i32, int32_t, "hs_i32", 6 * nn + 8);         // ndx, stop_val, mot_ndx, star_ptr[3]
    PINBUF(hs_f64, double, "hs_f64", 6 * nn + 8);          // cscore, sscore, rscore, uscore, tscore, mot_score
    PINBUF(hs_u8, uint8_t, "hs_u8", 10 * nn + 8);          // type, strand, edge, rbs[2], mot_len, mot_spacer, mot_spacendx
    PINBUF(hs_f32, float, "hs_f32", nn + 8);
    const bool scored = stage >= PGA_STAGE_SCORE;
    for (int g = 0; g < NG; g++) {
        const int64_t gn = group_nodes[g], o = g_n0[g];
        if (gn == 0) continue;
        HT(c, hipMemcpyAsync(hs_i32 + o, ga[g].ndx, 4 * gn, hipMemcpyDeviceToHost, st));
        HT(c, hipMemcpyAsync(hs_i32 + nn + o, ga[g].stop_val, 4 * gn, hipMemcpyDeviceToHost, st));
        HT(c, hipMemcpyAsync(hs_u8 + o, ga[g].type, gn, hipMemcpyDeviceToHost, st));
        HT(c, hipMemcpyAsync(hs_u8 + nn + o, ga[g].strand, gn, hipMemcpyDeviceToHost, st));
        if (!scored) HT(c, hipMemcpyAsync(hs_u8 + 2 * nn + o, ga[g].edge0, gn, hipMemcpyDeviceToHost, st));
        if (scored) HT(c, hipMemcpyAsync(hs_f32 + o, ga[g].gc_cont, 4 * gn, hipMemcpyDeviceToHost, st));
    }
    if (nn > 0 && scored) {
        HT(c, hipMemcpyAsync(hs_u8 + 2 * nn, ca.edge, nn, hipMemcpyDeviceToHost, st));
        HT(c, hipMemcpyAsync(hs_i32 + 2 * nn, ca.mot_ndx, 4 * nn, hipMemcpyDeviceToHost, st));
        HT(c, hipMemcpyAsync(hs_i32 + 3 * nn, ca.star_ptr, 12 * nn, hipMemcpyDeviceToHost, st));
        double* const src64[6] = {ca.cscore, ca.sscore, ca.rscore, ca.uscore, ca.tscore, ca.mot_score};
        for (int q = 0; q < 6; q++) HT(c, hipMemcpyAsync(hs_f64 + q * nn, src64[q], 8 * nn, hipMemcpyDeviceToHost, st));
        HT(c, hipMemcpyAsync(hs_u8 + 3 * nn, ca.rbs, 2 * nn, hipMemcpyDeviceToHost, st));
        HT(c, hipMemcpyAsync(hs_u8 + 5 * nn, ca.mot_len, nn, hipMemcpyDeviceToHost, st));
        HT(c, hipMemcpyAsync(hs_u8 + 6 * nn, ca.mot_spacer, nn, hipMemcpyDeviceToHost, st));
        HT(c, hipMemcpyAsync(hs_u8 + 7 * nn, ca.mot_spacendx, nn, hipMemcpyDeviceToHost, st));
    }
    if (const int rc = sync()) return rc;
    f->last.d_dig = d_dig; f->last.ga = ga[0]; f->last.ca = ca; f->last.n_nodes = (int)nn; f->last.len = batch->ct[0].len;
    R->nodes.resize(NC);
    for (int i = 0; i < NC; i++) {
        pga_nodes& N = R->nodes[i];
        const int g = multi ? cgrp[i] : 0;
        const int64_t oo = g_n0[g] + h_cb(g)[i]; const int n = contig_nodes(g, i);
        R->contigs[i].model = stage == PGA_STAGE_EXTRACT ? -1 : (per_contig ? model_of_contig[i] : 0); R->contigs[i].n_nodes = n;
        if (int rc = alloc_nodes(R, N, n)) return rc;
        copy_node_topology(N, n, hs_i32 + oo, hs_i32 + nn + oo, hs_u8 + oo, (const int8_t*)(hs_u8 + nn + oo), hs_u8 + 2 * nn + oo);
        reset_dp_fields(N, n);
        if (!scored) continue;
        if (stage >= PGA_STAGE_OVERLAP) memcpy(N.star_ptr, hs_i32 + 3 * nn + 3 * oo, 12 * (size_t)n);
        const double* const src64[6] = {hs_f64 + oo, hs_f64 + nn + oo, hs_f64 + 2 * nn + oo, hs_f64 + 3 * nn + oo, hs_f64 + 4 * nn + oo, hs_f64 + 5 * nn + oo};
        copy_node_scores(N, n, src64, hs_i32 + 2 * nn + oo, hs_u8 + 3 * nn + 2 * oo, hs_u8 + 5 * nn + oo, hs_u8 + 6 * nn + oo, hs_u8 + 7 * nn + oo, hs_f32 + oo);
    }
    return publish_result(out);
}

// one DP launch over the chains of every group (chains are independent, the more in flight the better), the read-back, the relaunch
// when a step schedule did not fit, the statistics and timings
int FindCall::score_connections() {
    PINBUF(h_segflags, int32_t, "h_segflags", (size_t)(PGA_SEG_ROUNDS + 2) * NCH + 1);      // [rounds][chains] flags, [chains] spine sizes, [chains] a round's verdict
    if (segmented && kn.dp_seg_readback) seg_dev.h_round = h_segflags + (size_t)(PGA_SEG_ROUNDS + 1) * NCH;
    HT(c, hipEventRecord(f->e_dp0[0], st));
    if (use_wave) {
        // PGA_DP_PROFILE=1: cycles per batch phase of every 64th chain (a synchronising debug aid)
        if (kn.dp_profile) {
            DEVBUF(d_prof, unsigned long long, "dp_prof", 16);
            HT(c, hipMemsetAsync(d_prof, 0, 128, st));
            dp.prof = d_prof;
        }
        pga_launch_dp_wave(d_chains, NCH, wgroups, c->d_model_const, dp, wbuf, st, d_dp_order, (int)dp_order.size(), use_sched);
        if (dp.prof != nullptr) {
            unsigned long long pr[16];
            HT(c, hipStreamSynchronize(st));
            HT(c, hipMemcpy(pr, dp.prof, 128, hipMemcpyDeviceToHost));
            const double nbp = pr[7] ? (double)pr[7] : 1.0;
            fprintf(stderr, "[pga dp profile] %s, %d chains, batches sampled=%llu, cycles/batch: load=%.0f near steps=%.0f far gene ends=%.0f "
                            "carries=%.0f chains=%.0f walk=%.0f finalize=%.0f | total=%.0f\n", use_sched ? "k_dp_wave" : "k_dpw_dyn", NCH, pr[7], pr[0] / nbp, pr[1] / nbp, pr[2] / nbp, pr[3] / nbp,
                    pr[4] / nbp, pr[5] / nbp, pr[6] / nbp, (pr[0] + pr[1] + pr[2] + pr[3] + pr[4] + pr[5] + pr[6]) / nbp);
            dp.prof = nullptr;
        }
    }
    else pga_launch_dp(kn, d_chains, NCH, c->d_model_const, dp, 1, st, segmented ? &seg_dev : nullptr);
    HT(c, hipEventRecord(f->e_dp1[0], st));
    HT(c, hipMemcpyAsync(h_maxscore, dp.max_score, sizeof(double) * 2 * (size_t)dp_slots, hipMemcpyDeviceToHost, st));       // scores, indices, path starts
    if (meta_run) HT(c, hipMemcpyAsync(h_conv, d_conv, (size_t)NG * NC, hipMemcpyDeviceToHost, st));
    if (segmented) {
        HT(c, hipMemcpyAsync(h_segflags, seg_dev.flags, sizeof(int32_t) * PGA_SEG_ROUNDS * NCH, hipMemcpyDeviceToHost, st));
        HT(c, hipMemcpyAsync(h_segflags + (size_t)PGA_SEG_ROUNDS * NCH, seg_dev.nsp, sizeof(int32_t) * NCH, hipMemcpyDeviceToHost, st));
    }
    if (const int rc = sync()) return rc;
    uint32_t sched_missed = 0;
    double dp_first_ms = 0.0;
    if (use_sched) {
        // a schedule that did not fit its buffer (node-dense input: more than two slots per node on average): the same launch again
        // with the kernel that works the lane masks out itself
        for (int g = 0; g < NG; g++) if (group_has_work(g)) sched_missed += h_scur[2 * g + 1];
        if (kn.dpw_sched_debug) for (int g = 0; g < NG; g++) fprintf(stderr, "[pga dpw sched] group %d: %u batches missed\n", g, h_scur[2 * g + 1]);
        if (sched_missed && use_wave) {      // (segments walked by the wave-batch kernel: a missed batch ends its segment's claims, the verification does the rest)
            // (the first launch's time counts: t_dp_ms covers both)
            { float ms = 0; HT(c, hipEventElapsedTime(&ms, f->e_dp0[0], f->e_dp1[0])); dp_first_ms = ms; }
            HT(c, hipEventRecord(f->e_dp0[0], st));
            pga_launch_dp_wave(d_chains, NCH, wgroups, c->d_model_const, dp, wbuf, st, d_dp_order, (int)dp_order.size(), false);
            HT(c, hipEventRecord(f->e_dp1[0], st));
            HT(c, hipMemcpyAsync(h_maxscore, dp.max_score, sizeof(double) * 2 * (size_t)dp_slots, hipMemcpyDeviceToHost, st));
            if (const int rc = sync()) return rc;
        }
    }
    pga_dp_note_stats(c, segmented ? &seg_plan : nullptr, h_segflags, NCH);
    c->dp_stats[6] = use_sched ? 1 : 0; c->dp_stats[7] = (int32_t)sched_missed;
    if (segmented && kn.dp_seg_debug) {
        fprintf(stderr, "[pga dp-seg] %d chains cut into %d segments (<= %d nodes each); nodes rejected per round: %d %d %d; walked serially: %d; spine:",
                seg_dev.n_big, seg_dev.n_segs, seg_dev.max_seg_nodes, c->dp_stats[2], c->dp_stats[3], c->dp_stats[4], c->dp_stats[5]);
        for (int k : seg_plan.big) fprintf(stderr, " %d/%d", h_segflags[(size_t)PGA_SEG_ROUNDS * NCH + k], chains[(size_t)k].n);
        fprintf(stderr, "\n");
    }
    { float ms = 0; HT(c, hipEventElapsedTime(&ms, f->e_dp0[0], f->e_dp1[0])); R->pub.t_dp_ms = NCH > 0 ? ms + dp_first_ms : 0.0; }
    c->dp_timings[0] = R->pub.t_dp_ms; c->dp_timings[1] = c->dp_timings[2] = c->dp_timings[3] = 0.0;
    if (wave_prep) for (int g = 0; g < NG && g < 4; g++) {
        if (!group_has_work(g)) continue;
        float ms = 0;
        if (hipEventElapsedTime(&ms, f->e_aux[4 * g], f->e_aux[4 * g + 1]) == hipSuccess) c->dp_timings[1] += ms;
        if (use_sched && hipEventElapsedTime(&ms, f->e_aux[4 * g + 2], f->e_aux[4 * g + 3]) == hipSuccess) c->dp_timings[2] += ms;
    }
    return PGA_OK;
}

// ---- pick the winning model per contig (the rules: find_plan.h) ---
void FindCall::pick_winners() {
    pga_plan::pick_winners(NC, NM, P.meta != 0, chains.data(), NCH, h_maxscore, h_ipath, use_sets ? set_of.data() : nullptr, NS,
                           c->model_scores.data(), c->set_model.data(), c->set_score.data(), win_chain);
}

// ---- fresh re-score of winners that were not the first model of their group (who: find_plan.h)
int FindCall::rescore_winners() {
    pga_plan::plan_rescore(NC, NG, P.meta != 0, chains.data(), win_chain.data(), h_conv, f->model_group.data(), tot_chain_nodes, *this);
    if (rescore.empty()) return PGA_OK;
    HT(c, hipMemcpyAsync(d_chains + NCH, rescore.data(), sizeof(ChainDesc) * rescore.size(), hipMemcpyHostToDevice, st));
    int2* h_cc2 = h_cc + (size_t)NG * NC;
    for (size_t k = 0; k < rescore.size(); k++)
        h_cc2[(size_t)f->model_group[rescore[k].model] * NC + rescore[k].contig] = make_int2(NCH + (int)k, 1);
    HT(c, hipMemcpyAsync(d_cc + (size_t)NG * NC, h_cc2, sizeof(int2) * (size_t)NG * NC, hipMemcpyHostToDevice, st));
    sp.conv_flag = nullptr; sp.cs_out = nullptr;
    for (int g = 0; g < NG; g++) {
        const int nch = r_c0[g + 1] - r_c0[g]; const int64_t nn = r_n0[g + 1] - r_n0[g];
        if (nch == 0 || nn == 0) continue;
        // no coding-score launch: the raw coding score of a start depends on the model only, not on which model of the group was scored
        // first on the contig, so the fresh re-score of a winning model (ref: lib.pyx:5380-5394) reads it where the winning pass left
        // it (ChainDesc::raw_off) instead of walking every ORF again
        const ScoreGroup grp = score_group(g, d_chains + NCH + r_c0[g], nch, r_n0[g], nn, d_cc + (size_t)NG * NC + (size_t)g * NC);
        StartScoreLaunch ss(grp);          // (a thread per node)
        ss.sp = sp; ss.d_sd_lut = f->d_sd_lut; ss.profile = kn.ss_profile;
        if (!pga_launch_start_scores(ss)) { c->err = "pga_find_genes: the re-score of the winners could not be launched"; return PGA_EDEVICE; }
        OverlapLaunch ov(grp);             // (k_overlapping_starts over every node)
        ov.d_mc = c->d_model_const; ov.max_overlap = sp.max_overlap;
        pga_launch_overlapping_starts(ov);
    }
    return PGA_OK;
}

// ---- gather the winners (the layout: find_plan.h) ------------------------------------------------
// the winners' final-pass fields only travel to the gathered arrays when somebody reads more of them than the two nodes
// of every gene: the caller (node arrays) or the host tail's attribute fetch (PGA_FULL_GATHER=1 keeps the full gather: tests)
int FindCall::gather_winners() {
    pga_plan::plan_gather(NC, NG, chains.data(), win_chain.data(), fin_off.data(), *this);
    // one device arena (and a pinned mirror, used only when the caller asks for the node arrays)
    {
        const size_t n = (size_t)out_nodes + 1;
        size_t off = 0;
        auto reserve = [&](size_t elem, size_t mult) { const size_t at = off; off += ((elem * mult * n + 255) / 256) * 256; return at; };
#define OFFS(field, type, mult) const size_t at_##field = reserve(sizeof(type), mult);
        OFFS(ndx, int32_t, 1) OFFS(stop_val, int32_t, 1) OFFS(type, uint8_t, 1) OFFS(strand, int8_t, 1)
        OFFS(edge_dp, uint8_t, 1) OFFS(cscore_dp, double, 1) OFFS(sscore_dp, double, 1) OFFS(rscore_dp, double, 1) OFFS(uscore_dp, double, 1) OFFS(tscore_dp, double, 1)
        OFFS(star_ptr, int32_t, 3) OFFS(traceb, int32_t, 1) OFFS(ov_mark, int8_t, 1) OFFS(score, double, 1)
        arena_dp = off;
        OFFS(gc_cont, float, 1)
        OFFS(edge, uint8_t, 1) OFFS(cscore, double, 1) OFFS(sscore, double, 1) OFFS(rscore, double, 1) OFFS(uscore, double, 1) OFFS(tscore, double, 1) OFFS(mot_score, double, 1)
        OFFS(mot_ndx, int32_t, 1) OFFS(rbs, uint8_t, 2) OFFS(mot_len, uint8_t, 1) OFFS(mot_spacer, uint8_t, 1) OFFS(mot_spacendx, uint8_t, 1)
        arena_all = off;
        void* dp__; void* hp__;
        { int rc__ = ensure_dev(c, "o_arena", arena_all + 256, &dp__); if (rc__) return rc__; }
        { int rc__ = ensure_pin(c, "h_arena", arena_all + 256, &hp__); if (rc__) return rc__; }
        char* db = (char*)dp__; char* hb = (char*)hp__;
#define OB(field, type) o.field = (type*)(db + at_##field); h.field = (type*)(hb + at_##field);
        OB(ndx, int32_t) OB(stop_val, int32_t) OB(type, uint8_t) OB(strand, int8_t) OB(gc_cont, float)
        OB(edge_dp, uint8_t) OB(cscore_dp, double) OB(sscore_dp, double) OB(rscore_dp, double) OB(uscore_dp, double) OB(tscore_dp, double)
        OB(star_ptr, int32_t) OB(traceb, int32_t) OB(ov_mark, int8_t) OB(score, double)
        OB(edge, uint8_t) OB(cscore, double) OB(sscore, double) OB(rscore, double) OB(uscore, double) OB(tscore, double) OB(mot_score, double)
        OB(mot_ndx, int32_t) OB(rbs, uint8_t) OB(mot_len, uint8_t) OB(mot_spacer, uint8_t) OB(mot_spacendx, uint8_t)
    }
    // lean and the device tail: gather only what the tail writes
    o.direct = direct_gather ? 1 : 0;
    for (int g = 0; g < 4; g++) {
        const bool in = g < NG;
        o.g_ndx[g] = in ? ga[g].ndx : nullptr; o.g_stop_val[g] = in ? ga[g].stop_val : nullptr;
        o.g_type[g] = in ? ga[g].type : nullptr; o.g_strand[g] = in ? ga[g].strand : nullptr;
    }
    o.c_edge = ca.edge; o.c_cscore = ca.cscore; o.c_rscore = ca.rscore; o.c_uscore = ca.uscore; o.c_tscore = ca.tscore;
    o.c_star_ptr = ca.star_ptr; o.d_score = dp.score;
    h.direct = 0;
    size_t nwin = 0; for (int g = 0; g < NG; g++) nwin += wg[g].size();
    DEVBUF(d_win, WinDesc, "d_win", nwin + 1);
    size_t k0 = 0;
    for (int g = 0; g < NG; g++) {
        if (wg[g].empty()) continue;
        HT(c, hipMemcpyAsync(d_win + k0, wg[g].data(), sizeof(WinDesc) * wg[g].size(), hipMemcpyHostToDevice, st));
        const int64_t nn = w_o0[g + 1] - w_o0[g];
        if (nn > 0)
            hipLaunchKernelGGL(k_gather_winners, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, d_win + k0, (int)wg[g].size(), w_o0[g], nn, ga[g], ca, dp, o, lean_gather ? 1 : 0);
        k0 += wg[g].size();
    }
    for (int i = 0; i < NC; i++) if (win_chain[i] >= 0) max_n = std::max(max_n, chains[win_chain[i]].n);
    return PGA_OK;
}

// the contigs of the result from the winners and the genes the tail found per contig; gene_begin (or nullptr): a copy of every contig's first gene
int64_t FindCall::contig_results(const int32_t* n_genes, int64_t* gene_begin) {
    int64_t ngenes = 0;
    for (int i = 0; i < NC; i++) {
        pga_contig_result& cr = R->contigs[i];
        const int k = win_chain[i];
        if (gene_begin) gene_begin[i] = ngenes;
        cr.gene_begin = ngenes; cr.n_genes = n_genes[i];
        ngenes += cr.n_genes;
        if (k < 0) { cr.model = -1; continue; }
        cr.model = chains[k].model; cr.n_nodes = chains[k].n;
        cr.score = P.meta ? 0.0 : (h_ipath[k] >= 0 ? h_maxscore[k] : 0.0);
    }
    return ngenes;
}

// PGA_TAIL=host (a cross-check): the winners' DP-pass fields come home and host threads walk them -- traceback untangling, bad-gene
// elimination, gene list, start tweaks per contig; the fields of every gene's two nodes come with a second, small gather
int FindCall::run_host_tail() {
    tracef.assign((size_t)out_nodes + 1, -1);
    elim.assign((size_t)out_nodes + 1, 0);
    if (out_nodes > 0)
        HT(c, hipMemcpyAsync(h.ndx, o.ndx, P.want_nodes == 1 ? arena_all : arena_dp, hipMemcpyDeviceToHost, st));   // arena starts at `ndx`
    if (const int rc = stop_clock()) return rc;

    tm->mark("gather+d2h+sync");
    // ---- host tail per contig ------------------------------------------------------------------
    std::vector<std::vector<GeneRec>> cg(NC);
    std::unique_ptr<int32_t[]> pathbuf(new int32_t[(size_t)out_nodes + 1]);      // written before it is read: no zero fill
    std::atomic<int> next(0);
    auto worker = [&]() {
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= NC) break;
            const int k = win_chain[i];
            if (k < 0) continue;
            const int64_t oo = out_off[i];
            NodeView v{chains[k].n, h.ndx + oo, h.stop_val + oo, h.type + oo, h.strand + oo, h.edge_dp + oo,
                       h.cscore_dp + oo, h.sscore_dp + oo, h.rscore_dp + oo, h.uscore_dp + oo, h.tscore_dp + oo,
                       h.star_ptr + 3 * oo, h.traceb + oo, tracef.data() + oo, h.ov_mark + oo, h.score + oo, elim.data() + oo};
            const int mx = h_maxidx[k];
            const double st_wt = c->models[chains[k].model].st_wt;
            const bool sub = NC == 1 && kn.timing;
            auto now = [] { return std::chrono::steady_clock::now(); };
            auto t0 = now(), t1 = t0, t2 = t0, t3 = t0;
            if (v.n > 0 && mx >= 0) {
                int32_t* pl = pathbuf.get() + oo;
                const int cnt = untangle(v, mx, pl);
                t1 = now();
                if (v.traceb[mx] != -1) {
                    if (NC < 4) eliminate_bad_genes_mt(v, pl, cnt, st_wt, f->pool, 16); else eliminate_bad_genes(v, pl, cnt, st_wt);
                    t2 = now();
                    cg[i].resize((size_t)cnt / 2 + 2);           // two path nodes per gene
                    cg[i].resize((size_t)extract_genes(v, pl, cnt, cg[i].data()));
                }
            }
            t3 = now();
            tweak_final_starts(v, cg[i], st_wt, P.max_overlap, NC < 4 ? 32 : 1, &f->pool);
            if (sub) {
                auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
                fprintf(stderr, "[pga timing] host tail: untangle=%.2f eliminate=%.2f extract=%.2f tweak=%.2f ms\n", ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, now()));
            }
        }
    };
    auto run_parallel = [&](const std::function<void()>& fn) {
        int nt = (int)std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 32u);
        if (NC < 4) nt = 1;
        if (nt == 1) fn(); else f->pool.run(fn, nt);
    };
    run_parallel(worker);
    // the tail moved start scores (eliminate_bad_genes): the arena kept on the device must say what the host copy says
    if (P.want_nodes && out_nodes > 0)
        HT(c, hipMemcpyAsync(o.sscore_dp, h.sscore_dp, sizeof(double) * (size_t)out_nodes, hipMemcpyHostToDevice, st));
    tm->mark("host_tail");
    // ---- results -----------------------------------------------------------------------------------
    std::vector<int32_t> n_genes((size_t)NC);
    for (int i = 0; i < NC; i++) n_genes[i] = (int32_t)cg[i].size();
    const int64_t ngenes = contig_results(n_genes.data(), nullptr);
    R->genes.resize((size_t)ngenes);
    // fields of the gene's start / stop nodes as of the final pass: a second, small gather
    PINBUF(h_gidx, int64_t, "h_gidx", 2 * ngenes + 1);
    PINBUF(h_attr, GeneNodeAttr, "h_attr", 2 * ngenes + 1);
    if (ngenes > 0) {
        DEVBUF(d_gidx, int64_t, "d_gidx", 2 * ngenes + 1);
        DEVBUF(d_attr, GeneNodeAttr, "d_attr", 2 * ngenes + 1);
        for (int i = 0; i < NC; i++) {
            int64_t gi = R->contigs[i].gene_begin;
            for (const GeneRec& gr : cg[i]) { h_gidx[2 * gi] = out_off[i] + gr.start_ndx; h_gidx[2 * gi + 1] = out_off[i] + gr.stop_ndx; gi++; }
        }
        HT(c, hipMemcpyAsync(d_gidx, h_gidx, sizeof(int64_t) * 2 * ngenes, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_gather_gene_nodes, dim3((unsigned)((2 * ngenes + 255) / 256)), dim3(256), 0, st, d_gidx, (int)(2 * ngenes), o, d_attr);
        HT(c, hipMemcpyAsync(h_attr, d_attr, sizeof(GeneNodeAttr) * 2 * ngenes, hipMemcpyDeviceToHost, st));
        if (const int rc = sync()) return rc;
    }
    tm->mark("gene_attrs");
    std::atomic<int> next2(0);
    auto filler = [&]() {
        for (;;) {
            const int i = next2.fetch_add(1);
            if (i >= NC) break;
            const int k = win_chain[i];
            if (k < 0) continue;
            const int64_t oo = out_off[i];
            const bool single = !P.meta;
            int64_t gi = R->contigs[i].gene_begin;
            for (const GeneRec& gr : cg[i]) {
                const GeneNodeAttr& as = h_attr[2 * gi]; const GeneNodeAttr& ae = h_attr[2 * gi + 1];
                const int64_t sn = oo + gr.start_ndx, en = oo + gr.stop_ndx;
                GeneSrc s;          // the DP pass came home with the winners; the final pass's fields of the two nodes are in `as` and `ae`
                s.topology(h.strand, h.type, sn);
                if (single) s.scores(h.edge_dp, h.cscore_dp, h.sscore_dp, h.rscore_dp, h.uscore_dp, h.tscore_dp, sn, en, sn);
                else { s.scores(&as.edge, &as.cscore, &as.sscore, &as.rscore, &as.uscore, &as.tscore, 0, 0, 0); s.edge_e = &ae.edge; }
                s.motifs(as.rbs, &as.mot_len, &as.mot_spacer, &as.mot_ndx, &as.mot_score, 0, &as.gc_cont, 0);
                R->genes[(size_t)gi++] = gene_record(i, gr, s);
            }
        }
    };
    run_parallel(filler);
    if (coding) {
        // the records are on the host already, so they are counted here -- a union of intervals per contig, the same definition as
        // k_cover_genes / k_count_cover
        std::vector<std::pair<int32_t, int32_t>> iv;
        for (int i = 0; i < NC; i++) {
            iv.clear();
            const int32_t len = batch->ct[i].len;
            for (const GeneRec& gr : cg[i]) {
                const int32_t b = std::max<int32_t>(gr.begin, 1), e = std::min<int32_t>(gr.end, len);
                if (b <= e) iv.emplace_back(b, e);
            }
            std::sort(iv.begin(), iv.end());
            int64_t n = 0; int32_t hi = 0;          // positions 1 .. hi are already counted
            for (const auto& x : iv) {
                if (x.second <= hi) continue;
                n += x.second - std::max(x.first - 1, hi);
                hi = x.second;
            }
            coding[i] = n;
        }
    }
    return PGA_OK;
}

// the work arrays of the device tail
struct TailBufs {
    TailDesc* d_td; int32_t* d_tracef; uint8_t* d_elim; GeneRec* d_gene0; GeneRec* d_gene1; GeneRec* d_gene2; int32_t* d_ngenes;
    int32_t* d_path; uint8_t* d_changed; int32_t* d_nchanged;
    int64_t n_slots; unsigned init_blocks;
};

// PGA_TAIL=par (the default): traceback untangling, bad-gene elimination and the gene list of every winning chain by parallel steps
// over the gathered nodes (tail.inl)
int FindCall::launch_tail_paths(const TailBufs& t) {
    bool tail_inited = false;
    for (int i = 0; i < NC; i++) if (win_chain[i] >= 0 && chains[win_chain[i]].n > 0) segs.push_back(TpSeg{out_off[i], chains[win_chain[i]].n, i});
    std::sort(segs.begin(), segs.end(), [](const TpSeg& a, const TpSeg& b) { return a.off < b.off; });
    if (!segs.empty() && out_nodes > 0) {
        if (out_nodes >= (1ll << 30)) { c->err = "pga_find_genes: more than 2^30 nodes in the winning chains of one batch"; return PGA_EINVAL; }
        int levels = 1;
        while ((1ll << levels) < max_n) levels++;
        const unsigned nblk = (unsigned)((out_nodes + 255) / 256);
        const bool tp_steps = kn.tp_steps;      // the many-launch form also for short chains (cross-check)
        const bool tp_one = max_n <= TP_SMALL_MAX && !tp_steps;
        const int64_t tpn = tp_one ? 0 : out_nodes;                   // the per-node work arrays of the many-launch form
        DEVBUF(tp_seg, TpSeg, "tp_seg", segs.size()) DEVBUF(tp_up, int32_t, "tp_up", (size_t)2 * tpn)
        DEVBUF(tp_mark, uint8_t, "tp_mark", tpn) DEVBUF(tp_slots, int32_t, "tp_slots", tpn)
        DEVBUF(tp_ins, int32_t, "tp_ins", 2 * tpn) DEVBUF(tp_excl, int32_t, "tp_excl", tpn + 1)
        DEVBUF(tp_bsum, int32_t, "tp_bsum", nblk + 1) DEVBUF(tp_cnt, int32_t, "tp_cnt", segs.size())
        HT(c, hipMemcpyAsync(tp_seg, segs.data(), sizeof(TpSeg) * segs.size(), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_tail_init, dim3(t.init_blocks), dim3(256), 0, st, t.d_tracef, t.d_elim, out_nodes, t.d_nchanged, t.d_ngenes, NC,
                           tp_one ? (int32_t*)nullptr : tp_cnt, (int)segs.size());
        tail_inited = true;
        const TpWork tw{tp_seg, (int)segs.size(), out_nodes, levels, tp_up, tp_mark, tp_slots, tp_ins, tp_excl, tp_bsum, tp_cnt};
        const dim3 grid(nblk), blk(256);
        if (tp_one) {
            const int cap = (int)((max_n + 63) & ~63ll);
            hipLaunchKernelGGL(k_tp_small, dim3((unsigned)segs.size()), dim3(max_n <= 2048 ? 64 : 256), sizeof(int32_t) * 3 * (size_t)cap, st, tw, t.d_td, o,
                               t.d_tracef, t.d_elim, t.d_gene0, t.d_ngenes, cap);
        } else {
            hipLaunchKernelGGL(k_tp_init, grid, blk, 0, st, tw, t.d_td, o);
            // pointer jumping: 2^levels >= the longest chain; eight hops per launch while three levels or more are left (PGA_TP_JUMP8=0: doubling only)
            {
                const bool j8 = kn.tp_jump8;
                int k = 0;
                for (int left = levels; left > 0; k++) {
                    const int32_t* in = tp_up + (size_t)(k & 1) * out_nodes; int32_t* outp = tp_up + (size_t)((k + 1) & 1) * out_nodes;
                    if (j8 && left >= 3) { hipLaunchKernelGGL(k_tp_jump8, grid, blk, 0, st, tw, in, outp); left -= 3; }
                    else { hipLaunchKernelGGL(k_tp_jump, grid, blk, 0, st, tw, in, outp); left -= 1; }
                }
            }
            hipLaunchKernelGGL(k_tp_slots, grid, blk, 0, st, tw, t.d_td, o);
            hipLaunchKernelGGL(k_tp_scan1, grid, blk, 0, st, tw);
            hipLaunchKernelGGL(k_tp_scan2, dim3(1), dim3(1024), 0, st, tw, (int)nblk);
            hipLaunchKernelGGL(k_tp_scan3, grid, blk, 0, st, tw);
            hipLaunchKernelGGL(k_tp_fill, grid, blk, 0, st, tw, o, t.d_path);
            hipLaunchKernelGGL(k_tp_link, grid, blk, 0, st, tw, o, t.d_path, t.d_tracef);
            hipLaunchKernelGGL(k_tp_elim_a, grid, blk, 0, st, tw, t.d_td, o, t.d_path);
            hipLaunchKernelGGL(k_tp_elim_b, grid, blk, 0, st, tw, t.d_td, o, t.d_path, t.d_elim);
            // a workgroup per contig: wide for genomes, narrow when there are many short paths
            if (max_n >= 32768 && segs.size() <= 64 && !kn.tp_extract_one) {
                // genomes: a workgroup per chunk of 1024 path positions (k_tp_extract: one workgroup per contig, 400 rounds)
                const int chunks = (max_n + 1023) / 1024;
                DEVBUF(tp_xsum, TpChunkSum, "tp_xsum", (size_t)chunks * segs.size() + 1);
                const dim3 xg((unsigned)chunks, (unsigned)segs.size());
                hipLaunchKernelGGL(k_tp_extract_sum, xg, dim3(1024), 0, st, tw, t.d_td, o, t.d_path, t.d_elim, tp_xsum, chunks);
                hipLaunchKernelGGL(k_tp_extract_chunk, xg, dim3(1024), 0, st, tw, t.d_td, o, t.d_path, t.d_elim, (const TpChunkSum*)tp_xsum, chunks, t.d_gene0,
                                   t.d_ngenes);
            } else
                hipLaunchKernelGGL(k_tp_extract, dim3((unsigned)segs.size()), dim3(max_n >= 32768 ? 1024 : 256), 0, st, tw, t.d_td, o, t.d_path, t.d_elim,
                                   t.d_gene0, t.d_ngenes);
        }
    }
    // (no winning chain at all: the counters the tweaks read still start from zero)
    if (!tail_inited) hipLaunchKernelGGL(k_tail_init, dim3(t.init_blocks), dim3(256), 0, st, t.d_tracef, t.d_elim, out_nodes, t.d_nchanged, t.d_ngenes, NC, (int32_t*)nullptr, 0);
    return PGA_OK;
}

// the start tweaks of every gene and their fix-up; t.d_gene2 holds the final records afterwards
int FindCall::launch_tail_tweaks(TailBufs& t) {
    if (max_n >= 32768 && NC <= 1024)       // genomes: a wavefront per gene (at most n / 2 + 2 genes per contig)
        hipLaunchKernelGGL(k_tail_tweak_wave, dim3((unsigned)((max_n / 2 + 2 + 3) / 4), (unsigned)NC), dim3(256), 0, st, t.d_td, NC, o, t.d_tracef,
                           t.d_elim, t.d_gene0, t.d_gene1, t.d_ngenes, P.max_overlap, t.d_changed, t.d_nchanged);
    else if (NC >= 256 && !kn.tweak_slots) {   // many contigs: one thread per gene of the batch, packed
        DEVBUF(d_gpre, int32_t, "d_gene_prefix", NC + 2);
        hipLaunchKernelGGL(k_gene_prefix, dim3(1), dim3(1024), 0, st, t.d_ngenes, NC, d_gpre);
        hipLaunchKernelGGL(k_tail_tweak_packed, dim3(1024), dim3(256), 0, st, t.d_td, NC, o, t.d_tracef, t.d_elim, t.d_gene0, t.d_gene1, t.d_ngenes,
                           P.max_overlap, t.d_changed, t.d_nchanged, d_gpre);
    } else
        hipLaunchKernelGGL(k_tail_tweak, dim3((unsigned)((t.n_slots + 255) / 256)), dim3(256), 0, st, t.d_td, NC, t.n_slots, o, t.d_tracef, t.d_elim,
                           t.d_gene0, t.d_gene1, t.d_ngenes, P.max_overlap, t.d_changed, t.d_nchanged);
    DEVSET(t.d_gene2, GeneRec, "d_gene2", t.n_slots + 1);
    DEVBUF(d_chfin, uint8_t, "d_chfin", t.n_slots + 1);
    hipLaunchKernelGGL(k_tail_tweak_fixup, dim3(NC), dim3(max_n >= 32768 ? 1024 : 128), 0, st, t.d_td, NC, o, t.d_tracef, t.d_elim, t.d_gene0, t.d_gene1,
                       t.d_ngenes, P.max_overlap, t.d_changed, t.d_nchanged, t.d_gene2, d_chfin);
    return PGA_OK;
}

// ---- tail on the device: traceback untangling, bad-gene elimination, gene list, start tweaks ----------
// The tail is a pointer chase per contig.  PGA_TAIL=device: one device thread per contig; par (the default): launch_tail_paths.
int FindCall::run_device_tail(const bool par_tail) {
    tm->mark("gather");
    tdv.resize(NC);
    int64_t n_slots = 0;
    for (int i = 0; i < NC; i++) {
        const int k = win_chain[i];
        TailDesc& d = tdv[i];
        d.out_off = k >= 0 ? out_off[i] : 0; d.gene_off = n_slots;
        d.n = k >= 0 ? chains[k].n : 0; d.mx = k >= 0 ? h_maxidx[k] : -1;
        d.st_wt = k >= 0 ? c->models[chains[k].model].st_wt : 0.0;
        d.fin_off = k >= 0 ? fin_off[i] : 0; d.topo_off = k >= 0 ? chains[k].topo_off : 0;
        d.group = k >= 0 ? chains[k].group : 0; d._pad = 0;
        d.dp_off = k >= 0 ? chains[k].off : 0;
        n_slots += d.n / 2 + 2;
    }
    DEVBUF(d_td, TailDesc, "d_taildesc", NC + 1);
    DEVBUF(d_tracef, int32_t, "d_tracef", out_nodes + 1);
    DEVBUF(d_elim, uint8_t, "d_elim", out_nodes + 1);
    DEVBUF(d_gene0, GeneRec, "d_gene0", n_slots + 1);
    DEVBUF(d_gene1, GeneRec, "d_gene1", n_slots + 1);
    DEVBUF(d_ngenes, int32_t, "d_ngenes", NC + 1);
    DEVBUF(d_gbegin, int64_t, "d_gbegin", NC + 1);
    PINBUF(h_ngenes, int32_t, "h_ngenes", NC + 1);
    PINBUF(h_gbegin, int64_t, "h_gbegin", NC + 1);
    HT(c, hipMemcpyAsync(d_td, tdv.data(), sizeof(TailDesc) * NC, hipMemcpyHostToDevice, st));
    DEVBUF(d_path, int32_t, "d_path", out_nodes + 1);
    DEVBUF(d_changed, uint8_t, "d_changed", n_slots + 1);
    DEVBUF(d_nchanged, int32_t, "d_nchanged", NC + 1);
    TailBufs t{d_td, d_tracef, d_elim, d_gene0, d_gene1, nullptr, d_ngenes, d_path, d_changed, d_nchanged, n_slots,
               (unsigned)std::min<int64_t>(2048, (std::max<int64_t>(out_nodes, NC) + 256) / 256)};
    if (!par_tail) {
        hipLaunchKernelGGL(k_tail_init, dim3(t.init_blocks), dim3(256), 0, st, d_tracef, d_elim, out_nodes, d_nchanged, (int32_t*)nullptr, NC, (int32_t*)nullptr, 0);
        hipLaunchKernelGGL(k_tail_path, dim3((NC + 63) / 64), dim3(64), 0, st, d_td, NC, o, d_tracef, d_elim, d_path, d_gene0, d_ngenes);
    } else if (const int rc = launch_tail_paths(t)) return rc;
    if (const int rc = launch_tail_tweaks(t)) return rc;
    HT(c, hipMemcpyAsync(h_ngenes, d_ngenes, sizeof(int32_t) * NC, hipMemcpyDeviceToHost, st));
    if (const int rc = sync()) return rc;
    tm->mark("tail");
    // ---- results --------------------------------------------------------------------------------------
    const int64_t ngenes = contig_results(h_ngenes, h_gbegin);
    pga_gene* const genes_out = coding || keep ? nullptr : R->gene_records((size_t)ngenes, kn.pageable_results);
    pga_gene* d_genes = nullptr;
    if (ngenes > 0) {
        DEVBUF(d_genes_out, pga_gene, keep ? keep->buf : "d_genes_out", ngenes + 1);
        d_genes = d_genes_out;
        HT(c, hipMemcpyAsync(d_gbegin, h_gbegin, sizeof(int64_t) * NC, hipMemcpyHostToDevice, st));
        GcPtrs gcs{};
        for (int g = 0; g < NG; g++) gcs.p[g] = ga[g].gc_cont;
        hipLaunchKernelGGL(k_emit_genes, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, st, d_td, NC, n_slots, o, t.d_gene2, d_ngenes,
                           d_gbegin, P.meta ? 0 : 1, d_genes, lean_gather ? 1 : 0, ca, gcs);
        if (genes_out) HT(c, hipMemcpyAsync(genes_out, d_genes, sizeof(pga_gene) * (size_t)ngenes, hipMemcpyDeviceToHost, st));
        if (keep) { keep->d_genes = d_genes; keep->n_genes = ngenes; }
    }
    if (coding) {
        // the coverage of the resident records: one bit per base of the batch, then a popcount per contig; NC counts come back
        const int64_t words = total / 32 + 2;
        DEVBUF(d_cover, uint32_t, "d_cover", words);
        DEVBUF(d_coding, int64_t, "d_coding", NC + 1);
        PINBUF(h_coding, int64_t, "h_coding", NC + 1);
        HT(c, hipMemsetAsync(d_cover, 0, sizeof(uint32_t) * (size_t)words, st));
        if (ngenes > 0)
            hipLaunchKernelGGL(k_cover_genes, dim3((unsigned)((ngenes + 3) / 4)), dim3(256), 0, st, d_genes, ngenes, d_ct, NC, d_cover);
        hipLaunchKernelGGL(k_count_cover, dim3((unsigned)NC), dim3(256), 0, st, d_cover, d_ct, d_coding);
        HT(c, hipMemcpyAsync(h_coding, d_coding, sizeof(int64_t) * NC, hipMemcpyDeviceToHost, st));
        if (const int rc = sync()) return rc;
        memcpy(coding, h_coding, sizeof(int64_t) * NC);
    }
    if (P.want_nodes == 1 && out_nodes > 0) {
        tracef.resize((size_t)out_nodes + 1); elim.resize((size_t)out_nodes + 1);
        HT(c, hipMemcpyAsync(h.ndx, o.ndx, arena_all, hipMemcpyDeviceToHost, st));   // arena starts at `ndx`
        HT(c, hipMemcpyAsync(tracef.data(), d_tracef, sizeof(int32_t) * (size_t)out_nodes, hipMemcpyDeviceToHost, st));
        HT(c, hipMemcpyAsync(elim.data(), d_elim, (size_t)out_nodes, hipMemcpyDeviceToHost, st));
    }
    if (const int rc = stop_clock()) return rc;
    tm->mark("genes+d2h");
    return PGA_OK;
}

// the winners' node arrays for the caller (want_nodes 1)
int FindCall::copy_out_nodes() {
    R->nodes.resize(NC);
    for (int i = 0; i < NC; i++) {
        pga_nodes& N = R->nodes[i];
        memset(&N, 0, sizeof N);
        const int k = win_chain[i];
        if (k < 0) continue;
        const int n = chains[k].n; const int64_t oo = out_off[i];
        const bool single = !P.meta;
        if (int rc = alloc_nodes(R, N, n)) return rc;
        // single mode: nodes as left by the DP + eliminate_bad_genes (ref: lib.pyx:5296-5311); meta mode: fresh re-score, DP fields
        // reset (ref: lib.pyx:5380-5394)
        copy_node_topology(N, n, h.ndx + oo, h.stop_val + oo, h.type + oo, h.strand + oo, (single ? h.edge_dp : h.edge) + oo);
        const double* const src64[6] = {(single ? h.cscore_dp : h.cscore) + oo, (single ? h.sscore_dp : h.sscore) + oo, (single ? h.rscore_dp : h.rscore) + oo,
                                        (single ? h.uscore_dp : h.uscore) + oo, (single ? h.tscore_dp : h.tscore) + oo, h.mot_score + oo};
        copy_node_scores(N, n, src64, h.mot_ndx + oo, h.rbs + 2 * oo, h.mot_len + oo, h.mot_spacer + oo, h.mot_spacendx + oo, h.gc_cont + oo);
        if (single) {
            memcpy(N.score, h.score + oo, 8 * (size_t)n); memcpy(N.traceb, h.traceb + oo, 4 * (size_t)n); memcpy(N.tracef, tracef.data() + oo, 4 * (size_t)n);
            memcpy(N.ov_mark, h.ov_mark + oo, n); memcpy(N.elim, elim.data() + oo, n); memcpy(N.star_ptr, h.star_ptr + 3 * oo, 12 * (size_t)n);
        } else reset_dp_fields(N, n);
    }
    return PGA_OK;
}

// the arena stays on the device for pga_render_genes until the next finder call (want_nodes 1 and PGA_NODES_DEVICE)
void FindCall::keep_device_nodes() {
    DevNodes& D = c->dev_nodes;
    D.off.assign(NC, 0); D.n.assign(NC, 0); D.len.resize(NC);
    for (int i = 0; i < NC; i++) {
        D.len[i] = batch->ct[i].len;
        if (win_chain[i] >= 0) { D.off[i] = out_off[i]; D.n[i] = chains[win_chain[i]].n; }
    }
    D.total = out_nodes;
    const bool single = !P.meta;
    D.a = DevNodeArrays{o.ndx, o.stop_val, o.type, o.strand, o.gc_cont,
                        single ? o.edge_dp : o.edge, single ? o.cscore_dp : o.cscore, single ? o.sscore_dp : o.sscore,
                        single ? o.rscore_dp : o.rscore, single ? o.uscore_dp : o.uscore, single ? o.tscore_dp : o.tscore,
                        o.mot_score, o.mot_ndx, o.rbs, o.mot_len, o.mot_spacer};
    D.batch = batch;
    D.contigs = R->contigs.data();
}

}  // namespace

// The driver of every entry point: the phases of a call in order (FindCall above).
// stage 0 = the whole path; PGA_STAGE_* = stop after that stage and return the node arrays (single chain per
// contig scored with model 0; P.meta then only selects the meta-mode start penalties of Nodes.score)
// model_of_contig (single mode: the path and the SCORE / OVERLAP stages; nullptr = model 0 everywhere): contig i is scored with that
// loaded model, its nodes extracted under that model's translation table -- the groups of meta mode, one chain per contig.
// tt_of_contig (EXTRACT stage; nullptr = tt_override everywhere): contig i is extracted under that table.  At most 4 tables.
// coding (stage 0, single mode; nullptr otherwise): coding[i] = bases of contig i inside at least one of its genes, counted where the
// gene records are (pga_find_coding_bases); the records are then not copied back and the result holds no genes.
// keep (stage 0; nullptr otherwise): a pass of a circular call (circular.inl) -- the gene records stay on the device, in the buffer
// `keep->buf`, and the result holds none; `keep` reports where they are (nothing when the call found no node at all).
static int find_impl(const Knobs& kn, pga_ctx* c, const pga_batch* batch, const pga_params* pp, const int stage, const int tt_override, pga_result** out,
                     const int32_t* model_of_contig, const int32_t* tt_of_contig, int64_t* coding = nullptr, GeneKeep* keep = nullptr) {
    FindCall s;
    s.stage = stage; s.tt_override = tt_override; s.model_of_contig = model_of_contig; s.tt_of_contig = tt_of_contig; s.coding = coding; s.keep = keep;
    if (const int rc = s.check_call(kn, c, batch, pp, out)) return rc;
    StageTimer tm(kn.timing);
    s.tm = &tm;
    if (s.NC > 0 && s.total > 0) {
        if (const int rc = s.run_sequence_and_masks()) return rc;
        if (stage == PGA_STAGE_SEQUENCE) return s.return_sequence_stage(out);
        if (const int rc = s.run_extract()) return rc;
        tm.mark("extract+sync");
        if (const int rc = s.place_nodes()) return rc;
        if (const int rc = s.plan_chains()) return rc;
        if (const int rc = s.plan_connection_scoring()) return rc;
        if (const int rc = s.upload_plan()) return rc;
        tm.mark("plan+alloc");
        if (const int rc = s.score_groups()) return rc;
        if (stage != 0) return s.return_stage_nodes(out);
        if (const int rc = s.score_connections()) return rc;
        tm.mark("score+dp+sync");
        s.pick_winners();
        if (const int rc = s.rescore_winners()) return rc;
        tm.mark("winners+rescore_launch");
        if (const int rc = s.gather_winners()) return rc;
        // The tail (traceback untangling, bad-gene elimination, gene list, start tweaks) is a pointer chase per contig:
        // PGA_TAIL = host | device (one thread per contig) | par (tail.inl, the default)
        const bool device_tail = kn.tail != Knobs::host;
        if (keep && !device_tail) { c->err = "pga_find_genes: circular contigs are called with the device tail only (PGA_TAIL=host is set)"; return PGA_EINVAL; }
        if (const int rc = device_tail ? s.run_device_tail(kn.tail == Knobs::par) : s.run_host_tail()) return rc;
        if (s.P.want_nodes == 1) { if (const int rc = s.copy_out_nodes()) return rc; }
        if (s.P.want_nodes) s.keep_device_nodes();
    }
    tm.mark("results");
    return s.publish_result(out);
}


#include "train.inl"
#include "circular.inl"
#include "device_input.inl"
#include "terminal_repeat.inl"

extern "C" int pga_find_genes(pga_ctx* c, const pga_batch* batch, const pga_params* pp, pga_result** out) {
    const Knobs kn = read_knobs();
    const auto t0 = std::chrono::steady_clock::now();
    const bool circular = c && batch && batch->ctx == c && !batch->circular.empty();
    if (c) { c->last_cuts.clear(); c->set_model.clear(); c->set_score.clear(); c->model_scores.clear(); c->model_scores_nm = 0; }
    if (out) *out = nullptr;
    if (c && batch && pp && batch->ctx == c && !batch->sets.empty()) {
        if (circular) { c->err = "pga_find_genes: the batch carries both set labels (pga_batch_set_sets) and circular flags (pga_batch_set_circular)"; return PGA_EINVAL; }
        if (!pp->meta) { c->err = "pga_find_genes: set labels (pga_batch_set_sets) are a meta-mode feature (params->meta must be 1)"; return PGA_EINVAL; }
    }
    const int rc = circular ? find_circular(kn, c, batch, pp, out, nullptr) : find_impl(kn, c, batch, pp, 0, 0, out, nullptr, nullptr);
    if (kn.timing) fprintf(stderr, "[pga timing] pga_find_genes wall=%.2fms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return rc;
}

extern "C" int pga_nodes_stage(pga_ctx* c, const pga_batch* batch, const pga_params* pp, int stage, int translation_table, pga_result** out) {
    if (stage < PGA_STAGE_EXTRACT || stage > PGA_STAGE_SEQUENCE) {
        if (out) *out = nullptr;
        if (c) c->err = "pga_nodes_stage: unknown stage";
        return PGA_EINVAL;
    }
    return find_impl(read_knobs(), c, batch, pp, stage, translation_table, out, nullptr, nullptr);
}

extern "C" int pga_find_genes_models(pga_ctx* c, const pga_batch* batch, const pga_params* pp, const int32_t* model_of_contig, pga_result** out) {
    if (out) *out = nullptr;
    if (!c) return PGA_EINVAL;
    if (!batch || !pp || !out || !model_of_contig) { c->err = "pga_find_genes_models: bad arguments"; return PGA_EINVAL; }
    if (pp->meta) { c->err = "pga_find_genes_models: a model per contig is a single-mode call (params->meta must be 0)"; return PGA_EINVAL; }
    for (int i = 0; i < batch->n; i++)
        if (model_of_contig[i] < 0 || model_of_contig[i] >= c->n_models) {
            c->err = "pga_find_genes_models: contig " + std::to_string(i) + " names model " + std::to_string(model_of_contig[i]) + " of " +
                     std::to_string(c->n_models) + " loaded";
            return PGA_EINVAL;
        }
    c->last_cuts.clear(); c->set_model.clear(); c->set_score.clear(); c->model_scores.clear(); c->model_scores_nm = 0;
    if (batch->ctx == c && !batch->circular.empty() && !batch->sets.empty()) {
        c->err = "pga_find_genes_models: the batch carries both set labels (pga_batch_set_sets) and circular flags (pga_batch_set_circular)";
        return PGA_EINVAL;
    }
    const Knobs kn = read_knobs();
    if (batch->ctx == c && !batch->circular.empty()) return find_circular(kn, c, batch, pp, out, model_of_contig);
    return find_impl(kn, c, batch, pp, 0, 0, out, model_of_contig, nullptr);
}

extern "C" int pga_train(pga_ctx* c, const pga_batch* batch, const pga_params* pp, int translation_table, double start_weight,
                         int force_nonsd, int upto, pga_training* out) {
    if (!c) return PGA_EINVAL;
    if (!batch || batch->n != 1) { c->err = "pga_train: needs a batch of exactly one sequence"; return PGA_EINVAL; }
    const int32_t tt = translation_table, fn = force_nonsd;
    int32_t status = PGA_OK;
    const int rc = train_impl(c, batch, pp, &tt, &start_weight, &fn, upto <= 0 ? TR_ALL : upto, out, &status);
    if (rc != PGA_OK) return rc;
    if (status != PGA_OK) { c->err = "pga_train: no start / stop node in the sequence"; return status; }
    return PGA_OK;
}

extern "C" int pga_train_batch(pga_ctx* c, const pga_batch* batch, const pga_params* pp, const int32_t* translation_table,
                               const double* start_weight, const int32_t* force_nonsd, int upto, pga_training* out, int32_t* status) {
    return train_impl(c, batch, pp, translation_table, start_weight, force_nonsd, upto <= 0 ? TR_ALL : upto, out, status);
}

extern "C" int pga_find_coding_bases(pga_ctx* c, const pga_batch* batch, const pga_params* pp, const int32_t* model_of_contig,
                                     int64_t* coding_bases, int32_t* n_genes, double* score) {
    if (!c) return PGA_EINVAL;
    if (!batch || !pp || !model_of_contig || !coding_bases || !n_genes || !score) { c->err = "pga_find_coding_bases: bad arguments"; return PGA_EINVAL; }
    if (pp->meta) { c->err = "pga_find_coding_bases: a single-mode call (params->meta must be 0)"; return PGA_EINVAL; }
    for (int i = 0; i < batch->n; i++)
        if (model_of_contig[i] < 0 || model_of_contig[i] >= c->n_models) {
            c->err = "pga_find_coding_bases: contig " + std::to_string(i) + " names model " + std::to_string(model_of_contig[i]) + " of " +
                     std::to_string(c->n_models) + " loaded";
            return PGA_EINVAL;
        }
    for (int i = 0; i < batch->n; i++) { coding_bases[i] = 0; n_genes[i] = 0; score[i] = 0.0; }
    pga_params P = *pp;
    P.want_nodes = 0;                       // nothing of the nodes is kept or gathered for the host
    pga_result* r = nullptr;
    const int rc = find_impl(read_knobs(), c, batch, &P, 0, 0, &r, model_of_contig, nullptr, coding_bases);
    if (rc != PGA_OK) return rc;
    for (int i = 0; i < batch->n; i++) { n_genes[i] = r->contigs[i].n_genes; score[i] = r->contigs[i].score; }
    pga_result_free(r);
    return PGA_OK;
}

extern "C" int pga_batch_replicate(pga_ctx* c, const pga_batch* src, int32_t n, const int32_t* contig_of_entry, pga_batch** out) {
    if (out) *out = nullptr;
    if (!c) return PGA_EINVAL;
    if (!src || !out || n < 0 || (n > 0 && !contig_of_entry) || src->ctx != c) { c->err = "pga_batch_replicate: bad arguments"; return PGA_EINVAL; }
    for (int i = 0; i < n; i++)
        if (contig_of_entry[i] < 0 || contig_of_entry[i] >= src->n) {
            c->err = "pga_batch_replicate: entry " + std::to_string(i) + " names contig " + std::to_string(contig_of_entry[i]) + " of " +
                     std::to_string(src->n);
            return PGA_EINVAL;
        }
    if (!c->finder) { int rc = pga_finder_models_changed(c); if (rc) return rc; }
    HT(c, hipSetDevice(c->device));
    pga_batch* b = new (std::nothrow) pga_batch();
    if (!b) return PGA_ENOMEM;
    b->ctx = c; b->n = n; b->d_seq = nullptr; b->d_tiles = nullptr; b->d_tile0 = nullptr; b->n_tiles = 0; b->ct.resize((size_t)n + 1);
    int64_t total = 0;
    for (int i = 0; i < n; i++) { b->ct[i].base = total; b->ct[i].len = src->ct[contig_of_entry[i]].len; b->ct[i]._pad = 0; total += b->ct[i].len; }
    b->ct[n].base = total; b->ct[n].len = 0; b->ct[n]._pad = 0;
    b->total = total;
    if (total >= 0x7fffffffLL) { delete b; c->err = "pga_batch_replicate: batch larger than 2^31 bases; split it"; return PGA_EINVAL; }
    if (total > 0) {
        std::vector<TileDesc> tiles; std::vector<int32_t> tile0;
        batch_tiles(b, tiles, tile0);
        if (batch_take_dev(c, (size_t)total + 16 + batch_tiles_bytes(tiles, tile0), &b->d_seq, &b->d_seq_cap) != hipSuccess) { delete b; c->err = "pga_batch_replicate: hipMalloc failed"; return PGA_ENOMEM; }
        std::lock_guard<std::mutex> up(c->finder->up_mu);
        hipStream_t st = nullptr;
        { const int rc = upload_resources(c, 0, &st, nullptr); if (rc) { batch_give_dev(c, b->d_seq, b->d_seq_cap); delete b; return rc; } }
        // device to device, one copy per run of entries that are consecutive contigs of the source
        hipError_t e = hipSuccess;
        for (int i = 0; i < n && e == hipSuccess;) {
            int j = i + 1;
            while (j < n && contig_of_entry[j] == contig_of_entry[j - 1] + 1) j++;
            const ContigDesc& s0 = src->ct[contig_of_entry[i]];
            const int64_t bytes = b->ct[j].base - b->ct[i].base;
            if (bytes > 0) e = hipMemcpyAsync(b->d_seq + b->ct[i].base, src->d_seq + s0.base, (size_t)bytes, hipMemcpyDeviceToDevice, st);
            i = j;
        }
        if (e == hipSuccess) e = batch_upload_tiles(b, b->d_seq + total + 16, tiles, tile0, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) { batch_give_dev(c, b->d_seq, b->d_seq_cap); delete b; return pga_hip_try_(c, e, "replication of the batch"); }
    }
    // the mask sources and the topology travel with the contigs
    if (!src->circular.empty()) {
        bool any = false;
        for (int i = 0; i < n; i++) any = any || src->circular[contig_of_entry[i]];
        if (any) { b->circular.resize((size_t)n); for (int i = 0; i < n; i++) b->circular[i] = src->circular[contig_of_entry[i]]; }
    }
    if (!src->sets.empty()) { b->sets.resize((size_t)n); for (int i = 0; i < n; i++) b->sets[(size_t)i] = src->sets[(size_t)contig_of_entry[i]]; }
    b->mask_case = src->mask_case;
    if (!src->regions.empty()) {
        b->reg_off.assign((size_t)n + 1, 0);
        for (int i = 0; i < n; i++) {
            const int s = contig_of_entry[i];
            for (int32_t k = src->reg_off[s]; k < src->reg_off[s + 1]; k++) b->regions.push_back(MaskRun{i, src->regions[k].begin, src->regions[k].end, 0});
            b->reg_off[(size_t)i + 1] = (int32_t)b->regions.size();
        }
        if (b->regions.empty()) b->reg_off.clear();
        const int rc = batch_upload_regions(c, b);
        if (rc) { pga_batch_free(b); return rc; }
    }
    *out = b;
    return PGA_OK;
}

// ---- contig sets ----------------------------------------------------------------------------------------------------
extern "C" int pga_batch_set_sets(pga_batch* b, const int32_t* set_of_contig) {
    if (!b) return PGA_EINVAL;
    b->sets.clear();
    if (set_of_contig) {
        for (int i = 0; i < b->n; i++) if (set_of_contig[i] < -1) {
            if (b->ctx) b->ctx->err = "pga_batch_set_sets: contig " + std::to_string(i) + " carries label " + std::to_string(set_of_contig[i]) + " (a label is >= 0, -1 means on its own)";
            return PGA_EINVAL;
        }
        b->sets.assign(set_of_contig, set_of_contig + b->n);
    }
    return PGA_OK;
}

extern "C" int pga_set_choice(const pga_ctx* c, int32_t n, int32_t* model, double* score) {
    if (!c || n < 0 || (n > 0 && (!model || !score))) return PGA_EINVAL;
    for (int i = 0; i < n; i++) {
        const bool in = i < (int)c->set_model.size();
        model[i] = in ? c->set_model[(size_t)i] : -1;
        score[i] = in ? c->set_score[(size_t)i] : std::numeric_limits<double>::quiet_NaN();
    }
    return PGA_OK;
}

extern "C" int pga_model_scores(const pga_ctx* c, int32_t n_contigs, int32_t n_models, double* out) {
    if (!c || n_contigs < 0 || n_models < 0 || ((int64_t)n_contigs * n_models > 0 && !out)) return PGA_EINVAL;
    const int nm = c->model_scores_nm;
    const int64_t nc = nm > 0 ? (int64_t)(c->model_scores.size() / (size_t)nm) : 0;
    for (int64_t i = 0; i < n_contigs; i++)
        for (int m = 0; m < n_models; m++)
            out[i * n_models + m] = (i < nc && m < nm) ? c->model_scores[(size_t)(i * nm + m)] : std::numeric_limits<double>::quiet_NaN();
    return PGA_OK;
}
