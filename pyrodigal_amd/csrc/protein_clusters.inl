// Near-identical proteins clustered on the device from their sketches (pga_cluster_sketches; the rule is in pyrodigal_amd.h, DESIGN.md
// 4.21).  Included by translate.hip, inside its anonymous namespace, behind protein_sketches.inl: the pair comparison is sk_pair, the one
// k_sketch_pairs calls.  Every record has `probes` slots, T = G probes in all, and every array below is laid out by slot: a stable radix
// sort of (hash, record) makes the buckets, a second sort of one packed pair per slot makes the candidates distinct and ordered, a wave
// per candidate decides it, and a lock-free union-find joins the accepted ones.  Nothing is compacted before the edges themselves: a
// slot that holds nothing carries a key that sorts behind every real one.  All integer; every atomic is a max, a min, an add or a
// compare-and-swap whose outcome does not depend on the order of arrival.

constexpr uint64_t kClBias = 1ull << 63;                       // int64 -> uint64, order kept
constexpr uint32_t kClNone = 0xffffffffu;                      // the record of a slot that probes nothing

struct ClArgs {
    const int64_t* sketch; const int64_t* count; const int64_t* weight;      // [G, s], [G], [G] or nullptr: all equal
    int64_t n, slots;                                          // G, T
    int32_t s, probes, num, den, min_union, _pad;
    uint64_t* key; uint64_t* skey;                             // [T] the probes' hashes, biased; sorted.  Then: the pair keys; sorted
    uint32_t* idx; uint32_t* sidx;                             // [T] the probes' records; sorted.  idx then: (shared, m) of an accepted slot
    uint32_t* start; uint32_t* runstart;                       // [T] i at a bucket's first slot, else 0; its running maximum.  Then: accepted?; its scan
    unsigned long long* wmax; uint32_t* centre;                // [T] at a bucket's first slot: the greatest weight, biased; the centre
    int32_t* parent; int32_t* root; int32_t* isroot; int32_t* number; int32_t* cnt;      // [G]
    unsigned long long* rw; uint32_t* rep;                     // [G] at a root: the greatest weight of the cluster, biased; its representative
    unsigned long long* small;                                 // [0] edges, [1] clusters, [2] distinct candidates, [3] probes
    int64_t* d_cluster; int64_t* d_rep; int64_t* d_size;
    int64_t* d_edges; int64_t* d_eshared; int64_t* d_eunion; int64_t edge_capacity;
};

__device__ __forceinline__ unsigned long long cl_weight(const ClArgs& a, const uint32_t g) {
    return (unsigned long long)a.weight[g] ^ kClBias;
}

// what the waves of a workgroup counted, added to *dst by one atomic per workgroup: tens of thousands of atomics on one address, one
// per wave, took longer than the rest of the kernel.  Every thread of the workgroup calls it; `mine` is the wave's, lane 0 adds it.
__device__ __forceinline__ void cl_count(unsigned long long* dst, const unsigned long long mine, unsigned long long* blk) {
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(blk, mine);
    __syncthreads();
    if (threadIdx.x == 0 && *blk) atomicAdd(dst, *blk);
}

// (a) one slot per thread, row-major, in a loop: slot g probes + j holds hash j of record g when the record probes with it
__global__ void __launch_bounds__(kRowThreads)
k_cluster_probes(const ClArgs a) {
    __shared__ unsigned long long blk;
    if (threadIdx.x == 0) blk = 0;
    __syncthreads();
    unsigned long long probing = 0;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < a.slots; i0 += (int64_t)gridDim.x * blockDim.x) {      // (i0 is the workgroup's)
        const int64_t i = i0 + threadIdx.x;
        bool valid = false;
        if (i < a.slots) {
            const int64_t g = i / a.probes;
            const int j = (int)(i - g * a.probes);
            const int c = (int)min(max(a.count[g], (int64_t)0), (int64_t)a.s);
            valid = j < min(a.probes, c);
            a.key[i] = valid ? (uint64_t)a.sketch[g * a.s + j] ^ kClBias : ~0ull;
            a.idx[i] = valid ? (uint32_t)g : kClNone;
            if (j == 0) { a.parent[g] = (int32_t)g; a.cnt[g] = 0; a.rw[g] = 0ull; a.rep[g] = kClNone; }
        }
        probing += __popcll(__ballot(valid));
    }
    cl_count(&a.small[3], probing, &blk);
}

// (b) the buckets: runs of equal keys.  A slot that probes nothing has the key of a genuine INT64_MAX hash and may lie inside that run: it
// is told apart by its record, kClNone, and takes no part in what follows.
__global__ void __launch_bounds__(kRowThreads)
k_cluster_heads(const ClArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.slots) return;
    a.start[i] = i == 0 || a.skey[i] != a.skey[i - 1] ? (uint32_t)i : 0u;
}
// the centre of every bucket: the greatest weight first (PASS 0, skipped when all weights are equal), then the smallest record that has it
template <int PASS>
__global__ void __launch_bounds__(kRowThreads)
k_cluster_centre(const ClArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.slots) return;
    const uint32_t g = a.sidx[i];
    if (g == kClNone) return;
    const uint32_t rs = a.runstart[i];
    if (PASS == 0) atomicMax(&a.wmax[rs], cl_weight(a, g));
    else if (!a.weight || cl_weight(a, g) == a.wmax[rs]) atomicMin(&a.centre[rs], g);
}

// (c) one key per slot: (a << 32 | b), a < b, for a member and its bucket's centre; (G << 32), which sorts behind them all, for a centre
// and for a slot that probes nothing
__global__ void __launch_bounds__(kRowThreads)
k_cluster_pairs(const ClArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.slots) return;
    const uint32_t g = a.sidx[i];
    uint64_t k = (uint64_t)a.n << 32;
    if (g != kClNone) {
        const uint32_t c = a.centre[a.runstart[i]];
        if (c != g) k = ((uint64_t)min(c, g) << 32) | max(c, g);
    }
    a.key[i] = k;
}

// (d) A wave takes 64 sorted slots at a time, in a loop: a slot is a candidate when it holds a pair and is the first of its key.  The
// candidates of the step -- a ballot -- are compared one after the other by the whole wave.
__global__ void __launch_bounds__(kRowThreads)
k_cluster_accept(const ClArgs a) {
    __shared__ unsigned long long blk;
    if (threadIdx.x == 0) blk = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t per = kRowThreads / 64;
    unsigned long long seen = 0;
    for (int64_t i0 = ((int64_t)blockIdx.x * per + threadIdx.x / 64) * 64; i0 < a.slots; i0 += (int64_t)gridDim.x * per * 64) {      // (i0 is the wave's)
        const int64_t i = i0 + lane;
        const uint64_t k = i < a.slots ? a.skey[i] : ~0ull;
        const bool live = i < a.slots && (int64_t)(k >> 32) < a.n && (i == 0 || a.skey[i - 1] != k);
        uint32_t ok = 0, info = 0;
        unsigned long long todo = __ballot(live);
        seen += __popcll(todo);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint64_t kk = (uint64_t)sk_lane((int64_t)k, src);
            int shared, m;
            sk_pair(a.sketch, a.count, a.s, (int64_t)(kk >> 32), (int64_t)(kk & 0xffffffffull), lane, shared, m);
            if (lane == src) {
                ok = m >= max(a.min_union, 1) && (int64_t)shared * a.den >= (int64_t)a.num * m ? 1u : 0u;
                info = (uint32_t)shared | ((uint32_t)m << 8);
            }
        }
        if (i < a.slots) { a.start[i] = ok; a.idx[i] = info; }
    }
    cl_count(&a.small[2], seen, &blk);
}

// (e) Union-find over the records.  parent[x] <= x always, and the only write that changes a root is a compare-and-swap that hangs it
// under a smaller record: the root of a tree is its smallest member.
// cl_find ends: every step goes to a strictly smaller record.  The loads are atomic at agent scope: another XCD's swap is seen.
__device__ __forceinline__ int cl_find(int32_t* parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p >= x) return x;
        x = p;
    }
}
// cl_unite ends: it waits for nobody.  A swap fails only because another thread's swap on the same root succeeded, and at most G - 1
// swaps succeed in a launch (each makes one root fewer), so a thread goes round at most G times whatever the scheduling.
__device__ __forceinline__ void cl_unite(int32_t* parent, int x, int y) {
    for (;;) {
        x = cl_find(parent, x);
        y = cl_find(parent, y);
        if (x == y) return;
        if (x < y) { const int t = x; x = y; y = t; }          // the larger root goes under the smaller
        const int old = atomicCAS(&parent[x], x, y);
        if (old == x) return;
        x = old;                                               // (x had been hung elsewhere: on from there)
    }
}

// the accepted slots, in sorted order: the edge goes out when there is room for it, and joins its two records either way
__global__ void __launch_bounds__(kRowThreads)
k_cluster_edges(const ClArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.slots) return;
    const uint32_t ok = a.start[i];
    const int64_t p = (int64_t)a.runstart[i];
    if (i == a.slots - 1) a.small[0] = (unsigned long long)(p + ok);
    if (!ok) return;
    const uint64_t k = a.skey[i];
    const int x = (int)(k >> 32), y = (int)(k & 0xffffffffull);
    if (a.d_edges && p < a.edge_capacity) {
        const uint32_t info = a.idx[i];
        a.d_edges[2 * p] = x; a.d_edges[2 * p + 1] = y;
        a.d_eshared[p] = info & 0xffu; a.d_eunion[p] = info >> 8;
    }
    cl_unite(a.parent, x, y);
}

// The root of every record, with path halving: a record on the way is hung under its grandparent.  Every value ever stored in parent[x]
// is an ancestor of x and smaller than x, whoever stored it and whichever of two racing stores lands, so the walk goes to strictly
// smaller records and ends at the root -- which no store of this kernel touches -- after at most G steps.
__global__ void __launch_bounds__(kRowThreads)
k_cluster_flatten(const ClArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    int x = (int)g;
    for (;;) {
        const int p = __hip_atomic_load(&a.parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p >= x) break;
        const int q = __hip_atomic_load(&a.parent[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (q >= p) { x = p; break; }
        __hip_atomic_store(&a.parent[x], q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = q;
    }
    a.root[g] = x;
    a.isroot[g] = x == (int)g ? 1 : 0;
}

// (f) numbering: the roots are the clusters' smallest members, so a scan over "is root" numbers the clusters in the rule's order
__global__ void __launch_bounds__(kRowThreads)
k_cluster_number(const ClArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    const int r = a.root[g];
    a.d_cluster[g] = a.number[r];
    if (a.d_size) atomicAdd(&a.cnt[r], 1);
    if (a.d_rep && a.weight) atomicMax(&a.rw[r], cl_weight(a, (uint32_t)g));
    if (g == a.n - 1) a.small[1] = (unsigned long long)((int64_t)a.number[g] + a.isroot[g]);
}
__global__ void __launch_bounds__(kRowThreads)
k_cluster_representative(const ClArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    const int r = a.root[g];
    if (!a.weight || cl_weight(a, (uint32_t)g) == a.rw[r]) atomicMin(&a.rep[r], (uint32_t)g);
}
__global__ void __launch_bounds__(kRowThreads)
k_cluster_emit(const ClArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n || !a.isroot[g]) return;
    if (a.d_rep) a.d_rep[a.number[g]] = a.rep[g];
    if (a.d_size) a.d_size[a.number[g]] = a.cnt[g];
}
