// Edges verified against the rows themselves (pga_align_pairs, pga_cluster_edges; the rule is in pyrodigal_amd.h).
// Included by translate.hip, inside its anonymous namespace, behind protein_clusters.inl: the components are its union-find, its
// numbering and its representatives.  The edit distance is a wave per pair over the band |j - i| <= K, K = max_distance: the wave
// walks the anti-diagonals s = i + j of the DP matrix, and a lane holds R consecutive diagonals d = j - i of the band.  Cell (i, j)
// needs (i - 1, j) and (i, j - 1) of step s - 1 -- the two neighbouring diagonals -- and (i - 1, j - 1) of step s - 2, its own
// diagonal.  A diagonal holds a cell only at every other step, so ONE value per diagonal, the last one computed there, is both "step
// s - 1" for its neighbours and "step s - 2" for itself: the diagonals of the other parity are not written at step s.  All integer;
// every value is clamped to K + 1, so nothing can wrap.

constexpr int kAlSteps = 128;                                  // anti-diagonals per staged chunk of the two rows

struct AlArgs {
    const void* tokens;                                        // element 0 of the caller's tensor
    const int64_t* begin; const int64_t* len;                  // [G] the rows
    const int64_t* pairs;                                      // [P, 2]
    int64_t n_rows, n_pairs;
    int32_t K, num, den, _pad;
    int64_t* d_distance; int64_t* d_pass;                      // [P]; [P] or nullptr
    unsigned long long* small;                                 // [0] decided without a DP, [1] ran the DP, [2] passed
};

// every lane takes its lower neighbour's value, lane 0 takes `in`: one DPP move (the counterpart of sk_down1)
__device__ __forceinline__ int al_up1(const int v, const int in) {
    return __builtin_amdgcn_update_dpp(in, v, kDppWaveShr1, 0xf, 0xf, false);
}

// min(ed(A, B), K + 1) of rows whose lengths differ by at most K, by a whole wave, the same in every lane.  R * 64 >= 2 K + 1: lane l
// holds the diagonals t = l R .. l R + R - 1 of the band, d = t - K; those at or beyond 2 K + 1 are never written and stay K + 1, and
// so do the values that come in over the two ends of the wave.  A cell (i, j) inside the matrix with i, j >= 1 has its three
// neighbours inside the matrix, so a diagonal's value is read only at a step right after (or two after) it was written.
// The rows are staged in the wave's own LDS a chunk of kAlSteps steps at a time: at step s the band touches i, j in
// [(s - K) / 2, (s + K) / 2], so a chunk that begins at s0 needs the elements lo .. lo + kAlSteps / 2 + K of either row,
// lo = floor((s0 - K) / 2) - 1, which is CW = kAlSteps / 2 + 32 R elements or fewer.
// Loops: the chunks and their steps together are the la + lb + 1 anti-diagonals; the fill is CW / 64 rounds.
template <typename T, int R>
__device__ __forceinline__ int al_band(const T* __restrict__ A, const int la, const T* __restrict__ B, const int lb, const int K, const int lane,
                                       T* const sa, T* const sb) {
    constexpr int CW = kAlSteps / 2 + 32 * R;
    const int INF = K + 1, W = 2 * K + 1;
    int v[R];
#pragma unroll
    for (int r = 0; r < R; r++) v[r] = INF;
    const int64_t S = (int64_t)la + lb + 1;
    const int dl = lane * R - K;                               // the diagonal of the lane's first slot
    for (int64_t s0 = 0; s0 < S; s0 += kAlSteps) {
        const int lo = (int)((s0 - K) >> 1) - 1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");      // (the last chunk's reads are done before it is overwritten)
        __builtin_amdgcn_wave_barrier();
        for (int k = lane; k < CW; k += 64) {
            const int64_t x = (int64_t)lo + k;
            sa[k] = x >= 0 && x < la ? A[x] : T(0);
            sb[k] = x >= 0 && x < lb ? B[x] : T(0);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
        // slot r of this lane at step s0 + u holds the cell i = (s0 + u + K - lane R - r) / 2, j = i + d, when that is whole
        const int64_t cb = s0 + K - (int64_t)lane * R;
        const int hb = (int)(cb >> 1), pb = (int)(cb & 1);
        const int nu = (int)min((int64_t)kAlSteps, S - s0);
        for (int u = 0; u < nu; u++) {
            const int pu = pb + u;
            const int left = al_up1(v[R - 1], INF), right = sk_down1(v[0], INF);
            auto cell = [&](const int r) {
                const int e = pu - r;
                const int i = hb + (e >> 1), j = i + dl + r;
                const bool ok = !(e & 1) && (unsigned)i <= (unsigned)la && (unsigned)j <= (unsigned)lb && lane * R + r < W;
                // (an index the chunk does not hold belongs to a cell that is not `ok`: it reads the chunk's last element instead)
                const unsigned oa = min((unsigned)(i - 1 - lo), (unsigned)(CW - 1)), ob = min((unsigned)(j - 1 - lo), (unsigned)(CW - 1));
                const int cost = sa[oa] != sb[ob] ? 1 : 0;
                const int up = r > 0 ? v[r > 0 ? r - 1 : 0] : left, dn = r < R - 1 ? v[r < R - 1 ? r + 1 : 0] : right;
                int val = min(min(v[r] + cost, up + 1), dn + 1);
                if (i == 0) val = j;
                if (j == 0) val = i;
                if (ok) v[r] = min(val, INF);
            };
            if (R == 1) cell(0);
            else if (__builtin_amdgcn_readfirstlane(pu) & 1) {     // (lane R is even: the parity is the wave's)
#pragma unroll
                for (int r = 1; r < R; r += 2) cell(r);
            } else {
#pragma unroll
                for (int r = 0; r < R; r += 2) cell(r);
            }
            int least = v[0];
#pragma unroll
            for (int r = 1; r < R; r++) least = min(least, v[r]);
            if (!__ballot(least <= K)) return INF;                 // every cell of the last two steps is beyond K: so is every later one
        }
    }
    const int ts = lb - la + K;                                    // the diagonal of (la, lb): written last at step la + lb
    int sel = v[0];
#pragma unroll
    for (int r = 1; r < R; r++) if (ts % R == r) sel = v[r];
    return __shfl(sel, ts / R);
}

// One pair per wave, in a loop.  Whatever decides a pair is the same in every lane of its wave.
template <int EB, int R>
__global__ void __launch_bounds__(kRowThreads)
k_align_pairs(const AlArgs a) {
    using T = typename TokElem<EB>::type;
    constexpr int CW = kAlSteps / 2 + 32 * R;
    __shared__ T rows[kRowThreads / 64][2][CW];
    __shared__ unsigned long long blk[3];
    if (threadIdx.x < 3) blk[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
    const int64_t per = kRowThreads / 64;
    const T* const tok = (const T*)a.tokens;
    unsigned long long quick = 0, ran = 0, passed = 0;
    for (int64_t p = (int64_t)blockIdx.x * per + wave; p < a.n_pairs; p += (int64_t)gridDim.x * per) {
        const int64_t ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
        if (ia < 0 || ia >= a.n_rows || ib < 0 || ib >= a.n_rows) {
            if (lane == 0) { a.d_distance[p] = -1; if (a.d_pass) a.d_pass[p] = 0; }
            quick++;
            continue;
        }
        const int64_t la = a.len[ia], lb = a.len[ib];
        int64_t dist;
        if (ia == ib) { dist = 0; quick++; }
        else if (la - lb > a.K || lb - la > a.K) { dist = a.K + 1; quick++; }
        else { dist = al_band<T, R>(tok + a.begin[ia], (int)la, tok + a.begin[ib], (int)lb, a.K, lane, rows[wave][0], rows[wave][1]); ran++; }
        const bool pass = dist <= a.K && dist * a.den <= (int64_t)(a.den - a.num) * max(la, lb);
        passed += pass ? 1 : 0;
        if (lane == 0) { a.d_distance[p] = dist; if (a.d_pass) a.d_pass[p] = pass ? 1 : 0; }
    }
    cl_count(&a.small[0], quick, &blk[0]);
    cl_count(&a.small[1], ran, &blk[1]);
    cl_count(&a.small[2], passed, &blk[2]);
}

// ---- the components of a caller's edges (pga_cluster_edges): what k_cluster_probes leaves of every record, and the joins ----
__global__ void __launch_bounds__(kRowThreads)
k_edges_reset(const ClArgs a) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= a.n) return;
    a.parent[g] = (int32_t)g; a.cnt[g] = 0; a.rw[g] = 0ull; a.rep[g] = kClNone;
}
// an edge per thread, in a loop: a kept edge with both records inside 0 .. n - 1 is counted (small[0]) and joins them (cl_unite: it
// waits for nobody, and parent[x] <= x throughout)
__global__ void __launch_bounds__(kRowThreads)
k_edges_join(const ClArgs a, const int64_t* __restrict__ edges, const int64_t* __restrict__ keep, const int64_t n_edges) {
    __shared__ unsigned long long blk;
    if (threadIdx.x == 0) blk = 0;
    __syncthreads();
    unsigned long long used = 0;
    for (int64_t e0 = (int64_t)blockIdx.x * blockDim.x; e0 < n_edges; e0 += (int64_t)gridDim.x * blockDim.x) {      // (e0 is the workgroup's)
        const int64_t e = e0 + threadIdx.x;
        bool use = false;
        if (e < n_edges && (!keep || keep[e] != 0)) {
            const int64_t x = edges[2 * e], y = edges[2 * e + 1];
            use = x >= 0 && x < a.n && y >= 0 && y < a.n;
            if (use && x != y) cl_unite(a.parent, (int)x, (int)y);
        }
        used += __popcll(__ballot(use));
    }
    cl_count(&a.small[0], used, &blk);
}
