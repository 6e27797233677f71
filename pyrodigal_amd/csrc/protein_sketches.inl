// Bottom-s MinHash sketches of predicted proteins, or of the genes' nucleotides, and their pairwise comparison (pga_sketch_proteins,
// pga_sketch_pairs; the rule is in pyrodigal_amd.h).  Included by translate.hip, inside its anonymous namespace,
// behind protein_groups.inl: the strings are those of pga_group_proteins, read through its GrpRow and grp_unit<UNIT>.  A wave keeps the
// sketch of its record sorted, one element per lane, and inserts only what passes the largest element kept: no sort, no LDS.

constexpr int64_t kSkNone = INT64_MAX;                         // what a sketch row holds behind its count
constexpr int kSkSkip = 255;                                   // the class of a letter that no window may hold

struct SkArgs {
    GrpArgs g;                                                 // seq, row, n, unk and strict: what grp_unit reads
    const uint8_t* classes;                                    // [128] the class of a residue letter (protein unit)
    int32_t k, s, bits, _pad;
    uint64_t salt;                                             // (seed + 1) * 0x9E3779B97F4A7C15 mod 2^64
    int64_t* d_sketch; int64_t* d_count; int64_t* d_windows;   // [G, s], [G], [G] or nullptr
    unsigned long long* passed;                                // PGA_SKETCH_COUNT_PASSES builds: insertions tried, or nullptr
};

// the finaliser of splitmix64 over key + salt, shifted into a non-negative int64
__device__ __forceinline__ int64_t sk_hash(const uint64_t x, const uint64_t salt) {
    uint64_t z = x + salt;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (int64_t)(z >> 1);
}

// Values across the wave without the LDS crossbar that __shfl goes through -- the insertion loop below is nothing but such moves.
// v of lane `src`, src being the same in every lane: two v_readlane
__device__ __forceinline__ int64_t sk_lane(const int64_t v, const int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), src);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
constexpr int kDppWaveShl1 = 0x130, kDppWaveShr1 = 0x138;    // DPP controls of gfx9: the whole wave moved by one lane
// every lane takes its lower neighbour's value, lane 0 keeps its own: two DPP moves
__device__ __forceinline__ int64_t sk_up1(const int64_t v) {
    const int lo = (int)(uint32_t)v, hi = (int)(uint32_t)((uint64_t)v >> 32);
    const uint32_t l = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, kDppWaveShr1, 0xf, 0xf, false);
    const uint32_t h = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, kDppWaveShr1, 0xf, 0xf, false);
    return (int64_t)(((uint64_t)h << 32) | l);
}
// every lane takes its upper neighbour's value, lane 63 takes `in`: one DPP move
__device__ __forceinline__ int sk_down1(const int v, const int in) {
    return __builtin_amdgcn_update_dpp(in, v, kDppWaveShl1, 0xf, 0xf, false);
}

// the code of unit x of a record's string, kSkSkip for a letter that is skipped and for x beyond the string
template <int UNIT>
__device__ __forceinline__ int sk_code(const SkArgs& a, const GrpRow& w, const int x) {
    if (x >= w.n) return kSkSkip;
    const int r = grp_unit<UNIT>(a.g, w, x);
    if (UNIT == kGrpGene) return r == 'A' ? 0 : r == 'C' ? 1 : r == 'G' ? 2 : r == 'T' ? 3 : kSkSkip;
    return r >= 128 ? kSkSkip : (int)a.classes[r];
}

// The sketch of every record.  Work is dealt by wave over the records, in a loop.  The wave holds the sketch so far sorted, lane i < cnt
// the i-th smallest hash and every other lane kSkNone; tau, the value of lane s - 1, is what a hash must stay below once the sketch is
// full.  A step takes 64 consecutive windows: lane l has the code of unit j0 + l (`cur`) and of unit j0 + 64 + l (`nxt`, the next
// step's `cur`: every unit is read once), the letters of window j0 + l come past lane l as the 128 codes move down one lane k times,
// and whether the window is valid follows from the two ballots of skipped letters.  The candidates of a step -- a ballot -- are inserted
// one after the other by the whole wave: an equal element drops it, otherwise the lanes above its rank take their lower neighbour's
// value.  The hash comes from its lane and tau from lane s - 1 by v_readlane, so what decides an insertion is scalar.  The first step
// of a record ranks its hashes instead (below).
template <int UNIT>
__global__ void __launch_bounds__(kRowThreads)
k_sketch(const SkArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t per = kRowThreads / 64;
    const int k = a.k, s = a.s, bits = a.bits;
    const uint64_t kmask = k >= 64 ? ~0ull : (1ull << k) - 1;
    for (int64_t g = (int64_t)blockIdx.x * per + threadIdx.x / 64; g < a.g.n; g += (int64_t)gridDim.x * per) {      // (g is the wave's)
        const GrpRow w = a.g.row[g];
        const int nwin = w.n - k + 1;                          // windows of the record, valid or not
        int64_t v = kSkNone;
        int cnt = 0;
        long long windows = 0;
        int nxt = nwin > 0 ? sk_code<UNIT>(a, w, lane) : kSkSkip;
        for (int j0 = 0; j0 < nwin; j0 += 64) {
            const int cur = nxt;
            nxt = sk_code<UNIT>(a, w, j0 + 64 + lane);
            const unsigned long long skip0 = __ballot(cur == kSkSkip), skip1 = __ballot(nxt == kSkSkip);
            const unsigned long long over = (skip0 >> lane) | (lane ? skip1 << (64 - lane) : 0ull);      // the letters from this window on
            const bool valid = j0 + lane < nwin && (over & kmask) == 0;
            uint64_t x = 0;
            uint32_t c = (uint32_t)cur;                        // after i moves: the code of unit j0 + lane + i
            for (int i = 0; i < k; i++) {
                x = (x << bits) | c;
                c = (uint32_t)sk_down1((int)c, __builtin_amdgcn_readlane(nxt, i));
            }
            const int64_t h = sk_hash(x, a.salt);
            const unsigned long long vmask = __ballot(valid);
            windows += __popcll(vmask);
            if (j0 == 0) {
                // The first step meets an empty sketch: every one of its hashes would be inserted, most of them only to be pushed out
                // again.  Instead every lane counts the distinct hashes below its own -- hash after hash comes round as a scalar; one
                // that a lower lane holds too is a duplicate and is neither counted nor placed -- and the hashes go to the lanes of
                // their ranks in one permutation, duplicates and invalid windows behind the distinct ones.
                unsigned long long dup = 0;
                int rank = 0;
                for (unsigned long long todo = vmask; todo;) {
                    const int m = __ffsll((long long)todo) - 1;
                    todo &= todo - 1;
                    const int64_t hm = sk_lane(h, m);
                    dup |= __ballot(h == hm) & vmask & ~((2ull << m) - 1);      // (2 << 63 is 0: no lane above lane 63)
                    if ((dup >> m) & 1) continue;
                    rank += hm < h ? 1 : 0;
                }
                const unsigned long long distinct = vmask & ~dup;
                const int D = __popcll(distinct);
                const bool mine = (distinct >> lane) & 1;
                const int dest = mine ? rank : D + __popcll(~distinct & ((1ull << lane) - 1));
                const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_permute(dest << 2, (int)(uint32_t)h);
                const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_permute(dest << 2, (int)(uint32_t)((uint64_t)h >> 32));
                cnt = min(D, s);
                v = lane < cnt ? (int64_t)(((uint64_t)hi << 32) | lo) : kSkNone;
                continue;
            }
            int64_t tau = sk_lane(v, s - 1);
            unsigned long long todo = __ballot(valid && (cnt < s || h < tau));
            while (todo) {
                const int src = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const int64_t hn = sk_lane(h, src);
                if (cnt == s && hn >= tau) continue;           // (tau fell since the ballot)
#ifdef PGA_SKETCH_COUNT_PASSES
                if (a.passed && lane == 0) atomicAdd(a.passed, 1ull);
#endif
                if (__ballot(lane < cnt && v == hn)) continue;
                const int rank = __popcll(__ballot(lane < cnt && v < hn));
                const int64_t below = sk_up1(v);
                if (lane > rank) v = below;
                if (lane == rank) v = hn;
                if (lane >= s) v = kSkNone;
                if (cnt < s) cnt++;
                tau = sk_lane(v, s - 1);
            }
        }
        if (lane < s) a.d_sketch[g * s + lane] = lane < cnt ? v : kSkNone;
        if (lane == 0) {
            a.d_count[g] = cnt;
            if (a.d_windows) a.d_windows[g] = windows;
        }
    }
}

struct SkPairArgs {
    const int64_t* sketch; const int64_t* count;               // [G, s], [G]
    const int64_t* pairs;                                      // [P, 2]
    int64_t n_genes, n_pairs;
    int32_t s, _pad;
    int64_t* d_shared; int64_t* d_union;                       // [P]
};

// the number of the first `n` elements of a sorted row (lane i holds element i) that are less than x: a binary search over shuffled
// values, seven halvings for n <= 64, every lane in every shuffle
__device__ __forceinline__ int sk_lower(const int64_t row, const int n, const int64_t x) {
    int lo = 0, hi = n;
#pragma unroll
    for (int it = 0; it < 7; it++) {
        const int mid = (lo + hi) >> 1;
        const int64_t m = __shfl(row, mid & 63);
        if (lo < hi) { if (m < x) lo = mid + 1; else hi = mid; }
    }
    return lo;
}

// (shared, m) of rows ia and ib, by a whole wave, the same in every lane (k_sketch_pairs, and k_cluster_accept of protein_clusters.inl).
// Lane i holds A[i] and B[i], both rows ascending and distinct.  An element of A lies in B where the search finds it; its rank in the
// distinct union is its index, plus the elements of B below it, less the common elements below it (a ballot's low bits, A being
// sorted).  |U| = |A| + |B| - common, m = min(s, |U|), shared = the common elements of rank < m.
__device__ __forceinline__ void sk_pair(const int64_t* __restrict__ sketch, const int64_t* __restrict__ count, const int s, const int64_t ia,
                                        const int64_t ib, const int lane, int& shared, int& m) {
    const int ca = (int)min(max(count[ia], (int64_t)0), (int64_t)s), cb = (int)min(max(count[ib], (int64_t)0), (int64_t)s);
    const int64_t A = lane < ca ? sketch[ia * s + lane] : kSkNone;
    const int64_t B = lane < cb ? sketch[ib * s + lane] : kSkNone;
    const int lb = sk_lower(B, cb, A);                         // elements of B below A[lane]
    const int64_t at = __shfl(B, lb & 63);
    const bool common = lane < ca && lb < cb && at == A;
    const unsigned long long cmask = __ballot(common);
    m = min(s, ca + cb - __popcll(cmask));
    const int rank = lane + lb - __popcll(cmask & ((1ull << lane) - 1));
    shared = __popcll(__ballot(common && rank < m));
}

// One pair per wave, in a loop.
__global__ void __launch_bounds__(kRowThreads)
k_sketch_pairs(const SkPairArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t per = kRowThreads / 64;
    for (int64_t p = (int64_t)blockIdx.x * per + threadIdx.x / 64; p < a.n_pairs; p += (int64_t)gridDim.x * per) {
        const int64_t ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
        if (ia < 0 || ia >= a.n_genes || ib < 0 || ib >= a.n_genes) {
            if (lane == 0) { a.d_shared[p] = -1; a.d_union[p] = -1; }
            continue;
        }
        int shared, m;
        sk_pair(a.sketch, a.count, a.s, ia, ib, lane, shared, m);
        if (lane == 0) { a.d_shared[p] = shared; a.d_union[p] = m; }
    }
}
