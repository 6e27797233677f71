// Device helpers shared by dp.hip, dp_wave.hip and pipeline.hip: the ones that need intrinsics (the scalar rules of connection
// scoring -- sel3, igm_apart, igm_same, the window start -- are in dpw_core.h, which the host model compiles too).
#pragma once
#include "pga_internal.h"

// v of lane `lane`, the same in every lane (two v_readlane)
__device__ __forceinline__ double readlane_f64(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane), __builtin_amdgcn_readlane(__double2loint(v), lane));
}

// Cross-lane moves through the data-parallel primitives of the vector ALU (DPP) instead of ds_bpermute: a lone wavefront waits out
// the full LDS round trip of every __shfl, six of them in a row per scan, and these scans sit on the serial path of a chain.
// CTRL: 0x111 .. 0x11f row_shr:1 .. 15, 0x138 wave_shr:1, 0x142 row_bcast15, 0x143 row_bcast31, 0x140 row_mirror, 0x141 row_half_mirror,
// quad_perm otherwise.  Lanes that receive nothing (shifted in from outside the row, or masked out by ROW_MASK) get `old`.
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_f64(const double old, const double v) {
    const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ int dpp_i32(const int old, const int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, false); }

// wave-wide minimum of an int, the same in every lane
__device__ __forceinline__ int wave_min_i32(int v) {
    const int BIG = 0x7fffffff;
    v = min(v, dpp_i32<0xb1>(BIG, v));             // quad_perm [1, 0, 3, 2]
    v = min(v, dpp_i32<0x4e>(BIG, v));             // quad_perm [2, 3, 0, 1]
    v = min(v, dpp_i32<0x141>(BIG, v));            // row_half_mirror
    v = min(v, dpp_i32<0x140>(BIG, v));            // row_mirror: every lane holds its row's minimum
    v = min(v, dpp_i32<0x142, 0xa>(BIG, v));       // row_bcast15 into rows 1 and 3
    v = min(v, dpp_i32<0x143, 0xc>(BIG, v));       // row_bcast31 into rows 2 and 3: lane 63 holds the minimum
    return __builtin_amdgcn_readlane(v, 63);
}

// Lexicographic (value, index) order: ties go to the larger index.  Its maximum is the reference's ascending ">=" scan
// (ref: _connection.h:135-139) in a form that does not depend on the order of the candidates, so partial maxima over disjoint
// source sets merge exactly.
__device__ __forceinline__ bool lex_gt(const double ov, const int oi, const double v, const int i) { return ov > v || (ov == v && oi > i); }
__device__ __forceinline__ void lex_max(double& v, int& i, const double ov, const int oi) {
    const bool c = lex_gt(ov, oi, v, i);
    v = c ? ov : v; i = c ? oi : i;
}
// The same over the lanes whose numbers differ in the bits LO .. HI (powers of two) only, by xor butterfly: <1, 4> leaves every
// lane the maximum of its block of 8, <8, 32> after that the wave's, <1, 32> the wave's at once.  `carry`: further values of the
// lane that holds the maximum.  Every lane of the wave must call it.
template <int LO, int HI, class... Carry>
__device__ __forceinline__ void wave_lexmax(double& v, int& i, Carry&... carry) {
#pragma unroll
    for (int m = LO; m <= HI; m <<= 1) {
        const double ov = __shfl_xor(v, m, 64); const int oi = __shfl_xor(i, m, 64);
        auto other = [m](const auto x) { return __shfl_xor(x, m, 64); };
        auto sel = [](const bool c, const auto a, const auto b) { return c ? a : b; };
        const bool c = lex_gt(ov, oi, v, i);
        ((carry = sel(c, other(carry), carry)), ...);
        lex_max(v, i, ov, oi);
    }
}

// chain containing global chain-node index g (chains sorted by off)
__device__ __forceinline__ int find_chain(const ChainDesc* __restrict__ chains, int n_chains, int64_t g) {
    int lo = 0, hi = n_chains - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chains[mid].off <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The last index in [0, n) whose key is <= x (keys ascend, key(0) <= x), found by ONE WAVEFRONT together: every lane probes one of 64
// evenly spaced positions of what is left of the range, a ballot narrows it 64-fold -- three rounds of one load each for 262 144
// entries, where the binary search of a lone thread is eighteen dependent loads in front of everything the workgroup does (round 6:
// k_ovl_stops, a workgroup of 256 short threads, spent a third of its life there).  All 64 lanes of the wavefront must call it.
template <class Key>
__device__ __forceinline__ int wave_search_le(const Key key, const int n, const int64_t x) {
    const int lane = threadIdx.x & 63;
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int step = (hi - lo + 63) >> 6;
        const int idx = min(lo + (lane + 1) * step, hi);           // (lane 63 probes hi)
        const int cnt = __popcll(__ballot((int64_t)key(idx) <= x));      // a prefix of the lanes
        const int nlo = cnt ? min(lo + cnt * step, hi) : lo;
        if (cnt < 64) hi = min(lo + (cnt + 1) * step, hi) - 1;
        lo = nlo;
    }
    return lo;
}
// ... once per workgroup (its first wavefront), the result in *s_slot for everybody (barrier inside: every thread must call it)
template <class Key>
__device__ __forceinline__ int block_search_le(const Key key, const int n, const int64_t x, int* s_slot) {
    if (threadIdx.x < 64) { const int r = wave_search_le(key, n, x); if (threadIdx.x == 0) *s_slot = r; }
    __syncthreads();
    return *s_slot;
}

// The same for every thread of a workgroup whose first element is block_first: one search per workgroup (its first wavefront), then
// a short forward walk per thread (a workgroup rarely spans more than two chains) -- a search per thread is sixteen dependent
// loads that nothing hides.  Every thread of the workgroup must call it (barrier inside).
__device__ __forceinline__ int find_chain_block(const ChainDesc* __restrict__ chains, int n_chains, int64_t block_first, int64_t g, int* s_slot) {
    int c = block_search_le([&](const int k) { return chains[k].off; }, n_chains, block_first, s_slot);
    while (c + 1 < n_chains && chains[c + 1].off <= g) c++;
    return c;
}
