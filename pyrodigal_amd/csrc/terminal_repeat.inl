// Direct terminal repeats: a contig whose first r letters are also its last r letters is a circle that the assembler
// wrote out with the overlap twice.  k_terminal_repeat finds the longest such r of every searched contig on the resident batch,
// k_tr_compact writes the batch without the second copy; the circular call (circular.inl) does the rest.  Included by finder.hip.

constexpr int kTrThreads = 256;
constexpr int kTrChunk = 4 * kTrThreads;                       // letters of each window a workgroup hashes per step: a 32-bit word per thread
constexpr uint32_t kTrP1 = 2147483647u, kTrP2 = 2147483629u;    // 2^31 - 1 and 2^31 - 19: the two largest primes below 2^31
constexpr uint32_t kTrX1 = 1000003u, kTrX2 = 998244353u % 2147483629u;

template <uint32_t P> __host__ __device__ __forceinline__ uint32_t tr_mul(const uint32_t a, const uint32_t b) { return (uint32_t)(((uint64_t)a * b) % P); }
template <uint32_t P> __host__ __device__ __forceinline__ uint32_t tr_add(const uint32_t a, const uint32_t b) { const uint32_t s = a + b; return s >= P ? s - P : s; }   // a, b < 2^31: no wrap

// Four letters of a word -> 1 A, 2 G, 3 C, 4 T (either case) and `unk` for anything else, byte-parallel as digits4 (pipeline.hip) does it
// and with its reading of the letters (digit_of).  The two windows get different `unk`: an unknown letter matches nothing.
__device__ __forceinline__ void tr_masks4(const uint32_t w, uint32_t& a, uint32_t& g, uint32_t& c, uint32_t& t) {      // 0x01 in the bytes that hold the base
    const uint32_t u = w & 0xdfdfdfdfu;
    auto eq = [](const uint32_t v) { return (~(((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) | v | 0x7f7f7f7fu)) >> 7; };
    a = eq(u ^ 0x41414141u); g = eq(u ^ 0x47474747u); c = eq(u ^ 0x43434343u); t = eq(u ^ 0x54545454u);
}
__device__ __forceinline__ uint32_t tr_codes4(const uint32_t w, const uint32_t unk) {
    uint32_t a, g, c, t;
    tr_masks4(w, a, g, c, t);
    const uint32_t n = ~(a | g | c | t) & 0x01010101u;
    return a + 2u * g + 3u * c + 4u * t + unk * n;
}
// bytes [0, nb) of a 16-byte piece, as a mask of each of its four words (nb >= 16: all of them)
__device__ __forceinline__ uint32_t tr_word_mask(const int nb, const int q) {
    const int v = nb - 4 * q;
    return v >= 4 ? 0xffffffffu : v <= 0 ? 0u : (1u << (8 * v)) - 1u;
}

// One modulus of the two: the running hashes of both windows up to the chunk, and the powers the scans need.
//   F(r) = sum_{j < r} p[j] x^j            p[j] = code of S[j]             (a sum: letters join at the high end)
//   G(r) = sum_{j < r} q[L - r + j] x^j    q = code of the suffix window   (Horner: a letter joins at the low end, G(r + 1) = G(r) x + q[L - r - 1])
// Both are the polynomial of the same r letters when S[0:r] matches S[L-r:L], letter by letter.
template <uint32_t P, uint32_t X>
struct TrHash {
    uint32_t F = 0, G = 0;          // F(r0), G(r0) of the chunk that starts at r0
    uint32_t xr0 = 1;               // x^r0
    uint32_t f, g;                  // the thread's values at its first letter, after scan()
    uint32_t xp;                    // x^(its first letter)
    // x^(4 * 2^k): the length of 2^k threads' letters
    static __device__ __forceinline__ uint32_t xd(const int k) { uint32_t v = tr_mul<P>(tr_mul<P>(X, X), tr_mul<P>(X, X)); for (int i = 0; i < k; i++) v = tr_mul<P>(v, v); return v; }
    // the thread's eight letters (pw[k], sw[k]: letter 4 t + k of the prefix chunk, of the suffix chunk read backwards) join the scans
    __device__ __forceinline__ void scan(const uint32_t pw, const uint32_t sw, const int lane, const int wave, uint32_t* s_f, uint32_t* s_g) {
        uint32_t xl = 1;                                          // x^(4 lane)
#pragma unroll
        for (int k = 0; k < 6; k++) if (lane >> k & 1) xl = tr_mul<P>(xl, xd(k));
        const uint32_t xw = wave == 0 ? 1u : wave == 1 ? xd(6) : wave == 2 ? xd(7) : tr_mul<P>(xd(6), xd(7));      // x^(256 wave)
        xp = tr_mul<P>(tr_mul<P>(xr0, xw), xl);
        const uint32_t p0 = pw & 255u, p1 = pw >> 8 & 255u, p2 = pw >> 16 & 255u, p3 = pw >> 24;
        const uint32_t q0 = sw & 255u, q1 = sw >> 8 & 255u, q2 = sw >> 16 & 255u, q3 = sw >> 24;
        // the thread's own stretch
        uint32_t fs = tr_add<P>(tr_mul<P>(tr_add<P>(tr_mul<P>(tr_add<P>(tr_mul<P>(p3, X), p2), X), p1), X), p0);     // p0 + p1 x + p2 x^2 + p3 x^3
        fs = tr_mul<P>(fs, xp);
        uint32_t gs = tr_add<P>(tr_mul<P>(tr_add<P>(tr_mul<P>(tr_add<P>(tr_mul<P>(q0, X), q1), X), q2), X), q3);     // ((q0 x + q1) x + q2) x + q3
        // inclusive scans over the wavefront: a lane that has a neighbour d lanes below holds exactly d stretches, 4 d letters
#pragma unroll
        for (int k = 0; k < 6; k++) {
            const int d = 1 << k;
            const uint32_t of = __shfl_up(fs, d, 64), og = __shfl_up(gs, d, 64);
            if (lane >= d) { fs = tr_add<P>(fs, of); gs = tr_add<P>(tr_mul<P>(og, xd(k)), gs); }
        }
        if (lane == 63) { s_f[wave] = fs; s_g[wave] = gs; }
        uint32_t fe = __shfl_up(fs, 1, 64), ge = __shfl_up(gs, 1, 64);      // exclusive
        if (lane == 0) { fe = 0; ge = 0; }
        __syncthreads();
        // across the workgroup: the four wavefronts' totals, in order
        uint32_t fw = F, gw = G, fall = F, gall = G;
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const uint32_t tf = s_f[v], tg = s_g[v];
            fall = tr_add<P>(fall, tf); gall = tr_add<P>(tr_mul<P>(gall, xd(6)), tg);
            if (v < wave) { fw = fall; gw = gall; }
        }
        f = tr_add<P>(fw, fe);
        g = tr_add<P>(tr_mul<P>(gw, xl), ge);
        F = fall; G = gall; xr0 = tr_mul<P>(xr0, xd(8));
    }
    // ... and the thread steps over its four letters: after step k, f == F(r) and g == G(r) for r = its first letter + k + 1
    __device__ __forceinline__ void step(const uint32_t p, const uint32_t q) {
        f = tr_add<P>(f, tr_mul<P>(p, xp));
        xp = tr_mul<P>(xp, X);
        g = tr_add<P>(tr_mul<P>(g, X), q);
    }
};

// A workgroup per searched contig that is long enough to hold a repeat: list[b] is its index in the batch.
//   1. the two windows S[0:W] and S[L-W:L] go by in chunks of kTrChunk letters, the suffix window backwards; the hashes F(r) and G(r)
//      of every r of the chunk come out of two scans (shuffles in the wavefront, LDS across the four of them) under two moduli;
//      the largest r below `limit` where both agree is the candidate;
//   2. the candidate is compared letter by letter, 16 bytes per thread and step.  It holds: that is the match.  It does not: a hash
//      collision; step 1 runs again for the r below it.  The answer is always that of the comparison;
//   3. the four bases of S[0:match] are counted for the low-complexity rule.
__global__ void __launch_bounds__(kTrThreads)
k_terminal_repeat(const char* __restrict__ seq, const ContigDesc* __restrict__ ct, const int32_t* __restrict__ list, const int32_t min_len,
                  const int32_t max_len, const int32_t max_pct, int32_t* __restrict__ match_out, int32_t* __restrict__ trim_out) {
    __shared__ uint32_t s_f[2][4], s_g[2][4];                 // [modulus][wavefront]: the totals of a chunk
    __shared__ int s_best;
    __shared__ int s_cnt[4];
    const int ci = list[blockIdx.x], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ContigDesc cd = ct[ci];
    const int32_t L = cd.len;
    const char* const S = seq + cd.base;
    const int32_t W = min(max_len, L / 2);
    int32_t match = 0;
    int32_t limit = W + 1;                                     // only r < limit is still open
    while (limit > min_len) {                                  // (uniform: once, and once more per hash collision)
        if (tid == 0) s_best = 0;
        int32_t best = 0;
        TrHash<kTrP1, kTrX1> h1;
        TrHash<kTrP2, kTrX2> h2;
        const int32_t top = limit - 1;
        for (int32_t r0 = 0; r0 < top; r0 += kTrChunk) {
            const int32_t i0 = r0 + 4 * tid;                   // the thread's letters: i0 .. i0 + 3 of the prefix, L - 1 - i0 .. L - 4 - i0 of the record
            uint32_t pw = 0, sw = 0;
            if (i0 + 4 <= W) {
                __builtin_memcpy(&pw, S + i0, 4);
                uint32_t t;
                __builtin_memcpy(&t, S + (L - 4 - i0), 4);
                sw = __builtin_bswap32(t);                     // backwards: byte k is letter L - 1 - i0 - k
            } else {
                for (int k = 0; k < 4; k++) if (i0 + k < W) {
                    pw |= (uint32_t)(uint8_t)S[i0 + k] << (8 * k);
                    sw |= (uint32_t)(uint8_t)S[L - 1 - i0 - k] << (8 * k);
                }
            }
            pw = tr_codes4(pw, 5u); sw = tr_codes4(sw, 6u);
            h1.scan(pw, sw, lane, wave, s_f[0], s_g[0]);        // (a barrier in each: the totals of one are read before the other's barrier,
            h2.scan(pw, sw, lane, wave, s_f[1], s_g[1]);        //  so a chunk's totals are never written over while they are read)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t p = pw >> (8 * k) & 255u, q = sw >> (8 * k) & 255u;
                h1.step(p, q); h2.step(p, q);
                const int32_t r = i0 + k + 1;
                if (r >= min_len && r <= top && h1.f == h1.g && h2.f == h2.g) best = r;
            }
        }
        for (int d = 32; d > 0; d >>= 1) best = max(best, __shfl_down(best, d, 64));
        __syncthreads();                                       // s_best is zero
        if (lane == 0 && best > 0) atomicMax(&s_best, best);
        __syncthreads();
        const int32_t r = s_best;
        __syncthreads();                                       // (read by all before the next round zeroes it)
        if (r == 0) break;
        // the comparison: S[j] against S[L - r + j], 4096 letters a step, until one differs
        int bad = 0;
        for (int32_t j0 = 0; j0 < r && !bad; j0 += 16 * kTrThreads) {
            const int32_t j = j0 + 16 * tid;
            int mine = 0;
            if (j < r) {
                uint4 a, b;                                     // (a load may run up to 15 bytes past the contig: the batch has 16 behind its letters)
                __builtin_memcpy(&a, S + j, 16);
                __builtin_memcpy(&b, S + (L - r) + j, 16);
                const int nb = r - j;
                const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int q = 0; q < 4; q++) mine |= ((tr_codes4(aw[q], 5u) ^ tr_codes4(bw[q], 6u)) & tr_word_mask(nb, q)) != 0;
            }
            bad = __syncthreads_or(mine);
        }
        if (!bad) { match = r; break; }
        limit = r;
    }
    // the most frequent base of the repeat
    int32_t trim = match;
    if (match > 0) {
        if (tid < 4) s_cnt[tid] = 0;
        __syncthreads();
        int na = 0, ng = 0, nc = 0, nt = 0;
        for (int32_t j = 16 * tid; j < match; j += 16 * kTrThreads) {
            uint4 a;
            __builtin_memcpy(&a, S + j, 16);
            const int nb = match - j;
            const uint32_t aw[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t ma, mg, mc, mt;
                tr_masks4(aw[q], ma, mg, mc, mt);
                const uint32_t m = tr_word_mask(nb, q);
                na += __popc(ma & m); ng += __popc(mg & m); nc += __popc(mc & m); nt += __popc(mt & m);
            }
        }
        for (int d = 32; d > 0; d >>= 1) { na += __shfl_down(na, d, 64); ng += __shfl_down(ng, d, 64); nc += __shfl_down(nc, d, 64); nt += __shfl_down(nt, d, 64); }
        if (lane == 0) { atomicAdd(&s_cnt[0], na); atomicAdd(&s_cnt[1], ng); atomicAdd(&s_cnt[2], nc); atomicAdd(&s_cnt[3], nt); }
        __syncthreads();
        const int32_t top = max(max(s_cnt[0], s_cnt[1]), max(s_cnt[2], s_cnt[3]));
        if ((int64_t)100 * top > (int64_t)max_pct * match) trim = 0;
    }
    if (tid == 0) { match_out[ci] = match; trim_out[ci] = trim; }
}

// ---- the batch without the second copies -------------------------------------------------------------------------------------------
// Contig i of the new batch is S[0 : len - trim] of contig i of the old one.  As k_circ_rotate: a thread per 16 bytes of the destination
// (its allocation is 256-byte aligned); where they lie in one contig they are one 16-byte load at whatever alignment the source has and
// one aligned 16-byte store, the few at a seam go letter by letter.
__global__ void __launch_bounds__(256)
k_tr_compact(const char* __restrict__ src, const ContigDesc* __restrict__ sct, const ContigDesc* __restrict__ dct, const int n, const int64_t total,
             char* __restrict__ dst) {
    const int64_t q0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (q0 >= total) return;
    const int64_t q1 = q0 + 16 < total ? q0 + 16 : total;
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (dct[mid].base <= q0) lo = mid; else hi = mid - 1; }
    int j = lo;
    ContigDesc d = dct[j];
    if (q1 - q0 == 16 && q0 - d.base + 16 <= d.len) {
        uint4 v;
        __builtin_memcpy(&v, src + sct[j].base + (q0 - d.base), 16);
        *reinterpret_cast<uint4*>(dst + q0) = v;
        return;
    }
    for (int64_t q = q0; q < q1; q++) {
        while (q >= d.base + d.len) { j++; d = dct[j]; }         // (empty contigs are stepped over; q < total ends it)
        dst[q] = src[sct[j].base + (q - d.base)];
    }
}

extern "C" int pga_terminal_repeat_chunk(void) { return kTrChunk; }

extern "C" int pga_batch_terminal_repeats(pga_ctx* c, const pga_batch* batch, const uint8_t* search, int32_t min_length, int32_t max_length,
                                          int32_t max_base_percent, int32_t* match_out, int32_t* trim_out) {
    if (!c) return PGA_EINVAL;
    if (!batch || batch->ctx != c || (batch->n > 0 && (!match_out || !trim_out))) { c->err = "pga_batch_terminal_repeats: bad arguments"; return PGA_EINVAL; }
    if (!(1 <= min_length && min_length <= max_length && max_length <= 1048576)) {
        c->err = "pga_batch_terminal_repeats: 1 <= min_length <= max_length <= 1048576 does not hold for " + std::to_string(min_length) + ", " + std::to_string(max_length);
        return PGA_EINVAL;
    }
    if (!(25 <= max_base_percent && max_base_percent <= 100)) {
        c->err = "pga_batch_terminal_repeats: max_base_percent " + std::to_string(max_base_percent) + " is not in 25 .. 100";
        return PGA_EINVAL;
    }
    const int n = batch->n;
    std::vector<int32_t> list;                                  // the searched contigs that can hold a repeat of min_length
    for (int i = 0; i < n; i++) {
        match_out[i] = 0; trim_out[i] = 0;
        if ((!search || search[i]) && batch->ct[i].len / 2 >= min_length) list.push_back(i);
    }
    if (list.empty()) return PGA_OK;
    const int nl = (int)list.size();
    hipStream_t st = c->stream;
    HT(c, hipSetDevice(c->device));
    DEVBUF(d_ct, ContigDesc, "tr_ct", n + 1);
    DEVBUF(d_list, int32_t, "tr_list", nl);
    DEVBUF(d_out, int32_t, "tr_out", 2 * (size_t)n);
    PINBUF(h_out, int32_t, "h_tr_out", 2 * (size_t)n);
    HT(c, hipMemcpyAsync(d_ct, batch->ct.data(), sizeof(ContigDesc) * ((size_t)n + 1), hipMemcpyHostToDevice, st));
    HT(c, hipMemcpyAsync(d_list, list.data(), sizeof(int32_t) * (size_t)nl, hipMemcpyHostToDevice, st));
    HT(c, hipMemsetAsync(d_out, 0, sizeof(int32_t) * 2 * (size_t)n, st));
    hipLaunchKernelGGL(k_terminal_repeat, dim3((unsigned)nl), dim3(kTrThreads), 0, st, batch->d_seq, d_ct, d_list, min_length, max_length, max_base_percent,
                       d_out, d_out + n);
    HT(c, hipGetLastError());
    HT(c, hipMemcpyAsync(h_out, d_out, sizeof(int32_t) * 2 * (size_t)n, hipMemcpyDeviceToHost, st));      // 8 n bytes: all that comes back
    HT(c, hipStreamSynchronize(st));
    memcpy(match_out, h_out, sizeof(int32_t) * (size_t)n);
    memcpy(trim_out, h_out + n, sizeof(int32_t) * (size_t)n);
    return PGA_OK;
}

extern "C" int pga_batch_trim_terminal_repeats(pga_ctx* c, const pga_batch* src, const int32_t* trim, pga_batch** out) {
    if (out) *out = nullptr;
    if (!c) return PGA_EINVAL;
    if (!src || !out || src->ctx != c || (src->n > 0 && !trim)) { c->err = "pga_batch_trim_terminal_repeats: bad arguments"; return PGA_EINVAL; }
    const int n = src->n;
    bool any = false;
    for (int i = 0; i < n; i++) {
        if (trim[i] < 0 || 2 * (int64_t)trim[i] > src->ct[i].len) {
            c->err = "pga_batch_trim_terminal_repeats: contig " + std::to_string(i) + " of " + std::to_string(src->ct[i].len) + " bases cannot lose " +
                     std::to_string(trim[i]) + " (0 <= trim and 2 trim <= length)";
            return PGA_EINVAL;
        }
        any = any || trim[i] > 0;
    }
    if (!any) return PGA_OK;                                     // nothing to take off: the caller goes on with src
    HT(c, hipSetDevice(c->device));
    pga_batch* b = new (std::nothrow) pga_batch();
    if (!b) return PGA_ENOMEM;
    struct BatchGuard { pga_batch* b; ~BatchGuard() { pga_batch_free(b); } } guard{b};
    b->ctx = c; b->n = n; b->d_seq = nullptr; b->d_tiles = nullptr; b->d_tile0 = nullptr; b->n_tiles = 0; b->ct.resize((size_t)n + 1);
    int64_t total = 0;
    for (int i = 0; i < n; i++) { b->ct[i].base = total; b->ct[i].len = src->ct[i].len - trim[i]; b->ct[i]._pad = 0; total += b->ct[i].len; }
    b->ct[n].base = total; b->ct[n].len = 0; b->ct[n]._pad = 0;
    b->total = total;
    if (total > 0) {
        hipStream_t st = c->stream;
        std::vector<TileDesc> tiles; std::vector<int32_t> tile0;
        batch_tiles(b, tiles, tile0);
        if (batch_take_dev(c, (size_t)total + 16 + batch_tiles_bytes(tiles, tile0), &b->d_seq, &b->d_seq_cap) != hipSuccess) {
            (void)hipGetLastError(); c->err = "pga_batch_trim_terminal_repeats: hipMalloc failed"; return PGA_ENOMEM;
        }
        DEVBUF(d_sct, ContigDesc, "tr_ct", n + 1);
        DEVBUF(d_dct, ContigDesc, "tr_ct2", n + 1);
        HT(c, hipMemcpyAsync(d_sct, src->ct.data(), sizeof(ContigDesc) * ((size_t)n + 1), hipMemcpyHostToDevice, st));
        HT(c, hipMemcpyAsync(d_dct, b->ct.data(), sizeof(ContigDesc) * ((size_t)n + 1), hipMemcpyHostToDevice, st));
        HT(c, batch_upload_tiles(b, b->d_seq + total + 16, tiles, tile0, st));
        hipLaunchKernelGGL(k_tr_compact, dim3((unsigned)(((total + 15) / 16 + 255) / 256)), dim3(256), 0, st, src->d_seq, d_sct, d_dct, n, total, b->d_seq);
        HT(c, hipGetLastError());
        HT(c, hipStreamSynchronize(st));                         // (the staging vectors go out of use)
    }
    // what travels with the contigs: a trimmed contig is a circle; the caller's regions end where the contig now ends
    b->circular.resize((size_t)n);
    for (int i = 0; i < n; i++) b->circular[i] = (trim[i] > 0 || (!src->circular.empty() && src->circular[i])) ? 1 : 0;
    b->sets = src->sets;
    b->mask_case = src->mask_case;
    if (!src->regions.empty()) {
        b->reg_off.assign((size_t)n + 1, 0);
        for (int i = 0; i < n; i++) {
            for (int32_t k = src->reg_off[i]; k < src->reg_off[i + 1]; k++) {
                const int32_t rb = src->regions[k].begin, re = std::min(src->regions[k].end, b->ct[i].len);
                if (rb < re) b->regions.push_back(MaskRun{i, rb, re, 0});
            }
            b->reg_off[(size_t)i + 1] = (int32_t)b->regions.size();
        }
        if (b->regions.empty()) b->reg_off.clear();
        const int rc = batch_upload_regions(c, b);
        if (rc) return rc;
    }
    guard.b = nullptr;
    *out = b;
    return PGA_OK;
}
