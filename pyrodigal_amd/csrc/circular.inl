// Circular contigs: a contig flagged circular (pga_batch_set_circular) is called twice by the unchanged linear finder.
// Pass 1 is the ordinary call on the whole batch; its gene records stay on the device and only say where NOT to cut: the widest
// stretch no gene covers, in the middle half of the record.  Pass 2 calls the contig rotated to start at that cut, closed; its records
// are mapped back to the record's coordinates (a gene across the origin ends beyond the contig's length) and spliced, on the device,
// into the records pass 1 found for the linear contigs of the batch.  Included by finder.hip behind find_impl.

// ---- the cut rule (host arithmetic; the device kernels below implement the same order) ------------------------------------------
// a gap [gb, gb + w) of a contig of L bases; mid = gb + w / 2 (= (gb + ge) / 2)
__host__ __device__ __forceinline__ bool circ_gap_inner(const int32_t gb, const int32_t w, const int32_t L) {
    const int32_t mid = gb + w / 2;
    return mid >= L / 4 && mid < L - L / 4;
}
// is gap a a better place to cut than gap b (w == 0: no gap): wider; then closer to L / 2; then lower
__host__ __device__ __forceinline__ bool circ_gap_better(const int32_t agb, const int32_t aw, const int32_t bgb, const int32_t bw, const int32_t L) {
    if (aw != bw) return aw > bw;
    if (aw == 0) return false;
    const int32_t am = agb + aw / 2, bm = bgb + bw / 2;
    const int32_t ad = am > L / 2 ? am - L / 2 : L / 2 - am, bd = bm > L / 2 ? bm - L / 2 : L / 2 - bm;
    if (ad != bd) return ad < bd;
    return am < bm;
}

extern "C" int pga_circular_cut(int32_t L, int32_t n, const int32_t* begin, const int32_t* end) {
    if (L < 0 || n < 0 || (n > 0 && (!begin || !end))) return PGA_EINVAL;
    std::vector<std::pair<int32_t, int32_t>> iv;          // covered, 0-based half-open, clipped to the contig
    for (int i = 0; i < n; i++) {
        const int32_t b = std::max(begin[i], 1) - 1, e = std::min(end[i], L);
        if (b < e) iv.emplace_back(b, e);
    }
    std::sort(iv.begin(), iv.end());
    int32_t in_gb = 0, in_w = 0, any_gb = 0, any_w = 0;
    auto gap = [&](const int32_t gb, const int32_t ge) {
        if (ge <= gb) return;
        if (circ_gap_inner(gb, ge - gb, L) && circ_gap_better(gb, ge - gb, in_gb, in_w, L)) { in_gb = gb; in_w = ge - gb; }
        if (circ_gap_better(gb, ge - gb, any_gb, any_w, L)) { any_gb = gb; any_w = ge - gb; }
    };
    int32_t hi = 0;                                       // positions [0, hi) are covered or already counted
    for (const auto& x : iv) { gap(hi, x.first); hi = std::max(hi, x.second); }
    gap(hi, L);
    if (in_w > 0) return in_gb + in_w / 2;
    if (any_w > 0) return any_gb + any_w / 2;
    return L / 2;
}

// ---- the cut on the device ----------------------------------------------------------------------------------------------------
// Summary of the free (uncovered) runs of a stretch [pos, pos + len) of a contig: the run that touches its left end, the one that
// touches its right end (both = len when nothing in it is covered), and the best gaps that touch neither end, among those whose middle
// lies in the contig's middle half and among all.  Summaries of neighbouring stretches combine into the summary of both.
struct CircSum {
    int32_t pos, len, lead, trail;
    int32_t in_gb, in_w, any_gb, any_w;
};
__device__ __forceinline__ void circ_note_gap(CircSum& s, const int32_t gb, const int32_t w, const int32_t L) {
    if (w <= 0) return;
    if (circ_gap_inner(gb, w, L) && circ_gap_better(gb, w, s.in_gb, s.in_w, L)) { s.in_gb = gb; s.in_w = w; }
    if (circ_gap_better(gb, w, s.any_gb, s.any_w, L)) { s.any_gb = gb; s.any_w = w; }
}
__device__ __forceinline__ CircSum circ_combine(const CircSum& a, const CircSum& b, const int32_t L) {      // a lies right before b
    CircSum r;
    const bool afree = a.lead == a.len, bfree = b.lead == b.len;
    r.pos = a.len ? a.pos : b.pos; r.len = a.len + b.len;
    r.lead = afree ? a.len + b.lead : a.lead;
    r.trail = bfree ? b.len + a.trail : b.trail;
    r.in_gb = a.in_gb; r.in_w = a.in_w; r.any_gb = a.any_gb; r.any_w = a.any_w;
    circ_note_gap(r, b.in_gb, b.in_w, L);
    circ_note_gap(r, b.any_gb, b.any_w, L);
    if (!afree && !bfree) circ_note_gap(r, b.pos - a.trail, a.trail + b.lead, L);     // the run across the seam is closed on both sides
    return r;
}
__device__ __forceinline__ CircSum circ_shfl_down(const CircSum& s, const int d) {
    CircSum r;
    r.pos = __shfl_down(s.pos, d, 64); r.len = __shfl_down(s.len, d, 64); r.lead = __shfl_down(s.lead, d, 64); r.trail = __shfl_down(s.trail, d, 64);
    r.in_gb = __shfl_down(s.in_gb, d, 64); r.in_w = __shfl_down(s.in_w, d, 64); r.any_gb = __shfl_down(s.any_gb, d, 64); r.any_w = __shfl_down(s.any_w, d, 64);
    return r;
}
// in-order reduction over the wavefront: lane 0 ends up with the summary of all 64 stretches
__device__ __forceinline__ CircSum circ_wave_reduce(CircSum s, const int lane, const int32_t L) {
    for (int d = 1; d < 64; d <<= 1) {
        const CircSum o = circ_shfl_down(s, d);
        if ((lane & (2 * d - 1)) == 0) s = circ_combine(s, o, L);
    }
    return s;
}

constexpr int kCircSpanWords = 32;                             // a thread's stretch: 32 words = 1024 positions
constexpr int kCircSpan = 32 * kCircSpanWords;
constexpr int kCircChunk = 256 * kCircSpan;                    // a workgroup's: 262 144 positions of ONE contig

// Work is dealt by words, not by contigs: chunk k of the launch is chunk k - chunk0[j] of circular contig j (circ[j] in the batch), so a
// genome of 200 Mbp is 763 workgroups and a plasmid one.  `bits` is the coverage bitmap of k_cover_genes (bit ct[c].base + p of
// position p, 0-based); a thread reads its 1024 positions as 32 words shifted into place, walks the free runs with ffs, and the
// summaries are combined in order across the wavefront (shuffles) and the workgroup (LDS).
__global__ void __launch_bounds__(256)
k_circ_gaps(const uint32_t* __restrict__ bits, const ContigDesc* __restrict__ ct, const int32_t* __restrict__ circ, const int32_t* __restrict__ chunk0,
            const int n_circ, CircSum* __restrict__ sums) {
    __shared__ CircSum part[4];
    const int k = blockIdx.x;
    int lo = 0, hi = n_circ - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (chunk0[mid] <= k) lo = mid; else hi = mid - 1; }
    const ContigDesc cd = ct[circ[lo]];
    const int32_t L = cd.len;
    const int64_t s64 = (int64_t)(k - chunk0[lo]) * kCircChunk + (int64_t)threadIdx.x * kCircSpan;
    CircSum s{0, 0, 0, 0, 0, 0, 0, 0};
    if (s64 < L) {
        const int32_t s0 = (int32_t)s64, e0 = s64 + kCircSpan < L ? (int32_t)(s64 + kCircSpan) : L;
        int32_t open = -1;                                     // start of the free run that is still open
        s.pos = s0; s.len = e0 - s0;
        for (int32_t p0 = s0; p0 < e0; p0 += 32) {
            const int64_t at = cd.base + p0;
            const int sh = (int)(at & 31);
            const uint32_t w0 = bits[at >> 5], w1 = bits[(at >> 5) + 1];         // (the bitmap has two words of slack behind the batch)
            const uint32_t cov = sh ? (w0 >> sh) | (w1 << (32 - sh)) : w0;
            const int nb = min(32, e0 - p0);
            const uint32_t f = ~cov & (nb < 32 ? (1u << nb) - 1u : 0xffffffffu);  // 1: free
            int b = 0;
            while (b < nb) {
                const uint32_t rest = f >> b;
                if (open < 0) {
                    if (rest == 0) break;
                    b += __ffs(rest) - 1;
                    open = p0 + b;
                } else {
                    const uint32_t nr = ~rest & (0xffffffffu >> b);
                    if (nr == 0) break;
                    b += __ffs(nr) - 1;
                    if (b >= nb) break;
                    if (open == s0) s.lead = p0 + b - s0; else circ_note_gap(s, open, p0 + b - open, L);
                    open = -1;
                }
            }
        }
        if (open == s0) { s.lead = s.len; s.trail = s.len; }
        else if (open >= 0) s.trail = e0 - open;
    }
    const int lane = threadIdx.x & 63;
    s = circ_wave_reduce(s, lane, L);
    if (lane == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) sums[k] = circ_combine(circ_combine(part[0], part[1], L), circ_combine(part[2], part[3], L), L);
}

// A wavefront per circular contig: the chunk summaries in order (a block of them per lane), then the runs at the contig's two ends
// join the candidates and step 2's order picks the cut.  cut[] holds -1 for the linear contigs (set by the caller).
__global__ void __launch_bounds__(64)
k_circ_pick(const CircSum* __restrict__ sums, const ContigDesc* __restrict__ ct, const int32_t* __restrict__ circ, const int32_t* __restrict__ chunk0,
            int32_t* __restrict__ cut) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const int32_t L = ct[circ[j]].len;
    const int c0 = chunk0[j], n = chunk0[j + 1] - c0;
    const int per = (n + 63) / 64;
    CircSum s{0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = lane * per; k < min(n, (lane + 1) * per); k++) s = circ_combine(s, sums[c0 + k], L);
    s = circ_wave_reduce(s, lane, L);
    if (lane != 0) return;
    int32_t r = L / 2;
    if (s.lead != s.len) {                   // something is covered: the end runs are gaps of their own
        CircSum t = s;
        circ_note_gap(t, 0, s.lead, L);
        circ_note_gap(t, L - s.trail, s.trail, L);
        if (t.in_w > 0) r = t.in_gb + t.in_w / 2;
        else if (t.any_w > 0) r = t.any_gb + t.any_w / 2;
    }
    cut[circ[j]] = r;
}

// ---- the rotation ----------------------------------------------------------------------------------------------------------------
// R = S[cut:] + S[:cut] for every circular contig, into the batch of pass 2 (contig j there = contig circ[j] here).  A thread per 16
// bytes of the destination (its allocation is 256-byte aligned): where they come from one piece of one contig they are one 16-byte
// load, aligned or not, and one aligned 16-byte store; the few that straddle a seam go letter by letter.
__global__ void __launch_bounds__(256)
k_circ_rotate(const char* __restrict__ src, const ContigDesc* __restrict__ sct, const int32_t* __restrict__ circ, const int32_t* __restrict__ cut,
              const ContigDesc* __restrict__ dct, const int n_circ, const int64_t total, char* __restrict__ dst) {
    const int64_t q0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (q0 >= total) return;
    const int64_t q1 = q0 + 16 < total ? q0 + 16 : total;
    int lo = 0, hi = n_circ - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (dct[mid].base <= q0) lo = mid; else hi = mid - 1; }
    int j = lo;
    ContigDesc d = dct[j];
    ContigDesc s = sct[circ[j]];
    int32_t ck = cut[circ[j]];
    {
        const int64_t r0 = q0 - d.base;                        // position in R of the first letter
        const int64_t first = r0 + ck < d.len ? r0 + ck : r0 + ck - d.len;
        if (q1 - q0 == 16 && r0 + 16 <= d.len && first + 16 <= d.len) {
            uint4 v;
            __builtin_memcpy(&v, src + s.base + first, 16);
            *reinterpret_cast<uint4*>(dst + q0) = v;
            return;
        }
    }
    for (int64_t q = q0; q < q1; q++) {
        while (q >= d.base + d.len) { j++; d = dct[j]; s = sct[circ[j]]; ck = cut[circ[j]]; }     // (empty contigs are stepped over; q < total ends it)
        const int64_t r = q - d.base;
        const int64_t p = r + ck < d.len ? r + ck : r + ck - d.len;
        dst[q] = src[s.base + p];
    }
}

// The caller's regions of the circular contigs follow the letters: [b, e) of S starts at (b - cut) mod L in R and is split in two where
// it contains the cut.  reg[2 k] holds region k as given (its contig already the one of pass 2's batch), reg[2 k + 1] takes the second piece.
__global__ void __launch_bounds__(256)
k_circ_regions(MaskRun* __restrict__ reg, const int n, const int32_t* __restrict__ circ, const int32_t* __restrict__ cut, const ContigDesc* __restrict__ dct) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    MaskRun a = reg[2 * k], b{a.contig, 0, 0, 0};
    const int32_t L = dct[a.contig].len, ck = cut[circ[a.contig]];
    const int32_t w = a.end - a.begin;
    if (L > 0 && w > 0) {
        const int32_t nb = a.begin >= ck ? a.begin - ck : a.begin - ck + L;
        a.begin = nb;
        if ((int64_t)nb + w <= L) a.end = nb + w;
        else { a.end = L; b.end = (int32_t)((int64_t)nb + w - L); }
    }
    reg[2 * k] = a; reg[2 * k + 1] = b;
}

// ---- the way back ----------------------------------------------------------------------------------------------------------------
struct CircSplice {
    int64_t src, dst;      // first record of the contig in its pass's array / in the result
    int32_t n;             // records
    int32_t j;             // -1: a linear contig, records of pass 1 as they are; else its index in pass 2's batch
};
// A workgroup per contig of `which` (contigs of few records: one wavefront; genomes: 1024 threads).  Linear: its records of pass 1 move
// to their place.  Circular: the records of pass 2 get the contig's index and the record's coordinates (step 4 of the rule) and are
// rotated so that begin ascends: those with begin_R > L - cut come first, each group in pass 2's order -- a stable partition, by
// ballots within a wavefront and running counts across the wavefronts of the workgroup.
constexpr int kCircSpliceBig = 1024;        // records from which a contig gets a workgroup of 1024 threads
__global__ void __launch_bounds__(1024)
k_circ_splice(const CircSplice* __restrict__ sp, const int32_t* __restrict__ which, const ContigDesc* __restrict__ ct, const int32_t* __restrict__ cut,
              const pga_gene* __restrict__ g1, const pga_gene* __restrict__ g2, pga_gene* __restrict__ out) {
    __shared__ int s_hi[16], s_lo[16], s_total;
    const int c = which[blockIdx.x], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = blockDim.x, waves = T >> 6;
    const CircSplice d = sp[c];
    if (d.j < 0) {
        for (int i = tid; i < d.n; i += T) out[d.dst + i] = g1[d.src + i];
        return;
    }
    const int32_t L = ct[c].len, ck = cut[c];
    const int32_t edge = L - ck;                               // begin_R beyond it: the record starts in S[:cut]
    if (tid == 0) s_total = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < d.n; i += T) mine += g2[d.src + i].begin > edge ? 1 : 0;
    for (int k = 32; k > 0; k >>= 1) mine += __shfl_down(mine, k, 64);
    if (lane == 0 && mine) atomicAdd(&s_total, mine);
    __syncthreads();
    const int n_hi = s_total;
    int seen_hi = 0, seen_lo = 0;                              // records of each kind in the tiles before this one
    for (int i0 = 0; i0 < d.n; i0 += T) {
        const int i = i0 + tid;
        const bool in = i < d.n;
        const int32_t gb = in ? g2[d.src + i].begin : 0, ge = in ? g2[d.src + i].end : 0;
        const bool is_hi = in && gb > edge;
        const unsigned long long mh = __ballot(is_hi), ml = __ballot(in && !is_hi);
        if (lane == 0) { s_hi[wave] = __popcll(mh); s_lo[wave] = __popcll(ml); }
        __syncthreads();
        int before_hi = 0, before_lo = 0, tile_hi = 0, tile_lo = 0;
        for (int w = 0; w < waves; w++) {
            if (w < wave) { before_hi += s_hi[w]; before_lo += s_lo[w]; }
            tile_hi += s_hi[w]; tile_lo += s_lo[w];
        }
        __syncthreads();                                       // (the counts are read: the next tile may write them)
        const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
        if (in) {
            const int at = is_hi ? seen_hi + before_hi + __popcll(mh & below) : n_hi + seen_lo + before_lo + __popcll(ml & below);
            const int32_t nb = (int32_t)(((int64_t)gb - 1 + ck) % L) + 1;
            pga_gene* const o = out + d.dst + at;             // (record to record, then the five fields: no private copy of the record)
            *o = g2[d.src + i];
            o->contig = c; o->begin = nb; o->end = nb + (ge - gb);
            o->partial_begin = 0; o->partial_end = 0;
        }
        seen_hi += tile_hi; seen_lo += tile_lo;
    }
}

// ---- the call ----------------------------------------------------------------------------------------------------------------------
static int find_circular(const Knobs& kn, pga_ctx* c, const pga_batch* batch, const pga_params* pp, pga_result** out, const int32_t* model_of_contig) {
    if (out) *out = nullptr;
    if (!pp || !out) { c->err = "pga_find_genes: bad arguments"; return PGA_EINVAL; }
    const int NC = batch->n;
    std::vector<int32_t> circ;                                  // the circular contigs, in batch order
    for (int i = 0; i < NC; i++) if (batch->circular[i]) circ.push_back(i);
    const int NR = (int)circ.size();
    c->last_cuts.assign((size_t)NC, -1);

    // pass 1: the ordinary call; the records stay where they are
    GeneKeep k1{"d_genes_pass1"};
    pga_result* r1 = nullptr;
    int rc = find_impl(kn, c, batch, pp, 0, 0, &r1, model_of_contig, nullptr, nullptr, &k1);
    if (rc) return rc;
    ResultOwner* R1 = reinterpret_cast<ResultOwner*>(r1);
    struct Guard { ResultOwner* r; ~Guard() { delete r; } } guard1{R1}, guard2{nullptr};
    struct BatchGuard { pga_batch* b; ~BatchGuard() { pga_batch_free(b); } } rot{nullptr};
    hipStream_t st = c->stream;
    const int64_t total = batch->total;

    // the batch of pass 2: the circular contigs, same lengths, hence the same tiles; its letters are written by k_circ_rotate
    pga_batch* b2 = new (std::nothrow) pga_batch();
    if (!b2) return PGA_ENOMEM;
    rot.b = b2;
    b2->ctx = c; b2->n = NR; b2->d_seq = nullptr; b2->d_tiles = nullptr; b2->d_tile0 = nullptr; b2->n_tiles = 0; b2->ct.resize((size_t)NR + 1);
    int64_t total2 = 0;
    for (int j = 0; j < NR; j++) { b2->ct[j].base = total2; b2->ct[j].len = batch->ct[circ[j]].len; b2->ct[j]._pad = 0; total2 += b2->ct[j].len; }
    b2->ct[NR].base = total2; b2->ct[NR].len = 0; b2->ct[NR]._pad = 0;
    b2->total = total2;
    b2->mask_case = batch->mask_case;

    std::vector<int32_t> h_cut((size_t)NC, -1);
    for (int j = 0; j < NR; j++) h_cut[circ[j]] = 0;           // (a batch without letters: every contig is empty, cut 0)
    ResultOwner* R2 = nullptr;
    GeneKeep k2{"d_genes_out"};
    std::vector<int32_t> moc2;
    DEVBUF(d_cut, int32_t, "circ_cut", NC + 1);
    DEVBUF(d_ct, ContigDesc, "circ_ct", NC + 1);
    HT(c, hipSetDevice(c->device));
    HT(c, hipMemcpyAsync(d_ct, batch->ct.data(), sizeof(ContigDesc) * ((size_t)NC + 1), hipMemcpyHostToDevice, st));
    HT(c, hipMemsetAsync(d_cut, 0xff, sizeof(int32_t) * (size_t)NC, st));
    if (total2 > 0) {
        // chunks of the cut search, dealt by words
        std::vector<int32_t> chunk0((size_t)NR + 1, 0);
        for (int j = 0; j < NR; j++) chunk0[(size_t)j + 1] = chunk0[j] + (int32_t)(((int64_t)b2->ct[j].len + kCircChunk - 1) / kCircChunk);
        const int n_chunks = chunk0[NR];
        const int64_t words = total / 32 + 4;
        DEVBUF(d_cover, uint32_t, "circ_cover", words);
        DEVBUF(d_sums, CircSum, "circ_sums", n_chunks + 1);
        DEVBUF(d_idx, int32_t, "circ_index", 2 * (size_t)NR + 2);      // circ[NR], chunk0[NR + 1]
        DEVBUF(d_ct2, ContigDesc, "circ_ct2", NR + 1);
        PINBUF(h_idx, int32_t, "h_circ_index", 2 * (size_t)NR + 2 + (size_t)NC);
        int32_t* const h_cut_pin = h_idx + 2 * (size_t)NR + 2;
        memcpy(h_idx, circ.data(), sizeof(int32_t) * NR);
        memcpy(h_idx + NR, chunk0.data(), sizeof(int32_t) * ((size_t)NR + 1));
        const int32_t* const d_circ = d_idx; const int32_t* const d_chunk0 = d_idx + NR;
        HT(c, hipMemcpyAsync(d_idx, h_idx, sizeof(int32_t) * (2 * (size_t)NR + 1), hipMemcpyHostToDevice, st));
        HT(c, hipMemcpyAsync(d_ct2, b2->ct.data(), sizeof(ContigDesc) * ((size_t)NR + 1), hipMemcpyHostToDevice, st));
        HT(c, hipMemsetAsync(d_cover, 0, sizeof(uint32_t) * (size_t)words, st));
        if (k1.n_genes > 0)
            hipLaunchKernelGGL(k_cover_genes, dim3((unsigned)((k1.n_genes + 3) / 4)), dim3(256), 0, st, k1.d_genes, k1.n_genes, d_ct, NC, d_cover);
        if (n_chunks > 0)
            hipLaunchKernelGGL(k_circ_gaps, dim3((unsigned)n_chunks), dim3(256), 0, st, d_cover, d_ct, d_circ, d_chunk0, NR, d_sums);
        hipLaunchKernelGGL(k_circ_pick, dim3((unsigned)NR), dim3(64), 0, st, d_sums, d_ct, d_circ, d_chunk0, d_cut);
        HT(c, hipMemcpyAsync(h_cut_pin, d_cut, sizeof(int32_t) * (size_t)NC, hipMemcpyDeviceToHost, st));

        std::vector<TileDesc> tiles; std::vector<int32_t> tile0;
        batch_tiles(b2, tiles, tile0);
        if (batch_take_dev(c, (size_t)total2 + 16 + batch_tiles_bytes(tiles, tile0), &b2->d_seq, &b2->d_seq_cap) != hipSuccess) { (void)hipGetLastError(); c->err = "pga_find_genes: hipMalloc of the rotated batch failed"; return PGA_ENOMEM; }
        HT(c, batch_upload_tiles(b2, b2->d_seq + total2 + 16, tiles, tile0, st));
        hipLaunchKernelGGL(k_circ_rotate, dim3((unsigned)(((total2 + 15) / 16 + 255) / 256)), dim3(256), 0, st, batch->d_seq, d_ct, d_circ, d_cut, d_ct2, NR,
                           total2, b2->d_seq);
        // the caller's regions of the circular contigs, two slots each
        if (!batch->regions.empty()) {
            std::vector<int32_t> jof((size_t)NC, -1);
            for (int j = 0; j < NR; j++) jof[circ[j]] = j;
            b2->reg_off.assign((size_t)NR + 1, 0);
            for (int j = 0; j < NR; j++) {
                const int s = circ[j];
                for (int32_t k = batch->reg_off[s]; k < batch->reg_off[s + 1]; k++) {
                    b2->regions.push_back(MaskRun{j, batch->regions[k].begin, batch->regions[k].end, 0});
                    b2->regions.push_back(MaskRun{j, 0, 0, 0});
                }
                b2->reg_off[(size_t)j + 1] = (int32_t)b2->regions.size();
            }
            if (b2->regions.empty()) b2->reg_off.clear();
            else {
                HT(c, hipMalloc((void**)&b2->d_regions, sizeof(MaskRun) * b2->regions.size()));
                HT(c, hipMemcpyAsync(b2->d_regions, b2->regions.data(), sizeof(MaskRun) * b2->regions.size(), hipMemcpyHostToDevice, st));
                const int nr = (int)(b2->regions.size() / 2);
                hipLaunchKernelGGL(k_circ_regions, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, st, b2->d_regions, nr, d_circ, d_cut, d_ct2);
            }
        }
        HT(c, hipGetLastError());
        HT(c, hipStreamSynchronize(st));                      // the staging vectors above go out of use; the cuts are on the host
        memcpy(h_cut.data(), h_cut_pin, sizeof(int32_t) * (size_t)NC);

        // pass 2: the same call on the rotated contigs, closed
        pga_params P2 = *pp;
        P2.closed = 1;
        if (model_of_contig) for (int j = 0; j < NR; j++) moc2.push_back(model_of_contig[circ[j]]);
        pga_result* r2 = nullptr;
        rc = find_impl(kn, c, b2, &P2, 0, 0, &r2, model_of_contig ? moc2.data() : nullptr, nullptr, nullptr, &k2);
        if (rc) return rc;
        R2 = reinterpret_cast<ResultOwner*>(r2);
        guard2.r = R2;
    }
    c->dev_nodes.clear();                                       // (they are pass 2's, in its coordinates: not for the start-score file)

    // one gene array: pass 1's records of the linear contigs, pass 2's of the circular ones, in batch order
    std::vector<CircSplice> sp((size_t)NC);
    int64_t ngenes = 0;
    {
        int j = 0;
        for (int i = 0; i < NC; i++) {
            pga_contig_result& cr = R1->contigs[i];
            if (batch->circular[i]) {
                if (R2) {
                    const pga_contig_result& c2 = R2->contigs[j];
                    sp[i] = CircSplice{c2.gene_begin, ngenes, c2.n_genes, j};
                    cr.model = c2.model; cr.n_nodes = c2.n_nodes; cr.n_genes = c2.n_genes; cr.score = c2.score;
                } else {
                    sp[i] = CircSplice{0, ngenes, 0, j};
                    cr.n_genes = 0;
                }
                j++;
            } else sp[i] = CircSplice{cr.gene_begin, ngenes, cr.n_genes, -1};
            cr.gene_begin = ngenes;
            ngenes += cr.n_genes;
        }
    }
    pga_gene* const genes_out = R1->gene_records((size_t)ngenes, kn.pageable_results);
    if (ngenes > 0) {
        DEVBUF(d_final, pga_gene, "circ_genes", ngenes + 1);
        DEVBUF(d_sp, CircSplice, "circ_splice", NC + 1);
        DEVBUF(d_which, int32_t, "circ_splice_list", NC + 1);
        // the contigs with records, those of few first: a wavefront each, the genomes a workgroup of 1024 threads each
        std::vector<int32_t> which;
        for (int i = 0; i < NC; i++) if (sp[i].n > 0 && sp[i].n < kCircSpliceBig) which.push_back(i);
        const int n_small = (int)which.size();
        for (int i = 0; i < NC; i++) if (sp[i].n >= kCircSpliceBig) which.push_back(i);
        const int n_big = (int)which.size() - n_small;
        HT(c, hipMemcpyAsync(d_sp, sp.data(), sizeof(CircSplice) * (size_t)NC, hipMemcpyHostToDevice, st));
        HT(c, hipMemcpyAsync(d_which, which.data(), sizeof(int32_t) * which.size(), hipMemcpyHostToDevice, st));
        if (n_small > 0)
            hipLaunchKernelGGL(k_circ_splice, dim3((unsigned)n_small), dim3(64), 0, st, d_sp, d_which, d_ct, d_cut, k1.d_genes, k2.d_genes, d_final);
        if (n_big > 0)
            hipLaunchKernelGGL(k_circ_splice, dim3((unsigned)n_big), dim3(1024), 0, st, d_sp, d_which + n_small, d_ct, d_cut, k1.d_genes, k2.d_genes, d_final);
        HT(c, hipMemcpyAsync(genes_out, d_final, sizeof(pga_gene) * (size_t)ngenes, hipMemcpyDeviceToHost, st));
        HT(c, hipGetLastError());
        HT(c, hipStreamSynchronize(st));
    }
    if (R2) {
        if (pp->want_nodes == 1 && !R2->nodes.empty()) {
            if (R1->nodes.empty()) { R1->nodes.resize((size_t)NC); for (auto& N : R1->nodes) memset(&N, 0, sizeof N); }
            for (int j = 0; j < NR; j++) R1->nodes[circ[j]] = R2->nodes[j];        // (pass 1's block of the contig stays with R1 until it is freed)
            for (void* blk : R2->blocks) R1->blocks.push_back(blk);
            R2->blocks.clear();
        }
        R1->pub.t_total_ms += R2->pub.t_total_ms; R1->pub.t_dp_ms += R2->pub.t_dp_ms;
        R1->pub.node_passes += R2->pub.node_passes; R1->pub.n_chains += R2->pub.n_chains;
    }
    c->last_cuts = h_cut;
    return publish(R1, guard1.r, *pp, out);
}

extern "C" int pga_batch_set_circular(pga_batch* b, const uint8_t* circular) {
    if (!b) return PGA_EINVAL;
    b->circular.clear();
    if (circular) {
        bool any = false;
        for (int i = 0; i < b->n; i++) any = any || circular[i] != 0;
        if (any) { b->circular.resize((size_t)b->n); for (int i = 0; i < b->n; i++) b->circular[i] = circular[i] ? 1 : 0; }
    }
    return PGA_OK;
}

extern "C" int pga_circular_cuts(const pga_ctx* c, int32_t n, int32_t* out) {
    if (!c || n < 0 || (n > 0 && !out)) return PGA_EINVAL;
    for (int i = 0; i < n; i++) out[i] = i < (int)c->last_cuts.size() ? c->last_cuts[i] : -1;
    return PGA_OK;
}
