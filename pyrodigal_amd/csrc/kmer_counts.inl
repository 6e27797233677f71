// The k-mers of every contig or gene record counted into integer vectors, one row per contig or per gene, left on the device
// (pga_count_kmers; the rule is in pyrodigal_amd.h).  Included by translate.hip, inside its anonymous namespace, behind
// device_rows.inl.  Of the batch, only the letters the rows name are read.

constexpr int kCntChunk = 32768;                       // window starts of one piece of work (pga_kmer_counts_chunk)
constexpr int kCntRun = 8;                             // consecutive window starts of one thread
constexpr int kCntSweep = kRowThreads * kCntRun;       // window starts a workgroup takes in one sweep over its piece
constexpr int kCntMaxBins = 4096;                      // 4^6: the codes of k = 6, and the most bins of a table
constexpr int kCntMaxLetters = (kCntRun - 1) * 3 + 6;  // the letters of a thread's run at step 3, k = 6
constexpr int kCntWords = (kCntMaxLetters + 3) / 4;    // ... as aligned 4-letter words
static_assert(kCntChunk % kCntSweep == 0, "a piece is a whole number of sweeps");

// One row of work, built on the host from a checked record or from a contig: the 88-byte gene records do not go up.  The row is an
// axis of letters; letter x lies at 0-based position q0 + x (forward) or q0 - x (reverse) of its contig, taken modulo L where the
// axis runs across the origin of a circle (at most once: the host has taken q0 into [0, L), and an axis is shorter than 2 L).
// Window w starts at letter w * step.
struct CntRow {
    int64_t base;              // the contig's first letter in the batch
    int32_t q0, L;
    int32_t n_win;             // window starts of the row
    int32_t dst;               // the row of d_out it counts into
    uint32_t bits;             // bit 0: forward.  Bit 1: dst is shared with other pieces (zeroed on the stream, flushed with atomicAdd)
    int32_t _pad;
};
static_assert(sizeof(CntRow) == 32, "CntRow");

// everything the kernel is told, by value
struct CntArgs {
    const char* seq; const CntRow* row;
    const int2* piece;         // [n_pieces] of work: the row, and the first of its window starts
    const int32_t* bin_of_code;
    int32_t* out;
    int64_t n_pieces, S;
    int32_t k, step, n_bins, wide;   // wide: the letters of the batch begin at a multiple of 4 bytes
};

// the rows of d_out that several pieces count into: elements 0 .. n_bins - 1 of each are zeroed, on the stream, in front of the count
__global__ void __launch_bounds__(kRowThreads)
k_kmer_zero(int32_t* __restrict__ out, const int64_t S, const int32_t n_bins, const int32_t* __restrict__ rows, const int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n_bins) return;
    const int64_t z = idx / n_bins;
    out[(int64_t)rows[z] * S + (idx - z * n_bins)] = 0;
}

// (host) the LDS of a launch: the histograms (none in the direct form), then the 16-bit bin table
static size_t cnt_lds_bytes(const bool direct, const int split, const int n_bins, const int n_codes) {
    return (direct ? 0 : sizeof(int32_t) * (size_t)split * (size_t)n_bins) + sizeof(int16_t) * (size_t)n_codes;
}

// the class of a letter: A, C, G, T = 0 .. 3 in either case, anything else 4
__device__ __forceinline__ uint32_t cnt_class(const uint32_t byte) {
    const uint32_t b = byte | 0x20u;
    return b == 'a' ? 0u : b == 'c' ? 1u : b == 'g' ? 2u : b == 't' ? 3u : 4u;
}

// Work is dealt by source positions: a piece is up to kCntChunk consecutive window starts of one row, named by the host's list (a
// binary search of 18 dependent loads per workgroup cost more than the counting of a gene), so one contig of 200 Mbp and 200 000
// genes both fill the device.  A piece belongs to a workgroup (SPLIT = 1) or, where the rows are short, to one of its four waves
// (SPLIT = 4, a histogram each: a gene of 300 codons keeps 38 of 64 lanes busy, not 38 of 256).  The owners sweep the piece
// kCntSweep / SPLIT window starts at a time; a thread owns kCntRun consecutive ones and reads the (run - 1) step + k letters under
// them once, in ascending address order on either strand: away from a wrap as aligned 4-byte words (the neighbours' words are the
// same cache lines), shifted into place, else letter by letter.  It rolls the code and the letters since the last N in registers: on the forward strand a letter
// enters as the least significant digit and closes the window that ends there, on the reverse strand its complement enters as the
// most significant digit and closes the window that starts there.  The bin table is staged in LDS (16-bit entries); the counts of
// the piece are summed in an LDS histogram (!DIRECT) and leave once: with plain stores, zeros included, where the piece is the
// row's only one, else with atomicAdd of the bins that are not zero onto the zeroed row -- integer sums, so the order of arrival
// does not show.  DIRECT (few windows under many bins, rows shared): no histogram, every window adds to the zeroed row itself.
template <bool DIRECT, int SPLIT>
__global__ void __launch_bounds__(kRowThreads)
k_kmer_counts(const CntArgs a) {
    static_assert(SPLIT == 1 || SPLIT == 4, "a piece per workgroup or per wave");
    constexpr int kOwners = kRowThreads / SPLIT;               // the threads of a piece
    // LDS as the launch sizes it (cnt_lds_bytes: 1.1 KB for codon rows per wave, 24 KB at most): SPLIT histograms of n_bins counts,
    // then the bin table.  A fixed 24 KB held codon rows at 6 workgroups per CU.
    extern __shared__ int32_t s_cnt[];
    const int tid = threadIdx.x, k = a.k, step = a.step, n_bins = a.n_bins;
    int32_t* const s_hist = s_cnt;
    int16_t* const s_bin = reinterpret_cast<int16_t*>(s_cnt + (DIRECT ? 0 : SPLIT * n_bins));
    const int lane = tid % kOwners, part = tid / kOwners;
    for (int i = tid; i < (1 << (2 * k)); i += kRowThreads) s_bin[i] = (int16_t)a.bin_of_code[i];
    if (!DIRECT) for (int i = tid; i < SPLIT * n_bins; i += kRowThreads) s_hist[i] = 0;
    int32_t* const hist = s_hist + (DIRECT ? 0 : part * n_bins);
    const int64_t piece = (int64_t)blockIdx.x * SPLIT + part;
    const bool live = piece < a.n_pieces;                       // (the last workgroup of a split launch may own fewer pieces)
    CntRow r{};
    int32_t w_lo = 0, w_hi = 0;
    if (live) {
        const int2 pd = a.piece[piece];
        r = a.row[pd.x];
        w_lo = pd.y;
        w_hi = r.n_win - w_lo < kCntChunk ? r.n_win : w_lo + kCntChunk;
    }
    const bool fwd = (r.bits & 1u) != 0u, shared = (r.bits & 2u) != 0u;
    const char* __restrict__ s = a.seq + r.base;
    int32_t* __restrict__ dst = a.out + (int64_t)r.dst * a.S;
    const uint32_t mask = (1u << (2 * k)) - 1u;
    const int top = 2 * k - 2;
    __syncthreads();
    for (int32_t w0 = w_lo + lane * kCntRun; w0 < w_hi; w0 += kCntSweep / SPLIT) {
        const int nw = w_hi - w0 < kCntRun ? w_hi - w0 : kCntRun;
        const int len = (nw - 1) * step + k;                    // the letters under the run, 0-based positions p0 .. p0 + len - 1 mod L
        int64_t p0 = fwd ? (int64_t)r.q0 + (int64_t)w0 * step : (int64_t)r.q0 - ((int64_t)w0 * step + len - 1);
        if (p0 >= r.L) p0 -= r.L;
        if (p0 < 0) p0 += r.L;
        uint32_t v[kCntWords];                                   // letter i of the run: byte i & 3 of v[i >> 2]
        if (a.wide && p0 + len <= r.L) {
            const uintptr_t at = (uintptr_t)(s + p0);
            const uint32_t* __restrict__ src = (const uint32_t*)(at & ~(uintptr_t)3);      // (inside the batch's allocation: it ends 16 bytes behind the letters)
            const uint32_t sh = (uint32_t)(at & 3u);
            const int nd = (int)(sh + len + 3) >> 2;
            uint32_t d[kCntWords + 1];
#pragma unroll
            for (int j = 0; j <= kCntWords; j++) d[j] = src[j < nd ? j : nd - 1];      // (a clamped index, not a predicated load: no exec mask each)
#pragma unroll
            for (int j = 0; j < kCntWords; j++) {               // (what lies behind the run's last letter reads as N: 0)
                const int keep = len - 4 * j;
                v[j] = keep <= 0 ? 0u : __builtin_amdgcn_alignbyte(d[j + 1], d[j], sh) & (keep >= 4 ? ~0u : (1u << (8 * keep)) - 1u);
            }
        } else {
            // (rare: a run across the origin of a circle.  The letters go in at the top of v and move down a byte per turn, so that
            //  after 4 kCntWords turns letter 0 lies in byte 0 -- no index into v depends on the turn)
#pragma unroll
            for (int j = 0; j < kCntWords; j++) v[j] = 0u;
#pragma unroll 1
            for (int i = 0; i < 4 * kCntWords; i++) {
                uint32_t b = 0u;
                if (i < len) { int64_t p = p0 + i; if (p >= r.L) p -= r.L; b = (uint32_t)(uint8_t)s[p]; }
#pragma unroll
                for (int j = 0; j < kCntWords - 1; j++) v[j] = __builtin_amdgcn_alignbyte(v[j + 1], v[j], 1u);
                v[kCntWords - 1] = (v[kCntWords - 1] >> 8) | (b << 24);
            }
        }
        uint32_t code = 0u;
        int since = 0, phase = 0;                                // phase: (i - (k - 1)) mod step from letter i = k - 1 on
        // a word of four letters per turn, the words moving down through v[0]: a loop unrolled over all 27 letters would walk the 14
        // dead ones of a run at step 1, and hold a mask in SGPRs for each (they spilled)
#pragma unroll 1
        for (int i0 = 0; i0 < len; i0 += 4) {
            const uint32_t w = v[0];
#pragma unroll
            for (int j = 0; j < kCntWords - 1; j++) v[j] = v[j + 1];
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const uint32_t c = cnt_class((w >> (8 * b)) & 0xffu);
                code = fwd ? ((code << 2) | (c & 3u)) & mask : (code >> 2) | ((3u - (c & 3u)) << top);
                since = c == 4u ? 0 : since + 1;
                const int bin = (phase == 0 && since >= k) ? (int)s_bin[code] : -1;      // (since >= k: k - 1 <= i < len, N lies behind)
                if (bin >= 0) {
                    if (DIRECT) atomicAdd(dst + bin, 1); else atomicAdd(&hist[bin], 1);
                }
                phase = i0 + b < k - 1 ? 0 : phase + 1 == step ? 0 : phase + 1;
            }
        }
    }
    if (DIRECT) return;
    __syncthreads();
    if (!live) return;
    if (!shared) {
        for (int i = lane; i < n_bins; i += kOwners) dst[i] = hist[i];
    } else {
        for (int i = lane; i < n_bins; i += kOwners) { const int32_t c = hist[i]; if (c != 0) atomicAdd(dst + i, c); }
    }
}
