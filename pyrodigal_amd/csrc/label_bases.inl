// The annotation of every base left on the device as a tensor in the shape of the input (pga_label_bases; the rule is in
// pyrodigal_amd.h).  Included by translate.hip, inside its anonymous namespace, behind device_rows.inl.  The letters
// of the batch are not read.

// One stretch of one gene record in contig coordinates, built on the host: the record covers positions [lo, hi) of its contig, and
// position p is base d = p - base of the gene, counted from `begin` (d = q - b of the rule; base = b - 1, or b - 1 - L for the stretch
// behind the origin of a gene across it, which is negative).  A contig's stretches are sorted by lo; rmax is the running maximum of hi
// over the contig's stretches up to and including this one, so the stretches that can reach p are those from the first with rmax > p.
struct LabIv {
    int32_t lo, hi, rmax, base;
    int32_t glen;              // e - b + 1, a multiple of 3
    uint32_t bits;             // bit 0: forward.  Bits 8..15: what the gene's first three bases add (0x40 forward, 0x80 reverse, 0 with
                               // partial_begin).  Bits 16..23: what its last three add (0x80 forward, 0x40 reverse, 0 with partial_end)
    int32_t _pad[2];
};
static_assert(sizeof(LabIv) == 32, "LabIv");

// (host) The stretches of checked records, contig after contig as iv_off says (the exclusive scan of their number per contig), each
// contig's sorted by lo with the running maxima beside them: a gene across the origin makes two.  Records may come in any order.
static void lab_stretches(const pga_gene* genes, const int64_t n_genes, const ContigDesc* ct, const int64_t* iv_off, const size_t n_contigs, LabIv* iv) {
    std::vector<int64_t> at(iv_off, iv_off + n_contigs);
    auto put = [&](const pga_gene& G, const int32_t lo, const int32_t hi, const int32_t base) {
        LabIv& v = iv[at[(size_t)G.contig]++];
        const bool fwd = G.strand == 1;
        v.lo = lo; v.hi = hi; v.rmax = 0; v.base = base; v.glen = G.end - G.begin + 1;
        v.bits = (fwd ? 1u : 0u) | (G.partial_begin ? 0u : (fwd ? 0x40u : 0x80u) << 8) | (G.partial_end ? 0u : (fwd ? 0x80u : 0x40u) << 16);
        v._pad[0] = v._pad[1] = 0;
    };
    for (int64_t g = 0; g < n_genes; g++) {
        const pga_gene& G = genes[g];
        const int32_t len = ct[G.contig].len;
        if (G.end > len) { put(G, G.begin - 1, len, G.begin - 1); put(G, 0, G.end - len, G.begin - 1 - len); }
        else put(G, G.begin - 1, G.end, G.begin - 1);
    }
    for (size_t i = 0; i < n_contigs; i++) {
        LabIv* const a0 = iv + iv_off[i]; LabIv* const a1 = iv + iv_off[i + 1];
        const auto by_lo = [](const LabIv& x, const LabIv& y) { return x.lo < y.lo; };
        if (!std::is_sorted(a0, a1, by_lo)) std::stable_sort(a0, a1, by_lo);      // (among equal lo any order serves: the rule is a union)
        int32_t m = 0;
        for (LabIv* p = a0; p < a1; p++) { if (p->hi > m) m = p->hi; p->rmax = m; }
    }
}

// everything the kernel is told, by value
struct LabArgs {
    const int64_t* iv_off;     // [n_contigs + 1] the stretches of contig i are iv[iv_off[i] .. iv_off[i + 1])
    const int64_t* cmap;       // [256]
    const LabIv* iv;
    RowArgs rows;              // one row per contig (behind the tables: `off` then comes with them in the kernel's first argument load)
};

// The raw bytes of positions k .. k + N - 1 of a contig whose stretches are iv[ib .. ie), packed four to a word (position k + j is
// byte j & 3 of w[j >> 2]).  Positions at or beyond the contig's end lie in no stretch and come out 0.
template <int N>
__device__ __forceinline__ void lab_raw(const LabIv* __restrict__ iv, const int64_t ib, const int64_t ie, const int32_t k, uint32_t (&w)[(N + 3) / 4]) {
#pragma unroll
    for (int j = 0; j < (N + 3) / 4; j++) w[j] = 0u;
    int64_t l = ib, h = ie;                                    // the first stretch whose running maximum passes k
    while (l < h) { const int64_t mid = (l + h) >> 1; if (iv[mid].rmax > k) h = mid; else l = mid + 1; }
    for (int64_t x = l; x < ie; x++) {
        const LabIv v = iv[x];
        if (v.lo >= k + N) break;                              // sorted by lo: nothing further reaches the piece
        if (v.hi <= k) continue;
        const int32_t d0 = k - v.base;                         // > -N: lo < k + N, and base <= lo
        const uint32_t r0 = (uint32_t)(d0 + 18) % 3u;          // (q - b) % 3 of position k
        const bool fwd = (v.bits & 1u) != 0u;
        const uint32_t first = (v.bits >> 8) & 255u, last = (v.bits >> 16) & 255u;
#pragma unroll
        for (int j = 0; j < N; j++) {
            const int32_t p = k + j, d = d0 + j;
            uint32_t f = r0 + (uint32_t)(j % 3);
            f = f >= 3u ? f - 3u : f;
            // the reverse gene counts from its own first base, `end`: (e - q) % 3 = 2 - (q - b) % 3, the length being whole codons
            const uint32_t val = (fwd ? 1u << f : 0x20u >> f) | (d <= 2 ? first : 0u) | (d >= v.glen - 3 ? last : 0u);
            if (p >= v.lo && p < v.hi) w[j >> 2] |= val << (8 * (j & 3));
        }
    }
}

// Work is dealt by destination bytes, as in k_translate_tokens: a thread owns one 16-byte aligned piece of the output by absolute
// address -- 16, 4 or 2 elements -- so one 200 Mbp contig and 100 000 short ones both fill the device.  It finds its contig from the
// row index (padded) or by binary search in `off` (ragged), finds the stretches that can reach its positions by binary search in the
// running maxima, walks that short run, maps the bytes through the class map (staged once per workgroup in LDS, 256 entries of the
// element width: the indices diverge per lane) and leaves as one 16-byte store.  Pieces that span a seam between contigs or rows,
// reach into a row's W .. S, are partial (the first and the last of the tensor) or cross empty contigs go element by element.
// Nothing but the elements the rule names is written.
template <int EB, bool PADDED>
__global__ void __launch_bounds__(kRowThreads)
k_label_bases(const LabArgs a) {
    static_assert(EB == 1 || EB == 4 || EB == 8, "element width");
    using T = typename TokElem<EB>::type;
    constexpr int PER = 16 / EB;
    __shared__ T s_map[256];
    s_map[threadIdx.x] = (T)a.cmap[threadIdx.x];               // (kRowThreads == 256)
    __syncthreads();
    const RowArgs& r = a.rows;
    const int64_t piece = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e0 = piece * PER - r.lead;                   // the piece's first element: below 0 only in piece 0
    if (e0 >= r.n_elems) return;
    const int64_t lo = e0 < 0 ? 0 : e0, hi = e0 + PER < r.n_elems ? e0 + PER : r.n_elems;
    T* __restrict__ out = reinterpret_cast<T*>(r.out0) + r.lead;      // d_out: element e is out[e]
    int64_t g, k;                                              // element lo is position k of contig g (or of its row)
    if (PADDED) {
        g = lo / r.S; k = lo - g * r.S;
    } else {
        // the last contig that begins at or before lo: it is not empty, since the next one begins beyond lo (or lo < off[B])
        int64_t l = 0, h = r.n_rows - 1;
        while (l < h) { const int64_t mid = (l + h + 1) >> 1; if (r.off[mid] <= lo) l = mid; else h = mid - 1; }
        g = l; k = lo - r.off[g];
    }
    int64_t len = r.off[g + 1] - r.off[g];
    // the whole piece lies in one contig (ragged) or in the first W elements of one row (padded): hi == e0 + PER follows
    if (e0 >= 0 && k + PER <= (PADDED ? r.W : len)) {
        uint32_t raw[(PER + 3) / 4] = {};
        if (k < len) lab_raw<PER>(a.iv, a.iv_off[g], a.iv_off[g + 1], (int32_t)k, raw);
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < PER; j++) {
            T v = (T)r.pad;
            if (!PADDED || k + j < len) v = s_map[(raw[j >> 2] >> (8 * (j & 3))) & 255u];
            if (EB == 1) w[j >> 2] |= (uint32_t)(uint8_t)v << (8 * (j & 3));
            else if (EB == 4) w[j] = (uint32_t)v;
            else { w[2 * j] = (uint32_t)(uint64_t)v; w[2 * j + 1] = (uint32_t)((uint64_t)v >> 32); }
        }
        *reinterpret_cast<uint4*>(r.out0 + piece * 16) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
    for (int64_t e = lo; e < hi; e++, k++) {
        if (PADDED) {
            if (k == r.S) { k = 0; g++; len = r.off[g + 1] - r.off[g]; }          // (e < n_elems: the row exists)
            if (k >= r.W) continue;
        } else {
            while (k == len) { g++; k = 0; len = r.off[g + 1] - r.off[g]; }        // (empty contigs are stepped over; e < off[B] ends it)
        }
        T v = (T)r.pad;
        if (k < len) {
            uint32_t raw[1];
            lab_raw<1>(a.iv, a.iv_off[g], a.iv_off[g + 1], (int32_t)k, raw);
            v = s_map[raw[0] & 255u];
        }
        out[e] = v;
    }
}
