// The nucleotides of every gene and of the region around it, in the gene's reading direction, left on the device as token ids, one row
// per gene record (pga_gene_windows; the rule is in pyrodigal_amd.h).  Included by translate.hip, inside its anonymous
// namespace, behind device_rows.inl.  Of the batch, only the letters the windows name are read.

// One row, built on the host from a checked record: the 88-byte gene records do not go up.  Base x of the window (x = 0 is offset t_lo
// of the rule) lies at 0-based position q0 + x on a forward gene and q0 - x on a reverse one, before the wrap of a circle or the edges
// of a linear contig; on a circle the host has taken q0 into [0, L) already.
struct WinRow {
    int64_t base;              // the contig's first letter in the batch
    int64_t q0;
    int32_t L;
    uint32_t bits;             // bit 0: forward.  Bit 1: the contig is flagged circular
};
static_assert(sizeof(WinRow) == 24, "WinRow");

// (host) the 0-based position of offset t_lo of a checked record
static WinRow win_row(const pga_gene& G, const ContigDesc& cd, const bool circular, const int64_t t_lo) {
    const bool fwd = G.strand == 1;
    int64_t q0 = fwd ? (int64_t)G.begin - 1 + t_lo : (int64_t)G.end - 1 - t_lo;
    if (circular) { q0 %= cd.len; if (q0 < 0) q0 += cd.len; }          // (a record lies inside its contig: len >= 3)
    WinRow w;
    w.base = cd.base; w.q0 = q0; w.L = cd.len; w.bits = (fwd ? 1u : 0u) | (circular ? 2u : 0u);
    return w;
}

// everything the kernel is told, by value
struct WinArgs {
    RowArgs rows;              // one row per gene record
    const char* seq; const WinRow* win;
    const int64_t* ids;        // [66]
    int64_t bos, eos;
    int32_t has_bos, has_eos, codons, _pad;
};

// what a thread keeps of the row it is in
struct WinGene { const char* s; int64_t len, q0; int32_t L; bool fwd, circ; };

__device__ __forceinline__ WinGene win_gene(const WinArgs& a, const int64_t g) {
    const WinRow w = a.win[g];
    WinGene t;
    t.s = a.seq + w.base; t.q0 = w.q0; t.L = w.L; t.fwd = (w.bits & 1u) != 0u; t.circ = (w.bits & 2u) != 0u;
    t.len = a.rows.off[g + 1] - a.rows.off[g];
    return t;
}

// the class of base x of the window: A, C, G, T = 0 .. 3 in the gene's own strand, N = 4, outside = 5
__device__ __forceinline__ int win_class(const WinGene& t, const int64_t x) {
    int64_t p = t.fwd ? t.q0 + x : t.q0 - x;
    if (p < 0 || p >= t.L) {
        if (!t.circ) return 5;
        p %= t.L;                                              // a flank may go round a small circle more than once
        if (p < 0) p += t.L;
    }
    int c;
    switch (t.s[p]) { case 'A': case 'a': c = 0; break; case 'C': case 'c': c = 1; break; case 'G': case 'g': c = 2; break;
                      case 'T': case 't': c = 3; break; default: return 4; }
    return t.fwd ? c : 3 - c;                                  // A <-> T, C <-> G
}

// token k of the row (k >= 0): bos, the units' ids, eos -- and pad from len on, which only the padded layout asks for
template <typename T>
__device__ __forceinline__ T win_at(const WinArgs& a, const WinGene& t, const T* s_ids, const int64_t k) {
    if (k >= t.len) return (T)a.rows.pad;
    if (a.has_bos && k == 0) return (T)a.bos;
    if (a.has_eos && k == t.len - 1) return (T)a.eos;
    const int64_t j = k - a.has_bos;
    if (!a.codons) return s_ids[win_class(t, j)];
    const int c0 = win_class(t, 3 * j), c1 = win_class(t, 3 * j + 1), c2 = win_class(t, 3 * j + 2);
    const int worst = max(c0, max(c1, c2));
    return s_ids[worst == 5 ? 65 : worst == 4 ? 64 : 16 * c0 + 4 * c1 + c2];
}

// Work is dealt by destination bytes, as in k_translate_tokens and k_label_bases: a thread owns one 16-byte aligned piece of the
// output by absolute address -- 16, 4 or 2 elements -- so one window of 100 000 bases and 200 000 short ones both fill the device.
// It finds its row by binary search in `off` (ragged) or from the row index (padded), reads the letters its tokens name one by one,
// maps their classes through the ids (staged once per workgroup in LDS, 66 entries of the element width: the indices diverge per
// lane) and leaves as one 16-byte store.  Pieces that span a seam between rows, reach into a row's W .. S, or are partial (the first
// and the last of the tensor) go element by element; rows without tokens are stepped over.  Nothing but the elements the rule names
// is written.  (The third walk over pieces, rows and seams in its own words, for the reason translate_tokens.inl gives.)
template <int EB, bool PADDED>
__global__ void __launch_bounds__(kRowThreads)
k_gene_windows(const WinArgs a) {
    static_assert(EB == 1 || EB == 4 || EB == 8, "element width");
    using T = typename TokElem<EB>::type;
    constexpr int PER = 16 / EB;
    __shared__ T s_ids[66];
    if (threadIdx.x < 66) s_ids[threadIdx.x] = (T)a.ids[threadIdx.x];
    __syncthreads();
    const RowArgs& r = a.rows;
    const int64_t piece = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e0 = piece * PER - r.lead;                   // the piece's first element: below 0 only in piece 0
    if (e0 >= r.n_elems) return;
    const int64_t lo = e0 < 0 ? 0 : e0, hi = e0 + PER < r.n_elems ? e0 + PER : r.n_elems;
    T* __restrict__ out = reinterpret_cast<T*>(r.out0) + r.lead;      // d_out: element e is out[e]
    int64_t g, k;                                              // element lo is token k of row g
    if (PADDED) {
        g = lo / r.S; k = lo - g * r.S;
    } else {
        // the last row that begins at or before lo: it is not empty, since the next one begins beyond lo (or lo < off[G])
        int64_t l = 0, h = r.n_rows - 1;
        while (l < h) { const int64_t mid = (l + h + 1) >> 1; if (r.off[mid] <= lo) l = mid; else h = mid - 1; }
        g = l; k = lo - r.off[g];
    }
    WinGene t = win_gene(a, g);
    // the whole piece lies in one row (ragged) or in the first W elements of one row (padded): hi == e0 + PER follows
    if (e0 >= 0 && k + PER <= (PADDED ? r.W : t.len)) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const T v = win_at<T>(a, t, s_ids, k + j);
            if (EB == 1) w[j >> 2] |= (uint32_t)(uint8_t)v << (8 * (j & 3));
            else if (EB == 4) w[j] = (uint32_t)v;
            else { w[2 * j] = (uint32_t)(uint64_t)v; w[2 * j + 1] = (uint32_t)((uint64_t)v >> 32); }
        }
        *reinterpret_cast<uint4*>(r.out0 + piece * 16) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
    for (int64_t e = lo; e < hi; e++, k++) {
        if (PADDED) {
            if (k == r.S) { k = 0; g++; t = win_gene(a, g); }            // (e < n_elems: the row exists)
            if (k < r.W) out[e] = win_at<T>(a, t, s_ids, k);
        } else {
            if (k == t.len) { do g++; while (r.off[g + 1] == r.off[g]); k = 0; t = win_gene(a, g); }   // (e < off[G] ends it)
            out[e] = win_at<T>(a, t, s_ids, k);
        }
    }
}
