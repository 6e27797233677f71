// Proteins left on the device as token ids (pga_translate_genes_tokens; the rule is in pyrodigal_amd.h).
// Included by translate.hip, inside its anonymous namespace, behind device_rows.inl: the __constant__ code tables and translate_rules.h
// are shared with k_translate.

// everything the kernel is told, by value
struct TokArgs {
    RowArgs rows;              // one row per gene
    const char* seq; const ContigDesc* ct; const pga_gene* genes; const int32_t* tt_of;
    const int64_t* vocab;      // [128]
    int64_t bos, eos;
    int32_t has_bos, has_eos, unk, strict;
};

// what a thread keeps of the gene it is in
struct TokGene { const char* s; int64_t len; int32_t clen, begin, end, tt; bool fwd, start_edge; };

__device__ __forceinline__ TokGene tok_gene(const TokArgs& a, const int64_t g) {
    const pga_gene* __restrict__ gp = a.genes + g;
    const int contig = gp->contig;
    const ContigDesc cd = a.ct[contig];
    TokGene t;
    t.s = a.seq + cd.base; t.clen = cd.len; t.begin = gp->begin; t.end = gp->end; t.tt = a.tt_of[contig];
    t.fwd = gp->strand == 1;
    // partial flags are in sequence orientation; the gene's own first codon follows its strand
    t.start_edge = t.fwd ? gp->partial_begin != 0 : gp->partial_end != 0;
    t.len = a.rows.off[g + 1] - a.rows.off[g];
    return t;
}

// token k of the gene (k >= 0): bos, the residues' ids, eos -- and pad from len on, which only the padded layout asks for
template <typename T>
__device__ __forceinline__ T tok_at(const TokArgs& a, const TokGene& t, const T* s_vocab, const int64_t k) {
    if (k >= t.len) return (T)a.rows.pad;
    if (a.has_bos && k == 0) return (T)a.bos;
    if (a.has_eos && k == t.len - 1) return (T)a.eos;
    const int i = (int)k - a.has_bos;
    // a gene across the origin of a circular contig reads position p >= len at p - len (the host checked that only such genes get there)
    auto at = [&](const int p) { return t.s[p >= t.clen ? p - t.clen : p]; };
    int x0, x1, x2;
    if (t.fwd) {
        const int p = t.begin - 1 + 3 * i;
        x0 = digit_of(at(p), false); x1 = digit_of(at(p + 1), false); x2 = digit_of(at(p + 2), false);
    } else {
        const int p = t.end - 1 - 3 * i;
        x0 = digit_of(at(p), true); x1 = digit_of(at(p - 1), true); x2 = digit_of(at(p - 2), true);
    }
    const int aa = translate_codon(c_code[t.tt], x0, x1, x2, t.tt, i, t.start_edge, a.strict, a.unk);
    return s_vocab[aa & 127];
}

// Work is dealt by destination bytes, as in k_pack_device: a thread owns one 16-byte aligned piece of the output by absolute address
// -- 16, 4 or 2 elements -- so one 10 000-residue gene and 200 000 short ones both fill the device.  It finds its gene by binary
// search in `off` (ragged) or from the row index (padded), translates the codons it owns, maps them through the vocabulary (staged
// once per workgroup in LDS, 128 entries of the element width: the indices diverge per lane) and leaves as one 16-byte store.
// Pieces that span a seam between genes or rows, reach into a row's W .. S, or are partial (the first and the last of the tensor)
// go element by element.  Nothing but the elements the rule names is written; of the batch, only the genes' own bases are read.
// (k_label_bases and k_gene_windows, gene_windows.inl, walk pieces, rows and seams the same way, each in its own words: written once
// over an element source, the walk made the padded instances of this kernel slower, profiles/device_rows_kernel_stats.md.  A change
// to the seam logic belongs in all three.)
template <int EB, bool PADDED>
__global__ void __launch_bounds__(kRowThreads)
k_translate_tokens(const TokArgs a) {
    static_assert(EB == 1 || EB == 4 || EB == 8, "element width");
    using T = typename TokElem<EB>::type;
    constexpr int PER = 16 / EB;
    __shared__ T s_vocab[128];
    if (threadIdx.x < 128) s_vocab[threadIdx.x] = (T)a.vocab[threadIdx.x];
    __syncthreads();
    const RowArgs& r = a.rows;
    const int64_t piece = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t e0 = piece * PER - r.lead;                   // the piece's first element: below 0 only in piece 0
    if (e0 >= r.n_elems) return;
    const int64_t lo = e0 < 0 ? 0 : e0, hi = e0 + PER < r.n_elems ? e0 + PER : r.n_elems;
    T* __restrict__ out = reinterpret_cast<T*>(r.out0) + r.lead;      // d_out: element e is out[e]
    int64_t g, k;                                              // element lo is token k of gene g
    if (PADDED) {
        g = lo / r.S; k = lo - g * r.S;
    } else {
        int64_t l = 0, h = r.n_rows - 1;
        while (l < h) { const int64_t mid = (l + h + 1) >> 1; if (r.off[mid] <= lo) l = mid; else h = mid - 1; }
        g = l; k = lo - r.off[g];
    }
    TokGene t = tok_gene(a, g);
    // the whole piece lies in one gene (ragged) or in the first W elements of one row (padded): hi == e0 + PER follows
    if (e0 >= 0 && k + PER <= (PADDED ? r.W : t.len)) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const T v = tok_at<T>(a, t, s_vocab, k + j);
            if (EB == 1) w[j >> 2] |= (uint32_t)(uint8_t)v << (8 * (j & 3));
            else if (EB == 4) w[j] = (uint32_t)v;
            else { w[2 * j] = (uint32_t)(uint64_t)v; w[2 * j + 1] = (uint32_t)((uint64_t)v >> 32); }
        }
        *reinterpret_cast<uint4*>(r.out0 + piece * 16) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
    for (int64_t e = lo; e < hi; e++, k++) {
        if (PADDED) {
            if (k == r.S) { k = 0; g++; t = tok_gene(a, g); }            // (e < n_elems: the row exists)
            if (k < r.W) out[e] = tok_at<T>(a, t, s_vocab, k);
        } else {
            if (k == t.len) { do g++; while (r.off[g + 1] == r.off[g]); k = 0; t = tok_gene(a, g); }   // (empty genes are stepped over; e < off[G] ends it)
            out[e] = tok_at<T>(a, t, s_vocab, k);
        }
    }
}
