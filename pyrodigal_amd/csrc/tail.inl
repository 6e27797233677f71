// The traceback tail on the device (included by finder.hip): the path of every contig, its untangling, the bad-gene elimination,
// the gene list, the start tweaks and the public gene records.  The rules are tail_rules.h's, one text each; the kernels here are
// the forms -- who enumerates, where the path lives, how a scan is carried.
//
// ref: lib.pyx:1253-1311 (_disentangle_overlaps, _max_forward_pointers, tracef), Prodigal dprog.c eliminate_bad_genes
// (call sites lib.pyx:5308, 5369), lib.pyx:3231-3270 (Genes._extract), 3272-3401 (Genes._tweak_final_starts).
//
// The reference follows traceb from the best gene end back to the head of the path, one node after the other, three
// times (two untangling passes that splice nodes into the path, one pass that sets tracef), then walks the path twice
// more.  One device thread per contig does the same at one memory round trip per step (k_tail_path): fine for a batch
// of small contigs side by side, hopeless for a genome (18 k steps).  The parallel forms:
//   * the nodes ON the path are found by pointer doubling: in round k every node's pointer reaches its 2^k-th traceb
//     ancestor and every marked node marks that ancestor, starting from the best gene end -- every ancestor of a marked node
//     is itself on the path, so the order inside a round does not matter; log2(longest chain) rounds;
//   * traceb always points to a smaller index, so the path in walk order is simply the marked nodes in decreasing index
//     order: a prefix sum over the marks gives every node its position;
//   * both untangling passes only look at one path edge (p, traceb[p]) at a time and splice 0, 1 or 2 nodes into it
//     (splice_of); the nodes they splice in never satisfy a splice condition themselves (the start of an overlapping gene is
//     no stop; the reverse stop spliced in by the first pass has its ov_mark reset; no second-pass rule fires on the new
//     edges), so the final path is the original one with per-edge insertions, counted before the prefix sum;
//   * elimination and the gene list are per-path-position work with neighbours (elim_add_terms, elim_mark_pair,
//     tp_extract_item: the reference's "last begin / end / start node / stop node seen" state becomes four running maxima
//     of positions, carried by tp_wave_scan across a wavefront and by tp_extract_rounds or the chunk pair beyond it).
// The start tweaks follow: every gene against its ORIGINAL neighbours (k_tail_tweak, _packed, _wave: a thread or a wavefront
// per gene over the same tweak_context .. tweak_pick), then k_tail_tweak_fixup redoes in order what the reference's in-order
// loop would have seen differently, and k_emit_genes writes the records (gene_record).

struct TpSeg { int64_t off; int32_t n; int32_t contig; };     // winning chains in the gathered arrays, ascending `off`

struct TpWork {
    const TpSeg* seg; int n_seg;
    int64_t nw;                 // nodes of all winning chains
    int levels;                 // 2^levels >= longest chain
    int32_t* up;                // [2][nw] global index of the 2^k-th ancestor in round k (a head points to itself), ping-pong
    uint8_t* mark;              // node is on the path
    int32_t* slots;             // path positions the node takes: itself + what the untangling splices in after it
    int32_t* ins;               // [nw][2] the spliced-in nodes (chain index), -1 = none
    int32_t* excl;              // [nw + 1] exclusive prefix sum of slots
    int32_t* bsum;              // per 256 nodes
    int32_t* cnt;               // [n_seg] path length
};

__device__ inline int contig_of_slot(const TailDesc* __restrict__ td, int n_contigs, int64_t slot) {
    return owner_of([&](const int k) { return td[k].gene_off; }, n_contigs, slot);
}
__device__ inline int tp_seg_of(const TpSeg* __restrict__ seg, int n_seg, int64_t g) {
    return owner_of([&](const int k) { return seg[k].off; }, n_seg, g);
}

__device__ inline NodeView node_view(const TailDesc& d, const OutArrays& o, int32_t* tracef, uint8_t* elim) {
    const int64_t oo = d.out_off;
    if (o.direct) {
        const int64_t t = d.topo_off, a = d.dp_off; const int g = d.group;
        return NodeView{d.n, o.g_ndx[g] + t, o.g_stop_val[g] + t, o.g_type[g] + t, o.g_strand[g] + t, o.c_edge + a,
                        const_cast<double*>(o.c_cscore) + a, o.sscore_dp + oo, o.c_rscore + a, o.c_uscore + a, o.c_tscore + a,
                        o.c_star_ptr + 3 * a, o.traceb + oo, tracef + oo, o.ov_mark + oo, o.d_score + a, elim + oo};
    }
    return NodeView{d.n, o.ndx + oo, o.stop_val + oo, o.type + oo, o.strand + oo, o.edge_dp + oo,
                    o.cscore_dp + oo, o.sscore_dp + oo, o.rscore_dp + oo, o.uscore_dp + oo, o.tscore_dp + oo,
                    o.star_ptr + 3 * oo, o.traceb + oo, tracef + oo, o.ov_mark + oo, o.score + oo, elim + oo};
}

// the tail's starting state in one launch (it was four or five memsets): tracef = -1, elim = 0 for every gathered node; the per-contig
// counters of changed genes and of genes; the per-chain counters of the many-launch path
__global__ void __launch_bounds__(256)
k_tail_init(int32_t* __restrict__ tracef, uint8_t* __restrict__ elim, const int64_t n_nodes, int32_t* __restrict__ nchanged, int32_t* __restrict__ ngenes /* or nullptr */,
            const int n_contigs, int32_t* __restrict__ seg_cnt /* or nullptr */, const int n_segs) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k = t; k <= n_nodes; k += stride) { tracef[k] = -1; elim[k] = 0; }
    for (int64_t k = t; k <= n_contigs; k += stride) { nchanged[k] = 0; if (ngenes != nullptr) ngenes[k] = 0; }
    if (seg_cnt != nullptr) for (int64_t k = t; k < n_segs; k += stride) seg_cnt[k] = 0;
}

// One thread per contig: untangle the traceback, eliminate bad genes, list the genes, each as the reference's serial walk.
// A path is a pointer chase, so contigs are the parallel axis.
__global__ void __launch_bounds__(64)
k_tail_path(const TailDesc* __restrict__ td, int n_contigs, OutArrays o, int32_t* tracef, uint8_t* elim, int32_t* __restrict__ path,
            GeneRec* __restrict__ genes, int32_t* __restrict__ n_genes) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_contigs) return;
    const TailDesc d = td[i];
    int ng = 0;
    if (d.n > 0 && d.mx >= 0) {
        NodeView v = node_view(d, o, tracef, elim);
        int32_t* pl = path + d.out_off;                  // at most n entries
        const int cnt = untangle(v, d.mx, pl);
        if (v.traceb[d.mx] != -1) {                      // ipath != -1
            eliminate_bad_genes(v, pl, cnt, d.st_wt);
            ng = extract_genes(v, pl, cnt, genes + d.gene_off);
        }
    }
    n_genes[i] = ng;
}

// ---- the many-launch form: a thread per node of every winning chain ---------------------------------------------------------------
__global__ void __launch_bounds__(256)
k_tp_init(TpWork w, const TailDesc* __restrict__ td, OutArrays o) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= w.nw) return;
    const TpSeg s = w.seg[tp_seg_of(w.seg, w.n_seg, g)];
    const int i = (int)(g - s.off);
    const int tb = o.traceb[g];
    w.up[g] = tb >= 0 ? (int32_t)(s.off + tb) : (int32_t)g;
    w.mark[g] = i == td[s.contig].mx ? 1 : 0;
}

// one round of pointer doubling: every marked node marks its 2^k-th ancestor, every node's pointer doubles its reach.
// After round k the marks cover the first 2^(k+1) nodes of the path (a node marked during the round may already pass the
// mark on: whatever it reaches is an ancestor of the best gene end, hence on the path).
__global__ void __launch_bounds__(256)
k_tp_jump(TpWork w, const int32_t* __restrict__ up_in, int32_t* __restrict__ up_out) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= w.nw) return;
    const int a = up_in[g];
    if (w.mark[g]) w.mark[a] = 1;
    up_out[g] = up_in[a];
}
// Eight hops per launch (round 6): pointers that reach R nodes become pointers that reach 8 R, a marked node marks its ancestors at R, 2 R,
// .. 7 R -- after round k the marks cover the first 8^(k+1) nodes of the path, six launches for a chain of 262 144 nodes where the
// doubling form takes eighteen (a launch of this kind is 3 us of work and 4 us of gap to the next: the genome-sized calls pay per launch).
__global__ void __launch_bounds__(256)
k_tp_jump8(TpWork w, const int32_t* __restrict__ up_in, int32_t* __restrict__ up_out) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= w.nw) return;
    const bool m = w.mark[g] != 0;
    int a = up_in[g];
#pragma unroll
    for (int h = 0; h < 7; h++) {
        if (m) w.mark[a] = 1;
        a = up_in[a];
    }
    up_out[g] = a;
}

// what the two untangling passes splice in after path node p (edge p -> nx = traceb[p])
__global__ void __launch_bounds__(256)
k_tp_slots(TpWork w, const TailDesc* __restrict__ td, OutArrays o) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= w.nw) return;
    Splice sp{0, -1, -1};
    if (w.mark[g]) {
        const TpSeg s = w.seg[tp_seg_of(w.seg, w.n_seg, g)];
        const NodeView v = node_view(td[s.contig], o, nullptr, nullptr);
        const int p = (int)(g - s.off);
        sp = splice_of(v, p, v.traceb[p]);
    }
    w.slots[g] = sp.slots; w.ins[2 * g] = sp.i0; w.ins[2 * g + 1] = sp.i1;
}

// exclusive prefix sum of slots over all nodes: block sums, their scan, the final values
__global__ void __launch_bounds__(256)
k_tp_scan1(TpWork w) {
    __shared__ int s_w[4];
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int v = g < w.nw ? w.slots[g] : 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) w.bsum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
__global__ void __launch_bounds__(1024)
k_tp_scan2(TpWork w, const int nblocks) {
    __shared__ int s_wsum[16];
    __shared__ int s_base;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t == 0) s_base = 0;
    __syncthreads();
    for (int q0 = 0; q0 < nblocks; q0 += 1024) {
        const int q = q0 + t;
        const int c = q < nblocks ? w.bsum[q] : 0;
        int inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const int o2 = __shfl_up(inc, d, 64); if (lane >= d) inc += o2; }
        if (lane == 63) s_wsum[wave] = inc;
        __syncthreads();
        int woff = 0;
        for (int k = 0; k < wave; k++) woff += s_wsum[k];
        const int base = s_base;
        if (q < nblocks) w.bsum[q] = base + woff + inc - c;
        __syncthreads();
        if (t == 1023) s_base = base + woff + inc;
        __syncthreads();
    }
    if (t == 0) w.excl[w.nw] = s_base;
}
__global__ void __launch_bounds__(256)
k_tp_scan3(TpWork w) {
    __shared__ int s_w[4];
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = g < w.nw ? w.slots[g] : 0;
    int inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o2 = __shfl_up(inc, d, 64); if (lane >= d) inc += o2; }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int woff = 0;
    for (int k = 0; k < wave; k++) woff += s_w[k];
    if (g < w.nw) w.excl[g] = w.bsum[blockIdx.x] + woff + inc - c;
}

// the path lists (path[0] = the best gene end, path[cnt - 1] = the head), ov_mark of the reverse stops spliced in
__global__ void __launch_bounds__(256)
k_tp_fill(TpWork w, OutArrays o, int32_t* __restrict__ path) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= w.nw) return;
    const int sl = w.slots[g];
    if (sl == 0) return;
    const int si = tp_seg_of(w.seg, w.n_seg, g);
    const TpSeg s = w.seg[si];
    const int q = w.excl[s.off + s.n] - w.excl[g] - sl;          // path positions taken by the nodes after g in walk order
    int32_t* pl = path + s.off;
    pl[q] = (int32_t)(g - s.off);
    if (sl >= 2) pl[q + 1] = w.ins[2 * g];
    if (sl == 3) { pl[q + 2] = w.ins[2 * g + 1]; o.ov_mark[s.off + w.ins[2 * g + 1]] = -1; }
    if (q == 0) w.cnt[si] = w.excl[s.off + s.n] - w.excl[s.off];      // the best gene end: first in walk order
}

// traceb / tracef along the final path
__global__ void __launch_bounds__(256)
k_tp_link(TpWork w, OutArrays o, const int32_t* __restrict__ path, int32_t* __restrict__ tracef) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= w.nw) return;
    const int si = tp_seg_of(w.seg, w.n_seg, g);
    const TpSeg s = w.seg[si];
    const int q = (int)(g - s.off);
    if (q + 1 >= w.cnt[si]) return;
    const int x = path[s.off + q], y = path[s.off + q + 1];
    o.traceb[s.off + x] = y; tracef[s.off + y] = x;
}

// eliminate_bad_genes: a thread per path position, the first loop and then the second
__global__ void __launch_bounds__(256)
k_tp_elim_a(TpWork w, const TailDesc* __restrict__ td, OutArrays o, const int32_t* __restrict__ path) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= w.nw) return;
    const int si = tp_seg_of(w.seg, w.n_seg, g);
    const TpSeg s = w.seg[si];
    const int q = (int)(g - s.off), cnt = w.cnt[si];
    if (q >= cnt || cnt < 2) return;                  // cnt < 2: the best gene end has no traceb (ref: lib.pyx:1311)
    const TailDesc d = td[s.contig];
    elim_add_terms(node_view(d, o, nullptr, nullptr), path + s.off, cnt, q, d.st_wt);
}
__global__ void __launch_bounds__(256)
k_tp_elim_b(TpWork w, const TailDesc* __restrict__ td, OutArrays o, const int32_t* __restrict__ path, uint8_t* __restrict__ elim) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= w.nw) return;
    const int si = tp_seg_of(w.seg, w.n_seg, g);
    const TpSeg s = w.seg[si];
    const int q = (int)(g - s.off), cnt = w.cnt[si];
    if (q < 1 || q >= cnt) return;
    elim_mark_pair(node_view(td[s.contig], o, nullptr, elim), path + s.off, q);
}

// ---- gene list: how the four running maxima and the emit count of tp_extract_item are carried ---------------------------------------
// inclusive scan over the wavefront
__device__ inline void tp_wave_scan(int* m /* [4] */, int& emits, const int lane) {
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) { const int o2 = __shfl_up(m[k], dd, 64); if (lane >= dd) m[k] = max(m[k], o2); }
        const int o3 = __shfl_up(emits, dd, 64); if (lane >= dd) emits += o3;
    }
}
// ... and their totals over the wavefront, in every lane (m[4] is the count)
__device__ inline void tp_wave_total(int* m /* [5] */) {
#pragma unroll
    for (int dd = 32; dd >= 1; dd >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) m[k] = max(m[k], __shfl_xor(m[k], dd, 64));
        m[4] += __shfl_xor(m[4], dd, 64);
    }
}

// One workgroup goes over the path `pl` (global memory or LDS) from its head in rounds of blockDim.x positions.  s_carry (-1) and
// s_ng (0) are set and synchronised by the caller; s_ng ends as the number of genes.
__device__ inline void tp_extract_rounds(const NodeView& v, const int32_t* pl, const uint8_t* el, const int cnt, GeneRec* __restrict__ out,
                                         int (*s_sc)[4], int* s_cnt, int* s_carry, int* s_ng) {
    const int t = threadIdx.x, nthr = blockDim.x, lane = t & 63, wave = t >> 6;
    for (int r0 = 0; r0 < cnt; r0 += nthr) {
        const int r = r0 + t;
        const ExtractItem it = tp_extract_item(v, pl, el, cnt, r);
        int m[4] = {it.set_b ? r : -1, it.set_e ? r : -1, it.set_s ? r : -1, it.set_t ? r : -1};
        int e1 = it.emit() ? 1 : 0;
        tp_wave_scan(m, e1, lane);
        if (lane == 63) { for (int k = 0; k < 4; k++) s_sc[wave][k] = m[k]; s_cnt[wave] = e1; }
        __syncthreads();
        int eoff = *s_ng;
        for (int k2 = 0; k2 < wave; k2++) {
            for (int k = 0; k < 4; k++) m[k] = max(m[k], s_sc[k2][k]);
            eoff += s_cnt[k2];
        }
        for (int k = 0; k < 4; k++) m[k] = max(m[k], s_carry[k]);
        if (it.emit()) out[eoff + e1 - 1] = tp_gene_at(v, pl, cnt, m);
        __syncthreads();
        if (t == nthr - 1) { for (int k = 0; k < 4; k++) s_carry[k] = m[k]; *s_ng = eoff + e1; }
        __syncthreads();
    }
}

// Genes._extract, one workgroup per contig
__global__ void __launch_bounds__(1024)
k_tp_extract(TpWork w, const TailDesc* __restrict__ td, OutArrays o, const int32_t* __restrict__ path, const uint8_t* __restrict__ elim,
             GeneRec* __restrict__ genes, int32_t* __restrict__ n_genes) {
    __shared__ int s_sc[16][4];      // per wave: running maxima of the four setters, then the emit count
    __shared__ int s_cnt[16];
    __shared__ int s_carry[4];       // last setter position (in processing order) of b, e, s, t before this round
    __shared__ int s_ng;
    const int si = blockIdx.x;
    const TpSeg s = w.seg[si];
    const TailDesc d = td[s.contig];
    const int cnt = w.cnt[si];
    const int t = threadIdx.x;
    if (t == 0) { s_ng = 0; }
    if (t < 4) s_carry[t] = -1;
    __syncthreads();
    if (cnt < 2) { if (t == 0) n_genes[s.contig] = 0; return; }
    tp_extract_rounds(node_view(d, o, nullptr, nullptr), path + s.off, elim + s.off, cnt, genes + d.gene_off, s_sc, s_cnt, s_carry, &s_ng);
    if (t == 0) n_genes[s.contig] = s_ng;
}

// ---- all of the above in ONE launch when every winning chain fits the LDS of a workgroup (batches of short contigs) ----
// A workgroup per contig.  The chain's traceb goes to LDS in one coalesced pass; ONE lane then follows it from the best gene end
// to the head of the path -- a pointer chase, but through LDS (a path of a 20 kbp contig is some sixty nodes: a few microseconds) --
// and what it lists IS the path in walk order, so marks, pointer doubling and the prefix sum over all nodes of the batch (twenty
// launches over every node of every winning chain) are not needed: the splices are counted per path position, a prefix sum over
// the path places them, and the passes that follow (links, the two elimination loops, the gene list) run over the final path in
// LDS.
constexpr int TP_SMALL_MAX = 4096;        // nodes of the longest chain: 3 arrays of int32 in LDS (48 KB)
constexpr int TP_SPLICED_STOP = 1 << 30;  // tag of a path entry: the reverse stop the first untangling pass splices in (its ov_mark is reset)

__device__ inline int tp_block_excl_scan(int v, int* s_w, int& total) {     // exclusive scan over the workgroup; total = sum
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwv = blockDim.x >> 6;
    int inc = v;
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) { const int x = __shfl_up(inc, dd, 64); if (lane >= dd) inc += x; }
    __syncthreads();                        // s_w may still be read from the previous round
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    int off = 0; total = 0;
    for (int k = 0; k < nwv; k++) { if (k < wave) off += s_w[k]; total += s_w[k]; }
    return off + inc - v;
}

__global__ void __launch_bounds__(256)
k_tp_small(TpWork w, const TailDesc* __restrict__ td, OutArrays o, int32_t* __restrict__ tracef, uint8_t* __restrict__ elim,
           GeneRec* __restrict__ genes, int32_t* __restrict__ n_genes, const int cap) {
    extern __shared__ int32_t s_dyn[];
    int32_t* s_tb = s_dyn; int32_t* s_base = s_dyn + cap; int32_t* s_pl = s_dyn + 2 * cap;
    __shared__ int s_w[4], s_m;
    __shared__ int s_sc[4][4], s_cnt[4], s_carry[4], s_ng;
    const int si = blockIdx.x;
    const TpSeg s = w.seg[si];
    const TailDesc d = td[s.contig];
    const int n = s.n, t = threadIdx.x, nthr = blockDim.x;
    NodeView v = node_view(d, o, tracef, elim);
    for (int i = t; i < n; i += nthr) s_tb[i] = v.traceb[i];
    if (t == 0) { s_ng = 0; s_m = 0; }
    if (t < 4) s_carry[t] = -1;
    __syncthreads();
    if (t == 0 && d.mx >= 0) { int m = 0; for (int p = d.mx; p != -1; p = s_tb[p]) s_base[m++] = p; s_m = m; }
    __syncthreads();
    const int m = s_m;
    // what the two untangling passes splice in after path node p (edge p -> nx)
    int cnt = 0;
    for (int k0 = 0; k0 < m; k0 += nthr) {
        const int k = k0 + t;
        Splice sp{0, -1, -1};
        int p = -1;
        if (k < m) { p = s_base[k]; sp = splice_of(v, p, s_tb[p]); }
        int total;
        const int q = cnt + tp_block_excl_scan(sp.slots, s_w, total);
        if (q + sp.slots <= cap) {        // always: the spliced-in nodes are nodes of the chain that are not on the path
            if (sp.slots >= 1) s_pl[q] = p;
            if (sp.slots >= 2) s_pl[q + 1] = sp.i0;
            if (sp.slots == 3) s_pl[q + 2] = sp.i1 | TP_SPLICED_STOP;
        }
        cnt += total;
    }
    cnt = min(cnt, cap);
    __syncthreads();
    // ov_mark of the spliced-in reverse stops (after every splice was decided: the decisions read ov_mark), traceb / tracef along the path
    for (int q = t; q < cnt; q += nthr) {
        const int e = s_pl[q];
        if (e & TP_SPLICED_STOP) { v.ov_mark[e & ~TP_SPLICED_STOP] = -1; s_pl[q] = e & ~TP_SPLICED_STOP; }
    }
    __syncthreads();
#pragma unroll 1
    for (int q = t; q + 1 < cnt; q += nthr) { const int x = s_pl[q], y = s_pl[q + 1]; v.traceb[x] = y; v.tracef[y] = x; }
    if (cnt < 2) { if (t == 0) n_genes[s.contig] = 0; return; }          // the best gene end has no traceb (ref: lib.pyx:1311)
    // eliminate_bad_genes: the first loop, then the second over the finished scores
    for (int q = t; q < cnt; q += nthr) elim_add_terms(v, s_pl, cnt, q, d.st_wt);
    __threadfence_block();
    __syncthreads();
    for (int q = 1 + t; q < cnt; q += nthr) elim_mark_pair(v, s_pl, q);
    __threadfence_block();
    __syncthreads();
    tp_extract_rounds(v, s_pl, v.elim, cnt, genes + d.gene_off, s_sc, s_cnt, s_carry, &s_ng);
    if (t == 0) n_genes[s.contig] = s_ng;
}

// ---- Genes._extract for genomes: the path cut into chunks of 1024 positions, a workgroup per chunk -----------------------------
// k_tp_extract is one workgroup per contig; a genome's path has some 400 000 positions, i.e. 400 rounds of one workgroup while
// the rest of the chip idles (1.5 ms on config 5).  Here every chunk first reports what it sets -- the last position (in
// processing order) that sets begin / end / start node / stop node, and how many genes it emits (k_tp_extract_sum) -- and then
// emits its genes with the carries of the chunks before it, which it combines itself (k_tp_extract_chunk).
struct TpChunkSum { int32_t m[4]; int32_t emits; int32_t _pad[3]; };

// the totals of a workgroup of sixteen wavefronts (four maxima, one count), in thread 0
__device__ inline void tp_block_total(int* m /* [5] */, int (*s_sc)[5]) {
    tp_wave_total(m);
    if ((threadIdx.x & 63) == 0) for (int k = 0; k < 5; k++) s_sc[threadIdx.x >> 6][k] = m[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < 4; k++) m[k] = -1;
        m[4] = 0;
        for (int k2 = 0; k2 < 16; k2++) { for (int k = 0; k < 4; k++) m[k] = max(m[k], s_sc[k2][k]); m[4] += s_sc[k2][4]; }
    }
}

__global__ void __launch_bounds__(1024)
k_tp_extract_sum(TpWork w, const TailDesc* __restrict__ td, OutArrays o, const int32_t* __restrict__ path, const uint8_t* __restrict__ elim,
                 TpChunkSum* __restrict__ sums, const int chunks_per_seg) {
    __shared__ int s_sc[16][5];
    const int si = blockIdx.y, b = blockIdx.x;
    const TpSeg s = w.seg[si];
    const int cnt = w.cnt[si];
    if (cnt < 2 || b * 1024 >= cnt) return;
    const NodeView v = node_view(td[s.contig], o, nullptr, nullptr);
    const int r = b * 1024 + threadIdx.x;
    const ExtractItem it = tp_extract_item(v, path + s.off, elim + s.off, cnt, r);
    int m[5] = {it.set_b ? r : -1, it.set_e ? r : -1, it.set_s ? r : -1, it.set_t ? r : -1, it.emit() ? 1 : 0};
    tp_block_total(m, s_sc);
    if (threadIdx.x == 0) sums[(size_t)si * chunks_per_seg + b] = TpChunkSum{{m[0], m[1], m[2], m[3]}, m[4], {0, 0, 0}};
}

__global__ void __launch_bounds__(1024)
k_tp_extract_chunk(TpWork w, const TailDesc* __restrict__ td, OutArrays o, const int32_t* __restrict__ path, const uint8_t* __restrict__ elim,
                   const TpChunkSum* __restrict__ sums, const int chunks_per_seg, GeneRec* __restrict__ genes, int32_t* __restrict__ n_genes) {
    __shared__ int s_sc[16][5];
    __shared__ int s_carry[5];
    const int si = blockIdx.y, b = blockIdx.x;
    const TpSeg s = w.seg[si];
    const int cnt = w.cnt[si];
    if (cnt < 2) { if (b == 0 && threadIdx.x == 0) n_genes[s.contig] = 0; return; }
    if (b * 1024 >= cnt) return;
    const TailDesc d = td[s.contig];
    const NodeView v = node_view(d, o, nullptr, nullptr);
    const int32_t* pl = path + s.off;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // what the chunks before this one leave behind
    {
        int c[5] = {-1, -1, -1, -1, 0};
        for (int k = t; k < b; k += 1024) {
            const TpChunkSum cs = sums[(size_t)si * chunks_per_seg + k];
            for (int q = 0; q < 4; q++) c[q] = max(c[q], cs.m[q]);
            c[4] += cs.emits;
        }
        tp_block_total(c, s_sc);
        if (t == 0) for (int q = 0; q < 5; q++) s_carry[q] = c[q];
        __syncthreads();
    }
    const int r = b * 1024 + t;
    const ExtractItem it = tp_extract_item(v, pl, elim + s.off, cnt, r);
    int mm[4] = {it.set_b ? r : -1, it.set_e ? r : -1, it.set_s ? r : -1, it.set_t ? r : -1};
    int e1 = it.emit() ? 1 : 0;
    tp_wave_scan(mm, e1, lane);
    __syncthreads();                                   // s_sc is read above
    if (lane == 63) { for (int k = 0; k < 4; k++) s_sc[wave][k] = mm[k]; s_sc[wave][4] = e1; }
    __syncthreads();
    int eoff = s_carry[4];
    for (int k2 = 0; k2 < wave; k2++) {
        for (int k = 0; k < 4; k++) mm[k] = max(mm[k], s_sc[k2][k]);
        eoff += s_sc[k2][4];
    }
    for (int k = 0; k < 4; k++) mm[k] = max(mm[k], s_carry[k]);
    if (it.emit()) genes[d.gene_off + eoff + e1 - 1] = tp_gene_at(v, pl, cnt, mm);
    if (r == cnt - 1) n_genes[s.contig] = eoff + e1;      // the last position of the path closes the count
}

// ---- start tweaks (Genes._tweak_final_starts) ------------------------------------------------------------------------------------------
// The reference loop runs in gene order: gene i sees its predecessor already tweaked and its successor untouched.  Here every
// gene is first tweaked against its ORIGINAL neighbours (a thread or a wavefront per gene), then k_tail_tweak_fixup redoes, in
// order, the genes whose predecessor did change (tweaks are rare).

// the record of the parallel pass and whether the in-order pass has to look at the gene behind it
__device__ inline void tweak_store(const NodeView& v, const GeneRec& cur, const GeneRec& orig, const int64_t slot, const int c,
                                   GeneRec* __restrict__ out, uint8_t* __restrict__ changed, int32_t* __restrict__ n_changed) {
    out[slot] = cur;
    const bool moved = tweak_moved_reverse_start(v, cur, orig);
    changed[slot] = moved ? 1 : 0;
    if (moved) atomicAdd(&n_changed[c], 1);
}

// one thread per gene slot (a contig of n nodes has n / 2 + 2 of them, mostly empty)
__global__ void __launch_bounds__(256)
k_tail_tweak(const TailDesc* __restrict__ td, int n_contigs, int64_t n_slots, OutArrays o, int32_t* tracef, uint8_t* elim,
             const GeneRec* __restrict__ orig, GeneRec* __restrict__ out, const int32_t* __restrict__ n_genes, int maxov,
             uint8_t* __restrict__ changed, int32_t* __restrict__ n_changed) {
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_slots) return;
    const int c = contig_of_slot(td, n_contigs, slot);
    const TailDesc d = td[c];
    const int g = (int)(slot - d.gene_off), ng = n_genes[c];
    if (g >= ng) return;
    const NodeView v = node_view(d, o, tracef, elim);
    const GeneRec* base = orig + d.gene_off;
    GeneRec cur = base[g];
    tweak_one(v, g > 0 ? &base[g - 1] : nullptr, cur, g < ng - 1 ? &base[g + 1] : nullptr, d.st_wt, maxov);
    tweak_store(v, cur, base[g], slot, c, out, changed, n_changed);
}

// running sum of n_genes: gpre[c] = genes of the contigs before c, gpre[n_contigs] = genes of the batch
__global__ void __launch_bounds__(1024)
k_gene_prefix(const int32_t* __restrict__ n_genes, int n_contigs, int32_t* __restrict__ gpre) {
    __shared__ int s_w[16];
    __shared__ int s_carry;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < n_contigs; base += 1024) {
        const int v = base + t < n_contigs ? n_genes[base + t] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int x = __shfl_up(inc, o, 64); if (lane >= o) inc += x; }
        if (lane == 63) s_w[w] = inc;
        __syncthreads();
        int run = s_carry + inc - v;
        for (int k = 0; k < w; k++) run += s_w[k];
        if (base + t < n_contigs) gpre[base + t] = run;
        __syncthreads();
        if (t == 1023) s_carry = run + v;
        __syncthreads();
    }
    if (t == 0) gpre[n_contigs] = s_carry;
}
// k_tail_tweak over the genes themselves instead of over their (mostly empty) slots: gene number q of the batch is gene q - gpre[c]
// of the contig c with gpre[c] <= q < gpre[c + 1] (k_gene_prefix).  With many short contigs the genes are a few per contig: one
// thread per slot leaves a handful of busy lanes in each of twenty thousand wavefronts, each of which takes as long as its slowest
// lane; packed, the same lanes fill a few hundred.
__global__ void __launch_bounds__(256)
k_tail_tweak_packed(const TailDesc* __restrict__ td, int n_contigs, OutArrays o, int32_t* tracef, uint8_t* elim,
                    const GeneRec* __restrict__ orig, GeneRec* __restrict__ out, const int32_t* __restrict__ n_genes, int maxov,
                    uint8_t* __restrict__ changed, int32_t* __restrict__ n_changed, const int32_t* __restrict__ gpre) {
    const int total = gpre[n_contigs];
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < total; q += gridDim.x * blockDim.x) {
        const int c = owner_of([&](const int k) { return gpre[k]; }, n_contigs, q);
        const int g = q - gpre[c], ng = n_genes[c];
        const TailDesc d = td[c];
        const NodeView v = node_view(d, o, tracef, elim);
        const GeneRec* base = orig + d.gene_off;
        GeneRec cur = base[g];
        tweak_one(v, g > 0 ? &base[g - 1] : nullptr, cur, g < ng - 1 ? &base[g + 1] : nullptr, d.st_wt, maxov);
        tweak_store(v, cur, base[g], d.gene_off + g, c, out, changed, n_changed);
    }
}

// tweak_one with the wavefront on ONE gene: the 200 candidate nodes are filtered and priced by the lanes (that is where the
// memory traffic is), the few that pass are then merged one after the other in index order, as the reference's loop
// meets them.  Every lane returns the same record.
__device__ void tweak_one_wave(const NodeView& v, const GeneRec* prev, GeneRec& cur, const GeneRec* next, double w, int maxov, const int lane) {
    const int nn = v.n;
    const TweakCtx c = tweak_context(v, prev, cur, next, w, maxov);
    TwoBest best;
    for (int base = c.ndx - 100; base < c.ndx + 100; base += 64) {
        const int j = base + lane;
        bool cand = j >= 0 && j < nn && j != c.ndx && j < c.ndx + 100;
        double tg = 0.0, cs = 0.0;
        if (cand) cand = tweak_same_orf_start(v, c, j);
        if (cand) cand = tweak_price(v, c, j, tg);
        if (cand) cs = v.cscore[j] + v.sscore[j];
        unsigned long long m = __ballot(cand);
        while (m) {
            const int k = __builtin_ctzll(m);
            m &= m - 1ull;
            tweak_take(best, base + k, __shfl(cs, k, 64), __shfl(tg, k, 64));
        }
    }
    tweak_pick(v, c, best, cur);
}

// k_tail_tweak for long contigs: a genome has few thousand genes, too few for one thread each to hide the latency of a
// 200-candidate scan, so every gene gets a wavefront (tweak_one_wave); blockIdx.y = contig, four genes per workgroup.
__global__ void __launch_bounds__(256)
k_tail_tweak_wave(const TailDesc* __restrict__ td, int n_contigs, OutArrays o, int32_t* tracef, uint8_t* elim,
                  const GeneRec* __restrict__ orig, GeneRec* __restrict__ out, const int32_t* __restrict__ n_genes, int maxov,
                  uint8_t* __restrict__ changed, int32_t* __restrict__ n_changed) {
    const int c = blockIdx.y, lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), ng = n_genes[c];
    if (g >= ng) return;
    const TailDesc d = td[c];
    const NodeView v = node_view(d, o, tracef, elim);
    const GeneRec* base = orig + d.gene_off;
    GeneRec cur = base[g];
    GeneRec prev{}, nxt{};
    if (g > 0) prev = base[g - 1];
    if (g < ng - 1) nxt = base[g + 1];
    tweak_one_wave(v, g > 0 ? &prev : nullptr, cur, g < ng - 1 ? &nxt : nullptr, d.st_wt, maxov, lane);
    if (lane != 0) return;
    tweak_store(v, cur, base[g], d.gene_off + g, c, out, changed, n_changed);
}

// The in-order pass over the genes whose predecessor moved (the reference's loop semantics, ref: lib.pyx:3272-3401): one
// workgroup per contig, windows of 64 genes.  A window only depends on the one before it through its first gene's
// predecessor, and only if that predecessor -- the last gene of the window before -- was itself redone: so every wavefront
// first runs its windows assuming it was not (phase 1, all windows side by side), then one wavefront goes over the
// windows in order and redoes, from their parallel-pass state, those whose assumption failed (phase 2, rare).  Within a
// window genes are taken in order; a redone gene's 200 candidates are priced by the lanes (tweak_one_wave).
//   par / ch0   the parallel pass (k_tail_tweak): records against the ORIGINAL neighbours, "start moved on the reverse strand"
//   fin / chf   the final records and flags
#define PGA_FIX_MAXWIN 4096
__global__ void __launch_bounds__(1024)
k_tail_tweak_fixup(const TailDesc* __restrict__ td, int n_contigs, OutArrays o, int32_t* tracef, uint8_t* elim,
                   const GeneRec* __restrict__ orig, const GeneRec* __restrict__ par_all, const int32_t* __restrict__ n_genes, int maxov,
                   const uint8_t* __restrict__ ch0_all, const int32_t* __restrict__ n_changed, GeneRec* __restrict__ fin_all,
                   uint8_t* __restrict__ chf_all) {
    __shared__ uint8_t s_redone[PGA_FIX_MAXWIN];
    const int c = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    if (c >= n_contigs) return;
    const TailDesc d = td[c];
    const int ng = n_genes[c];
    const GeneRec* ob = orig + d.gene_off; const GeneRec* par = par_all + d.gene_off; const uint8_t* ch0 = ch0_all + d.gene_off;
    GeneRec* fin = fin_all + d.gene_off; uint8_t* chf = chf_all + d.gene_off;
    for (int g = threadIdx.x; g < ng; g += blockDim.x) { fin[g] = par[g]; chf[g] = ch0[g]; }
    if (n_changed[c] == 0 || ng < 2) return;
    __threadfence_block();
    __syncthreads();
    const NodeView v = node_view(d, o, tracef, elim);
    const int nwin = (ng - 1 + 63) >> 6;                  // genes 1 .. ng-1
    // one window, in gene order; `assume`: its first gene's predecessor is as the parallel pass left it.  Returns whether the
    // window's last gene was redone (then the next window may not assume that).
    auto run_window = [&](const int w, const bool assume) -> bool {
        const int g0 = 1 + (w << 6), g1 = min(ng, g0 + 64);
        const int g = g0 + lane;
        if (!assume) {
            if (g < g1) { fin[g] = par[g]; chf[g] = ch0[g]; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
        const int pf = g < g1 ? ((lane == 0 && !assume) ? chf[g - 1] : ch0[g - 1]) : 0;
        unsigned long long mask = __ballot(pf != 0);
        bool last = false;
        while (mask) {
            const int k = __builtin_ctzll(mask);
            mask &= mask - 1ull;
            const int gg = g0 + k;
            GeneRec cur = ob[gg];
            const GeneRec prev = (k == 0 && assume) ? par[gg - 1] : fin[gg - 1];
            GeneRec nxt{};
            if (gg < ng - 1) nxt = ob[gg + 1];
            tweak_one_wave(v, &prev, cur, gg < ng - 1 ? &nxt : nullptr, d.st_wt, maxov, lane);
            const int nf = tweak_moved_reverse_start(v, cur, ob[gg]);
            if (lane == 0) { fin[gg] = cur; chf[gg] = (uint8_t)nf; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");     // fin[gg] is read back by all lanes if gg + 1 is redone
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            // the next gene's predecessor flag is this gene's new flag
            if (gg + 1 < g1) { if (nf) mask |= 1ull << (k + 1); else mask &= ~(1ull << (k + 1)); }
            if (gg == g1 - 1) last = true;
        }
        return last;
    };
    if (nwin <= PGA_FIX_MAXWIN) {
        for (int w = wave; w < nwin; w += nwaves) { const bool r = run_window(w, true); if (lane == 0) s_redone[w] = r; }
        __threadfence_block();
        __syncthreads();
        if (wave == 0)
            for (int w = 1; w < nwin; w++)
                if (s_redone[w - 1]) { const bool r = run_window(w, false); if (lane == 0) s_redone[w] = r; __builtin_amdgcn_wave_barrier(); }
    } else if (wave == 0) {
        for (int w = 0; w < nwin; w++) run_window(w, false);       // a contig of more than 262 k genes: plainly in order
    }
}

// ---- the public gene records ------------------------------------------------------------------------------------------------------------
// the final-pass fields of the two nodes of every gene, for the host tail's records
__global__ void __launch_bounds__(256)
k_gather_gene_nodes(const int64_t* __restrict__ idx, int n, OutArrays o, GeneNodeAttr* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int64_t g = idx[t];
    GeneNodeAttr a;
    a.cscore = o.cscore[g]; a.sscore = o.sscore[g]; a.rscore = o.rscore[g]; a.uscore = o.uscore[g]; a.tscore = o.tscore[g];
    a.mot_score = o.mot_score[g]; a.gc_cont = o.gc_cont[g]; a.mot_ndx = o.mot_ndx[g];
    a.edge = o.edge[g]; a.rbs[0] = o.rbs[2 * g]; a.rbs[1] = o.rbs[2 * g + 1]; a.mot_len = o.mot_len[g]; a.mot_spacer = o.mot_spacer[g];
    a._pad[0] = a._pad[1] = a._pad[2] = 0;
    out[t] = a;
}

// One thread per gene slot, the records packed in (contig, gene) order.  Where the fields of the gene's two nodes sit depends on
// what was gathered: everything (full), the winners without their final-pass fields (lean), or only what the tail writes
// (direct, lean as well: the DP pass's read-only fields and the topology stay where the scorers left them).
__global__ void __launch_bounds__(256)
k_emit_genes(const TailDesc* __restrict__ td, int n_contigs, int64_t n_slots, OutArrays o, const GeneRec* __restrict__ fin,
             const int32_t* __restrict__ n_genes, const int64_t* __restrict__ gene_begin, int single, pga_gene* __restrict__ out,
             const int lean, ChainArrays ca, GcPtrs gcs) {
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= n_slots) return;
    const int c = contig_of_slot(td, n_contigs, slot);
    const TailDesc d = td[c];
    const int g = (int)(slot - d.gene_off);
    if (g >= n_genes[c]) return;
    const GeneRec gr = fin[slot];
    const int64_t sn = d.out_off + gr.start_ndx, en = d.out_off + gr.stop_ndx;       // in the gathered arrays
    const int64_t fs = d.fin_off + gr.start_ndx, fe = d.fin_off + gr.stop_ndx;       // in the scorers' final pass
    const int64_t ts = d.topo_off + gr.start_ndx;                                    // in the group's topology
    GeneSrc s;
    if (o.direct) {
        const int64_t as = d.dp_off + gr.start_ndx, ae = d.dp_off + gr.stop_ndx;     // in the scorers' DP pass
        s.topology(o.g_strand[d.group], o.g_type[d.group], ts);
        if (single) s.scores(o.c_edge, o.c_cscore, o.sscore_dp, o.c_rscore, o.c_uscore, o.c_tscore, as, ae, sn);
        else s.scores(ca.edge, ca.cscore, ca.sscore, ca.rscore, ca.uscore, ca.tscore, fs, fe, fs);
        s.motifs(ca.rbs, ca.mot_len, ca.mot_spacer, ca.mot_ndx, ca.mot_score, fs, gcs.p[d.group], ts);
    } else if (lean) {
        s.topology(o.strand, o.type, sn);
        if (single) s.scores(o.edge_dp, o.cscore_dp, o.sscore_dp, o.rscore_dp, o.uscore_dp, o.tscore_dp, sn, en, sn);
        else s.scores(ca.edge, ca.cscore, ca.sscore, ca.rscore, ca.uscore, ca.tscore, fs, fe, fs);
        s.motifs(ca.rbs, ca.mot_len, ca.mot_spacer, ca.mot_ndx, ca.mot_score, fs, gcs.p[d.group], ts);
    } else {
        s.topology(o.strand, o.type, sn);
        if (single) s.scores(o.edge_dp, o.cscore_dp, o.sscore_dp, o.rscore_dp, o.uscore_dp, o.tscore_dp, sn, en, sn);
        else s.scores(o.edge, o.cscore, o.sscore, o.rscore, o.uscore, o.tscore, sn, en, sn);
        s.motifs(o.rbs, o.mot_len, o.mot_spacer, o.mot_ndx, o.mot_score, sn, o.gc_cont, sn);
    }
    out[gene_begin[c] + g] = gene_record(c, gr, s);
}
