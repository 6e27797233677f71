// Training on the device, many genomes per call (ref: lib.pyx:5236-5279 GeneFinder._train, TrainingInfo._calc_dicodon_gene
// 4284-4358, _train_starts_sd 4391-4599, _train_starts_nonsd 4601-4827; Prodigal node.c record_gc_bias /
// determine_sd_usage).  Included by finder.hip: the driver continues from the device arrays that the stage-level
// runs (extraction, scoring) leave behind.  Everything per base / per node runs in kernels; every accumulation is
// a count (an exact integer in a double, so the order of additions does not matter); libm's log stays on the host,
// where the reference calls it.
// Genome dimension: the nodes of every genome of the batch lie back to back in one set of arrays; node i belongs to genome
// gof[i], whose nodes are [n0, n1) and whose digits start at `base`.  Weights and counters are per genome.
namespace {

struct TrGenome { int64_t base; int32_t len, n0, n1, _pad; };

constexpr int TR_GC_HALF = 60;          // GC_WINDOW / 2 (ref: lib.pyx:171)

__device__ inline int tr_is_gc(const uint8_t* __restrict__ d, int i) { const int x = d[i]; return x != 0 && x != 3; }   // unknown bases count as GC
__device__ inline int tr_max_fr(int a, int b, int c) { return a > b ? (a > c ? 0 : 2) : (b > c ? 1 : 2); }
__device__ inline int tr_comp(int d) { return d <= 3 ? (d ^ 3) : 6; }
// 2-bit word of `len` bases starting at strand position i (ref: _sequence.h:207-220)
__device__ inline int tr_mer(const uint8_t* __restrict__ d, int L, int i, int len, int strand) {
    int v = 0;
    if (strand == 1) { for (int j = 0; j < len; j++) v |= (d[i + j] & 3) << (2 * j); }
    else { const int k = L - 1 - i; for (int j = 0; j < len; j++) v |= (tr_comp(d[k - j]) & 3) << (2 * j); }
    return v;
}

// ref: lib.pyx:724-768 (Sequence._max_gc_frame_plot).  The running sums of the reference reduce to
// tot[i] = sum of gc[i + 3 m] for |m| < 20 inside the sequence; the codon at i (i % 3 == 0) gets the frame with the most.
// grid.y: genome
__global__ void __launch_bounds__(256)
k_gc_frame(const uint8_t* __restrict__ dig, const TrGenome* __restrict__ gs, int8_t* __restrict__ gp_all) {
    const TrGenome G = gs[blockIdx.y];
    const uint8_t* __restrict__ d = dig + G.base;
    int8_t* __restrict__ gp = gp_all + G.base;
    const int L = G.len;
    const int c = blockIdx.x * blockDim.x + threadIdx.x;       // codon index
    const int i = 3 * c;
    if (i >= L) return;
    if (i >= L - 2) { for (int q = i; q < L; q++) gp[q] = -1; return; }
    int tot[3];
    for (int f = 0; f < 3; f++) {
        int s = 0;
        for (int m = -(TR_GC_HALF / 3 - 1); m <= TR_GC_HALF / 3 - 1; m++) {
            const int p = i + f + 3 * m;
            if (p >= 0 && p < L) s += tr_is_gc(d, p);
        }
        tot[f] = s;
    }
    const int w = tr_max_fr(tot[0], tot[1], tot[2]);
    gp[i] = gp[i + 1] = gp[i + 2] = (int8_t)w;
}

// Prodigal node.c record_gc_bias: per start node, how often each codon position is the GC-richest one between the
// start and its stop.
__global__ void __launch_bounds__(256)
k_gc_bias(int n, const int32_t* __restrict__ gof, const TrGenome* __restrict__ gs, const int32_t* __restrict__ ndx,
          const int32_t* __restrict__ stop_val, const uint8_t* __restrict__ type, const int8_t* __restrict__ strand,
          const int8_t* __restrict__ gp_all, double* __restrict__ gc_score, uint8_t* __restrict__ gc_bias) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int8_t* __restrict__ gp = gp_all + gs[gof[i]].base;
    gc_score[3 * i] = gc_score[3 * i + 1] = gc_score[3 * i + 2] = 0.0; gc_bias[i] = 0;
    if (type[i] == PGA_T_STOP) return;
    int ctr[3] = {0, 0, 0};
    const int fr = ndx[i] % 3;
    if (strand[i] == 1) {
        const int fm = 3 - fr;
        for (int j = stop_val[i]; j >= ndx[i]; j -= 3) ctr[(gp[j] + fm) % 3]++;
        for (int q = 0; q < 3; q++) { double g = 3.0 * ctr[q]; g /= 1.0 * (stop_val[i] - ndx[i] + 3); gc_score[3 * i + q] = g; }
    } else {
        const int fm = fr;
        for (int j = stop_val[i]; j <= ndx[i]; j += 3) ctr[((3 - gp[j]) + fm) % 3]++;
        for (int q = 0; q < 3; q++) { double g = 3.0 * ctr[q]; g /= 1.0 * (ndx[i] - stop_val[i] + 3); gc_score[3 * i + q] = g; }
    }
    gc_bias[i] = (uint8_t)tr_max_fr(ctr[0], ctr[1], ctr[2]);
}
// the one ordered floating-point sum of the training: node order within a genome, one thread per genome
__global__ void __launch_bounds__(64)
k_bias_sum(int n_genomes, const TrGenome* __restrict__ gs, const int32_t* __restrict__ ndx, const int32_t* __restrict__ stop_val,
           const uint8_t* __restrict__ type, const double* __restrict__ gc_score, const uint8_t* __restrict__ gc_bias,
           double* __restrict__ bias_all /* [genome][4] */) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_genomes) return;
    double* __restrict__ bias = bias_all + 4 * g;
    double b[3] = {0.0, 0.0, 0.0};
    for (int i = gs[g].n0; i < gs[g].n1; i++) {
        if (type[i] == PGA_T_STOP) continue;
        const int len = abs(stop_val[i] - ndx[i]) + 1;
        b[gc_bias[i]] += (gc_score[3 * i + gc_bias[i]] * len) / 1000.0;
    }
    const double tot = b[0] + b[1] + b[2];
    for (int q = 0; q < 3; q++) bias[q] = b[q] * (3.0 / tot);
}
__global__ void __launch_bounds__(256)
k_gcb(int n, const int32_t* __restrict__ gof, const double* __restrict__ gc_score, const double* __restrict__ bias_all, double* __restrict__ gcb) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* __restrict__ bias = bias_all + 4 * gof[i];
    gcb[i] = bias[0] * gc_score[3 * i] + bias[1] * gc_score[3 * i + 1] + bias[2] * gc_score[3 * i + 2];
}

// ref: lib.pyx:2279-2329 with flag == 0: the first start of each frame met while walking away from the stop
__global__ void __launch_bounds__(256)
k_ovl_starts0(int n_all, const int32_t* __restrict__ gof, const TrGenome* __restrict__ gs, const int32_t* __restrict__ ndx,
              const int32_t* __restrict__ stop_val, const uint8_t* __restrict__ type, const int8_t* __restrict__ strand,
              const uint8_t* __restrict__ edge, int maxov, int32_t* __restrict__ star_ptr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_all) return;
    // the genome's nodes [lo, n); star_ptr holds genome-local indices, as the connection scorer reads them
    const int lo = gs[gof[i]].n0, n = gs[gof[i]].n1;
    int sp[3] = {-1, -1, -1};
    if (type[i] == PGA_T_STOP && edge[i] != 1) {
        const int me = ndx[i];
        if (strand[i] == 1) {
            for (int j = i + 3; j >= lo; j--) {
                if (j >= n || ndx[j] > me + 2) continue;
                if (ndx[j] + maxov < me) break;
                if (strand[j] != 1 || type[j] == PGA_T_STOP) continue;
                if (stop_val[j] <= me) continue;
                const int f = ndx[j] % 3;
                if (sp[f] == -1) sp[f] = j - lo;
            }
        } else {
            for (int j = i - 3; j < n; j++) {
                if (j < lo || ndx[j] < me - 2) continue;
                if (ndx[j] - maxov > me) break;
                if (strand[j] != -1 || type[j] == PGA_T_STOP) continue;
                if (stop_val[j] >= me) continue;
                const int f = ndx[j] % 3;
                if (sp[f] == -1) sp[f] = j - lo;
            }
        }
    }
    star_ptr[3 * i] = sp[0]; star_ptr[3 * i + 1] = sp[1]; star_ptr[3 * i + 2] = sp[2];
}

// hexamer statistics (ref: lib.pyx:4284-4358): every window of both strands, then the codons of the genes of the path
__global__ void __launch_bounds__(256)
k_hexamer_bg(const uint8_t* __restrict__ dig, const TrGenome* __restrict__ gs, unsigned int* __restrict__ counts_all /* [genome][2][4096] */) {
    const TrGenome G = gs[blockIdx.y];
    const uint8_t* __restrict__ d = dig + G.base;
    const int L = G.len;
    unsigned int* __restrict__ counts = counts_all + (size_t)blockIdx.y * 8192;
    __shared__ unsigned int s_c[4096];
    for (int q = threadIdx.x; q < 4096; q += blockDim.x) s_c[q] = 0;
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < L - 5; i += gridDim.x * blockDim.x) {
        atomicAdd(&s_c[tr_mer(d, L, i, 6, 1)], 1u);
        atomicAdd(&s_c[tr_mer(d, L, i, 6, -1)], 1u);
    }
    __syncthreads();
    for (int q = threadIdx.x; q < 4096; q += blockDim.x) if (s_c[q]) atomicAdd(&counts[q], s_c[q]);
}
struct TrGene { int left, right, strand, genome; };     // strand-local [left, right - 5) step 3
__global__ void __launch_bounds__(256)
k_hexamer_genes(const uint8_t* __restrict__ dig, const TrGenome* __restrict__ gs, const TrGene* __restrict__ genes, int n_genes,
                unsigned int* __restrict__ counts_all) {
    const int g = blockIdx.x;
    if (g >= n_genes) return;
    const TrGene G = genes[g];
    const uint8_t* __restrict__ d = dig + gs[G.genome].base;
    const int L = gs[G.genome].len;
    unsigned int* __restrict__ counts = counts_all + (size_t)G.genome * 8192 + 4096;
    for (int i = G.left + 3 * threadIdx.x; i < G.right - 5; i += 3 * blockDim.x) atomicAdd(&counts[tr_mer(d, L, i, 6, G.strand)], 1u);
}


// ---- start training (ref: lib.pyx:4391-4599 _train_starts_sd, 4601-4827 _train_starts_nonsd) ----------------------
struct TrWeights {            // what changes from one iteration to the next
    double rbs_wt[28], type_wt[3], st_wt, sthresh, no_mot;
    int last_iter, stage, uses_sd, skip;     // skip: the genome takes no part in this round
};
struct TrCounts {             // everything counted in one iteration (integers)
    unsigned int rbg[28], rreal[28], treal[3], tbg[3], ngenes, zero_bg, zero_real, _pad;
    unsigned int ups[32][4];
};
__device__ inline int tr_pick_rbs(const double* __restrict__ w, int r0, int r1) {   // ref: lib.pyx:4441-4448
    const double w0 = w[r0], w1 = w[r1];
    if (w0 > w1 + 1.0 || r1 == 0) return r0;
    if (w0 < w1 - 1.0 || r0 == 0) return r1;
    return r0 > r1 ? r0 : r1;
}
// ref: lib.pyx:4360-4389 (TrainingInfo._count_upstream_composition)
__device__ inline void tr_count_upstream(const uint8_t* __restrict__ d, int L, int pos, int strand, TrCounts* __restrict__ cn) {
    int k = 0;
    for (int pass = 0; pass < 2; pass++) {
        const int lo = pass ? 15 : 1, hi = pass ? 45 : 3;
        for (int j = lo; j < hi; j++, k++) {
            if (strand == 1) { if (pos >= j) atomicAdd(&cn->ups[k][d[pos - j] & 3], 1u); }
            else { if (pos + j < L) atomicAdd(&cn->ups[k][tr_comp(d[pos + j]) & 3], 1u); }
        }
    }
}
// background of one iteration: start types (all starts) and the RBS bin each non-edge start would pick
__global__ void __launch_bounds__(256)
k_ts_background(int n, const int32_t* __restrict__ gof, const uint8_t* __restrict__ type, const uint8_t* __restrict__ edge,
                const uint8_t* __restrict__ rbs, const TrWeights* __restrict__ w_all, TrCounts* __restrict__ cn_all, int count_types) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || type[i] == PGA_T_STOP) return;
    const TrWeights* __restrict__ w = w_all + gof[i];
    TrCounts* __restrict__ cn = cn_all + gof[i];
    if (w->skip) return;
    if (count_types) atomicAdd(&cn->tbg[type[i]], 1u);
    if (edge[i]) return;
    atomicAdd(&cn->rbg[tr_pick_rbs(w->rbs_wt, rbs[2 * i], rbs[2 * i + 1])], 1u);
}
// One thread per stop node: the best non-edge start of its ORF under the current weights; a confident one is counted.
// The reference sweeps the nodes in strand order with ">=", i.e. among equal best starts the one met last wins:
// the highest index on the forward strand, the lowest on the reverse strand.
template <bool SD>
__global__ void __launch_bounds__(256)
k_ts_best(int n_all, const int32_t* __restrict__ gof, const TrGenome* __restrict__ gs, const int32_t* __restrict__ ndx,
          const int32_t* __restrict__ stop_val, const uint8_t* __restrict__ type, const int8_t* __restrict__ strand,
          const uint8_t* __restrict__ edge, const double* __restrict__ cscore, const uint8_t* __restrict__ rbs,
          const double* __restrict__ mot_score, const uint8_t* __restrict__ dig, const TrWeights* __restrict__ w_all,
          TrCounts* __restrict__ cn_all, int32_t* __restrict__ best_of_stop) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_all) return;
    if (best_of_stop) best_of_stop[s] = -1;
    if (type[s] != PGA_T_STOP) return;
    const int gi = gof[s];
    const TrWeights* __restrict__ w = w_all + gi;
    TrCounts* __restrict__ cn = cn_all + gi;
    if (w->skip) return;
    const int lo = gs[gi].n0, n = gs[gi].n1, L = gs[gi].len;
    const uint8_t* __restrict__ d = dig + gs[gi].base;
    const int st = strand[s], ph = ndx[s] % 3, sv = stop_val[s];
    const double wt = w->st_wt;
    double best = 0.0; int bndx = -1, brbs = 0;
    const int step = st == 1 ? -1 : 1;
    for (int j = s + step; j >= lo && j < n; j += step) {
        if (st == 1 ? ndx[j] <= sv : ndx[j] >= sv) break;            // past the other end of the ORF
        if (strand[j] != st || ndx[j] % 3 != ph) continue;
        if (type[j] == PGA_T_STOP) break;                             // the neighbouring stop of this frame (defensive: sv marks it)
        if (edge[j]) continue;
        int mr = 0; double v;
        if (SD) { mr = tr_pick_rbs(w->rbs_wt, rbs[2 * j], rbs[2 * j + 1]); v = cscore[j] + wt * w->rbs_wt[mr] + wt * w->type_wt[type[j]]; }
        else v = cscore[j] + wt * mot_score[j] + wt * w->type_wt[type[j]];
        if (bndx == -1 ? v >= 0.0 : v > best) { best = v; bndx = j; brbs = mr; }
    }
    if (bndx == -1 || !(best >= w->sthresh)) return;
    if (SD) atomicAdd(&cn->rreal[brbs], 1u);
    else { atomicAdd(&cn->ngenes, 1u); if (best_of_stop) best_of_stop[s] = bndx; }
    atomicAdd(&cn->treal[type[bndx]], 1u);
    if (w->last_iter) tr_count_upstream(d, L, ndx[bndx], st, cn);
}

// ---- motif statistics of the non-SD training -------------------------------------------------------------------------
struct TrMotifs { int32_t* ndx; uint8_t* len; uint8_t* spacer; uint8_t* spacendx; double* score; };   // per node
__device__ inline int tr_spacer_index(int j, int start, int i) {
    if (j <= start - 16 - i) return 3;
    if (j <= start - 14 - i) return 2;
    if (j >= start - 7 - i) return 1;
    return 0;
}
// ref: lib.pyx:1556-1616 (Node._find_best_upstream_motif) with the training stages
__global__ void __launch_bounds__(256)
k_mot_best(int n, const int32_t* __restrict__ gof, const TrGenome* __restrict__ gs, const int32_t* __restrict__ ndx,
           const uint8_t* __restrict__ type, const int8_t* __restrict__ strand, const uint8_t* __restrict__ edge,
           const uint8_t* __restrict__ dig, const double* __restrict__ mot_wt_all /* [genome][4][4][4096] */,
           const TrWeights* __restrict__ w_all, TrMotifs m) {
    const int i0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (i0 >= n || type[i0] == PGA_T_STOP || edge[i0]) return;
    const int gi = gof[i0];
    const TrWeights* __restrict__ w = w_all + gi;
    if (w->skip) return;
    const uint8_t* __restrict__ d = dig + gs[gi].base;
    const int L = gs[gi].len;
    const double* __restrict__ mot_wt = mot_wt_all + (size_t)gi * 4 * 4 * 4096;
    const int st = strand[i0], start = st == 1 ? ndx[i0] : L - 1 - ndx[i0];
    int bsp = 0, bsi = 0, blen = 0, bndx = 0; double bsc = -100.0;
    for (int i = 3; i >= 0; i--) {
        for (int j = start - 18 - i; j < start - 5 - i; j++) {
            if (j < 0) continue;
            const int si = tr_spacer_index(j, start, i);
            const int idx = tr_mer(d, L, j, i + 3, st);
            const double sc = mot_wt[(i * 4 + si) * 4096 + idx];
            if (sc > bsc) { bsc = sc; bsi = si; bsp = start - j - i - 3; bndx = idx; blen = i + 3; }
        }
    }
    if (w->stage == 2 && (bsc == -4.0 || bsc < w->no_mot + 0.69)) {
        m.ndx[i0] = 0; m.len[i0] = 0; m.spacendx[i0] = 0; m.spacer[i0] = 0; m.score[i0] = w->no_mot;
    } else {
        m.ndx[i0] = bndx; m.len[i0] = (uint8_t)blen; m.spacendx[i0] = (uint8_t)bsi; m.spacer[i0] = (uint8_t)(bsp & 15); m.score[i0] = bsc;
    }
}
// ref: lib.pyx:4225-4282 (TrainingInfo._update_motif_counts) for node i
__device__ inline void tr_update_motif_counts(int i0, const int32_t* __restrict__ ndx, const int8_t* __restrict__ strand,
                                              const uint8_t* __restrict__ d, int L, const TrMotifs& m, int stage,
                                              unsigned int* __restrict__ cnt /* [4][4][4096] */, unsigned int* __restrict__ zero) {
    if (m.len[i0] == 0) { atomicAdd(zero, 1u); return; }
    const int st = strand[i0], start = st == 1 ? ndx[i0] : L - 1 - ndx[i0];
    const int mlen = m.len[i0];
    if (stage == 0) {
        for (int i = 3; i >= 0; i--)
            for (int j = start - 18 - i; j < start - 5 - i; j++) {
                if (j < 0) continue;
                const int mer = tr_mer(d, L, j, i + 3, st);
                for (int k = 0; k < 4; k++) atomicAdd(&cnt[(i * 4 + k) * 4096 + mer], 1u);
            }
    } else if (stage == 1) {
        atomicAdd(&cnt[((mlen - 3) * 4 + m.spacendx[i0]) * 4096 + m.ndx[i0]], 1u);
        for (int i = 0; i < mlen - 3; i++)
            for (int j = start - m.spacer[i0] - mlen; j < start - m.spacer[i0] - i - 2; j++) {
                if (j < 0) continue;
                atomicAdd(&cnt[(i * 4 + tr_spacer_index(j, start, i)) * 4096 + tr_mer(d, L, j, i + 3, st)], 1u);
            }
    } else atomicAdd(&cnt[((mlen - 3) * 4 + m.spacendx[i0]) * 4096 + m.ndx[i0]], 1u);
}
// background: every non-edge start; real: the start chosen for each confident ORF (best_of_stop from k_ts_best<false>)
__global__ void __launch_bounds__(256)
k_mot_counts(int n, const int32_t* __restrict__ gof, const TrGenome* __restrict__ gs, const int32_t* __restrict__ ndx,
             const uint8_t* __restrict__ type, const int8_t* __restrict__ strand, const uint8_t* __restrict__ edge,
             const uint8_t* __restrict__ dig, TrMotifs m, const TrWeights* __restrict__ w_all, const int32_t* __restrict__ best_of_stop,
             unsigned int* __restrict__ cnt_all /* [genome][2][4][4][4096] */, unsigned int* __restrict__ zero_all /* [genome][2] */) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int node = i;
    if (best_of_stop) { node = best_of_stop[i]; if (node < 0) return; }
    if (type[node] == PGA_T_STOP || edge[node] == 1) return;
    const int gi = gof[node], real = best_of_stop != nullptr;
    const TrWeights* __restrict__ w = w_all + gi;
    if (w->skip) return;
    const size_t MT = (size_t)4 * 4 * 4096;
    tr_update_motif_counts(node, ndx, strand, dig + gs[gi].base, gs[gi].len, m, w->stage, cnt_all + (2 * (size_t)gi + real) * MT,
                           zero_all + 2 * gi + real);
}

// stages of the driver, for step-by-step validation against the oracle (PGA_TRAIN_* in the header)
enum { TR_BIAS = 1, TR_DICODON = 2, TR_SD = 3, TR_ALL = 4 };

// log-odds of the hexamer usage in genes against the whole sequence (ref: lib.pyx:4336-4358); libm on the host
void tr_gene_dc(const unsigned int* bgc, const unsigned int* gc, pga_training* t) {
    unsigned long long glob_bg = 0, glob = 0;
    for (int i = 0; i < 4096; i++) { glob_bg += bgc[i]; glob += gc[i]; }
    for (int i = 0; i < 4096; i++) {
        const double bg = (double)(int)bgc[i] / (double)(int)glob_bg;
        const double prob = (double)(int)gc[i] / (double)(int)glob;
        double v;
        if (prob == 0 && bg != 0) v = -5.0;
        else if (bg == 0) v = 0.0;
        else v = log(prob / bg);
        if (v > 5.0) v = 5.0; else if (v < -5.0) v = -5.0;
        t->gene_dc[i] = v;
    }
}


void tr_log_odds(const unsigned int* real, const double* bgv, double* out, int nq) {     // ref: lib.pyx:4528-4569
    double sum = 0.0;
    for (int j = 0; j < nq; j++) sum += (double)real[j];
    if (sum == 0.0) { for (int j = 0; j < nq; j++) out[j] = 0.0; return; }
    for (int j = 0; j < nq; j++) {
        const double r = (double)real[j] / sum;
        out[j] = bgv[j] != 0 ? log(r / bgv[j]) : -4.0;
        if (out[j] > 4.0) out[j] = 4.0; else if (out[j] < -4.0) out[j] = -4.0;
    }
}
void tr_ups_to_log(const unsigned int (*ups)[4], pga_training* t) {     // ref: lib.pyx:4571-4599 / 4797-4827
    for (int i = 0; i < 32; i++) {
        double sum = 0.0;
        for (int j = 0; j < 4; j++) { t->ups_comp[i][j] = (double)ups[i][j]; sum += t->ups_comp[i][j]; }
        if (sum == 0.0) { for (int j = 0; j < 4; j++) t->ups_comp[i][j] = 0.0; continue; }
        for (int j = 0; j < 4; j++) {
            double* u = &t->ups_comp[i][j];
            *u /= sum;
            const bool at = (j == 0 || j == 3);
            if (t->gc <= 0.1) *u = log(*u * 2.0 / (at ? 0.90 : 0.10));
            else if (t->gc >= 0.9) *u = log(*u * 2.0 / (at ? 0.10 : 0.90));
            else *u = at ? log(*u * 2.0 / (1.0 - t->gc)) : log(*u * 2.0 / t->gc);
            if (*u > 4.0) *u = 4.0;
            if (*u < -4.0) *u = -4.0;
        }
    }
}
void tr_determine_sd_usage(pga_training* t) {       // Prodigal node.c determine_sd_usage
    t->uses_sd = 1;
    if (t->rbs_wt[0] >= 0.0) t->uses_sd = 0;
    if (t->rbs_wt[16] < 1.0 && t->rbs_wt[13] < 1.0 && t->rbs_wt[15] < 1.0 &&
        (t->rbs_wt[0] >= -0.5 || (t->rbs_wt[22] < 2.0 && t->rbs_wt[24] < 2.0 && t->rbs_wt[27] < 2.0))) t->uses_sd = 0;
}


// Prodigal node.c build_coverage_map: which motifs are frequent enough (and their one-mismatch neighbours) to be modelled
void tr_build_coverage_map(const unsigned int* real /* [4][4][4096] */, int* good /* [4][4][4096] */, double ng) {
    const double thresh = 0.2;
#define RC(a, b, l) real[((a) * 4 + (b)) * 4096 + (l)]
#define GD(a, b, l) good[((a) * 4 + (b)) * 4096 + (l)]
    memset(good, 0, sizeof(int) * 4 * 4 * 4096);
    for (int i = 0; i < 4; i++) for (int j = 0; j < 64; j++)
        if ((double)RC(0, i, j) / ng >= thresh) for (int k = 0; k < 4; k++) GD(0, k, j) = 1;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 256; j++) {
        const int d0 = (j & 252) >> 2, d1 = j & 63;
        if (GD(0, i, d0) == 0 || GD(0, i, d1) == 0) continue;
        GD(1, i, j) = 1;
    }
    for (int i = 0; i < 4; i++) for (int j = 0; j < 1024; j++) {
        const int d0 = (j & 1008) >> 4, d1 = (j & 252) >> 2, d2 = j & 63;
        if (GD(0, i, d0) == 0 || GD(0, i, d1) == 0 || GD(0, i, d2) == 0) continue;
        GD(2, i, j) = 1;
        int tmp = j;
        for (int k = 0; k <= 16; k += 16) {
            tmp ^= k;
            for (int l = 0; l <= 32; l += 32) { tmp ^= l; if (GD(2, i, tmp) == 0) GD(2, i, tmp) = 2; }
        }
    }
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4096; j++) {
        const int d0 = (j & 4092) >> 2, d1 = j & 1023;
        if (GD(2, i, d0) == 0 || GD(2, i, d1) == 0) continue;
        GD(3, i, j) = (GD(2, i, d0) == 1 && GD(2, i, d1) == 1) ? 1 : 2;
    }
#undef RC
#undef GD
}

}  // namespace

// ref: lib.pyx:5236-5279 (GeneFinder._train) for every sequence of the batch at once: sequence g is genome g (the host layer
// joins the contigs of a genome with the reference's spacer), trained with tts[g], sws[g], fns[g].  One device pass per stage or
// round for all genomes; status[g] is PGA_OK or what a single-genome training would have returned.
static int train_body(const Knobs& kn, pga_ctx* c, const pga_batch* batch, const pga_params* pp, const int32_t* tts, const double* sws, const int32_t* fns,
                      int upto, pga_training* out, int32_t* status, bool& models_replaced) {
    if (!c || !batch || !pp || !out || !status || !tts || !sws || !fns || batch->ctx != c || batch->n < 1) {
        if (c) c->err = "pga_train_batch: bad arguments";
        return PGA_EINVAL;
    }
    const int G = batch->n;
    {
        std::vector<int32_t> seen;
        for (int g = 0; g < G; g++) if (std::find(seen.begin(), seen.end(), tts[g]) == seen.end()) seen.push_back(tts[g]);
        if (seen.size() > 4) { c->err = "pga_train_batch: more than 4 distinct translation tables in one call"; return PGA_EINVAL; }
    }
    for (int g = 0; g < G; g++) {
        pga_training* t = &out[g];
        memset(t, 0, sizeof *t);
        t->trans_table = tts[g]; t->st_wt = sws[g]; t->uses_sd = 1;
        status[g] = PGA_OK;
    }
    pga_params P = *pp; P.meta = 0; P.want_nodes = 1;
    hipStream_t st = c->stream;
    // ---- nodes (ref: lib.pyx:5252-5257): extraction + sort of every genome under its own table, through the stage-level path
    pga_result* r1 = nullptr;
    if (int rc = find_impl(kn, c, batch, &P, PGA_STAGE_EXTRACT, tts[0], &r1, nullptr, tts)) return rc;
    struct Free { pga_result* r; ~Free() { if (r) pga_result_free(r); } } fr1{r1};
    FinderState* f = c->finder;
    const uint8_t* d_dig = f->last.d_dig;            // the batch's digits, genome g at ct[g].base
    std::vector<TrGenome> gsv((size_t)G);
    int N = 0, maxL = 0;
    for (int g = 0; g < G; g++) {
        out[g].gc = r1->contigs[g].gc;
        const int n = r1->nodes[g].n;
        gsv[g] = TrGenome{batch->ct[g].base, batch->ct[g].len, N, N + n, 0};
        N += n; maxL = std::max(maxL, batch->ct[g].len);
        if (n == 0) { status[g] = PGA_EINVAL; c->err = "pga_train_batch: genome " + std::to_string(g) + " has no start / stop node"; }
    }
    if (N == 0) return PGA_OK;
    // the genomes' nodes back to back (host copies of the topology: the path walk reads them)
    std::vector<int32_t> h_ndx((size_t)N), h_sv((size_t)N), h_gof((size_t)N);
    std::vector<uint8_t> h_type((size_t)N), h_edge((size_t)N);
    std::vector<int8_t> h_strand((size_t)N);
    for (int g = 0; g < G; g++) {
        const pga_nodes& H = r1->nodes[g];
        const size_t o = (size_t)gsv[g].n0, n = (size_t)H.n;
        if (n == 0) continue;
        memcpy(&h_ndx[o], H.ndx, 4 * n); memcpy(&h_sv[o], H.stop_val, 4 * n);
        memcpy(&h_type[o], H.type, n); memcpy(&h_edge[o], H.edge, n); memcpy(&h_strand[o], H.strand, n);
        std::fill(h_gof.begin() + o, h_gof.begin() + o + n, g);
    }
    DEVBUF(d_gs, TrGenome, "tr_genomes", G);
    DEVBUF(d_ndx, int32_t, "tr_ndx", N) DEVBUF(d_sv, int32_t, "tr_stop_val", N) DEVBUF(d_gof, int32_t, "tr_genome_of", N)
    DEVBUF(d_type, uint8_t, "tr_type", N) DEVBUF(d_edge, uint8_t, "tr_edge", N) DEVBUF(d_strand, int8_t, "tr_strand", N)
    HT(c, hipMemcpyAsync(d_gs, gsv.data(), sizeof(TrGenome) * G, hipMemcpyHostToDevice, st));
    HT(c, hipMemcpyAsync(d_ndx, h_ndx.data(), 4 * (size_t)N, hipMemcpyHostToDevice, st));
    HT(c, hipMemcpyAsync(d_sv, h_sv.data(), 4 * (size_t)N, hipMemcpyHostToDevice, st));
    HT(c, hipMemcpyAsync(d_gof, h_gof.data(), 4 * (size_t)N, hipMemcpyHostToDevice, st));
    HT(c, hipMemcpyAsync(d_type, h_type.data(), (size_t)N, hipMemcpyHostToDevice, st));
    HT(c, hipMemcpyAsync(d_edge, h_edge.data(), (size_t)N, hipMemcpyHostToDevice, st));
    HT(c, hipMemcpyAsync(d_strand, h_strand.data(), (size_t)N, hipMemcpyHostToDevice, st));
    // host work of different genomes side by side: at most 16 threads, whatever the machine reports
    const int n_threads = std::max(1, std::min({16, G, (int)std::max(1u, std::thread::hardware_concurrency())}));
    auto per_genome = [&](const std::function<void(int)>& fn) {
        std::atomic<int> next(0);
        std::function<void()> job = [&]() { for (int g; (g = next.fetch_add(1)) < G;) fn(g); };
        if (n_threads == 1) job(); else f->pool.run(job, n_threads);
    };
    // ---- GC frame bias (ref: lib.pyx:5259-5261)
    DEVBUF(d_gp, int8_t, "tr_gp", batch->total + 4);
    DEVBUF(d_gcs, double, "tr_gc_score", 3 * (size_t)N + 3);
    DEVBUF(d_gcbias, uint8_t, "tr_gc_bias", N + 1);
    DEVBUF(d_bias, double, "tr_bias", 4 * (size_t)G);
    DEVBUF(d_gcb, double, "tr_gcb", N + 1);
    DEVBUF(d_star, int32_t, "tr_star", 3 * (size_t)N + 3);
    const int nb = (N + 255) / 256;
    hipLaunchKernelGGL(k_gc_frame, dim3((maxL / 3 + 256) / 256, G), dim3(256), 0, st, d_dig, d_gs, d_gp);
    hipLaunchKernelGGL(k_gc_bias, dim3(nb), dim3(256), 0, st, N, d_gof, d_gs, d_ndx, d_sv, d_type, d_strand, d_gp, d_gcs, d_gcbias);
    hipLaunchKernelGGL(k_bias_sum, dim3((G + 63) / 64), dim3(64), 0, st, G, d_gs, d_ndx, d_sv, d_type, d_gcs, d_gcbias, d_bias);
    std::vector<double> hb(4 * (size_t)G);
    HT(c, hipMemcpyAsync(hb.data(), d_bias, sizeof(double) * 4 * G, hipMemcpyDeviceToHost, st));
    HT(c, hipGetLastError());
    HT(c, hipStreamSynchronize(st));
    for (int g = 0; g < G; g++) memcpy(out[g].bias, &hb[4 * (size_t)g], sizeof out[g].bias);
    if (upto == TR_BIAS) return PGA_OK;
    // ---- training pass of the dynamic programme (ref: lib.pyx:5263-5267): one chain per genome, one launch
    hipLaunchKernelGGL(k_gcb, dim3(nb), dim3(256), 0, st, N, d_gof, d_gcs, d_bias, d_gcb);
    hipLaunchKernelGGL(k_ovl_starts0, dim3(nb), dim3(256), 0, st, N, d_gof, d_gs, d_ndx, d_sv, d_type, d_strand, d_edge, P.max_overlap, d_star);
    DpBuffers dp;
    {
        DEVBUF(b0, DpSrc, "dp_src", N + 1) DEVBUF(b1, DpTgt, "dp_tgt", N + 1) DEVBUF(b2, double, "dp_score", N + 1) DEVBUF(b3, int32_t, "dp_traceb", N + 1)
        DEVBUF(b4, int32_t, "dp_tbn", N + 1) DEVBUF(b5, int8_t, "dp_ov", N + 1) DEVBUF(b6, int32_t, "dp_maxidx", G + 1) DEVBUF(b7, double, "dp_maxscore", G + 1)
        DEVBUF(b8, int32_t, "dp_ipath", G + 1)
        dp = DpBuffers{b0, b1, b2, b3, b4, b5, b6, b7, b8, nullptr, {nullptr, nullptr, nullptr}, nullptr, nullptr, nullptr};
    }
    DEVBUF(d_chain, ChainDesc, "tr_chain", G);
    DEVBUF(d_mc, ModelConst, "tr_mc", G);
    std::vector<ChainDesc> chv;
    std::vector<ModelConst> mcv((size_t)G);
    for (int g = 0; g < G; g++) {
        ChainDesc ch{gsv[g].n0, gsv[g].n0, gsv[g].n1 - gsv[g].n0, g, g, 1};
        chv.push_back(ch);
        pga_fill_model_const(&mcv[g], sws[g]);
    }
    HT(c, hipMemcpyAsync(d_chain, chv.data(), sizeof(ChainDesc) * G, hipMemcpyHostToDevice, st));
    HT(c, hipMemcpyAsync(d_mc, mcv.data(), sizeof(ModelConst) * G, hipMemcpyHostToDevice, st));
    NodeArrays na{d_ndx, d_sv, d_type, d_strand, d_gcb, d_gcb, d_gcb, d_gcb, d_star, d_gcb};   // scores are not read when final = 0
    pga_launch_dp_prepare(d_chain, G, 0, N, na, d_mc, dp, st, 0);
    pga_launch_dp(kn, d_chain, G, d_mc, dp, 0, st);
    std::vector<int32_t> traceb((size_t)N), tracef((size_t)N, -1), star((size_t)3 * N), path((size_t)N + 1), mx((size_t)G, -1);
    std::vector<int8_t> ovm((size_t)N);
    std::vector<uint8_t> elim((size_t)N, 0);
    HT(c, hipMemcpyAsync(traceb.data(), dp.traceb, sizeof(int32_t) * N, hipMemcpyDeviceToHost, st));
    HT(c, hipMemcpyAsync(ovm.data(), dp.ov_mark, N, hipMemcpyDeviceToHost, st));
    HT(c, hipMemcpyAsync(star.data(), d_star, sizeof(int32_t) * 3 * N, hipMemcpyDeviceToHost, st));
    HT(c, hipMemcpyAsync(mx.data(), dp.max_index, 4 * (size_t)G, hipMemcpyDeviceToHost, st));
    HT(c, hipGetLastError());
    HT(c, hipStreamSynchronize(st));
    // ---- the genes of every genome's best path (ref: lib.pyx:1253-1311 untangling; 4299-4334 walk from the path's end)
    std::vector<std::vector<TrGene>> ggenes((size_t)G);
    per_genome([&](int g) {
        const int o = gsv[g].n0, n = gsv[g].n1 - o, L = gsv[g].len;
        if (n == 0 || mx[g] < 0) return;
        NodeView v{n, &h_ndx[o], &h_sv[o], &h_type[o], &h_strand[o], &h_edge[o], nullptr, nullptr, nullptr, nullptr, nullptr,
                   &star[3 * (size_t)o], &traceb[o], &tracef[o], &ovm[o], nullptr, &elim[o]};
        untangle(v, mx[g], &path[o]);
        const int* tb = &traceb[o];
        const int ipath = tb[mx[g]] == -1 ? -1 : mx[g];
        int in_gene = 0, left = -1, right = -1;
        for (int p = ipath; p != -1; p = tb[p]) {
            const int q = o + p;
            if (h_strand[q] == 1) {
                if (h_type[q] == PGA_T_STOP) { in_gene = 1; right = h_ndx[q] + 2; }
                else if (in_gene == 1) { left = h_ndx[q]; ggenes[g].push_back(TrGene{left, right, 1, g}); in_gene = 0; }
            } else {
                if (h_type[q] != PGA_T_STOP) { in_gene = -1; left = L - h_ndx[q] - 1; }
                else if (in_gene == -1) { right = L - h_ndx[q] + 1; ggenes[g].push_back(TrGene{left, right, -1, g}); in_gene = 0; }
            }
        }
    });
    std::vector<TrGene> genes;
    for (auto& v : ggenes) genes.insert(genes.end(), v.begin(), v.end());
    // ---- hexamer statistics (ref: lib.pyx:5269, 4284-4358), [genome][background, genes][4096]
    DEVBUF(d_cnt, unsigned int, "tr_hex", 8192 * (size_t)G);
    DEVBUF(d_genes, TrGene, "tr_genes", genes.size() + 1);
    HT(c, hipMemsetAsync(d_cnt, 0, sizeof(unsigned int) * 8192 * (size_t)G, st));
    if (!genes.empty()) HT(c, hipMemcpyAsync(d_genes, genes.data(), sizeof(TrGene) * genes.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_hexamer_bg, dim3(std::max(8, 1024 / G), G), dim3(256), 0, st, d_dig, d_gs, d_cnt);
    if (!genes.empty()) hipLaunchKernelGGL(k_hexamer_genes, dim3((unsigned)genes.size()), dim3(64), 0, st, d_dig, d_gs, d_genes, (int)genes.size(), d_cnt);
    std::vector<unsigned int> cnt(8192 * (size_t)G);
    HT(c, hipMemcpyAsync(cnt.data(), d_cnt, sizeof(unsigned int) * 8192 * (size_t)G, hipMemcpyDeviceToHost, st));
    HT(c, hipGetLastError());
    HT(c, hipStreamSynchronize(st));
    per_genome([&](int g) { tr_gene_dc(&cnt[8192 * (size_t)g], &cnt[8192 * (size_t)g + 4096], &out[g]); });
    if (upto == TR_DICODON) return PGA_OK;
    // ---- coding scores and RBS bins under the new statistics (ref: lib.pyx:5271-5273): the scoring stage of the path, every
    //      genome under its own half-trained model
    {
        std::vector<const pga_training*> tp((size_t)G);
        for (int g = 0; g < G; g++) tp[g] = &out[g];
        models_replaced = true;
        if (int rc = pga_set_models(c, tp.data(), G)) return rc;
    }
    std::vector<int32_t> moc((size_t)G);
    for (int g = 0; g < G; g++) moc[g] = g;
    pga_result* r2 = nullptr;
    if (int rc = find_impl(kn, c, batch, &P, PGA_STAGE_SCORE, tts[0], &r2, moc.data(), nullptr)) return rc;
    Free fr2{r2};
    f = c->finder;
    d_dig = f->last.d_dig;
    std::vector<double> h_cs((size_t)N);
    std::vector<uint8_t> h_rbs(2 * (size_t)N);
    for (int g = 0; g < G; g++) {
        const pga_nodes& H = r2->nodes[g];
        const size_t o = (size_t)gsv[g].n0, n = (size_t)(gsv[g].n1 - gsv[g].n0);
        if (H.n != (int)n) { c->err = "pga_train_batch: node count changed between the stages"; return PGA_EDEVICE; }
        if (n == 0) continue;
        memcpy(&h_cs[o], H.cscore, 8 * n); memcpy(&h_rbs[2 * o], H.rbs, 2 * n);
    }
    DEVBUF(d_cs, double, "tr_cscore", N) DEVBUF(d_rbs, uint8_t, "tr_rbs", 2 * (size_t)N)
    HT(c, hipMemcpyAsync(d_cs, h_cs.data(), 8 * (size_t)N, hipMemcpyHostToDevice, st));
    HT(c, hipMemcpyAsync(d_rbs, h_rbs.data(), 2 * (size_t)N, hipMemcpyHostToDevice, st));
    DEVBUF(d_w, TrWeights, "tr_weights", G);
    DEVBUF(d_cn, TrCounts, "tr_counts", G);
    std::vector<TrWeights> w((size_t)G);
    std::vector<TrCounts> cn((size_t)G);
    std::vector<double> tbg(3 * (size_t)G, 0.0);
    for (int g = 0; g < G; g++) {
        memset(&w[g], 0, sizeof w[g]);
        w[g].st_wt = out[g].st_wt; w[g].sthresh = 35.0; w[g].uses_sd = 1; w[g].skip = status[g] != PGA_OK;
        memset(out[g].type_wt, 0, sizeof out[g].type_wt); memset(out[g].rbs_wt, 0, sizeof out[g].rbs_wt); memset(out[g].ups_comp, 0, sizeof out[g].ups_comp);
    }
    // ---- Shine-Dalgarno start training: 10 rounds (ref: lib.pyx:4391-4599)
    for (int it = 0; it < 10; it++) {
        for (int g = 0; g < G; g++) {
            memcpy(w[g].rbs_wt, out[g].rbs_wt, sizeof w[g].rbs_wt); memcpy(w[g].type_wt, out[g].type_wt, sizeof w[g].type_wt);
            w[g].last_iter = it == 9;
        }
        HT(c, hipMemcpyAsync(d_w, w.data(), sizeof(TrWeights) * G, hipMemcpyHostToDevice, st));
        HT(c, hipMemsetAsync(d_cn, 0, sizeof(TrCounts) * G, st));
        hipLaunchKernelGGL(k_ts_background, dim3(nb), dim3(256), 0, st, N, d_gof, d_type, d_edge, d_rbs, d_w, d_cn, 1);
        hipLaunchKernelGGL(k_ts_best<true>, dim3(nb), dim3(256), 0, st, N, d_gof, d_gs, d_ndx, d_sv, d_type, d_strand, d_edge, d_cs,
                           d_rbs, (const double*)nullptr, d_dig, d_w, d_cn, (int32_t*)nullptr);
        HT(c, hipMemcpyAsync(cn.data(), d_cn, sizeof(TrCounts) * G, hipMemcpyDeviceToHost, st));
        HT(c, hipGetLastError());
        HT(c, hipStreamSynchronize(st));
        for (int g = 0; g < G; g++) {
            if (w[g].skip) continue;
            pga_training* t = &out[g];
            const int n = gsv[g].n1 - gsv[g].n0;
            double* tb = &tbg[3 * (size_t)g];
            if (it == 0) {
                double sum = 0.0;
                for (int j = 0; j < 3; j++) { tb[j] = (double)cn[g].tbg[j]; sum += tb[j]; }
                for (int j = 0; j < 3; j++) tb[j] /= sum;
            }
            double rbg[28], sum = 0.0;
            for (int j = 0; j < 28; j++) { rbg[j] = (double)cn[g].rbg[j]; sum += rbg[j]; }
            for (int j = 0; j < 28; j++) rbg[j] /= sum;
            tr_log_odds(cn[g].rreal, rbg, t->rbs_wt, 28);
            sum = 0.0; for (int j = 0; j < 3; j++) sum += (double)cn[g].treal[j];
            tr_log_odds(cn[g].treal, tb, t->type_wt, 3);
            if (sum * 2000.0 <= n) w[g].sthresh /= 2.0;
        }
    }
    std::vector<int> motif;                      // genomes that go on to the motif-based start training
    for (int g = 0; g < G; g++) {
        if (w[g].skip) continue;
        pga_training* t = &out[g];
        tr_ups_to_log(cn[g].ups, t);
        if (fns[g]) t->uses_sd = 0; else tr_determine_sd_usage(t);
        if (!t->uses_sd) motif.push_back(g);
    }
    if (upto == TR_SD || motif.empty()) return PGA_OK;
    // ---- motif-based start training: 20 rounds in three stages (ref: lib.pyx:4601-4827); the SD genomes sit these out
    const size_t MT = (size_t)4 * 4 * 4096;
    DEVBUF(d_motwt, double, "tr_mot_wt", MT * G);
    DEVBUF(d_mcnt, unsigned int, "tr_mot_counts", 2 * MT * G);
    DEVBUF(d_zero, unsigned int, "tr_mot_zero", 2 * (size_t)G);
    DEVBUF(d_best, int32_t, "tr_best_of_stop", N + 1);
    TrMotifs mot;
    {
        DEVBUF(m0, int32_t, "tr_mot_ndx", N + 1) DEVBUF(m1, uint8_t, "tr_mot_len", N + 1) DEVBUF(m2, uint8_t, "tr_mot_spacer", N + 1)
        DEVBUF(m3, uint8_t, "tr_mot_spacendx", N + 1) DEVBUF(m4, double, "tr_mot_score", N + 1)
        mot = TrMotifs{m0, m1, m2, m3, m4};
        HT(c, hipMemsetAsync(m1, 0, (size_t)N + 1, st));
    }
    std::vector<unsigned int> hc(2 * MT * G), zeros(2 * (size_t)G);
    for (int g = 0; g < G; g++) w[g].skip = 1;
    for (int g : motif) {
        memset(out[g].ups_comp, 0, sizeof out[g].ups_comp);
        memset(out[g].type_wt, 0, sizeof out[g].type_wt);
        w[g].sthresh = 35.0; w[g].uses_sd = 0; w[g].skip = 0;
    }
    struct MotifScratch { std::vector<double> mbg, mreal; std::vector<int> mgood; };
    std::vector<MotifScratch> scratch((size_t)G);
    for (int g : motif) { scratch[g].mbg.resize(MT); scratch[g].mreal.resize(MT); scratch[g].mgood.assign(MT, 0); }
    const int NMOT = (int)motif.size();
    for (int it = 0; it < 20; it++) {
        const int stage = it < 4 ? 0 : (it < 12 ? 1 : 2);
        for (int g : motif) {
            memcpy(w[g].type_wt, out[g].type_wt, sizeof w[g].type_wt);
            w[g].no_mot = out[g].no_mot; w[g].stage = stage; w[g].last_iter = it == 19;
            HT(c, hipMemcpyAsync(d_motwt + MT * g, &out[g].mot_wt[0][0][0], sizeof(double) * MT, hipMemcpyHostToDevice, st));
        }
        HT(c, hipMemcpyAsync(d_w, w.data(), sizeof(TrWeights) * G, hipMemcpyHostToDevice, st));
        HT(c, hipMemsetAsync(d_cn, 0, sizeof(TrCounts) * G, st));
        HT(c, hipMemsetAsync(d_mcnt, 0, sizeof(unsigned int) * 2 * MT * G, st));
        HT(c, hipMemsetAsync(d_zero, 0, sizeof(unsigned int) * 2 * G, st));
        hipLaunchKernelGGL(k_mot_best, dim3(nb), dim3(256), 0, st, N, d_gof, d_gs, d_ndx, d_type, d_strand, d_edge, d_dig, d_motwt, d_w, mot);
        hipLaunchKernelGGL(k_mot_counts, dim3(nb), dim3(256), 0, st, N, d_gof, d_gs, d_ndx, d_type, d_strand, d_edge, d_dig, mot, d_w,
                           (const int32_t*)nullptr, d_mcnt, d_zero);
        hipLaunchKernelGGL(k_ts_best<false>, dim3(nb), dim3(256), 0, st, N, d_gof, d_gs, d_ndx, d_sv, d_type, d_strand, d_edge, d_cs,
                           d_rbs, mot.score, d_dig, d_w, d_cn, d_best);
        hipLaunchKernelGGL(k_mot_counts, dim3(nb), dim3(256), 0, st, N, d_gof, d_gs, d_ndx, d_type, d_strand, d_edge, d_dig, mot, d_w,
                           d_best, d_mcnt, d_zero);
        for (int g : motif) HT(c, hipMemcpyAsync(&hc[2 * MT * g], d_mcnt + 2 * MT * g, sizeof(unsigned int) * 2 * MT, hipMemcpyDeviceToHost, st));
        HT(c, hipMemcpyAsync(zeros.data(), d_zero, sizeof(unsigned int) * 2 * G, hipMemcpyDeviceToHost, st));
        HT(c, hipMemcpyAsync(cn.data(), d_cn, sizeof(TrCounts) * G, hipMemcpyDeviceToHost, st));
        HT(c, hipGetLastError());
        HT(c, hipStreamSynchronize(st));
        // ---- the weights of the next round, genome by genome on the pool (host: sums of counts, libm log)
        std::atomic<int> next(0);
        std::function<void()> job = [&]() {
            for (int k; (k = next.fetch_add(1)) < NMOT;) {
                const int g = motif[k];
                pga_training* t = &out[g];
                const unsigned int* h = &hc[2 * MT * g];
                std::vector<double>& mbg = scratch[g].mbg; std::vector<double>& mreal = scratch[g].mreal; std::vector<int>& mgood = scratch[g].mgood;
                const int n = gsv[g].n1 - gsv[g].n0;
                double zbg = (double)zeros[2 * g], zreal = (double)zeros[2 * g + 1], sum = 0.0;
                const double ngenes = (double)cn[g].ngenes;
                for (size_t q = 0; q < MT; q++) { mbg[q] = (double)h[q]; sum += mbg[q]; }
                sum += zbg;
                for (size_t q = 0; q < MT; q++) mbg[q] /= sum;
                zbg /= sum;
                if (stage < 2) tr_build_coverage_map(h + MT, mgood.data(), ngenes);
                sum = 0.0;
                for (size_t q = 0; q < MT; q++) { mreal[q] = (double)h[MT + q]; sum += mreal[q]; }
                sum += zreal;
                if (sum == 0.0) {
                    memset(t->mot_wt, 0, sizeof t->mot_wt); t->no_mot = 0.0;
                } else {
                    double* wt = &t->mot_wt[0][0][0];
                    for (size_t q = 0; q < MT; q++) {
                        if (mgood[q] == 0) { zreal += mreal[q]; zbg += mreal[q]; mreal[q] = 0.0; mbg[q] = 0.0; }
                        mreal[q] /= sum;
                        double v = mbg[q] != 0 ? log(mreal[q] / mbg[q]) : -4.0;
                        if (v > 4.0) v = 4.0; else if (v < -4.0) v = -4.0;
                        wt[q] = v;
                    }
                }
                zreal /= sum;
                t->no_mot = zbg != 0 ? log(zreal / zbg) : -4.0;
                if (t->no_mot > 4.0) t->no_mot = 4.0; else if (t->no_mot < -4.0) t->no_mot = -4.0;
                sum = 0.0; for (int j = 0; j < 3; j++) sum += (double)cn[g].treal[j];
                tr_log_odds(cn[g].treal, &tbg[3 * (size_t)g], t->type_wt, 3);
                if (sum * 2000.0 <= n) w[g].sthresh /= 2.0;
            }
        };
        const int k = std::min(n_threads, NMOT);
        if (k <= 1) job(); else f->pool.run(job, k);
    }
    for (int g : motif) tr_ups_to_log(cn[g].ups, &out[g]);
    return PGA_OK;
}

// The scoring stage of the training runs through the context's model slots (the half-trained models are loaded as models
// 0 .. G - 1); the caller's model set is put back afterwards, so that pga_set_models(bins) ... pga_train ... pga_find_genes keeps
// scoring with the bins.
static int train_impl(pga_ctx* c, const pga_batch* batch, const pga_params* pp, const int32_t* tts, const double* sws, const int32_t* fns,
                      int upto, pga_training* out, int32_t* status) {
    if (!c) return PGA_EINVAL;
    const Knobs kn = read_knobs();      // once for the whole training call, its two finder passes included
    c->dev_nodes.clear();               // training runs the finder: it reuses the node arena of the last find
    const std::vector<pga_training> saved = c->models;
    bool replaced = false;
    const int rc = train_body(kn, c, batch, pp, tts, sws, fns, upto, out, status, replaced);
    if (replaced) {
        const std::string err = c->err;
        std::vector<const pga_training*> ptrs;
        for (const pga_training& m : saved) ptrs.push_back(&m);
        const int rc2 = pga_set_models(c, ptrs.data(), (int)ptrs.size());
        // a failed restore must not pass unseen: the context would keep scoring with the half-trained model
        if (rc != PGA_OK) { c->err = rc2 != PGA_OK ? err + "; and the context's models could not be restored: " + c->err : err; return rc; }
        if (rc2 != PGA_OK) return rc2;
        c->err = err;
    }
    return rc;
}
