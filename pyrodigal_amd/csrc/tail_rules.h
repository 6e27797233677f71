// The rules of the traceback tail, one text each, for the host, the one-thread-per-contig and the parallel forms
// (finder.hip's host tail, tail.inl's kernels): what an edge of the path splices in, what a path position does in
// eliminate_bad_genes, who sets what in the gene list, how one start candidate is priced and merged, and what a gene
// record says.  No kernels and no wave intrinsics: who enumerates, where the path lives and how a scan is carried is
// the business of the forms.
//
// ref: lib.pyx:1253-1311 (_disentangle_overlaps, _max_forward_pointers), Prodigal dprog.c eliminate_bad_genes (call sites
// lib.pyx:5308, 5369), lib.pyx:3231-3270 (Genes._extract), 3272-3401 (Genes._tweak_final_starts), 2644-2830 (Gene).
#pragma once
#include "pga_internal.h"

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

// nodes of one contig for its winning model
struct NodeView {
    int n;
    const int32_t* ndx; const int32_t* stop_val; const uint8_t* type; const int8_t* strand; const uint8_t* edge;
    double* cscore; double* sscore; const double* rscore; const double* uscore; const double* tscore;
    const int32_t* star_ptr; int32_t* traceb; int32_t* tracef; int8_t* ov_mark; const double* score; uint8_t* elim;
};
struct GeneRec { int begin, end, start_ndx, stop_ndx; };

__host__ __device__ inline bool is_stop_n(const NodeView& v, int i) { return v.type[i] == PGA_T_STOP; }

// ref: _connection.h:52-78
__host__ __device__ inline double igm_same_h(const NodeView& v, int a, int b, double st_wt) {
    const int dist = abs(v.ndx[a] - v.ndx[b]);
    const bool ovl = v.ndx[a] + 2 * v.strand[a] >= v.ndx[b];
    double r = 0.0;
    if (v.ndx[a] + 2 == v.ndx[b] || v.ndx[a] == v.ndx[b] + 1) {
        if (v.strand[a] == 1) { if (v.rscore[b] < 0) r -= v.rscore[b]; if (v.uscore[b] < 0) r -= v.uscore[b]; }
        else                  { if (v.rscore[a] < 0) r -= v.rscore[a]; if (v.uscore[a] < 0) r -= v.uscore[a]; }
    }
    if (dist > 3 * PGA_OPER_DIST) r -= 0.15 * st_wt;
    else if ((dist <= PGA_OPER_DIST && !ovl) || dist * 4 < PGA_OPER_DIST) r += (2.0 - (double)dist / PGA_OPER_DIST) * 0.15 * st_wt;
    return r;
}
__host__ __device__ inline double igm_h(const NodeView& v, int a, int b, double st_wt) {   // ref: _connection.h:81-91
    return v.strand[a] == v.strand[b] ? igm_same_h(v, a, b, st_wt) : -0.15 * st_wt;
}

// The reference walks down from node `from` until it meets a node at position `pos` (the other end of the ORF, which
// always exists): positions are sorted, so the first hit of that walk is the LAST node at or below `from` with
// ndx == pos, which a binary search finds in O(log n) loads instead of one dependent load per node of the gene.
__host__ __device__ inline int walk_down_to(const NodeView& v, int from, int pos) {
    int a = 0, b = from + 1;                      // first index in [0, from] with ndx > pos
    while (a < b) { const int m = (a + b) >> 1; if (v.ndx[m] <= pos) a = m + 1; else b = m; }
    return a - 1;
}

// the last of n ascending keys (key(0) <= x) that is <= x: which contig, chain or gene run owns slot x
template <class Key>
__host__ __device__ inline int owner_of(Key key, int n, int64_t x) {
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (key(mid) <= x) lo = mid; else hi = mid - 1; }
    return lo;
}

// ---- splices: what the edge (p, nx = traceb[p]) of the path takes in (ref: lib.pyx:1253-1295) -------------------------------
// Every test reads its operands first, unconditionally: the loads of one edge then leave together instead of one round
// trip per `&&`.

// the triple-overlap rule: a reverse stop followed by a forward stop further down, with an overlapping gene on record.  The
// first node to splice in (the record's star_ptr target; its ORF's other end follows it), or -1.
__host__ __device__ inline int splice_triple(const NodeView& v, int p, int nx) {
    const int sp = v.strand[p], sn = v.strand[nx], ov = v.ov_mark[p], np = v.ndx[p], nn = v.ndx[nx];
    const bool stp = is_stop_n(v, p), stn = is_stop_n(v, nx);
    return ((sp == -1) & stp & (sn == 1) & stn & (ov != -1) & (np > nn)) ? v.star_ptr[3 * p + ov] : -1;
}
// the missing-node rule (reverse start -> forward stop, forward stop -> forward stop, reverse stop -> reverse stop): the
// node to insert, or -1
__host__ __device__ inline int splice_missing(const NodeView& v, int p, int nx) {
    const int sp = v.strand[p], sn = v.strand[nx], np = v.ndx[p], nn = v.ndx[nx];
    const bool stp = is_stop_n(v, p), stn = is_stop_n(v, nx);
    const bool p_rb = sp == -1 && !stp, p_fs = sp == 1 && stp, p_rs = sp == -1 && stp;
    const bool n_fs = sn == 1 && stn, n_rs = sn == -1 && stn;
    int ins = -1;
    if (p_rb && n_fs) ins = walk_down_to(v, p, v.stop_val[p]);
    if (p_fs && n_fs) ins = v.star_ptr[3 * nx + np % 3];
    if (p_rs && n_rs) ins = v.star_ptr[3 * p + nn % 3];
    return ins;
}
// both passes on an edge of the ORIGINAL path: the positions node p takes (itself and what follows it) and who follows.  The
// nodes spliced in never meet a rule themselves (tail.inl's head comment), so an edge is decided on its own.
struct Splice { int slots, i0, i1; };
__host__ __device__ inline Splice splice_of(const NodeView& v, int p, int nx) {
    if (nx == -1) return Splice{1, -1, -1};
    const int t = splice_triple(v, p, nx);
    if (t != -1) return Splice{3, t, walk_down_to(v, t, v.stop_val[t])};
    const int ins = splice_missing(v, p, nx);
    return Splice{ins != -1 ? 2 : 1, ins, -1};
}

// The reference's own shape (_disentangle_overlaps, _max_forward_pointers): two passes along traceb that splice in place, in
// the reference's order of events -- the walk of either pass continues through the nodes it has just spliced in.  The writing
// behind the one-thread-per-contig and host forms; returns the length of the path it lists.
__host__ __device__ inline int untangle(NodeView& v, int mx, int32_t* __restrict__ path) {
    for (int p = mx, nx = v.traceb[p]; nx != -1; p = nx, nx = v.traceb[p]) {
        const int tmp = splice_triple(v, p, nx);
        if (tmp != -1) {
            const int k = walk_down_to(v, tmp, v.stop_val[tmp]);
            v.traceb[p] = tmp; v.traceb[tmp] = k; v.ov_mark[k] = -1; v.traceb[k] = nx;
            nx = tmp;
        }
    }
    for (int p = mx, nx = v.traceb[p]; nx != -1; p = nx, nx = v.traceb[p]) {
        const int ins = splice_missing(v, p, nx);
        if (ins != -1) { v.traceb[p] = ins; v.traceb[ins] = nx; nx = ins; }
    }
    // forward pointers; the nodes of the path are also listed (from mx back to its head) so that the later passes
    // read them with independent loads instead of chasing pointers again
    int cnt = 0;
    int p = mx;
    for (; v.traceb[p] != -1; p = v.traceb[p]) { path[cnt++] = p; v.tracef[v.traceb[p]] = p; }
    path[cnt++] = p;
    return cnt;
}

// ---- eliminate_bad_genes, per path position (path[cnt - 1] is the head of the path, path[0] its last node) ----------------
// first loop: the terms the start score of node path[q] receives, in the reference's order -- as the node after a forward
// stop, then as a reverse start.  Nodes are independent of each other (igm_h reads no start score).
__host__ __device__ inline void elim_add_terms(const NodeView& v, const int32_t* path, int cnt, int q, double st_wt) {
    const int x = path[q];
    if (q + 1 <= cnt - 1) {
        const int p = path[q + 1];
        if (v.strand[p] == 1 && is_stop_n(v, p)) v.sscore[x] += igm_h(v, p, x, st_wt);
    }
    if (q >= 1 && v.strand[x] == -1 && !is_stop_n(v, x)) v.sscore[x] += igm_h(v, x, path[q - 1], st_wt);
}
// second loop, q >= 1: the gene made of path[q] and path[q - 1] goes when its start node scores below zero
__host__ __device__ inline void elim_mark_pair(const NodeView& v, const int32_t* path, int q) {
    const int p = path[q], f = path[q - 1];
    const int sp = v.strand[p]; const bool stp = is_stop_n(v, p);
    const double gp = v.cscore[p] + v.sscore[p], gf = v.cscore[f] + v.sscore[f];
    if ((sp == 1 && !stp && gp < 0) || (sp == -1 && stp && gf < 0)) { v.elim[p] = 1; v.elim[f] = 1; }
}

__host__ __device__ inline void eliminate_bad_genes(const NodeView& v, const int32_t* __restrict__ path, int cnt, double st_wt) {
    for (int q = cnt - 1; q >= 0; q--) elim_add_terms(v, path, cnt, q, st_wt);
    for (int q = cnt - 1; q >= 1; q--) elim_mark_pair(v, path, q);
}

// ---- gene list (Genes._extract): the reference's serial walk (returns the number of genes written to `out`) -----------------
__host__ __device__ inline int extract_genes(const NodeView& v, const int32_t* __restrict__ path, int cnt, GeneRec* out) {
    int b = 0, e = 0, s = 0, t = 0, ng = 0;
    for (int q = cnt - 1; q >= 0; q--) {
        const int p = path[q];
        const int el = v.elim[p], sp = v.strand[p], np = v.ndx[p]; const bool stp = is_stop_n(v, p);
        if (el == 1) continue;
        if (sp == 1) {
            if (!stp) { b = np + 1; s = p; }
            else { e = np + 3; t = p; out[ng++] = GeneRec{b, e, s, t}; }
        } else {
            if (!stp) { e = np + 1; s = p; out[ng++] = GeneRec{b, e, s, t}; }
            else { b = np - 1; t = p; }
        }
    }
    return ng;
}

// ---- ... and for the parallel forms: position r of the processing order is path position cnt - 1 - r ---
// who sets what (the four branches of Genes._extract): begin, end, start node, stop node.  Whoever sets the end emits a gene.
struct ExtractItem {
    bool set_b, set_e, set_s, set_t;
    __host__ __device__ bool emit() const { return set_e; }
};
__host__ __device__ inline ExtractItem tp_extract_item(const NodeView& v, const int32_t* pl, const uint8_t* el, const int cnt, const int r) {
    bool live = false, fwd = false, stp = false;
    if (r < cnt) { const int p = pl[cnt - 1 - r]; live = el[p] != 1; fwd = v.strand[p] == 1; stp = is_stop_n(v, p); }
    return ExtractItem{live && ((fwd && !stp) || (!fwd && stp)),       // forward start: begin; reverse stop: begin
                       live && ((fwd && stp) || (!fwd && !stp)),       // forward stop: end;   reverse start: end
                       live && !stp, live && stp};
}
// the record from the last positions that set begin, end, start node and stop node (-1: none yet)
__host__ __device__ inline GeneRec tp_gene_at(const NodeView& v, const int32_t* pl, const int cnt, const int* m) {
    GeneRec gr{0, 0, 0, 0};
    if (m[0] >= 0) { const int p = pl[cnt - 1 - m[0]]; gr.begin = v.strand[p] == 1 ? v.ndx[p] + 1 : v.ndx[p] - 1; }
    if (m[1] >= 0) { const int p = pl[cnt - 1 - m[1]]; gr.end = v.strand[p] == 1 ? v.ndx[p] + 3 : v.ndx[p] + 1; }
    if (m[2] >= 0) gr.start_ndx = pl[cnt - 1 - m[2]];
    if (m[3] >= 0) gr.stop_ndx = pl[cnt - 1 - m[3]];
    return gr;
}

// ---- start tweak of one gene (Genes._tweak_final_starts); `prev` / `next` are its neighbours as the reference's in-order
// loop would see them (prev already tweaked, next not yet) -------------------------------------------------------------------
struct TweakCtx {           // (a) what every candidate of the gene is judged against
    const GeneRec* prev; const GeneRec* next;
    int ndx, sv_ndx, maxov;
    double w, sc, ig;
    bool prev_fwd, prev_rev, next_fwd, next_rev;
};
__host__ __device__ inline TweakCtx tweak_context(const NodeView& v, const GeneRec* prev, const GeneRec& cur, const GeneRec* next, double w, int maxov) {
    TweakCtx c;
    c.prev = prev; c.next = next; c.ndx = cur.start_ndx; c.maxov = maxov; c.w = w;
    const int ndx = c.ndx;
    c.sc = v.sscore[ndx] + v.cscore[ndx];
    c.ig = 0.0;
    c.prev_fwd = prev && v.strand[prev->start_ndx] == 1; c.prev_rev = prev && v.strand[prev->start_ndx] == -1;
    c.next_fwd = next && v.strand[next->start_ndx] == 1; c.next_rev = next && v.strand[next->start_ndx] == -1;
    if (v.strand[ndx] == 1 && c.prev_fwd) c.ig = igm_same_h(v, prev->stop_ndx, ndx, w);
    if (v.strand[ndx] == 1 && c.prev_rev) c.ig = -0.15 * w;
    if (v.strand[ndx] == -1 && c.next_fwd) c.ig = -0.15 * w;
    if (v.strand[ndx] == -1 && c.next_rev) c.ig = igm_same_h(v, ndx, next->stop_ndx, w);
    c.sv_ndx = v.stop_val[ndx];
    return c;
}
// (b) node j (a valid index) is a start node of the gene's own ORF
__host__ __device__ inline bool tweak_same_orf_start(const NodeView& v, const TweakCtx& c, int j) {
    return !(is_stop_n(v, j) | (v.stop_val[j] != c.sv_ndx));
}
// (c) the intergenic term of candidate j against the gene's neighbours; false: the candidate is cut (it overlaps a
// neighbour on its own strand by more than max_overlap, or reaches the start of one on the other strand)
__host__ __device__ inline bool tweak_price(const NodeView& v, const TweakCtx& c, int j, double& tg) {
    const int sj = v.strand[j];
    tg = 0.0;
    if (sj == 1 && c.prev_fwd) {
        if (v.ndx[c.prev->stop_ndx] - v.ndx[j] > c.maxov) return false;
        tg = igm_same_h(v, c.prev->stop_ndx, j, c.w);
    }
    if (sj == 1 && c.prev_rev) { if (v.ndx[c.prev->start_ndx] - v.ndx[j] >= 0) return false; tg = -0.15 * c.w; }
    if (sj == -1 && c.next_fwd) { if (v.ndx[j] - v.ndx[c.next->start_ndx] >= 0) return false; tg = -0.15 * c.w; }
    if (sj == -1 && c.next_rev) {
        if (v.ndx[j] - v.ndx[c.next->stop_ndx] > c.maxov) return false;
        tg = igm_same_h(v, j, c.next->stop_ndx, c.w);
    }
    return true;
}
// (d) the two best candidates so far, met in index order (the bookkeeping depends on that order).  Scalars, not arrays: an
// array indexed by the pick would leave the registers.
struct TweakCand { int j = -1; double cs = 0.0, tg = 0.0; };        // node, its own score, its intergenic term
struct TwoBest { TweakCand first, second; };
__host__ __device__ inline void tweak_take(TwoBest& b, int j, double cs, double tg) {
    const TweakCand x{j, cs, tg};
    if (b.first.j == -1) b.first = x;
    else if (cs + tg > b.first.cs) { b.second = b.first; b.first = x; }
    else if (b.second.j == -1 || cs + tg > b.second.cs) b.second = x;
}
// (e) the far / near / rejected adjustment of a kept candidate's score ...
__host__ __device__ inline void tweak_adjust(const NodeView& v, const TweakCtx& c, TweakCand& x) {
    const int ndx = c.ndx, m = x.j;
    if (m == -1) return;
    if (v.tscore[m] < v.tscore[ndx] && x.cs - v.tscore[m] >= c.sc - v.tscore[ndx] + c.w && v.rscore[m] > v.rscore[ndx] &&
        v.uscore[m] > v.uscore[ndx] && v.cscore[m] > v.cscore[ndx] && abs(v.ndx[m] - v.ndx[ndx]) > 15) {
        x.cs += v.tscore[ndx] - v.tscore[m];
    } else if (abs(v.ndx[m] - v.ndx[ndx]) <= 15 && v.rscore[m] + v.tscore[m] > v.rscore[ndx] + v.tscore[ndx] &&
               v.edge[ndx] == 0 && v.edge[m] == 0) {
        if (v.cscore[ndx] > v.cscore[m]) x.cs += v.cscore[ndx] - v.cscore[m];
        if (v.uscore[ndx] > v.uscore[m]) x.cs += v.uscore[ndx] - v.uscore[m];
        if (c.ig > x.tg) x.cs += c.ig - x.tg;
    } else x.cs = -1000.0;
}
// ... and the pick: the first that beats the gene's own start, the second if it beats that too; the record with its new start
__host__ __device__ inline void tweak_pick(const NodeView& v, const TweakCtx& c, TwoBest& b, GeneRec& cur) {
    tweak_adjust(v, c, b.first);
    tweak_adjust(v, c, b.second);
    int pick = -1;
    double bar = c.sc + c.ig;
    if (b.first.j != -1 && b.first.cs + b.first.tg > bar) { pick = b.first.j; bar = b.first.cs + b.first.tg; }
    if (b.second.j != -1 && b.second.cs + b.second.tg > bar) pick = b.second.j;
    if (pick != -1 && v.strand[pick] == 1) { cur.start_ndx = pick; cur.begin = v.ndx[pick] + 1; }
    else if (pick != -1 && v.strand[pick] == -1) { cur.start_ndx = pick; cur.end = v.ndx[pick] + 1; }
}
// one gene, its 200 neighbours forty at a time: what rules nearly all of them out (b) is asked for in one go -- one memory
// round trip per forty candidates instead of one per candidate, on the device one thread walks them -- then those that
// pass are priced and merged in index order
__host__ __device__ inline void tweak_one(const NodeView& v, const GeneRec* prev, GeneRec& cur, const GeneRec* next, double w, int maxov) {
    const int nn = v.n;
    const TweakCtx c = tweak_context(v, prev, cur, next, w, maxov);
    TwoBest best;
    constexpr int TWB = 40;             // 200 = 5 x 40
    for (int j0 = c.ndx - 100; j0 < c.ndx + 100; j0 += TWB) {
        unsigned long long pass = 0;
#pragma unroll
        for (int q = 0; q < TWB; q++) {
            const int j = j0 + q;
            const int jj = j < 0 ? 0 : (j >= nn ? nn - 1 : j);
            const bool ok = tweak_same_orf_start(v, c, jj) && j >= 0 && j < nn && j != c.ndx;
            pass |= (unsigned long long)ok << q;
        }
        while (pass) {
            const int j = j0 + __builtin_ctzll(pass);
            pass &= pass - 1ull;
            double tg;
            if (tweak_price(v, c, j, tg)) tweak_take(best, j, v.cscore[j] + v.sscore[j], tg);
        }
    }
    tweak_pick(v, c, best, cur);
}
// only a reverse-strand predecessor hands its START to the next gene's tweak (a forward one hands its stop, which never
// moves): that is the one case the in-order pass has to revisit
__host__ __device__ inline bool tweak_moved_reverse_start(const NodeView& v, const GeneRec& cur, const GeneRec& orig) {
    return cur.start_ndx != orig.start_ndx && v.strand[cur.start_ndx] == -1;
}

// ---- the public gene record (ref: lib.pyx:2644-2830 for what Gene reads) -----------------------------------------------------
// Which arrays, and which element of them, hold the fields of a gene's two nodes.  Single mode keeps the nodes of the DP pass
// (ref: lib.pyx:5296-5311), meta mode re-scores (5380-5394): the edge flags and the five scores come from the one or the
// other, the motif and RBS fields and the GC content always from the final pass.  The source is picked first; gene_record
// then loads from it alone.
struct GeneSrc {
    const int8_t* strand; const uint8_t* type; int64_t topo;                 // the start node's strand and type at [topo]
    const uint8_t* edge_s; const uint8_t* edge_e;                            // the start node's edge flag at [sc], the stop node's at [sc_stop]
    const double* cscore; const double* rscore; const double* uscore; const double* tscore;     // ... of the start node, at [sc]
    const double* sscore;                                                    // at [ss] (the tail adds to it: it may sit elsewhere)
    int64_t sc, sc_stop, ss;
    const uint8_t* rbs; const uint8_t* mot_len; const uint8_t* mot_spacer; const int32_t* mot_ndx; const double* mot_score;
    int64_t mot;                                                             // the start node's motif fields at [mot], rbs at [2 mot]
    const float* gc_cont; int64_t gc;

    __host__ __device__ void topology(const int8_t* strand_, const uint8_t* type_, int64_t i) { strand = strand_; type = type_; topo = i; }
    __host__ __device__ void scores(const uint8_t* edge_, const double* c_, const double* s_, const double* r_, const double* u_, const double* t_,
                                    int64_t start, int64_t stop, int64_t start_of_sscore) {
        edge_s = edge_e = edge_; cscore = c_; sscore = s_; rscore = r_; uscore = u_; tscore = t_;
        sc = start; sc_stop = stop; ss = start_of_sscore;
    }
    __host__ __device__ void motifs(const uint8_t* rbs_, const uint8_t* len_, const uint8_t* spacer_, const int32_t* ndx_, const double* score_, int64_t i,
                                    const float* gc_, int64_t gc_i) {
        rbs = rbs_; mot_len = len_; mot_spacer = spacer_; mot_ndx = ndx_; mot_score = score_; mot = i; gc_cont = gc_; gc = gc_i;
    }
};
__host__ __device__ inline pga_gene gene_record(const int contig, const GeneRec& gr, const GeneSrc& s) {
    pga_gene G;
    memset(&G, 0, sizeof G);
    G.contig = contig; G.begin = gr.begin; G.end = gr.end; G.start_ndx = gr.start_ndx; G.stop_ndx = gr.stop_ndx;
    G.strand = s.strand[s.topo];
    const uint8_t se = s.edge_s[s.sc], ee = s.edge_e[s.sc_stop];
    G.partial_begin = G.strand == 1 ? se : ee; G.partial_end = G.strand == 1 ? ee : se;
    G.start_type = se ? 3 : s.type[s.topo];
    G.rbs[0] = s.rbs[2 * s.mot]; G.rbs[1] = s.rbs[2 * s.mot + 1];
    G.mot_len = s.mot_len[s.mot]; G.mot_spacer = s.mot_spacer[s.mot]; G.mot_ndx = s.mot_ndx[s.mot]; G.mot_score = s.mot_score[s.mot];
    G.gc_cont = s.gc_cont[s.gc];
    G.cscore = s.cscore[s.sc]; G.sscore = s.sscore[s.ss]; G.rscore = s.rscore[s.sc]; G.uscore = s.uscore[s.sc]; G.tscore = s.tscore[s.sc];
    return G;
}
