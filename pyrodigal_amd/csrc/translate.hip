// Device-side translation of gene records into proteins: one thread per codon.
// ref: lib.pyx:2932-3047 (Gene.translate), 770-789 (Sequence._amino); the codes and codon rules are in translate_rules.h.
#include "pga_internal.h"
#include <mutex>
#include "pipeline.h"
#include "translate_rules.h"

#include <hipcub/hipcub.hpp>

#include <float.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <numeric>
#include <string>
#include <type_traits>
#include <vector>

struct pga_batch_view { pga_ctx* ctx; int32_t n; int64_t total; const ContigDesc* ct; const char* d_seq; const uint8_t* circular /* or nullptr: all linear */; };
pga_batch_view pga_batch_peek(const pga_batch*);      // finder.hip
struct pga_upload_lease { hipStream_t st; hipEvent_t ev; char* pin; char* dev; };
int  pga_upload_lease_take(pga_ctx*, size_t bytes, pga_upload_lease* out);   // finder.hip: up_mu is held until _give
void pga_upload_lease_give(pga_ctx*);

namespace {

using namespace pga_tr;

__constant__ char c_code[34][64];      // [table][a << 4 | b << 2 | c] with A0 G1 C2 T3; all-zero rows = unknown tables
__constant__ unsigned char c_known[34];

__global__ void __launch_bounds__(256)
k_translate(const char* __restrict__ seq, const ContigDesc* __restrict__ ct, const pga_gene* __restrict__ genes, const int64_t n_genes,
            const int32_t* __restrict__ tt_of, const int64_t* __restrict__ off, const int unk, const int include_stop, const int strict,
            char* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= off[n_genes]) return;
    int64_t lo = 0, hi = n_genes - 1;
    while (lo < hi) { const int64_t mid = (lo + hi + 1) >> 1; if (off[mid] <= idx) lo = mid; else hi = mid - 1; }
    const pga_gene g = genes[lo];
    const int i = (int)(idx - off[lo]);
    const ContigDesc cd = ct[g.contig];
    const char* __restrict__ s = seq + cd.base;
    const int tt = tt_of[g.contig];
    // a gene across the origin of a circular contig reads position p >= len at p - len (the host checked that only such genes get there)
    auto at = [&](const int p) { return s[p >= cd.len ? p - cd.len : p]; };
    int x0, x1, x2;
    if (g.strand == 1) {
        const int p = g.begin - 1 + 3 * i;
        x0 = digit_of(at(p), false); x1 = digit_of(at(p + 1), false); x2 = digit_of(at(p + 2), false);
    } else {
        const int p = g.end - 1 - 3 * i;
        x0 = digit_of(at(p), true); x1 = digit_of(at(p - 1), true); x2 = digit_of(at(p - 2), true);
    }
    // partial flags are in sequence orientation; the gene's own first codon follows its strand
    const bool start_edge = g.strand == 1 ? g.partial_begin : g.partial_end;
    out[idx] = translate_codon(c_code[tt], x0, x1, x2, tt, i, start_edge, strict, unk);
}

// the tables are __constant__ symbols: one copy per DEVICE, so readiness is tracked per device (several GPUs may be driven
// from one process) and the first use on a device uploads them under a lock
std::mutex g_tables_mu;
bool g_tables_ready[64] = {false};
int upload_tables() {
    static char code[34][64];
    static unsigned char known[34];
    code_table(code, known);
    if (hipMemcpyToSymbol(HIP_SYMBOL(c_code), code, sizeof code) != hipSuccess) return PGA_EDEVICE;
    if (hipMemcpyToSymbol(HIP_SYMBOL(c_known), known, sizeof known) != hipSuccess) return PGA_EDEVICE;
    return PGA_OK;
}

int tables_ready(pga_ctx* c) {
    std::lock_guard<std::mutex> lk(g_tables_mu);
    const int dev = c->device & 63;
    if (!g_tables_ready[dev]) { const int rc = upload_tables(); if (rc) return rc; g_tables_ready[dev] = true; }
    return PGA_OK;
}

// a record lies inside its contig; on a contig flagged circular it may run across the origin, over less than the whole circle
bool gene_inside(const pga_batch_view& bv, const pga_gene& G) {
    if (G.contig < 0 || G.contig >= bv.n || G.begin < 1 || G.end < G.begin) return false;
    const int64_t len = bv.ct[G.contig].len;
    return bv.circular && bv.circular[G.contig] ? G.begin <= len && (int64_t)G.end - G.begin < len : G.end <= len;
}
// the residues of a record (ref: lib.pyx:3006-3018): the final stop codon counts only with include_stop, and not at a partial end
int64_t gene_residues(const pga_gene& G, const int include_stop) {
    const bool stop_edge = G.strand == 1 ? G.partial_end : G.partial_begin;
    const int64_t r = ((int64_t)G.end - G.begin + 1) / 3 - ((!stop_edge && !include_stop) ? 1 : 0);
    return r > 0 ? r : 0;
}

#include "device_rows.inl"
#include "translate_tokens.inl"
#include "label_bases.inl"
#include "gene_windows.inl"
#include "kmer_counts.inl"
#include "protein_groups.inl"
#include "protein_sketches.inl"
#include "protein_clusters.inl"
#include "protein_alignments.inl"
#include "start_candidates.inl"

// the records as k_string_digest, k_group_verify and k_sketch read them
void grp_rows(GrpRow* rows, const pga_gene* genes, const int64_t n, const pga_batch_view& bv, const bool protein, const int include_stop,
              const int32_t* table_of_contig) {
    for (int64_t g = 0; g < n; g++) {
        const pga_gene& R = genes[g];
        const bool fwd = R.strand == 1;
        GrpRow& w = rows[g];
        w.base = bv.ct[R.contig].base; w.L = bv.ct[R.contig].len;
        w.q0 = fwd ? R.begin - 1 : R.end - 1;
        w.n = protein ? (int32_t)gene_residues(R, include_stop) : R.end - R.begin + 1;
        // partial flags are in sequence orientation; the gene's own first codon follows its strand
        const bool start_edge = fwd ? R.partial_begin != 0 : R.partial_end != 0;
        w.bits = (fwd ? 1u : 0u) | (start_edge ? 2u : 0u) | (protein ? (uint32_t)table_of_contig[R.contig] << 8 : 0u);
    }
}

}  // namespace

extern "C" int pga_translate_genes(pga_ctx* c, const pga_batch* batch, int64_t n_genes, const pga_gene* genes, const int32_t* table_of_contig,
                                   int unknown_residue, int include_stop, int strict, const int64_t* offsets, char* out) {
    if (!c || !batch || n_genes < 0 || (n_genes > 0 && (!genes || !table_of_contig || !offsets || !out))) { if (c) c->err = "pga_translate_genes: bad arguments"; return PGA_EINVAL; }
    const pga_batch_view bv = pga_batch_peek(batch);
    if (bv.ctx != c) { c->err = "pga_translate_genes: the batch belongs to another context"; return PGA_EINVAL; }
    if (n_genes == 0) return PGA_OK;
    if (unknown_residue <= 0 || unknown_residue > 127) { c->err = "pga_translate_genes: `unknown_residue` must be a single ASCII character"; return PGA_EINVAL; }
    for (int i = 0; i < bv.n; i++)
        if (!table_known(table_of_contig[i])) { c->err = "pga_translate_genes: not a valid translation table index"; return PGA_EINVAL; }
    // the caller's layout must be the one the kernel writes
    if (offsets[0] != 0) { c->err = "pga_translate_genes: offsets[0] must be 0"; return PGA_EINVAL; }
    for (int64_t g = 0; g < n_genes; g++) {
        if (!gene_inside(bv, genes[g])) { c->err = "pga_translate_genes: gene outside its contig"; return PGA_EINVAL; }
        if (offsets[g + 1] - offsets[g] != gene_residues(genes[g], include_stop)) { c->err = "pga_translate_genes: offsets do not match the gene lengths"; return PGA_EINVAL; }
    }
    const int64_t total = offsets[n_genes];
    if (total == 0) return PGA_OK;
    if (hipSetDevice(c->device) != hipSuccess) return PGA_EDEVICE;
    { const int rc = tables_ready(c); if (rc) return rc; }
    pga_gene* d_genes = nullptr; int32_t* d_tt = nullptr; int64_t* d_off = nullptr; char* d_out = nullptr; ContigDesc* d_ct = nullptr;
    auto cleanup = [&]() { hipFree(d_genes); hipFree(d_tt); hipFree(d_off); hipFree(d_out); hipFree(d_ct); };
    hipStream_t st = c->stream;
    hipError_t e = hipMalloc((void**)&d_genes, sizeof(pga_gene) * (size_t)n_genes);
    if (e == hipSuccess) e = hipMalloc((void**)&d_tt, sizeof(int32_t) * (size_t)bv.n);
    if (e == hipSuccess) e = hipMalloc((void**)&d_off, sizeof(int64_t) * (size_t)(n_genes + 1));
    if (e == hipSuccess) e = hipMalloc((void**)&d_out, (size_t)total);
    if (e == hipSuccess) e = hipMalloc((void**)&d_ct, sizeof(ContigDesc) * (size_t)(bv.n + 1));
    if (e == hipSuccess) e = hipMemcpyAsync(d_genes, genes, sizeof(pga_gene) * (size_t)n_genes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_tt, table_of_contig, sizeof(int32_t) * (size_t)bv.n, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off, offsets, sizeof(int64_t) * (size_t)(n_genes + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_ct, bv.ct, sizeof(ContigDesc) * (size_t)(bv.n + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_translate, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, bv.d_seq, d_ct, d_genes, n_genes, d_tt, d_off,
                           unknown_residue, include_stop, strict, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, (size_t)total, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    cleanup();
    return pga_hip_try_(c, e, "pga_translate_genes");
}

extern "C" int pga_translate_genes_tokens(pga_ctx* c, const pga_batch* batch, int64_t n_genes, const pga_gene* genes, const int32_t* table_of_contig,
                                          const pga_token_opts* o, void* d_out, int64_t n_out_elems, void* stream, int64_t* len_out) {
    if (!c) return PGA_EINVAL;
    RowDest d{c, "pga_translate_genes_tokens"};
    if (!batch || !o || n_genes < 0 || n_out_elems < 0 || (n_genes > 0 && (!genes || !table_of_contig || !len_out))) return d.bad("bad arguments");
    const pga_batch_view bv = pga_batch_peek(batch);
    if (bv.ctx != c) return d.bad("the batch belongs to another context");
    // ---- validation: all of it on the host, before anything is allocated or launched ----
    if (const int rc = d.format(o->elem_bytes, o->layout)) return rc;
    if (o->unknown_residue <= 0 || o->unknown_residue > 127) return d.bad("`unknown_residue` must be a single ASCII character");
    const bool has_bos = o->bos != PGA_TOKEN_NONE, has_eos = o->eos != PGA_TOKEN_NONE;
    const int64_t s = (has_bos ? 1 : 0) + (has_eos ? 1 : 0);
    if (const int rc = d.fits("vocab", o->vocab, 128)) return rc;
    if (has_bos) if (const int rc = d.fits("bos", o->bos)) return rc;
    if (has_eos) if (const int rc = d.fits("eos", o->eos)) return rc;
    if (d.padded) if (const int rc = d.fits("pad", o->pad)) return rc;
    if (o->max_length < 0 || (o->max_length != 0 && o->max_length < s + 1))
        return d.bad("max_length = " + std::to_string(o->max_length) + " leaves no room for a residue beside " + std::to_string(s) + " special tokens (0: no limit)");
    if (n_genes > 0) if (const int rc = d.tables_known(bv, table_of_contig)) return rc;
    std::vector<int64_t> off((size_t)n_genes + 1, 0);
    for (int64_t g = 0; g < n_genes; g++) {
        if (const int rc = d.record_inside(bv, genes[g], g)) return rc;
        int64_t r = gene_residues(genes[g], o->include_stop);
        if (o->max_length != 0 && r > o->max_length - s) r = o->max_length - s;
        off[(size_t)g + 1] = off[(size_t)g] + s + r;
    }
    if (const int rc = d.shape(off, "tokens of gene", o->row_width, o->row_stride, o->pad, n_out_elems)) return rc;
    if (const int rc = d.memory(d_out)) return rc;
    for (int64_t g = 0; g < n_genes; g++) len_out[g] = off[(size_t)g + 1] - off[(size_t)g];
    if (d.a.n_elems == 0) return PGA_OK;
    { const int rc = tables_ready(c); if (rc) return rc; }
    // ---- the kernel's tables: staged in the upload's pinned area as they will lie on the device, one copy ----
    const size_t G = (size_t)n_genes, n = (size_t)bv.n;
    Staging tab;
    const size_t p_off = tab.put(off.data(), sizeof(int64_t) * (G + 1)), p_voc = tab.put(o->vocab, sizeof(int64_t) * 128), p_ct = tab.put(bv.ct, sizeof(ContigDesc) * (n + 1));
    const size_t p_gen = tab.put(genes, sizeof(pga_gene) * G), p_tt = tab.put(table_of_contig, sizeof(int32_t) * n);
    if (const int rc = tab.lease(c)) return rc;
    TokArgs a{};
    a.rows = d.a; a.rows.off = tab.dev<const int64_t>(p_off);
    a.seq = bv.d_seq;
    a.vocab = tab.dev<const int64_t>(p_voc); a.ct = tab.dev<const ContigDesc>(p_ct);
    a.genes = tab.dev<const pga_gene>(p_gen); a.tt_of = tab.dev<const int32_t>(p_tt);
    a.bos = has_bos ? o->bos : 0; a.eos = has_eos ? o->eos : 0;
    a.has_bos = has_bos; a.has_eos = has_eos; a.unk = o->unknown_residue; a.strict = o->strict;
    return d.run(tab, stream, [&](const dim3 grid, const dim3 block, hipStream_t st) {
        with_elem_layout(d.eb, d.padded, [&](auto EB, auto PADDED) {
            hipLaunchKernelGGL((k_translate_tokens<decltype(EB)::value, decltype(PADDED)::value>), grid, block, 0, st, a);
        });
    });
}

extern "C" int pga_label_bases(pga_ctx* c, const pga_batch* batch, int64_t n_genes, const pga_gene* genes, const pga_label_opts* o, void* d_out,
                               int64_t n_out_elems, void* stream, int64_t* len_out) {
    if (!c) return PGA_EINVAL;
    RowDest d{c, "pga_label_bases"};
    if (!batch || !o || n_genes < 0 || n_out_elems < 0 || (n_genes > 0 && !genes)) return d.bad("bad arguments");
    const pga_batch_view bv = pga_batch_peek(batch);
    if (bv.ctx != c) return d.bad("the batch belongs to another context");
    if (bv.n > 0 && !len_out) return d.bad("bad arguments");
    // ---- validation: all of it on the host, before anything is allocated or launched ----
    if (const int rc = d.format(o->elem_bytes, o->layout)) return rc;
    if (const int rc = d.fits("class_map", o->class_map, 256)) return rc;
    if (d.padded) if (const int rc = d.fits("pad", o->pad)) return rc;
    const size_t B = (size_t)bv.n;
    std::vector<int64_t> off(B + 1, 0), iv_off(B + 1, 0);
    for (size_t i = 0; i < B; i++) {
        if (bv.ct[i].len > INT32_MAX - 16) return d.bad("contig " + std::to_string(i) + " is too long");
        off[i + 1] = off[i] + bv.ct[i].len;
    }
    if (const int rc = d.shape(off, "bases of contig", o->row_width, o->row_stride, o->pad, n_out_elems)) return rc;
    // every record inside its contig, in whole codons; a record across the origin makes two stretches
    for (int64_t g = 0; g < n_genes; g++) {
        const pga_gene& G = genes[g];
        if (const int rc = d.whole_codon_record(bv, G, g)) return rc;
        iv_off[(size_t)G.contig + 1] += G.end > bv.ct[G.contig].len ? 2 : 1;
    }
    if (const int rc = d.memory(d_out)) return rc;
    for (size_t i = 0; i < B; i++) len_out[i] = bv.ct[i].len;
    if (d.a.n_elems == 0) return PGA_OK;
    // ---- the kernel's tables: staged in the upload's pinned area as they will lie on the device, one copy ----
    for (size_t i = 0; i < B; i++) iv_off[i + 1] += iv_off[i];
    Staging tab;
    const size_t p_off = tab.put(off.data(), sizeof(int64_t) * (B + 1)), p_ivoff = tab.put(iv_off.data(), sizeof(int64_t) * (B + 1));
    const size_t p_map = tab.put(o->class_map, sizeof(int64_t) * 256), p_iv = tab.take(sizeof(LabIv) * (size_t)iv_off[B]);      // (the stretches begin at a multiple of 16 bytes)
    if (const int rc = tab.lease(c)) return rc;
    lab_stretches(genes, n_genes, bv.ct, iv_off.data(), B, tab.pin<LabIv>(p_iv));
    LabArgs a{};
    a.rows = d.a; a.rows.off = tab.dev<const int64_t>(p_off);
    a.iv_off = tab.dev<const int64_t>(p_ivoff); a.cmap = tab.dev<const int64_t>(p_map);
    a.iv = tab.dev<const LabIv>(p_iv);
    return d.run(tab, stream, [&](const dim3 grid, const dim3 block, hipStream_t st) {
        with_elem_layout(d.eb, d.padded, [&](auto EB, auto PADDED) {
            hipLaunchKernelGGL((k_label_bases<decltype(EB)::value, decltype(PADDED)::value>), grid, block, 0, st, a);
        });
    });
}

extern "C" int pga_gene_windows(pga_ctx* c, const pga_batch* batch, int64_t n_genes, const pga_gene* genes, const pga_window_opts* o, void* d_out,
                                int64_t n_out_elems, void* stream, int64_t* len_out) {
    if (!c) return PGA_EINVAL;
    RowDest d{c, "pga_gene_windows"};
    if (!batch || !o || n_genes < 0 || n_out_elems < 0 || (n_genes > 0 && (!genes || !len_out))) return d.bad("bad arguments");
    const pga_batch_view bv = pga_batch_peek(batch);
    if (bv.ctx != c) return d.bad("the batch belongs to another context");
    // ---- validation: all of it on the host, before anything is allocated or launched ----
    if (const int rc = d.format(o->elem_bytes, o->layout)) return rc;
    if (o->unit != PGA_WINDOW_BASES && o->unit != PGA_WINDOW_CODONS) return d.bad("unit must be PGA_WINDOW_BASES or PGA_WINDOW_CODONS, not " + std::to_string(o->unit));
    const bool codons = o->unit == PGA_WINDOW_CODONS;
    const bool has_bos = o->bos != PGA_TOKEN_NONE, has_eos = o->eos != PGA_TOKEN_NONE;
    const int64_t s = (has_bos ? 1 : 0) + (has_eos ? 1 : 0);
    if (const int rc = d.fits("ids", o->ids, codons ? 66 : 6)) return rc;
    if (has_bos) if (const int rc = d.fits("bos", o->bos)) return rc;
    if (has_eos) if (const int rc = d.fits("eos", o->eos)) return rc;
    if (d.padded) if (const int rc = d.fits("pad", o->pad)) return rc;
    const struct { const char* name; int32_t anchor; int64_t delta; } ends[2] = {{"from", o->from_anchor, o->from_delta}, {"to", o->to_anchor, o->to_delta}};
    for (const auto& x : ends) {
        if (x.anchor != PGA_WINDOW_START && x.anchor != PGA_WINDOW_END)
            return d.bad(std::string(x.name) + "_anchor must be PGA_WINDOW_START or PGA_WINDOW_END, not " + std::to_string(x.anchor));
        if (x.delta < -((int64_t)1 << 30) || x.delta > ((int64_t)1 << 30))
            return d.bad(std::string(x.name) + "_delta = " + std::to_string(x.delta) + " is beyond 2^30 in size");
        if (codons && x.delta % 3) return d.bad(std::string(x.name) + "_delta = " + std::to_string(x.delta) + " is no multiple of 3, which the codon unit needs");
    }
    if (o->max_length < 0 || (o->max_length != 0 && o->max_length < s + 1))
        return d.bad("max_length = " + std::to_string(o->max_length) + " leaves no room for a unit beside " + std::to_string(s) + " special tokens (0: no limit)");
    // every record inside its contig, in whole codons; the tokens of its row
    const int64_t per_unit = codons ? 3 : 1;
    std::vector<int64_t> off((size_t)n_genes + 1, 0);
    for (int64_t g = 0; g < n_genes; g++) {
        const pga_gene& G = genes[g];
        if (const int rc = d.whole_codon_record(bv, G, g)) return rc;
        const int64_t glen = (int64_t)G.end - G.begin + 1;
        const int64_t t_lo = (o->from_anchor == PGA_WINDOW_END ? glen : 0) + o->from_delta, t_hi = (o->to_anchor == PGA_WINDOW_END ? glen : 0) + o->to_delta;
        int64_t r = t_hi > t_lo ? (t_hi - t_lo) / per_unit : 0;
        if (o->max_length != 0 && r > o->max_length - s) r = o->max_length - s;
        off[(size_t)g + 1] = off[(size_t)g] + s + r;
    }
    if (const int rc = d.shape(off, "tokens of gene", o->row_width, o->row_stride, o->pad, n_out_elems)) return rc;
    if (const int rc = d.memory(d_out)) return rc;
    for (int64_t g = 0; g < n_genes; g++) len_out[g] = off[(size_t)g + 1] - off[(size_t)g];
    if (d.a.n_elems == 0) return PGA_OK;
    // ---- the kernel's tables: staged in the upload's pinned area as they will lie on the device, one copy ----
    const size_t G = (size_t)n_genes;
    Staging tab;
    const size_t p_off = tab.put(off.data(), sizeof(int64_t) * (G + 1)), p_ids = tab.put(o->ids, sizeof(int64_t) * 66), p_win = tab.take(sizeof(WinRow) * G);
    if (const int rc = tab.lease(c)) return rc;
    WinRow* const win = tab.pin<WinRow>(p_win);
    for (size_t g = 0; g < G; g++) {
        const pga_gene& R = genes[g];
        const int64_t glen = (int64_t)R.end - R.begin + 1;
        win[g] = win_row(R, bv.ct[R.contig], bv.circular && bv.circular[R.contig], (o->from_anchor == PGA_WINDOW_END ? glen : 0) + o->from_delta);
    }
    WinArgs a{};
    a.rows = d.a; a.rows.off = tab.dev<const int64_t>(p_off);
    a.seq = bv.d_seq;
    a.ids = tab.dev<const int64_t>(p_ids); a.win = tab.dev<const WinRow>(p_win);
    a.bos = has_bos ? o->bos : 0; a.eos = has_eos ? o->eos : 0;
    a.has_bos = has_bos; a.has_eos = has_eos; a.codons = codons;
    return d.run(tab, stream, [&](const dim3 grid, const dim3 block, hipStream_t st) {
        with_elem_layout(d.eb, d.padded, [&](auto EB, auto PADDED) {
            hipLaunchKernelGGL((k_gene_windows<decltype(EB)::value, decltype(PADDED)::value>), grid, block, 0, st, a);
        });
    });
}

extern "C" int pga_kmer_counts_chunk(void) { return kCntChunk; }

extern "C" int pga_count_kmers(pga_ctx* c, const pga_batch* batch, int64_t n_genes, const pga_gene* genes, const pga_count_opts* o, void* d_out,
                               int64_t n_out_elems, void* stream, int64_t* win_out) {
    if (!c) return PGA_EINVAL;
    const Knobs kn = read_knobs();
    RowDest d{c, "pga_count_kmers"};
    if (!batch || !o || n_genes < 0 || n_out_elems < 0) return d.bad("bad arguments");
    const pga_batch_view bv = pga_batch_peek(batch);
    if (bv.ctx != c) return d.bad("the batch belongs to another context");
    // ---- validation: all of it on the host, before anything is allocated or launched ----
    if (o->rows != PGA_COUNT_CONTIG && o->rows != PGA_COUNT_GENE && o->rows != PGA_COUNT_CONTIG_GENES)
        return d.bad("rows must be PGA_COUNT_CONTIG, PGA_COUNT_GENE or PGA_COUNT_CONTIG_GENES, not " + std::to_string(o->rows));
    const bool by_contig = o->rows == PGA_COUNT_CONTIG, summed = o->rows == PGA_COUNT_CONTIG_GENES;
    if (by_contig) n_genes = 0;                                    // (contig rows read no records)
    if (n_genes > 0 && !genes) return d.bad("bad arguments");
    const int64_t k = o->k, step = o->step;
    if (k < 1 || k > 6) return d.bad("k must be 1 .. 6, not " + std::to_string(k));
    if (by_contig ? step != 1 : (step != 1 && step != 3)) return d.bad(std::string("step must be ") + (by_contig ? "1 for contig rows" : "1 or 3") + ", not " + std::to_string(step));
    if (o->n_bins < 1 || o->n_bins > kCntMaxBins) return d.bad("n_bins must be 1 .. " + std::to_string(kCntMaxBins) + ", not " + std::to_string(o->n_bins));
    if (!o->bin_of_code) return d.bad("bin_of_code is NULL");
    const int n_codes = 1 << (2 * (int)k);
    for (int x = 0; x < n_codes; x++)
        if (o->bin_of_code[x] < -1 || o->bin_of_code[x] >= o->n_bins)
            return d.bad("bin_of_code[" + std::to_string(x) + "] = " + std::to_string(o->bin_of_code[x]) + " lies outside -1 .. n_bins - 1 = " + std::to_string(o->n_bins - 1));
    const int64_t B = bv.n, R = o->rows == PGA_COUNT_GENE ? n_genes : B, S = o->row_stride, n_bins = o->n_bins;
    if (R > 0 && !win_out) return d.bad("bad arguments");
    if (S < n_bins) return d.bad("row_stride = " + std::to_string(S) + " is less than n_bins = " + std::to_string(n_bins));
    if (R > 1 && S > (INT64_MAX / 8 - n_bins) / (R - 1)) return d.bad("row_stride = " + std::to_string(S) + " is too large");
    d.eb = 4; d.a.n_rows = R; d.a.n_elems = R > 0 ? (R - 1) * S + n_bins : 0;
    if (const int rc = d.room(n_out_elems)) return rc;
    // the rows of work: a contig each, or a checked record each; the windows of every row of d_out
    const size_t NW = (size_t)(by_contig ? B : n_genes);
    if (NW > (size_t)INT32_MAX) return d.bad("more than 2^31 - 1 gene records");
    std::vector<CntRow> rows(NW);
    std::vector<int64_t> win((size_t)R, 0);
    auto windows = [&](const int64_t n) { return n >= k ? (n - k) / step + 1 : (int64_t)0; };
    for (size_t i = 0; i < NW; i++) {
        CntRow& w = rows[i];
        w._pad = 0;
        if (by_contig) {
            const ContigDesc& cd = bv.ct[i];
            const bool circ = bv.circular && bv.circular[i];
            w.base = cd.base; w.q0 = 0; w.L = cd.len; w.dst = (int32_t)i; w.bits = 1u;
            w.n_win = (int32_t)(cd.len < k ? 0 : circ ? cd.len : cd.len - k + 1);
            win[i] = w.n_win;
            continue;
        }
        const pga_gene& G = genes[i];
        if (const int rc = d.whole_codon_record(bv, G, (int64_t)i)) return rc;
        const WinRow q = win_row(G, bv.ct[G.contig], bv.circular && bv.circular[G.contig], 0);
        w.base = q.base; w.q0 = (int32_t)q.q0; w.L = q.L; w.bits = q.bits & 1u;
        w.n_win = (int32_t)windows((int64_t)G.end - G.begin + 1);
        w.dst = summed ? G.contig : (int32_t)i;
        win[(size_t)w.dst] += w.n_win;
    }
    for (int64_t r = 0; r < R; r++)
        if (win[(size_t)r] > INT32_MAX)
            return d.bad(std::string(summed ? "contig " : "row ") + std::to_string(r) + " has " + std::to_string(win[(size_t)r]) + " window positions, more than an int32 count holds");
    if (const int rc = d.memory(d_out)) return rc;
    for (int64_t r = 0; r < R; r++) win_out[r] = win[(size_t)r];
    if (R == 0) return PGA_OK;
    // ---- the pieces, and the form of the kernel ----
    // A row of d_out that one piece owns whole is set by that piece; every other row is zeroed on the stream and added to.
    // PGA_KMER_COUNTS_FORM (lds / direct, with -wave / -group) forces a form for measurements and tests.
    std::vector<int2> piece;                                     // (row, the first of its window starts)
    piece.reserve(NW);
    std::vector<char> cut(NW, 0);                                // the row has more than one piece
    int64_t total_win = 0;
    for (size_t i = 0; i < NW; i++) {
        for (int64_t w = 0; w < rows[i].n_win || (w == 0 && !summed); w += kCntChunk) piece.push_back(make_int2((int)i, (int)w));
        cut[i] = rows[i].n_win > kCntChunk;
        total_win += rows[i].n_win;
    }
    const int64_t pieces = (int64_t)piece.size();
    // the forms (DESIGN.md 4.18 has the measurements): without a histogram where the rows are shared and hold few windows under
    // many bins; a piece per wave where the pieces are short and four histograms fit
    bool direct = summed && pieces > 0 && total_win / pieces < n_bins / 4;
    bool per_wave = pieces > 0 && total_win / pieces <= kCntSweep;
    if (kn.kmer_direct >= 0) direct = kn.kmer_direct != 0;
    if (kn.kmer_per_wave >= 0) per_wave = kn.kmer_per_wave != 0;
    if (!direct && 4 * n_bins > kCntMaxBins) per_wave = false;
    std::vector<int32_t> zero;
    if (summed || direct) { zero.resize((size_t)R); std::iota(zero.begin(), zero.end(), 0); for (auto& w : rows) w.bits |= 2u; }
    else for (size_t i = 0; i < NW; i++) if (cut[i]) { rows[i].bits |= 2u; zero.push_back(rows[i].dst); }
    // ---- the kernel's tables: staged in the upload's pinned area as they will lie on the device, one copy ----
    Staging tab(16);
    const size_t p_piece = tab.put(piece.data(), sizeof(int2) * piece.size()), p_row = tab.put(rows.data(), sizeof(CntRow) * NW);
    const size_t p_bin = tab.put(o->bin_of_code, sizeof(int32_t) * (size_t)n_codes), p_zero = tab.put(zero.data(), sizeof(int32_t) * zero.size());
    if (const int rc = tab.lease(c)) return rc;
    CntArgs a{};
    a.seq = bv.d_seq; a.piece = tab.dev<const int2>(p_piece); a.row = tab.dev<const CntRow>(p_row);
    a.bin_of_code = tab.dev<const int32_t>(p_bin);
    a.out = (int32_t*)d_out; a.n_pieces = pieces; a.S = S;
    a.k = (int32_t)k; a.step = (int32_t)step; a.n_bins = (int32_t)n_bins; a.wide = ((uintptr_t)bv.d_seq & 3u) == 0;
    const int32_t* d_zero = tab.dev<const int32_t>(p_zero);
    const int64_t n_zero = (int64_t)zero.size();
    return d.run(tab, stream, [&](const dim3, const dim3 block, hipStream_t st) {
        if (n_zero > 0) hipLaunchKernelGGL(k_kmer_zero, dim3((unsigned)((n_zero * n_bins + kRowThreads - 1) / kRowThreads)), block, 0, st, a.out, S, a.n_bins, d_zero, n_zero);
        if (pieces == 0) return;
        const dim3 grid((unsigned)(per_wave ? (pieces + 3) / 4 : pieces));
        const size_t lds = cnt_lds_bytes(direct, per_wave ? 4 : 1, (int)n_bins, n_codes);
        if (direct && per_wave) hipLaunchKernelGGL((k_kmer_counts<true, 4>), grid, block, lds, st, a);
        else if (direct) hipLaunchKernelGGL((k_kmer_counts<true, 1>), grid, block, lds, st, a);
        else if (per_wave) hipLaunchKernelGGL((k_kmer_counts<false, 4>), grid, block, lds, st, a);
        else hipLaunchKernelGGL((k_kmer_counts<false, 1>), grid, block, lds, st, a);
    });
}

// ---- identical proteins (protein_groups.inl) ----------------------------------------------------------------------------------
extern "C" int pga_protein_groups_stats(pga_ctx* c, int64_t out[2]) {
    if (!c || !out) return PGA_EINVAL;
    out[0] = c->group_stats[0]; out[1] = c->group_stats[1];
    return PGA_OK;
}

extern "C" int pga_group_proteins(pga_ctx* c, const pga_batch* batch, int64_t n_genes, const pga_gene* genes, const int32_t* table_of_contig,
                                  const pga_group_opts* o, int64_t* d_group, int64_t* d_representative, int64_t* d_size, int64_t* d_digest,
                                  int64_t capacity, void* stream, int64_t* n_groups) {
    if (!c) return PGA_EINVAL;
    const Knobs kn = read_knobs();
    DevCall d{c, "pga_group_proteins"};
    if (!batch || !o || !n_groups || n_genes < 0 || (n_genes > 0 && !genes)) return d.bad("bad arguments");
    const pga_batch_view bv = pga_batch_peek(batch);
    if (bv.ctx != c) return d.bad("the batch belongs to another context");
    // ---- validation: all of it on the host, before anything is allocated or launched ----
    if (o->unit != PGA_GROUP_PROTEIN && o->unit != PGA_GROUP_GENE) return d.bad("unit must be PGA_GROUP_PROTEIN or PGA_GROUP_GENE, not " + std::to_string(o->unit));
    const bool protein = o->unit == PGA_GROUP_PROTEIN;
    if (o->unknown_residue <= 0 || o->unknown_residue > 127) return d.bad("`unknown_residue` must be a single ASCII character");
    if (n_genes > INT32_MAX) return d.bad("more than 2^31 - 1 gene records");
    if (capacity < 0 || ((d_representative || d_size) && capacity < n_genes))
        return d.bad("capacity = " + std::to_string(capacity) + " is less than the " + std::to_string(n_genes) + " gene records");
    if (protein && n_genes > 0) {
        if (!table_of_contig) return d.bad("table_of_contig is NULL");
        if (const int rc = d.tables_known(bv, table_of_contig)) return rc;
    }
    for (int64_t g = 0; g < n_genes; g++) if (const int rc = d.record_inside(bv, genes[g], g)) return rc;
    const int key_bits = kn.protein_groups_key_bits;
    if (key_bits == 0) return d.bad("PGA_PROTEIN_GROUPS_KEY_BITS must be a number, 1 .. 61");
    c->group_stats[0] = c->group_stats[1] = 0;
    if (n_genes == 0) { *n_groups = 0; return PGA_OK; }
    if (const int rc = d.destinations({{"d_group", d_group, 8, d.kRequired}, {"d_representative", d_representative, 8, d.kOptional},
                                       {"d_size", d_size, 8, d.kOptional}, {"d_digest", d_digest, 8, d.kOptional}})) return rc;
    if (protein) { const int rc = tables_ready(c); if (rc) return rc; }
    // ---- the lease: the records as the kernels read them, staged in the pinned area, and behind them the work arrays of the call ----
    const size_t G = (size_t)n_genes;
    const int iG = (int)n_genes;
    size_t sort_b = 0, max_b = 0, sum_b = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, iG, 0, key_bits, (hipStream_t)nullptr);
    hipcub::DeviceScan::InclusiveScan(nullptr, max_b, (uint32_t*)nullptr, (uint32_t*)nullptr, GrpMax{}, iG, (hipStream_t)nullptr);
    hipcub::DeviceScan::ExclusiveSum(nullptr, sum_b, (int32_t*)nullptr, (int32_t*)nullptr, iG, (hipStream_t)nullptr);
    const size_t tmp_b = std::max(sort_b, std::max(max_b, sum_b));
    Staging tab(256);
    const size_t row_b = sizeof(GrpRow) * G;
    const size_t p_row = tab.take(row_b), p_small = tab.take(256), p_w0 = tab.take(8 * G), p_w1 = tab.take(8 * G), p_skey = tab.take(8 * G), p_idx = tab.take(4 * G), p_sidx = tab.take(4 * G);
    const size_t p_start = tab.take(4 * G), p_runstart = tab.take(4 * G), p_cand0 = tab.take(4 * G), p_cand1 = tab.take(4 * G), p_head = tab.take(4 * G), p_tmp = tab.take(tmp_b + 1);
    if (const int rc = tab.lease(c)) return rc;
    grp_rows(tab.pin<GrpRow>(p_row), genes, n_genes, bv, protein, o->include_stop, table_of_contig);
    volatile long long* const h_small = tab.pin<volatile long long>(p_small);        // [0]: what a round left, [1]: U
    GrpArgs a{};
    a.seq = bv.d_seq; a.row = tab.dev<const GrpRow>(p_row); a.n = n_genes;
    a.unk = o->unknown_residue; a.strict = o->strict; a.precheck = key_bits == 61;
    a.key_mask = (1ull << key_bits) - 1;
    a.w0 = tab.dev<uint64_t>(p_w0); a.w1 = tab.dev<uint64_t>(p_w1); a.idx = tab.dev<uint32_t>(p_idx);
    a.skey = tab.dev<const uint64_t>(p_skey); a.sidx = tab.dev<const uint32_t>(p_sidx);
    a.start = tab.dev<uint32_t>(p_start); a.runstart = tab.dev<uint32_t>(p_runstart);
    a.head = tab.dev<int32_t>(p_head);
    a.unresolved = tab.dev<unsigned long long>(p_small);
    a.d_digest = d_digest;
    uint32_t* const cand[2] = {tab.dev<uint32_t>(p_cand0), tab.dev<uint32_t>(p_cand1)};
    void* const d_tmp = tab.dev<char>(p_tmp);
    size_t tb = tmp_b;
    const dim3 block(kRowThreads), per_gene((unsigned)((n_genes + kRowThreads - 1) / kRowThreads));
    auto launched = [&]() { return hipGetLastError(); };
    int64_t rounds = 0, differing = 0;
    // the records go up; the rounds wait for the stream themselves
    return d.run(tab.L, row_b, stream, [&](hipStream_t st) {
        hipError_t e = hipMemsetAsync(a.head, 0xff, 4 * G, st);
        if (e == hipSuccess) {
            // a wave per four records, and several rounds of them per wave where there are many
            const int64_t quads = (n_genes + 3) / 4, per_block = kRowThreads / 64;
            const dim3 grid((unsigned)std::min<int64_t>((quads + per_block - 1) / per_block, 8192));
            if (protein) hipLaunchKernelGGL((k_string_digest<kGrpProtein>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((k_string_digest<kGrpGene>), grid, block, 0, st, a);
            e = launched();
        }
        if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(d_tmp, tb, (const uint64_t*)a.w0, (uint64_t*)a.skey, (const uint32_t*)a.idx, (uint32_t*)a.sidx, iG, 0, key_bits, st);
        a.cand = cand[0];
        if (e == hipSuccess) { hipLaunchKernelGGL(k_group_runs, per_gene, block, 0, st, a); e = launched(); }
        tb = tmp_b;
        if (e == hipSuccess) e = hipcub::DeviceScan::InclusiveScan(d_tmp, tb, (const uint32_t*)a.start, a.runstart, GrpMax{}, iG, st);
        while (e == hipSuccess) {
            a.cand = cand[rounds & 1]; a.cand_next = cand[(rounds + 1) & 1];
            e = hipMemsetAsync(a.cand_next, 0xff, 4 * G, st);
            if (e == hipSuccess) e = hipMemsetAsync(a.unresolved, 0, 8, st);
            if (e == hipSuccess) {
                if (protein) hipLaunchKernelGGL((k_group_verify<kGrpProtein>), per_gene, block, 0, st, a);
                else hipLaunchKernelGGL((k_group_verify<kGrpGene>), per_gene, block, 0, st, a);
                e = launched();
            }
            if (e == hipSuccess) e = hipMemcpyAsync((void*)h_small, a.unresolved, 8, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) break;
            rounds++;
            const int64_t left = h_small[0];
            differing += left;
            if (left == 0) break;                                  // (a round resolves the head of every run that has members left: it ends)
        }
        // ---- numbering: representatives flagged, an exclusive scan, and the outputs (flags, numbers and counts over the rounds' arrays) ----
        GrpOut w{};
        w.head = a.head; w.flag = (int32_t*)a.start; w.num = (const int32_t*)a.runstart; w.cnt = (int32_t*)cand[0]; w.n = n_genes;
        w.d_group = d_group; w.d_rep = d_representative; w.d_size = d_size; w.n_groups = tab.dev<long long>(p_small) + 1;
        if (e == hipSuccess) { hipLaunchKernelGGL(k_group_flags, per_gene, block, 0, st, w); e = launched(); }
        tb = tmp_b;
        if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, (const int32_t*)w.flag, (int32_t*)a.runstart, iG, st);
        if (e == hipSuccess) { hipLaunchKernelGGL(k_group_count, per_gene, block, 0, st, w); e = launched(); }
        if (e == hipSuccess && (d_representative || d_size)) { hipLaunchKernelGGL(k_group_emit, per_gene, block, 0, st, w); e = launched(); }
        if (e == hipSuccess) e = hipMemcpyAsync((void*)(h_small + 1), w.n_groups, 8, hipMemcpyDeviceToHost, st);
        return e;
    }, [&] { *n_groups = h_small[1]; c->group_stats[0] = rounds; c->group_stats[1] = differing; });
}

// ---- MinHash sketches (protein_sketches.inl) -----------------------------------------------------------------------------------
extern "C" int pga_sketch_passes(pga_ctx* c, int64_t* out) {
    if (!c || !out) return PGA_EINVAL;
    *out = c->sketch_passes;
    return PGA_OK;
}

extern "C" int pga_sketch_proteins(pga_ctx* c, const pga_batch* batch, int64_t n_genes, const pga_gene* genes, const int32_t* table_of_contig,
                                   const pga_sketch_opts* o, int64_t* d_sketch, int64_t* d_count, int64_t* d_windows, void* stream) {
    if (!c) return PGA_EINVAL;
    DevCall d{c, "pga_sketch_proteins"};
    if (!batch || !o || n_genes < 0 || (n_genes > 0 && !genes)) return d.bad("bad arguments");
    const pga_batch_view bv = pga_batch_peek(batch);
    if (bv.ctx != c) return d.bad("the batch belongs to another context");
    // ---- validation: all of it on the host, before anything is allocated or launched ----
    if (o->unit != PGA_SKETCH_PROTEIN && o->unit != PGA_SKETCH_GENE) return d.bad("unit must be PGA_SKETCH_PROTEIN or PGA_SKETCH_GENE, not " + std::to_string(o->unit));
    const bool protein = o->unit == PGA_SKETCH_PROTEIN;
    const int kmax = protein ? 8 : 32;
    if (o->k < 1 || o->k > kmax) return d.bad("k = " + std::to_string(o->k) + " is outside 1 .. " + std::to_string(kmax) + " for this unit");
    if (o->size < 1 || o->size > 64) return d.bad("size = " + std::to_string(o->size) + " is outside 1 .. 64");
    if (o->unknown_residue <= 0 || o->unknown_residue > 127) return d.bad("`unknown_residue` must be a single ASCII character");
    if (n_genes > INT32_MAX) return d.bad("more than 2^31 - 1 gene records");
    if (protein && n_genes > 0) {
        if (!table_of_contig) return d.bad("table_of_contig is NULL");
        if (const int rc = d.tables_known(bv, table_of_contig)) return rc;
    }
    for (int64_t g = 0; g < n_genes; g++) if (const int rc = d.record_inside(bv, genes[g], g)) return rc;
    c->sketch_passes = -1;
    if (n_genes == 0) return PGA_OK;
    if (const int rc = d.destinations({{"d_sketch", d_sketch, 8, d.kRequired}, {"d_count", d_count, 8, d.kRequired}, {"d_windows", d_windows, 8, d.kOptional}})) return rc;
    if (protein) { const int rc = tables_ready(c); if (rc) return rc; }
    // ---- the lease: the records as the kernel reads them, and behind them the class table and a counter ----
    Staging tab(256);
    const size_t p_row = tab.take(sizeof(GrpRow) * (size_t)n_genes), p_cls = tab.put(o->classes, 128), p_small = tab.take(256);
    if (const int rc = tab.lease(c)) return rc;
    grp_rows(tab.pin<GrpRow>(p_row), genes, n_genes, bv, protein, o->include_stop, table_of_contig);
    memset(tab.pin<char>(p_cls) + 128, 0, p_small + 256 - (p_cls + 128));       // (the rest of the table's slice, and the counter)
    SkArgs a{};
    a.g.seq = bv.d_seq; a.g.row = tab.dev<const GrpRow>(p_row); a.g.n = n_genes; a.g.unk = o->unknown_residue; a.g.strict = o->strict;
    a.classes = tab.dev<const uint8_t>(p_cls);
    a.k = o->k; a.s = o->size; a.bits = protein ? 8 : 2;
    a.salt = ((uint64_t)o->seed + 1ull) * 0x9E3779B97F4A7C15ull;
    a.d_sketch = d_sketch; a.d_count = d_count; a.d_windows = d_windows;
#ifdef PGA_SKETCH_COUNT_PASSES
    a.passed = tab.dev<unsigned long long>(p_small);
#endif
    return d.run(tab.L, tab.bytes(), stream, [&](hipStream_t st) {
        // a wave per record, and several rounds of them per wave where there are many
        const int64_t per_block = kRowThreads / 64;
        const dim3 grid((unsigned)std::min<int64_t>((n_genes + per_block - 1) / per_block, 16384)), block(kRowThreads);
        if (protein) hipLaunchKernelGGL((k_sketch<kGrpProtein>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((k_sketch<kGrpGene>), grid, block, 0, st, a);
        hipError_t e = hipGetLastError();
#ifdef PGA_SKETCH_COUNT_PASSES
        if (e == hipSuccess) e = hipMemcpyAsync(tab.pin<char>(p_small), tab.dev<char>(p_small), 8, hipMemcpyDeviceToHost, st);
#endif
        return e;
    }, [&] {
#ifdef PGA_SKETCH_COUNT_PASSES
        c->sketch_passes = *tab.pin<volatile long long>(p_small);
#endif
    });
}

extern "C" int pga_sketch_pairs(pga_ctx* c, const int64_t* d_sketch, const int64_t* d_count, int64_t n_genes, int32_t size,
                                const int64_t* d_pairs, int64_t n_pairs, int64_t* d_shared, int64_t* d_union, void* stream) {
    if (!c) return PGA_EINVAL;
    DevCall d{c, "pga_sketch_pairs"};
    // ---- validation: all of it on the host, before anything is launched ----
    if (n_genes < 0 || n_pairs < 0) return d.bad("bad arguments");
    if (size < 1 || size > 64) return d.bad("size = " + std::to_string(size) + " is outside 1 .. 64");
    if (n_genes > INT32_MAX) return d.bad("more than 2^31 - 1 gene records");
    if (n_pairs == 0) return PGA_OK;
    const int rows_read = n_genes > 0 ? d.kRequired : d.kUnread;
    if (const int rc = d.destinations({{"d_sketch", d_sketch, 8, rows_read}, {"d_count", d_count, 8, rows_read}, {"d_pairs", d_pairs, 8, d.kRequired},
                                       {"d_shared", d_shared, 8, d.kRequired}, {"d_union", d_union, 8, d.kRequired}})) return rc;
    SkPairArgs a{};
    a.sketch = d_sketch; a.count = d_count; a.pairs = d_pairs; a.n_genes = n_genes; a.n_pairs = n_pairs; a.s = size;
    a.d_shared = d_shared; a.d_union = d_union;
    Staging tab;                                                 // (no tables to send)
    if (const int rc = tab.lease(c)) return rc;
    return d.run(tab.L, 0, stream, [&](hipStream_t st) {
        const int64_t per_block = kRowThreads / 64;
        const dim3 grid((unsigned)std::min<int64_t>((n_pairs + per_block - 1) / per_block, 16384)), block(kRowThreads);
        hipLaunchKernelGGL(k_sketch_pairs, grid, block, 0, st, a);
        return hipGetLastError();
    });
}

// ---- clusters of near-identical proteins (protein_clusters.inl) ----------------------------------------------------------------
void pga_cluster_release(pga_ctx* c) {
    if (c->cluster_dev) hipFree(c->cluster_dev);
    c->cluster_dev = nullptr; c->cluster_cap = 0;
}

// the context's block, grown to at least `bytes`, for a call that holds the upload lease: the lease goes back when there is no memory
static int pga_cluster_block(pga_ctx* c, const char* fn, const size_t bytes) {
    if (c->cluster_cap >= bytes) return PGA_OK;
    pga_cluster_release(c);
    const size_t want = bytes + bytes / 4 + 4096;
    if (hipMalloc((void**)&c->cluster_dev, want) != hipSuccess) {
        (void)hipGetLastError();
        c->cluster_dev = nullptr;
        pga_upload_lease_give(c);
        c->err = std::string(fn) + ": no device memory for " + std::to_string(want) + " bytes of work arrays";
        return PGA_ENOMEM;
    }
    c->cluster_cap = want;
    return PGA_OK;
}

extern "C" int pga_cluster_stats(pga_ctx* c, int64_t out[4]) {
    if (!c || !out) return PGA_EINVAL;
    memcpy(out, c->cluster_stats, sizeof c->cluster_stats);
    return PGA_OK;
}

extern "C" int pga_cluster_sketches(pga_ctx* c, const int64_t* d_sketch, const int64_t* d_count, const int64_t* d_weight, int64_t n,
                                    const pga_cluster_opts* o, int64_t* d_cluster, int64_t* d_representative, int64_t* d_size, int64_t capacity,
                                    int64_t* d_edges, int64_t* d_edge_shared, int64_t* d_edge_union, int64_t edge_capacity, void* stream,
                                    int64_t* n_clusters, int64_t* n_edges) {
    if (!c) return PGA_EINVAL;
    DevCall d{c, "pga_cluster_sketches"};
    // ---- validation: all of it on the host, before anything is allocated or launched ----
    if (!o || !n_clusters || !n_edges || n < 0) return d.bad("bad arguments");
    if (o->size < 1 || o->size > 64) return d.bad("size = " + std::to_string(o->size) + " is outside 1 .. 64");
    if (o->probes < 1 || o->probes > o->size) return d.bad("probes = " + std::to_string(o->probes) + " is outside 1 .. size = " + std::to_string(o->size));
    if (o->num < 1 || o->den < o->num || o->den > (1 << 20))
        return d.bad("num / den = " + std::to_string(o->num) + " / " + std::to_string(o->den) + " is outside 1 <= num <= den <= 2^20");
    if (o->min_union < 0 || o->min_union > o->size) return d.bad("min_union = " + std::to_string(o->min_union) + " is outside 0 .. size = " + std::to_string(o->size));
    if (n > INT32_MAX) return d.bad("more than 2^31 - 1 records");
    if (n * o->probes > INT32_MAX) return d.bad("more than 2^31 - 1 probes: " + std::to_string(n) + " records of " + std::to_string(o->probes));
    if (capacity < 0 || ((d_representative || d_size) && capacity < n))
        return d.bad("capacity = " + std::to_string(capacity) + " is less than the " + std::to_string(n) + " records");
    const int n_edge_arrays = (d_edges ? 1 : 0) + (d_edge_shared ? 1 : 0) + (d_edge_union ? 1 : 0);
    if (n_edge_arrays != 0 && n_edge_arrays != 3) return d.bad("d_edges, d_edge_shared and d_edge_union are given all three or not at all");
    if (edge_capacity < 0) return d.bad("edge_capacity = " + std::to_string(edge_capacity) + " is negative");
    memset(c->cluster_stats, 0, sizeof c->cluster_stats);
    if (n == 0) { *n_clusters = 0; *n_edges = 0; return PGA_OK; }
    if (const int rc = d.destinations({{"d_sketch", d_sketch, 8, d.kRequired}, {"d_count", d_count, 8, d.kRequired}, {"d_weight", d_weight, 8, d.kOptional},
                                       {"d_cluster", d_cluster, 8, d.kRequired}, {"d_representative", d_representative, 8, d.kOptional},
                                       {"d_size", d_size, 8, d.kOptional}, {"d_edges", d_edges, 8, d.kOptional},
                                       {"d_edge_shared", d_edge_shared, 8, d.kOptional}, {"d_edge_union", d_edge_union, 8, d.kOptional}})) return rc;
    // ---- the work arrays: a block the context keeps and grows; every element that is read was written by this call ----
    const size_t G = (size_t)n, T = G * (size_t)o->probes;
    const int iG = (int)n, iT = (int)T;
    int pair_bits = 33;                                          // 32 + the bits of G: the key behind every pair is G << 32
    while (pair_bits < 63 && (G >> (pair_bits - 32)) != 0) pair_bits++;
    size_t sort_b = 0, keys_b = 0, max_b = 0, sum_b = 0, sum_g = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, sort_b, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, iT, 0, 64, (hipStream_t)nullptr);
    hipcub::DeviceRadixSort::SortKeys(nullptr, keys_b, (uint64_t*)nullptr, (uint64_t*)nullptr, iT, 0, pair_bits, (hipStream_t)nullptr);
    hipcub::DeviceScan::InclusiveScan(nullptr, max_b, (uint32_t*)nullptr, (uint32_t*)nullptr, GrpMax{}, iT, (hipStream_t)nullptr);
    hipcub::DeviceScan::ExclusiveSum(nullptr, sum_b, (uint32_t*)nullptr, (uint32_t*)nullptr, iT, (hipStream_t)nullptr);
    hipcub::DeviceScan::ExclusiveSum(nullptr, sum_g, (int32_t*)nullptr, (int32_t*)nullptr, iG, (hipStream_t)nullptr);
    const size_t tmp_b = std::max(std::max(sort_b, keys_b), std::max(max_b, std::max(sum_b, sum_g)));
    Staging work(256);                                           // (only its offsets: the block is the context's own)
    const size_t p_key = work.take(8 * T), p_skey = work.take(8 * T), p_wmax = work.take(8 * T), p_idx = work.take(4 * T), p_sidx = work.take(4 * T);
    const size_t p_start = work.take(4 * T), p_runstart = work.take(4 * T), p_centre = work.take(4 * T);
    const size_t p_rw = work.take(8 * G), p_parent = work.take(4 * G), p_root = work.take(4 * G), p_isroot = work.take(4 * G), p_number = work.take(4 * G);
    const size_t p_cnt = work.take(4 * G), p_rep = work.take(4 * G), p_tmp = work.take(tmp_b + 1);
    Staging tab(256);
    const size_t p_small = tab.take(256);
    if (const int rc = tab.lease(c)) return rc;                  // (one such call at a time per context from here on)
    if (const int rc = pga_cluster_block(c, "pga_cluster_sketches", work.bytes())) return rc;
    char* const W = c->cluster_dev;
    volatile long long* const h_small = tab.pin<volatile long long>(p_small);
    ClArgs a{};
    a.sketch = d_sketch; a.count = d_count; a.weight = d_weight; a.n = n; a.slots = (int64_t)T;
    a.s = o->size; a.probes = o->probes; a.num = o->num; a.den = o->den; a.min_union = o->min_union;
    a.key = (uint64_t*)(W + p_key); a.skey = (uint64_t*)(W + p_skey); a.idx = (uint32_t*)(W + p_idx); a.sidx = (uint32_t*)(W + p_sidx);
    a.start = (uint32_t*)(W + p_start); a.runstart = (uint32_t*)(W + p_runstart);
    a.wmax = (unsigned long long*)(W + p_wmax); a.centre = (uint32_t*)(W + p_centre);
    a.parent = (int32_t*)(W + p_parent); a.root = (int32_t*)(W + p_root); a.isroot = (int32_t*)(W + p_isroot); a.number = (int32_t*)(W + p_number);
    a.cnt = (int32_t*)(W + p_cnt); a.rw = (unsigned long long*)(W + p_rw); a.rep = (uint32_t*)(W + p_rep);
    a.small = tab.dev<unsigned long long>(p_small);
    a.d_cluster = d_cluster; a.d_rep = d_representative; a.d_size = d_size;
    a.d_edges = d_edges; a.d_eshared = d_edge_shared; a.d_eunion = d_edge_union; a.edge_capacity = edge_capacity;
    void* const d_tmp = W + p_tmp;
    const dim3 block(kRowThreads), per_slot((unsigned)((T + kRowThreads - 1) / kRowThreads)), per_rec((unsigned)((G + kRowThreads - 1) / kRowThreads));
    auto launched = [&]() { return hipGetLastError(); };
    return d.run(tab.L, 0, stream, [&](hipStream_t st) {
        size_t tb = tmp_b;
        hipError_t e = hipMemsetAsync(a.small, 0, 32, st);
        if (e == hipSuccess) { hipLaunchKernelGGL(k_cluster_probes, dim3(std::min(per_slot.x, 2048u)), block, 0, st, a); e = launched(); }
        if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(d_tmp, tb, (const uint64_t*)a.key, a.skey, (const uint32_t*)a.idx, a.sidx, iT, 0, 64, st);
        if (e == hipSuccess) { hipLaunchKernelGGL(k_cluster_heads, per_slot, block, 0, st, a); e = launched(); }
        tb = tmp_b;
        if (e == hipSuccess) e = hipcub::DeviceScan::InclusiveScan(d_tmp, tb, (const uint32_t*)a.start, a.runstart, GrpMax{}, iT, st);
        if (e == hipSuccess) e = hipMemsetAsync(a.centre, 0xff, 4 * T, st);
        if (e == hipSuccess && d_weight) {
            e = hipMemsetAsync(a.wmax, 0, 8 * T, st);
            if (e == hipSuccess) { hipLaunchKernelGGL(k_cluster_centre<0>, per_slot, block, 0, st, a); e = launched(); }
        }
        if (e == hipSuccess) { hipLaunchKernelGGL(k_cluster_centre<1>, per_slot, block, 0, st, a); e = launched(); }
        if (e == hipSuccess) { hipLaunchKernelGGL(k_cluster_pairs, per_slot, block, 0, st, a); e = launched(); }
        tb = tmp_b;
        if (e == hipSuccess) e = hipcub::DeviceRadixSort::SortKeys(d_tmp, tb, (const uint64_t*)a.key, a.skey, iT, 0, pair_bits, st);
        if (e == hipSuccess) {
            // a wave per 64 slots, and several rounds of them per wave where there are many: 2 048 workgroups fill the device
            const int64_t steps = ((int64_t)T + 63) / 64, per_block = kRowThreads / 64;
            const dim3 grid((unsigned)std::min<int64_t>((steps + per_block - 1) / per_block, 2048));
            hipLaunchKernelGGL(k_cluster_accept, grid, block, 0, st, a);
            e = launched();
        }
        tb = tmp_b;
        if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, (const uint32_t*)a.start, a.runstart, iT, st);
        if (e == hipSuccess) { hipLaunchKernelGGL(k_cluster_edges, per_slot, block, 0, st, a); e = launched(); }
        if (e == hipSuccess) { hipLaunchKernelGGL(k_cluster_flatten, per_rec, block, 0, st, a); e = launched(); }
        tb = tmp_b;
        if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, (const int32_t*)a.isroot, a.number, iG, st);
        if (e == hipSuccess) { hipLaunchKernelGGL(k_cluster_number, per_rec, block, 0, st, a); e = launched(); }
        if (e == hipSuccess && d_representative) { hipLaunchKernelGGL(k_cluster_representative, per_rec, block, 0, st, a); e = launched(); }
        if (e == hipSuccess && (d_representative || d_size)) { hipLaunchKernelGGL(k_cluster_emit, per_rec, block, 0, st, a); e = launched(); }
        if (e == hipSuccess) e = hipMemcpyAsync((void*)h_small, a.small, 32, hipMemcpyDeviceToHost, st);
        return e;
    }, [&] {
        *n_edges = h_small[0]; *n_clusters = h_small[1];
        c->cluster_stats[0] = h_small[3]; c->cluster_stats[1] = h_small[2]; c->cluster_stats[2] = h_small[0]; c->cluster_stats[3] = h_small[1];
    });
}

// ---- edges verified by edit distance, and the components of a caller's edges (protein_alignments.inl) ---------------------------
extern "C" int pga_align_stats(pga_ctx* c, int64_t out[4]) {
    if (!c || !out) return PGA_EINVAL;
    memcpy(out, c->align_stats, sizeof c->align_stats);
    return PGA_OK;
}

extern "C" int pga_align_pairs(pga_ctx* c, const void* d_tokens, int64_t n_elems, const int64_t* row_begin, const int64_t* row_len, int64_t n_rows,
                               const int64_t* d_pairs, int64_t n_pairs, const pga_align_opts* o, int64_t* d_distance, int64_t* d_pass, void* stream) {
    if (!c) return PGA_EINVAL;
    DevCall d{c, "pga_align_pairs"};
    // ---- validation: all of it on the host, before anything is allocated or launched ----
    if (!o || n_elems < 0 || n_rows < 0 || n_pairs < 0 || (n_rows > 0 && (!row_begin || !row_len))) return d.bad("bad arguments");
    const int eb = o->elem_bytes;
    if (eb != 1 && eb != 4 && eb != 8) return d.bad("elem_bytes must be 1, 4 or 8, not " + std::to_string(eb));
    if (o->max_distance < 0 || o->max_distance > 255) return d.bad("max_distance = " + std::to_string(o->max_distance) + " is outside 0 .. 255");
    if (o->num < 1 || o->den < o->num || o->den > (1 << 20))
        return d.bad("num / den = " + std::to_string(o->num) + " / " + std::to_string(o->den) + " is outside 1 <= num <= den <= 2^20");
    if (n_rows > INT32_MAX) return d.bad("more than 2^31 - 1 rows");
    if (n_pairs > INT32_MAX) return d.bad("more than 2^31 - 1 pairs");
    bool any_elem = false;
    for (int64_t g = 0; g < n_rows; g++) {
        const int64_t b = row_begin[g], n = row_len[g];
        if (n < 0 || n > ((int64_t)1 << 30)) return d.bad("row " + std::to_string(g) + " has length " + std::to_string(n) + ", outside 0 .. 2^30");
        if (b < 0 || b > n_elems - n)
            return d.bad("row " + std::to_string(g) + " is elements " + std::to_string(b) + " .. " + std::to_string(b) + " + " + std::to_string(n) +
                         ", outside the " + std::to_string(n_elems) + " of the tensor");
        any_elem |= n > 0;
    }
    memset(c->align_stats, 0, sizeof c->align_stats);
    if (n_pairs == 0) return PGA_OK;
    if (const int rc = d.destinations({{"d_tokens", d_tokens, eb, any_elem ? d.kRequired : d.kUnread}, {"d_pairs", d_pairs, 8, d.kRequired},
                                       {"d_distance", d_distance, 8, d.kRequired}, {"d_pass", d_pass, 8, d.kOptional}})) return rc;
    // ---- the lease: the rows' offsets and lengths, and behind them the counters ----
    const size_t G = (size_t)n_rows;
    Staging tab(256);
    const size_t p_beg = tab.put(row_begin, sizeof(int64_t) * G), p_len = tab.put(row_len, sizeof(int64_t) * G), p_small = tab.take(256);
    if (const int rc = tab.lease(c)) return rc;
    memset(tab.pin<char>(p_small), 0, 256);
    volatile long long* const h_small = tab.pin<volatile long long>(p_small);
    AlArgs a{};
    a.tokens = d_tokens; a.begin = tab.dev<const int64_t>(p_beg); a.len = tab.dev<const int64_t>(p_len);
    a.pairs = d_pairs; a.n_rows = n_rows; a.n_pairs = n_pairs;
    a.K = o->max_distance; a.num = o->num; a.den = o->den;
    a.d_distance = d_distance; a.d_pass = d_pass;
    a.small = tab.dev<unsigned long long>(p_small);
    // a lane holds R diagonals of the band's 2 K + 1: the least R of 1, 2, 4, 8 with 64 R of them or more
    const int R = a.K <= 31 ? 1 : a.K <= 63 ? 2 : a.K <= 127 ? 4 : 8;
    return d.run(tab.L, tab.bytes(), stream, [&](hipStream_t st) {
        const int64_t per_block = kRowThreads / 64;
        const dim3 grid((unsigned)std::min<int64_t>((n_pairs + per_block - 1) / per_block, 16384)), block(kRowThreads);
        auto launch = [&](auto EB) {
            constexpr int E = decltype(EB)::value;
            if (R == 1) hipLaunchKernelGGL((k_align_pairs<E, 1>), grid, block, 0, st, a);
            else if (R == 2) hipLaunchKernelGGL((k_align_pairs<E, 2>), grid, block, 0, st, a);
            else if (R == 4) hipLaunchKernelGGL((k_align_pairs<E, 4>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((k_align_pairs<E, 8>), grid, block, 0, st, a);
        };
        if (eb == 1) launch(std::integral_constant<int, 1>{});
        else if (eb == 4) launch(std::integral_constant<int, 4>{});
        else launch(std::integral_constant<int, 8>{});
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync((void*)h_small, a.small, 32, hipMemcpyDeviceToHost, st);
        return e;
    }, [&] {
        c->align_stats[0] = n_pairs; c->align_stats[1] = h_small[0]; c->align_stats[2] = h_small[1]; c->align_stats[3] = h_small[2];
    });
}

extern "C" int pga_cluster_edges(pga_ctx* c, const int64_t* d_edges, const int64_t* d_keep, int64_t n_edges, int64_t n, const int64_t* d_weight,
                                 int64_t* d_cluster, int64_t* d_representative, int64_t* d_size, int64_t capacity, void* stream,
                                 int64_t* n_clusters, int64_t* n_used) {
    if (!c) return PGA_EINVAL;
    DevCall d{c, "pga_cluster_edges"};
    // ---- validation: all of it on the host, before anything is allocated or launched ----
    if (!n_clusters || !n_used || n < 0 || n_edges < 0) return d.bad("bad arguments");
    if (n > INT32_MAX) return d.bad("more than 2^31 - 1 records");
    if (n_edges > INT32_MAX) return d.bad("more than 2^31 - 1 edges");
    if (capacity < 0 || ((d_representative || d_size) && capacity < n))
        return d.bad("capacity = " + std::to_string(capacity) + " is less than the " + std::to_string(n) + " records");
    if (n == 0) { *n_clusters = 0; *n_used = 0; return PGA_OK; }
    if (const int rc = d.destinations({{"d_edges", d_edges, 8, n_edges > 0 ? d.kRequired : d.kUnread}, {"d_keep", d_keep, 8, n_edges > 0 ? d.kOptional : d.kUnread},
                                       {"d_weight", d_weight, 8, d.kOptional}, {"d_cluster", d_cluster, 8, d.kRequired},
                                       {"d_representative", d_representative, 8, d.kOptional}, {"d_size", d_size, 8, d.kOptional}})) return rc;
    // ---- the work arrays: the per-record part of pga_cluster_sketches' block; every element that is read was written by this call ----
    const size_t G = (size_t)n;
    const int iG = (int)n;
    size_t tmp_b = 0;
    hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_b, (int32_t*)nullptr, (int32_t*)nullptr, iG, (hipStream_t)nullptr);
    Staging work(256);                                           // (only its offsets: the block is the context's own)
    const size_t p_rw = work.take(8 * G), p_parent = work.take(4 * G), p_root = work.take(4 * G), p_isroot = work.take(4 * G), p_number = work.take(4 * G);
    const size_t p_cnt = work.take(4 * G), p_rep = work.take(4 * G), p_tmp = work.take(tmp_b + 1);
    Staging tab(256);
    const size_t p_small = tab.take(256);
    if (const int rc = tab.lease(c)) return rc;                  // (one such call at a time per context from here on)
    if (const int rc = pga_cluster_block(c, "pga_cluster_edges", work.bytes())) return rc;
    char* const W = c->cluster_dev;
    memset(tab.pin<char>(p_small), 0, 256);
    volatile long long* const h_small = tab.pin<volatile long long>(p_small);
    ClArgs a{};
    a.weight = d_weight; a.n = n;
    a.parent = (int32_t*)(W + p_parent); a.root = (int32_t*)(W + p_root); a.isroot = (int32_t*)(W + p_isroot); a.number = (int32_t*)(W + p_number);
    a.cnt = (int32_t*)(W + p_cnt); a.rw = (unsigned long long*)(W + p_rw); a.rep = (uint32_t*)(W + p_rep);
    a.small = tab.dev<unsigned long long>(p_small);
    a.d_cluster = d_cluster; a.d_rep = d_representative; a.d_size = d_size;
    void* const d_tmp = W + p_tmp;
    const dim3 block(kRowThreads), per_rec((unsigned)((G + kRowThreads - 1) / kRowThreads));
    auto launched = [&]() { return hipGetLastError(); };
    return d.run(tab.L, tab.bytes(), stream, [&](hipStream_t st) {
        size_t tb = tmp_b;
        hipError_t e = hipSuccess;
        hipLaunchKernelGGL(k_edges_reset, per_rec, block, 0, st, a); e = launched();
        if (e == hipSuccess && n_edges > 0) {
            const dim3 grid((unsigned)std::min<int64_t>((n_edges + kRowThreads - 1) / kRowThreads, 2048));
            hipLaunchKernelGGL(k_edges_join, grid, block, 0, st, a, d_edges, d_keep, n_edges);
            e = launched();
        }
        if (e == hipSuccess) { hipLaunchKernelGGL(k_cluster_flatten, per_rec, block, 0, st, a); e = launched(); }
        if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(d_tmp, tb, (const int32_t*)a.isroot, a.number, iG, st);
        if (e == hipSuccess) { hipLaunchKernelGGL(k_cluster_number, per_rec, block, 0, st, a); e = launched(); }
        if (e == hipSuccess && d_representative) { hipLaunchKernelGGL(k_cluster_representative, per_rec, block, 0, st, a); e = launched(); }
        if (e == hipSuccess && (d_representative || d_size)) { hipLaunchKernelGGL(k_cluster_emit, per_rec, block, 0, st, a); e = launched(); }
        if (e == hipSuccess) e = hipMemcpyAsync((void*)h_small, a.small, 32, hipMemcpyDeviceToHost, st);
        return e;
    }, [&] {
        *n_used = h_small[0]; *n_clusters = h_small[1];
    });
}

// ---- start candidates (start_candidates.inl) ----------------------------------------------------------------------------------
struct pga_start_plan {
    pga_ctx* ctx = nullptr;
    uint64_t serial = 0;                 // DevNodes::serial of the record the plan was made on
    const void* batch = nullptr;
    int64_t n_genes = 0, total = 0;      // T = sum n_g
    int64_t longest = 0, longest_g = -1;
    char* dev = nullptr; size_t cap = 0; // the context's block while the plan lives
    const uint32_t* sval = nullptr; const int2* grp = nullptr; const int64_t* off = nullptr;
    std::vector<int64_t> h_off;          // the scan of n_g, and the arena offset of every record's contig: pga_start_plan_nodes
    std::vector<int64_t> h_aoff;
};

// pga_destroy: the blocks go, and a plan that is still alive is orphaned -- it can only be freed
void pga_start_release(pga_ctx* c) {
    for (auto& b : c->start_blocks) if (b.first) hipFree(b.first);
    c->start_blocks.clear();
    for (pga_start_plan* p : c->start_plans) { if (p->dev) hipFree(p->dev); p->dev = nullptr; p->cap = 0; p->ctx = nullptr; }
    c->start_plans.clear();
}

// a block of at least `need` bytes from the ones freed plans gave back: the smallest that fits, else a new one in the place of the largest
static hipError_t start_block_take(pga_ctx* c, const size_t need, char** p, size_t* cap) {
    auto& B = c->start_blocks;
    int best = -1, largest = -1;
    for (int k = 0; k < (int)B.size(); k++) {
        if (B[k].second >= need && (best < 0 || B[k].second < B[best].second)) best = k;
        if (largest < 0 || B[k].second > B[largest].second) largest = k;
    }
    if (best >= 0) { *p = B[best].first; *cap = B[best].second; B.erase(B.begin() + best); return hipSuccess; }
    if (largest >= 0) { (void)hipFree(B[largest].first); B.erase(B.begin() + largest); }
    const size_t want = need + need / 4 + 4096;
    const hipError_t e = hipMalloc((void**)p, want);
    *cap = e == hipSuccess ? want : 0;
    return e;
}

extern "C" void pga_start_plan_free(pga_ctx* c, pga_start_plan* p) {
    if (!p) return;
    (void)c;                             // (the plan knows its context, and whether it still exists)
    if (p->ctx) {
        auto& live = p->ctx->start_plans;
        live.erase(std::remove(live.begin(), live.end(), p), live.end());
        if (p->dev) p->ctx->start_blocks.emplace_back(p->dev, p->cap);
    }
    delete p;
}

extern "C" int pga_start_plan_create(pga_ctx* c, const pga_batch* batch, int64_t n_genes, const pga_gene* genes, pga_start_plan** plan,
                                     int32_t* count_out, int32_t* chosen_out) {
    if (plan) *plan = nullptr;
    if (!c) return PGA_EINVAL;
    DevCall d{c, "pga_start_plan_create"};
    if (!batch || !plan || n_genes < 0 || (n_genes > 0 && (!genes || !count_out || !chosen_out))) return d.bad("bad arguments");
    const pga_batch_view bv = pga_batch_peek(batch);
    if (bv.ctx != c) return d.bad("the batch belongs to another context");
    // ---- validation on the host, before anything is allocated or launched ----
    if (bv.circular) return d.bad("the start-score file is not written for circular contigs (the batch carries pga_batch_set_circular flags)");
    if (const char* why = pga_dev_nodes_refusal(c, batch, bv.n, bv.ct, nullptr)) return d.bad(why);
    const DevNodes& DN = c->dev_nodes;
    const int NC = bv.n;
    std::vector<StartReq> req((size_t)n_genes);
    for (int64_t g = 0; g < n_genes; g++) {
        const pga_gene& G = genes[g];
        auto who = [g] { return "gene " + std::to_string(g); };      // (only a refusal needs the words)
        if (const int rc = d.contig_known(bv, G, g)) return rc;
        const int32_t n = DN.n[G.contig];
        if (G.start_ndx < 0 || G.start_ndx >= n) return d.bad(who() + ": start_ndx = " + std::to_string(G.start_ndx) + " lies outside the " + std::to_string(n) + " nodes of contig " + std::to_string(G.contig));
        if (G.stop_ndx < 0 || G.stop_ndx >= n) return d.bad(who() + ": stop_ndx = " + std::to_string(G.stop_ndx) + " lies outside the " + std::to_string(n) + " nodes of contig " + std::to_string(G.contig));
        if (G.strand != 1 && G.strand != -1) return d.bad(who() + ": strand = " + std::to_string((int)G.strand) + " is neither 1 nor -1");
        req[(size_t)g] = StartReq{G.contig, (int32_t)(DN.off[G.contig] + G.start_ndx), G.strand == 1 ? G.begin : G.end, G.strand};
    }
    pga_start_plan* P = new (std::nothrow) pga_start_plan();
    if (!P) return PGA_ENOMEM;
    P->ctx = c; P->serial = DN.serial; P->batch = batch; P->n_genes = n_genes;
    P->h_off.assign((size_t)n_genes + 1, 0); P->h_aoff.resize((size_t)n_genes);
    for (int64_t g = 0; g < n_genes; g++) P->h_aoff[(size_t)g] = DN.off[genes[g].contig];
    c->start_plans.push_back(P);
    if (n_genes == 0) { *plan = P; return PGA_OK; }
    if (hipSetDevice(c->device) != hipSuccess) { pga_start_plan_free(c, P); return PGA_EDEVICE; }
    // ---- the plan's block (what the write step reads) and the scratch of this call (the renderer's) ----
    const int64_t NN = std::accumulate(DN.n.begin(), DN.n.end(), (int64_t)0);      // > 0: a record named a node
    const size_t G = (size_t)n_genes, nn = (size_t)NN;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t p_off = 0, p_grp = p_off + al(sizeof(int64_t) * (G + 1)), p_sval = p_grp + al(sizeof(int2) * G), p_end = p_sval + al(sizeof(uint32_t) * nn);
    hipStream_t st = c->stream;
    const size_t tmp_b = pga_node_order_temp_bytes(NN, NC, st);
    const size_t s_naoff = 0, s_ncum = s_naoff + al(sizeof(int64_t) * (NC + 1)), s_srow = s_ncum + al(sizeof(int64_t) * (NC + 1));
    const size_t s_req = s_srow + al(sizeof(int64_t) * (NC + 1)), s_res = s_req + al(sizeof(StartReq) * G), s_skey = s_res + al(sizeof(int2) * G);
    const size_t s_skey2 = s_skey + al(sizeof(uint64_t) * nn), s_sval = s_skey2 + al(sizeof(uint64_t) * nn), s_tmp = s_sval + al(sizeof(uint32_t) * nn);
    const size_t s_end = s_tmp + al(tmp_b + 1);
    char* s = nullptr;
    hipError_t e = start_block_take(c, p_end, &P->dev, &P->cap);
    if (e == hipSuccess) e = pga_render_scratch(c, s_end, &s);
    auto fail = [&](const hipError_t err) {
        hipStreamSynchronize(st);
        pga_start_plan_free(c, P);
        return pga_hip_try_(c, err, d.fn);
    };
    if (e != hipSuccess) return fail(e);
    std::vector<int64_t> naoff((size_t)NC + 1, 0), ncum((size_t)NC + 1, 0);
    for (int i = 0; i < NC; i++) { naoff[i] = DN.off[i]; ncum[i + 1] = ncum[i] + DN.n[i]; }
    e = hipMemcpyAsync(s + s_naoff, naoff.data(), sizeof(int64_t) * (NC + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s + s_ncum, ncum.data(), sizeof(int64_t) * (NC + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(s + s_req, req.data(), sizeof(StartReq) * G, hipMemcpyHostToDevice, st);
    NodeOrder no{DN.a, (const int64_t*)(s + s_naoff), (const int64_t*)(s + s_ncum), (uint64_t*)(s + s_skey), (uint32_t*)(s + s_sval),
                 (uint64_t*)(s + s_skey2), (uint32_t*)(P->dev + p_sval), (int64_t*)(s + s_srow), NN, NC};
    if (e == hipSuccess) e = pga_node_order(no, s + s_tmp, tmp_b, st);
    std::vector<int2> res(G);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_start_lookup, dim3((unsigned)((n_genes + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0, st, DN.a,
                           (const uint64_t*)no.skey, (const uint32_t*)no.sval, (const int64_t*)no.srow, NC, (const StartReq*)(s + s_req), n_genes,
                           (int2*)(P->dev + p_grp), (int2*)(s + s_res));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(res.data(), s + s_res, sizeof(int2) * G, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(e);
    // ---- what the look-up found: the three checks that read the arena, the counts, their scan ----
    std::vector<int64_t>& off = P->h_off;
    for (size_t g = 0; g < G; g++) {
        const pga_gene& R = genes[g];
        auto who = [g] { return "gene " + std::to_string(g); };
        if (res[g].x <= 0) {
            pga_start_plan_free(c, P);
            switch (-res[g].x) {
                case kStartIsStop:   return d.bad(who() + ": start_ndx = " + std::to_string(R.start_ndx) + " is a stop node of contig " + std::to_string(R.contig));
                case kStartStrand:   return d.bad(who() + ": strand = " + std::to_string((int)R.strand) + " is not the strand of node start_ndx = " + std::to_string(R.start_ndx));
                case kStartPosition: return d.bad(who() + ": " + (R.strand == 1 ? "begin = " + std::to_string(R.begin) : "end = " + std::to_string(R.end)) +
                                                " is not ndx + 1 of node start_ndx = " + std::to_string(R.start_ndx));
                default:             return d.bad(who() + ": node start_ndx = " + std::to_string(R.start_ndx) + " was not found in the sorted arena");
            }
        }
        count_out[g] = res[g].x; chosen_out[g] = res[g].y;
        off[g + 1] = off[g] + res[g].x;
        if (res[g].x > P->longest) { P->longest = res[g].x; P->longest_g = (int64_t)g; }
    }
    e = hipMemcpyAsync(P->dev + p_off, off.data(), sizeof(int64_t) * (G + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(e);
    P->total = off[G];
    P->off = (const int64_t*)(P->dev + p_off); P->grp = (const int2*)(P->dev + p_grp); P->sval = (const uint32_t*)(P->dev + p_sval);
    *plan = P;
    return PGA_OK;
}

extern "C" int pga_start_plan_write(pga_ctx* c, const pga_start_plan* P, const pga_start_opts* o, void* d_positions, void* d_types, void* d_scores,
                                    int64_t n_positions, int64_t n_types, int64_t n_scores, void* stream) {
    if (!c) return PGA_EINVAL;
    DevCall d{c, "pga_start_plan_write"};
    if (!P || !o || n_positions < 0 || n_types < 0 || n_scores < 0) return d.bad("bad arguments");
    if (P->ctx != c) return d.bad("the plan belongs to another context");
    // ---- validation: all of it on the host, before anything is launched ----
    if (o->index_bytes != 4 && o->index_bytes != 8) return d.bad("index_bytes must be 4 or 8, not " + std::to_string(o->index_bytes));
    if (o->score_bytes != 4 && o->score_bytes != 8) return d.bad("score_bytes must be 4 or 8, not " + std::to_string(o->score_bytes));
    if (o->layout != PGA_TOKENS_RAGGED && o->layout != PGA_TOKENS_PADDED) return d.bad("layout must be PGA_TOKENS_RAGGED or PGA_TOKENS_PADDED, not " + std::to_string(o->layout));
    const bool padded = o->layout == PGA_TOKENS_PADDED;
    if (o->n_fields < 1 || o->n_fields > 7) return d.bad("n_fields must be 1 .. 7, not " + std::to_string(o->n_fields));
    for (int k = 0; k < o->n_fields; k++) {
        if (o->fields[k] < PGA_START_TOTAL || o->fields[k] > PGA_START_GC_CONT) return d.bad("fields[" + std::to_string(k) + "] = " + std::to_string(o->fields[k]) + " is no PGA_START_* field");
        for (int j = 0; j < k; j++) if (o->fields[j] == o->fields[k]) return d.bad("fields[" + std::to_string(k) + "] repeats fields[" + std::to_string(j) + "]");
    }
    if (padded) {
        if (o->index_bytes == 4 && (o->index_pad < INT32_MIN || o->index_pad > INT32_MAX)) return d.bad("index_pad = " + std::to_string(o->index_pad) + " does not fit int32");
        if (o->score_bytes == 4 && std::isfinite(o->score_pad) && std::fabs(o->score_pad) > (double)FLT_MAX) return d.bad("score_pad = " + std::to_string(o->score_pad) + " does not fit float32");
    }
    const DevNodes& DN = c->dev_nodes;
    if (!DN.contigs || DN.serial != P->serial || DN.batch != P->batch)
        return d.bad("the node arrays the plan was made on are no longer on record: a later call on the context ran the finder or loaded models");
    const int64_t G = P->n_genes, F = o->n_fields;
    int64_t W = 0, S = 0, n_layout = P->total, n_cells = P->total;
    if (padded) {
        W = o->row_width; S = o->row_stride;
        if (W < P->longest) return d.bad("row_width = " + std::to_string(W) + " is less than the " + std::to_string(P->longest) + " candidates of gene " + std::to_string(P->longest_g));
        if (W < 0 || S < W) return d.bad("row_stride = " + std::to_string(S) + " is less than row_width = " + std::to_string(W));
        if (G > 1 && S > (INT64_MAX / 64 - W) / (G - 1)) return d.bad("row_stride = " + std::to_string(S) + " is too large");
        if (G > 0 && W > 0 && W > (INT64_MAX / 64) / G) return d.bad("row_width = " + std::to_string(W) + " is too large");
        n_layout = G > 0 ? (G - 1) * S + W : 0;
        n_cells = G * W;
    }
    if (n_positions < n_layout) return d.bad("n_positions = " + std::to_string(n_positions) + " is less than the " + std::to_string(n_layout) + " elements of the layout");
    if (n_types < n_layout) return d.bad("n_types = " + std::to_string(n_types) + " is less than the " + std::to_string(n_layout) + " elements of the layout");
    if (n_scores < n_layout * F) return d.bad("n_scores = " + std::to_string(n_scores) + " is less than the " + std::to_string(n_layout * F) + " elements of the layout");
    if (n_cells == 0) return PGA_OK;
    if (const int rc = d.destinations({{"d_positions", d_positions, o->index_bytes, d.kRequired}, {"d_types", d_types, o->index_bytes, d.kRequired},
                                       {"d_scores", d_scores, o->score_bytes, d.kRequired}}, true)) return rc;
    StartArgs a{};
    a.nd = DN.a; a.sval = P->sval; a.grp = P->grp; a.off = P->off;
    a.n_genes = G; a.n_cells = n_cells; a.W = W; a.S = S;
    a.index_pad = o->index_pad; a.score_pad = o->score_pad;
    a.n_fields = o->n_fields;
    for (int k = 0; k < 7; k++) a.fields[k] = k < o->n_fields ? o->fields[k] : 0;
    a.pos = d_positions; a.typ = d_types; a.sco = d_scores;
    Staging tab;                                                 // (no tables to send)
    if (const int rc = tab.lease(c)) return rc;
    return d.run(tab.L, 0, stream, [&](hipStream_t st) {
        const dim3 grid((unsigned)((n_cells + kRowThreads - 1) / kRowThreads)), block(kRowThreads);
        auto scores = [&](auto IB, auto PADDED) {
            if (o->score_bytes == 4) hipLaunchKernelGGL((k_start_candidates<decltype(IB)::value, 4, decltype(PADDED)::value>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((k_start_candidates<decltype(IB)::value, 8, decltype(PADDED)::value>), grid, block, 0, st, a);
        };
        auto layout = [&](auto IB) { if (padded) scores(IB, std::true_type{}); else scores(IB, std::false_type{}); };
        if (o->index_bytes == 4) layout(std::integral_constant<int, 4>{}); else layout(std::integral_constant<int, 8>{});
        return hipGetLastError();
    });
}

extern "C" int pga_start_plan_nodes(pga_ctx* c, const pga_start_plan* P, int32_t* node_out, int64_t n_out) {
    if (!c) return PGA_EINVAL;
    DevCall d{c, "pga_start_plan_nodes"};
    if (!P || n_out < 0) return d.bad("bad arguments");
    if (P->ctx != c) return d.bad("the plan belongs to another context");
    if (n_out < P->total) return d.bad("n_out = " + std::to_string(n_out) + " is less than the " + std::to_string(P->total) + " candidates of the plan");
    if (P->total == 0) return PGA_OK;
    if (!node_out) return d.bad("node_out is NULL");
    if (hipSetDevice(c->device) != hipSuccess) return PGA_EDEVICE;
    char* s = nullptr;
    hipError_t e = pga_render_scratch(c, sizeof(uint32_t) * (size_t)P->total, &s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_start_nodes, dim3((unsigned)((P->total + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0, c->stream,
                           P->sval, P->grp, P->off, P->n_genes, P->total, (uint32_t*)s);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(node_out, s, sizeof(uint32_t) * (size_t)P->total, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return pga_hip_try_(c, e, d.fn);
    for (int64_t g = 0; g < P->n_genes; g++)            // arena index -> index in the contig's node arrays
        for (int64_t k = P->h_off[(size_t)g]; k < P->h_off[(size_t)g + 1]; k++) node_out[k] = (int32_t)((int64_t)(uint32_t)node_out[k] - P->h_aoff[(size_t)g]);
    return PGA_OK;
}

extern "C" int pga_device_read(pga_ctx* c, const void* d_src, int64_t bytes, void* dst, void* stream) {
    if (bytes < 0 || (bytes > 0 && (!d_src || !dst))) { if (c) c->err = "pga_device_read: bad arguments"; return PGA_EINVAL; }
    if (bytes == 0) return PGA_OK;
    if (!c) {
        // without a context (a result that outlives the call that made it): the pointer names its device, and no message is kept
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, d_src) != hipSuccess) { (void)hipGetLastError(); return PGA_EINVAL; }
        if (at.type != hipMemoryTypeDevice) return PGA_EINVAL;
        if (hipSetDevice(at.device) != hipSuccess) return PGA_EDEVICE;
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return PGA_EDEVICE;
        return hipMemcpy(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost) == hipSuccess ? PGA_OK : PGA_EDEVICE;
    }
    if (hipSetDevice(c->device) != hipSuccess) return PGA_EDEVICE;
    if (const int rc = pga_device_memory_(c, d_src, "pga_device_read", "d_src")) return rc;
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpy(dst, d_src, (size_t)bytes, hipMemcpyDeviceToHost);
    return pga_hip_try_(c, e, "pga_device_read");
}
