// Device-side translation of gene records into proteins: one thread per codon.
// ref: lib.pyx:2932-3047 (Gene.translate), 770-789 (Sequence._amino); the codes and codon rules are in translate_rules.h.
#include "pga_internal.h"
#include <mutex>
#include "pipeline.h"
#include "translate_rules.h"

#include <string.h>

#include <algorithm>
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

#include "translate_tokens.inl"
#include "label_bases.inl"

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
    // the caller's layout must be the one the kernel writes (ref: lib.pyx:3006-3018 for the lengths)
    if (offsets[0] != 0) { c->err = "pga_translate_genes: offsets[0] must be 0"; return PGA_EINVAL; }
    for (int64_t g = 0; g < n_genes; g++) {
        const pga_gene& G = genes[g];
        const bool circ = bv.circular && G.contig >= 0 && G.contig < bv.n && bv.circular[G.contig];
        const bool inside = G.contig >= 0 && G.contig < bv.n &&
                            (circ ? G.begin <= bv.ct[G.contig].len && (int64_t)G.end - G.begin < bv.ct[G.contig].len : G.end <= bv.ct[G.contig].len);
        if (!inside || G.begin < 1 || G.end < G.begin) { c->err = "pga_translate_genes: gene outside its contig"; return PGA_EINVAL; }
        const bool stop_edge = G.strand == 1 ? G.partial_end : G.partial_begin;
        const int64_t want = (G.end - G.begin + 1) / 3 - ((!stop_edge && !include_stop) ? 1 : 0);
        if (offsets[g + 1] - offsets[g] != (want > 0 ? want : 0)) { c->err = "pga_translate_genes: offsets do not match the gene lengths"; return PGA_EINVAL; }
    }
    const int64_t total = offsets[n_genes];
    if (total == 0) return PGA_OK;
    if (hipSetDevice(c->device) != hipSuccess) return PGA_EDEVICE;
    {
        std::lock_guard<std::mutex> lk(g_tables_mu);
        const int dev = c->device & 63;
        if (!g_tables_ready[dev]) { const int rc = upload_tables(); if (rc) return rc; g_tables_ready[dev] = true; }
    }
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
    auto bad = [&](std::string msg) { c->err = "pga_translate_genes_tokens: " + msg; return PGA_EINVAL; };
    if (!batch || !o || n_genes < 0 || n_out_elems < 0 || (n_genes > 0 && (!genes || !table_of_contig || !len_out))) return bad("bad arguments");
    const pga_batch_view bv = pga_batch_peek(batch);
    if (bv.ctx != c) return bad("the batch belongs to another context");
    // ---- validation: all of it on the host, before anything is allocated or launched ----
    const int eb = o->elem_bytes;
    if (eb != 1 && eb != 4 && eb != 8) return bad("elem_bytes must be 1, 4 or 8, not " + std::to_string(eb));
    if (o->layout != PGA_TOKENS_RAGGED && o->layout != PGA_TOKENS_PADDED) return bad("layout must be PGA_TOKENS_RAGGED or PGA_TOKENS_PADDED, not " + std::to_string(o->layout));
    const bool padded = o->layout == PGA_TOKENS_PADDED;
    if (o->unknown_residue <= 0 || o->unknown_residue > 127) return bad("`unknown_residue` must be a single ASCII character");
    const bool has_bos = o->bos != PGA_TOKEN_NONE, has_eos = o->eos != PGA_TOKEN_NONE;
    const int64_t s = (has_bos ? 1 : 0) + (has_eos ? 1 : 0);
    auto fits = [&](const int64_t v) { return eb == 8 || (eb == 4 ? v >= INT32_MIN && v <= INT32_MAX : v >= 0 && v <= 255); };
    const char* const elem_name = eb == 1 ? "uint8" : eb == 4 ? "int32" : "int64";
    for (int k = 0; k < 128; k++)
        if (!fits(o->vocab[k])) return bad("vocab[" + std::to_string(k) + "] = " + std::to_string(o->vocab[k]) + " does not fit " + elem_name);
    if (has_bos && !fits(o->bos)) return bad("bos = " + std::to_string(o->bos) + " does not fit " + elem_name);
    if (has_eos && !fits(o->eos)) return bad("eos = " + std::to_string(o->eos) + " does not fit " + elem_name);
    if (padded && !fits(o->pad)) return bad("pad = " + std::to_string(o->pad) + " does not fit " + elem_name);
    if (o->max_length < 0 || (o->max_length != 0 && o->max_length < s + 1))
        return bad("max_length = " + std::to_string(o->max_length) + " leaves no room for a residue beside " + std::to_string(s) + " special tokens (0: no limit)");
    for (int i = 0; i < (n_genes > 0 ? bv.n : 0); i++)
        if (!table_known(table_of_contig[i])) return bad("contig " + std::to_string(i) + ": " + std::to_string(table_of_contig[i]) + " is not a valid translation table index");
    std::vector<int64_t> off((size_t)n_genes + 1, 0);
    int64_t longest = 0, longest_g = -1;
    for (int64_t g = 0; g < n_genes; g++) {
        const pga_gene& G = genes[g];
        const bool circ = bv.circular && G.contig >= 0 && G.contig < bv.n && bv.circular[G.contig];
        const bool inside = G.contig >= 0 && G.contig < bv.n &&
                            (circ ? G.begin <= bv.ct[G.contig].len && (int64_t)G.end - G.begin < bv.ct[G.contig].len : G.end <= bv.ct[G.contig].len);
        if (!inside || G.begin < 1 || G.end < G.begin) return bad("gene " + std::to_string(g) + " lies outside its contig");
        const bool stop_edge = G.strand == 1 ? G.partial_end : G.partial_begin;
        int64_t r = ((int64_t)G.end - G.begin + 1) / 3 - ((!stop_edge && !o->include_stop) ? 1 : 0);
        if (r < 0) r = 0;
        if (o->max_length != 0 && r > o->max_length - s) r = o->max_length - s;
        off[(size_t)g + 1] = off[(size_t)g] + s + r;
        if (s + r > longest) { longest = s + r; longest_g = g; }
    }
    int64_t need = off[(size_t)n_genes];
    if (padded) {
        const int64_t W = o->row_width, S = o->row_stride;
        if (W < longest) return bad("row_width = " + std::to_string(W) + " is less than the " + std::to_string(longest) + " tokens of gene " + std::to_string(longest_g));
        if (W < 0 || S < W) return bad("row_stride = " + std::to_string(S) + " is less than row_width = " + std::to_string(W));
        if (n_genes > 1 && S > (INT64_MAX / 8 - W) / (n_genes - 1)) return bad("row_stride = " + std::to_string(S) + " is too large");
        need = n_genes > 0 ? (n_genes - 1) * S + W : 0;
    }
    if (n_out_elems < need) return bad("n_out_elems = " + std::to_string(n_out_elems) + " is less than the " + std::to_string(need) + " elements of the layout");
    if (need > 0) {
        if (!d_out) return bad("d_out is NULL");
        if ((uintptr_t)d_out % (uintptr_t)eb) return bad("d_out is not aligned to its " + std::to_string(eb) + "-byte elements");
        if (hipSetDevice(c->device) != hipSuccess) return PGA_EDEVICE;
        // the pointer is asked about, never dereferenced on the host, and never handed to a kernel unless the runtime calls it device memory
        hipPointerAttribute_t at{};
        const hipError_t pe = hipPointerGetAttributes(&at, d_out);
        if (pe != hipSuccess) (void)hipGetLastError();
        if (pe != hipSuccess || at.type != hipMemoryTypeDevice) return bad("d_out is not device memory (a host pointer?)");
        if (at.device != c->device) return bad("d_out is not device memory of the context's device " + std::to_string(c->device) + " but of device " + std::to_string(at.device));
    }
    for (int64_t g = 0; g < n_genes; g++) len_out[g] = off[(size_t)g + 1] - off[(size_t)g];
    if (need == 0) return PGA_OK;
    { const int rc = tables_ready(c); if (rc) return rc; }
    // ---- the kernel's tables: staged in the upload's pinned area as they will lie on the device, one copy ----
    const size_t G = (size_t)n_genes, n = (size_t)bv.n;
    const size_t off_b = sizeof(int64_t) * (G + 1), voc_b = sizeof(int64_t) * 128, ct_b = sizeof(ContigDesc) * (n + 1), gen_b = sizeof(pga_gene) * G, tt_b = sizeof(int32_t) * n;
    const size_t tab = off_b + voc_b + ct_b + gen_b + tt_b;
    pga_upload_lease L{};
    { const int rc = pga_upload_lease_take(c, tab, &L); if (rc) return rc; }
    memcpy(L.pin, off.data(), off_b);
    memcpy(L.pin + off_b, o->vocab, voc_b);
    memcpy(L.pin + off_b + voc_b, bv.ct, ct_b);
    memcpy(L.pin + off_b + voc_b + ct_b, genes, gen_b);
    memcpy(L.pin + off_b + voc_b + ct_b + gen_b, table_of_contig, tt_b);
    TokArgs a{};
    a.seq = bv.d_seq;
    a.off = (const int64_t*)L.dev; a.vocab = (const int64_t*)(L.dev + off_b); a.ct = (const ContigDesc*)(L.dev + off_b + voc_b);
    a.genes = (const pga_gene*)(L.dev + off_b + voc_b + ct_b); a.tt_of = (const int32_t*)(L.dev + off_b + voc_b + ct_b + gen_b);
    a.n_genes = n_genes; a.n_elems = need; a.W = padded ? o->row_width : 0; a.S = padded ? o->row_stride : 0;
    a.bos = has_bos ? o->bos : 0; a.eos = has_eos ? o->eos : 0; a.pad = padded ? o->pad : 0;
    a.has_bos = has_bos; a.has_eos = has_eos; a.unk = o->unknown_residue; a.strict = o->strict;
    a.out0 = (char*)((uintptr_t)d_out & ~(uintptr_t)15);
    a.lead = (int32_t)(((uintptr_t)d_out - (uintptr_t)a.out0) / (uintptr_t)eb);
    const int64_t per = 16 / eb, pieces = (a.lead + need + per - 1) / per;
    const dim3 grid((unsigned)((pieces + kTokThreads - 1) / kTokThreads)), block(kTokThreads);
    // the upload stream is non-blocking: it waits for what the caller's stream held when the call came
    hipError_t e = hipEventRecord(L.ev, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(L.st, L.ev, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(L.dev, L.pin, tab, hipMemcpyHostToDevice, L.st);
    if (e == hipSuccess) {
        if (padded) {
            if (eb == 1) hipLaunchKernelGGL((k_translate_tokens<1, true>), grid, block, 0, L.st, a);
            else if (eb == 4) hipLaunchKernelGGL((k_translate_tokens<4, true>), grid, block, 0, L.st, a);
            else hipLaunchKernelGGL((k_translate_tokens<8, true>), grid, block, 0, L.st, a);
        } else {
            if (eb == 1) hipLaunchKernelGGL((k_translate_tokens<1, false>), grid, block, 0, L.st, a);
            else if (eb == 4) hipLaunchKernelGGL((k_translate_tokens<4, false>), grid, block, 0, L.st, a);
            else hipLaunchKernelGGL((k_translate_tokens<8, false>), grid, block, 0, L.st, a);
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(L.st);         // on return the tensor is complete for any stream
    pga_upload_lease_give(c);
    return pga_hip_try_(c, e, "pga_translate_genes_tokens");
}

extern "C" int pga_label_bases(pga_ctx* c, const pga_batch* batch, int64_t n_genes, const pga_gene* genes, const pga_label_opts* o, void* d_out,
                               int64_t n_out_elems, void* stream, int64_t* len_out) {
    if (!c) return PGA_EINVAL;
    auto bad = [&](std::string msg) { c->err = "pga_label_bases: " + msg; return PGA_EINVAL; };
    if (!batch || !o || n_genes < 0 || n_out_elems < 0 || (n_genes > 0 && !genes)) return bad("bad arguments");
    const pga_batch_view bv = pga_batch_peek(batch);
    if (bv.ctx != c) return bad("the batch belongs to another context");
    if (bv.n > 0 && !len_out) return bad("bad arguments");
    // ---- validation: all of it on the host, before anything is allocated or launched ----
    const int eb = o->elem_bytes;
    if (eb != 1 && eb != 4 && eb != 8) return bad("elem_bytes must be 1, 4 or 8, not " + std::to_string(eb));
    if (o->layout != PGA_TOKENS_RAGGED && o->layout != PGA_TOKENS_PADDED) return bad("layout must be PGA_TOKENS_RAGGED or PGA_TOKENS_PADDED, not " + std::to_string(o->layout));
    const bool padded = o->layout == PGA_TOKENS_PADDED;
    auto fits = [&](const int64_t v) { return eb == 8 || (eb == 4 ? v >= INT32_MIN && v <= INT32_MAX : v >= 0 && v <= 255); };
    const char* const elem_name = eb == 1 ? "uint8" : eb == 4 ? "int32" : "int64";
    for (int k = 0; k < 256; k++)
        if (!fits(o->class_map[k])) return bad("class_map[" + std::to_string(k) + "] = " + std::to_string(o->class_map[k]) + " does not fit " + elem_name);
    if (padded && !fits(o->pad)) return bad("pad = " + std::to_string(o->pad) + " does not fit " + elem_name);
    const size_t B = (size_t)bv.n;
    std::vector<int64_t> off(B + 1, 0), iv_off(B + 1, 0);
    int64_t longest = 0, longest_i = -1;
    for (size_t i = 0; i < B; i++) {
        const int64_t len = bv.ct[i].len;
        if (len > INT32_MAX - 16) return bad("contig " + std::to_string(i) + " is too long");
        off[i + 1] = off[i] + len;
        if (len > longest) { longest = len; longest_i = (int64_t)i; }
    }
    int64_t need = off[B];
    if (padded) {
        const int64_t W = o->row_width, S = o->row_stride;
        if (W < longest) return bad("row_width = " + std::to_string(W) + " is less than the " + std::to_string(longest) + " bases of contig " + std::to_string(longest_i));
        if (W < 0 || S < W) return bad("row_stride = " + std::to_string(S) + " is less than row_width = " + std::to_string(W));
        if (B > 1 && S > (INT64_MAX / 8 - W) / (int64_t)(B - 1)) return bad("row_stride = " + std::to_string(S) + " is too large");
        need = B > 0 ? (int64_t)(B - 1) * S + W : 0;
    }
    if (n_out_elems < need) return bad("n_out_elems = " + std::to_string(n_out_elems) + " is less than the " + std::to_string(need) + " elements of the layout");
    // every record inside its contig, in whole codons; a record across the origin makes two stretches
    for (int64_t g = 0; g < n_genes; g++) {
        const pga_gene& G = genes[g];
        const std::string who = "gene " + std::to_string(g);
        if (G.contig < 0 || G.contig >= bv.n) return bad(who + " names contig " + std::to_string(G.contig) + " of " + std::to_string(bv.n));
        const int64_t len = bv.ct[G.contig].len, glen = (int64_t)G.end - G.begin + 1;
        if (G.begin < 1 || G.begin > len || glen < 3 || glen > len) return bad(who + " lies outside its contig");
        if (glen % 3) return bad(who + " is " + std::to_string(glen) + " bases long, no whole number of codons");
        if (G.end > len && !(bv.circular && bv.circular[G.contig])) return bad(who + " ends beyond its contig, which is not flagged circular");
        iv_off[(size_t)G.contig + 1] += G.end > len ? 2 : 1;
    }
    if (need > 0) {
        if (!d_out) return bad("d_out is NULL");
        if ((uintptr_t)d_out % (uintptr_t)eb) return bad("d_out is not aligned to its " + std::to_string(eb) + "-byte elements");
        if (hipSetDevice(c->device) != hipSuccess) return PGA_EDEVICE;
        // the pointer is asked about, never dereferenced on the host, and never handed to a kernel unless the runtime calls it device memory
        hipPointerAttribute_t at{};
        const hipError_t pe = hipPointerGetAttributes(&at, d_out);
        if (pe != hipSuccess) (void)hipGetLastError();
        if (pe != hipSuccess || at.type != hipMemoryTypeDevice) return bad("d_out is not device memory (a host pointer?)");
        if (at.device != c->device) return bad("d_out is not device memory of the context's device " + std::to_string(c->device) + " but of device " + std::to_string(at.device));
    }
    for (size_t i = 0; i < B; i++) len_out[i] = bv.ct[i].len;
    if (need == 0) return PGA_OK;
    // ---- the kernel's tables: staged in the upload's pinned area as they will lie on the device, one copy ----
    for (size_t i = 0; i < B; i++) iv_off[i + 1] += iv_off[i];
    const size_t n_iv = (size_t)iv_off[B];
    const size_t off_b = sizeof(int64_t) * (B + 1), map_b = sizeof(int64_t) * 256, iv_b = sizeof(LabIv) * n_iv;
    const size_t tab = 2 * off_b + map_b + iv_b;               // (the stretches begin at a multiple of 16 bytes)
    pga_upload_lease L{};
    { const int rc = pga_upload_lease_take(c, tab, &L); if (rc) return rc; }
    memcpy(L.pin, off.data(), off_b);
    memcpy(L.pin + off_b, iv_off.data(), off_b);
    memcpy(L.pin + 2 * off_b, o->class_map, map_b);
    lab_stretches(genes, n_genes, bv.ct, iv_off.data(), B, (LabIv*)(L.pin + 2 * off_b + map_b));
    LabArgs a{};
    a.off = (const int64_t*)L.dev; a.iv_off = (const int64_t*)(L.dev + off_b); a.cmap = (const int64_t*)(L.dev + 2 * off_b);
    a.iv = (const LabIv*)(L.dev + 2 * off_b + map_b);
    a.n_contigs = bv.n; a.n_elems = need; a.W = padded ? o->row_width : 0; a.S = padded ? o->row_stride : 0; a.pad = padded ? o->pad : 0;
    a.out0 = (char*)((uintptr_t)d_out & ~(uintptr_t)15);
    a.lead = (int32_t)(((uintptr_t)d_out - (uintptr_t)a.out0) / (uintptr_t)eb);
    const int64_t per = 16 / eb, pieces = (a.lead + need + per - 1) / per;
    const dim3 grid((unsigned)((pieces + kLabThreads - 1) / kLabThreads)), block(kLabThreads);
    // the upload stream is non-blocking: it waits for what the caller's stream held when the call came
    hipError_t e = hipEventRecord(L.ev, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(L.st, L.ev, 0);
    if (e == hipSuccess) e = hipMemcpyAsync(L.dev, L.pin, tab, hipMemcpyHostToDevice, L.st);
    if (e == hipSuccess) {
        if (padded) {
            if (eb == 1) hipLaunchKernelGGL((k_label_bases<1, true>), grid, block, 0, L.st, a);
            else if (eb == 4) hipLaunchKernelGGL((k_label_bases<4, true>), grid, block, 0, L.st, a);
            else hipLaunchKernelGGL((k_label_bases<8, true>), grid, block, 0, L.st, a);
        } else {
            if (eb == 1) hipLaunchKernelGGL((k_label_bases<1, false>), grid, block, 0, L.st, a);
            else if (eb == 4) hipLaunchKernelGGL((k_label_bases<4, false>), grid, block, 0, L.st, a);
            else hipLaunchKernelGGL((k_label_bases<8, false>), grid, block, 0, L.st, a);
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(L.st);         // on return the tensor is complete for any stream
    pga_upload_lease_give(c);
    return pga_hip_try_(c, e, "pga_label_bases");
}
