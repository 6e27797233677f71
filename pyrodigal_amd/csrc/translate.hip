// Device-side translation of gene records into proteins: one thread per codon.
// ref: lib.pyx:2932-3047 (Gene.translate), 770-789 (Sequence._amino); the codes and codon rules are in translate_rules.h.
#include "pga_internal.h"
#include <mutex>
#include "pipeline.h"
#include "translate_rules.h"

#include <string.h>

#include <vector>

struct pga_batch_view { pga_ctx* ctx; int32_t n; int64_t total; const ContigDesc* ct; const char* d_seq; const uint8_t* circular /* or nullptr: all linear */; };
pga_batch_view pga_batch_peek(const pga_batch*);      // finder.hip

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
