// Device rendering of gene records into the text the host writers emit: GFF (Genes.write_gff), protein FASTA
// (Genes.write_translations) and gene FASTA (Genes.write_genes), contig after contig, byte for byte.
// ref: lib.pyx:3534-3792 (the writers), 2844-2872 (Gene._rbs), gene.c calculate_confidence.
//
// Per format: a length pass (the line renderers run with a counting sink), an exclusive scan of the lengths, and a write pass
// (the same renderers, now writing at the scanned offsets).  One text arena per format, copied back once into pinned memory.
//   GFF            one thread per line: the three header lines of a contig are one unit, every gene line one unit
//   FASTA records  one thread per record header; one wavefront per record body (residues / bases, newline every `width`)
// Numbers are printed by render_fmt.h (exact '%.Nf').  A GFF line whose confidence lies within `fallback_margin` of a rounding
// midpoint is flagged: the device exp may differ from glibc's by an ulp, so the host renders that line itself.
#include "pga_internal.h"
#include "pipeline.h"
#include "render_fmt.h"
#include "translate_rules.h"

#include <hipcub/hipcub.hpp>

#include <string.h>

#include <string>
#include <vector>

struct pga_batch_view { pga_ctx* ctx; int32_t n; int64_t total; const ContigDesc* ct; const char* d_seq; };
pga_batch_view pga_batch_peek(const pga_batch*);      // finder.hip

namespace {

using pga_fmt::Sink;

// ref: lib.pyx:143-153 (_RBS_MOTIF / _RBS_SPACER; index 0 prints as Python's None)
__constant__ char c_rbs_motif[28][16] = {
    "None", "GGA/GAG/AGG", "3Base/5BMM", "4Base/6BMM", "AGxAG", "AGxAG", "GGA/GAG/AGG", "GGxGG", "GGxGG",
    "AGxAG", "AGGAG(G)/GGAGG", "AGGA/GGAG/GAGG", "AGGA/GGAG/GAGG", "GGA/GAG/AGG", "GGxGG", "AGGA",
    "GGAG/GAGG", "AGxAGG/AGGxGG", "AGxAGG/AGGxGG", "AGxAGG/AGGxGG", "AGGAG/GGAGG", "AGGAG", "AGGAG",
    "GGAGG", "GGAGG", "AGGAGG", "AGGAGG", "AGGAGG"};
__constant__ char c_rbs_spacer[28][8] = {
    "None", "3-4bp", "13-15bp", "13-15bp", "11-12bp", "3-4bp", "11-12bp", "11-12bp", "3-4bp", "5-10bp",
    "13-15bp", "3-4bp", "11-12bp", "5-10bp", "5-10bp", "5-10bp", "5-10bp", "11-12bp", "3-4bp", "5-10bp",
    "11-12bp", "3-4bp", "5-10bp", "3-4bp", "5-10bp", "11-12bp", "3-4bp", "5-10bp"};
__constant__ char c_node_type[4][5] = {"ATG", "GTG", "TTG", "Edge"};

// what the lines need of a model (pga_training)
struct RenderModel {
    double rbs_wt[28];
    double st_wt, no_mot, gc;
    int32_t tt, uses_sd;
    int32_t desc_off, desc_len;     // in the string arena
};

struct RenderArgs {
    const char* seq; const ContigDesc* ct; const pga_gene* genes; const int64_t* gene_begin; const int32_t* moc;
    const RenderModel* models; const char* str; const int64_t* id_off; const char* code;   // code: [34][64] residues by digits
    int32_t src_off, src_len, ver_off, ver_len;
    int32_t n_contigs, meta;
    int64_t n_genes, first_seqnum;
    int32_t header, incl_tt, full_id, width, tt, include_stop, strict;
    double margin;
    int64_t* len;          // length pass: [n_units + 1] line / record lengths (the last one 0)
    int64_t* off;          // their exclusive scan: where every unit starts; off[n_units] = the text's size
    int32_t* hdr_len;      // FASTA: [n_genes] header line length of every record
    uint8_t* flag;         // [n_units] 1: the host renders this unit
    unsigned long long* n_flag;
    char* out;
};

__device__ __forceinline__ void put_id(Sink& o, const RenderArgs& a, const int c) {
    o.put_n(a.str + a.id_off[c], a.id_off[c + 1] - a.id_off[c]);
}

// Gene._gene_data (lib.pyx:1091-1095): ID=..;partial=..;start_type=..;rbs_motif=..;rbs_spacer=..;gc_cont=..
__device__ bool gene_data(Sink& o, const RenderArgs& a, const pga_gene& g, const int c, const int64_t k, const int full_id) {
    o.puts("ID=");
    if (full_id) put_id(o, a, c); else pga_fmt::put_i64(o, a.first_seqnum + c);
    o.put('_'); pga_fmt::put_i64(o, k + 1);
    o.puts(";partial="); o.put((char)('0' + (g.partial_begin ? 1 : 0))); o.put((char)('0' + (g.partial_end ? 1 : 0)));
    o.puts(";start_type="); o.puts(c_node_type[g.start_type & 3]);
    // Gene._rbs (lib.pyx:951-969)
    const RenderModel& m = a.models[a.moc[c]];
    const double st = m.st_wt;
    const int k0 = g.rbs[0], k1 = g.rbs[1];
    const double r1 = m.rbs_wt[k0] * st, r2 = m.rbs_wt[k1] * st, ms = g.mot_score * st;
    int site = -1;
    if (m.uses_sd) site = r1 > r2 ? k0 : k1;
    else if (m.no_mot > -0.5 && r1 > r2 && r1 > ms) site = k0;
    else if (m.no_mot > -0.5 && r2 >= r1 && r2 > ms) site = k1;
    o.puts(";rbs_motif=");
    if (site >= 0) {
        o.puts(c_rbs_motif[site]); o.puts(";rbs_spacer="); o.puts(c_rbs_spacer[site]);
    } else if (g.mot_len == 0) {
        o.puts("None;rbs_spacer=None");
    } else {
        for (int i = 0; i < g.mot_len; i++) {
            const int s = 2 * i;
            const int d = s < 32 ? (g.mot_ndx >> s) & 3 : (g.mot_ndx < 0 ? 3 : 0);
            o.put("AGCT"[d]);
        }
        o.puts(";rbs_spacer="); pga_fmt::put_i64(o, g.mot_spacer); o.puts("bp");
    }
    o.puts(";gc_cont=");
    return pga_fmt::fmt_fixed(o, (double)g.gc_cont, 3);
}

// the header lines of contig c in write_gff (lib.pyx:1167-1178)
__device__ void gff_header(Sink& o, const RenderArgs& a, const int c) {
    const RenderModel& m = a.models[a.moc[c]];
    if (a.header) o.puts("##gff-version  3\n");
    o.puts("# Sequence Data: seqnum="); pga_fmt::put_i64(o, a.first_seqnum + c);
    o.puts(";seqlen="); pga_fmt::put_i64(o, a.ct[c].len);
    o.puts(";seqhdr=\""); put_id(o, a, c);
    o.puts("\"\n# Model Data: version="); o.put_n(a.str + a.ver_off, a.ver_len);
    o.puts(a.meta ? ";run_type=Metagenomic;model=\"" : ";run_type=Single;model=\"");
    o.put_n(a.str + m.desc_off, m.desc_len);
    o.puts("\";gc_cont=");
    pga_fmt::fmt_fixed(o, m.gc * 100, 2);             // gc in [0, 1]: always the exact path
    o.puts(";transl_table="); pga_fmt::put_i64(o, m.tt);
    o.puts(";uses_sd="); o.put(m.uses_sd ? '1' : '0');
    o.put('\n');
}

// one gene line of write_gff (lib.pyx:1179-1188)
__device__ bool gff_gene(Sink& o, const RenderArgs& a, const int64_t gi) {
    const pga_gene g = a.genes[gi];
    const int c = g.contig;
    const RenderModel& m = a.models[a.moc[c]];
    bool ok = true;
    put_id(o, a, c); o.put('\t');
    o.put_n(a.str + a.src_off, a.src_len);
    o.puts("\tCDS\t"); pga_fmt::put_i64(o, g.begin); o.put('\t'); pga_fmt::put_i64(o, g.end); o.put('\t');
    ok &= pga_fmt::fmt_fixed(o, g.sscore + g.cscore, 1);
    o.puts(g.strand > 0 ? "\t+\t0\t" : "\t-\t0\t");
    ok &= gene_data(o, a, g, c, gi - a.gene_begin[c], a.full_id);
    o.put(';');
    if (a.incl_tt) { o.puts("transl_table="); pga_fmt::put_i64(o, m.tt); o.put(';'); }
    // Gene._score_data (lib.pyx:1097-1099), the confidence as _confidence (lib.pyx:908)
    const double score = g.cscore + g.sscore;
    const double r = score / m.st_wt;
    double conf;
    bool hazard = false;
    if (r < 41) {
        conf = exp(r);
        conf = (conf / (conf + 1)) * 100.0;
        hazard = true;
    } else {
        conf = 99.99;
    }
    conf = fmax(conf, 50.0);
    if (hazard && conf != 50.0 && pga_fmt::near_midpoint(conf, 2, a.margin)) ok = false;
    o.puts("conf="); ok &= pga_fmt::fmt_fixed(o, conf, 2);
    o.puts(";score="); ok &= pga_fmt::fmt_fixed(o, score, 2);
    o.puts(";cscore="); ok &= pga_fmt::fmt_fixed(o, g.cscore, 2);
    o.puts(";sscore="); ok &= pga_fmt::fmt_fixed(o, g.sscore, 2);
    o.puts(";rscore="); ok &= pga_fmt::fmt_fixed(o, g.rscore, 2);
    o.puts(";uscore="); ok &= pga_fmt::fmt_fixed(o, g.uscore, 2);
    o.puts(";tscore="); ok &= pga_fmt::fmt_fixed(o, g.tscore, 2);
    o.puts(";\n");
    return ok;
}

// units 0 .. n_contigs - 1: the header of contig idx; the rest: gene idx - n_contigs.  Unit u of the text: a contig's header
// comes right before its genes, u = c + gene_begin[c] for the header and c + 1 + g for gene g
__global__ void __launch_bounds__(256) k_gff(const RenderArgs a, const int write) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.n_contigs + a.n_genes) return;
    int64_t u;
    int c = -1;
    int64_t g = -1;
    if (idx < a.n_contigs) { c = (int)idx; u = c + a.gene_begin[c]; }
    else { g = idx - a.n_contigs; u = a.genes[g].contig + 1 + g; }
    Sink o{write ? a.out + a.off[u] : nullptr, 0};
    bool ok = true;                  // (a header is never flagged: the host checked every model's gc)
    if (c >= 0) gff_header(o, a, c); else ok = gff_gene(o, a, g);
    if (!write) {
        a.len[u] = o.n;
        a.flag[u] = ok ? 0 : 1;
        if (!ok) atomicAdd(a.n_flag, 1ull);
    }
}

__device__ __forceinline__ int64_t body_len(const RenderArgs& a, const pga_gene& g, const int protein) {
    const int64_t n = g.end - g.begin + 1;
    if (!protein) return n;
    const bool stop_edge = g.strand == 1 ? g.partial_end : g.partial_begin;
    const int64_t l = n / 3 - ((!stop_edge && !a.include_stop) ? 1 : 0);
    return l > 0 ? l : 0;
}

// FASTA record headers (lib.pyx:1194-1196 / 1210-1212): '>id_k # begin # end # strand # gene data'; the length pass sizes the
// whole record (header + body + a newline every `width` letters)
__global__ void __launch_bounds__(256) k_fa_head(const RenderArgs a, const int protein, const int write) {
    const int64_t gi = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= a.n_genes) return;
    const pga_gene g = a.genes[gi];
    const int c = g.contig;
    const int64_t k = gi - a.gene_begin[c];
    Sink o{write ? a.out + a.off[gi] : nullptr, 0};
    o.put('>'); put_id(o, a, c); o.put('_'); pga_fmt::put_i64(o, k + 1);
    o.puts(" # "); pga_fmt::put_i64(o, g.begin); o.puts(" # "); pga_fmt::put_i64(o, g.end);
    o.puts(" # "); pga_fmt::put_i64(o, g.strand); o.puts(" # ");
    const bool ok = gene_data(o, a, g, c, k, a.full_id);
    o.put('\n');
    if (!write) {
        const int64_t L = body_len(a, g, protein);
        a.hdr_len[gi] = (int32_t)o.n;
        a.len[gi] = o.n + L + (L + a.width - 1) / a.width;
        a.flag[gi] = ok ? 0 : 1;
        if (!ok) atomicAdd(a.n_flag, 1ull);
    }
}

__device__ __forceinline__ char base_at(const char* s, const int64_t p, const bool comp) {
    char ch = s[p];
    if (ch >= 'a' && ch <= 'z') ch = (char)(ch - 32);
    if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T') return 'N';
    if (!comp) return ch;
    return ch == 'A' ? 'T' : ch == 'T' ? 'A' : ch == 'C' ? 'G' : 'C';
}

// FASTA record bodies: one wavefront per record, lane l writes letters l, l + 64, ... and the newline after each full line
// and after the last letter (Gene.sequence, lib.pyx:1021-1028 / Gene.translate, 1030-1089)
__global__ void __launch_bounds__(256) k_fa_body(const RenderArgs a, const int protein) {
    const int64_t gi = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (gi >= a.n_genes) return;
    const pga_gene g = a.genes[gi];
    const int c = g.contig;
    const char* __restrict__ s = a.seq + a.ct[c].base;
    const int L = (int)body_len(a, g, protein);       // < 2^31: a contig's length is an int32
    char* __restrict__ out = a.out + a.off[gi] + a.hdr_len[gi];
    const int w = a.width;
    const int tt = a.tt > 0 ? a.tt : a.models[a.moc[c]].tt;
    const char* row = a.code + 64 * tt;
    const bool start_edge = g.strand == 1 ? g.partial_begin : g.partial_end;
    // line / column of letter i, stepped by 64 letters per iteration: one division per lane, not one per letter
    const int step_line = 64 / w, step_col = 64 % w;
    int line = lane / w, col = lane % w;
    for (int i = lane; i < L; i += 64) {
        char ch;
        if (!protein) {
            ch = g.strand == 1 ? base_at(s, g.begin - 1 + i, false) : base_at(s, g.end - 1 - i, true);
        } else {
            int x0, x1, x2;
            if (g.strand == 1) {
                const int p = g.begin - 1 + 3 * i;
                x0 = pga_tr::digit_of(s[p], false); x1 = pga_tr::digit_of(s[p + 1], false); x2 = pga_tr::digit_of(s[p + 2], false);
            } else {
                const int p = g.end - 1 - 3 * i;
                x0 = pga_tr::digit_of(s[p], true); x1 = pga_tr::digit_of(s[p - 1], true); x2 = pga_tr::digit_of(s[p - 2], true);
            }
            ch = pga_tr::translate_codon(row, x0, x1, x2, tt, i, start_edge, a.strict, 'X');
        }
        const int64_t at = (int64_t)i + line;
        out[at] = ch;
        if (col == w - 1 || i == L - 1) out[at + 1] = '\n';
        line += step_line; col += step_col;
        if (col >= w) { col -= w; line++; }
    }
}

// contig i's first byte: the first unit of the contig (its GFF header, or its first record); off[n_units] = total
__global__ void k_contig_off(const int64_t* __restrict__ off, const int64_t* __restrict__ gene_begin, const int n_contigs,
                             const int64_t n_units, const int gff, int64_t* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_contigs) return;
    out[c] = c == n_contigs ? off[n_units] : off[gff ? c + gene_begin[c] : gene_begin[c]];
}

struct CodeTables {
    char code[34][64];
    unsigned char known[34];
    CodeTables() { pga_tr::code_table(code, known); }
};

}  // namespace

// grow-only buffers of the context: reallocated only when a call needs more than the last one (with a quarter of headroom)
static hipError_t grow(char*& p, size_t& cap, const size_t need, const bool pinned) {
    if (need <= cap && p) return hipSuccess;
    if (p) { if (pinned) hipHostFree(p); else hipFree(p); }
    p = nullptr; cap = 0;
    const size_t want = need + need / 4 + 4096;
    const hipError_t e = pinned ? hipHostMalloc((void**)&p, want, hipHostMallocDefault) : hipMalloc((void**)&p, want);
    if (e == hipSuccess) cap = want; else p = nullptr;
    return e;
}

void pga_render_release(pga_ctx* c) {
    if (c->render_dev) hipFree(c->render_dev);
    if (c->render_text) hipFree(c->render_text);
    if (c->render_host) hipHostFree(c->render_host);
    if (c->render_small) hipHostFree(c->render_small);
    c->render_dev = c->render_text = c->render_host = nullptr;
    c->render_small = nullptr;
    c->render_dev_cap = c->render_text_cap = c->render_host_cap = 0;
}

extern "C" void pga_render_free(pga_render_result* r) {
    if (!r) return;
    for (pga_text& t : r->text) {
        free(t.contig_off);
        free(t.fallback);
    }
    delete r;
}

extern "C" int pga_render_genes(pga_ctx* c, const pga_batch* batch, const pga_contig_result* contigs, int64_t n_genes, const pga_gene* genes,
                                const int32_t* model_of_contig, const char* ids, const int64_t* id_off, const pga_render_opts* opts,
                                pga_render_result** out) {
#define BAD(msg) do { c->err = "pga_render_genes: " msg; return PGA_EINVAL; } while (0)
    if (!c) return PGA_EINVAL;
    if (!batch || !contigs || n_genes < 0 || (n_genes > 0 && !genes) || !model_of_contig || !id_off || !opts || !out) BAD("bad arguments");
    *out = nullptr;
    const pga_batch_view bv = pga_batch_peek(batch);
    if (bv.ctx != c) BAD("the batch belongs to another context");
    const pga_render_opts& O = *opts;
    const int NC = bv.n;
    if ((O.formats & ~7) || !O.formats) BAD("`formats` must be a non-empty set of PGA_RENDER_* bits");
    if (((O.formats & PGA_RENDER_FAA) && O.faa_width < 1) || ((O.formats & PGA_RENDER_FNA) && O.fna_width < 1)) BAD("`width` must be at least 1");
    if ((O.formats & PGA_RENDER_FAA) && O.faa_translation_table != 0 && !pga_tr::table_known(O.faa_translation_table))
        BAD("not a valid translation table index");
    if (!O.source || !O.version || (c->n_models > 0 && !O.model_desc)) BAD("missing tool strings");
    if (!(O.fallback_margin >= 0)) BAD("`fallback_margin` must be >= 0");
    // the layout the kernels rely on: genes of contig i are genes[gene_begin .. + n_genes), contig after contig, inside the contig
    int64_t run = 0;
    std::vector<int64_t> gbeg((size_t)NC + 1);
    for (int i = 0; i < NC; i++) {
        if (contigs[i].gene_begin != run || contigs[i].n_genes < 0) BAD("contig records do not tile the gene records");
        gbeg[i] = run;
        run += contigs[i].n_genes;
        const int m = model_of_contig[i];
        if (m < -1 || m >= c->n_models) BAD("model index outside the loaded set");
        if (m < 0 && (contigs[i].n_genes > 0 || (O.formats & PGA_RENDER_GFF))) BAD("no model was selected for a contig");
        if (id_off[i + 1] < id_off[i] || id_off[i] < 0) BAD("id offsets are not increasing");
    }
    gbeg[NC] = run;
    if (run != n_genes) BAD("contig records do not tile the gene records");
    if (id_off[0] != 0 || (id_off[NC] > 0 && !ids)) BAD("id offsets must start at 0");
    for (int i = 0; i < NC; i++)
        for (int64_t g = gbeg[i]; g < gbeg[i + 1]; g++) {
            const pga_gene& G = genes[g];
            if (G.contig != i || G.begin < 1 || G.end > bv.ct[i].len || G.end < G.begin || G.rbs[0] >= 28 || G.rbs[1] >= 28)
                BAD("gene record outside its contig");
        }
    // models and the string arena: ids, then the model descriptions, the source and the version
    std::string str(ids ? ids : "", (size_t)id_off[NC]);
    std::vector<RenderModel> models((size_t)std::max(c->n_models, 1));
    for (int m = 0; m < c->n_models; m++) {
        const pga_training& t = c->models[m];
        RenderModel& R = models[m];
        memcpy(R.rbs_wt, t.rbs_wt, sizeof R.rbs_wt);
        R.st_wt = t.st_wt; R.no_mot = t.no_mot; R.gc = t.gc; R.tt = t.trans_table; R.uses_sd = t.uses_sd != 0;
        const char* d = O.model_desc[m] ? O.model_desc[m] : "";
        R.desc_off = (int32_t)str.size(); R.desc_len = (int32_t)strlen(d); str += d;
        if (!pga_tr::table_known(R.tt) && (O.formats & PGA_RENDER_FAA)) BAD("a loaded model has an unknown translation table");
        if (!(t.gc >= 0 && t.gc <= 1) || !(t.st_wt != 0)) BAD("a loaded model has no GC content or start weight");
    }
    const int32_t src_off = (int32_t)str.size(), src_len = (int32_t)strlen(O.source); str += O.source;
    const int32_t ver_off = (int32_t)str.size(), ver_len = (int32_t)strlen(O.version); str += O.version;
    static const CodeTables tables;         // built once (thread-safe static initialisation)
    const auto& code = tables.code;

    pga_render_result* R = new pga_render_result();
    R->n_contigs = NC;
    if (hipSetDevice(c->device) != hipSuccess) { delete R; return PGA_EDEVICE; }
    hipStream_t st = c->stream;
    const int fmts[3] = {PGA_RENDER_GFF, PGA_RENDER_FAA, PGA_RENDER_FNA};
    int64_t units[3];
    for (int f = 0; f < 3; f++) units[f] = (O.formats & fmts[f]) ? (f == 0 ? NC + n_genes : n_genes) : -1;
    // one device allocation for everything but the text: inputs, then per format lengths / offsets, flags, header lengths
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t o_genes = 0, o_ct = o_genes + al(sizeof(pga_gene) * (size_t)std::max<int64_t>(n_genes, 1));
    size_t o_gb = o_ct + al(sizeof(ContigDesc) * (NC + 1)), o_moc = o_gb + al(sizeof(int64_t) * (NC + 1));
    size_t o_mod = o_moc + al(sizeof(int32_t) * (NC + 1)), o_idoff = o_mod + al(sizeof(RenderModel) * models.size());
    size_t o_str = o_idoff + al(sizeof(int64_t) * (NC + 1)), o_code = o_str + al(str.size() + 1);
    size_t o_cnt = o_code + al(sizeof code), o_f = o_cnt + al(sizeof(unsigned long long) * 8);
    size_t o_len[3], o_off[3], o_flag[3], o_hdr[3], o_coff[3];
    size_t scan_bytes = 0, o_tmp;
    for (int f = 0; f < 3; f++) {
        const int64_t nu = std::max<int64_t>(units[f], 0);
        o_len[f] = o_f; o_f += al(sizeof(int64_t) * (nu + 1));
        o_off[f] = o_f; o_f += al(sizeof(int64_t) * (nu + 1));
        o_flag[f] = o_f; o_f += al((size_t)nu + 1);
        o_hdr[f] = o_f; o_f += al(sizeof(int32_t) * (size_t)(f ? std::max<int64_t>(n_genes, 1) : 1));
        o_coff[f] = o_f; o_f += al(sizeof(int64_t) * (NC + 1));
        if (units[f] >= 0) {
            size_t b = 0;
            hipcub::DeviceScan::ExclusiveSum(nullptr, b, (int64_t*)nullptr, (int64_t*)nullptr, (int)(units[f] + 1), st);
            scan_bytes = std::max(scan_bytes, b);
        }
    }
    o_tmp = o_f; o_f += al(scan_bytes + 1);
    char* d = nullptr;
    char* d_text = nullptr;
    unsigned long long* h_small = nullptr;
    hipEvent_t ev[3][4] = {};
    auto fail = [&](hipError_t e) {
        hipStreamSynchronize(st);
        for (auto& row : ev) for (auto& x : row) if (x) hipEventDestroy(x);
        pga_render_free(R);
        return pga_hip_try_(c, e, "pga_render_genes");
    };
    hipError_t e = grow(c->render_dev, c->render_dev_cap, o_f, false);
    d = c->render_dev;
    if (e == hipSuccess && !c->render_small) e = hipHostMalloc((void**)&c->render_small, sizeof(unsigned long long) * 8, hipHostMallocDefault);
    h_small = c->render_small;
    for (int f = 0; f < 3 && e == hipSuccess; f++)
        for (int k = 0; k < 4 && e == hipSuccess; k++) e = hipEventCreate(&ev[f][k]);
    if (e != hipSuccess) return fail(e);
    if (n_genes > 0) e = hipMemcpyAsync(d + o_genes, genes, sizeof(pga_gene) * (size_t)n_genes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_ct, bv.ct, sizeof(ContigDesc) * (NC + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_gb, gbeg.data(), sizeof(int64_t) * (NC + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && NC > 0) e = hipMemcpyAsync(d + o_moc, model_of_contig, sizeof(int32_t) * NC, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_mod, models.data(), sizeof(RenderModel) * models.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_idoff, id_off, sizeof(int64_t) * (NC + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_str, str.c_str(), str.size() + 1, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_code, code, sizeof code, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d + o_cnt, 0, sizeof(unsigned long long) * 8, st);
    if (e != hipSuccess) return fail(e);

    RenderArgs A{};
    A.seq = bv.d_seq; A.ct = (const ContigDesc*)(d + o_ct); A.genes = (const pga_gene*)(d + o_genes);
    A.gene_begin = (const int64_t*)(d + o_gb); A.moc = (const int32_t*)(d + o_moc); A.models = (const RenderModel*)(d + o_mod);
    A.str = d + o_str; A.id_off = (const int64_t*)(d + o_idoff); A.code = d + o_code;
    A.src_off = src_off; A.src_len = src_len; A.ver_off = ver_off; A.ver_len = ver_len;
    A.n_contigs = NC; A.meta = O.meta; A.n_genes = n_genes; A.first_seqnum = O.first_seqnum; A.margin = O.fallback_margin;
    RenderArgs fa[3];
    for (int f = 0; f < 3; f++) {
        RenderArgs& a = fa[f];
        a = A;
        a.len = (int64_t*)(d + o_len[f]); a.off = (int64_t*)(d + o_off[f]); a.flag = (uint8_t*)(d + o_flag[f]); a.hdr_len = (int32_t*)(d + o_hdr[f]);
        a.n_flag = (unsigned long long*)(d + o_cnt) + f;
        if (f == 0) { a.header = O.gff_header; a.incl_tt = O.gff_include_translation_table; a.full_id = O.gff_full_id; a.width = 1; }
        if (f == 1) { a.width = O.faa_width; a.tt = O.faa_translation_table; a.include_stop = O.faa_include_stop; a.strict = O.faa_strict; a.full_id = O.faa_full_id; }
        if (f == 2) { a.width = O.fna_width; a.full_id = O.fna_full_id; a.include_stop = 1; a.strict = 1; }
    }
    // length passes and scans
    for (int f = 0; f < 3 && e == hipSuccess; f++) {
        if (units[f] < 0) continue;
        RenderArgs& a = fa[f];
        e = hipEventRecord(ev[f][0], st);
        if (e == hipSuccess) e = hipMemsetAsync(a.len + units[f], 0, sizeof(int64_t), st);
        if (e == hipSuccess && units[f] > 0) {
            const unsigned nb = (unsigned)((units[f] + 255) / 256);
            if (f == 0) hipLaunchKernelGGL(k_gff, dim3(nb), dim3(256), 0, st, a, 0);
            else hipLaunchKernelGGL(k_fa_head, dim3(nb), dim3(256), 0, st, a, f == 1 ? 1 : 0, 0);
            e = hipGetLastError();
        }
        size_t tb = scan_bytes;
        if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(d + o_tmp, tb, a.len, a.off, (int)(units[f] + 1), st);
        if (e == hipSuccess) e = hipEventRecord(ev[f][1], st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_small + f, a.off + units[f], sizeof(int64_t), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_small + 3, d + o_cnt, sizeof(unsigned long long) * 3, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(e);
    int64_t total[3], toff[3], tsum = 0;
    for (int f = 0; f < 3; f++) { total[f] = units[f] < 0 ? 0 : (int64_t)h_small[f]; toff[f] = tsum; tsum += total[f]; }
    if (tsum > 0) e = grow(c->render_text, c->render_text_cap, (size_t)tsum, false);
    if (e == hipSuccess && tsum > 0) e = grow(c->render_host, c->render_host_cap, (size_t)tsum, true);
    if (e != hipSuccess) return fail(e);
    d_text = c->render_text;
    // write passes, contig offsets, copies back
    for (int f = 0; f < 3 && e == hipSuccess; f++) {
        if (units[f] < 0) continue;
        RenderArgs& a = fa[f];
        a.out = d_text + toff[f];
        e = hipEventRecord(ev[f][2], st);
        if (e == hipSuccess && units[f] > 0) {
            const unsigned nb = (unsigned)((units[f] + 255) / 256);
            if (f == 0) hipLaunchKernelGGL(k_gff, dim3(nb), dim3(256), 0, st, a, 1);
            else {
                hipLaunchKernelGGL(k_fa_head, dim3(nb), dim3(256), 0, st, a, f == 1 ? 1 : 0, 1);
                hipLaunchKernelGGL(k_fa_body, dim3((unsigned)((n_genes + 3) / 4)), dim3(256), 0, st, a, f == 1 ? 1 : 0);
            }
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ev[f][3], st);
        int64_t* d_coff = (int64_t*)(d + o_coff[f]);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_contig_off, dim3((unsigned)((NC + 1 + 255) / 256)), dim3(256), 0, st, (const int64_t*)a.off, A.gene_begin, NC,
                               units[f], f == 0 ? 1 : 0, d_coff);
            e = hipGetLastError();
        }
        pga_text& T = R->text[f];
        T.contig_off = (int64_t*)malloc(sizeof(int64_t) * (NC + 1));
        T.size = total[f];
        if (!T.contig_off) e = hipErrorOutOfMemory;
        T.data = total[f] > 0 ? c->render_host + toff[f] : nullptr;
        if (e == hipSuccess && total[f] > 0) e = hipMemcpyAsync(T.data, a.out, (size_t)total[f], hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(T.contig_off, d_coff, sizeof(int64_t) * (NC + 1), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(e);
    // flagged units (rare): their gene index and byte range
    for (int f = 0; f < 3 && e == hipSuccess; f++) {
        if (units[f] < 0) continue;
        pga_text& T = R->text[f];
        T.n_fallback = (int64_t)h_small[3 + f];
        float ms_a = 0, ms_b = 0;
        hipEventElapsedTime(&ms_a, ev[f][0], ev[f][1]);
        hipEventElapsedTime(&ms_b, ev[f][2], ev[f][3]);
        R->t_kernels_ms[f] = (double)ms_a + (double)ms_b;
        if (T.n_fallback == 0) continue;
        const int64_t nu = units[f];
        std::vector<int64_t> off((size_t)nu + 1);
        std::vector<uint8_t> fl((size_t)nu);
        std::vector<int32_t> hl((size_t)std::max<int64_t>(f ? n_genes : 0, 1));
        e = hipMemcpy(off.data(), fa[f].off, sizeof(int64_t) * (nu + 1), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(fl.data(), fa[f].flag, (size_t)nu, hipMemcpyDeviceToHost);
        if (e == hipSuccess && f) e = hipMemcpy(hl.data(), fa[f].hdr_len, sizeof(int32_t) * n_genes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) break;
        T.fallback = (int64_t*)malloc(sizeof(int64_t) * 3 * (size_t)T.n_fallback);
        if (!T.fallback) { e = hipErrorOutOfMemory; break; }
        int64_t k = 0;
        // unit -> gene: GFF units of contig i are its header and then its genes (headers are never flagged)
        int ci = 0;
        for (int64_t u = 0; u < nu && k < T.n_fallback; u++) {
            int64_t gi = u;
            if (f == 0) {
                while (ci + 1 < NC && u >= (ci + 1) + gbeg[ci + 1]) ci++;
                gi = u - ci - 1;
            }
            if (!fl[u]) continue;
            T.fallback[3 * k] = gi;
            T.fallback[3 * k + 1] = off[u];
            T.fallback[3 * k + 2] = f == 0 ? off[u + 1] : off[u] + hl[u];
            k++;
        }
        T.n_fallback = k;
    }
    if (e != hipSuccess) return fail(e);
    for (auto& row : ev) for (auto& x : row) if (x) hipEventDestroy(x);
    for (int f = 0; f < 3; f++)
        if (units[f] < 0) { R->text[f].data = nullptr; free(R->text[f].contig_off); R->text[f].contig_off = nullptr; }
    *out = R;
    return PGA_OK;
#undef BAD
}
