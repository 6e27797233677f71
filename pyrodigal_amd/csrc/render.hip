// Device rendering of gene records into the text the host writers emit: GFF (Genes.write_gff), protein FASTA
// (Genes.write_translations), gene FASTA (Genes.write_genes), GenBank (Genes.write_genbank) and the start-score file
// (Genes.write_scores), contig after contig, byte for byte.
// ref: lib.pyx:3405-3894 (the writers), 2844-2872 (Gene._rbs), gene.c calculate_confidence.
//
// Per format: a length pass (the line renderers run with a counting sink), an exclusive scan of the lengths, and a write pass
// (the same renderers, now writing at the scanned offsets).  One text arena per format, copied back once into pinned memory.
//   GFF            one thread per line: the three header lines of a contig are one unit, every gene line one unit
//   FASTA records  one thread per record header; one wavefront per record body (residues / bases, newline every `width`)
//   GenBank        one thread per contig header (LOCUS .. FEATURES) and per gene's qualifier lines; one wavefront per
//                  /translation block; ORIGIN is one unit per contig whose length has a closed form, written by workgroups
//                  of 10-base blocks
//   start scores   the start nodes the finder kept on the device, sorted into Prodigal's stopcmp_nodes order by a radix sort
//                  over (contig, stop_val, strand) keys (stable: the arena is in ndx order within a contig); one thread per row,
//                  one per contig header
// Numbers are printed by render_fmt.h (exact '%.Nf').  A GFF line whose confidence lies within `fallback_margin` of a rounding
// midpoint is flagged: the device exp may differ from glibc's by an ulp, so the host renders that line itself.
#include "pga_internal.h"
#include "pipeline.h"
#include "render_fmt.h"
#include "translate_rules.h"

#include <hipcub/hipcub.hpp>

#include <string.h>

#include <numeric>

#include <string>
#include <vector>

struct pga_batch_view { pga_ctx* ctx; int32_t n; int64_t total; const ContigDesc* ct; const char* d_seq; const uint8_t* circular /* or nullptr: all linear */; };
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
    const int64_t* seqnum;          // or nullptr: contig c is sequence first_seqnum + c (pga_render_seqnums)
    int32_t header, incl_tt, full_id, width, tt, include_stop, strict;
    int32_t div_off, div_len, date_off, date_len, infv_off, infv_len;     // GenBank strings in the arena
    double margin;
    // GenBank ORIGIN: workgroup w of k_gbk_origin works on contig c for w in [org_wg0[c], org_wg0[c + 1])
    const int64_t* org_wg0;
    // start scores: the kept node arrays, arena offset / nodes of every contig and their prefix in contig order, the sorted
    // (key, arena index) pairs of all nodes (start nodes first, contig-major), and srow[c]: the first sorted row of contig c
    DevNodeArrays nd;
    const int64_t* naoff; const int64_t* ncum;
    uint64_t* skey; uint32_t* sval; uint64_t* skey2; uint32_t* sval2;
    int64_t* srow;
    int64_t n_nodes;
    int64_t* len;          // length pass: [n_units + 1] line / record lengths (the last one 0)
    int64_t* off;          // their exclusive scan: where every unit starts; off[n_units] = the text's size
    int32_t* hdr_len;      // FASTA: [n_genes] header line length of every record
    uint8_t* flag;         // [n_units] 1: the host renders this unit
    unsigned long long* n_flag;
    char* out;
};

__device__ __forceinline__ int64_t seqnum_of(const RenderArgs& a, const int c) { return a.seqnum ? a.seqnum[c] : a.first_seqnum + c; }
__device__ __forceinline__ void put_id(Sink& o, const RenderArgs& a, const int c) {
    o.put_n(a.str + a.id_off[c], a.id_off[c + 1] - a.id_off[c]);
}

// the four-way rule of Gene._rbs (lib.pyx:951-969) and write_scores (1302-1315): the RBS site whose motif and spacer print, or -1
// (then the upstream motif itself, or None when there is none)
__device__ __forceinline__ int rbs_site(const RenderModel& m, const int k0, const int k1, const double mot_score) {
    const double st = m.st_wt;
    const double r1 = m.rbs_wt[k0] * st, r2 = m.rbs_wt[k1] * st, ms = mot_score * st;
    if (m.uses_sd) return r1 > r2 ? k0 : k1;
    if (m.no_mot > -0.5 && r1 > r2 && r1 > ms) return k0;
    if (m.no_mot > -0.5 && r2 >= r1 && r2 > ms) return k1;
    return -1;
}

// "".join("AGCT"[(mot_ndx >> (2 * i)) & 3] for i in range(mot_len)), Python's arithmetic shift of any width
__device__ __forceinline__ void put_motif(Sink& o, const int mot_len, const int32_t mot_ndx) {
    for (int i = 0; i < mot_len; i++) {
        const int s = 2 * i;
        const int d = s < 32 ? (mot_ndx >> s) & 3 : (mot_ndx < 0 ? 3 : 0);
        o.put("AGCT"[d]);
    }
}

// Gene._gene_data (lib.pyx:1091-1095): ID=..;partial=..;start_type=..;rbs_motif=..;rbs_spacer=..;gc_cont=..
__device__ bool gene_data(Sink& o, const RenderArgs& a, const pga_gene& g, const int c, const int64_t k, const int full_id) {
    o.puts("ID=");
    if (full_id) put_id(o, a, c); else pga_fmt::put_i64(o, seqnum_of(a, c));
    o.put('_'); pga_fmt::put_i64(o, k + 1);
    o.puts(";partial="); o.put((char)('0' + (g.partial_begin ? 1 : 0))); o.put((char)('0' + (g.partial_end ? 1 : 0)));
    o.puts(";start_type="); o.puts(c_node_type[g.start_type & 3]);
    // Gene._rbs (lib.pyx:951-969)
    const int site = rbs_site(a.models[a.moc[c]], g.rbs[0], g.rbs[1], g.mot_score);
    o.puts(";rbs_motif=");
    if (site >= 0) {
        o.puts(c_rbs_motif[site]); o.puts(";rbs_spacer="); o.puts(c_rbs_spacer[site]);
    } else if (g.mot_len == 0) {
        o.puts("None;rbs_spacer=None");
    } else {
        put_motif(o, g.mot_len, g.mot_ndx);
        o.puts(";rbs_spacer="); pga_fmt::put_i64(o, g.mot_spacer); o.puts("bp");
    }
    o.puts(";gc_cont=");
    return pga_fmt::fmt_fixed(o, (double)g.gc_cont, 3);
}

// the header lines of contig c in write_gff (lib.pyx:1167-1178)
__device__ void gff_header(Sink& o, const RenderArgs& a, const int c) {
    const RenderModel& m = a.models[a.moc[c]];
    if (a.header) o.puts("##gff-version  3\n");
    o.puts("# Sequence Data: seqnum="); pga_fmt::put_i64(o, seqnum_of(a, c));
    o.puts(";seqlen="); pga_fmt::put_i64(o, a.ct[c].len);
    o.puts(";seqhdr=\""); put_id(o, a, c);
    o.puts(a.ct[c]._pad ? "\";topology=circular\n# Model Data: version=" : "\"\n# Model Data: version="); o.put_n(a.str + a.ver_off, a.ver_len);
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
    return pga_fmt::body_letters(g.begin, g.end, g.strand, g.partial_begin, g.partial_end, protein, a.include_stop);
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

__device__ __forceinline__ int wrap_at(const int p, const int slen) { return p >= slen ? p - slen : p; }
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
    const int slen = a.ct[c].len;                     // a gene across the origin of a circular contig reads position p >= slen at p - slen
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
            const int p = g.strand == 1 ? g.begin - 1 + i : g.end - 1 - i;
            ch = base_at(s, p >= slen ? p - slen : p, g.strand != 1);
        } else {
            int x0, x1, x2;
            if (g.strand == 1) {
                const int p = g.begin - 1 + 3 * i;
                x0 = pga_tr::digit_of(s[wrap_at(p, slen)], false); x1 = pga_tr::digit_of(s[wrap_at(p + 1, slen)], false); x2 = pga_tr::digit_of(s[wrap_at(p + 2, slen)], false);
            } else {
                const int p = g.end - 1 - 3 * i;
                x0 = pga_tr::digit_of(s[wrap_at(p, slen)], true); x1 = pga_tr::digit_of(s[wrap_at(p - 1, slen)], true); x2 = pga_tr::digit_of(s[wrap_at(p - 2, slen)], true);
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

// ---- GenBank (Genes.write_genbank, lib.pyx:1219-1268) ----------------------------------------------------------------------
// Units of contig c: its header at 2 c + gene_begin[c], gene g at 2 c + 1 + g, ORIGIN at 2 c + 1 + gene_begin[c + 1].

#define GBK_PAD "                     "     // the 21 columns of a qualifier line
// the closed forms of ORIGIN (its length, where a line starts) and of a /translation block are in render_fmt.h, where the host shim reaches them
using pga_fmt::kOriginLong;
using pga_fmt::origin_len;
using pga_fmt::origin_line_at;
using pga_fmt::gbk_tr_bytes;

__device__ void gbk_header(Sink& o, const RenderArgs& a, const int c) {
    const int64_t slen = a.ct[c].len;
    o.puts("LOCUS       ");
    put_id(o, a, c);
    // '{:<23}' pads to 23 characters: code points of the UTF-8 id, never truncated
    int64_t chars = 0;
    for (int64_t i = a.id_off[c]; i < a.id_off[c + 1]; i++) chars += ((unsigned char)a.str[i] & 0xC0) != 0x80;
    for (; chars < 23; chars++) o.put(' ');
    o.put(' '); pga_fmt::put_i64(o, slen); o.puts(" bp    DNA     linear   ");
    o.put_n(a.str + a.div_off, a.div_len); o.put(' '); o.put_n(a.str + a.date_off, a.date_len); o.put('\n');
    o.puts("REFERENCE   1  (bases 1 to "); pga_fmt::put_i64(o, slen); o.puts(")\n");
    o.puts("  AUTHORS   Hyatt,D., Chen,G-L., LoCascio,P.F., Land,M.L., Larimer,F.W.\n"
           "            Hauser,L.J.\n"
           "  TITLE     Prodigal: prokaryotic gene recognition and translation initiation\n"
           "            site identification\n"
           "  JOURNAL   BMC Bioinformatics. 2010;11:119.\n"
           "   PUBMED   20211023\n"
           "FEATURES             Location/Qualifiers\n");
}

__device__ __forceinline__ int gbk_table(const RenderArgs& a, const int c) { return a.tt > 0 ? a.tt : a.models[a.moc[c]].tt; }

// the CDS line and the qualifiers up to /transl_table of gene gi (k-th of its contig)
__device__ void gbk_gene_head(Sink& o, const RenderArgs& a, const pga_gene& g, const int c, const int64_t k) {
    const bool start_edge = g.strand == 1 ? g.partial_begin : g.partial_end;
    const bool stop_edge = g.strand == 1 ? g.partial_end : g.partial_begin;
    o.puts("     CDS             ");
    if (g.strand != 1) o.puts("complement(");
    if (start_edge) o.put('<');
    pga_fmt::put_i64(o, g.begin); o.puts("..");
    if (stop_edge) o.put('>');
    pga_fmt::put_i64(o, g.end);
    if (g.strand != 1) o.put(')');
    o.puts("\n" GBK_PAD "/codon_start=1\n" GBK_PAD "/inference=\"ab initio prediction:pyrodigal_amd:");
    o.put_n(a.str + a.infv_off, a.infv_len);
    o.puts("\"\n" GBK_PAD "/locus_tag=\""); put_id(o, a, c); o.put('_'); pga_fmt::put_i64(o, k + 1);
    o.puts("\"\n" GBK_PAD "/transl_table="); pga_fmt::put_i64(o, gbk_table(a, c)); o.put('\n');
}

// '/translation="<protein without its stop>"' wrapped by textwrap.wrap(_, 59) (no whitespace in it: 59-character pieces), every
// piece on a qualifier line: 21 spaces + piece + newline
__device__ __forceinline__ int64_t gbk_tr_chars(const RenderArgs& a, const pga_gene& g) { return 15 + body_len(a, g, 1); }

__global__ void __launch_bounds__(256) k_gbk(const RenderArgs a, const int write) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int NC = a.n_contigs;
    if (idx >= 2 * (int64_t)NC + a.n_genes) return;
    int64_t u;
    Sink o{nullptr, 0};
    int64_t extra = 0;
    if (idx < NC) {
        const int c = (int)idx;
        u = 2 * c + a.gene_begin[c];
        o.p = write ? a.out + a.off[u] : nullptr;
        gbk_header(o, a, c);
    } else if (idx < 2 * (int64_t)NC) {
        const int c = (int)(idx - NC);
        u = 2 * c + 1 + a.gene_begin[c + 1];
        const int64_t L = origin_len(a.ct[c].len);
        if (write) {          // the lines in between: k_gbk_origin
            char* p = a.out + a.off[u];
            const char* h = "ORIGIN\n";
            for (int i = 0; i < 7; i++) p[i] = h[i];
            p[L - 3] = '/'; p[L - 2] = '/'; p[L - 1] = '\n';
        }
        o.n = L;
    } else {
        const int64_t gi = idx - 2 * (int64_t)NC;
        const pga_gene g = a.genes[gi];
        const int c = g.contig;
        u = 2 * (int64_t)c + 1 + gi;
        o.p = write ? a.out + a.off[u] : nullptr;
        gbk_gene_head(o, a, g, c, gi - a.gene_begin[c]);
        if (!write) a.hdr_len[gi] = (int32_t)o.n;
        extra = gbk_tr_bytes(gbk_tr_chars(a, g));
    }
    if (!write) { a.len[u] = o.n + extra; a.flag[u] = 0; }
}

// the /translation block of every gene: one wavefront per gene, lane l writes characters l, l + 64, ... of the wrapped string
__global__ void __launch_bounds__(256) k_gbk_tr(const RenderArgs a) {
    const int64_t gi = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (gi >= a.n_genes) return;
    const pga_gene g = a.genes[gi];
    const int c = g.contig;
    const char* __restrict__ s = a.seq + a.ct[c].base;
    const int L = (int)gbk_tr_chars(a, g);
    char* __restrict__ out = a.out + a.off[2 * (int64_t)c + 1 + gi] + a.hdr_len[gi];
    const int tt = gbk_table(a, c);
    const char* row = a.code + 64 * tt;
    const bool start_edge = g.strand == 1 ? g.partial_begin : g.partial_end;
    const char* head = "/translation=\"";
    for (int p = lane; p < L; p += 64) {
        char ch;
        if (p < 14) ch = head[p];
        else if (p == L - 1) ch = '"';
        else {
            const int i = p - 14;
            int x0, x1, x2;
            if (g.strand == 1) {
                const int q = g.begin - 1 + 3 * i;
                x0 = pga_tr::digit_of(s[q], false); x1 = pga_tr::digit_of(s[q + 1], false); x2 = pga_tr::digit_of(s[q + 2], false);
            } else {
                const int q = g.end - 1 - 3 * i;
                x0 = pga_tr::digit_of(s[q], true); x1 = pga_tr::digit_of(s[q - 1], true); x2 = pga_tr::digit_of(s[q - 2], true);
            }
            ch = pga_tr::translate_codon(row, x0, x1, x2, tt, i, start_edge, a.strict, 'X');
        }
        const int k = p / 59, col = p - 59 * k;
        char* line = out + (int64_t)k * 81;          // 21 + 59 + 1 bytes per full line
        if (col == 0) for (int j = 0; j < 21; j++) line[j] = ' ';
        line[21 + col] = ch;
        if (col == 58 || p == L - 1) line[22 + col] = '\n';
    }
}

// the ORIGIN lines: a thread per ten-base block (' ' + the bases in lower case, anything but ACGT as 'n'); the first block of a
// line writes the position before it, the last one the newline after it.  A workgroup covers 2 048 blocks of one contig.
constexpr int kOriginBlocksPerWG = 2048;
__global__ void __launch_bounds__(256) k_gbk_origin(const RenderArgs a) {
    __shared__ int s_c;
    const int64_t w = blockIdx.x;
    if (threadIdx.x == 0) {            // the contig of this workgroup: last c with org_wg0[c] <= w
        int lo = 0, hi = a.n_contigs - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.org_wg0[mid] <= w) lo = mid; else hi = mid - 1; }
        s_c = lo;
    }
    __syncthreads();
    const int c = s_c;
    const int64_t n = a.ct[c].len;
    const int64_t nblk = (n + 9) / 10;
    const char* __restrict__ s = a.seq + a.ct[c].base;
    char* __restrict__ out = a.out + a.off[2 * (int64_t)c + 1 + a.gene_begin[c + 1]];
    const int64_t b0 = (w - a.org_wg0[c]) * kOriginBlocksPerWG;
    for (int j = threadIdx.x; j < kOriginBlocksPerWG; j += blockDim.x) {
        const int64_t b = b0 + j;
        if (b >= nblk) break;
        const int64_t k = b / 6;
        const int q = (int)(b - 6 * k);
        const int wk = k >= kOriginLong ? 10 : 9;
        char* line = out + origin_line_at(k);
        if (q == 0) {
            const int64_t pos = 60 * k + 1;
            int nd = 1;
            for (int64_t t = pos; t >= 10; t /= 10) nd++;
            Sink o{line, 0};
            for (int i = nd; i < wk; i++) o.put(' ');
            pga_fmt::put_i64(o, pos);
        }
        char* blk = line + wk + 11 * q;
        const int64_t p0 = 10 * b;
        const int nb = (int)(n - p0 < 10 ? n - p0 : 10);
        blk[0] = ' ';
        for (int i = 0; i < nb; i++) blk[1 + i] = (char)(base_at(s, p0 + i, false) + 32);
        if (q == 5 || b == nblk - 1) blk[1 + nb] = '\n';
    }
}

// ---- start scores (Genes.write_scores, lib.pyx:1270-1318) ------------------------------------------------------------------
// Units of contig c: its header at c + srow[c] (with the final blank line when the contig has no start node), row r at
// contig + 1 + r.  Rows r >= srow[n_contigs] (the stop nodes, sorted last) are empty units at n_contigs + r.

// the sort key of every kept node (pga_node_order_key) and its arena index
__global__ void __launch_bounds__(256) k_sco_keys(const NodeOrder a) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= a.n_nodes) return;
    int lo = 0, hi = a.n_contigs - 1;           // last c with ncum[c] <= v
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (a.ncum[mid] <= v) lo = mid; else hi = mid - 1; }
    const int64_t x = a.naoff[lo] + (v - a.ncum[lo]);
    a.skey[v] = pga_node_order_key(a.n_contigs, lo, a.nd.type[x], a.nd.stop_val[x], a.nd.strand[x]);
    a.sval[v] = (uint32_t)x;
}

// srow[c] = first sorted row of contig c, srow[n_contigs] = start nodes in all (every entry is written by exactly one thread)
__global__ void __launch_bounds__(256) k_sco_bounds(const NodeOrder a) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > a.n_nodes) return;
    const int64_t cr = r < a.n_nodes ? (int64_t)(a.skey[r] >> 33) : a.n_contigs;
    const int64_t cp = r == 0 ? -1 : (int64_t)(a.skey[r - 1] >> 33);
    for (int64_t k = cp + 1; k <= cr; k++) a.srow[k] = r;
}

__device__ void sco_header(Sink& o, const RenderArgs& a, const int c) {
    const RenderModel& m = a.models[a.moc[c]];
    o.puts("# Sequence Data: seqnum="); pga_fmt::put_i64(o, seqnum_of(a, c));
    o.puts(";seqlen="); pga_fmt::put_i64(o, a.ct[c].len);
    o.puts(";seqhdr=\""); put_id(o, a, c);
    o.puts("\"\n# Run Data: version="); o.put_n(a.str + a.ver_off, a.ver_len);
    o.puts(";gc_cont="); pga_fmt::fmt_fixed(o, m.gc * 100, 2);
    o.puts(";transl_table="); pga_fmt::put_i64(o, m.tt);
    o.puts(";uses_sd="); o.put(m.uses_sd ? '1' : '0');
    o.puts("\nBeg\tEnd\tStd\tTotal\tCodPot\tStrtSc\tCodon\tRBSMot\tSpacer\tRBSScr\tUpsScr\tTypeScr\tGCCont\n");
}

// one row of write_scores (lib.pyx:1295-1316): the start node at arena index x
__device__ bool sco_row(Sink& o, const RenderArgs& a, const int c, const int64_t x) {
    const DevNodeArrays& N = a.nd;
    const int32_t ndx = N.ndx[x], sv = N.stop_val[x];
    bool ok = true;
    if (N.strand[x] == 1) {
        pga_fmt::put_i64(o, (int64_t)ndx + 1); o.put('\t'); pga_fmt::put_i64(o, (int64_t)sv + 3); o.puts("\t+\t");
    } else {
        pga_fmt::put_i64(o, (int64_t)sv - 1); o.put('\t'); pga_fmt::put_i64(o, (int64_t)ndx + 1); o.puts("\t-\t");
    }
    const double cs = N.cscore[x], ss = N.sscore[x];
    ok &= pga_fmt::fmt_fixed(o, cs + ss, 2); o.put('\t');
    ok &= pga_fmt::fmt_fixed(o, cs, 2); o.put('\t');
    ok &= pga_fmt::fmt_fixed(o, ss, 2); o.put('\t');
    o.puts(c_node_type[N.edge[x] ? 3 : (N.type[x] & 3)]); o.put('\t');
    const int r0 = N.rbs[2 * x] < 28 ? N.rbs[2 * x] : 27, r1 = N.rbs[2 * x + 1] < 28 ? N.rbs[2 * x + 1] : 27;
    const int site = rbs_site(a.models[a.moc[c]], r0, r1, N.mot_score[x]);
    if (site >= 0) { o.puts(c_rbs_motif[site]); o.put('\t'); o.puts(c_rbs_spacer[site]); }
    else if (N.mot_len[x] == 0) o.puts("None\tNone");
    else { put_motif(o, N.mot_len[x], N.mot_ndx[x]); o.put('\t'); pga_fmt::put_i64(o, N.mot_spacer[x]); o.puts("bp"); }
    o.put('\t'); ok &= pga_fmt::fmt_fixed(o, N.rscore[x], 2);
    o.put('\t'); ok &= pga_fmt::fmt_fixed(o, N.uscore[x], 2);
    o.put('\t'); ok &= pga_fmt::fmt_fixed(o, N.tscore[x], 2);
    o.put('\t'); ok &= pga_fmt::fmt_fixed(o, (double)N.gc_cont[x], 3);
    o.put('\n');
    return ok;
}

__global__ void __launch_bounds__(256) k_sco(const RenderArgs a, const int write) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int NC = a.n_contigs;
    if (idx >= NC + a.n_nodes) return;
    const int64_t n_rows = a.srow[NC];
    int64_t u;
    bool ok = true;
    Sink o{nullptr, 0};
    if (idx < NC) {
        const int c = (int)idx;
        u = c + a.srow[c];
        o.p = write ? a.out + a.off[u] : nullptr;
        if (a.header) sco_header(o, a, c);
        if (a.srow[c + 1] == a.srow[c]) o.put('\n');
    } else {
        const int64_t r = idx - NC;
        if (r >= n_rows) {                   // a stop node: an empty unit
            if (!write) { a.len[idx] = 0; a.flag[idx] = 0; }
            return;
        }
        const uint64_t key = a.skey[r];
        const int c = (int)(key >> 33);
        u = c + 1 + r;
        o.p = write ? a.out + a.off[u] : nullptr;
        if (r == a.srow[c] || key != a.skey[r - 1]) o.put('\n');      // a new (stop_val, strand) group
        ok = sco_row(o, a, c, a.sval[r]);
        if (r + 1 == a.srow[c + 1]) o.put('\n');                        // the blank line after the contig's last row
    }
    if (!write) {
        a.len[u] = o.n;
        a.flag[u] = ok ? 0 : 1;
        if (!ok) atomicAdd(a.n_flag, 1ull);
    }
}

// contig i's first byte: the first unit of the contig, unit mul * i + begin[i] (its header or its first record);
// off[n_units] = total
__global__ void k_contig_off(const int64_t* __restrict__ off, const int64_t* __restrict__ begin, const int n_contigs,
                             const int64_t n_units, const int mul, int64_t* __restrict__ out) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c > n_contigs) return;
    out[c] = c == n_contigs ? off[n_units] : off[(int64_t)mul * c + begin[c]];
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

hipError_t pga_render_scratch(pga_ctx* c, const size_t bytes, char** d) {
    const hipError_t e = grow(c->render_dev, c->render_dev_cap, bytes, false);
    *d = c->render_dev;
    return e;
}

// ---- the kept nodes in stopcmp_nodes order: keys, a stable radix sort, where every contig's rows begin ----
static int node_order_bits(const int n_contigs) {
    int bits = 33;
    while (bits < 64 && ((uint64_t)n_contigs >> (bits - 33)) != 0) bits++;
    return bits;
}

size_t pga_node_order_temp_bytes(const int64_t n_nodes, const int n_contigs, hipStream_t st) {
    size_t b = 0;
    if (n_nodes > 0)
        hipcub::DeviceRadixSort::SortPairs(nullptr, b, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                           (int)n_nodes, 0, node_order_bits(n_contigs), st);
    return b;
}

hipError_t pga_node_order(NodeOrder& o, void* tmp, size_t tmp_bytes, hipStream_t st) {
    const int64_t NN = o.n_nodes;
    auto blocks = [](const int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    hipError_t e = hipSuccess;
    if (NN > 0) {
        hipLaunchKernelGGL(k_sco_keys, blocks(NN), dim3(256), 0, st, o);
        e = hipGetLastError();
        if (e == hipSuccess)
            e = hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, o.skey, o.skey2, o.sval, o.sval2, (int)NN, 0, node_order_bits(o.n_contigs), st);
        o.skey = o.skey2; o.sval = o.sval2;
    }
    if (e == hipSuccess) { hipLaunchKernelGGL(k_sco_bounds, blocks(NN + 1), dim3(256), 0, st, o); e = hipGetLastError(); }
    return e;
}

const char* pga_dev_nodes_refusal(const pga_ctx* c, const void* batch, const int n_contigs, const ContigDesc* ct, const pga_contig_result* contigs) {
    const DevNodes& DN = c->dev_nodes;
    if (!DN.contigs || (contigs && DN.contigs != contigs) || DN.batch != batch || (int)DN.n.size() != n_contigs)
        return "no node arrays of this result on the device: find the genes with want_nodes = PGA_NODES_DEVICE (or 1), and render "
               "before the next call on the context that runs the finder or loads models";
    for (int i = 0; i < n_contigs; i++)
        if (DN.len[i] != ct[i].len || DN.off[i] < 0 || DN.n[i] < 0 || DN.off[i] + DN.n[i] > DN.total)
            return "the batch is not the one the node arrays were found on";
    if (DN.total >= ((int64_t)1 << 31)) return "more than 2^31 - 1 nodes in one call";
    return nullptr;
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

extern "C" int pga_render_seqnums(pga_ctx* c, int32_t n, const int64_t* seqnum) {
    if (!c || n < 0) return PGA_EINVAL;
    c->render_seqnums.clear();
    if (seqnum && n > 0) c->render_seqnums.assign(seqnum, seqnum + n);
    return PGA_OK;
}

extern "C" int pga_render_genes(pga_ctx* c, const pga_batch* batch, const pga_contig_result* contigs, int64_t n_genes, const pga_gene* genes,
                                const int32_t* model_of_contig, const char* ids, const int64_t* id_off, const pga_render_opts* opts,
                                pga_render_result** out) {
#define BAD(msg) do { c->err = "pga_render_genes: " msg; return PGA_EINVAL; } while (0)
    constexpr int NF = 5;
    if (!c) return PGA_EINVAL;
    if (!batch || !contigs || n_genes < 0 || (n_genes > 0 && !genes) || !model_of_contig || !id_off || !opts || !out) BAD("bad arguments");
    *out = nullptr;
    const pga_batch_view bv = pga_batch_peek(batch);
    if (bv.ctx != c) BAD("the batch belongs to another context");
    const pga_render_opts& O = *opts;
    const int NC = bv.n;
    const bool want_gbk = (O.formats & PGA_RENDER_GBK) != 0, want_sco = (O.formats & PGA_RENDER_SCO) != 0;
    if ((O.formats & ~31) || !O.formats) BAD("`formats` must be a non-empty set of PGA_RENDER_* bits");
    if (((O.formats & PGA_RENDER_FAA) && O.faa_width < 1) || ((O.formats & PGA_RENDER_FNA) && O.fna_width < 1)) BAD("`width` must be at least 1");
    if ((O.formats & PGA_RENDER_FAA) && O.faa_translation_table != 0 && !pga_tr::table_known(O.faa_translation_table))
        BAD("not a valid translation table index");
    if (want_gbk && O.gbk_translation_table != 0 && !pga_tr::table_known(O.gbk_translation_table)) BAD("not a valid translation table index");
    if (want_gbk && (!O.gbk_division || !O.gbk_date || !O.gbk_version)) BAD("missing GenBank strings (division, date, version)");
    if (!O.source || !O.version || (c->n_models > 0 && !O.model_desc)) BAD("missing tool strings");
    if (!(O.fallback_margin >= 0)) BAD("`fallback_margin` must be >= 0");
    // circular contigs: their nodes live in the rotated contig's coordinates, and GenBank locations across the origin are the host writer's
    if (bv.circular && want_sco) BAD("the start-score file is not written for circular contigs (the batch carries pga_batch_set_circular flags)");
    if (bv.circular && want_gbk) BAD("GenBank records of circular contigs are written by the host writer (the batch carries pga_batch_set_circular flags)");
    // the start-score file reads the node arrays the last finder call kept on the device: only for that result and batch
    const DevNodes& DN = c->dev_nodes;
    if (want_sco)
        if (const char* why = pga_dev_nodes_refusal(c, batch, NC, bv.ct, contigs)) { c->err = std::string("pga_render_genes: ") + why; return PGA_EINVAL; }
    // the layout the kernels rely on: genes of contig i are genes[gene_begin .. + n_genes), contig after contig, inside the contig
    int64_t run = 0;
    std::vector<int64_t> gbeg((size_t)NC + 1);
    for (int i = 0; i < NC; i++) {
        if (contigs[i].gene_begin != run || contigs[i].n_genes < 0) BAD("contig records do not tile the gene records");
        gbeg[i] = run;
        run += contigs[i].n_genes;
        const int m = model_of_contig[i];
        if (m < -1 || m >= c->n_models) BAD("model index outside the loaded set");
        if (m < 0 && (contigs[i].n_genes > 0 || (O.formats & (PGA_RENDER_GFF | PGA_RENDER_SCO)))) BAD("no model was selected for a contig");
        if (id_off[i + 1] < id_off[i] || id_off[i] < 0) BAD("id offsets are not increasing");
    }
    gbeg[NC] = run;
    if (run != n_genes) BAD("contig records do not tile the gene records");
    if (id_off[0] != 0 || (id_off[NC] > 0 && !ids)) BAD("id offsets must start at 0");
    for (int i = 0; i < NC; i++)
        for (int64_t g = gbeg[i]; g < gbeg[i + 1]; g++) {
            const pga_gene& G = genes[g];
            const bool circ = bv.circular && bv.circular[i];  // a gene across the origin ends beyond the length, and is no longer than the circle
            const bool inside = circ ? G.begin <= bv.ct[i].len && (int64_t)G.end - G.begin < bv.ct[i].len : G.end <= bv.ct[i].len;
            if (G.contig != i || G.begin < 1 || !inside || G.end < G.begin || G.rbs[0] >= 28 || G.rbs[1] >= 28)
                BAD("gene record outside its contig");
        }
    // models and the string arena: ids, then the model descriptions, the source and the version, the GenBank strings
    std::string str(ids ? ids : "", (size_t)id_off[NC]);
    std::vector<RenderModel> models((size_t)std::max(c->n_models, 1));
    for (int m = 0; m < c->n_models; m++) {
        const pga_training& t = c->models[m];
        RenderModel& R = models[m];
        memcpy(R.rbs_wt, t.rbs_wt, sizeof R.rbs_wt);
        R.st_wt = t.st_wt; R.no_mot = t.no_mot; R.gc = t.gc; R.tt = t.trans_table; R.uses_sd = t.uses_sd != 0;
        const char* d = O.model_desc[m] ? O.model_desc[m] : "";
        R.desc_off = (int32_t)str.size(); R.desc_len = (int32_t)strlen(d); str += d;
        if (!pga_tr::table_known(R.tt) && ((O.formats & PGA_RENDER_FAA) || (want_gbk && O.gbk_translation_table == 0)))
            BAD("a loaded model has an unknown translation table");
        if (!(t.gc >= 0 && t.gc <= 1) || !(t.st_wt != 0)) BAD("a loaded model has no GC content or start weight");
    }
    auto add_str = [&](const char* x, int32_t& off, int32_t& len) { off = (int32_t)str.size(); len = (int32_t)strlen(x ? x : ""); str += x ? x : ""; };
    int32_t src_off, src_len, ver_off, ver_len, div_off = 0, div_len = 0, date_off = 0, date_len = 0, infv_off = 0, infv_len = 0;
    add_str(O.source, src_off, src_len);
    add_str(O.version, ver_off, ver_len);
    if (want_gbk) { add_str(O.gbk_division, div_off, div_len); add_str(O.gbk_date, date_off, date_len); add_str(O.gbk_version, infv_off, infv_len); }
    static const CodeTables tables;         // built once (thread-safe static initialisation)
    const auto& code = tables.code;
    // GenBank ORIGIN: workgroups of every contig
    std::vector<int64_t> org_wg0((size_t)NC + 1, 0);
    for (int i = 0; i < NC; i++) org_wg0[i + 1] = org_wg0[i] + ((bv.ct[i].len + 9) / 10 + kOriginBlocksPerWG - 1) / kOriginBlocksPerWG;
    // start scores: arena offsets of the contigs and their node counts' prefix, in contig order
    const int64_t NN = want_sco ? std::accumulate(DN.n.begin(), DN.n.end(), (int64_t)0) : 0;
    std::vector<int64_t> naoff((size_t)NC + 1, 0), ncum((size_t)NC + 1, 0);
    if (want_sco)
        for (int i = 0; i < NC; i++) { naoff[i] = DN.off[i]; ncum[i + 1] = ncum[i] + DN.n[i]; }

    pga_render_result* R = new pga_render_result();
    R->n_contigs = NC;
    if (hipSetDevice(c->device) != hipSuccess) { delete R; return PGA_EDEVICE; }
    hipStream_t st = c->stream;
    const int fmts[NF] = {PGA_RENDER_GFF, PGA_RENDER_FAA, PGA_RENDER_FNA, PGA_RENDER_GBK, PGA_RENDER_SCO};
    int64_t units[NF];
    for (int f = 0; f < NF; f++) {
        const int64_t u[NF] = {NC + n_genes, n_genes, n_genes, 2 * (int64_t)NC + n_genes, NC + NN};
        units[f] = (O.formats & fmts[f]) ? u[f] : -1;
    }
    // one device allocation for everything but the text: inputs, then per format lengths / offsets, flags, header lengths
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    size_t o_genes = 0, o_ct = o_genes + al(sizeof(pga_gene) * (size_t)std::max<int64_t>(n_genes, 1));
    size_t o_gb = o_ct + al(sizeof(ContigDesc) * (NC + 1)), o_moc = o_gb + al(sizeof(int64_t) * (NC + 1));
    size_t o_mod = o_moc + al(sizeof(int32_t) * (NC + 1)), o_idoff = o_mod + al(sizeof(RenderModel) * models.size());
    size_t o_str = o_idoff + al(sizeof(int64_t) * (NC + 1)), o_code = o_str + al(str.size() + 1);
    size_t o_cnt = o_code + al(sizeof code), o_wg0 = o_cnt + al(sizeof(unsigned long long) * 8);
    size_t o_naoff = o_wg0 + al(sizeof(int64_t) * (NC + 1)), o_ncum = o_naoff + al(sizeof(int64_t) * (NC + 1));
    size_t o_srow = o_ncum + al(sizeof(int64_t) * (NC + 1)), o_seqn = o_srow + al(sizeof(int64_t) * (NC + 1));
    size_t o_skey = o_seqn + al(sizeof(int64_t) * (NC + 1));
    const bool own_seqnums = NC > 0 && (int)c->render_seqnums.size() == NC;
    const size_t nn1 = (size_t)std::max<int64_t>(NN, 1);
    size_t o_sval = o_skey + al(sizeof(uint64_t) * 2 * nn1), o_f = o_sval + al(sizeof(uint32_t) * 2 * nn1);
    size_t o_len[NF], o_off[NF], o_flag[NF], o_hdr[NF], o_coff[NF];
    size_t scan_bytes = 0, o_tmp;
    for (int f = 0; f < NF; f++) {
        const int64_t nu = std::max<int64_t>(units[f], 0);
        o_len[f] = o_f; o_f += al(sizeof(int64_t) * (nu + 1));
        o_off[f] = o_f; o_f += al(sizeof(int64_t) * (nu + 1));
        o_flag[f] = o_f; o_f += al((size_t)nu + 1);
        o_hdr[f] = o_f; o_f += al(sizeof(int32_t) * (size_t)(f >= 1 && f <= 3 ? std::max<int64_t>(n_genes, 1) : 1));
        o_coff[f] = o_f; o_f += al(sizeof(int64_t) * (NC + 1));
        if (units[f] >= 0) {
            size_t b = 0;
            hipcub::DeviceScan::ExclusiveSum(nullptr, b, (int64_t*)nullptr, (int64_t*)nullptr, (int)(units[f] + 1), st);
            scan_bytes = std::max(scan_bytes, b);
        }
    }
    if (want_sco) scan_bytes = std::max(scan_bytes, pga_node_order_temp_bytes(NN, NC, st));
    o_tmp = o_f; o_f += al(scan_bytes + 1);
    char* d = nullptr;
    char* d_text = nullptr;
    unsigned long long* h_small = nullptr;
    hipEvent_t ev[NF][4] = {};
    auto fail = [&](hipError_t e) {
        hipStreamSynchronize(st);
        for (auto& row : ev) for (auto& x : row) if (x) hipEventDestroy(x);
        pga_render_free(R);
        return pga_hip_try_(c, e, "pga_render_genes");
    };
    hipError_t e = grow(c->render_dev, c->render_dev_cap, o_f, false);
    d = c->render_dev;
    if (e == hipSuccess && !c->render_small) e = hipHostMalloc((void**)&c->render_small, sizeof(unsigned long long) * 16, hipHostMallocDefault);
    h_small = c->render_small;
    for (int f = 0; f < NF && e == hipSuccess; f++)
        for (int k = 0; k < 4 && e == hipSuccess; k++) e = hipEventCreate(&ev[f][k]);
    if (e != hipSuccess) return fail(e);
    if (n_genes > 0) e = hipMemcpyAsync(d + o_genes, genes, sizeof(pga_gene) * (size_t)n_genes, hipMemcpyHostToDevice, st);
    // (the copy of the contig table the kernels read carries the topology in its spare field: 1 = circular)
    std::vector<ContigDesc> ctv(bv.ct, bv.ct + NC + 1);
    if (bv.circular) for (int i = 0; i < NC; i++) ctv[i]._pad = bv.circular[i] ? 1 : 0;
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_ct, ctv.data(), sizeof(ContigDesc) * (NC + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_gb, gbeg.data(), sizeof(int64_t) * (NC + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && NC > 0) e = hipMemcpyAsync(d + o_moc, model_of_contig, sizeof(int32_t) * NC, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_mod, models.data(), sizeof(RenderModel) * models.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_idoff, id_off, sizeof(int64_t) * (NC + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_str, str.c_str(), str.size() + 1, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d + o_code, code, sizeof code, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d + o_cnt, 0, sizeof(unsigned long long) * 8, st);
    if (e == hipSuccess && want_gbk) e = hipMemcpyAsync(d + o_wg0, org_wg0.data(), sizeof(int64_t) * (NC + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && want_sco) e = hipMemcpyAsync(d + o_naoff, naoff.data(), sizeof(int64_t) * (NC + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && want_sco) e = hipMemcpyAsync(d + o_ncum, ncum.data(), sizeof(int64_t) * (NC + 1), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && own_seqnums) e = hipMemcpyAsync(d + o_seqn, c->render_seqnums.data(), sizeof(int64_t) * NC, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(e);

    RenderArgs A{};
    A.seq = bv.d_seq; A.ct = (const ContigDesc*)(d + o_ct); A.genes = (const pga_gene*)(d + o_genes);
    A.gene_begin = (const int64_t*)(d + o_gb); A.moc = (const int32_t*)(d + o_moc); A.models = (const RenderModel*)(d + o_mod);
    A.str = d + o_str; A.id_off = (const int64_t*)(d + o_idoff); A.code = d + o_code;
    A.src_off = src_off; A.src_len = src_len; A.ver_off = ver_off; A.ver_len = ver_len;
    A.div_off = div_off; A.div_len = div_len; A.date_off = date_off; A.date_len = date_len; A.infv_off = infv_off; A.infv_len = infv_len;
    A.n_contigs = NC; A.meta = O.meta; A.n_genes = n_genes; A.first_seqnum = O.first_seqnum; A.margin = O.fallback_margin;
    A.org_wg0 = (const int64_t*)(d + o_wg0);
    A.seqnum = own_seqnums ? (const int64_t*)(d + o_seqn) : nullptr;
    if (want_sco) A.nd = DN.a;
    A.naoff = (const int64_t*)(d + o_naoff); A.ncum = (const int64_t*)(d + o_ncum);
    A.skey = (uint64_t*)(d + o_skey); A.skey2 = A.skey + nn1; A.sval = (uint32_t*)(d + o_sval); A.sval2 = A.sval + nn1;
    A.srow = (int64_t*)(d + o_srow); A.n_nodes = NN;
    RenderArgs fa[NF];
    for (int f = 0; f < NF; f++) {
        RenderArgs& a = fa[f];
        a = A;
        a.len = (int64_t*)(d + o_len[f]); a.off = (int64_t*)(d + o_off[f]); a.flag = (uint8_t*)(d + o_flag[f]); a.hdr_len = (int32_t*)(d + o_hdr[f]);
        a.n_flag = (unsigned long long*)(d + o_cnt) + f;
        if (f == 0) { a.header = O.gff_header; a.incl_tt = O.gff_include_translation_table; a.full_id = O.gff_full_id; a.width = 1; }
        if (f == 1) { a.width = O.faa_width; a.tt = O.faa_translation_table; a.include_stop = O.faa_include_stop; a.strict = O.faa_strict; a.full_id = O.faa_full_id; }
        if (f == 2) { a.width = O.fna_width; a.full_id = O.fna_full_id; a.include_stop = 1; a.strict = 1; }
        if (f == 3) { a.width = 59; a.tt = O.gbk_translation_table; a.include_stop = 0; a.strict = O.gbk_strict; }
        if (f == 4) { a.header = O.sco_header; }
    }
    auto blocks = [](const int64_t n) { return dim3((unsigned)((n + 255) / 256)); };
    // length passes and scans
    for (int f = 0; f < NF && e == hipSuccess; f++) {
        if (units[f] < 0) continue;
        RenderArgs& a = fa[f];
        e = hipEventRecord(ev[f][0], st);
        if (e == hipSuccess) e = hipMemsetAsync(a.len + units[f], 0, sizeof(int64_t), st);
        if (e == hipSuccess && f == 4) {
            // the rows in stopcmp_nodes order (pga_node_order)
            NodeOrder no{a.nd, a.naoff, a.ncum, a.skey, a.sval, a.skey2, a.sval2, a.srow, NN, NC};
            e = pga_node_order(no, d + o_tmp, scan_bytes, st);
            a.skey = no.skey; a.sval = no.sval;
        }
        if (e == hipSuccess && units[f] > 0) {
            if (f == 0) hipLaunchKernelGGL(k_gff, blocks(units[f]), dim3(256), 0, st, a, 0);
            else if (f <= 2) hipLaunchKernelGGL(k_fa_head, blocks(units[f]), dim3(256), 0, st, a, f == 1 ? 1 : 0, 0);
            else if (f == 3) hipLaunchKernelGGL(k_gbk, blocks(units[f]), dim3(256), 0, st, a, 0);
            else hipLaunchKernelGGL(k_sco, blocks(units[f]), dim3(256), 0, st, a, 0);
            e = hipGetLastError();
        }
        size_t tb = scan_bytes;
        if (e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(d + o_tmp, tb, a.len, a.off, (int)(units[f] + 1), st);
        if (e == hipSuccess) e = hipEventRecord(ev[f][1], st);
        if (e == hipSuccess) e = hipMemcpyAsync(h_small + f, a.off + units[f], sizeof(int64_t), hipMemcpyDeviceToHost, st);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h_small + 8, d + o_cnt, sizeof(unsigned long long) * NF, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(e);
    int64_t total[NF], toff[NF], tsum = 0;
    for (int f = 0; f < NF; f++) { total[f] = units[f] < 0 ? 0 : (int64_t)h_small[f]; toff[f] = tsum; tsum += total[f]; }
    if (tsum > 0) e = grow(c->render_text, c->render_text_cap, (size_t)tsum, false);
    if (e == hipSuccess && tsum > 0) e = grow(c->render_host, c->render_host_cap, (size_t)tsum, true);
    if (e != hipSuccess) return fail(e);
    d_text = c->render_text;
    // write passes, contig offsets, copies back
    for (int f = 0; f < NF && e == hipSuccess; f++) {
        if (units[f] < 0) continue;
        RenderArgs& a = fa[f];
        a.out = d_text + toff[f];
        e = hipEventRecord(ev[f][2], st);
        if (e == hipSuccess && units[f] > 0) {
            const unsigned nb = (unsigned)((units[f] + 255) / 256);
            if (f == 0) hipLaunchKernelGGL(k_gff, dim3(nb), dim3(256), 0, st, a, 1);
            else if (f <= 2) {
                hipLaunchKernelGGL(k_fa_head, dim3(nb), dim3(256), 0, st, a, f == 1 ? 1 : 0, 1);
                hipLaunchKernelGGL(k_fa_body, dim3((unsigned)((n_genes + 3) / 4)), dim3(256), 0, st, a, f == 1 ? 1 : 0);
            } else if (f == 3) {
                hipLaunchKernelGGL(k_gbk, dim3(nb), dim3(256), 0, st, a, 1);
                if (n_genes > 0) hipLaunchKernelGGL(k_gbk_tr, dim3((unsigned)((n_genes + 3) / 4)), dim3(256), 0, st, a);
                if (org_wg0[NC] > 0) hipLaunchKernelGGL(k_gbk_origin, dim3((unsigned)org_wg0[NC]), dim3(256), 0, st, a);
            } else hipLaunchKernelGGL(k_sco, dim3(nb), dim3(256), 0, st, a, 1);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipEventRecord(ev[f][3], st);
        int64_t* d_coff = (int64_t*)(d + o_coff[f]);
        if (e == hipSuccess) {
            const int mul[NF] = {1, 0, 0, 2, 1};
            hipLaunchKernelGGL(k_contig_off, dim3((unsigned)((NC + 1 + 255) / 256)), dim3(256), 0, st, (const int64_t*)a.off,
                               f == 4 ? (const int64_t*)A.srow : A.gene_begin, NC, units[f], mul[f], d_coff);
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
    // flagged units (rare): their gene index and byte range.  GenBank prints no fraction; a start-score row flags only a value the
    // exact printer does not cover (non-finite), and is reported as a count without ranges
    for (int f = 0; f < NF && e == hipSuccess; f++) {
        if (units[f] < 0) continue;
        pga_text& T = R->text[f];
        T.n_fallback = (int64_t)h_small[8 + f];
        float ms_a = 0, ms_b = 0;
        hipEventElapsedTime(&ms_a, ev[f][0], ev[f][1]);
        hipEventElapsedTime(&ms_b, ev[f][2], ev[f][3]);
        R->t_kernels_ms[f] = (double)ms_a + (double)ms_b;
        if (T.n_fallback == 0 || f >= 3) continue;
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
    for (int f = 0; f < NF; f++)
        if (units[f] < 0) { R->text[f].data = nullptr; free(R->text[f].contig_off); R->text[f].contig_off = nullptr; }
    *out = R;
    return PGA_OK;
#undef BAD
}
