// Host-only build of pyrodigal_amd/csrc/find_plan.h for tests/test_find_plan_cpu.py: flat arrays in, flat arrays out.
// With -DFIND_PLAN_MAIN the file is a stand-alone program that runs a few of the same cases (for a sanitizer build).
#include "../pyrodigal_amd/csrc/find_plan.h"

#include <string.h>

struct Win { int64_t out_off, dp_off, fin_off, topo_off; int32_t n, _pad; };      // as the gather kernel's record (finder.hip)

extern "C" {

int find_plan_dense_sets(const int32_t* labels, int n, int32_t* set_of) {
    std::vector<int32_t> v;
    const int ns = pga_plan::dense_set_ids(labels, n, v);
    if (n > 0) memcpy(set_of, v.data(), sizeof(int32_t) * (size_t)n);
    return ns;
}

// chains out as rows of 8: off, topo_off, n, model, contig, first, group, soff; returns their number, -1: host and device disagree.
// g_c0, g_n0, g_s0: NG + 1 entries each; totals: chain nodes, chain stops.
int64_t find_plan_chains(int NC, int NM, int NG, int meta_run, const int32_t* lens, const int32_t* h_cnt, const int32_t* h_cbase, const int32_t* h_sbase,
                         const uint8_t* h_enabled, const double* model_gc, const int32_t* model_tt, const int32_t* model_group,
                         const int32_t* model_of_contig, const int32_t* cgrp, const int32_t* set_of, int NS,
                         int64_t* rows, int64_t cap, int64_t* g_c0, int64_t* g_n0, int64_t* g_s0, int64_t* totals) {
    std::vector<ContigDesc> ct((size_t)NC + 1);
    int64_t base = 0;
    for (int i = 0; i < NC; i++) { ct[i] = ContigDesc{base, lens[i], 0}; base += lens[i]; }
    ct[NC] = ContigDesc{base, 0, 0};
    std::vector<int> tt(model_tt, model_tt + NM), grp(model_group, model_group + NM), cg;
    if (cgrp) cg.assign(cgrp, cgrp + NC);
    const pga_plan::ChainPlanIn in{NC, NM, NG, meta_run != 0, ct.data(), h_cnt, h_cbase, h_sbase, h_enabled, model_gc, tt.data(), grp.data(),
                                   model_of_contig, cgrp ? cg.data() : nullptr, set_of, NS};
    pga_plan::ChainPlan p;
    if (!pga_plan::plan_chains(in, p)) return -1;
    for (int g = 0; g <= NG; g++) { g_c0[g] = p.g_c0[g]; g_n0[g] = p.g_n0[g]; g_s0[g] = p.g_s0[g]; }
    totals[0] = p.tot_chain_nodes; totals[1] = p.tot_chain_stops;
    for (size_t k = 0; k < p.chains.size() && (int64_t)k < cap; k++) {
        const ChainDesc& c = p.chains[k];
        int64_t* r = rows + 8 * k;
        r[0] = c.off; r[1] = c.topo_off; r[2] = c.n; r[3] = c.model; r[4] = c.contig; r[5] = c.first; r[6] = c.group; r[7] = c.soff;
    }
    return (int64_t)p.chains.size();
}

static std::vector<ChainDesc> chains_of(const int64_t* rows, int n) {
    std::vector<ChainDesc> v((size_t)n);
    for (int k = 0; k < n; k++) {
        const int64_t* r = rows + 8 * (size_t)k;
        ChainDesc c{r[0], r[1], (int32_t)r[2], (int32_t)r[3], (int32_t)r[4], (int32_t)r[5]};
        c.group = (int32_t)r[6]; c.soff = r[7];
        v[(size_t)k] = c;
    }
    return v;
}

// model_scores [NC][NM], set_model / set_score [NC]: prefilled by the caller as the finder does (NaN, -1, NaN)
void find_plan_winners(int NC, int NM, int meta, const int64_t* rows, int NCH, const double* maxscore, const int32_t* ipath, const int32_t* set_of, int NS,
                       double* model_scores, int32_t* set_model, double* set_score, int32_t* win_chain) {
    const std::vector<ChainDesc> ch = chains_of(rows, NCH);
    std::vector<int> w;
    pga_plan::pick_winners(NC, NM, meta != 0, ch.data(), NCH, maxscore, ipath, set_of, NS, model_scores, set_model, set_score, w);
    for (int i = 0; i < NC; i++) win_chain[i] = w[(size_t)i];
}

// re-score chains out as rows of 4: off, raw_off, contig, model; returns their number
int64_t find_plan_rescore(int NC, int NG, int meta, const int64_t* rows, int NCH, const int32_t* win_chain, const uint8_t* h_conv, const int32_t* model_group, int NM,
                          int64_t tot_chain_nodes, int64_t* rs_rows, int64_t* r_c0, int64_t* r_n0, int64_t* fin_off) {
    const std::vector<ChainDesc> ch = chains_of(rows, NCH);
    std::vector<int> w(win_chain, win_chain + NC), grp(model_group, model_group + NM);
    pga_plan::RescorePlan p;
    pga_plan::plan_rescore(NC, NG, meta != 0, ch.data(), w.data(), h_conv, grp.data(), tot_chain_nodes, p);
    for (int g = 0; g <= NG; g++) { r_c0[g] = p.r_c0[g]; r_n0[g] = p.r_n0[g]; }
    for (int i = 0; i < NC; i++) fin_off[i] = p.fin_off[(size_t)i];
    for (size_t k = 0; k < p.rescore.size(); k++) {
        const ChainDesc& c = p.rescore[k];
        int64_t* r = rs_rows + 4 * k;
        r[0] = c.off; r[1] = c.raw_off; r[2] = c.contig; r[3] = c.model;
    }
    return (int64_t)p.rescore.size();
}

// winners out as rows of 6: group, out_off, dp_off, fin_off, topo_off, n (group-major); returns the gathered nodes
int64_t find_plan_gather(int NC, int NG, const int64_t* rows, int NCH, const int32_t* win_chain, const int64_t* fin_off, int64_t* win_rows, int64_t* out_off, int64_t* w_o0) {
    const std::vector<ChainDesc> ch = chains_of(rows, NCH);
    std::vector<int> w(win_chain, win_chain + NC);
    pga_plan::GatherPlan<Win> p;
    pga_plan::plan_gather(NC, NG, ch.data(), w.data(), fin_off, p);
    size_t k = 0;
    for (int g = 0; g < NG; g++) for (const Win& d : p.wg[(size_t)g]) {
        int64_t* r = win_rows + 6 * k++;
        r[0] = g; r[1] = d.out_off; r[2] = d.dp_off; r[3] = d.fin_off; r[4] = d.topo_off; r[5] = d.n;
    }
    for (int i = 0; i < NC; i++) out_off[i] = p.out_off[(size_t)i];
    for (int g = 0; g <= NG; g++) w_o0[g] = p.w_o0[(size_t)g];
    return p.out_nodes;
}

}

#ifdef FIND_PLAN_MAIN
#include <stdio.h>
#include <limits>

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "find_plan: line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    // sets: labels 7, -1, 7, 3, -1 -> 0 1 0 2 3
    { const int32_t lab[5] = {7, -1, 7, 3, -1}; int32_t so[5]; CHECK(find_plan_dense_sets(lab, 5, so) == 4); CHECK(so[0] == 0 && so[1] == 1 && so[2] == 0 && so[3] == 2 && so[4] == 3); }
    // chains: three contigs (one of length 0), three models in two groups; gc of contig 0 = 0.5: low = 0.4322413, high = 0.5461791
    const int NC = 3, NM = 3, NG = 2;
    const int32_t lens[3] = {1000, 0, 1000}, cnt[6] = {500, 0, 900, 0, 0, 0};
    const int32_t cbase[8] = {0, 10, 10, 14, 0, 6, 6, 6}, sbase[8] = {0, 4, 4, 6, 0, 2, 2, 2};
    const uint8_t en[6] = {1, 1, 1, 1, 1, 0};
    const double mgc[3] = {0.88495 * 0.5 - 0.0102337, 0.86596 * 0.5 + 0.1131991, 0.8};
    const int32_t mtt[3] = {11, 4, 11}, mgrp[3] = {0, 1, 0};
    int64_t rows[8 * 16], c0[3], n0[3], s0[3], tot[2];
    const int64_t nch = find_plan_chains(NC, NM, NG, 1, lens, cnt, cbase, sbase, en, mgc, mtt, mgrp, nullptr, nullptr, nullptr, 0, rows, 16, c0, n0, s0, tot);
    CHECK(nch == 3);                       // contig 0 under models 0 and 1 (both window ends inclusive), contig 1 (gc 0) under none, contig 2 under model 2
    CHECK(rows[3] == 0 && rows[4] == 0 && rows[8 + 3] == 2 && rows[8 + 4] == 2 && rows[16 + 3] == 1 && rows[16 + 6] == 1);
    CHECK(tot[0] == 10 + 4 + 6 && tot[1] == 4 + 2 + 2 && c0[1] == 2 && c0[2] == 3);
    // winners: a tie between groups goes to the lower model, -100 loses, ipath < 0 does not count
    const double ms[3] = {5.0, -100.0, 5.0}; const int32_t ip[3] = {3, 1, 2};
    int32_t win[3];
    find_plan_winners(NC, NM, 1, rows, 3, ms, ip, nullptr, 0, nullptr, nullptr, nullptr, win);
    CHECK(win[0] == 0 && win[1] == -1 && win[2] == -1);
    // sets: contigs 0 and 2 in one set
    { const int32_t so[3] = {0, 1, 0}; double sc[9]; int32_t sm[3] = {-1, -1, -1}; double ss[3] = {nan, nan, nan};
      for (double& v : sc) v = nan;
      find_plan_winners(NC, NM, 1, rows, 3, ms, ip, so, 2, sc, sm, ss, win);
      CHECK(sm[0] == 0 && sm[2] == 0 && win[0] == 0 && win[2] == -1 && ss[0] == 5.0); }
    // re-score and gather
    { const int32_t w[3] = {2, -1, 1}; const uint8_t conv[6] = {1, 0, 0, 1, 0, 0};
      int64_t rs[4 * 4], rc0[3], rn0[3], fin[3], wr[6 * 4], oo[3], wo[3];
      CHECK(find_plan_rescore(NC, NG, 1, rows, 3, w, conv, mgrp, NM, tot[0], rs, rc0, rn0, fin) == 0);      // both winners were `first`
      CHECK(find_plan_gather(NC, NG, rows, 3, w, fin, wr, oo, wo) == 6 + 4); }
    printf("find_plan ok\n");
    return 0;
}
#endif
