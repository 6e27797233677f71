// The host arithmetic of a finder call (finder.hip): dense set ids, the (contig, model) chains from the GC windows, the winning
// chain of every contig, who needs a fresh re-score, the layout of the gathered winners.  Plain arrays in, plain vectors out, no HIP
// header: tests/find_plan_shim.cpp builds this file with a host compiler.
#pragma once
#include <math.h>
#include <stdint.h>

#include <unordered_map>
#include <vector>

#include "find_pods.h"

namespace pga_plan {

// contig sets: dense ids in order of first appearance, a contig without a label (< 0) a set of its own; returns the number of sets
inline int dense_set_ids(const int32_t* labels, const int NC, std::vector<int32_t>& set_of) {
    int NS = 0;
    set_of.resize((size_t)NC);
    std::unordered_map<int32_t, int32_t> dense;
    for (int i = 0; i < NC; i++) {
        const int32_t lab = labels[(size_t)i];
        if (lab < 0) { set_of[(size_t)i] = NS++; continue; }
        auto it = dense.find(lab);
        if (it == dense.end()) it = dense.emplace(lab, NS++).first;
        set_of[(size_t)i] = it->second;
    }
    return NS;
}

struct ChainPlanIn {
    int NC, NM, NG;
    bool meta_run;
    const ContigDesc* ct;
    const int32_t* h_cnt;              // per contig: G+C bases
    const int32_t* h_cbase;            // [NG][NC + 1] first node of every contig
    const int32_t* h_sbase;            // [NG][NC + 1] first stop node
    const uint8_t* h_enabled;          // [NG][NC] meta mode: what the device made of the same windows
    const double* model_gc; const int* model_tt; const int* model_group;        // per model
    const int32_t* model_of_contig;    // single mode with a model per contig, or nullptr: model 0
    const int* cgrp;                   // single mode with a group per contig, or nullptr: group 0
    const int32_t* set_of; int NS;     // contig sets, or nullptr
};
struct ChainPlan {
    std::vector<ChainDesc> chains;     // group-major, per group in (contig, model) order
    std::vector<int> g_c0;             // [NG + 1] chains before group g
    std::vector<int64_t> g_n0, g_s0;   // [NG + 1] chain nodes / (chain, stop node) pairs before the chains of group g
    int64_t tot_chain_nodes = 0, tot_chain_stops = 0;
};
// the (contig, model) chains (ref: lib.pyx:5335-5362); false: host and device disagree on a GC window
inline bool plan_chains(const ChainPlanIn& in, ChainPlan& out) {
    const int NC = in.NC, NM = in.NM, NG = in.NG;
    std::vector<std::vector<ChainDesc>> gch((size_t)NG);     // per group, in (contig, model) order
    for (int g = 0; g < NG; g++) gch[g].reserve(in.meta_run ? (size_t)NC * 6 : (size_t)NC);
    // contig sets: the same pooled numbers the device summed (integers, exact), one division per set
    std::vector<double> set_gc;
    if (in.set_of) {
        std::vector<int64_t> sum((size_t)2 * in.NS, 0);
        for (int i = 0; i < NC; i++) { sum[2 * (size_t)in.set_of[i]] += in.h_cnt[i]; sum[2 * (size_t)in.set_of[i] + 1] += in.ct[i].len; }
        set_gc.resize((size_t)in.NS);
        for (int s = 0; s < in.NS; s++) set_gc[(size_t)s] = sum[2 * (size_t)s + 1] > 0 ? (double)sum[2 * (size_t)s] / (double)sum[2 * (size_t)s + 1] : 0.0;
    }
    for (int i = 0; i < NC; i++) {
        if (!in.meta_run) {
            const int m = in.model_of_contig ? in.model_of_contig[i] : 0, g = in.cgrp ? in.cgrp[i] : 0;
            const int32_t* cb = in.h_cbase + (size_t)g * (NC + 1);
            ChainDesc ch{0, cb[i], cb[i + 1] - cb[i], m, i, 1};
            ch.group = g;
            gch[g].push_back(ch);
            continue;
        }
        const int L = in.ct[i].len;
        const double gc = in.set_of ? set_gc[(size_t)in.set_of[i]] : (L > 0 ? (double)in.h_cnt[i] / (double)L : 0.0);
        const double low = fmin(0.65, 0.88495 * gc - 0.0102337), high = fmax(0.35, 0.86596 * gc + 0.1131991);
        int tt_prev = -1;
        for (int m = 0; m < NM; m++) {
            if (in.model_gc[m] < low || in.model_gc[m] > high) continue;
            const int g = in.model_group[m];
            if (!in.h_enabled[(size_t)g * NC + i]) return false;
            const int32_t* cb = in.h_cbase + (size_t)g * (NC + 1);
            ChainDesc ch{0, cb[i], cb[i + 1] - cb[i], m, i, in.model_tt[m] != tt_prev ? 1 : 0};
            ch.group = g;
            tt_prev = in.model_tt[m];
            gch[g].push_back(ch);
        }
    }
    { size_t tot = 0; for (int g = 0; g < NG; g++) tot += gch[g].size(); out.chains.clear(); out.chains.reserve(tot); }
    out.g_c0.assign((size_t)NG + 1, 0); out.g_n0.assign((size_t)NG + 1, 0); out.g_s0.assign((size_t)NG + 1, 0);
    out.tot_chain_nodes = 0; out.tot_chain_stops = 0;
    for (int g = 0; g < NG; g++) {
        out.g_c0[g] = (int)out.chains.size(); out.g_n0[g] = out.tot_chain_nodes;
        for (ChainDesc& ch : gch[g]) {
            ch.off = out.tot_chain_nodes; out.tot_chain_nodes += ch.n;
            ch.soff = out.tot_chain_stops;
            const int32_t* sb = in.h_sbase + (size_t)ch.group * (NC + 1);
            out.tot_chain_stops += sb[ch.contig + 1] - sb[ch.contig];
            out.chains.push_back(ch);
        }
        out.g_s0[g + 1] = out.tot_chain_stops;
    }
    out.g_c0[NG] = (int)out.chains.size(); out.g_n0[NG] = out.tot_chain_nodes;
    return true;
}

// The winning chain of every contig, -1: none (ref: lib.pyx:5364-5367, strict '>' from -100).  The reference visits the models of a
// contig in model order and keeps a strictly better one: the winner is the highest score, the lowest model among equals -- one pass
// over the chains, whatever group they sit in.  Single mode (!meta): the contig's first chain.
// set_of (meta mode, or nullptr) -- contig sets: a contig contributes its path score under a model iff it has nodes and a path there;
// S_m of a set is the sum of its members' contributions in batch order; the set's model is the largest S_m above -100, the lowest index
// among equals; a member that contributed under it is called from that chain, the others have no genes.  model_scores [NC][NM] (NaN
// on entry: no contribution), set_model and set_score [NC] (-1 / NaN on entry) are what the context reports of the choice.
inline void pick_winners(const int NC, const int NM, const bool meta, const ChainDesc* chains, const int NCH, const double* h_maxscore,
                         const int32_t* h_ipath, const int32_t* set_of, const int NS, double* model_scores, int32_t* set_model,
                         double* set_score, std::vector<int>& win_chain) {
    win_chain.assign((size_t)NC, -1);
    if (!meta) { for (int k = NCH - 1; k >= 0; k--) win_chain[chains[k].contig] = k; return; }
    if (set_of) {
        std::vector<int32_t> chain_of((size_t)NC * NM, -1);
        for (int k = 0; k < NCH; k++) {
            const ChainDesc& ch = chains[k];
            if (ch.n <= 0 || h_ipath[k] < 0) continue;
            model_scores[(size_t)ch.contig * NM + ch.model] = h_maxscore[k];
            chain_of[(size_t)ch.contig * NM + ch.model] = k;
        }
        std::vector<double> S((size_t)NS * NM, 0.0);
        std::vector<uint8_t> has((size_t)NS * NM, 0);
        for (int i = 0; i < NC; i++) {
            const size_t s0 = (size_t)set_of[i] * NM;
            for (int m = 0; m < NM; m++) {
                if (chain_of[(size_t)i * NM + m] < 0) continue;
                const double v = model_scores[(size_t)i * NM + m];
                if (has[s0 + m]) S[s0 + m] += v; else { S[s0 + m] = v; has[s0 + m] = 1; }
            }
        }
        std::vector<int32_t> W((size_t)NS, -1);
        for (int s = 0; s < NS; s++) {
            double best = -100.0;
            for (int m = 0; m < NM; m++) if (has[(size_t)s * NM + m] && S[(size_t)s * NM + m] > best) { best = S[(size_t)s * NM + m]; W[(size_t)s] = m; }
        }
        for (int i = 0; i < NC; i++) {
            const int w = W[(size_t)set_of[i]];
            if (w < 0) continue;
            set_model[(size_t)i] = w; set_score[(size_t)i] = S[(size_t)set_of[i] * NM + w];
            win_chain[i] = chain_of[(size_t)i * NM + w];
        }
        return;
    }
    std::vector<double> best((size_t)NC, -100.0);
    for (int k = 0; k < NCH; k++) {
        const ChainDesc& ch = chains[k];
        if (ch.n <= 0 || h_ipath[k] < 0) continue;
        const int w = win_chain[ch.contig];
        if (h_maxscore[k] > best[ch.contig] || (w >= 0 && h_maxscore[k] == best[ch.contig] && ch.model < chains[w].model)) {
            best[ch.contig] = h_maxscore[k]; win_chain[ch.contig] = k;
        }
    }
}

// Fresh re-score of winners that were not the first model of their group (ref: lib.pyx:5380-5394).  A later model of a run sees the
// edge flags its predecessors left (lib.pyx:2424-2434); where the contig has no start node that scoring turns into an edge node
// (h_conv [NG][NC] clear), that state is the fresh one and the winning pass already is the re-score.  The re-score chains go behind the
// tot_chain_nodes nodes of the call's chains, group-major; fin_off[i]: where contig i's final-pass fields are, -1: no winner.
struct RescorePlan {
    std::vector<ChainDesc> rescore;
    std::vector<int> r_c0;             // [NG + 1]
    std::vector<int64_t> r_n0;         // [NG + 1]
    std::vector<int64_t> fin_off;      // [NC]
};
inline void plan_rescore(const int NC, const int NG, const bool meta, const ChainDesc* chains, const int* win_chain, const uint8_t* h_conv,
                         const int* model_group, const int64_t tot_chain_nodes, RescorePlan& out) {
    std::vector<std::vector<ChainDesc>> rs_g((size_t)NG);
    out.rescore.clear();
    out.fin_off.assign((size_t)NC, -1);
    int64_t rs_nodes = 0;
    for (int i = 0; i < NC; i++) {
        const int k = win_chain[i];
        if (k < 0) continue;
        if (!meta || chains[k].first || !h_conv[(size_t)model_group[chains[k].model] * NC + i]) { out.fin_off[i] = chains[k].off; continue; }
        ChainDesc ch = chains[k]; ch.first = 1;
        ch.raw_off = chains[k].off;                 // same contig, same model: the ORF walk of the winning pass stands
        rs_g[model_group[ch.model]].push_back(ch);
    }
    out.r_c0.assign((size_t)NG + 1, 0); out.r_n0.assign((size_t)NG + 1, 0);
    for (int g = 0; g < NG; g++) {
        out.r_c0[g] = (int)out.rescore.size(); out.r_n0[g] = tot_chain_nodes + rs_nodes;
        for (ChainDesc ch : rs_g[g]) { ch.off = tot_chain_nodes + rs_nodes; out.fin_off[ch.contig] = ch.off; rs_nodes += ch.n; out.rescore.push_back(ch); }
    }
    out.r_c0[NG] = (int)out.rescore.size(); out.r_n0[NG] = tot_chain_nodes + rs_nodes;
}

// The gathered winners -- output order: group-major then contig, so each group's launch covers a contiguous output range.
// (Win: the record of the gather kernel -- out_off, dp_off, fin_off, topo_off, n, padding -- which lives with that kernel.)
template <class Win> struct GatherPlan {
    std::vector<std::vector<Win>> wg;          // per group
    std::vector<int64_t> out_off;              // [NC] first gathered node of the contig's winner (0: none)
    std::vector<int64_t> w_o0;                 // [NG + 1] gathered nodes before group g
    int64_t out_nodes = 0;
};
template <class Win> void plan_gather(const int NC, const int NG, const ChainDesc* chains, const int* win_chain, const int64_t* fin_off, GatherPlan<Win>& out) {
    out.wg.assign((size_t)NG, {});
    out.out_off.assign((size_t)NC, 0);
    out.w_o0.assign((size_t)NG + 1, 0);
    out.out_nodes = 0;
    for (int g = 0; g < NG; g++) {
        out.w_o0[g] = out.out_nodes;
        for (int i = 0; i < NC; i++) {
            const int k = win_chain[i];
            if (k < 0 || chains[k].group != g) continue;
            out.out_off[i] = out.out_nodes;
            out.wg[g].push_back(Win{out.out_nodes, chains[k].off, fin_off[i], chains[k].topo_off, chains[k].n, 0});
            out.out_nodes += chains[k].n;
        }
    }
    out.w_o0[NG] = out.out_nodes;
}

}  // namespace pga_plan
