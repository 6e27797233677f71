// The plain records of a finder call's host plan: what find_plan.h (host arithmetic, built without HIP by the tests) shares with the
// kernels.  Nothing here may need a HIP header.
#pragma once
#include <stdint.h>

// One contig of the batch: `len` bases starting at byte `base` of the concatenated batch buffers.
struct ContigDesc {
    int64_t base;
    int32_t len;
    int32_t _pad;
};

// One DP chain = one (contig, model) pass.
struct ChainDesc {
    int64_t off;        // first element of the chain in the per-chain arrays (scores, DP records)
    int64_t topo_off;   // first element of the contig's nodes in the topology arrays of its group
    int32_t n;          // node count
    int32_t model;
    int32_t contig;
    int32_t first;      // 1: first model scored after (re-)extraction (edge flags not yet converted;
                        //    ref: lib.pyx:2424-2434 mutates node.edge, which persists to the next bin)
    // connection scoring of a SEGMENT of a chain (dp.hip "segmented chains"): the sub-chain reads the records of the
    // chain it belongs to, from node `rebase` on, and keeps its own results at `off`
    int64_t rec_off = -1;   // first DpSrc / DpTgt record of the sub-chain; -1: the chain's own, at `off`
    int32_t rebase = 0;     // chain index of the sub-chain's node 0: index fields of DpTgt are shifted down by it
    int32_t group = 0;      // translation-table group of the chain's model: whose topology arrays `topo_off` indexes (dp_wave.hip)
    int64_t raw_off = -1;   // node scoring: read the raw coding scores of the chain at this offset (same contig, same model)
                            // instead of the chain's own; -1: its own
    int64_t soff = 0;       // stop nodes of the chains before this one (in launch order): its first slot in a launch over (chain, stop) pairs
    int32_t sched_b0 = 0;   // wave-batch scorer: first 64-node batch of the chain's contig in its group's step schedule (dpw_core.h)
    int32_t _pad0 = 0;
};
