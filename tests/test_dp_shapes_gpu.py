"""GPU parity of connection scoring at its distance, overlap and window edges (tests/dp_shapes.py; DESIGN.md 4.4.1, "Connection scoring
at its edges"; tests/test_dp_shapes_cpu.py proves on the CPU what each shape contains).  Scorer level: every shape's designed score
arrays through `pga_score_connections` under every kernel family and topology switch, and through the shrunk segment plan; the pair
shapes through `pga_score_connections_training` as well.  Finder level: the contigs of the pair shapes through `find_genes_batch`,
all in one launch and each alone, single and meta mode, closed and open ends, max_overlap 30 / 60 / 200 -- scores cannot be injected
there, what it adds is k_ovl_stops and the finder's own launch on these topologies.  Scores equal in all 64 bits, traceb, ov_mark
among reached nodes and the best gene end equal (test_dp_ties_gpu.same); every node field and gene (test_finder_gpu.compare_contig)."""
import os

import numpy as np
import pytest

from tests import dp_inject, dp_shapes
from tests.test_dp_shapes_cpu import solve
from tests.test_dp_ties_gpu import ENV as DP_ENV, VARIANTS, run, same

pytestmark = pytest.mark.gpu

ENV = DP_ENV + ("PGA_DPW_TOPO_WALK",)
ST_WT = dp_shapes.ST_WT
SHRUNK = {"PGA_DP_SEG_MIN": "256", "PGA_DP_SEG_LEN": "64", "PGA_DP_SEG_WARM": "64"}
TOPO_SWITCHES = {"walk": {"PGA_DPW_TOPO_WALK": "1"}, "global": {"PGA_DPW_TOPO_LDS": "0"}}


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def clean_env():
    saved = {k: os.environ.pop(k, None) for k in ENV}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


@pytest.fixture(scope="module")
def cases():
    """[(name, before, ref, ref_max)] of every shape, from the oracle, once for all tests."""
    out = []
    for s in dp_shapes.all_shapes():
        o, before, ref, ref_max, ev, eg = solve(s)
        out.append((s.name, before, ref, ref_max))
    return out


@pytest.fixture(scope="module")
def lds_cases():
    out = []
    for n, seq in dp_shapes.lds_contigs().items():
        before, ref, ref_max, ev = dp_inject.inject(seq, "quant", ST_WT, seed=1)
        assert len(ref) == n
        out.append(("lds/n%d" % n, before, ref, ref_max))
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_shape_under_every_kernel_family(ctx, cases, lds_cases, variant):
    os.environ.update(VARIANTS[variant])
    for name, before, ref, ref_max in cases + lds_cases:
        same(run(ctx, before, ST_WT), ref, ref_max, (variant, name))


@pytest.mark.parametrize("variant", ["wave", "wavedyn", "wavemiss"])
@pytest.mark.parametrize("switch", list(TOPO_SWITCHES))
def test_every_shape_under_the_topology_switches(ctx, cases, lds_cases, switch, variant):
    os.environ.update(VARIANTS[variant])
    os.environ.update(TOPO_SWITCHES[switch])
    for name, before, ref, ref_max in cases + lds_cases:
        same(run(ctx, before, ST_WT), ref, ref_max, (variant, switch, name))


def test_the_shrunk_segment_plan(ctx, cases):
    """Segments of 64 nodes with a warm-up of 64 from 256 nodes on: the serial loop's results whatever the verification rejects; chains
    below 256 nodes are not segmented."""
    os.environ.update(SHRUNK)
    segmented = set()
    for name, before, ref, ref_max in cases:
        same(run(ctx, before, ST_WT), ref, ref_max, ("shrunk", name))
        chains = ctx.dp_stats()["chains"]
        assert chains == (1 if len(ref) >= 256 else 0), (name, len(ref), chains)
        if chains:
            segmented.add(len(ref))
    assert {256, 257, 319, 320, 321, 1023, 1024, 1025} <= segmented and 255 not in segmented


def test_a_single_node_on_a_sub_chains_first_node_and_one_before_it(ctx, cases):
    """dp_shapes.segment_series under the shrunk plan: a reverse start's own stop, and a reverse stop's operon source, as the first node
    of the target's sub-chain (`one` in load_target keeps it: every segment verifies clean, nothing is rejected in any round) and as the
    node before it (the single node is "none" for the walk, the verification rejects the target and the re-scoring repairs it).
    Nothing else in these chains is reached, so a rejected node can only be the target or what follows from it."""
    seen = set()
    for name, before, ref, ref_max in cases:
        if not name.startswith("segment"):
            continue
        os.environ.update(SHRUNK)
        if name.startswith("segment128/"):
            os.environ["PGA_DP_SEG_LEN"] = "128"
        same(run(ctx, before, ST_WT), ref, ref_max, ("shrunk", name))
        st = ctx.dp_stats()
        print(name, st)
        assert st["chains"] == 1 and st["segments"] >= 4, (name, st)
        if name.endswith("/first"):
            assert sum(st["rejected"]) == 0 and st["serial"] == 0, (name, st)
        else:
            assert st["rejected"][0] > 0, (name, st)
        seen.add(name)
    assert len(seen) == 8


@pytest.mark.parametrize("kernel", ["default", "wave"])
def test_the_training_pass_on_the_pair_shapes(ctx, kernel):
    os.environ.update(VARIANTS[kernel])
    joins = 0
    for s in dp_shapes.all_pair_shapes():
        o, before, ref, ref_max, ev, eg = solve(s, final=False)
        joins += ev["joins"]
        out = ctx.score_connections_training(before["ndx"], before["stop_val"], before["type"], before["strand"], before["gc_score"],
                                             np.ones(3), before["star_ptr"], ST_WT)
        same(out, ref, ref_max, (kernel, s.name))
    assert joins > 0


# ---- finder level ----

@pytest.mark.parametrize("tag", ["nctc", "meta"])
@pytest.mark.parametrize("closed", [True, False])
def test_the_pair_shapes_through_the_finder(ctx, tag, closed):
    from tests.test_tail_shapes_gpu import check
    shapes = dp_shapes.all_pair_shapes()
    for maxov in (30, 60, 200):
        seqs = [s.seq for s in shapes if s.max_overlap == maxov and (maxov == 60 or s.name.startswith("operon"))]
        assert len(seqs) >= 20
        if maxov == 60 and not closed:              # open ends: the ORFs that run off the contig give edge stops, which take no overlapping start
            seqs += [s.seq for s in dp_shapes.edge_stop_series()]
        check(ctx, seqs, tag, closed=closed, max_overlap=maxov)                 # one launch of many chains
        for seq in seqs:
            check(ctx, [seq], tag, closed=closed, max_overlap=maxov)            # a launch of one
