"""Connection scoring at its distance, overlap and window edges, proven on the CPU (tests/dp_shapes.py; DESIGN.md 4.4.1, "Connection
scoring at its edges"): from the oracle alone that every shape is what its design says -- the node list, the probe pair that
decides the target's traceb on the allowed side of a rule and does not on the refused side, the intergenic term to the last bit, the
window the reference gives each target, the index of each node in the kernels' own units -- and from the oracle's edge counters that
every integer comparison of the rules was decided at its threshold and one step beside it somewhere in the catalogue, or cannot be.
Then the host model of the wave-batch kernel (tests/dpw_model.cpp, which shares dpw_core.h with the kernel) on every shape, bit for
bit against the oracle, the training pass included."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import dp_inject, dp_shapes
from tests.test_dpw_model import compare, model, run_model  # noqa: F401  (model is a fixture)

ST_WT = dp_shapes.ST_WT


def index_of(nodes, node):
    return dp_inject.node_index(nodes, node.kind, node.ndx)


def solve(shape, final=True):
    """(oracle, before, ref, ref_max, events, edges) of a shape under its assignment."""
    o = dp_inject.extracted(shape.seq, shape.closed)
    named = [(shape.nodes[k].kind, shape.nodes[k].ndx, v) for k, v in shape.scores.items()]
    return (o,) + dp_inject.inject_assigned(o, named, shape.meta.get("default", dp_shapes.DEFAULT), ST_WT, shape.max_overlap, final=final)


@pytest.fixture(scope="module")
def solved():
    return [(s,) + solve(s) for s in dp_shapes.all_shapes()]


def test_every_node_list_is_the_designed_one(solved):
    for s, o, before, ref, ref_max, ev, eg in solved:
        if s.n_nodes is not None:
            assert len(ref) == s.n_nodes, (s.name, len(ref), s.n_nodes)
        for name, node in s.nodes.items():
            k = index_of(ref, node)                       # position, strand and kind: exactly one such node
            assert ref["stop_val"][k] == node.stop_val, (s.name, name, int(ref["stop_val"][k]), node.stop_val)
        if s.nodes and s.n_nodes is not None and s.n_nodes == len(s.nodes):
            assert sorted((n.ndx, -dp_shapes.KIND[n.kind][0]) for n in s.nodes.values()) == [(int(x["ndx"]), -int(x["strand"])) for x in ref]
    # every design states its node count; only the two open contigs, whose edge nodes the extraction decides, state their claims otherwise
    assert [s.name for s, *_ in solved if s.n_nodes is None] == ["edge/+", "edge/-"]


def test_the_probe_pair_decides_the_target(solved):
    sides = {}
    for s, o, before, ref, ref_max, ev, eg in solved:
        if s.probe is None:
            continue
        src, tgt, allowed = s.probe
        si, ti = index_of(ref, s.nodes[src]), index_of(ref, s.nodes[tgt])
        assert si < ti or not allowed, s.name            # (a pair at one position sorts the forward node first: refused by the order)
        assert (ref["traceb"][ti] == si) == allowed, (s.name, int(ref["traceb"][ti]), si, allowed)
        if not allowed and s.meta.get("refused_traceb", 0) != 0:
            other = s.meta["refused_traceb"]
            assert ref["traceb"][ti] == (-1 if other is None else index_of(ref, s.nodes[other])), s.name
        if "ov_mark" in s.meta:
            assert ref["ov_mark"][ti] == s.meta["ov_mark"], (s.name, int(ref["ov_mark"][ti]))
        if s.series:
            sides.setdefault(s.series, set()).add(allowed)
    # every series of neighbours has a shape on either side of its threshold, but those whose rule changes the value, not the source
    one_sided = {k for k, v in sides.items() if len(v) < 2}
    assert all(k.startswith(("triple/ovlp200", "triple/n3", "triple/traceb", "triple/zero")) for k in one_sided), one_sided
    marks = {}
    for s, o, before, ref, *_ in solved:
        if s.series in one_sided:
            marks.setdefault(s.series, set()).add(s.meta["ov_mark"] >= 0)
    assert all(v == {True, False} for v in marks.values()) and len(marks) == len(one_sided), marks


def igm_same_ref(dist, overlap, st_wt, adjacent=False, r=0.0, u=0.0):
    """ref: _connection.h:52-78, in its order of operations."""
    v = 0.0
    if adjacent:
        if r < 0:
            v -= r
        if u < 0:
            v -= u
    if dist > 180:
        v -= 0.15 * st_wt
    elif (dist <= 60 and not overlap) or dist * 4 < 60:
        v += (2.0 - dist / 60) * 0.15 * st_wt
    return v


def test_the_intergenic_term_is_the_formulas_to_the_last_bit(solved):
    seen = set()
    for s, o, before, ref, ref_max, ev, eg in solved:
        if s.probe is None or not s.probe[2] or not s.series:
            continue
        si, ti = index_of(ref, s.nodes[s.probe[0]]), index_of(ref, s.nodes[s.probe[1]])
        if s.series.startswith("igm/"):
            d = s.at
            assert abs(int(ref["ndx"][ti]) - int(ref["ndx"][si])) == d
            want = ref["score"][si] + igm_same_ref(d, False, ST_WT)
            seen.add(("direct", d))
        elif s.series.startswith("operon"):
            third = before[index_of(ref, s.nodes[s.meta["third"]])]
            d = s.meta["overlap_dist"]
            ig = igm_same_ref(d, True, ST_WT, s.at[0] in (-2, 1), third["rscore"], third["uscore"])
            want = ref["score"][si] + ((third["cscore"] + third["sscore"]) + ig)
            seen.add(("third", d))
        else:
            continue
        assert ref["score"][ti] == want, (s.name, ref["score"][ti], want)
    for d in (3, 14, 15, 59, 60, 179, 180):
        assert ("direct", d) in seen, d
    for d in (1, 2, 13, 14, 16, 17, 59, 61, 199, 200):
        assert ("third", d) in seen, d
    # and the differences between neighbours that the formula states: the bonus ends behind 60 (direct) and behind 14 (overlapping)
    assert igm_same_ref(60, False, ST_WT) == 1.0 * 0.15 * ST_WT and igm_same_ref(61, False, ST_WT) == 0.0
    assert igm_same_ref(14, True, ST_WT) > 0.0 and igm_same_ref(16, True, ST_WT) == 0.0 and igm_same_ref(181, False, ST_WT) == -0.15 * ST_WT


def test_every_comparison_was_decided_at_its_threshold_and_beside_it(solved):
    total = {k: [0, 0, 0] for k in orc.DP_EDGES}
    for s, o, before, ref, ref_max, ev, eg in solved:
        for k, v in eg.items():
            for j in range(3):
                total[k][j] += v[j]
    missing = {(k, j - 1) for k, v in total.items() for j in range(3)
               if v[j] == 0 and (j - 1) in dp_shapes.EVENT_SLOTS.get(k, (-1, 0, 1))}
    assert missing == set(dp_shapes.IMPOSSIBLE), (sorted(missing - set(dp_shapes.IMPOSSIBLE)), sorted(set(dp_shapes.IMPOSSIBLE) - missing))
    print({k: tuple(v) for k, v in total.items()})


def test_each_window_lands_where_its_design_says(solved):
    cases = set()
    for s, o, before, ref, ref_max, ev, eg in solved:
        for name, want in s.meta.get("window", {}).items():
            assert o.dp_window(index_of(ref, s.nodes[name])) == want, (s.name, name)
        g = s.meta.get("giant")
        if not g:
            continue
        node = s.nodes[g["target"]]
        i = index_of(ref, node)
        assert i > 500 and ref["ndx"][i - 500] > node.stop_val            # the ORF begins more than 500 nodes back
        lo, walked, landed = o.dp_window(i)
        assert walked
        at = np.flatnonzero(ref["ndx"] == node.stop_val)
        assert len(at) == {"one": 1, "two": 2, "none": 0}[g["case"]], (s.name, at)
        assert landed == (at[-1] if len(at) else 0), (s.name, landed, at)
        assert (lo == 0 and landed < 500) if g["clamped"] or g["case"] == "none" else (lo == landed - 500 and lo > 0), (s.name, lo, landed)
        cases.add((node.kind, g["case"], lo > 0))
    assert cases == {("fs", "one", False), ("fs", "one", True), ("fs", "two", False), ("fs", "two", True), ("fs", "none", False),
                     ("rb", "one", False), ("rb", "one", True), ("rb", "two", False), ("rb", "two", True)}, cases


def test_indices_lanes_and_chain_lengths_are_what_the_designs_claim(solved):
    lanes, near, chains = set(), set(), set()
    for s, o, before, ref, ref_max, ev, eg in solved:
        for name, want in s.meta.get("index", {}).items():
            assert index_of(ref, s.nodes[name]) == want, (s.name, name)
        if s.series and s.series.startswith(("lane/", "dense/", "size/")):
            ti, si = index_of(ref, s.nodes[s.probe[1]]), index_of(ref, s.nodes[s.probe[0]])
            lanes.add((ti % 64, si // 64 - ti // 64))
            t_ndx = int(ref["ndx"][ti])
            within = int((ref["ndx"][:ti] >= t_ndx - 180).sum())          # p_near = ti - within
            near.add(within)
            if "near" in s.meta:
                assert within == s.meta["near"], (s.name, within)
                assert (ti - within < (ti // 64) * 64 - 64) == (within >= 65) and ti % 64 == 0
            if s.series.startswith("size/"):
                assert (ti - within) % 8 == {128: 7, 129: 0}[ti] if s.at == 180 else True
        if "chain" in s.meta:
            assert len(ref) == s.meta["chain"]
            chains.add(len(ref))
    # the window's first node at the last node of a block of eight, at its first and inside one, from the oracle's accessor
    lo_mod8 = set()
    for s, o, before, ref, ref_max, ev, eg in solved:
        if "lo_mod8" in s.meta:
            lo = o.dp_window(index_of(ref, s.nodes[s.probe[1]]))[0]
            assert lo % 8 == s.meta["lo_mod8"] and lo > 0, (s.name, lo)
            assert (index_of(ref, s.nodes[s.probe[0]]) == lo) == s.probe[2], s.name       # the source IS node lo, or the one before
            lo_mod8.add(lo % 8)
    assert {7, 0, 4} <= lo_mod8, lo_mod8
    # a never-reached gene end as the only source: without a traceb itself, refused by the rule, and the target left at 0.0
    arts = [x for x in solved if x[0].meta.get("artifact")]
    assert len(arts) >= 4
    for s, o, before, ref, ref_max, ev, eg in arts:
        si, ti = index_of(ref, s.nodes[s.probe[0]]), index_of(ref, s.nodes[s.probe[1]])
        assert ref["traceb"][si] == -1 and ref["traceb"][ti] == -1 and ref["score"][ti] == 0.0 and eg["artifact"][1] >= 1, s.name
    assert {(63, 0), (0, -1), (0, -2)} <= lanes, lanes
    assert {62, 63, 64, 65, 66, 67} <= near
    assert chains == set(dp_shapes.SIZES)
    edge = [x for x in solved if x[0].meta.get("edge")]
    assert len(edge) == 2
    for s, o, before, ref, ref_max, ev, eg in edge:
        stops = (before["type"] == 3) & (before["edge"] == 1)
        assert stops.sum() >= 3 and (before["star_ptr"][stops] == -1).all() and eg["ovl_edge_stop"][1] == stops.sum()
    # ... while an ordinary stop of the same contig does take the start before it
    assert any((x[2]["star_ptr"][(x[2]["type"] == 3) & (x[2]["edge"] == 0)] >= 0).any() for x in edge)


def test_a_dead_forward_stop_offers_its_operon_value_to_nobody(solved):
    """dead_end/+: the target lies more than two batches behind the forward stop, whose own value plus its overlapping start's is more
    than the target's own start gives -- in `alive` the target takes it, in `dead` (the stop has no traceb) it may not."""
    seen = set()
    for s, o, before, ref, ref_max, ev, eg in solved:
        if "dead_end" not in s.meta:
            continue
        si, ti, bi = (index_of(ref, s.nodes[k]) for k in ("as", "bs", "bb"))
        assert ti - si > 128 and ref["strand"][si + 1:ti].max() == -1              # nothing but reverse nodes between them
        offer = (before["cscore"][bi] + before["sscore"][bi]) + igm_same_ref(13, True, ST_WT)
        own = ref["score"][bi] + (before["cscore"][bi] + before["sscore"][bi])
        assert before["star_ptr"][si][int(ref["ndx"][ti]) % 3] == bi and 0.0 + offer > own > 0.0, s.name
        if s.meta["dead_end"] == "alive":
            assert ref["traceb"][si] >= 0 and ref["traceb"][ti] == si and ref["score"][ti] == ref["score"][si] + offer
        else:
            assert ref["traceb"][si] == -1 and ref["score"][si] == 0.0 and ref["traceb"][ti] == bi and ref["score"][ti] == own
        seen.add(s.meta["dead_end"])
    assert seen == {"alive", "dead"}


def test_the_host_model_on_every_shape(model, solved):
    for s, o, before, ref, ref_max, ev, eg in solved:
        try:
            compare(model, before, ref, ref_max, ST_WT)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (s.name, e))


def test_the_training_pass_of_the_pair_rules_on_the_oracle():
    """final = 0: a connection is worth (right - left + 1 - 2 ovlp) times the frame score of the gene's start, which pins the +-2
    adjustments of left and right.  The host model has no training pass (the training pass never takes the wave-batch kernel), so the
    CPU states the factor for the gene connections from the formula; tests/test_dp_shapes_gpu.py compares the chain kernel on the same
    arrays.  gc_score is derived from the design's assignment (dp_inject.inject_assigned), star_ptr holds the first candidates."""
    shapes = dp_shapes.all_pair_shapes()
    genes = overlaps = 0
    for s in shapes:
        o, before, ref, ref_max, ev, eg = solve(s, final=False)
        mod = before["gc_score"].sum(axis=1)
        for i in np.flatnonzero((ref["type"] == 3) | (ref["strand"] == -1)):
            j = int(ref["traceb"][i])
            if j < 0:
                continue
            a, b = ref[j], ref[i]
            fwd_gene = a["strand"] == 1 and a["type"] != 3 and b["strand"] == 1 and b["type"] == 3
            rev_gene = a["strand"] == -1 and a["type"] == 3 and b["strand"] == -1 and b["type"] != 3
            if fwd_gene or rev_gene:
                length = int(b["ndx"]) - int(a["ndx"]) + 3
                assert b["score"] == a["score"] + float(length) * mod[j if fwd_gene else i], (s.name, i, j)
                genes += 1
            if a["strand"] == 1 and a["type"] == 3 and b["strand"] == -1 and b["type"] != 3:      # forward stop -> reverse start
                ovlp = int(a["ndx"]) + 2 - (int(b["stop_val"]) - 2) + 1
                length = int(b["ndx"]) - (int(b["stop_val"]) - 2) + 1 - 2 * ovlp
                assert b["score"] == a["score"] + float(length) * mod[i], (s.name, i, j)
                overlaps += 1
    assert genes >= len(shapes) and overlaps >= 5, (genes, overlaps)


def test_the_host_model_at_the_lds_edges_of_the_topology_kernel(model):
    """Contigs of exactly TOPO_LDS_NODES - 1, TOPO_LDS_NODES and one more node, and the two counts on either side of the point where
    k_dpw_topo_lds asks for more than 64 KB: 12 bytes per node and 32 of dynamic LDS next to its static arrays (the masks of the
    forward stops, 3 x 96 words, and four counters), taken from the kernel's size expression."""
    assert dp_shapes.LDS_STATIC == 2320 and 12 * (dp_shapes.LDS_FIRST_OVER - 1) + 32 + dp_shapes.LDS_STATIC <= 65536 < 12 * dp_shapes.LDS_FIRST_OVER + 32 + dp_shapes.LDS_STATIC
    assert 12 * (dp_shapes.LDS_DYNAMIC_OVER - 1) + 32 <= 65536 < 12 * dp_shapes.LDS_DYNAMIC_OVER + 32
    contigs = dp_shapes.lds_contigs()
    assert sorted(contigs) == sorted(dp_shapes.LDS_COUNTS)
    for n, seq in contigs.items():
        before, ref, ref_max, ev = dp_inject.inject(seq, "quant", ST_WT, seed=1)
        assert len(ref) == n and ev["joins"] > n
        compare(model, before, ref, ref_max, ST_WT)
