"""The catalogue of tests/extract_shapes.py holds what it claims -- from the CPU oracle alone, so that tests/test_extract_shapes_gpu.py
compares the device on inputs that are known to sit on both sides of every threshold -- and tests/extract_ref.py, the extraction with
the mask list as an argument, equals the oracle wherever the oracle applies."""
import math

import numpy as np
import pytest

from oracle import oracle as orc
from tests import extract_shapes as xs
from tests import sets_ref
from tests.extract_ref import MAX_LEN, extract_ref, union

TOPO = ("ndx", "stop_val", "type", "strand", "edge")


def oracle_nodes(seq, tt=11, closed=False, min_gene=90, min_edge_gene=60, min_mask=None):
    o = orc.Oracle(seq, mask=min_mask is not None, mask_size=min_mask or 0)
    o.extract(tt, orc.Params(closed=closed, min_gene=min_gene, min_edge_gene=min_edge_gene))
    o.sort()
    return o.nodes(), o.masks()


def hits(shape, nodes, node):
    """How many of `nodes` sit where the design put `node`."""
    same = (nodes["ndx"] == xs.to_ndx(shape, node.at)) & (nodes["strand"] == shape.strand)
    return int((same & ((nodes["type"] == xs.T_STOP) == (node.kind == "stop"))).sum())


def check_designed_nodes(shapes, **kw):
    """Every designed node is there exactly once where the design says so and absent where it says so; returns (present, absent)."""
    count = [0, 0]
    for sh in shapes:
        for closed in (False, True):
            nodes, _ = oracle_nodes(sh.seq, closed=closed, **kw)
            for nd in sh.meta["nodes"]:
                want = nd.closed if closed else nd.open
                assert hits(sh, nodes, nd) == int(want), (sh.name, closed, nd)
                count[0 if want else 1] += 1
    return tuple(count)


def ref_contigs():
    """(shape, min_gene, min_edge_gene) of every contig extract_ref is held against the oracle on: the short series whole, every
    seventh contig of the long ones."""
    out = [(sh, mg, meg) for mg, meg in xs.GENE_LENGTHS for sh in xs.length_series(mg, meg)]
    out += [(sh, 90, 60) for sh in xs.ends_series() + xs.unknown_series(10) + xs.unknown_series(50) + xs.region_series()]
    out += [(sh, 90, 60) for sh in (xs.phase_series() + xs.left_of_tile_series() + xs.lone_stop_series())[::7] if len(sh.seq) <= MAX_LEN]
    out += [(xs.Shape("neighbour/%d" % k, s, 1, None, {}), 90, 60) for k, s in enumerate(xs.neighbour_series())]
    return out


def test_extract_ref_equals_the_oracle():
    shapes = ref_contigs()
    assert len(shapes) > 1000 and max(len(sh.seq) for sh, _, _ in shapes) > 2 * xs.TILE
    n_nodes = n_masked = 0
    for sh, mg, meg in shapes:
        for min_mask in (None, 0, 10, 50):
            for closed in (False, True):
                for tt in (11, 4):
                    nodes, masks = oracle_nodes(sh.seq, tt, closed, mg, meg, min_mask)
                    got = extract_ref(sh.seq, masks.tolist(), tt, closed, mg, meg)
                    for k, name in enumerate(TOPO):
                        assert np.array_equal(got[k], nodes[name].astype(np.int64)), (sh.name, min_mask, closed, tt, name)
                    n_nodes += len(nodes)
                    n_masked += len(masks)
    assert n_nodes > 10000 and n_masked > 100


@pytest.mark.parametrize("min_gene,min_edge_gene", xs.GENE_LENGTHS)
def test_length_series_sits_on_both_sides_of_every_threshold(min_gene, min_edge_gene):
    shapes = xs.length_series(min_gene, min_edge_gene)
    # 3 residues of L x (3 closed ORFs + 3 frames x 3 lengths off the right end + 3 frames x 3 lengths off the left end) x 2 strands
    assert len(shapes) == 3 * (3 + 9 + 9) * 2
    assert {len(sh.seq) % 3 for sh in shapes} == {0, 1, 2}
    present, absent = check_designed_nodes(shapes, min_gene=min_gene, min_edge_gene=min_edge_gene)
    # closed ORFs: 2 of 3 lengths, open and closed contig; right-open: 2 of 3, open only; left-open (strict): 1 of 3, open only
    assert present == 2 * 2 * 3 * (2 * 2 + 3 * 2 + 3 * 1)
    assert present + absent == 2 * 2 * len(shapes)
    for sh in shapes:                               # the start node exists AT the threshold length and not three bases below it ...
        start = sh.meta["nodes"][0]
        limit = {"closed_orf": min_gene, "right_open": min_edge_gene, "left_open": min_edge_gene + 3}[sh.meta["kind"]]
        assert start.open == (sh.meta["g"] >= limit)
        # ... and the designed start codon is the only one of its strand (left_open: there is none)
        assert len(xs.sites(sh.seq, sh.strand, xs.START_CODONS)) == (0 if sh.meta["kind"] == "left_open" else 1)


def test_phase_series_puts_a_start_and_a_stop_on_every_target():
    shapes = xs.phase_series()
    assert xs.PHASE_TARGETS == tuple(range(1200, 1212)) + (766, 767, 768, 769) + (3069, 3070, 3071, 3072, 3073)
    assert check_designed_nodes(shapes) == (2 * 2 * len(shapes), 0)
    seen = {}
    for sh in shapes:
        kind, T = sh.meta["target"]
        nodes, _ = oracle_nodes(sh.seq, closed=True)              # (closed: without the edge ORF that ends at the far stop)
        mine = nodes[(nodes["strand"] == sh.strand) & ((nodes["type"] == xs.T_STOP) == (kind == "stop"))]
        assert mine["ndx"].tolist() == [T], sh.name               # the one designed node of that kind, at the target
        start = nodes[(nodes["strand"] == sh.strand) & (nodes["type"] != xs.T_STOP) & (nodes["edge"] == 0)]
        assert len(start) == 1 and abs(int(start["stop_val"][0]) - int(start["ndx"][0])) + 3 == 90       # exactly min_gene
        key = (sh.strand, len(sh.seq), kind)
        seen.setdefault(key, []).append(T)
    lengths = {1: [xs.TILE + 300], -1: [2 * xs.TILE + t for t in (0, 1, 2, 11, 12, 13)]}
    assert sorted(seen) == sorted((s, L, k) for s in (1, -1) for L in lengths[s] for k in ("start", "stop"))
    for key, targets in seen.items():
        assert sorted(targets) == sorted(xs.PHASE_TARGETS), key       # each target exactly once


def test_left_of_tile_series_reaches_every_path_of_the_walk():
    shapes = xs.left_of_tile_series()
    present, absent = check_designed_nodes(shapes)
    combos = {}
    for sh in shapes:
        m = sh.meta
        lo = xs.TILE if sh.strand == 1 else m["L"] - xs.TILE
        stop, start = m["nodes"][1].at, m["nodes"][0].at
        x = stop + 3 - 90
        assert stop - lo == m["off"] and (x < lo) == (m["where"] == "below") and start < lo
        if m["k"] != "none":
            assert (lo - 1 - start) // 3 + 1 == m["k"]            # the k-th codon of its frame left of the tile
            assert m["nodes"][0].open == (start <= x)
            assert xs.sites(sh.seq, sh.strand, xs.START_CODONS) == [start]
        else:
            assert not m["nodes"][0].open and len(xs.sites(sh.seq, sh.strand, xs.STOP_CODONS)) == 3
        key = (sh.strand, m["where"], m["k"])
        combos[key] = combos.get(key, 0) + int(m["nodes"][1].open)
    # per strand: x left of the tile and x inside it, with the start 1, 2, 30 and 400 codons left of the tile, each with a stop node ...
    for strand in (1, -1):
        for where in ("below", "at"):
            for k in xs.LEFT_START_CODONS:
                assert combos[(strand, where, k)] > 0, (strand, where, k)
            assert combos[(strand, where, "none")] == 0            # ... and never when the start lies beyond the previous stop
    assert {m for _, m in xs.LEFT_STOP_OFFSETS} == {"below", "at"} and [o - 87 for o, m in xs.LEFT_STOP_OFFSETS if m == "at"] == [0, 11, 12, 100]
    assert present > 0 and absent > 0 and present + absent == 4 * len(shapes)


def test_lone_stop_series_holds_one_stop_at_every_chunk_edge():
    shapes = xs.lone_stop_series()
    assert set(xs.LONE_OFFSETS) == {0, 1, 2, 3069} | set(range(381, 387)) | set(range(765, 771)) | set(range(2686, 2691))
    lone = [sh for sh in shapes if "p" in sh.meta]
    assert sorted(sh.meta["p"] for sh in lone) == sorted(2 * xs.LONE_OFFSETS)
    for sh in lone:
        L, p = len(sh.seq), sh.meta["p"]
        assert L == 3 * xs.TILE
        stops = xs.sites(sh.seq, sh.strand, xs.STOP_CODONS)
        assert [s for s in stops if s < 2 * xs.TILE] == [xs.TILE + p] and len(stops) == 4       # tile 0 none, tile 1 this one, three at the end
        for closed in (False, True):
            nodes, _ = oracle_nodes(sh.seq, closed=closed)
            mine = nodes[nodes["strand"] == sh.strand]
            local = lambda v: v.astype(np.int64) if sh.strand == 1 else L - 1 - v.astype(np.int64)
            at, sv = local(mine["ndx"]), local(mine["stop_val"])
            starts = (mine["type"] != xs.T_STOP) & (mine["edge"] == 0)
            # the three start codons of p's frame in tile 0 end at p, across the tile boundary
            assert sorted(at[starts & (sv == xs.TILE + p)]) == [a for a, _ in xs._starts_at(300) + xs._starts_at(1500) + xs._starts_at(2900) if a % 3 == p % 3]
            # ... and p is the stop value of the stop node that follows it, two tiles on
            follows = at[(mine["type"] == xs.T_STOP) & (sv == xs.TILE + p)]
            assert len(follows) == 1 and follows[0] >= 3 * xs.TILE - 11
            # the start codons of the other two frames in tile 0 end beyond tile 1
            assert int((starts & (at < xs.TILE) & (sv >= 3 * xs.TILE - 11)).sum()) == 6
    assert sorted(sh.meta["last_tile"] for sh in shapes if "last_tile" in sh.meta) == sorted(2 * xs.LAST_TILE_LENGTHS)
    for sh in shapes:
        if "last_tile" in sh.meta:
            assert len(sh.seq) - 2 * xs.TILE == sh.meta["last_tile"]
    five = [sh for sh in shapes if "empty_tiles" in sh.meta]
    assert len(five) == 2
    for sh in five:
        nodes, _ = oracle_nodes(sh.seq)
        assert len(sh.seq) == 5 * xs.TILE and xs.tile_node_counts(nodes, len(sh.seq))[1:4].tolist() == [0, 0, 0]
        assert all(s < xs.TILE or s >= 4 * xs.TILE for strand in (1, -1) for s in xs.sites(sh.seq, strand, xs.STOP_CODONS + xs.START_CODONS))
        spans = np.abs(nodes["stop_val"].astype(np.int64) - nodes["ndx"].astype(np.int64))
        assert int(spans.max()) > 4 * xs.TILE                       # an ORF across the three empty tiles


def test_ends_series_occupies_every_edge_position():
    shapes = xs.ends_series()
    assert xs.END_LENGTHS == tuple(range(3, 21)) + tuple(range(87, 97))
    assert {L % 3 for L in range(3, 21)} == {L % 3 for L in range(87, 97)} == {0, 1, 2}
    by_len = {}
    for sh in shapes:
        by_len.setdefault(sh.meta["L"], []).append(sh)
        assert len(sh.seq) == sh.meta["L"]
        if "start" in sh.meta:
            assert xs.sites(sh.seq, sh.strand, xs.START_CODONS) == [sh.meta["start"]]
        if "stop" in sh.meta:
            assert xs.sites(sh.seq, sh.strand, xs.STOP_CODONS) == [sh.meta["stop"]]
    for L in xs.END_LENGTHS:
        group = by_len[L]
        if L >= 6:          # every frame's edge start and virtual stop holds a codon of its own, on either strand
            for strand in (1, -1):
                assert sorted(sh.meta["start"] for sh in group if sh.strand == strand and "start" in sh.meta and "stop" not in sh.meta) == [0, 1, 2]
                assert sorted(sh.meta["stop"] for sh in group if sh.strand == strand and "stop" in sh.meta and "start" not in sh.meta) == sorted(xs.virtual_stop(L, f) for f in range(3))
        for sh in group:
            open_nodes, _ = oracle_nodes(sh.seq)
            closed_nodes, _ = oracle_nodes(sh.seq, closed=True)
            if L <= 20:
                assert len(open_nodes) == 0 and len(closed_nodes) == 0
            elif sh.name.endswith("bare/+"):
                long_frames = [f for f in range(3) if xs.virtual_stop(L, f) - f > 60]
                assert len(open_nodes) == 4 * len(long_frames) and len(closed_nodes) == 0 and bool(open_nodes["edge"].all())
    assert sum(len(oracle_nodes(sh.seq)[0]) for sh in shapes) > 1000


def test_neighbour_series_would_form_a_codon_across_every_boundary():
    batch = xs.neighbour_series()
    assert len(batch) == 4 * len(xs.NEIGHBOUR_ENDS) * len(xs.NEIGHBOUR_BEGINS)
    formed = []
    for k in range(0, len(batch), 4):
        left, right, rc_right, rc_left = batch[k:k + 4]
        assert rc_right == xs.revcomp(right) and rc_left == xs.revcomp(left)
        cut = len(left) - len(left) % 3                           # the codon of the ORF's frame that the end cuts off
        assert left[:6] == b"TAAATG" and cut == 111 and 0 < len(left) - cut < 3
        joined = (left + right)[cut:cut + 3]
        assert xs.revcomp((rc_right + rc_left)[len(rc_right) - (cut + 3 - len(left)):][:3]) == joined     # and in the mirror image
        nodes, _ = oracle_nodes(left)
        assert len(nodes) > 0 and len(oracle_nodes(right)[0]) > 0
        if joined not in xs.STOP_CODONS + xs.START_CODONS:
            continue
        formed.append(joined)
        # with the neighbour's letters appended the nodes WOULD differ
        other, _ = oracle_nodes(left + right[:3 - (len(left) - cut)])
        assert len(other) != len(nodes) or any(not np.array_equal(other[f], nodes[f]) for f in TOPO)
    assert len(formed) == 10                                       # of the 16 pairs (T|AC, T|GC, AT|A., TT|A. form none)
    formed = set(formed)
    assert formed == {b"TAA", b"TAG", b"TGA", b"ATG", b"TTG"}


@pytest.mark.parametrize("min_mask", [10, 50])
def test_unknown_series(min_mask):
    shapes = xs.unknown_series(min_mask)
    assert len(shapes) == 2 * (3 * 3 + 1 + 3 * 3 * 2)
    start = xs.Node("start", xs._ORF_START, True, True)
    for sh in shapes:
        assert sh.seq.count(b"N") == sh.meta["run"][1] - sh.meta["run"][0]
        nodes, masks = oracle_nodes(sh.seq, min_mask=min_mask)
        plain, _ = oracle_nodes(sh.seq)
        n = sh.seq.count(b"N")
        kind = sh.name.split("/")[2]
        assert len(masks) == int(n >= min_mask)
        if kind.startswith("start"):
            assert hits(sh, nodes, start) == 0 and hits(sh, plain, start) == 0      # a codon with an unknown base is no start
        elif kind == "after":                                                       # a masked run inside the ORF hides the start
            assert hits(sh, nodes, start) == int(n < min_mask) and hits(sh, plain, start) == 1
        else:                                                                       # far / near / inside / before: the start stays
            assert hits(sh, nodes, start) == 1 and hits(sh, plain, start) == 1
        if kind.startswith("near") or kind.startswith("far"):                       # ... on an ORF that no longer ends at that stop
            ref, _ = oracle_nodes(bytes(xs._one_orf()) if sh.strand == 1 else xs.revcomp(bytes(xs._one_orf())))
            pick = lambda a: a[(a["strand"] == sh.strand) & (a["type"] != xs.T_STOP) & (a["edge"] == 0)]
            assert (pick(nodes)["stop_val"][0] != pick(ref)["stop_val"][0]) == kind.startswith("near")
    runs = sorted({(sh.name.split("/")[2], sh.meta["run"][1] - sh.meta["run"][0]) for sh in shapes if "/m" in sh.name})
    assert runs == sorted((k, m) for k in ("after", "before") for m in (min_mask - 1, min_mask, min_mask + 1))


def test_region_series_and_the_boundary_case():
    shapes = xs.region_series()
    got = {}
    for sh in shapes:
        assert sh.regions == union(sh.regions) and all(0 <= b < e <= len(sh.seq) for b, e in sh.regions)
        assert b"N" not in sh.seq                                  # real bases under every interval
        for closed in (False, True):
            ndx, stop_val, typ, strand, edge = extract_ref(sh.seq, sh.regions, closed=closed)
            nodes = dict(ndx=ndx, strand=strand, type=typ)
            for nd in sh.meta.get("nodes", []):
                assert hits(sh, nodes, nd) == int(nd.open), (sh.name, nd)
            got[(sh.name, closed)] = hits(sh, nodes, xs.Node("start", xs._ORF_START, True, True))
        lower = xs.lower_cased(sh)
        assert lower.upper() == sh.seq and sum(c > 96 for c in lower) == sum(e - b for b, e in sh.regions)
    for tag in ("+", "-1"):                                        # the second region hides the first from the ORF
        for closed in (False, True):
            assert got[("region/two/" + tag, closed)] == 1 and got[("region/one/" + tag, closed)] == 0
            assert got[("region/begin_at_last/" + tag, closed)] == 1 and got[("region/begin_at_last-1/" + tag, closed)] == 0
            assert got[("region/end_at_i/" + tag, closed)] == 1 and got[("region/end_at_i+1/" + tag, closed)] == 0
    # the reverse strand's test is the forward one moved by a base: the unmoved mirror image of the boundary case is masked
    assert got[("region/begin_at_last/-0", False)] == 0 and got[("region/two/-0", False)] == 0
    # without the regions every ORF has its start
    plain = extract_ref(shapes[0].seq)
    assert hits(shapes[0], dict(ndx=plain[0], strand=plain[3], type=plain[2]), xs.Node("start", xs._ORF_START, True, True)) == 1


def test_digitise_series_puts_a_boundary_everywhere():
    first, second = xs.digitise_series()
    assert sorted(first) == sorted(second) and first != second
    for seqs in (first, second):
        b = xs.boundaries(seqs)
        assert set((b % 16).tolist()) == set(range(16))
    b = xs.boundaries(first)
    for piece in xs.DIGITISE_PIECES:                               # a boundary just below and just above a multiple of every piece size
        assert piece - 1 in b and piece + 1 in b
        assert {piece + d for d in (-17, -1, 0, 1, 17)} <= {len(s) for s in first}
    assert set(range(41)) <= {len(s) for s in first}
    assert set(b"".join(first)) == set(range(256))
    assert b"G" * 40000 in first and b"N" * 40000 in first
    gc = [orc.Oracle(s).gc for s in first]
    assert max(gc) == 1.0 and min(gc) == 0.0 and len(set(gc)) > 30


def test_tile_count_series():
    batches = xs.tile_count_series()
    assert tuple(sorted(batches)) == (4095, 4096, 4097, 8193)
    for n, seqs in batches.items():
        assert xs.n_tiles(seqs) == n == len(seqs) and all(100 <= len(s) <= 200 for s in seqs)
    kinds = set(batches[8193])
    assert len(kinds) == 101 and all(len(oracle_nodes(s)[0]) >= 2 for s in kinds)


def test_staging_series_holds_the_named_node_counts():
    count = lambda s: xs.tile_node_counts(oracle_nodes(s)[0], len(s))
    series = xs.staging_series(count)
    assert sorted(series) == sorted(["room-1", "room", "room+1", "edge3"] + ["place%d" % c for c in xs.PLACE_COUNTS])
    for name, delta in (("room-1", -1), ("room", 0), ("room+1", 1)):
        s = series[name]
        counts = count(s)
        assert len(counts) == 2 and counts[1] == xs.room(len(s) - xs.TILE, xs.STAGING_SHIFT) + delta
        assert counts[0] <= xs.room(xs.TILE, xs.STAGING_SHIFT)
        assert counts[1] < xs.room(len(s) - xs.TILE, 1)            # the default shift has room to spare (see staging_series)
    for c in xs.PLACE_COUNTS:
        s = series["place%d" % c]
        assert count(s).tolist()[1] == c and c <= xs.room(len(s) - xs.TILE, 1)
    s = series["edge3"]
    nodes, _ = oracle_nodes(s)
    assert len(s) == xs.TILE + 3 and count(s)[1] == 4 and bool(nodes["edge"][nodes["ndx"] >= xs.TILE].all())
    assert len(oracle_nodes(s, closed=True)[0][oracle_nodes(s, closed=True)[0]["ndx"] >= xs.TILE]) == 0


def test_gc_window_table():
    """The three contigs of the GC-window test and the six model GC values around each of their bounds."""
    table = xs.gc_window_table()
    assert [name for name, _, _, _ in table] == ["unclamped", "low_clamped", "high_clamped"]
    for name, seq, low, high in table:
        gc = sets_ref.gc_count(seq) / len(seq)
        assert (low, high) == sets_ref.window(gc) and gc == orc.Oracle(seq).gc
        assert (low == 0.65) == (name == "low_clamped") and (high == 0.35) == (name == "high_clamped")
        values = xs.gc_window_values(low, high)
        assert [v for v, _ in values] == [low, math.nextafter(low, -1.0), math.nextafter(low, 1.0), high, math.nextafter(high, -1.0), math.nextafter(high, 2.0)]
        assert [keep for _, keep in values] == [True, False, True, True, True, False]
        for v, keep in values:
            assert (not (v < low or v > high)) == keep
            m = xs.gc_window_model(); m.set_gc(v)
            o = orc.Oracle(seq)
            assert o.find_genes_meta([m]) == (0 if keep else -1) and (o.num_genes > 5) == keep       # a kept model does call genes
