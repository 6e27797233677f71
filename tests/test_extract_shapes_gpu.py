"""The front end -- k_digitize, the GC prefix, k_tile_stops, k_extract_tile / extract_strand, k_scan_counts, k_place_nodes,
k_group_enable -- on the catalogue of tests/extract_shapes.py, bit for bit against the CPU oracle (and against tests/extract_ref.py
where the masks cover known bases).  tests/test_extract_shapes_cpu.py proves from the oracle alone that the catalogue sits on both
sides of every threshold; here only the device is in question."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import extract_shapes as xs
from tests.extract_ref import extract_ref, union
from tests.test_finder_gpu import compare_contig
from tests.test_stages_gpu import TOPO, check
from tests.util import golden_path

pytestmark = pytest.mark.gpu

KNOBS = {"default": {}, "slab": {"PGA_EXTRACT_C": "0"}}          # compact stop-value lists / a value for every position
_ORACLE = {}


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sd():
    """The SD model of tests/start_shapes.py: base_models()["sd"] (loaded alone: the other two base models are trained)."""
    t = orc.Training.load(golden_path("SRR492066.training.bin.gz"))
    assert t.uses_sd == 1 and t.trans_table == 11
    return t


def oracle_nodes(seq, stage=1, tinf=None, tt=11, closed=False, min_gene=90, min_edge_gene=60, min_mask=None):
    """The oracle's nodes of one contig, computed once and left unchanged."""
    key = (seq, stage, tt, closed, min_gene, min_edge_gene, min_mask)
    if key not in _ORACLE:
        o = orc.Oracle(seq, mask=min_mask is not None, mask_size=min_mask or 0)
        o.extract(tt, orc.Params(closed=closed, min_gene=min_gene, min_edge_gene=min_edge_gene))
        o.sort()
        if stage >= 2:
            o.reset_scores()
            o.score_nodes(tinf, closed, False)
        _ORACLE[key] = o.nodes()
    return _ORACLE[key]


def orders(seqs):
    """As built, reversed, rotated by one (which moves every contig's first base to another residue mod 16): (batch, index of seqs)."""
    n = len(seqs)
    for idx in (list(range(n)), list(range(n))[::-1], list(range(1, n)) + [0]):
        yield [seqs[k] for k in idx], idx


def set_knobs(monkeypatch, env):
    for k in ("PGA_EXTRACT_C", "PGA_EXTRACT_POOL", "PGA_STAGE_SHIFT", "PGA_STAGE_FULL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def run_and_check(ctx, seqs, stage=1, tinf=None, tt=11, closed=False, min_gene=90, min_edge_gene=60, min_mask=None, all_orders=False):
    """The batch (in three orders: the results of a contig must not depend on its place) against the oracle; returns the node total."""
    total = 0
    for batch, idx in orders(seqs) if all_orders else [(seqs, range(len(seqs)))]:
        kw = dict(mask=True, min_mask=min_mask) if min_mask is not None else {}
        out = ctx.nodes_stage(batch, stage, translation_table=tt, closed=closed, min_gene=min_gene, min_edge_gene=min_edge_gene, **kw)
        assert len(out) == len(batch)
        for nd, s in zip(out, batch):
            check(nd, oracle_nodes(s, stage, tinf, tt, closed, min_gene, min_edge_gene, min_mask), stage)
            total += nd["n"]
    return total


SERIES = {
    "length": lambda: [([sh.seq for sh in xs.length_series(mg, meg)], dict(min_gene=mg, min_edge_gene=meg)) for mg, meg in xs.GENE_LENGTHS],
    "phase": lambda: [([sh.seq for sh in xs.phase_series()], dict(all_orders=True))],
    "left_of_tile": lambda: [([sh.seq for sh in xs.left_of_tile_series()], dict(all_orders=True))],
    "lone_stop": lambda: [([sh.seq for sh in xs.lone_stop_series()], {})],
    "ends": lambda: [([sh.seq for sh in xs.ends_series()], dict(all_orders=True))],
    "neighbour": lambda: [(xs.neighbour_series(), {})],
    "unknown": lambda: [([sh.seq for sh in xs.unknown_series(mm)], dict(min_mask=use)) for mm in (10, 50) for use in (None, 0, mm)],
}


@pytest.mark.parametrize("knob", list(KNOBS))
@pytest.mark.parametrize("tt", [11, 4])
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("series", list(SERIES))
def test_series_at_the_extraction_stage(ctx, monkeypatch, series, closed, tt, knob):
    from pyrodigal_amd import _cabi
    set_knobs(monkeypatch, KNOBS[knob])
    total = 0
    for seqs, kw in SERIES[series]():
        total += run_and_check(ctx, seqs, _cabi.STAGE_EXTRACT, tt=tt, closed=closed, **kw)
        assert ctx.extract_stats()["passes"] == 1
    assert total > 0 or (closed and series == "neighbour")        # (whose ORFs all run off an end)


def end_sensitive_contigs():
    """What happens within sixteen bases of an end: the ends series from 87 bases on and the ORFs of the length series that run off an
    end."""
    out = [sh.seq for sh in xs.ends_series() if len(sh.seq) >= 87]
    out += [sh.seq for sh in xs.length_series(90, 60) if sh.meta["kind"] != "closed_orf"]
    return out


def test_first_and_last_of_a_batch(ctx):
    """strand_codon_masks reads sixteen bytes at once unless they begin before the batch (the reverse strand at the left end of the
    batch's first contig) or end behind it (the forward strand at the right end of its last): every contig whose nodes lie at an end
    as the first and as the last of a batch, next to a neighbour whose letters would change its codons."""
    from pyrodigal_amd import _cabi
    seqs = end_sensitive_contigs()
    assert len(seqs) > 200
    filler = b"AATG" + xs.quiet(90) + b"TGATT"
    total = 0
    for s in seqs:
        first = ctx.nodes_stage([s, filler], _cabi.STAGE_EXTRACT)
        last = ctx.nodes_stage([filler, s], _cabi.STAGE_EXTRACT)
        on = oracle_nodes(s)
        check(first[0], on, 1)
        check(last[1], on, 1)
        check(first[1], oracle_nodes(filler), 1)
        check(last[0], oracle_nodes(filler), 1)
        total += len(on)
    assert total > 1000


SCORED = {
    "length": lambda: [([sh.seq for sh in xs.length_series(mg, meg)], dict(min_gene=mg, min_edge_gene=meg)) for mg, meg in xs.GENE_LENGTHS],
    "phase": lambda: [([sh.seq for sh in xs.phase_series()], {})],
    "lone_stop": lambda: [([sh.seq for sh in xs.lone_stop_series()], {})],
    "unknown": lambda: [([sh.seq for sh in xs.unknown_series(50)], dict(min_mask=use)) for use in (None, 50)],
}


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("series", list(SCORED))
def test_series_at_the_scoring_stage(ctx, sd, monkeypatch, series, closed):
    """gc_cont at every ndx % 16 and every residue of a contig's first base (gc_prefix adds a partial group of 1 .. 15 bases to a prefix
    kept per 16 BATCH positions), c16 of tiles that hold no node (read by the ORF walks only), the coding score of ORFs that cross
    them."""
    from pyrodigal_amd import _cabi
    set_knobs(monkeypatch, {})
    ctx.set_models([sd.buf])
    for seqs, kw in SCORED[series]():
        bases = set()
        for batch, _ in orders(seqs):
            bases |= set((xs.boundaries(batch)[:-1] % 16).tolist())
        assert len(bases) == 16 or series in ("lone_stop", "unknown")      # (whole tiles, and 600 bases each: fewer residues)
        assert run_and_check(ctx, seqs, _cabi.STAGE_SCORE, tinf=sd, closed=closed, all_orders=True, **kw) > 0
    if series == "phase":
        on = [oracle_nodes(s, 2, sd, closed=closed) for s in SCORED["phase"]()[0][0]]
        assert {int(x) % 16 for n in on for x in n["ndx"]} == set(range(16))


def check_topo(nd, ref, what):
    assert nd["n"] == len(ref[0]), what
    for k, name in enumerate(TOPO):
        assert np.array_equal(nd[name].astype(np.int64), ref[k]), (what, name)


@pytest.mark.parametrize("tt", [11, 4])
@pytest.mark.parametrize("closed", [False, True])
def test_named_regions_over_known_bases(ctx, closed, tt):
    """mask_bound with the one-mask-per-ORF rule of DESIGN.md 4.9 -- the boundary case included -- against the plain restatement of
    the sweep that takes the mask list as an argument; the same intervals as lower-case runs."""
    from pyrodigal_amd import _cabi
    shapes = xs.region_series()
    seqs = [sh.seq for sh in shapes]
    ref = [extract_ref(sh.seq, sh.regions, tt, closed) for sh in shapes]
    plain = [extract_ref(sh.seq, (), tt, closed) for sh in shapes]
    assert sum(len(a[0]) != len(b[0]) for a, b in zip(ref, plain)) >= 10          # the regions do hide nodes
    for batch, idx in orders(seqs):
        out = ctx.nodes_stage(batch, _cabi.STAGE_EXTRACT, translation_table=tt, closed=closed, regions=[shapes[k].regions for k in idx])
        for nd, k in zip(out, idx):
            check_topo(nd, ref[k], shapes[k].name)
        lower = ctx.nodes_stage([xs.lower_cased(shapes[k]) for k in idx], _cabi.STAGE_EXTRACT, translation_table=tt, closed=closed,
                                mask_lowercase=True, min_mask=1)
        for nd, k in zip(lower, idx):
            check_topo(nd, ref[k], shapes[k].name + " (lower case)")
    # the reported lists are the intervals themselves
    r = ctx.nodes_stage(seqs, _cabi.STAGE_SEQUENCE, regions=[sh.regions for sh in shapes])
    assert [m.tolist() for m in r.masks] == [[list(iv) for iv in union(sh.regions)] for sh in shapes]


@pytest.mark.parametrize("order", [0, 1])
def test_digitise_series(ctx, order):
    from pyrodigal_amd import _cabi
    seqs = xs.digitise_series()[order]
    known = np.zeros(256, bool)
    known[list(b"ACGTacgt")] = True
    for min_mask in (0, 50):
        r = ctx.nodes_stage(seqs, _cabi.STAGE_SEQUENCE, mask=True, min_mask=min_mask)
        for i, s in enumerate(seqs):
            o = orc.Oracle(s, mask=True, mask_size=min_mask)
            assert np.float64(r.contigs["gc"][i]).view(np.uint64) == np.float64(o.gc).view(np.uint64), (i, len(s))
            assert r.contigs["n_unknown"][i] == int((~known[np.frombuffer(s, np.uint8)]).sum()), (i, len(s))
            assert r.masks[i].tolist() == o.masks().tolist(), (i, len(s), min_mask)
    assert run_and_check(ctx, seqs, _cabi.STAGE_EXTRACT) > 0        # the only view of the digits themselves


@pytest.mark.parametrize("n", xs.TILE_COUNTS)
def test_tile_count_series(ctx, n):
    from pyrodigal_amd import _cabi
    seqs = xs.tile_count_series()[n]
    assert xs.n_tiles(seqs) == n
    total = run_and_check(ctx, seqs, _cabi.STAGE_EXTRACT)
    assert total == sum(len(oracle_nodes(s)) for s in seqs) and total >= 2 * n


def _staging(closed=False):
    count = lambda s: xs.tile_node_counts(oracle_nodes(s, closed=closed), len(s))
    return xs.staging_series(count)


def find(ctx, seqs):
    res = ctx.find_genes_batch(seqs, meta=False, want_nodes=True)
    return res, ctx.extract_stats()["passes"]


def same_results(a, b, n):
    assert a.genes.tobytes() == b.genes.tobytes() and np.array_equal(a.contigs["n_nodes"], b.contigs["n_nodes"])
    for i in range(n):
        for k in TOPO:
            assert a.nodes[i][k].tobytes() == b.nodes[i][k].tobytes(), (i, k)


def test_staging_room(ctx, monkeypatch):
    """A tile overflows its staging slots iff it holds MORE nodes than room = (len >> shift) + PGA_STAGE_SLACK: exactly room - 1 and
    room take one pass, room + 1 takes two, and the results are those of full staging and of the oracle either way.  At
    PGA_STAGE_SHIFT=2 -- at the default of 1 no sequence fills a tile's room (tests/extract_shapes.py: staging_series) -- and set
    explicitly, so that the overflow does not stick to the context."""
    from pyrodigal_amd import _cabi
    series = _staging()
    tinf = orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz"))
    ordinary = [xs.gc_window_table()[0][1]]
    ctx.set_models([tinf.buf])
    fresh = _cabi.Context(0)
    try:
        fresh.set_models([tinf.buf])
        for name, passes in (("room-1", 1), ("room", 1), ("room+1", 2)):
            seqs = [series[name], ordinary[0]]
            set_knobs(monkeypatch, {"PGA_STAGE_SHIFT": str(xs.STAGING_SHIFT)})
            res, got = find(ctx, seqs)
            assert got == passes, name
            for i, s in enumerate(seqs):
                compare_contig(res, i, s, orc.Oracle(s), [tinf], meta=False)
            set_knobs(monkeypatch, {"PGA_STAGE_FULL": "1"})
            full, got = find(fresh, seqs)
            assert got == 1
            same_results(res, full, len(seqs))
        # the call after the overflow is back on one pass: under the same knob ...
        set_knobs(monkeypatch, {"PGA_STAGE_SHIFT": str(xs.STAGING_SHIFT)})
        assert find(ctx, [series["room"]])[1] == 1
        # ... and without it (the context did not keep full staging, which takes one pass whatever the input)
        set_knobs(monkeypatch, {})
        assert find(ctx, ordinary)[1] == 1
        set_knobs(monkeypatch, {"PGA_STAGE_SHIFT": str(xs.STAGING_SHIFT)})
        assert find(ctx, [series["room+1"]])[1] == 2
    finally:
        set_knobs(monkeypatch, {})
        fresh.close()


@pytest.mark.parametrize("closed", [False, True])
def test_placement_rounds_and_a_three_base_tile(ctx, monkeypatch, closed):
    """k_place_nodes moves 128 nodes per round: tiles of exactly 128, 129, 256 and 257 nodes; and a last tile of three bases that
    holds four edge nodes of an open contig (its staging room is the slack alone)."""
    from pyrodigal_amd import _cabi
    set_knobs(monkeypatch, {})
    series = _staging(closed)                                      # (the run lengths that give these counts with the contig closed)
    seqs = [series["place%d" % c] for c in xs.PLACE_COUNTS] + [series["edge3"]]
    for c, s in zip(xs.PLACE_COUNTS, seqs):
        assert xs.tile_node_counts(oracle_nodes(s, closed=closed), len(s))[1] == c
    tinf = orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz"))
    ctx.set_models([tinf.buf])
    assert run_and_check(ctx, seqs, _cabi.STAGE_EXTRACT, closed=closed, all_orders=True) >= 3 * sum(xs.PLACE_COUNTS)
    assert ctx.extract_stats()["passes"] == 1
    res = ctx.find_genes_batch(seqs, meta=False, closed=closed, want_nodes=True)
    for i, s in enumerate(seqs):
        compare_contig(res, i, s, orc.Oracle(s), [tinf], meta=False, closed=closed)


@pytest.mark.parametrize("name", ["unclamped", "low_clamped", "high_clamped"])
def test_gc_window_bounds(ctx, monkeypatch, name):
    """k_group_enable keeps a model iff !(gc < low || gc > high): a model whose GC is a bound, the double below it and the double
    above it, for either bound, clamped and not."""
    set_knobs(monkeypatch, {})
    _, seq, low, high = [row for row in xs.gc_window_table() if row[0] == name][0]
    other = xs.quiet(500)                                           # a second contig, outside every one of these windows or inside all
    for v, keep in xs.gc_window_values(low, high):
        m = xs.gc_window_model()
        m.set_gc(v)
        ctx.set_models([m.buf])
        res = ctx.find_genes_batch([seq, other], meta=True, want_nodes=True)
        n = compare_contig(res, 0, seq, orc.Oracle(seq), [m], meta=True)
        compare_contig(res, 1, other, orc.Oracle(other), [m], meta=True)
        assert res.contigs["model"][0] == (0 if keep else -1), (name, v)
        assert (n > 5) == keep, (name, v, n)
