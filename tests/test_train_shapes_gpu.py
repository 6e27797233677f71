"""The training on the device (pyrodigal_amd/csrc/train.inl) against the oracle, byte for byte, on the genomes of
tests/train_shapes.py: every genome alone at every stage, and packed into batches of 1 .. 257 genomes of unequal length with
empty genomes, neighbours of a few nodes, mixed tables, start weights and start models.  tests/test_train_cpu.py asserts which
side of every rule these genomes reach; here a wrong window, comparison or bound changes a byte of a named genome."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc
from tests import train_ref as tr
from tests import train_shapes as ts

pytestmark = pytest.mark.gpu

UPTO = (1, 2, 3, 0)


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def want():
    """The oracle's blob of (sequence, options, stage), computed once per module; None for a genome without a node."""
    cache = {}

    def get(seq, upto, translation_table=11, start_weight=4.35, force_nonsd=False, closed=False, min_gene=90, mask=False):
        key = (seq, upto, translation_table, start_weight, bool(force_nonsd), closed, min_gene, mask)
        if key not in cache:
            o = orc.Oracle(seq, mask=mask)
            p = orc.Params(closed=closed, min_gene=min_gene)
            if o.extract(translation_table, p) == 0:
                cache[key] = None
            else:
                cache[key] = o.train(p, force_nonsd=force_nonsd, start_weight=start_weight, tt=translation_table, upto=upto).tobytes()
        return cache[key]
    return get


# ---- every genome alone -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("upto", UPTO)
@pytest.mark.parametrize("name", list(ts.SERIES))
def test_every_genome_alone(ctx, want, name, upto):
    bad, refused = [], 0
    for g in ts.series(name):
        w = want(g.seq, upto, **g.opts)
        if w is None:
            with pytest.raises(ValueError, match="no start / stop node"):
                ctx.train(g.seq, upto=upto, **g.opts)
            refused += 1
            continue
        d = tr.differing_fields(ctx.train(g.seq, upto=upto, **g.opts), w)                # byte for byte, NaNs included
        if d:
            bad.append((g.tag, g.side, d))
    assert bad == []
    assert refused == (6 if name == "degenerate" else 0)


# ---- batches ------------------------------------------------------------------------------------------------------------------------

def train_batch(ctx, members, upto, closed=False, mask=False):
    """pga_train_batch at the C level: (return code, status per genome, blob per genome)."""
    from pyrodigal_amd import _cabi
    n = len(members)
    b = _cabi.Batch(ctx, [m.seq for m in members])
    try:
        p = _cabi.Params(int(closed), 90, 60, 60, 0, 0, int(mask), 50)
        out = np.zeros(n * _cabi.TRAINING_SIZE, np.uint8)
        status = np.full(n, 99, np.int32)
        tt = np.asarray([m.translation_table for m in members], np.int32)
        sw = np.asarray([m.start_weight for m in members], np.float64)
        fn = np.asarray([int(m.force_nonsd) for m in members], np.int32)
        rc = ctx.L.pga_train_batch(ctx.h, b.h, ctypes.byref(p), tt.ctypes.data, sw.ctypes.data, fn.ctypes.data, int(upto), out.ctypes.data,
                                   status.ctypes.data)
    finally:
        b.close()
    return rc, status.tolist(), [out[g * _cabi.TRAINING_SIZE:(g + 1) * _cabi.TRAINING_SIZE].tobytes() for g in range(n)]


def check_batch(ctx, want, members, upto, **kw):
    from pyrodigal_amd import _cabi
    rc, status, got = train_batch(ctx, members, upto, **kw)
    assert rc == 0
    bad = []
    for g, m in enumerate(members):
        w = want(m.seq, upto, m.translation_table, m.start_weight, m.force_nonsd, **kw)
        if w is None:
            if status[g] != _cabi.PGA_EINVAL:
                bad.append((g, "status", status[g]))
        elif status[g] != 0 or got[g] != w:
            bad.append((g, status[g], tr.differing_fields(got[g], w)))
    assert bad == []
    return got


@pytest.fixture(scope="module")
def loaded():
    """A context with the meta-mode model set loaded, and what it finds before any training: every batch below trains on this context,
    and the same call afterwards must find the same (the training runs its half-trained models through the context's model slots and
    puts the caller's set back)."""
    from pyrodigal_amd import _cabi, benchdata
    c = _cabi.Context(0)
    c.set_models([m[1] for m in benchdata.load_model_set()])
    seqs = [benchdata.synthetic_contig(20000, gc, 60 + i) for i, gc in enumerate((0.4, 0.55))]
    before = c.find_genes_batch(seqs, meta=True)

    def unchanged():
        after = c.find_genes_batch(seqs, meta=True)
        assert np.array_equal(before.contigs["model"], after.contigs["model"])
        assert before.genes.tobytes() == after.genes.tobytes()
    yield c, unchanged
    c.close()


@pytest.mark.parametrize("upto", UPTO)
@pytest.mark.parametrize("G", ts.BATCH_SIZES)
def test_every_batch(loaded, want, G, upto):
    c, unchanged = loaded
    members, empty_at = ts.batch(G)
    assert len(members) == G and (empty_at is None or want(members[empty_at].seq, upto) is None)
    assert len({m.translation_table for m in members}) <= 4
    check_batch(c, want, members, upto)
    unchanged()


@pytest.mark.parametrize("G", [G for G in ts.BATCH_SIZES if G > 1])
def test_every_batch_in_another_order(loaded, want, G):
    c, unchanged = loaded
    members, _ = ts.batch(G)
    perm = ts.permutation(G)
    assert perm != list(range(G))
    check_batch(c, want, [members[k] for k in perm], 0)
    unchanged()


def test_the_batch_has_what_it_is_for():
    """The batches hold what the batch dimension can get wrong: neighbours with a handful of nodes, two neighbours with one sequence,
    an empty genome first, last and at a boundary of 64, the longest genome first, in the middle and last, both start models.  (What
    a stop's walk meets in a neighbour is in tests/test_train_cpu.py: test_no_walk_of_a_stop_takes_a_node_of_a_neighbouring_genome.)"""
    places = set()
    for G in ts.BATCH_SIZES:
        members, empty_at = ts.batch(G)
        lens = [len(m.seq) for m in members]
        places.add("first" if lens.index(max(lens)) == 0 else ("last" if lens.index(max(lens)) == G - 1 else "middle"))
        if G >= 63:
            nn = [ts.n_nodes(m.seq, m.translation_table) for m in members[:40]]
            assert any(0 < a < 20 and 0 < b < 20 for a, b in zip(nn, nn[1:]))
            assert any(a.seq == b.seq for a, b in zip(members, members[1:]))
            assert len({m.translation_table for m in members}) == 4 and len({m.start_weight for m in members}) == 3
        if empty_at is not None:
            places.add(("empty", "first" if empty_at == 0 else ("last" if empty_at == G - 1 else empty_at % 64)))
    assert places >= {"first", "middle", "last", ("empty", "first"), ("empty", "last"), ("empty", 63)}


def test_five_tables_in_one_call_are_refused(ctx, want):
    from pyrodigal_amd import _cabi
    members = [ts.Member(g.seq, tt, 4.35, False) for g, tt in zip(ts.series("tie"), ts.FIVE_TABLES)]
    rc, status, _ = train_batch(ctx, members, 0)
    assert rc == _cabi.PGA_EINVAL
    with pytest.raises(ValueError, match="more than 4 distinct translation tables"):
        ctx.train_batch([m.seq for m in members], translation_table=list(ts.FIVE_TABLES))
    check_batch(ctx, want, members[:4], 0)                                  # four of them are taken


@pytest.mark.parametrize("closed", [False, True])
def test_a_batch_with_masked_runs(ctx, want, closed):
    """mask=True and closed ends belong to the call: genomes with runs of N (one of 49, below the shortest masked run), the genome of N
    alone (twelve edge nodes with open ends, none with closed ends), and unmasked neighbours."""
    seqs = [g.seq for g in ts.series("degenerate") if g.tag[0] in ("n_runs", "edge_nodes_only")] + [g.seq for g in ts.series("tie")]
    members = [ts.Member(s, 11, 4.35, k % 3 == 0) for k, s in enumerate(seqs)]
    for upto in UPTO:
        check_batch(ctx, want, members, upto, closed=closed, mask=True)


def test_neighbours_of_an_empty_genome_equal_their_solo_training(ctx):
    """The device against itself: what a genome's neighbours are, and whether one of them is refused, changes nothing.  At G = 65 the
    empty genome stands last, at G = 257 in the middle (place 63): the genome before it, the one after it where there is one, the first and the last."""
    for G in (65, 257):
        members, empty_at = ts.batch(G)
        rc, status, got = train_batch(ctx, members, 0)
        assert rc == 0 and status[empty_at] == -1 and status.count(0) == G - 1
        near = {empty_at - 1, empty_at + 1, 0, G - 1} - {empty_at, G}
        assert len(near) == (2 if G == 65 else 4)
        for g in sorted(near):
            m = members[g]
            assert got[g] == ctx.train(m.seq, translation_table=m.translation_table, start_weight=m.start_weight, force_nonsd=m.force_nonsd), (G, g)
