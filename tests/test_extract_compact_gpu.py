"""The extraction's compact stop-value lists: a thread of `k_extract_tile` lists up to C = 4 stop values per strand in
LDS, a pool of the workgroup takes what a thread finds beyond that, and a tile that exhausts the pool has its batch extracted again
by the instantiation that keeps a value for every position.  Results must not depend on C, on the pool or on which path ran: the node
arrays and the genes of every contig against the CPU oracle and against a run with the full-slab kernel forced (PGA_EXTRACT_C=0)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_finder_gpu import compare_contig
from tests.util import golden_path, synthetic_contig

pytestmark = pytest.mark.gpu

TILE = 3072            # pga_extract_tile_size()
WINDOW = 12            # positions of a thread: tiles start at multiples of 3072 = 256 * 12, so a thread owns [12 j, 12 j + 12) of a contig
C_DEFAULT = 4
NODE_KEYS = ("ndx", "stop_val", "type", "strand", "edge")
STOPS = b"TAACTAACTAA"         # a stop codon in each of the three frames
STOPS_RC = b"TTAGTTAGTTA"      # ... of the reverse strand (it reads them to the left of the run)
UNITS = {"GT": (b"GT", 60), "AC": (b"AC", 60), "CATGTG": (b"CATGTG", 40), "TGCA": (b"TGCA", 60)}


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tinf():
    """The single-mode model under translation tables 11 and 4."""
    t11 = orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz"))
    t4 = t11.copy(); t4.set_trans_table(4)
    return {11: t11, 4: t4}


@pytest.fixture(scope="module")
def meta_models(tinf):
    m = [orc.Training.load(golden_path("SRR492066.training.bin.gz")), tinf[11]]
    for src, gc, tt in [(0, 0.36, 11), (1, 0.47, 11), (1, 0.60, 11), (1, 0.42, 4), (0, 0.33, 4), (1, 0.64, 11)]:
        t = m[src].copy(); t.set_gc(gc); t.set_trans_table(tt); m.append(t)
    return m


def dense_block(name):
    unit, n = UNITS[name]
    return STOPS_RC + unit * n + STOPS


def dense_contig(name, seed, gap=None):
    """One dense run at the contig's first bases, one mid-tile, one across the tile boundary (the run itself from three bases before
    3072 on), one at the contig's last bases, on ordinary sequence; `gap`: that many unknown bases written over the far end of each run
    (its first bases; (AC)n, whose nodes are the reverse strand's, its last): a mask there hides the starts under it and leaves the
    others, while a mask anywhere else in the run hides every start on the far side of it."""
    unit, n = UNITS[name]
    run = unit * n
    if gap:
        run = run[:-gap] + b"N" * gap if name == "AC" else b"N" * gap + run[gap:]
    s = bytearray(synthetic_contig(2 * TILE + 900, 0.5, seed))
    first, block, last = run + STOPS, STOPS_RC + run + STOPS, STOPS_RC + run
    s[:len(first)] = first
    s[1500:1500 + len(block)] = block
    at = TILE - 3 - len(STOPS_RC)
    s[at:at + len(block)] = block
    s[len(s) - len(last):] = last
    return bytes(s)


def densest_window(on):
    """Most nodes of one strand in an aligned window of twelve positions, from the oracle's nodes alone."""
    best = 0
    for strand in (1, -1):
        w = on["ndx"][on["strand"] == strand].astype(np.int64) // WINDOW
        if len(w):
            best = max(best, int(np.bincount(w).max()))
    return best


def same_as(res, ref, n):
    assert res.genes.tobytes() == ref.genes.tobytes()
    assert np.array_equal(res.contigs["model"], ref.contigs["model"]) and np.array_equal(res.contigs["n_nodes"], ref.contigs["n_nodes"])
    for i in range(n):
        for k in NODE_KEYS:
            assert res.nodes[i][k].tobytes() == ref.nodes[i][k].tobytes(), (i, k)


def run_with(ctx, monkeypatch, env, seqs, **kw):
    for k in ("PGA_EXTRACT_C", "PGA_EXTRACT_POOL"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    res = ctx.find_genes_batch(seqs, want_nodes=True, **kw)
    passes = ctx.extract_stats()["passes"]
    for k in env:
        monkeypatch.delenv(k)
    return res, passes


@pytest.mark.parametrize("tt", [11, 4])
@pytest.mark.parametrize("closed", [False, True])
def test_dense_runs_go_through_the_pool(ctx, tinf, monkeypatch, tt, closed):
    """(GT)x60 and (AC)x60 hold six nodes of a strand in a thread's twelve positions, (CATGTG)x40 four, (TGCA)x60 three: with the
    default C = 4 the first two reach the pool, with PGA_EXTRACT_C=2 all four do.  One pass each: the pool is for them."""
    names = list(UNITS)
    seqs = [dense_contig(nm, 900 + k) for k, nm in enumerate(names)]
    ctx.set_models([tinf[tt].buf])
    ref, _ = run_with(ctx, monkeypatch, {"PGA_EXTRACT_C": "0"}, seqs, meta=False, closed=closed)
    dens = {}
    for i, (nm, s) in enumerate(zip(names, seqs)):
        o = orc.Oracle(s)
        compare_contig(ref, i, s, o, [tinf[tt]], meta=False, closed=closed)
        dens[nm] = densest_window(o.nodes())
    for c in (C_DEFAULT, 2):
        for nm in names if c == 2 else ("GT", "AC"):
            assert dens[nm] > c, (nm, c, dens)       # otherwise the input does not reach the overflow code
        res, passes = run_with(ctx, monkeypatch, {} if c == C_DEFAULT else {"PGA_EXTRACT_C": str(c)}, seqs, meta=False, closed=closed)
        assert passes == 1
        same_as(res, ref, len(seqs))
        for i, s in enumerate(seqs):
            compare_contig(res, i, s, orc.Oracle(s), [tinf[tt]], meta=False, closed=closed)


def test_dense_runs_under_a_region_mask(ctx, tinf, monkeypatch):
    """A masked region (twelve unknown bases, min_mask 10) over the far end of every run: the starts under it go, the others stay."""
    names = list(UNITS)
    seqs = [dense_contig(nm, 950 + k, gap=12) for k, nm in enumerate(names)]
    ctx.set_models([tinf[11].buf])
    ref, _ = run_with(ctx, monkeypatch, {"PGA_EXTRACT_C": "0"}, seqs, meta=False, mask=True, min_mask=10)
    for c in (C_DEFAULT, 2):
        res, passes = run_with(ctx, monkeypatch, {} if c == C_DEFAULT else {"PGA_EXTRACT_C": str(c)}, seqs, meta=False, mask=True, min_mask=10)
        assert passes == 1
        same_as(res, ref, len(seqs))
        for i, (nm, s) in enumerate(zip(names, seqs)):
            o = orc.Oracle(s, mask=True, mask_size=10)
            compare_contig(res, i, s, o, [tinf[11]], meta=False)
            assert len(o.masks()) >= 4
            if c == 2 or nm in ("GT", "AC"):
                assert densest_window(o.nodes()) > c, (nm, c)


def ordinary_contigs():
    lens = [k * TILE + r for k in (1, 2) for r in range(1, 9)]
    rng = np.random.default_rng(77)
    lens += [int(x) for x in rng.integers(TILE // 2, 3 * TILE, size=30 - len(lens))]
    return [synthetic_contig(L, 0.30 + 0.40 * (i % 11) / 10, 8800 + i) for i, L in enumerate(lens)]


def test_ordinary_sequence_stays_on_one_pass(ctx, meta_models, monkeypatch):
    seqs = ordinary_contigs()
    assert len(seqs) == 30 and max(map(len, seqs)) <= 3 * TILE
    ctx.set_models([m.buf for m in meta_models])
    res, passes = run_with(ctx, monkeypatch, {}, seqs, meta=True)
    assert passes == 1
    n = sum(compare_contig(res, i, s, orc.Oracle(s), meta_models, meta=True) for i, s in enumerate(seqs))
    assert n > 0
    ref, _ = run_with(ctx, monkeypatch, {"PGA_EXTRACT_C": "0"}, seqs, meta=True)
    same_as(res, ref, len(seqs))


def test_pool_exhaustion_extracts_again_and_does_not_stick(ctx, tinf, meta_models, monkeypatch):
    """(GT)x1500 in one tile: 250 threads with six forward nodes each want 500 pool entries.  The batch is extracted again with a value
    for every position (two passes), with the same results; the next call of the context is back on one pass."""
    full = synthetic_contig(40, 0.5, 31) + STOPS_RC + b"GT" * 1500 + STOPS
    assert len(full) <= TILE
    seqs = [full, synthetic_contig(5000, 0.45, 32), dense_contig("GT", 33)]
    ctx.set_models([tinf[11].buf])
    ref, p0 = run_with(ctx, monkeypatch, {"PGA_EXTRACT_C": "0"}, seqs, meta=False)
    res, p1 = run_with(ctx, monkeypatch, {}, seqs, meta=False)
    assert (p0, p1) == (1, 2)
    same_as(res, ref, len(seqs))
    for i, s in enumerate(seqs):
        compare_contig(res, i, s, orc.Oracle(s), [tinf[11]], meta=False)
    assert densest_window(_nodes_of(full, tinf[11])) > C_DEFAULT
    ordinary = ordinary_contigs()[:10]
    ctx.set_models([m.buf for m in meta_models])
    after, p2 = run_with(ctx, monkeypatch, {}, ordinary, meta=True)
    assert p2 == 1
    # no pool at all and one list slot: an ordinary contig exhausts it (a thread with two nodes of a strand is enough)
    small, p3 = run_with(ctx, monkeypatch, {"PGA_EXTRACT_POOL": "0", "PGA_EXTRACT_C": "1"}, ordinary, meta=True)
    assert p3 == 2
    same_as(small, after, len(ordinary))
    for i, s in enumerate(ordinary):
        compare_contig(small, i, s, orc.Oracle(s), meta_models, meta=True)
    again, p4 = run_with(ctx, monkeypatch, {}, ordinary, meta=True)
    assert p4 == 1
    same_as(again, after, len(ordinary))


def _nodes_of(seq, model):
    o = orc.Oracle(seq)
    o.find_genes_single(model, orc.Params())
    return o.nodes()


def test_smallest_list_equals_the_default_byte_for_byte(ctx, tinf, meta_models, monkeypatch):
    dense = [dense_contig(nm, 970 + k) for k, nm in enumerate(UNITS)]
    ctx.set_models([tinf[11].buf])
    a, _ = run_with(ctx, monkeypatch, {}, dense, meta=False)
    b, _ = run_with(ctx, monkeypatch, {"PGA_EXTRACT_C": "1"}, dense, meta=False)
    same_as(b, a, len(dense))
    seqs = ordinary_contigs() + dense
    ctx.set_models([m.buf for m in meta_models])
    a, _ = run_with(ctx, monkeypatch, {}, seqs, meta=True)
    b, _ = run_with(ctx, monkeypatch, {"PGA_EXTRACT_C": "1"}, seqs, meta=True)
    same_as(b, a, len(seqs))
    for i, s in enumerate(seqs):
        compare_contig(b, i, s, orc.Oracle(s), meta_models, meta=True)
