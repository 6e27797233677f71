"""The listed start scoring in two kernels (k_start_prologue + k_score_starts_mm, model-major items) against the model loop of
k_score_starts (PGA_SS_MM=0): gene records, contig scores and every node field of the returned chains, as bit patterns."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.util import golden_path, read_fasta, synthetic_contig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def models():
    """SD and non-SD models, two translation tables."""
    m = [orc.Training.load(golden_path("SRR492066.training.bin.gz")),
         orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic.tinf_closed.bin.gz"))]
    kk = orc.Oracle(read_fasta("KK037166.fna.gz")[0][1]).train()
    assert kk.uses_sd == 0
    m.append(kk)
    for src, gc, tt in [(0, 0.36, 11), (2, 0.47, 11), (2, 0.60, 4), (1, 0.42, 4), (0, 0.33, 4), (2, 0.66, 11), (1, 0.55, 11)]:
        t = m[src].copy(); t.set_gc(gc); t.set_trans_table(tt); m.append(t)
    assert {t.uses_sd for t in m} == {0, 1}
    return m


def _contigs():
    from pyrodigal_amd import benchdata
    rng = np.random.default_rng(77)
    out = []
    # many short contigs: tiles of 256 items span more than four of them; every meta penalty below 1 500 and 3 000 bases
    for k in range(120):
        out.append(synthetic_contig(int(rng.integers(120, 1500)), 0.3 + 0.4 * rng.random(), 41_000 + k))
    for k in range(30):
        out.append(synthetic_contig(int(rng.integers(1500, 3000)), 0.3 + 0.4 * rng.random(), 42_000 + k))
    # contigs without start nodes (stop codons on both strands and no start codon), and empty ones
    out += [b"TAATAA" * 60, b"", b"N" * 500, b"ATGAAATAA"]
    # start nodes at the contig edges (converted to edge nodes by the first model of a run, or by a later one)
    for k in range(12):
        s = synthetic_contig(int(rng.integers(2000, 9000)), 0.35 + 0.03 * k, 43_000 + k)
        out.append(b"ATG" + s[3:-3] + b"CAT" if k % 2 else b"GTG" + s[3:])
    for k in range(10):                  # (planted genes: plenty of calls to compare)
        out.append(benchdata.planted_contig(int(rng.integers(9000, 40000)), 0.3 + 0.04 * k, 44_000 + k))
    return out


def _same(a, b):
    assert a.genes.tobytes() == b.genes.tobytes()
    assert np.array_equal(a.contigs["model"], b.contigs["model"])
    assert a.contigs["score"].tobytes() == b.contigs["score"].tobytes()
    if a.nodes is None:
        assert b.nodes is None
        return
    for x, y in zip(a.nodes, b.nodes):
        assert x.keys() == y.keys()
        for k, v in x.items():
            v, w = np.asarray(v), np.asarray(y[k])
            if v.dtype.kind == "f":
                assert np.array_equal(v.view(np.uint8), w.view(np.uint8)), k
            else:
                assert np.array_equal(v, w), k


def _both(ctx, monkeypatch, *args, **kw):
    monkeypatch.delenv("PGA_SS_MM", raising=False)
    new = ctx.find_genes_batch(*args, **kw)
    monkeypatch.setenv("PGA_SS_MM", "0")
    old = ctx.find_genes_batch(*args, **kw)
    monkeypatch.delenv("PGA_SS_MM")
    return new, old


@pytest.mark.parametrize("closed", [False, True])
def test_meta_mode_both_tables(ctx, models, closed, monkeypatch):
    seqs = _contigs()
    ctx.set_models([m.buf for m in models])
    for want_nodes in (True, False):
        new, old = _both(ctx, monkeypatch, seqs, meta=True, closed=closed, want_nodes=want_nodes)
        _same(new, old)
        assert len(new.genes) > 50
    # a sample against the oracle
    for i in range(0, len(seqs), 23):
        o = orc.Oracle(seqs[i])
        assert o.find_genes_meta(models, orc.Params(closed=closed)) == new.contigs[i]["model"]


def test_single_mode(ctx, models, monkeypatch):
    # (one model loaded: both settings run the model loop; the switch must not change that path either)
    seqs = _contigs()
    for k in (0, 2):                     # an SD and a non-SD model
        ctx.set_models([models[k].buf])
        new, old = _both(ctx, monkeypatch, seqs, meta=False, want_nodes=True)
        _same(new, old)
        assert len(new.genes) > 50


def test_a_model_per_contig(ctx, models, monkeypatch):
    # every model scores some contigs; its node fields come back for each of them
    seqs = _contigs()
    ctx.set_models([m.buf for m in models if m.trans_table == 11])
    n = sum(1 for m in models if m.trans_table == 11)
    moc = [i % n for i in range(len(seqs))]
    new, old = _both(ctx, monkeypatch, seqs, meta=False, want_nodes=True, model_of_contig=moc)
    _same(new, old)
    assert len(new.genes) > 50
