"""Every start node the start scorer scores (k_score_starts with a thread per node and with a thread per listed start; k_start_prologue +
k_score_starts_mm, the model-major form; pyrodigal_amd/csrc/pipeline.hip) against the CPU oracle, every node field as a bit pattern:
at every distance from the upstream end of a contig at which a window shortens, at the ORF and contig lengths the scores switch on,
on either side of the 500 nodes the scan for a shared edge node covers, and across the tile cuts of the model-major order.
tests/start_shapes.py builds the inputs; tests/test_start_score_cpu.py shows with the oracle alone that they hold what they are meant
to hold.  The run-time knobs choose between the forms; only values the code accepts are set."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import start_shapes as ss
from tests.test_finder_gpu import compare_contig
from tests.test_stages_gpu import check, oracle_stage

pytestmark = pytest.mark.gpu

KNOBS = ("PGA_SS_MM", "PGA_SS_MM_TILE", "PGA_SS_STARTS_ONLY", "PGA_SS_MODELS_PER_PASS", "PGA_SS_FULL_STOPS")
VARIANTS = {
    "default": {},                                                    # prologue + model-major items in tiles of 1024
    "tile256": {"PGA_SS_MM_TILE": "256"},
    "tile512": {"PGA_SS_MM_TILE": "512"},
    "loop": {"PGA_SS_MM": "0"},                                       # the model loop with a thread per listed start
    "pernode": {"PGA_SS_STARTS_ONLY": "0"},                           # the model loop with a thread per node
    "loop1": {"PGA_SS_MODELS_PER_PASS": "1", "PGA_SS_MM": "0"},       # ... one model per pass over the workgroup's model set
    "fullstops": {"PGA_SS_FULL_STOPS": "1"},                          # the stop nodes' zeros written in full
}
SERIES = ("end", "orf", "scan", "tile")


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def models():
    return ss.base_models()


@pytest.fixture(scope="module")
def listed(models):
    lm = ss.listed_models(models)
    assert len(lm) >= 3 and {m.trans_table for m in lm} == {4, 11} and {m.uses_sd for m in lm} == {0, 1}
    return lm


@pytest.fixture
def knobs(monkeypatch):
    """Sets the knobs of a variant (the library reads them at every call); all of them are gone again after the test."""
    def use(variant):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in VARIANTS[variant].items():
            monkeypatch.setenv(k, v)
    yield use
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


_INPUT, _REF = {}, {}


def batch(name):
    if not _INPUT:
        _INPUT["end"] = [s for *_, s in ss.end_series()]
        _INPUT["orf"] = [s for *_, s in ss.orf_series()]
        _INPUT["scan"] = [s for *_, s in ss.scan_series()]
        _INPUT["tile"] = ss.tile_series()
    return _INPUT[name]


def staged_reference(name, i, stage, tinf, model, closed, is_meta, **kw):
    """The oracle's nodes of contig i of a batch after a stage, computed once and shared (never written to)."""
    key = ("stage", name, i, stage, model, closed, is_meta, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = oracle_stage(batch(name)[i], stage, tinf=tinf, closed=closed, is_meta=is_meta, **kw)
        _REF[key].setflags(write=False)
    return _REF[key]


class Called:
    """The oracle's call of one contig, kept: what compare_contig of tests/test_finder_gpu.py asks an Oracle for."""

    def __init__(self, seq, models, meta, closed):
        o = orc.Oracle(seq)
        p = orc.Params(closed=closed)
        self.phase = o.find_genes_meta(models, p) if meta else o.find_genes_single(models[0], p)
        self._genes, self._nodes = o.genes(), o.nodes()
        self._genes.setflags(write=False)
        self._nodes.setflags(write=False)

    def find_genes_meta(self, models, params):
        return self.phase

    def find_genes_single(self, tinf, params):
        return self.phase

    def genes(self):
        return self._genes

    def nodes(self):
        return self._nodes


def called_reference(name, i, lm, model, closed):
    """model: the loaded model contig i is called with (single mode), or None: meta mode over all of them."""
    key = ("call", name, i, model, closed)
    if key not in _REF:
        _REF[key] = Called(batch(name)[i], lm if model is None else [lm[model]], model is None, closed)
    return _REF[key]


# ---- 1. a thread per node, one model ------------------------------------------------------------------------------------------------------

def run_per_node(ctx, models, model, closed, is_meta, stage=2, names=SERIES, order=1):
    tinf = models[model]
    ctx.set_models([tinf.tobytes()])
    seqs = [(n, i) for n in names for i in range(len(batch(n)))][::order]
    out = ctx.nodes_stage([batch(n)[i] for n, i in seqs], stage, closed=closed, is_meta=is_meta)
    starts = 0
    for (n, i), nd in zip(seqs, out):
        on = staged_reference(n, i, stage, tinf, model, closed, is_meta)
        check(nd, on, stage)
        starts += int(np.count_nonzero(on["type"] != 3))
    assert starts > 10000


@pytest.mark.parametrize("is_meta", [False, True])
@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("model", ss.MODEL_NAMES)
def test_thread_per_node(ctx, models, model, closed, is_meta):
    run_per_node(ctx, models, model, closed, is_meta)
    # the ORF series again with the shortest listed ORF exactly at the minimum gene length
    tinf, g = models[model], {"min_gene": ss.ORF_MIN_GENE, "min_edge_gene": ss.ORF_MIN_EDGE_GENE}
    out = ctx.nodes_stage(batch("orf"), 2, closed=closed, is_meta=is_meta, **g)
    for i, nd in enumerate(out):
        check(nd, staged_reference("orf", i, 2, tinf, model, closed, is_meta, **g), 2)


def test_thread_per_node_with_overlapping_starts(ctx, models):
    run_per_node(ctx, models, "sd", False, False, stage=3)


# ---- 2. the listed launches, several models ------------------------------------------------------------------------------------------------

def run_listed(ctx, lm, name, meta, closed=False, order=1, want_nodes=True):
    """One call on a batch; every contig against the oracle: under its own model (single mode, a model per contig) or the winner and the
    winner's nodes (meta mode)."""
    seqs = batch(name)
    idx = list(range(len(seqs)))[::order]
    moc = ss.model_of_contig(len(seqs))
    if meta:
        res = ctx.find_genes_batch([seqs[i] for i in idx], meta=True, closed=closed, want_nodes=want_nodes)
    else:
        res = ctx.find_genes_batch([seqs[i] for i in idx], meta=False, closed=closed, want_nodes=want_nodes, model_of_contig=[moc[i] for i in idx])
    genes = 0
    for k, i in enumerate(idx):
        o = called_reference(name, i, lm, None if meta else moc[i], closed)
        genes += compare_contig(res, k, seqs[i], o, lm if meta else [lm[moc[i]]], meta=meta, closed=closed)
    return genes


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_listed_a_model_per_contig(ctx, listed, knobs, variant):
    ctx.set_models([m.buf for m in listed])
    knobs(variant)
    assert sum(run_listed(ctx, listed, name, meta=False) for name in SERIES) > 300


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("closed", [False, True])
def test_listed_meta_mode(ctx, listed, knobs, closed, variant):
    ctx.set_models([m.buf for m in listed])
    knobs(variant)
    assert sum(run_listed(ctx, listed, name, meta=True, closed=closed) for name in SERIES) > 300
    if variant in ("default", "fullstops"):         # without node arrays the stop nodes' zero scores may stay unwritten: the genes
        assert run_listed(ctx, listed, "tile", meta=True, closed=closed, want_nodes=False) > 0


# ---- 3. batch order -----------------------------------------------------------------------------------------------------------------------

def test_batch_order_thread_per_node(ctx, models):
    """The contig at the head of a workgroup (its edge candidates in LDS with those of the next three) and the contigs behind the fourth
    (read from global memory) change roles when the batch is reversed."""
    for order in (1, -1):
        run_per_node(ctx, models, "sd", False, False, names=("end", "tile"), order=order)


@pytest.mark.parametrize("variant", ["default", "loop"])
def test_batch_order_listed(ctx, listed, knobs, variant):
    ctx.set_models([m.buf for m in listed])
    knobs(variant)
    for name in ("end", "tile"):
        assert run_listed(ctx, listed, name, meta=False, order=-1) > 0
        assert run_listed(ctx, listed, name, meta=True, order=-1) > 0
