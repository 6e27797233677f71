"""Contig sets on the device (pga_batch_set_sets) against the rule restated over the CPU oracle (tests/sets_ref.py):
the model of every set, every gene, the node arrays, the per-model scores and the summed score of the choice, as bit patterns."""
import ctypes
import io
import warnings

import numpy as np
import pytest

from tests import sets_ref as sr
from tests.test_finder_gpu import NODE_F64, NODE_INT
from tests.util import synthetic_contig

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib as L
    return L


@pytest.fixture(scope="module")
def bins():
    return sr.meta_bins()


_REF = {}


def reference(case, bins, **kw):
    """The restatement of a case, computed once and shared."""
    key = (case.__name__, tuple(sorted(kw.items())))
    if key not in _REF:
        seqs, labels = case()[:2]
        _REF[key] = (seqs, labels, sr.find_genes_sets(seqs, labels, bins, **kw))
    return _REF[key]


def b64(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def compare_member(res, i, mb, n_models):
    """Contig i of a labelled call against its Member of the restatement (the checks of test_finder_gpu.compare_contig, plus the
    choice): exact."""
    cr = res.contigs[i]
    assert cr["model"] == mb.model, i
    assert res.set_models[i] == mb.set_model, i
    assert b64(res.set_scores[i]) == b64(mb.set_score), i
    want = np.full(n_models, np.nan)
    for m, v in mb.scores.items():
        want[m] = v
    assert np.array_equal(b64(res.model_scores[i]), b64(want)), i
    og, on = mb.genes, mb.nodes
    gg = res.genes_of(i)
    assert len(gg) == len(og), i
    for k in ("begin", "end", "start_ndx", "stop_ndx"):
        assert np.array_equal(gg[k], og[k]), (i, k)
    assert np.all(gg["contig"] == i)
    if res.nodes is not None:
        nd = res.nodes[i]
        assert nd["n"] == len(on), i
        if mb.model >= 0:
            for k in NODE_INT:
                assert np.array_equal(nd[k].astype(np.int64), on[k].astype(np.int64)), (i, k)
            for k in NODE_F64:
                assert np.array_equal(nd[k].view(np.uint64), on[k].view(np.uint64)), (i, k)
            assert np.array_equal(nd["gc_cont"].view(np.uint32), on["gc_cont"].view(np.uint32))
            assert np.array_equal(nd["rbs"], on["rbs"])
    if len(gg):
        s = on[og["start_ndx"]]
        assert np.array_equal(gg["strand"], s["strand"])
        for k in ("cscore", "sscore", "rscore", "uscore", "tscore"):
            assert np.array_equal(gg[k].view(np.uint64), np.ascontiguousarray(s[k]).view(np.uint64)), (i, k)
        assert np.array_equal(gg["start_type"], np.where(s["edge"] != 0, 3, s["type"]))
    return len(gg)


def check_call(ctx, seqs, labels, want, n_models, **kw):
    res = ctx.find_genes_batch(seqs, meta=True, want_nodes=True, sets=labels, **kw)
    own_gc = [sr.gc_count(s) / len(s) if len(s) else 0.0 for s in seqs]
    assert np.array_equal(b64(res.contigs["gc"]), b64(own_gc))           # a member's gc stays its own
    return res, sum(compare_member(res, i, mb, n_models) for i, mb in enumerate(want))


# (a) ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("closed", [False, True])
def test_interleaved_sets(ctx, bins, closed):
    seqs, labels, want = reference(sr.case_interleaved, bins, closed=closed)
    ctx.set_models([m.buf for m in bins])
    res, n = check_call(ctx, seqs, labels, want, len(bins), closed=closed)
    assert n > 0
    a = [i for i, lab in enumerate(labels) if lab == "A"]
    assert len({int(res.contigs[i]["model"]) for i in a}) == 1


def test_sets_with_mask_sources(ctx, bins):
    """mask=True, a caller's region and lower-case runs combine with sets unchanged (the union masks like runs of unknown bases)."""
    seqs, labels = sr.case_interleaved()
    seqs = list(seqs)
    seqs[0] = seqs[0][:3000] + b"N" * 120 + seqs[0][3120:]
    seqs[4] = seqs[4][:1000] + b"N" * 75 + seqs[4][1075:]
    want = sr.find_genes_sets(seqs, labels, bins, mask=True, mask_size=50)
    ctx.set_models([m.buf for m in bins])
    res, n = check_call(ctx, seqs, labels, want, len(bins), mask=True)
    assert n > 0 and len(res.masks[0]) == 1 and len(res.masks[4]) == 1
    # the same runs named by the caller / written in lower case instead of found
    regions = [None] * len(seqs)
    regions[0], regions[4] = [(3000, 3120)], [(1000, 1075)]
    res2, n2 = check_call(ctx, seqs, labels, want, len(bins), regions=regions)
    soft = list(seqs)
    soft[0] = seqs[0][:3000] + b"n" * 120 + seqs[0][3120:]
    soft[4] = seqs[4][:1000] + b"n" * 75 + seqs[4][1075:]
    res3, n3 = check_call(ctx, soft, labels, want, len(bins), mask_lowercase=True)
    assert n == n2 == n3


# (b) ---------------------------------------------------------------------------------------------------------------------------------

def test_mixed_gc_set_uses_the_pooled_window(ctx, bins):
    seqs, labels, want = reference(sr.case_mixed_gc, bins)
    ctx.set_models([m.buf for m in bins])
    res, n = check_call(ctx, seqs, labels, want, len(bins))
    w = int(res.set_models[0])
    assert n > 0 and bins[w].trans_table == 4 and np.all(res.contigs["model"] == w)
    # the members alone: windows that do not hold W, another table
    alone = ctx.find_genes_batch(seqs, meta=True)
    assert w not in set(alone.contigs["model"].tolist()) and alone.set_models is None
    assert res.n_chains == sum(len(mb.window) for mb in want)


# (c) ---------------------------------------------------------------------------------------------------------------------------------

def test_set_of_300_short_members(ctx, bins):
    seqs, labels, want = reference(sr.case_many_short, bins)
    ctx.set_models([m.buf for m in bins])
    res, n = check_call(ctx, seqs, labels, want, len(bins))
    members = np.asarray([lab == "many" for lab in labels])
    assert n > 0 and np.any(res.contigs["model"][members] < 0) and np.any(res.contigs["model"][members] >= 0)
    assert len(set(res.set_models[members].tolist())) == 1


# (d) ---------------------------------------------------------------------------------------------------------------------------------

def test_sets_without_nodes_and_without_a_model(ctx, bins):
    seqs, labels, want = reference(sr.case_no_nodes, bins)
    ctx.set_models([m.buf for m in bins])
    res, n = check_call(ctx, seqs, labels, want, len(bins))
    empty = np.asarray([lab in ("empty", "nopath") for lab in labels])
    assert n > 0 and np.all(res.set_models[empty] == -1) and np.all(np.isnan(res.set_scores[empty]))
    assert np.all(res.contigs["n_genes"][empty] == 0) and np.all(np.isnan(res.model_scores[empty]))
    seqs, labels, subset = sr.case_no_model()
    models = [bins[m] for m in subset]
    want = sr.find_genes_sets(seqs, labels, models)
    ctx.set_models([m.buf for m in models])
    res, n = check_call(ctx, seqs, labels, want, len(models))
    assert res.set_models.tolist()[:2] == [-1, -1] and res.contigs["model"][2] >= 0 and n > 0


# (e) ---------------------------------------------------------------------------------------------------------------------------------

def same_records(a, b):
    assert a.contigs.tobytes() == b.contigs.tobytes()
    assert a.genes.tobytes() == b.genes.tobytes()
    assert (a.node_passes, a.n_chains) == (b.node_passes, b.n_chains)
    for x, y in zip(a.nodes, b.nodes):
        assert x["n"] == y["n"]
        assert all(np.array_equal(np.ascontiguousarray(x[k]).view(np.uint8), np.ascontiguousarray(y[k]).view(np.uint8)) for k in x if k != "n")


def test_no_labels_and_labels_of_minus_one_are_the_unlabelled_call(ctx, bins):
    seqs = sr.case_interleaved()[0] + sr.case_mixed_gc()[0] + sr.case_no_nodes()[0]
    ctx.set_models([m.buf for m in bins])
    plain = ctx.find_genes_batch(seqs, meta=True, want_nodes=True)
    none = ctx.find_genes_batch(seqs, meta=True, want_nodes=True, sets=None)
    same_records(plain, none)
    assert plain.set_models is None and none.model_scores is None
    for labels in ([None] * len(seqs), [-1] * len(seqs), list(range(100, 100 + len(seqs)))):     # on their own, one way or another
        own = ctx.find_genes_batch(seqs, meta=True, want_nodes=True, sets=labels)
        same_records(plain, own)
        assert np.array_equal(own.set_models, plain.contigs["model"])
    # labels set and cleared again on a resident batch
    b = ctx.upload(seqs).set_sets(["x"] * len(seqs))
    try:
        pooled = ctx.find_genes(b, meta=True, want_nodes=True)
        assert pooled.contigs.tobytes() != plain.contigs.tobytes()
        b.set_sets(None)
        same_records(plain, ctx.find_genes(b, meta=True, want_nodes=True))
    finally:
        b.close()


# (f) ---------------------------------------------------------------------------------------------------------------------------------

def test_translation_and_text_follow_the_model_of_the_set(ctx, lib, bins, tmp_path):
    from pyrodigal_amd.pipeline import render_fasta
    seqs, labels, want = reference(sr.case_interleaved, bins)
    ids = ["contig_%d" % i for i in range(len(seqs))]
    mbins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b.tobytes()), "bin number %d" % i) for i, b in enumerate(bins)])
    finder = lib.GeneFinder(meta=True, metagenomic_bins=mbins)
    genes = finder.find_genes_batch(seqs, sets=labels, translate=True)
    assert finder.find_genes_batch(seqs[:2])[0].set_score is None and finder.find_genes_batch(seqs[:2])[0].model_scores is None
    gff, faa = io.StringIO(), io.StringIO()
    for i, (g, mb) in enumerate(zip(genes, want)):
        assert mb.model >= 0 and g.metagenomic_bin is mbins[mb.model]
        assert g.set_score == mb.set_score and g.model_scores == mb.scores
        assert [(x.begin, x.end) for x in g] == [(int(b), int(e)) for b, e in zip(mb.genes["begin"], mb.genes["end"])]
        tt = bins[mb.model].trans_table
        for x in g:
            assert x.translate() == x.translate(translation_table=tt)     # the device's proteins: W's table
        g.write_gff(gff, ids[i])
        g.write_translations(faa, ids[i])
    a = [i for i, lab in enumerate(labels) if lab == "A"]
    w = want[a[0]].model
    assert bins[w].trans_table == 4                                       # (so a wrong table would show: TGA reads W)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                   # (another table than the genes were called with: that is the point)
        assert any(x.translate() != x.translate(translation_table=11) for i in a for x in genes[i])
    path = tmp_path / "sets.fa"
    with open(path, "wb") as f:
        for sid, s in zip(ids, seqs):
            f.write(b">" + sid.encode() + b" some description\n" + s + b"\n")
    out_gff, out_faa = io.BytesIO(), io.BytesIO()
    by_id = {sid: lab for sid, lab in zip(ids, labels) if lab is not None}
    stats = render_fasta(str(path), [b.tobytes() for b in bins], gff=out_gff, faa=out_faa, meta=True,
                         descriptions=[b.description for b in mbins], sets_by_id=by_id, n_contexts=1)
    assert stats["records"] == len(seqs) and stats["sets_unmatched"] == [] and stats["device_calls"] == 1
    assert out_gff.getvalue() == gff.getvalue().encode()
    assert out_faa.getvalue() == faa.getvalue().encode()
    text = out_gff.getvalue().decode()
    for i in a:
        assert ('seqhdr="%s"\n# Model Data: version=pyrodigal_amd.v%s;run_type=Metagenomic;model="bin number %d";gc_cont=%.2f;transl_table=4;'
                % (ids[i], __import__("pyrodigal_amd").__version__, w, bins[w].gc * 100)) in text


# (g) ---------------------------------------------------------------------------------------------------------------------------------

def test_getters_on_sparse_labels_and_a_replicated_batch(ctx, bins):
    """pga_set_choice / pga_model_scores through the C-ABI with labels that are neither dense nor in order, against the sums of the
    restatement: the same doubles added in the same order."""
    seqs, labels, want = reference(sr.case_interleaved, bins)
    raw = np.asarray([{"A": 1000000, "B": 7, None: -1}[lab] for lab in labels], np.int32)
    ctx.set_models([m.buf for m in bins])
    n, nm = len(seqs), len(bins)
    b = ctx.upload(seqs)
    try:
        assert ctx.L.pga_batch_set_sets(b.h, ctypes.c_void_p(raw.ctypes.data)) == 0
        b.sets = raw
        res = ctx.find_genes(b, meta=True)
        model, score = np.zeros(n, np.int32), np.zeros(n, np.float64)
        ms = np.zeros((n, nm), np.float64)
        assert ctx.L.pga_set_choice(ctx.h, n, ctypes.c_void_p(model.ctypes.data), ctypes.c_void_p(score.ctypes.data)) == 0
        assert ctx.L.pga_model_scores(ctx.h, n, nm, ctypes.c_void_p(ms.ctypes.data)) == 0
        for i, mb in enumerate(want):
            assert model[i] == mb.set_model and b64(score[i]) == b64(mb.set_score)
            assert b64(score[i]) == b64(mb.set_sums[mb.set_model])
            for m in range(nm):
                assert b64(ms[i, m]) == b64(mb.scores.get(m, np.nan)), (i, m)
            # S_W from the device's own per-contig numbers, left to right in batch order
            acc = None
            for j, other in enumerate(want):
                if other.set == mb.set and not np.isnan(ms[j, mb.set_model]):
                    acc = ms[j, mb.set_model] if acc is None else acc + ms[j, mb.set_model]
            assert b64(acc) == b64(score[i])
        # a wider request than the call: NaN / -1 beyond it
        wide = np.zeros((n + 2, nm + 1), np.float64)
        assert ctx.L.pga_model_scores(ctx.h, n + 2, nm + 1, ctypes.c_void_p(wide.ctypes.data)) == 0
        assert np.all(np.isnan(wide[n:])) and np.all(np.isnan(wide[:, nm])) and np.array_equal(b64(wide[:n, :nm]), b64(ms))
        # the labels travel with a replicated batch: the members of A alone, in another order
        a = [i for i, lab in enumerate(labels) if lab == "A"]
        rep = ctx.replicate(b, a[::-1])
        try:
            r2 = ctx.find_genes(rep, meta=True)
        finally:
            rep.close()
        assert r2.set_models.tolist() == [want[a[0]].set_model] * len(a)
        for k, i in enumerate(a[::-1]):
            x, y = r2.genes_of(k), res.genes_of(i)
            assert all(np.array_equal(x[f], y[f]) for f in ("begin", "end", "strand", "start_ndx", "stop_ndx"))
        # a call without labels forgets the choice
        b.set_sets(None)
        ctx.find_genes(b, meta=True)
        assert ctx.L.pga_set_choice(ctx.h, n, ctypes.c_void_p(model.ctypes.data), ctypes.c_void_p(score.ctypes.data)) == 0
        assert np.all(model == -1) and np.all(np.isnan(score))
    finally:
        b.close()


# (h) ---------------------------------------------------------------------------------------------------------------------------------

def test_refusals(ctx, lib, bins):
    seqs = [synthetic_contig(2500, 0.5, 4601), synthetic_contig(2100, 0.45, 4602)]
    ctx.set_models([m.buf for m in bins])
    with pytest.raises(ValueError, match="pga_batch_set_sets.*pga_batch_set_circular"):
        ctx.find_genes_batch(seqs, meta=True, sets=["a", "a"], circular=[True, False])
    with pytest.raises(ValueError, match="meta"):
        ctx.find_genes_batch(seqs, meta=False, sets=["a", "a"])
    with pytest.raises(ValueError, match="3 entries for 2"):
        ctx.find_genes_batch(seqs, meta=True, sets=["a", "a", "a"])
    b = ctx.upload(seqs)
    try:
        bad = np.asarray([0, -2], np.int32)
        assert ctx.L.pga_batch_set_sets(b.h, ctypes.c_void_p(bad.ctypes.data)) == -1
        b.set_sets(["a", "a"]).set_circular(True)
        with pytest.raises(ValueError, match="circular"):
            ctx.find_genes(b, meta=False, model_of_contig=[0, 0])
        b.set_circular(None)
        ok = ctx.find_genes(b, meta=True)                               # the context and the batch go on working
        assert ok.set_models[0] == ok.set_models[1] >= 0
    finally:
        b.close()
    mbins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=m.tobytes()), "bin %d" % i) for i, m in enumerate(bins)])
    finder = lib.GeneFinder(meta=True, metagenomic_bins=mbins)
    with pytest.raises(ValueError, match="circular"):
        finder.find_genes_batch(seqs, sets=["a", "a"], circular=True)
    with pytest.raises(ValueError, match="1 entries for 2"):
        finder.find_genes_batch(seqs, sets=["a"])
    got = finder.find_genes_batch(seqs, sets=[("bin", 1), ("bin", 1)])    # any hashable
    assert got[0].metagenomic_bin is got[1].metagenomic_bin and got[0].set_score == got[1].set_score
    assert finder.find_genes(seqs[0]).set_score is None                  # find_genes is unchanged
