"""Single mode with a model per contig (pga_find_genes_models, GeneFinder.find_genes_batch(..., training_infos=...)): many
genomes, each under its own trained model, in one device call -- every contig's result is identical, field for field, to a
single-model call with that one model loaded, and to the CPU oracle."""
import gzip
import io
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests.util import golden_path, read_fasta

pytestmark = pytest.mark.gpu

NODE_INT = ["ndx", "stop_val", "type", "strand", "edge", "traceb", "tracef", "ov_mark", "elim", "mot_ndx", "mot_len", "mot_spacer",
            "mot_spacendx"]
NODE_F64 = ["cscore", "sscore", "rscore", "uscore", "tscore", "score", "mot_score"]


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def genomes(ctx):
    """(name, sequence, trained model blob): two SD genomes, a motif-model genome, a table-4 genome and two planted ones."""
    from pyrodigal_amd import benchdata
    out = []
    for name, tt in (("SRR492066", 11), ("KK037166", 11), ("MIIJ01000039", 4)):
        seq = read_fasta(name + ".fna.gz")[0][1]
        out.append((name, seq, ctx.train(seq, translation_table=tt), tt))
    for k, gc in enumerate((0.33, 0.66)):
        seq = benchdata.planted_contig(150_000, gc, 900 + k).decode()
        out.append(("planted%d" % k, seq, ctx.train(seq), 11))
    return out


def _same_genes(a, b, skip=()):
    """Gene records field by field, bit patterns (the records have padding bytes that nobody writes)."""
    assert len(a) == len(b)
    for k in a.dtype.names:
        if k in skip:
            continue
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.tobytes() == y.tobytes(), k


def _same_contig(got, i, want, j):
    """Contig i of `got` and contig j of `want`: gene records (but their batch index), node arrays, score."""
    _same_genes(got.genes_of(i), want.genes_of(j), skip=("contig",))
    assert got.contigs[i]["score"].tobytes() == want.contigs[j]["score"].tobytes()
    assert got.contigs[i]["n_nodes"] == want.contigs[j]["n_nodes"]
    if got.nodes is not None:
        for k, v in got.nodes[i].items():
            assert np.array_equal(np.asarray(v), np.asarray(want.nodes[j][k])), (i, k)


def _against_oracle(res, i, seq, blob, closed=False):
    o = orc.Oracle(seq)
    o.find_genes_single(orc.Training(blob), orc.Params(closed=closed))
    og, on, gg = o.genes(), o.nodes(), res.genes_of(i)
    assert len(gg) == len(og)
    for k in ("begin", "end", "start_ndx", "stop_ndx"):
        assert np.array_equal(gg[k], og[k]), k
    nd = res.nodes[i]
    assert nd["n"] == len(on)
    for k in NODE_INT:
        assert np.array_equal(nd[k].astype(np.int64), on[k].astype(np.int64)), k
    for k in NODE_F64:
        assert np.array_equal(nd[k].view(np.uint64), on[k].view(np.uint64)), k
    assert np.array_equal(nd["star_ptr"], on["star_ptr"])


@pytest.mark.parametrize("closed", [False, True])
def test_interleaved_genomes_each_under_its_own_model(ctx, genomes, closed):
    contigs, moc = [], []
    for part in range(3):                       # the contigs of every genome, interleaved with those of the others
        for m, (_, seq, _, _) in enumerate(genomes):
            n = len(seq)
            lo, hi = [(0, n // 3), (n // 3, n // 2), (n // 2, n)][part]
            contigs.append(seq[lo:hi])
            moc.append(m)
    ctx.set_models([g[2] for g in genomes])
    got = ctx.find_genes_batch(contigs, meta=False, closed=closed, want_nodes=True, model_of_contig=moc)
    assert list(got.contigs["model"]) == moc
    assert got.n_chains == len(contigs)
    for m, (_, _, blob, _) in enumerate(genomes):
        ctx.set_models([blob])
        mine = [i for i, x in enumerate(moc) if x == m]
        want = ctx.find_genes_batch([contigs[i] for i in mine], meta=False, closed=closed, want_nodes=True)
        for j, i in enumerate(mine):
            _same_contig(got, i, want, j)
            if not closed and j == 0:
                _against_oracle(got, i, contigs[i], blob)


def test_all_zeros_is_the_plain_single_mode_call(ctx, genomes):
    seqs = [g[1] for g in genomes[:3]]
    ctx.set_models([genomes[0][2], genomes[2][2]])
    want = ctx.find_genes_batch(seqs, meta=False, want_nodes=True)
    got = ctx.find_genes_batch(seqs, meta=False, want_nodes=True, model_of_contig=[0, 0, 0])
    _same_genes(got.genes, want.genes)
    _same_genes(got.contigs, want.contigs)
    for i in range(len(seqs)):
        _same_contig(got, i, want, i)


def test_more_models_than_one_start_scoring_pass_holds(ctx, genomes):
    """600 loaded models (k_score_starts walks 512 per pass; a group of 400 models is past the LDS form of the coding score):
    every contig on a model of its own, many of them above 512."""
    from pyrodigal_amd import benchdata
    blobs = [genomes[k % 3][2] for k in range(600)]            # tables 11, 11, 4: two groups of 400 and 200 models
    contigs = [benchdata.planted_contig(20_000 + 1000 * i, 0.3 + 0.4 * (i % 7) / 6, 1200 + i).decode() for i in range(40)]
    moc = [(15 * i + 7) % 600 if i % 3 else 599 - i for i in range(40)]
    assert len(set(moc)) == 40 and sum(m >= 512 for m in moc) >= 5
    ctx.set_models(blobs)
    got = ctx.find_genes_batch(contigs, meta=False, want_nodes=True, model_of_contig=moc)
    assert list(got.contigs["model"]) == moc
    for k in range(3):
        ctx.set_models([genomes[k][2]])
        want = ctx.find_genes_batch(contigs, meta=False, want_nodes=True)
        for i in range(40):
            if moc[i] % 3 == k:
                _same_contig(got, i, want, i)


def test_bad_arguments_are_rejected(ctx, genomes):
    ctx.set_models([genomes[0][2], genomes[1][2]])
    seqs = [genomes[0][1][:30000], genomes[1][1][:30000]]
    for moc in ([0, 2], [-1, 0]):
        with pytest.raises(ValueError, match="names model"):
            ctx.find_genes_batch(seqs, meta=False, model_of_contig=moc)
    with pytest.raises(ValueError, match="meta"):
        ctx.find_genes_batch(seqs, meta=True, model_of_contig=[0, 1])
    with pytest.raises(ValueError, match="2 contigs"):
        ctx.find_genes_batch(seqs, meta=False, model_of_contig=[0])
    # the context is still good
    assert len(ctx.find_genes_batch(seqs, meta=False, model_of_contig=[1, 0]).genes) > 0


def _lib():
    try:
        from pyrodigal_amd import lib
    except ImportError:
        import __graft_entry__
        __graft_entry__.build_cython_host()
        from pyrodigal_amd import lib
    return lib


def test_two_genomes_in_one_call_reproduce_the_reference_proteins():
    """SRR492066 (Shine-Dalgarno) and KK037166 (motif model) in one translated call: the reference's `*.single.faa` files
    byte for byte (the second sequence of a finder's call is its sequence 2: its gene IDs read 2_k where the file, written
    from a finder of its own, reads 1_k)."""
    lib = _lib()
    recs = [read_fasta(n + ".fna.gz")[0] for n in ("SRR492066", "KK037166")]
    tinfs = [lib.TrainingInfo(raw=orc.Oracle(seq).train().tobytes()) for _, seq in recs]
    finder = lib.GeneFinder()
    out = finder.find_genes_batch([seq for _, seq in recs], translate=True, training_infos=tinfs)
    assert finder.training_info is None
    for k, (name, (hdr, _)) in enumerate(zip(("SRR492066", "KK037166"), recs)):
        assert out[k].training_info is tinfs[k]
        buf = io.StringIO()
        out[k].write_translations(buf, hdr.split()[0])
        text = buf.getvalue().replace("ID=%d_" % (k + 1), "ID=1_")
        assert text == gzip.open(golden_path(name + ".single.faa.gz"), "rt").read()


def _normalise(text):
    return re.sub(r"seqnum=\d+", "seqnum=N", re.sub(r"ID=\d+_", "ID=N_", text))


def test_find_genes_batch_with_training_infos_equals_a_finder_per_genome(genomes):
    lib = _lib()
    tinfs = [lib.TrainingInfo(raw=np.frombuffer(g[2], np.uint8).copy()) for g in genomes]
    seqs, ts = [], []
    for rep in range(2):
        for k in (4, 2, 0, 3, 1):
            seqs.append(genomes[k][1][rep * 20000:])
            ts.append(tinfs[k])                                      # the same object twice: loaded once
    for kw in ({}, {"closed": True}):
        finder = lib.GeneFinder(**kw)
        got = finder.find_genes_batch(seqs, training_infos=ts)
        tiny = lib.GeneFinder(coalesce_bases=1, **kw).find_genes_batch(seqs, translate=True, training_infos=ts)
        for i, s in enumerate(seqs):
            want = lib.GeneFinder(ts[i], **kw).find_genes(s)
            for g in (got[i], tiny[i]):
                assert g.training_info is ts[i]
                assert [(x.begin, x.end, x.strand, x.start_type, x.rbs_motif, x.score) for x in g] == \
                       [(x.begin, x.end, x.strand, x.start_type, x.rbs_motif, x.score) for x in want]
                for writer in ("write_gff", "write_translations"):
                    a, b = io.StringIO(), io.StringIO()
                    getattr(g, writer)(a, "seq%d" % i)
                    getattr(want, writer)(b, "seq%d" % i)
                    assert _normalise(a.getvalue()) == _normalise(b.getvalue()), (i, writer)


def test_ordinary_calls_keep_the_finders_model_after_a_per_genome_call(genomes):
    lib = _lib()
    t0 = lib.TrainingInfo(raw=np.frombuffer(genomes[0][2], np.uint8).copy())
    t2 = lib.TrainingInfo(raw=np.frombuffer(genomes[2][2], np.uint8).copy())
    finder = lib.GeneFinder(t0, contexts=1)
    seq = genomes[1][1]
    before = [(g.begin, g.end, g.strand) for g in finder.find_genes(seq)]
    other = finder.find_genes_batch([seq], training_infos=[t2])[0]
    assert other.training_info is t2
    after = finder.find_genes(seq)
    assert after.training_info is t0
    assert [(g.begin, g.end, g.strand) for g in after] == before
    assert [(g.begin, g.end, g.strand) for g in other] != before
