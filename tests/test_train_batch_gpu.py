"""Training many genomes in one call (pga_train_batch, Context.train_batch, GeneFinder.train_batch): every genome's
TrainingInfo is byte-identical to the reference's fixtures, to the oracle at every intermediate stage, and to a training of
that genome alone."""
import gzip
import random

import numpy as np
import pytest

from oracle import oracle as orc
from tests.util import golden_path, read_fasta

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


def _seq(name):
    return read_fasta(name + ".fna.gz")[0][1]


def test_fixtures_in_one_batch(ctx):
    full, part = _seq("GCF_001457455.1_NCTC11397_genomic"), _seq("GCF_001457455.1_NCTC11397_genomic_100kb")
    got = ctx.train_batch([full, part], closed=True)
    assert got[0] == gzip.open(golden_path("GCF_001457455.1_NCTC11397_genomic.tinf_closed.bin.gz")).read()
    assert got[1] == gzip.open(golden_path("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz")).read()
    got = ctx.train_batch([_seq("KK037166"), _seq("SRR492066"), _seq("MIIJ01000039")], translation_table=[11, 11, 4])
    assert got[1] == gzip.open(golden_path("SRR492066.training.bin.gz")).read()


def _mixed():
    srr = _seq("SRR492066")
    with_n = srr[:60000] + "N" * 400 + srr[60000:120000] + "N" * 80 + srr[120000:]
    # (sequence, tt, start_weight, force_nonsd)
    return [(srr, 11, 4.35, False), (_seq("KK037166"), 11, 4.35, False), (srr, 11, 4.35, True), (_seq("MIIJ01000039"), 4, 4.35, False),
            (srr, 11, 3.0, False), (with_n, 11, 4.35, False)]


@pytest.mark.parametrize("upto", [1, 2, 3, 0])
def test_mixed_batch_stages_match_the_oracle(ctx, upto):
    batch = _mixed()
    got = ctx.train_batch([b[0] for b in batch], translation_table=[b[1] for b in batch], start_weight=[b[2] for b in batch],
                          force_nonsd=[b[3] for b in batch], upto=upto)
    for g, (seq, tt, sw, fn) in enumerate(batch):
        want = orc.Oracle(seq).train(orc.Params(), force_nonsd=fn, start_weight=sw, tt=tt, upto=upto).tobytes()
        assert got[g] == want, g


def test_mixed_batch_with_masking_matches_the_oracle(ctx):
    batch = _mixed()
    got = ctx.train_batch([b[0] for b in batch], translation_table=[b[1] for b in batch], start_weight=[b[2] for b in batch],
                          force_nonsd=[b[3] for b in batch], mask=True)
    for g, (seq, tt, sw, fn) in enumerate(batch):
        assert got[g] == orc.Oracle(seq, mask=True).train(orc.Params(), force_nonsd=fn, start_weight=sw, tt=tt).tobytes(), g


def _lib():
    try:
        from pyrodigal_amd import lib
    except ImportError:
        import __graft_entry__
        __graft_entry__.build_cython_host()
        from pyrodigal_amd import lib
    return lib


@pytest.fixture(scope="module")
def genomes():
    """About 24 genomes in shuffled order: planted ones at 60-400 kbp over GC 0.30-0.70 (mostly motif models), the fixtures, some
    given as 2-3 contigs."""
    from pyrodigal_amd import benchdata
    rng = random.Random(11)
    out = []
    for k in range(20):
        s = benchdata.planted_contig(rng.randrange(60_000, 400_000), 0.30 + 0.40 * k / 19, 3000 + k).decode()
        if k % 4 == 1:
            out.append([s[:len(s) // 2], s[len(s) // 2:]])
        elif k % 4 == 2:
            out.append((s[:len(s) // 3], s[len(s) // 3:2 * len(s) // 3], s[2 * len(s) // 3:]))
        else:
            out.append(s)
    out += [_seq("SRR492066"), _seq("KK037166"), [_seq("GCF_001457455.1_NCTC11397_genomic_100kb")[:50000],
            _seq("GCF_001457455.1_NCTC11397_genomic_100kb")[50000:]], _seq("MIIJ01000039")]
    rng.shuffle(out)
    return out


def _train_one(lib, g, **kw):
    return lib.GeneFinder().train(*g, **kw) if isinstance(g, (list, tuple)) else lib.GeneFinder().train(g, **kw)


def test_the_batch_equals_the_loop(genomes):
    lib = _lib()
    want = [_train_one(lib, g).raw.tobytes() for g in genomes]
    finder = lib.GeneFinder()
    got = finder.train_batch(genomes)
    assert finder.training_info is None
    assert [t.raw.tobytes() for t in got] == want
    perm = list(range(len(genomes)))
    random.Random(5).shuffle(perm)
    assert [t.raw.tobytes() for t in lib.GeneFinder().train_batch([genomes[k] for k in perm])] == [want[k] for k in perm]
    # a tiny budget: one device call per genome
    assert [t.raw.tobytes() for t in lib.GeneFinder(coalesce_bases=1).train_batch(genomes)] == want
    # per-genome options
    tts = [4 if k % 5 == 0 else 11 for k in range(len(genomes))]
    fns = [k % 3 == 0 for k in range(len(genomes))]
    got = lib.GeneFinder().train_batch(genomes, translation_table=tts, force_nonsd=fns, start_weight=3.5)
    for k in (0, 1, 3, 5):
        assert got[k].raw.tobytes() == _train_one(lib, genomes[k], translation_table=tts[k], force_nonsd=fns[k], start_weight=3.5).raw.tobytes()


def test_a_batch_of_one_is_pga_train(ctx):
    seq = _seq("KK037166")
    assert ctx.train_batch([seq]) == [ctx.train(seq)]


def test_a_genome_without_nodes_is_named_and_the_others_are_still_trained(ctx):
    import ctypes
    from pyrodigal_amd import _cabi
    # (with closed ends a genome of only N has no node at all; with open ends it has its twelve edge nodes, and trains)
    seqs = [_seq("SRR492066"), "N" * 30000, _seq("KK037166")]
    with pytest.raises(ValueError, match="genome 1"):
        ctx.train_batch(seqs, closed=True)
    # at the C level: status per genome, the others' results as trained alone
    b = _cabi.Batch(ctx, seqs)
    try:
        p = _cabi.Params(1, 90, 60, 60, 0, 0, 0, 50)
        out = np.zeros(3 * _cabi.TRAINING_SIZE, np.uint8)
        status = np.zeros(3, np.int32)
        tt = np.full(3, 11, np.int32); sw = np.full(3, 4.35); fn = np.zeros(3, np.int32)
        rc = ctx.L.pga_train_batch(ctx.h, b.h, ctypes.byref(p), tt.ctypes.data, sw.ctypes.data, fn.ctypes.data, 0, out.ctypes.data,
                                   status.ctypes.data)
    finally:
        b.close()
    assert rc == 0 and list(status) == [0, _cabi.PGA_EINVAL, 0]
    assert out[:_cabi.TRAINING_SIZE].tobytes() == ctx.train(seqs[0], closed=True)
    assert out[2 * _cabi.TRAINING_SIZE:].tobytes() == ctx.train(seqs[2], closed=True)
    with pytest.raises(ValueError, match="no start / stop node"):
        ctx.train(seqs[1], closed=True)


def test_train_batch_leaves_the_loaded_model_set_in_place():
    from pyrodigal_amd import _cabi, benchdata
    models = [m[1] for m in benchdata.load_model_set()]
    seqs = [benchdata.synthetic_contig(30000, gc, 40 + i) for i, gc in enumerate((0.4, 0.55))]
    c = _cabi.Context(0)
    try:
        c.set_models(models)
        want = c.find_genes_batch(seqs, meta=True)
        c.train_batch([_seq("SRR492066"), _seq("KK037166")])
        got = c.find_genes_batch(seqs, meta=True)
        assert np.array_equal(want.contigs["model"], got.contigs["model"])
        assert len(want.genes) == len(got.genes)
        for k in ("begin", "end", "start_ndx", "stop_ndx", "cscore", "sscore"):
            assert np.array_equal(want.genes[k], got.genes[k]), k
    finally:
        c.close()


def test_train_batch_then_find_genes_batch_reproduces_the_per_genome_loop(genomes):
    lib = _lib()
    tinfs = lib.GeneFinder().train_batch(genomes)
    seqs = ["TTAATTAATTAA".join(g) if isinstance(g, (list, tuple)) else g for g in genomes]
    got = lib.GeneFinder().find_genes_batch(seqs, training_infos=tinfs)
    for k in (0, 4, 9):
        want = lib.GeneFinder(tinfs[k]).find_genes(seqs[k])
        assert [(x.begin, x.end, x.strand, x.score) for x in got[k]] == [(x.begin, x.end, x.strand, x.score) for x in want]
