"""GPU parity of the whole finder under models whose scores tie.  Score arrays cannot be injected into `pga_find_genes`, but a
model with coarse tables can be loaded, and under it the scoring stage itself produces equal values: the connection scoring
inside the finder, the overlapping starts (k_ovl_stops), the traceback tail, the gene records and the start tweaks all have to
break ties as the reference does (ref: _connection.h:135/197 `>=` in ascending order, lib.pyx:1239-1251, 2279-2329).  Every node
field and every gene against the CPU oracle (compare_contig of test_finder_gpu.py); each case asserts from the oracle's event
counters (Oracle.dp_events) that ties were decided on its input.

  model (a)  a blank training info: translation table 11, gc 0.5, start weight 0, every table zero -- only the length factor of
             the coding score is left, and it is equal for ORFs of equal length
  model (b)  the SRR492066 model with every table entry (all doubles from byte 80 on) and the three start-type weights rounded to
             whole numbers, start weight 0.0 or 4.0

The models are built here from the committed fixtures."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_finder_gpu import compare_contig
from tests.util import golden_path, read_fasta, synthetic_contig

pytestmark = pytest.mark.gpu

ENV = ("PGA_TAIL", "PGA_DP_KERNEL", "PGA_DP_SEG_WAVE")


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def clean_env():
    saved = {k: os.environ.pop(k, None) for k in ENV}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def model_a(gc=0.5):
    t = orc.Training()
    t.set_trans_table(11)
    t.set_gc(gc)
    t._f64(16)[0] = 0.0
    return t


def model_b(st_wt, gc=None):
    t = orc.Training.load(golden_path("SRR492066.training.bin.gz"))
    tables = t.buf[80:].view(np.float64)          # rbs_wt, ups_comp, mot_wt, no_mot, gene_dc
    tables[:] = np.round(tables)
    t.type_wt[:] = np.round(t.type_wt)
    t._f64(16)[0] = st_wt
    if gc is not None:
        t.set_gc(gc)
    return t


def events(seq, tinf, closed=False, is_meta=False):
    """The oracle's tie counters of the gene prediction pass of `seq` under `tinf`."""
    o = orc.Oracle(seq)
    o.extract(tinf.trans_table, orc.Params(closed=closed)); o.sort(); o.reset_scores()
    o.score_nodes(tinf, closed, is_meta)
    o.overlapping_starts(tinf, 1, 60)
    ev = o.dp_events()
    o.dprog_raw(tinf, True)
    o.find_max_index()
    ev.update({k: v for k, v in o.dp_events().items() if k != "ovl_ties"})
    return ev


S20K = synthetic_contig(20000, 0.5, 5)


def srr():
    return read_fasta("SRR492066.fna.gz")[0][1].encode()


SINGLE = {                                        # model, sequence, genes the oracle finds
    "a": (lambda: model_a(), lambda: S20K, 19),
    "b_st0": (lambda: model_b(0.0), srr, 84),
    "b_st4": (lambda: model_b(4.0), srr, 75),
}


@pytest.mark.parametrize("kernel", ["default", "wave"])
@pytest.mark.parametrize("tail", ["device", "host"])
@pytest.mark.parametrize("case", list(SINGLE))
def test_single_mode_under_models_that_tie(ctx, case, tail, kernel):
    make_model, make_seq, n_genes = SINGLE[case]
    tinf, seq = make_model(), make_seq()
    ev = events(seq, tinf)
    assert ev["ties"] >= 200, ev
    os.environ["PGA_TAIL"] = tail
    if kernel != "default":
        os.environ["PGA_DP_KERNEL"] = kernel
    ctx.set_models([tinf.buf])
    # the target contig alone, and among others (launches of many chains take other kernels than a launch of one)
    others = [synthetic_contig(4000 + 1500 * k, 0.42 + 0.03 * k, 8800 + k) for k in range(6)]
    for seqs in ([seq], others[:3] + [seq] + others[3:]):
        res = ctx.find_genes_batch(seqs, meta=False, want_nodes=True)
        got = [compare_contig(res, i, s, orc.Oracle(s), [tinf], meta=False) for i, s in enumerate(seqs)]
        assert got[seqs.index(seq)] == n_genes
        res = ctx.find_genes_batch(seqs, meta=False)                      # the path proper: no node arrays
        assert [compare_contig(res, i, s, orc.Oracle(s), [tinf], meta=False) for i, s in enumerate(seqs)] == got


@pytest.fixture(scope="module")
def bins():
    """The models that tie, labelled for the GC windows of the contigs below, next to two ordinary models."""
    return [orc.Training.load(golden_path("SRR492066.training.bin.gz")),                                        # gc 0.301
            orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz")),      # gc 0.558
            model_a(0.5), model_b(0.0, 0.5), model_b(4.0, 0.5), model_a(0.30), model_b(0.0, 0.30), model_b(4.0, 0.30)]


META_SEQS = [S20K, synthetic_contig(9000, 0.45, 3), synthetic_contig(30000, 0.55, 4), synthetic_contig(2500, 0.5, 8),
             synthetic_contig(60000, 0.5, 6), synthetic_contig(12000, 0.31, 9), b"", b"ATGAAATAA"]


@pytest.mark.parametrize("kernel", ["default", "wave"])
@pytest.mark.parametrize("tail", ["device", "host"])
def test_meta_mode_with_models_that_tie_among_the_bins(ctx, bins, tail, kernel):
    seqs = META_SEQS + [srr()]
    os.environ["PGA_TAIL"] = tail
    if kernel != "default":
        os.environ["PGA_DP_KERNEL"] = kernel
    ctx.set_models([m.buf for m in bins])
    for closed in (False, True):
        res = ctx.find_genes_batch(seqs, meta=True, closed=closed, want_nodes=True)
        n = sum(compare_contig(res, i, s, orc.Oracle(s), bins, meta=True, closed=closed) for i, s in enumerate(seqs))
        assert n > 100
        # models that tie win contigs, and ties were decided in the winning passes
        won = [(i, int(res.contigs[i]["model"])) for i in range(len(seqs)) if res.contigs[i]["model"] >= 2]
        assert len(won) >= 3, won
        assert sum(events(seqs[i], bins[m], closed, True)["ties"] for i, m in won) >= 200


def test_segments_of_a_genome_under_a_model_that_ties(ctx):
    """The full genome under model (a): 3.5 million ties.  Its one chain is cut into segments, walked by the chain kernel (the
    default for a chain of this length) and by the wave-batch kernel (PGA_DP_SEG_WAVE=1), verified and given to the parallel tail."""
    seq = read_fasta("GCF_001457455.1_NCTC11397_genomic.fna.gz")[0][1]
    tinf = model_a()
    ev = events(seq, tinf, closed=True)
    assert ev["ties"] >= 100_000 and ev["ovl_ties"] >= 1, ev
    ctx.set_models([tinf.buf])
    first = None
    for seg_wave in ("0", "1"):
        os.environ["PGA_DP_SEG_WAVE"] = seg_wave
        res = ctx.find_genes_batch([seq], meta=False, closed=True, want_nodes=True)
        st = ctx.dp_stats()
        print(f"PGA_DP_SEG_WAVE={seg_wave}: segments {st['segments']} rejected {st['rejected']} serial {st['serial']}")
        assert st["chains"] == 1
        if first is None:
            first = res
            assert compare_contig(res, 0, seq, orc.Oracle(seq), [tinf], meta=False, closed=True) > 2000
        else:
            assert res.genes.tobytes() == first.genes.tobytes()
            for k in ("traceb", "tracef", "ov_mark", "elim"):
                assert np.array_equal(res.nodes[0][k], first.nodes[0][k]), k
            for k in ("score", "sscore"):
                assert np.array_equal(res.nodes[0][k].view(np.uint64), first.nodes[0][k].view(np.uint64)), k
