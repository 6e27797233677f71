"""The inputs of tests/test_coding_score_gpu.py are what they claim to be: checked with the CPU oracle alone (tests/orf_shapes.py
builds them).  Also the assumption behind CS_LIST of k_coding_score_quads, restated over the oracle's sorted node arrays."""
import math

import numpy as np
import pytest

from oracle import oracle as orc
from tests import orf_shapes as osh
from tests import sets_ref as sr
from tests.util import golden_path, read_fasta

GENE_DC = orc.TRAINING_SIZE - 4096 * 8          # offset of gene_dc, the last member of struct _training


def extracted(seq, closed, min_gene=90):
    o = orc.Oracle(seq)
    o.extract(11, orc.Params(closed=closed, min_gene=min_gene, min_edge_gene=min(60, min_gene)))
    o.sort()
    return o


@pytest.fixture(scope="module", params=["designed", "short"])
def shaped(request):
    if request.param == "designed":
        seq, lay = osh.designed(layout=True)
        return seq, lay, 90, osh.SPANS
    seq, lay = osh.designed_short_edges(layout=True)
    return seq, lay, osh.SHORT_MIN_GENE, osh.SHORT_SPANS


@pytest.mark.parametrize("closed", [False, True])
def test_every_span_on_both_strands_with_its_planted_starts(shaped, closed):
    seq, lay, min_gene, spans = shaped
    o = orc.Oracle(seq)
    o.extract(11, orc.Params(closed=closed, min_gene=min_gene, min_edge_gene=min_gene))
    o.sort()
    nd = o.nodes()
    idx, sp, st = osh.orf_spans(nd, len(seq))
    at = {(int(nd["ndx"][i]), int(nd["strand"][i])): (int(i), int(n)) for i, n in zip(idx, sp)}
    seen = {1: set(), -1: set()}
    for p, strand, ncod, starts in lay:
        want = [ci for ci in starts if 3 * (ci + 2) >= min_gene]
        if not want:
            assert (p, strand) not in at and ncod in (16, 17) and min_gene == 90     # too short for a node: the short contig has them
            continue
        i, n = at[(p, strand)]
        assert n == ncod
        assert sorted(osh.start_codons_of(nd, len(seq), i)) == want                 # exactly the planted starts
        seen[strand].add(ncod)
    for strand in (1, -1):
        assert seen[strand] == set(spans) - ({16, 17} if min_gene == 90 else set())


def test_designed_contig_node_positions():
    seq = osh.designed()
    assert len(seq) < 165000
    nd = extracted(seq, False).nodes()
    fwd, rev = set(nd["ndx"][nd["strand"] == 1].tolist()), set(nd["ndx"][nd["strand"] == -1].tolist())
    assert len(fwd & rev) >= 10                                     # positions that hold a node of each strand
    for strand in (1, -1):
        at = nd["ndx"][nd["strand"] == strand]
        assert np.count_nonzero(at % 16 == 0) >= 50 and np.count_nonzero(at % 16 == 15) >= 50
    idx, sp, st = osh.orf_spans(nd, len(seq))
    # what test_coding_score_gpu.py asserts again before it relies on it: ORFs whose start lies in another piece of 256 nodes
    for strand in (1, -1):
        across = sum(1 for i in idx[st == strand] if any(k // 256 != i // 256 for k in osh.start_codons_of(nd, len(seq), i).values()))
        assert across >= 6


def length_factor(tinf, gsize):
    """ref: lib.pyx:2160-2210, table 11."""
    gc = tinf.gc
    no_stop = ((1 - gc) * (1 - gc) * gc) / 4.0
    no_stop += ((1 - gc) * (1 - gc) * (1 - gc)) / 8.0
    no_stop = 1 - no_stop
    lmax = math.log((1 - math.pow(no_stop, 1000.0)) / math.pow(no_stop, 1000.0))
    lmin = math.log((1 - math.pow(no_stop, 80)) / math.pow(no_stop, 80))
    if float(gsize) > 1000.0:
        return (lmax - lmin) * (float(gsize) - 80) / 920.0
    tmp = math.pow(no_stop, float(gsize))
    return math.log((1 - tmp) / tmp) - lmin


def test_ordered_hexamer_sums_pin_the_codon_numbering():
    """ORFs of 65, 257 and 2049 codons with one start, at their outermost codon: the hexamer sum from the stop outwards in codon
    order, plus the length factor, is the oracle's cscore bit for bit -- on both strands.  A helper that counted codons from
    another origin would plant every edge of the GPU tests one codon off."""
    pad = [999, 1000, 1001]
    seq, lay = osh.designed_contig(pad + [(n, [n - 1]) for n in (65, 257, 2049)] + pad, np.random.default_rng(5), layout=True)
    tinf = orc.Training.load(golden_path("SRR492066.training.bin.gz"))
    gene_dc = tinf.buf[GENE_DC:].view(np.float64)
    assert len(gene_dc) == 4096 and tinf.trans_table == 11
    o = extracted(seq, True)
    o.reset_scores()
    o.score_nodes(tinf, True, False)
    nd = o.nodes()
    digit = {65: 0, 71: 1, 67: 2, 84: 3}                              # A G C T
    text = {1: seq, -1: osh.revcomp(seq)}
    checked = 0
    for p, strand, ncod, starts in lay:
        if len(starts) != 1:
            continue
        stop = int(np.flatnonzero((nd["ndx"] == p) & (nd["strand"] == strand) & (nd["type"] == osh.T_STOP))[0])
        (ci, k), = osh.start_codons_of(nd, len(seq), stop).items()
        assert ci == ncod - 1 and osh.orf_codons(p, int(nd["stop_val"][stop]), strand, len(seq)) == ncod
        # a stop node of the same strand and frame lies further out: the running maxima of the reference start afresh at this ORF
        out = (nd["strand"] == strand) & (nd["type"] == osh.T_STOP) & (nd["ndx"] % 3 == p % 3)
        assert np.any(out & (nd["ndx"] < nd["ndx"][k])) if strand == 1 else np.any(out & (nd["ndx"] > nd["ndx"][k]))
        s = text[strand]
        p0 = p if strand == 1 else len(seq) - 1 - p                   # first base of the stop codon in reading direction
        total = 0.0
        for c in range(ci + 1):
            x = p0 - 3 * (c + 1)
            total += float(gene_dc[sum(digit[s[x + j]] << (2 * j) for j in range(6))])
        lfac = length_factor(tinf, ci + 2)
        if lfac > 3.0 and total < 0.5 * lfac:
            total = 0.5 * lfac
        total += lfac
        assert np.float64(total).view(np.uint64) == nd["cscore"][k:k + 1].view(np.uint64)[0], (ncod, strand)
        checked += 1
    assert checked == 6


def test_model_sets_fill_every_column_of_every_quad():
    """Decided by the oracle alone: under the model sets of the GPU test all window models of the GC 0.5 contig are scored, and
    the winners sit in at least three different columns of their quads, one of them in the second quad."""
    seqs = osh.model_contigs()
    gcs = [sr.gc_count(s) / len(s) for s in seqs]
    assert sr.window(gcs[1])[1] < sr.window(gcs[0])[0] and sr.window(gcs[0])[1] < sr.window(gcs[2])[0]
    slots = []
    for size in osh.MODEL_SET_SIZES:
        models = osh.model_set(size)
        n = sum(size) if isinstance(size, tuple) else size
        assert sr.models_in(gcs[0], models) == list(range(3, 3 + n))
        assert sr.models_in(gcs[1], models) == [0] and sr.models_in(gcs[2], models) == [1, 2]
        w = orc.Oracle(seqs[0]).find_genes_meta(models, orc.Params())
        slots.append(w - 3)
    assert len({s % 4 for s in slots}) >= 3 and any(s // 4 == 1 for s in slots) and any(s // 4 == 2 for s in slots)


# ---- CS_LIST ----------------------------------------------------------------------------------------------------------------------------

def _list_inputs():
    yield "designed", osh.designed(), 90
    yield "short", osh.designed_short_edges(), osh.SHORT_MIN_GENE
    yield "SRR492066", read_fasta("SRR492066.fna.gz")[0][1], 90
    yield "KK037166", read_fasta("KK037166.fna.gz")[0][1], 90
    yield "genome 100 kb", read_fasta("GCF_001457455.1_NCTC11397_genomic_100kb.fna.gz")[0][1], 90


@pytest.mark.parametrize("closed", [False, True])
def test_stop_nodes_of_a_piece_stay_within_the_list(closed):
    """k_coding_score_quads lists the stop nodes of a round in CS_LIST = 5120 slots and traps beyond: a piece of n consecutive nodes
    (cut at multiples of the task size, as pga_cs_tasks cuts) holds at most n / 2 + 12 stop nodes -- every stop node has a start
    node, and at each of the two cuts one ORF per strand and frame may have its starts on the other side."""
    for name, seq, min_gene in _list_inputs():
        o = orc.Oracle(seq)
        o.extract(11, orc.Params(closed=closed, min_gene=min_gene, min_edge_gene=min(60, min_gene)))
        o.sort()
        stop = o.nodes()["type"] == osh.T_STOP
        for piece in (256, 512, 5120, 8192):
            for f0 in range(0, len(stop), piece):
                n = min(piece, len(stop) - f0)
                assert int(stop[f0:f0 + n].sum()) <= n // 2 + 12, (name, piece, f0)
