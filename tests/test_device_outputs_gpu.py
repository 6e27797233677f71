"""The host steps that the seven device-tensor outputs share, on one tiny batch: three contigs of 90, 0 and 63
bases, the third flagged circular, and five records, one of them across the origin of the third.

The entry points that read bases (pga_label_bases, pga_gene_windows, pga_count_kmers) must refuse a malformed record in the same
words, the ones that read proteins (pga_translate_genes_tokens, pga_group_proteins, pga_sketch_proteins) an unknown translation
table, and every entry point that takes a destination a pointer off by one byte.  After all refusals one good call of each output,
with no stream and with a side stream, must equal the host references (tests/*_ref.py) -- never the code under test.  The start
candidates are not written for a batch with circular flags (asserted): their good call runs on the same three sequences uploaded
without the flag.  Device memory comes from tests/hip_mem.py (no torch)."""
import numpy as np
import pytest

from tests import hip_mem
from tests import protein_groups_ref as groups_ref
from tests import protein_sketches_ref as sketches_ref
from tests.base_labels_ref import base_labels_ref, preset_map
from tests.gene_windows_ref import gene_windows_ref
from tests.kmer_counts_ref import kmer_counts_ref
from tests.protein_tokens_ref import AMINO_ACIDS, protein_tokens_ref, vocab_table
from tests.start_candidates_ref import start_candidates_ref

pytestmark = pytest.mark.gpu

SEQS = [b"ATG" + (b"GCTAAAGACCTGGAA" * 6)[:84] + b"TAA", b"", (b"GCAGGTCCATACGTT" * 5)[:63]]
CIRCULAR = [False, False, True]
TABLES = [11, 11, 4]
# (contig, begin, end, strand, partial_begin, partial_end): whole codons; the second and third hold the same bases (the contig repeats
# every 15), the last runs across the origin of the circle
RECORDS = [(0, 1, 90, 1, 0, 0), (0, 4, 33, 1, 1, 1), (0, 19, 48, 1, 1, 1), (0, 34, 63, -1, 0, 0), (2, 52, 75, -1, 0, 0)]
VOCABULARY = AMINO_ACIDS + "*X"
PAIRS = [(0, 1), (1, 2), (3, 4), (4, 9)]                          # (the last names a record that does not exist: -1, -1)


def gene_array(recs):
    from pyrodigal_amd import _cabi
    genes = np.zeros(len(recs), _cabi.GENE_DTYPE)
    for name, col in zip(("contig", "begin", "end", "strand", "partial_begin", "partial_end"), zip(*recs)):
        genes[name] = col
    return genes


LIVE = []        # what a test put on the device: closed when the test ends, passed or failed, while the module's context still exists


def keep(x):
    LIVE.append(x)
    return x


class View:
    """A pointer into somebody's device memory with a shape: what `out=` takes."""

    def __init__(self, ptr, shape, dtype):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": np.dtype(dtype).str, "data": (ptr, False), "version": 3,
                                         "strides": None}


class Out:
    """A zeroed device tensor of a shape, and the same memory one byte on."""

    def __init__(self, shape, dtype):
        self.shape, self.dtype, self.mem = tuple(shape), np.dtype(dtype), None
        self.zero()

    def zero(self):
        if self.mem is not None:
            self.mem.close()
        self.mem = keep(hip_mem.DeviceArray.from_numpy(np.zeros(int(np.prod(self.shape)) + 2, self.dtype)))
        self.view, self.skewed = View(self.mem.ptr, self.shape, self.dtype), View(self.mem.ptr + 1, self.shape, self.dtype)

    def read(self):
        return self.mem.to_numpy(self.dtype)[:int(np.prod(self.shape))].reshape(self.shape)


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi, benchdata
    c = _cabi.Context(0)
    c.set_models([b for _, b in benchdata.load_model_set()])
    yield c
    while LIVE:
        LIVE.pop().close()
    c.close()


def message(call, fn):
    """What a refused call says, without the name of the function in front."""
    with pytest.raises(ValueError) as e:
        call()
    text = str(e.value)
    assert text.startswith(fn + ": ")
    while text.startswith(fn + ": "):
        text = text[len(fn) + 2:]
    return text


def rules():
    from pyrodigal_amd import BaseLabels, GeneWindows, KmerCounts, ProteinGroups, ProteinSketches, ProteinTokens, StartCandidates
    return dict(tokens=ProteinTokens(VOCABULARY, pad=99, layout="padded"), labels=BaseLabels("frame", layout="ragged"),
                windows=GeneWindows(("start", -6), ("end", 6), layout="ragged"), counts=KmerCounts(2, rows="gene"),
                groups=ProteinGroups("protein"), sketches=ProteinSketches(3, 4), starts=StartCandidates(dtype="float64"))


def references(r):
    """What every output must hold for RECORDS, from the host references."""
    want = {}
    proteins = [groups_ref.string_of(SEQS, CIRCULAR, rec, "protein", TABLES) for rec in RECORDS]
    want["tokens"] = protein_tokens_ref(proteins, vocab_table(VOCABULARY), pad=99, layout="padded")[0]
    want["labels"] = base_labels_ref([len(s) for s in SEQS], RECORDS, preset_map("frame"), "ragged")[0]
    want["windows"], _, want["window_lengths"] = gene_windows_ref(SEQS, CIRCULAR, RECORDS, r["windows"].begin, r["windows"].end,
                                                                  ids=r["windows"].ids, layout="ragged")
    want["counts"], want["count_windows"] = kmer_counts_ref(SEQS, CIRCULAR, RECORDS, 2, "gene", 1, r["counts"].table, r["counts"].n_bins)
    want["groups"] = groups_ref.protein_groups_ref(SEQS, CIRCULAR, RECORDS, "protein", TABLES)[:4]
    want["sketches"] = sketches_ref.protein_sketches_ref(SEQS, CIRCULAR, RECORDS, 3, 4, "protein", 0, None, TABLES)[:3]
    want["pairs"] = sketches_ref.pairs_ref(want["sketches"][0], PAIRS, 4)
    return want


def test_shared_refusals_then_every_output(ctx):
    r = rules()
    want = references(r)
    genes, G = gene_array(RECORDS), len(RECORDS)
    batch = keep(ctx.upload(SEQS))
    batch.set_circular(CIRCULAR)
    big = Out((4096,), np.int64)

    # ---- 1. a malformed record: the same words from the three entry points that read bases ----
    for bad, words in (((3, 1, 30, 1, 0, 0), "gene 1 names contig 3 of 3"), ((0, 0, 29, 1, 0, 0), "gene 1 lies outside its contig"),
                       ((0, 1, 4, 1, 0, 0), "gene 1 is 4 bases long, no whole number of codons"),
                       ((0, 70, 99, 1, 0, 0), "gene 1 ends beyond its contig, which is not flagged circular")):
        two = gene_array([RECORDS[0], bad])
        said = [message(lambda: ctx.label_bases(batch, two, r["labels"], out=big.view), "pga_label_bases"),
                message(lambda: ctx.gene_windows(batch, two, r["windows"], out=big.view), "pga_gene_windows"),
                message(lambda: ctx.kmer_counts(batch, two, r["counts"], out=Out((2, 16), np.int32).view), "pga_count_kmers")]
        print(bad, said)
        assert said[0] == said[1] == said[2] == words

    # ---- 2. an unknown translation table: the same words from the three entry points that read proteins ----
    tokens_out = Out(want["tokens"].shape, np.int64)
    group_out = [Out((G,), np.int64), Out((G,), np.int64), Out((G,), np.int64), Out((G, 2), np.int64)]
    sketch_out = [Out((G, 4), np.int64), Out((G,), np.int64), Out((G,), np.int64)]
    said = [message(lambda: ctx.translate_tokens(batch, genes, r["tokens"], out=tokens_out.view, tables=[11, 7, 4]), "pga_translate_genes_tokens"),
            message(lambda: ctx.protein_groups(batch, genes, r["groups"], tables=[11, 7, 4], out=[o.view for o in group_out]), "pga_group_proteins"),
            message(lambda: ctx.protein_sketches(batch, genes, r["sketches"], tables=[11, 7, 4], out=[o.view for o in sketch_out]), "pga_sketch_proteins")]
    print(said)
    assert said[0] == said[1] == said[2] == "contig 1: 7 is not a valid translation table index"

    # ---- 3. the start candidates: not for this batch; the same sequences without the flag, every start node a record ----
    assert "circular" in message(lambda: ctx.start_candidates(batch, genes, r["starts"]), "pga_start_plan_create")
    linear = keep(ctx.upload(SEQS))
    res = ctx.find_genes(linear, meta=True, want_nodes=True)
    nodes = [res.nodes[i] for i in range(len(res.nodes))]
    starts = [(c, y) for c, nd in enumerate(nodes) for y in range(nd["n"]) if int(nd["type"][y]) != 3]
    start_genes = np.zeros(len(starts), genes.dtype)
    for g, (c, y) in enumerate(starts):
        nd = nodes[c]
        fwd = int(nd["strand"][y]) == 1
        ndx, sv = int(nd["ndx"][y]), int(nd["stop_val"][y])
        start_genes["contig"][g], start_genes["start_ndx"][g], start_genes["strand"][g] = c, y, 1 if fwd else -1
        start_genes["begin"][g], start_genes["end"][g] = (ndx + 1, sv + 3) if fwd else (sv - 1, ndx + 1)
    want["starts"] = start_candidates_ref(nodes, starts, r["starts"].fields, "ragged")
    T, F = len(want["starts"][0]), len(r["starts"].fields)
    print("start nodes:", len(starts), "candidates:", T)
    assert T > 0
    start_out = [Out((T,), np.int64), Out((T,), np.int64), Out((T, F), np.float64)]

    # ---- 4. a pointer off by one byte: every entry point that takes a destination ----
    def skew(outs, k=0):
        return [o.skewed if j == k else o.view for j, o in enumerate(outs)]

    label_out, window_out = Out(want["labels"].shape, np.int64), Out(want["windows"].shape, np.int64)
    count_out = Out(want["counts"].shape, np.int32)
    pair_in = keep(hip_mem.DeviceArray.from_numpy(np.array(PAIRS, np.int64)))
    pair_out = [Out((len(PAIRS),), np.int64), Out((len(PAIRS),), np.int64)]
    made = ctx.protein_sketches(batch, genes, r["sketches"], tables=TABLES, out=[o.view for o in sketch_out])
    for fn, name, n, call in (
            ("pga_translate_genes_tokens", "d_out", 8, lambda: ctx.translate_tokens(batch, genes, r["tokens"], out=tokens_out.skewed, tables=TABLES)),
            ("pga_label_bases", "d_out", 8, lambda: ctx.label_bases(batch, genes, r["labels"], out=label_out.skewed)),
            ("pga_gene_windows", "d_out", 8, lambda: ctx.gene_windows(batch, genes, r["windows"], out=window_out.skewed)),
            ("pga_count_kmers", "d_out", 4, lambda: ctx.kmer_counts(batch, genes, r["counts"], out=count_out.skewed)),
            ("pga_group_proteins", "d_group", 8, lambda: ctx.protein_groups(batch, genes, r["groups"], tables=TABLES, out=skew(group_out))),
            ("pga_group_proteins", "d_digest", 8, lambda: ctx.protein_groups(batch, genes, r["groups"], tables=TABLES, out=skew(group_out, 3))),
            ("pga_sketch_proteins", "d_sketch", 8, lambda: ctx.protein_sketches(batch, genes, r["sketches"], tables=TABLES, out=skew(sketch_out))),
            ("pga_sketch_proteins", "d_windows", 8, lambda: ctx.protein_sketches(batch, genes, r["sketches"], tables=TABLES, out=skew(sketch_out, 2))),
            ("pga_sketch_pairs", "d_shared", 8, lambda: made.compare(pair_in, out=skew(pair_out))),
            ("pga_start_plan_write", "d_positions", 8, lambda: ctx.start_candidates(linear, start_genes, r["starts"], out=skew(start_out))),
            ("pga_start_plan_write", "d_scores", 8, lambda: ctx.start_candidates(linear, start_genes, r["starts"], out=skew(start_out, 2)))):
        said = message(call, fn)
        print(fn, said)
        assert said == f"{name} is not aligned to its {n}-byte elements"

    # ---- 5. the good calls, on no stream and on a side stream ----
    side = hip_mem.Stream()
    try:
        for stream in (None, side):
            ds = ctx.start_candidates(linear, start_genes, r["starts"], out=[o.view for o in start_out], stream=stream)
            pos, typ, sco, lens, chosen, _ = want["starts"]
            assert ds.lengths.tolist() == lens.tolist() and ds.chosen.tolist() == chosen.tolist()
            assert np.array_equal(start_out[0].read(), pos) and np.array_equal(start_out[1].read(), typ)
            assert np.array_equal(start_out[2].read(), sco.reshape(T, F))
            ds.release()

            d = ctx.translate_tokens(batch, genes, r["tokens"], out=tokens_out.view, tables=TABLES, stream=stream)
            assert np.array_equal(tokens_out.read(), want["tokens"]) and d.gene_begin.tolist() == [0, 4, 4, 5]
            ctx.label_bases(batch, genes, r["labels"], out=label_out.view, stream=stream)
            assert np.array_equal(label_out.read(), want["labels"])
            d = ctx.gene_windows(batch, genes, r["windows"], out=window_out.view, stream=stream)
            assert np.array_equal(window_out.read(), want["windows"]) and d.lengths.tolist() == want["window_lengths"].tolist()
            d = ctx.kmer_counts(batch, genes, r["counts"], out=count_out.view, stream=stream)
            assert np.array_equal(count_out.read(), want["counts"]) and d.windows.tolist() == want["count_windows"].tolist()
            d = ctx.protein_groups(batch, genes, r["groups"], tables=TABLES, out=[o.view for o in group_out], stream=stream)
            group, reps, sizes, digests = want["groups"]
            U = len(reps)
            assert d.n_groups == U and np.array_equal(group_out[0].read(), group) and np.array_equal(group_out[3].read(), digests)
            assert np.array_equal(group_out[1].read()[:U], reps) and np.array_equal(group_out[2].read()[:U], sizes)
            d = ctx.protein_sketches(batch, genes, r["sketches"], tables=TABLES, out=[o.view for o in sketch_out], stream=stream)
            for o, w in zip(sketch_out, want["sketches"]):
                assert np.array_equal(o.read(), np.asarray(w, np.int64).reshape(o.shape))
            d.compare(pair_in, out=[o.view for o in pair_out], stream=stream)
            shared, union = want["pairs"]
            assert np.array_equal(pair_out[0].read(), shared) and np.array_equal(pair_out[1].read(), union)
            for outs in ([tokens_out, label_out, window_out, count_out], group_out, sketch_out, pair_out, start_out):
                for o in outs:                                        # (the second round writes into zeros again)
                    o.zero()
    finally:
        side.close()
