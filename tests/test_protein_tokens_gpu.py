"""Proteins left on the device as token tensors (pga_translate_genes_tokens, ProteinTokens, Context.translate_tokens,
GeneFinder.find_proteins_batch).

Every expected value is an exact integer: the numpy restatement of the rule (tests/protein_tokens_ref.py) applied to the letters that
Context.translate_genes returns -- the existing path, pinned to tests/tables_ref.py, never the code under test.  Device memory comes
from tests/hip_mem.py (no torch), but for the one torch test, which runs in a child process."""
import ctypes
import functools
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import hip_mem
from tests.protein_tokens_ref import (AMINO_ACIDS, CIRCULAR, TABLES, protein_tokens_ref, synthetic_contigs, synthetic_proteins,
                                      synthetic_records, vocab_table)
from tests.util import read_fasta

pytestmark = pytest.mark.gpu

VOCAB = "-" + AMINO_ACIDS + "X*"                     # id = position: '-' 0 (the pad), A 1 .. Y 20, X 21, * 22
IDS = vocab_table(VOCAB)
BOS, EOS, PAD = 30, 31, 0
DTYPES = {"uint8": np.uint8, "int32": np.int32, "int64": np.int64}
CANARY = 0xA5


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi, benchdata
    c = _cabi.Context(0)
    c.set_models([b for _, b in benchdata.load_model_set()])
    yield c
    c.close()


LIVE = []        # what a test put on the device: closed when the test ends, passed or failed, while the module's context still exists


@pytest.fixture(autouse=True)
def release_device_objects():
    yield
    while LIVE:
        LIVE.pop().close()


def keep(x):
    LIVE.append(x)
    return x


class View:
    """A pointer into somebody's device memory with a shape: what `out=` takes."""

    def __init__(self, ptr, shape, dtype, strides=None):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": np.dtype(dtype).str if np.dtype(dtype).itemsize > 1 else "|u1",
                                         "data": (ptr, False), "version": 3, "strides": strides}


class Target:
    """An allocation full of a fill byte and a tensor that starts ONE element into it (element-aligned, nothing more), with `slack`
    elements behind the tensor: `expect()` is what the whole allocation must hold after a call."""

    def __init__(self, dtype, layout, n_genes, width, total, fill=CANARY, extra_stride=5, slack=40):
        self.dtype, self.layout, self.eb = np.dtype(dtype), layout, np.dtype(dtype).itemsize
        self.G, self.W, self.S = n_genes, width, width + extra_stride
        self.n = ((n_genes - 1) * self.S + width if n_genes else 0) if layout == "padded" else total
        self.before = np.full((1 + self.n + slack) * self.eb, fill, np.uint8)
        self.mem = keep(hip_mem.DeviceArray.from_numpy(self.before))
        self.ptr = self.mem.ptr + self.eb
        if layout == "padded":
            self.out = View(self.ptr, (n_genes, width), dtype, (self.S * self.eb, self.eb))
        else:
            self.out = View(self.ptr, (total,), dtype)

    def read(self):
        return self.mem.to_numpy(self.dtype)

    def expect(self, want):
        e = self.before.view(self.dtype).copy()
        if self.layout == "padded":
            for g in range(self.G):
                e[1 + g * self.S:1 + g * self.S + self.W] = want[g]
        else:
            e[1:1 + self.n] = want
        return e


def gene_array(recs):
    from pyrodigal_amd import _cabi
    genes = np.zeros(len(recs), _cabi.GENE_DTYPE)
    for name, col in zip(("contig", "begin", "end", "strand", "partial_begin", "partial_end"), zip(*recs)):
        genes[name] = col
    return genes


def letters_of(ctx, batch, genes, tables, **kw):
    """The proteins by the existing path (pga_translate_genes): one bytes per gene."""
    letters, off = ctx.translate_genes(batch, types.SimpleNamespace(genes=genes), tables=tables, **kw)
    return [letters[off[g]:off[g + 1]].tobytes() for g in range(len(genes))]


@pytest.fixture(scope="module")
def synthetic(ctx):
    """The synthetic batch, its records, and their proteins by the existing path with and without the final stop (computed once)."""
    batch = ctx.upload(synthetic_contigs())
    batch.set_circular(list(CIRCULAR))
    genes = gene_array(synthetic_records())
    prot = {stop: letters_of(ctx, batch, genes, TABLES, include_stop=stop) for stop in (False, True)}
    for stop in (False, True):                        # the existing path is the one tests/tables_ref.py describes, on these records too
        assert [p.decode() for p in prot[stop]] == synthetic_proteins(include_stop=stop)
    yield batch, genes, prot
    batch.close()


def spec_of(dtype, layout, bos, eos, **kw):
    from pyrodigal_amd import ProteinTokens
    return ProteinTokens(VOCAB, bos=BOS if bos else None, eos=EOS if eos else None, pad=PAD, dtype=dtype, layout=layout, **kw)


def run(ctx, batch, genes, tables, prot, spec, fill=CANARY, extra_width=3, extra_stride=5, **kw):
    """One call into a Target; returns (what the allocation holds, what it must hold, the DeviceProteins, the Target)."""
    ref = dict(bos=spec.bos, eos=spec.eos, pad=spec.pad, max_length=spec.max_length, dtype=DTYPES[spec.dtype])
    _, lens, off = protein_tokens_ref(prot, IDS, layout="ragged", **ref)
    width = int(lens.max(initial=0)) + extra_width
    t = Target(DTYPES[spec.dtype], spec.layout, len(genes), width, int(off[-1]), fill, extra_stride)
    want, _, _ = protein_tokens_ref(prot, IDS, layout=spec.layout, width=width, **ref)
    dp = ctx.translate_tokens(batch, genes, spec, out=t.out, tables=tables, **kw)
    assert dp.lengths.tolist() == lens.tolist() and dp.lengths.dtype == np.int64
    assert (dp.offsets is None) if spec.layout == "padded" else (dp.offsets.tolist() == off.tolist())
    return t.read(), t.expect(want), dp, t


# ---- 1. the synthetic records ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bos,eos", [(False, False), (True, True), (True, False), (False, True)])
@pytest.mark.parametrize("layout", ["ragged", "padded"])
@pytest.mark.parametrize("dtype", ["uint8", "int32", "int64"])
def test_synthetic_records(ctx, synthetic, dtype, layout, bos, eos):
    batch, genes, prot = synthetic
    spec = spec_of(dtype, layout, bos, eos)
    got, want, dp, t = run(ctx, batch, genes, TABLES, prot[False], spec)
    assert t.ptr % 16 == t.eb                                        # element-aligned only
    if dtype == "uint8" and layout == "ragged":
        assert len({(t.ptr + int(o)) % 16 for o in dp.offsets}) >= 8     # seams fall inside the 16-byte pieces
    assert np.array_equal(got, want)                                 # the tokens, and the canary everywhere else
    assert dp.gene_begin.tolist() == [0] + [int(np.sum(genes["contig"] <= c)) for c in range(3)]


def test_stop_letters_strictness_and_the_unknown_id(ctx, synthetic):
    """include_stop, strict = False and another unknown_residue reach the kernel; letters without an id of their own get `unknown`."""
    from pyrodigal_amd import ProteinTokens
    batch, genes, prot = synthetic
    got, want, _, _ = run(ctx, batch, genes, TABLES, prot[True], spec_of("int32", "ragged", True, True, include_stop=True))
    assert np.array_equal(got, want) and IDS[ord("*")] in got
    loose = letters_of(ctx, batch, genes, TABLES, include_stop=True, strict=False, unknown_residue="Z")
    assert loose != prot[True] and b"Z" in b"".join(loose)
    spec = ProteinTokens(AMINO_ACIDS, unknown=99, dtype="uint8", layout="padded", pad=255, include_stop=True, strict=False, unknown_residue="Z")
    ids = vocab_table(AMINO_ACIDS, unknown=99)
    lens = [len(p) for p in loose]
    t = Target(np.uint8, "padded", len(genes), max(lens) + 1, 0)
    dp = ctx.translate_tokens(batch, genes, spec, out=t.out, tables=TABLES)
    want, _, _ = protein_tokens_ref(loose, ids, pad=255, width=max(lens) + 1, dtype=np.uint8)
    assert np.array_equal(t.read(), t.expect(want)) and dp.lengths.tolist() == lens and 99 in want


def records_where(pick):
    return [k for k, r in enumerate(synthetic_records()) if pick(r)]


def tiny_records():
    """The records of 0 and 1 codons, the two that keep a residue without specials moved inwards: empty genes lead, lie between, trail."""
    tiny = records_where(lambda r: (r[2] - r[1] + 1) // 3 <= 1)
    return tiny[:3] + tiny[-2:-1] + tiny[3:6] + tiny[-1:] + tiny[6:-2]


# the degenerate shapes: which of the synthetic records, with bos and eos or without, and the columns beyond the longest gene
SHAPES = {
    "no record": (lambda: [], False, 3),
    "one record": (lambda: [40], True, 3),
    "empty genes": (tiny_records, False, 3),
    "empty genes, specials": (tiny_records, True, 3),
    "across the origin": (lambda: records_where(lambda r: r[0] == 1 and r[2] > len(synthetic_contigs()[1])), False, 3),
    "wide rows": (lambda: records_where(lambda r: True), True, 50),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("layout", ["ragged", "padded"])
@pytest.mark.parametrize("dtype", ["uint8", "int32", "int64"])
def test_smallest_shapes(ctx, synthetic, dtype, layout, shape):
    """The seams between rows where rows are few, empty or short (the counterpart of test_base_labels_gpu.py::test_smallest_shapes)."""
    batch, genes, prot = synthetic
    records, specials, extra_width = SHAPES[shape]
    pick = records()
    sub, sub_prot = np.ascontiguousarray(genes[pick]), [prot[False][k] for k in pick]
    n = [len(p) for p in sub_prot]
    if shape == "no record":
        assert n == []
    elif shape == "one record":
        assert len(n) == 1 and n[0] > 16
    elif shape.startswith("empty genes"):
        assert n == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 0]
    elif shape == "across the origin":
        assert len(n) == 2 and min(n) >= 19
    for extra_stride in (0, 5):
        got, want, _, t = run(ctx, batch, sub, TABLES, sub_prot, spec_of(dtype, layout, specials, specials), extra_width=extra_width,
                              extra_stride=extra_stride)
        assert t.ptr % 16 == t.eb
        assert np.array_equal(got, want), extra_stride


# ---- 2. truncation -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ragged", "padded"])
@pytest.mark.parametrize("dtype", ["uint8", "int64"])
def test_truncation_keeps_eos(ctx, synthetic, dtype, layout):
    batch, genes, prot = synthetic
    n = np.array([len(p) for p in prot[False]])
    assert (n > 16).sum() > 10 and (n == 16).sum() >= 2 and (n < 16).sum() > 10          # some truncate, some fit exactly, some fall short
    spec = spec_of(dtype, layout, True, True, max_length=18)
    got, want, dp, t = run(ctx, batch, genes, TABLES, prot[False], spec)
    assert np.array_equal(got, want)
    assert dp.lengths.max() == 18 and dp.lengths.tolist() == (np.minimum(n, 16) + 2).tolist()
    flat = want[1:1 + t.n] if layout == "ragged" else None
    for g in np.flatnonzero(n > 16)[:5]:
        row = flat[dp.offsets[g]:dp.offsets[g + 1]] if layout == "ragged" else want[1 + g * t.S:1 + g * t.S + t.W]
        assert row[0] == BOS and row[17] == EOS


# ---- 3. independence from old memory -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("poison", [None, 0xFF])
def test_result_does_not_depend_on_what_the_memory_held(ctx, synthetic, poison):
    batch, genes, prot = synthetic
    if poison is not None:
        ctx.debug_poison(poison)
    try:
        for dtype, layout in (("uint8", "ragged"), ("int32", "padded"), ("int64", "ragged")):
            spec = spec_of(dtype, layout, True, True)
            written = []
            for fill in (0xFF, 0x00):
                got, want, _, t = run(ctx, batch, genes, TABLES, prot[False], spec, fill=fill)
                assert np.array_equal(got, want)                     # the tokens, and the fill everywhere else
                named = t.expect(np.ones((t.G, t.W) if layout == "padded" else t.n, t.dtype)) != t.before.view(t.dtype)
                written.append(got[named])                           # the elements the rule names
            assert len(written[0]) == (t.G * t.W if layout == "padded" else t.n) and np.array_equal(written[0], written[1])
    finally:
        if poison is not None:
            ctx.debug_poison(None)


# ---- 4. stream order -----------------------------------------------------------------------------------------------------------------
def test_tokens_wait_for_the_producer_stream(ctx, synthetic):
    """A poison fill of `out` is on its way on a producer stream, behind twenty fills of 1 GB.  translate_tokens is called at once
    with that stream: it waits for the fill, so after the producer has drained `out` holds the tokens."""
    batch, genes, prot = synthetic
    hip = hip_mem.hip()
    spec = spec_of("int32", "ragged", True, True)
    want, lens, off = protein_tokens_ref(prot[False], IDS, bos=BOS, eos=EOS, layout="ragged", dtype=np.int32)
    out = keep(hip_mem.DeviceArray(4 * len(want), (len(want),), "<i4"))
    scratch = keep(hip_mem.DeviceArray(1 << 30))
    producer = hip_mem.Stream()
    try:
        for k in range(20):
            hip_mem.check(hip.hipMemsetAsync(scratch.ptr, k, scratch.nbytes, producer.cuda_stream), "hipMemsetAsync")
        hip_mem.check(hip.hipMemsetAsync(out.ptr, 0xEE, out.nbytes, producer.cuda_stream), "hipMemsetAsync")
        ctx.translate_tokens(batch, genes, spec, out=out, tables=TABLES, stream=producer)
        producer.synchronize()
        got = out.to_numpy(np.int32)
        assert np.array_equal(got, want)
    finally:
        producer.synchronize()                                       # (before the buffers it writes are released)
        producer.close()


# ---- 5. end to end on the committed fixtures -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def contigs():
    """The committed fixtures, cuts of them, a few contigs of 61 .. 400 bases, and one that ends in a copy of its first 40 bases (the
    contigs of tests/test_device_input_gpu.py)."""
    miij, srr, kk = (read_fasta(n + ".fna.gz")[0][1].encode() for n in ("MIIJ01000039", "SRR492066", "KK037166"))
    rng = np.random.default_rng(500)
    low = bytearray(srr[30000:42000])
    low[2000:2600] = bytes(low[2000:2600]).lower()
    circle = kk[4000:12000]
    out = [miij[:120000], srr, kk, miij[300000:300061], srr[1000:1400], bytes(low), kk[:3073], miij[500000:506145],
           np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=211)].tobytes(), circle + circle[:40], srr[50000:50100]]
    return tuple(out)


def model_tables(ctx, res):
    tts = [int(np.frombuffer(m[8:12].tobytes(), np.int32)[0]) for m in ctx._models]
    return [tts[c["model"]] if c["model"] >= 0 else 11 for c in res.contigs]


def test_meta_mode_end_to_end(ctx):
    seqs = list(contigs())
    batch = keep(ctx.upload(seqs))
    res = ctx.find_genes(batch, meta=True)
    assert len(res.genes) > 100
    prot = letters_of(ctx, batch, np.ascontiguousarray(res.genes), model_tables(ctx, res), include_stop=False)
    assert sum(map(len, prot)) > 10000
    for dtype, layout in (("int64", "padded"), ("uint8", "ragged")):
        spec = spec_of(dtype, layout, True, True)
        ref = dict(bos=BOS, eos=EOS, pad=PAD, dtype=DTYPES[dtype])
        _, lens, off = protein_tokens_ref(prot, IDS, layout="ragged", **ref)
        t = Target(DTYPES[dtype], layout, len(prot), int(lens.max()), int(off[-1]), extra_stride=0)
        want, _, _ = protein_tokens_ref(prot, IDS, layout=layout, **ref)
        dp = ctx.translate_tokens(batch, res, spec, out=t.out)              # a result: the tables are those of the winning models
        assert np.array_equal(t.read(), t.expect(want))
        assert dp.gene_begin.tolist() == [int(c["gene_begin"]) for c in res.contigs] + [len(res.genes)]
    # a reversed subset of the records: any subset, any order
    pick = np.arange(len(res.genes))[::-1][::3]
    sub = np.ascontiguousarray(res.genes[pick])
    spec = spec_of("int32", "ragged", False, True)
    want, lens, off = protein_tokens_ref([prot[k] for k in pick], IDS, eos=EOS, layout="ragged", dtype=np.int32)
    t = Target(np.int32, "ragged", len(sub), 0, int(off[-1]))
    dp = ctx.translate_tokens(batch, sub, spec, out=t.out, tables=model_tables(ctx, res))
    assert np.array_equal(t.read(), t.expect(want)) and dp.gene_begin is None
    with pytest.raises(ValueError, match="tables"):
        ctx.translate_tokens(batch, sub, spec, out=t.out)


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib
    return lib


@pytest.fixture(scope="module")
def bins(lib):
    from pyrodigal_amd import benchdata
    return lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])


FIELDS = ("begin", "end", "strand", "partial_begin", "partial_end", "start_type", "rbs_motif", "rbs_spacer", "gc_cont",
          "translation_table", "cscore", "rscore", "sscore", "tscore", "uscore", "score")


def same_genes(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.sequence.data == w.sequence.data
        assert [[getattr(x, f) for f in FIELDS] for x in g] == [[getattr(x, f) for f in FIELDS] for x in w], i
        assert (g.circular, g.cut, g.score, g.terminal_repeat) == (w.circular, w.cut, w.score, w.terminal_repeat)
        assert [x.translate() for x in g] == [x.translate() for x in w]


@pytest.mark.parametrize("case", ["circular", "device"])
def test_find_proteins_batch(ctx, lib, bins, case):
    from pyrodigal_amd import DeviceSequences
    seqs = list(contigs()[1:])
    options = {"translate": True}
    given = seqs
    if case == "circular":
        options["circular"] = [i in (0, 1, 8) for i in range(len(seqs))]
    else:
        d = keep(hip_mem.DeviceArray.from_numpy(np.frombuffer(b"".join(seqs), np.uint8)))
        given = DeviceSequences(d, [len(s) for s in seqs])
    want_genes = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_genes_batch(given, **options)
    prot = [g.translate() for genes in want_genes for g in genes]          # translate=True: the device's own letters (k_translate)
    assert len(prot) > 100
    spec = spec_of("int64", "padded", True, True, include_stop=True)
    want, lens, _ = protein_tokens_ref(prot, IDS, bos=BOS, eos=EOS, pad=PAD)
    t = Target(np.int64, "padded", len(prot), int(lens.max()), 0)
    finder = lib.GeneFinder(meta=True, metagenomic_bins=bins)
    got_genes, dp = finder.find_proteins_batch(given, spec, out=t.out, **options)
    same_genes(got_genes, want_genes)
    assert finder.stats["device_calls"] == 1
    assert np.array_equal(t.read(), t.expect(want)) and dp.lengths.tolist() == lens.tolist() and dp.tokens is t.out
    counts = [len(g) for g in want_genes]
    assert dp.gene_begin.tolist() == [0] + list(np.cumsum(counts)) and len(dp.proteins) == len(seqs)
    with pytest.raises(TypeError, match="ProteinTokens"):
        finder.find_proteins_batch(given, "ACDEFGHIKLMNPQRSTVWYX")


def test_find_proteins_batch_refuses_a_request_that_splits(lib):
    import gzip
    from tests.util import golden_path
    blobs = [gzip.open(golden_path(n)).read() for n in ("SRR492066.training.bin.gz", "GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz")]
    tinfs = [lib.TrainingInfo(raw=np.frombuffer(b, np.uint8).copy()) for b in blobs]
    seqs = list(contigs()[1:])
    small = lib.GeneFinder(coalesce_bases=50000)
    with pytest.raises(ValueError, match="device calls"):
        small.find_proteins_batch(seqs, spec_of("int64", "ragged", False, False), training_infos=[tinfs[i % 2] for i in range(len(seqs))])


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_host_and_leave_the_context_usable(ctx, synthetic):
    from pyrodigal_amd import _cabi
    batch, genes, prot = synthetic
    spec = spec_of("int32", "padded", True, True)
    _, lens, off = protein_tokens_ref(prot[False], IDS, bos=BOS, eos=EOS, layout="ragged")
    W, S, G = int(lens.max()), int(lens.max()) + 2, len(genes)
    need = (G - 1) * S + W
    mem = keep(hip_mem.DeviceArray.from_numpy(np.full(4 * (need + 8), CANARY, np.uint8)))
    tables = np.array(TABLES, np.int32)
    len_out = np.zeros(G, np.int64)

    def raw(ptr=mem.ptr, n_out=need, recs=genes, tt=tables, **change):
        o = spec.opts(W, S)
        for k, v in change.items():
            if k == "vocab_A":
                o.vocab[ord("A")] = v
            else:
                setattr(o, k, v)
        rc = ctx.L.pga_translate_genes_tokens(ctx.h, batch.h, len(recs), ctypes.c_void_p(recs.ctypes.data), ctypes.c_void_p(tt.ctypes.data),
                                              ctypes.byref(o), ctypes.c_void_p(ptr), n_out, None, ctypes.c_void_p(len_out.ctypes.data))
        return rc, ctx.L.pga_last_error(ctx.h).decode()

    host = np.zeros(need + 8, np.int32)
    outside = genes.copy()
    outside["end"][5] = 5000
    for what, kw, word in (("a host pointer", dict(ptr=host.ctypes.data), "not device memory"),
                           ("n_out_elems one too small", dict(n_out=need - 1), "n_out_elems"),
                           ("W one too small", dict(row_width=W - 1), "row_width"),
                           ("elem_bytes 2", dict(elem_bytes=2), "elem_bytes"),
                           ("an id of 256 with uint8", dict(elem_bytes=1, vocab_A=256), "256"),
                           ("max_length < s + 1", dict(max_length=2), "max_length"),
                           ("a pointer that is not element-aligned", dict(ptr=mem.ptr + 1), "aligned"),
                           ("a gene outside its contig", dict(recs=outside), "gene 5"),
                           ("an unknown table", dict(tt=np.array([11, 7, 4], np.int32)), "contig 1")):
        rc, msg = raw(**kw)
        assert rc == _cabi.PGA_EINVAL and word in msg, (what, rc, msg)
    with pytest.raises(ValueError, match="not device memory"):
        ctx.translate_tokens(batch, genes, spec, out=View(host.ctypes.data, (G, W), np.int32, (4 * S, 4)), tables=TABLES)
    assert np.all(host == 0) and np.all(mem.to_numpy(np.uint8) == CANARY)           # nothing was written anywhere
    rc, msg = raw()                                                                  # the context runs a good call afterwards
    assert rc == 0, msg
    assert len_out.tolist() == lens.tolist()
    want, _, _ = protein_tokens_ref(prot[False], IDS, bos=BOS, eos=EOS, pad=PAD, width=W, dtype=np.int32)
    got = mem.to_numpy(np.int32)
    for g in range(G):
        assert np.array_equal(got[g * S:g * S + W], want[g]), g


# ---- 7. torch ------------------------------------------------------------------------------------------------------------------------
TORCH_SCRIPT = r'''
import sys
import torch                                   # first: the library then binds to the HIP runtime of torch's wheel
if not torch.cuda.is_available():
    print("torch sees no GPU")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
import numpy as np
from pyrodigal_amd import DeviceProteins, ProteinTokens, benchdata, lib
from tests.protein_tokens_ref import AMINO_ACIDS, protein_tokens_ref, vocab_table

VOCAB = "-" + AMINO_ACIDS + "X*"
bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])
seqs = [benchdata.synthetic_contig(n, gc, 900 + i) for i, (n, gc) in enumerate(((20000, 0.4), (12345, 0.6), (61, 0.5), (30011, 0.5)))]
want_genes = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_genes_batch(seqs, translate=True)
prot = [g.translate() for genes in want_genes for g in genes]
assert len(prot) > 30
side = torch.cuda.Stream()
for layout, dtype in (("ragged", "int32"), ("padded", "int64")):
    spec = ProteinTokens(VOCAB, bos=30, eos=31, pad=0, dtype=dtype, layout=layout, include_stop=True)
    with torch.cuda.stream(side):
        genes, dp = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_proteins_batch(seqs, spec)
    assert isinstance(dp, DeviceProteins) and dp.tokens.is_cuda and dp.tokens.dtype == getattr(torch, dtype)
    assert [[(g.begin, g.end, g.strand) for g in x] for x in genes] == [[(g.begin, g.end, g.strand) for g in x] for x in want_genes]
    want, lens, off = protein_tokens_ref(prot, vocab_table(VOCAB), bos=30, eos=31, pad=0, layout=layout, dtype=np.dtype(dtype))
    assert np.array_equal(dp.tokens.cpu().numpy(), want), "tokens differ"
    cu = dp.cu_seqlens()
    assert cu.is_cuda and cu.dtype == torch.int32 and cu.cpu().tolist() == [0] + np.cumsum(lens).tolist()
    first = dp.proteins[0]
    assert first.data_ptr() == dp.tokens.data_ptr() and len(dp.proteins) == len(seqs)
    n0 = len(want_genes[0])
    assert np.array_equal(first.cpu().numpy(), want[:off[n0]] if layout == "ragged" else want[:n0])
print("torch protein tokens ok: %d genes" % len(prot))
'''


def test_torch_tensor_in_a_fresh_process(tmp_path):
    """torch is imported by the child alone (this process holds the library's HIP runtime and gets no second one); `out=None`
    allocates the tensor under torch's current stream.  The child says so when torch sees no GPU, and the test is skipped."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "torch_protein_tokens.py"
    script.write_text(TORCH_SCRIPT)
    done = subprocess.run([sys.executable, str(script), root], timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, "child ended with %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    if "torch sees no GPU" in done.stdout:
        pytest.skip("torch sees no GPU")
    assert "torch protein tokens ok" in done.stdout
