"""Per-base gene labels left on the device as a tensor aligned with the input (pga_label_bases, BaseLabels, Context.label_bases,
GeneFinder.find_labels_batch).

Every expected value is an exact integer: the numpy restatement of the rule (tests/base_labels_ref.py) applied to records the test
wrote by hand or to records the existing finder path returned -- never the code under test.  Device memory comes from
tests/hip_mem.py (no torch), but for the one torch test, which runs in a child process."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hip_mem
from tests.base_labels_ref import base_labels_ref, preset_map
from tests.util import read_fasta

pytestmark = pytest.mark.gpu

DTYPES = {"uint8": np.uint8, "int32": np.int32, "int64": np.int64}
PAD = {"uint8": 250, "int32": -100, "int64": -100}
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

    def __init__(self, dtype, layout, lengths, width=None, fill=CANARY, extra_stride=5, slack=40):
        self.dtype, self.layout, self.eb = np.dtype(dtype), layout, np.dtype(dtype).itemsize
        self.B, self.W = len(lengths), max(lengths, default=0) if width is None else width
        self.S = self.W + extra_stride
        self.n = ((self.B - 1) * self.S + self.W if self.B else 0) if layout == "padded" else int(sum(lengths))
        self.before = np.full((1 + self.n + slack) * self.eb, fill, np.uint8)
        self.mem = keep(hip_mem.DeviceArray.from_numpy(self.before))
        self.ptr = self.mem.ptr + self.eb
        if layout == "padded":
            self.out = View(self.ptr, (self.B, self.W), dtype, (self.S * self.eb, self.eb))
        else:
            self.out = View(self.ptr, (self.n,), dtype)

    def read(self):
        return self.mem.to_numpy(self.dtype)

    def expect(self, want):
        e = self.before.view(self.dtype).copy()
        if self.layout == "padded":
            for i in range(self.B):
                e[1 + i * self.S:1 + i * self.S + self.W] = want[i]
        else:
            e[1:1 + self.n] = want
        return e


def gene_array(recs):
    from pyrodigal_amd import _cabi
    genes = np.zeros(len(recs), _cabi.GENE_DTYPE)
    for name, col in zip(("contig", "begin", "end", "strand", "partial_begin", "partial_end"), zip(*recs)):
        genes[name] = col
    return genes


def letters(n, seed):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, size=n)].tobytes()


def gene(contig, begin, codons, strand, partial_begin=0, partial_end=0):
    return (contig, begin, begin + 3 * codons - 1, strand, partial_begin, partial_end)


# ---- the synthetic batch: about 2 kbp, written by hand -------------------------------------------------------------------------------
SYN_LENGTHS = [700, 333, 600, 450]
SYN_CIRCULAR = [False, False, True, False]
SYN_RECORDS = [
    gene(0, 1, 30, 1, partial_begin=1),          # from base 1, its partial flag on: no start codon
    gene(0, 100, 33, -1),                        # [100, 198]
    gene(0, 195, 35, 1),                         # [195, 299]: four bases under the reverse gene before it
    gene(0, 296, 30, 1),                         # [296, 385]: a 4-base same-strand overlap, another frame
    gene(0, 290, 20, -1),                        # [290, 349]: 296 .. 299 lie under three genes
    gene(0, 611, 30, 1, partial_end=1),          # to base L = 700, its partial flag on: no stop codon
    gene(1, 1, 20, 1),                           # from base 1, flag off
    gene(1, 70, 10, -1, 1, 1),                   # both flags on a reverse gene
    gene(1, 274, 20, -1),                        # to base L = 333, flag off: the reverse gene's start codon ends the contig
    gene(2, 599, 40, 1),                         # [599, 718] on the circle of 600: the start codon 599, 600, 1 straddles the origin
    gene(2, 450, 51, 1),                         # [450, 602]: the stop codon 600, 1, 2 straddles it
    gene(2, 590, 30, -1),                        # [590, 679]: a reverse gene across it
    gene(2, 200, 25, -1, partial_begin=1),
    gene(3, 1, 25, -1, partial_begin=1),         # from base 1, reverse, flag on: no stop codon
    gene(3, 376, 25, 1),                         # to base L = 450, flag off
    gene(3, 100, 60, 1, 0, 1),
]


@pytest.fixture(scope="module")
def synthetic(ctx):
    assert sum(SYN_LENGTHS) == 2083 and all(r[2] <= SYN_LENGTHS[r[0]] or SYN_CIRCULAR[r[0]] for r in SYN_RECORDS)
    batch = ctx.upload([letters(n, 40 + i) for i, n in enumerate(SYN_LENGTHS)])
    batch.set_circular(SYN_CIRCULAR)
    yield batch
    batch.close()


def spec_of(dtype, layout, classes="raw"):
    from pyrodigal_amd import BaseLabels
    return BaseLabels(classes, pad=PAD[dtype], dtype=dtype, layout=layout)


def run(ctx, batch, lengths, records, spec, width=None, fill=CANARY, **kw):
    """One call into a Target: (what the allocation holds, what it must hold, the DeviceLabels, the Target)."""
    t = Target(DTYPES[spec.dtype], spec.layout, lengths, width, fill, **kw)
    want, off = base_labels_ref(lengths, records, preset_map(spec.classes), layout=spec.layout, pad=spec.pad, width=t.W, dtype=DTYPES[spec.dtype])
    dl = ctx.label_bases(batch, gene_array(records) if records else gene_array([gene(0, 1, 1, 1)])[:0], spec, out=t.out)
    assert dl.lengths.tolist() == list(lengths) and dl.lengths.dtype == np.int64 and dl.labels is t.out
    assert (dl.offsets is None) if spec.layout == "padded" else (dl.offsets.tolist() == off.tolist())
    return t.read(), t.expect(want), dl, t


# ---- 1. the synthetic records --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", ["raw", "frame"])
@pytest.mark.parametrize("layout", ["ragged", "padded"])
@pytest.mark.parametrize("dtype", ["uint8", "int32", "int64"])
def test_synthetic_records(ctx, synthetic, dtype, layout, classes):
    got, want, dl, t = run(ctx, synthetic, SYN_LENGTHS, SYN_RECORDS, spec_of(dtype, layout, classes), width=max(SYN_LENGTHS) + 3)
    assert t.ptr % 16 == t.eb and t.S == t.W + 5                     # element-aligned only; rows a stride apart
    assert np.array_equal(got, want)                                 # the labels, and the canary everywhere else
    if classes == "raw" and layout == "ragged":
        flat = want[1:1 + t.n]
        assert {0x41, 0x84, 0x48, 0xa0} <= set(flat.tolist()) and int((flat == 0).sum()) > 300
        third = flat[dl.offsets[2]:dl.offsets[3]]
        assert third[0] & 0x40 and third[598] & 0x40 and third[1] & 0x80 and third[599] & 0x80     # codons on both sides of the origin


# ---- 2. the smallest shapes at which the kernel can go wrong ---------------------------------------------------------------------------
SMALL_LENGTHS = [0, 1, 2, 15, 16, 17, 31, 33, 3, 1, 5, 2, 4, 1, 3, 5, 0, 0, 7]      # first and last without genes
SMALL_RECORDS = [gene(3, 1, 5, 1), gene(4, 2, 5, -1, 0, 1), gene(5, 3, 5, 1), gene(6, 1, 4, 1), gene(6, 11, 7, -1), gene(7, 1, 11, 1),
                 gene(7, 4, 9, -1), gene(8, 1, 1, 1), gene(10, 2, 1, -1), gene(12, 2, 1, 1, 1, 0), gene(14, 1, 1, -1), gene(15, 3, 1, 1)]
SHAPES = {
    "odd lengths and a run of tiny contigs": (SMALL_LENGTHS, SMALL_RECORDS, None),
    "no gene at all": (SMALL_LENGTHS, [], None),
    "one contig": ([33], [gene(0, 1, 11, 1), gene(0, 4, 9, -1)], None),
    "one contig of one base": ([1], [], None),
    "W larger than every contig": (SMALL_LENGTHS, SMALL_RECORDS, 50),
}


@pytest.fixture(scope="module")
def small_batches(ctx):
    made = {}
    for lengths in ([33], [1], SMALL_LENGTHS):
        made[tuple(lengths)] = ctx.upload([letters(n, 7 + n) for n in lengths])
    yield made
    for b in made.values():
        b.close()


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("layout", ["ragged", "padded"])
@pytest.mark.parametrize("dtype", ["uint8", "int32", "int64"])
def test_smallest_shapes(ctx, small_batches, dtype, layout, shape):
    lengths, records, width = SHAPES[shape]
    for extra_stride in (0, 5):
        got, want, _, t = run(ctx, small_batches[tuple(lengths)], lengths, records, spec_of(dtype, layout, "raw"), width=width,
                              extra_stride=extra_stride)
        assert np.array_equal(got, want), extra_stride


# ---- 3. record order does not matter ---------------------------------------------------------------------------------------------------
def test_record_order_and_subsets(ctx, synthetic):
    rng = np.random.default_rng(11)
    shuffled = [SYN_RECORDS[k] for k in rng.permutation(len(SYN_RECORDS))]
    subset = [SYN_RECORDS[k] for k in (14, 9, 3, 0, 11, 7)]
    assert shuffled != SYN_RECORDS
    for records in (shuffled, subset, SYN_RECORDS[::-1]):
        for dtype, layout in (("uint8", "ragged"), ("int64", "padded")):
            got, want, _, _ = run(ctx, synthetic, SYN_LENGTHS, records, spec_of(dtype, layout, "raw"))
            assert np.array_equal(got, want)
    a = run(ctx, synthetic, SYN_LENGTHS, shuffled, spec_of("uint8", "ragged", "raw"))[0]
    b = run(ctx, synthetic, SYN_LENGTHS, SYN_RECORDS, spec_of("uint8", "ragged", "raw"))[0]
    assert np.array_equal(a, b)


# ---- 4. through the finder -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def contigs():
    """A few contigs of the committed fixtures and slices of them down to 61 bp; the last ends in a copy of its first 40 bases."""
    miij, srr, kk = (read_fasta(n + ".fna.gz")[0][1].encode() for n in ("MIIJ01000039", "SRR492066", "KK037166"))
    circle = kk[4000:12000]
    return (srr[:20000], kk[:3073], miij[300000:300061], srr[30000:30400], miij[500000:506145], circle + circle[:40])


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib
    return lib


@pytest.fixture(scope="module")
def bins(lib):
    from pyrodigal_amd import benchdata
    return lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])


def records_of_genes(all_genes):
    return [(i, g.begin, g.end, g.strand, int(g.partial_begin), int(g.partial_end)) for i, genes in enumerate(all_genes) for g in genes]


def covered_bases(records, lengths):
    """Per contig, the number of distinct bases its genes cover: from the records, on the host."""
    sets = [set() for _ in lengths]
    for c, b, e, *_ in records:
        sets[c].update((q - 1) % lengths[c] for q in range(b, e + 1))
    return [len(s) for s in sets]


def device_input(seqs):
    """The sequences as a DeviceSequences [B, Lmax] of uint8 letters."""
    from pyrodigal_amd import DeviceSequences
    rows = np.full((len(seqs), max(map(len, seqs))), ord("N"), np.uint8)
    for i, s in enumerate(seqs):
        rows[i, :len(s)] = np.frombuffer(s, np.uint8)
    return DeviceSequences(keep(hip_mem.DeviceArray.from_numpy(rows)), [len(s) for s in seqs])


def check_finder(finder, given, seqs, trimmed=(), **options):
    """find_labels_batch against the restatement on the Genes it returns; returns (genes, records, lengths)."""
    lengths = [len(s) - (40 if i in trimmed else 0) for i, s in enumerate(seqs)]
    out = {}
    for dtype, layout, classes in (("int64", "padded", "frame"), ("uint8", "ragged", "coding")):
        spec = spec_of(dtype, layout, classes)
        t = Target(DTYPES[dtype], layout, lengths, max(lengths) + 2 if layout == "padded" else None)
        genes, dl = finder.find_labels_batch(given, spec, out=t.out, **options)
        records = records_of_genes(genes)
        assert [len(g.sequence.data) for g in genes] == lengths
        want, off = base_labels_ref(lengths, records, preset_map(classes), layout=layout, pad=spec.pad, width=t.W, dtype=DTYPES[dtype])
        assert dl.lengths.tolist() == lengths and dl.labels is t.out
        assert np.array_equal(t.read(), t.expect(want))
        if classes == "coding":
            flat = t.read()[1:1 + t.n]
            assert [int(np.count_nonzero(flat[off[i]:off[i + 1]])) for i in range(len(lengths))] == covered_bases(records, lengths)
        else:
            rows = t.read()[1:1 + t.n + t.S - t.W].reshape(len(lengths), t.S)
            for i, n in enumerate(lengths):
                assert np.all(rows[i, n:t.W] == spec.pad)                    # the rest of the row is pad
        out[classes] = records
    assert out["frame"] == out["coding"]
    return genes, records, lengths


@pytest.mark.parametrize("source", ["host", "device"])
def test_find_labels_batch(lib, bins, source):
    seqs = list(contigs())
    given = seqs if source == "host" else device_input(seqs)
    finder = lib.GeneFinder(meta=True, metagenomic_bins=bins)
    genes, records, _ = check_finder(finder, given, seqs)
    assert len(records) > 25 and finder.stats["device_calls"] == 2
    want = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_genes_batch(given)
    assert records == records_of_genes(want)                                # the same Genes as find_genes_batch
    with pytest.raises(TypeError, match="BaseLabels"):
        finder.find_labels_batch(given, "frame")


@pytest.mark.parametrize("source", ["host", "device"])
def test_find_labels_batch_on_circles_and_trimmed_records(lib, bins, source):
    seqs = list(contigs())
    finder = lib.GeneFinder(meta=True, metagenomic_bins=bins)
    # the first contig again, turned so that it begins in the middle of its longest gene: as a circle it has a gene across the origin
    longest = max(finder.find_genes_batch(seqs[:1])[0], key=lambda g: g.end - g.begin)
    turn = (longest.begin + longest.end) // 2
    seqs.append(seqs[0][turn:] + seqs[0][:turn])
    given = seqs if source == "host" else device_input(seqs)
    circular = [True, False, False, True, True, False, True]
    genes, records, lengths = check_finder(finder, given, seqs, circular=circular)
    assert [g.circular for g in genes] == circular
    across = [r for r in records if r[2] > lengths[r[0]]]
    assert across and all(circular[r[0]] for r in across)                   # genes with end > seqlen: both ends of the row are painted
    genes, records, lengths = check_finder(finder, given, seqs, trimmed=(5,), trim_terminal_repeats=True)
    assert genes[5].terminal_repeat == 40 and genes[5].circular and lengths[5] == len(seqs[5]) - 40
    assert [g.terminal_repeat for g in genes[:5]] == [0] * 5 and not genes[0].circular


def test_find_labels_batch_with_sets_and_training_infos(lib, bins):
    import gzip
    from tests.util import golden_path
    seqs = list(contigs())
    finder = lib.GeneFinder(meta=True, metagenomic_bins=bins)
    sets = ["a", "b", "a", None, "b", "a"]
    genes, records, _ = check_finder(finder, seqs, seqs, sets=sets)
    want = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_genes_batch(seqs, sets=sets)
    assert records == records_of_genes(want) and [g.metagenomic_bin for g in genes] == [g.metagenomic_bin for g in want]
    assert genes[0].metagenomic_bin is genes[5].metagenomic_bin and genes[0].set_score == want[0].set_score
    blobs = [gzip.open(golden_path(n)).read() for n in ("SRR492066.training.bin.gz", "GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz")]
    tinfs = [lib.TrainingInfo(raw=np.frombuffer(b, np.uint8).copy()) for b in blobs]
    single = lib.GeneFinder()
    genes, records, _ = check_finder(single, seqs, seqs, training_infos=[tinfs[i % 2] for i in range(len(seqs))])
    assert len(records) > 25 and single.stats["device_calls"] == 2          # one device call per request
    small = lib.GeneFinder(coalesce_bases=15000)
    with pytest.raises(ValueError, match="device calls.*find_labels_batch"):
        small.find_labels_batch(seqs, spec_of("int64", "ragged", "frame"), training_infos=[tinfs[i % 2] for i in range(len(seqs))])


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_host_and_leave_the_context_usable(ctx, synthetic):
    from pyrodigal_amd import _cabi
    spec = spec_of("int32", "padded", "raw")
    genes = gene_array(SYN_RECORDS)
    B, W, S = len(SYN_LENGTHS), max(SYN_LENGTHS), max(SYN_LENGTHS) + 2
    need = (B - 1) * S + W
    mem = keep(hip_mem.DeviceArray.from_numpy(np.full(4 * (need + 8), CANARY, np.uint8)))
    len_out = np.zeros(B, np.int64)

    def raw(ptr=mem.ptr, n_out=need, recs=genes, **change):
        o = spec.opts(W, S)
        for k, v in change.items():
            if k == "class_0":
                o.class_map[0] = v
            else:
                setattr(o, k, v)
        rc = ctx.L.pga_label_bases(ctx.h, synthetic.h, len(recs), ctypes.c_void_p(recs.ctypes.data), ctypes.byref(o), ctypes.c_void_p(ptr),
                                   n_out, None, ctypes.c_void_p(len_out.ctypes.data))
        return rc, ctx.L.pga_last_error(ctx.h).decode()

    def changed(k, **fields):
        g = genes.copy()
        for name, v in fields.items():
            g[name][k] = v
        return g

    host = np.zeros(need + 8, np.int32)
    for what, kw, word in (("a host pointer", dict(ptr=host.ctypes.data), "not device memory"),
                           ("out one element too small", dict(n_out=need - 1), "n_out_elems"),
                           ("W below the longest contig", dict(row_width=W - 1), "row_width"),
                           ("a record outside its contig", dict(recs=changed(6, begin=334, end=336)), "gene 6 lies outside"),
                           ("a record longer than its contig", dict(recs=changed(9, begin=1, end=603)), "gene 9 lies outside"),
                           ("a record of another contig", dict(recs=changed(2, contig=4)), "gene 2 names contig 4"),
                           ("e > L on a contig that is not circular", dict(recs=changed(5, begin=650, end=739)), "gene 5 ends beyond"),
                           ("a length that is no multiple of 3", dict(recs=changed(1, end=199)), "gene 1 is 100 bases"),
                           ("elem_bytes 2", dict(elem_bytes=2), "elem_bytes"),
                           ("an id of 256 with uint8", dict(elem_bytes=1, class_0=256), "256"),
                           ("a pointer that is not element-aligned", dict(ptr=mem.ptr + 1), "aligned")):
        rc, msg = raw(**kw)
        assert rc == _cabi.PGA_EINVAL and word in msg, (what, rc, msg)
    with pytest.raises(ValueError, match="not device memory"):
        ctx.label_bases(synthetic, genes, spec, out=View(host.ctypes.data, (B, W), np.int32, (4 * S, 4)))
    with pytest.raises(ValueError, match="columns"):
        ctx.label_bases(synthetic, genes, spec, out=View(mem.ptr, (B, W - 1), np.int32, (4 * S, 4)))
    with pytest.raises(ValueError, match="elements"):
        ctx.label_bases(synthetic, genes, spec_of("int32", "ragged"), out=View(mem.ptr, (sum(SYN_LENGTHS) - 1,), np.int32))
    assert np.all(host == 0) and np.all(mem.to_numpy(np.uint8) == CANARY)           # nothing was written anywhere
    rc, msg = raw()                                                                  # the context runs a good call afterwards
    assert rc == 0, msg
    assert len_out.tolist() == SYN_LENGTHS
    want, _ = base_labels_ref(SYN_LENGTHS, SYN_RECORDS, preset_map("raw"), pad=spec.pad, dtype=np.int32)
    got = mem.to_numpy(np.int32)
    for i in range(B):
        assert np.array_equal(got[i * S:i * S + W], want[i]), i


# ---- 6. history --------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_earlier_calls(ctx, synthetic):
    spec = spec_of("uint8", "ragged", "frame")
    first = run(ctx, synthetic, SYN_LENGTHS, SYN_RECORDS, spec)
    assert np.array_equal(first[0], first[1])
    lengths = [5000, 1234, 0, 9000, 777]
    records = [gene(0, 1 + 97 * k, 30, 1 if k % 3 else -1) for k in range(50)] + [gene(3, 8990, 40, -1)] + \
              [gene(3, 5 + 61 * k, 25, -1 if k % 2 else 1, k % 2, k % 3 == 0) for k in range(140)] + [gene(4, 1, 259, 1)]
    other = keep(ctx.upload([letters(n, 90 + n) for n in lengths]))
    other.set_circular([False, False, False, True, False])
    for dtype, layout in (("int64", "padded"), ("uint8", "ragged")):
        got, want, _, _ = run(ctx, other, lengths, records, spec_of(dtype, layout, "raw"))
        assert np.array_equal(got, want)
    third = run(ctx, synthetic, SYN_LENGTHS, SYN_RECORDS, spec)
    assert np.array_equal(third[0], first[0]) and np.array_equal(third[0], third[1])


# ---- 7. torch --------------------------------------------------------------------------------------------------------------------------
TORCH_SCRIPT = r'''
import sys
import torch                                   # first: the library then binds to the HIP runtime of torch's wheel
if not torch.cuda.is_available():
    print("torch sees no GPU")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
import numpy as np
from pyrodigal_amd import BaseLabels, DeviceLabels, benchdata, lib
from tests.base_labels_ref import base_labels_ref, preset_map

bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])
seqs = [benchdata.synthetic_contig(n, gc, 900 + i) for i, (n, gc) in enumerate(((20000, 0.4), (12345, 0.6), (61, 0.5), (30011, 0.5)))]
lengths = [len(s) for s in seqs]
want_genes = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_genes_batch(seqs)
records = [(i, g.begin, g.end, g.strand, int(g.partial_begin), int(g.partial_end)) for i, genes in enumerate(want_genes) for g in genes]
assert len(records) > 30
side = torch.cuda.Stream()
for layout, dtype in (("ragged", "int32"), ("padded", "int64")):
    spec = BaseLabels("frame", dtype=dtype, layout=layout)
    with torch.cuda.stream(side):
        genes, dl = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_labels_batch(seqs, spec)
    assert isinstance(dl, DeviceLabels) and dl.labels.is_cuda and dl.labels.dtype == getattr(torch, dtype)
    assert dl.labels.device.index == 0 and tuple(dl.labels.shape) == ((len(seqs), max(lengths)) if layout == "padded" else (sum(lengths),))
    assert [[(g.begin, g.end, g.strand) for g in x] for x in genes] == [[(g.begin, g.end, g.strand) for g in x] for x in want_genes]
    want, off = base_labels_ref(lengths, records, preset_map("frame"), layout=layout, pad=-100, dtype=np.dtype(dtype))
    assert np.array_equal(dl.labels.cpu().numpy(), want), "labels differ"
    cu = dl.cu_seqlens()
    assert cu.is_cuda and cu.dtype == torch.int32 and cu.cpu().tolist() == off.tolist()
    view = dl.labels_of[1]
    assert len(dl.labels_of) == len(seqs) and tuple(view.shape) == (lengths[1],)
    assert np.array_equal(view.cpu().numpy(), want[off[1]:off[2]] if layout == "ragged" else want[1, :lengths[1]])
    if layout == "padded":
        assert int((dl.labels == -100).sum()) == len(seqs) * max(lengths) - sum(lengths)
        logits = torch.randn(len(seqs), 8, max(lengths), device=dl.labels.device)
        loss = torch.nn.functional.cross_entropy(logits, dl.labels, ignore_index=-100)
        assert torch.isfinite(loss).item() and loss.item() > 0
print("torch base labels ok: %d genes" % len(records))
'''


def test_torch_tensor_in_a_fresh_process(tmp_path):
    """torch is imported by the child alone (this process holds the library's HIP runtime and gets no second one); `out=None`
    allocates the tensor under torch's current stream.  The child says so when torch sees no GPU, and the test is skipped."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "torch_base_labels.py"
    script.write_text(TORCH_SCRIPT)
    done = subprocess.run([sys.executable, str(script), root], timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, "child ended with %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    if "torch sees no GPU" in done.stdout:
        pytest.skip("torch sees no GPU")
    assert "torch base labels ok" in done.stdout
