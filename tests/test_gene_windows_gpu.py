"""Gene and flanking nucleotide windows left on the device as tokens (pga_gene_windows, GeneWindows, Context.gene_windows,
GeneFinder.find_windows_batch).

Every expected value is an exact integer: the plain-Python restatement of the rule (tests/gene_windows_ref.py) applied to records the
test wrote by hand, or `Gene.sequence()` and slices of the input for records the existing finder path returned -- never the code
under test.  Device memory comes from tests/hip_mem.py (no torch), but for the one torch test, which runs in a child process."""
import ctypes
import functools
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hip_mem
from tests.gene_windows_ref import gene_windows_ref
from tests.util import golden_path, read_fasta

pytestmark = pytest.mark.gpu

DTYPES = {"uint8": np.uint8, "int32": np.int32, "int64": np.int64}
PAD = {"uint8": 250, "int32": -100, "int64": -100}
CANARY = 0xA5
BASE_IDS = {"A": 10, "C": 11, "G": 12, "T": 13, "N": 14}       # and 15 for outside: every class has an id of its own
OUTSIDE = 15
CODONS = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]
CODON_IDS = {c: 100 + k for k, c in enumerate(CODONS)}         # and 164 for a codon with an N, 170 for one that touches outside
CODON_OUTSIDE = 170                                            # (not 165: that is the canary byte)
CODON_IDS["NNN"] = 164


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
    for name, col in zip(("contig", "begin", "end", "strand"), zip(*recs)):
        genes[name] = col
    return genes


def gene(contig, begin, codons, strand):
    return (contig, begin, begin + 3 * codons - 1, strand)


def letters(n, seed):
    """Upper-case, lower-case and IUPAC letters, with a run of five N in the middle and an `n` near either end."""
    s = np.frombuffer(b"ACGTACGTACGTacgtRYKMSWn", np.uint8)[np.random.default_rng(seed).integers(0, 23, size=n)].copy()
    s[n // 2:n // 2 + 5] = ord("N")
    s[2] = s[n - 3] = ord("n")
    return s.tobytes()


# ---- the synthetic batch: 441 bases, written by hand ---------------------------------------------------------------------------------
SYN_LENGTHS = [120, 58, 30, 200, 33]
SYN_CIRCULAR = [False, False, True, True, False]
SYN_SEQS = [letters(n, 60 + i) for i, n in enumerate(SYN_LENGTHS)]
SYN_SEQS[2] = b"GATCAtgcaNNNNNnRYKacgtTGCAGTCA"    # the circle of 30 letter by letter: 29 30 1 2 3 4 read C A G A T C
SYN_RECORDS = [
    gene(0, 10, 20, 1),                          # [10, 69]
    gene(0, 40, 25, -1),                         # [40, 114]: a 40-base flank behind it (to the left) stays inside, in front it does not
    gene(1, 6, 16, 1),                           # [6, 53] of 58: five bases from either end, so 40-base flanks are outside on both sides
    gene(1, 6, 16, -1),                          # the same on the reverse strand
    gene(2, 4, 4, 1),                            # [4, 15] on the circle of 30: a 40-base flank goes round more than once
    gene(2, 4, 4, -1),
    gene(2, 25, 4, 1),                           # [25, 36]: e > L
    gene(2, 29, 2, -1),                          # [29, 34]: its codons are 34 33 32 and 31 30 29, the first across the origin
    gene(2, 29, 2, 1),                           # its first codon is 29 30 1
    gene(3, 10, 10, 1),                          # [10, 39] on the circle of 200: the upstream flank wraps at the left end
    gene(3, 170, 9, -1),                         # [170, 196]: the upstream flank of a reverse gene wraps at the right end
    gene(3, 190, 7, 1),                          # [190, 210]: e > L, and the downstream flank reads on from there
    gene(4, 1, 11, 1),                           # the whole contig
    gene(4, 1, 1, -1),                           # [1, 3]
]
WINDOWS = {
    "body": (("start", 0), ("end", 0)),
    "upstream": (("start", -40), ("start", 0)),
    "downstream": (("end", 0), ("end", 40)),
    "body with flanks": (("start", -40), ("end", 40)),
}


@pytest.fixture(scope="module")
def synthetic(ctx):
    assert sum(SYN_LENGTHS) == 441 and all(r[2] <= SYN_LENGTHS[r[0]] or SYN_CIRCULAR[r[0]] for r in SYN_RECORDS)
    batch = ctx.upload(SYN_SEQS)
    batch.set_circular(SYN_CIRCULAR)
    yield batch
    batch.close()


def spec_of(dtype, layout, window="body", unit="base", **kw):
    from pyrodigal_amd import GeneWindows
    begin, end = WINDOWS[window] if isinstance(window, str) else window
    vocabulary, outside = (BASE_IDS, OUTSIDE) if unit == "base" else (CODON_IDS, CODON_OUTSIDE)
    return GeneWindows(begin, end, unit=unit, vocabulary=vocabulary, outside=outside, pad=PAD[dtype], dtype=dtype, layout=layout, **kw)


def run(ctx, batch, seqs, circular, records, spec, width=None, **kw):
    """One call into a Target: (what the allocation holds, what it must hold, the DeviceWindows, the Target)."""
    want, off, lens = gene_windows_ref(seqs, circular, records, spec.begin, spec.end, spec.token_unit, spec.ids, spec.bos, spec.eos,
                                       spec.max_length, layout=spec.layout, pad=spec.pad, width=width, dtype=DTYPES[spec.dtype])
    t = Target(DTYPES[spec.dtype], spec.layout, lens.tolist(), width, **kw)
    dw = ctx.gene_windows(batch, gene_array(records) if records else gene_array([gene(0, 1, 1, 1)])[:0], spec, out=t.out)
    assert dw.lengths.tolist() == lens.tolist() and dw.lengths.dtype == np.int64 and dw.tokens is t.out
    assert (dw.offsets is None) if spec.layout == "padded" else (dw.offsets.tolist() == off.tolist())
    return t.read(), t.expect(want), dw, t


# ---- 1. strands, windows, linear edges and circles -------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", sorted(WINDOWS))
@pytest.mark.parametrize("layout", ["ragged", "padded"])
@pytest.mark.parametrize("dtype", ["uint8", "int32", "int64"])
def test_synthetic_records(ctx, synthetic, dtype, layout, window):
    got, want, dw, t = run(ctx, synthetic, SYN_SEQS, SYN_CIRCULAR, SYN_RECORDS, spec_of(dtype, layout, window))
    assert t.ptr % 16 == t.eb and t.S == t.W + 5                     # element-aligned only; rows a stride apart
    assert np.array_equal(got, want)                                 # the tokens, and the canary everywhere else
    assert dw.gene_begin.tolist() == [0, 2, 4, 9, 12, 14]
    if layout == "padded" and window == "body with flanks":
        rows = want[1:1 + t.n + t.S - t.W].reshape(len(SYN_RECORDS), t.S)
        for g in (2, 3):                                             # 35 of the 40 flanking bases lie outside, on the left and on the right
            assert np.all(rows[g, :35] == OUTSIDE) and np.all(rows[g, 93:128] == OUTSIDE) and not np.any(rows[g, 35:93] == OUTSIDE)
        circles = rows[[k for k, r in enumerate(SYN_RECORDS) if SYN_CIRCULAR[r[0]]]]
        assert not np.any(circles == OUTSIDE) and np.any(rows == BASE_IDS["N"])
        # the circle of 30: bases 31 .. 40 of the upstream flank are bases 1 .. 10 of it again
        assert np.array_equal(rows[4, :10], rows[4, 30:40]) and rows[4, 40 + 12 + 39] == rows[4, 40 + 12 + 9]


# ---- 2. row lengths around the piece size, empty rows, one gene, none --------------------------------------------------------------------
@pytest.mark.parametrize("dtype, tokens", [("uint8", 15), ("uint8", 16), ("uint8", 17), ("int32", 3), ("int32", 4), ("int32", 5),
                                           ("int64", 1), ("int64", 2), ("int64", 3)])
def test_rows_around_the_piece_size(ctx, synthetic, dtype, tokens):
    for layout in ("ragged", "padded"):
        for extra_stride in (0, 5):
            spec = spec_of(dtype, layout, (("start", -2), ("start", tokens - 2)))
            got, want, _, t = run(ctx, synthetic, SYN_SEQS, SYN_CIRCULAR, SYN_RECORDS, spec, extra_stride=extra_stride)
            assert t.W == tokens and np.array_equal(got, want), (layout, extra_stride)


EMPTY_FIRST_LAST_AND_TWICE = [SYN_RECORDS[k] for k in (4, 0, 8, 5, 1, 2, 13)]          # n = 12, 60, 6, 12, 75, 48, 3
SHAPES = {
    "empty rows first, last and two in a row": (EMPTY_FIRST_LAST_AND_TWICE, (("start", 30), ("end", 0))),
    "every row empty": (EMPTY_FIRST_LAST_AND_TWICE, (("end", 0), ("start", 0))),
    "a single gene": ([SYN_RECORDS[7]], (("start", -3), ("end", 2))),
    "a single gene without bases": ([SYN_RECORDS[13]], (("start", 3), ("end", 0))),
    "no genes": ([], (("start", 0), ("end", 0))),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("layout", ["ragged", "padded"])
@pytest.mark.parametrize("dtype", ["uint8", "int32", "int64"])
def test_smallest_shapes(ctx, synthetic, dtype, layout, shape):
    records, window = SHAPES[shape]
    got, want, dw, t = run(ctx, synthetic, SYN_SEQS, SYN_CIRCULAR, records, spec_of(dtype, layout, window))
    assert np.array_equal(got, want)
    if shape.startswith("empty rows"):
        assert dw.lengths.tolist() == [0, 30, 0, 0, 45, 18, 0]
    if shape == "every row empty" and layout == "padded":
        assert t.W == 0 and t.n == 6 * t.S                           # rows of no columns: nothing at all is written


# ---- 3. special tokens, max_length, codons ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["ragged", "padded"])
@pytest.mark.parametrize("dtype", ["uint8", "int32", "int64"])
def test_special_tokens_and_max_length(ctx, synthetic, dtype, layout):
    for kw in (dict(bos=1), dict(eos=2), dict(bos=1, eos=2), dict(bos=1, eos=2, max_length=20), dict(max_length=16)):
        for window in ("body", (("start", 30), ("end", 0))):           # the second: rows of the specials alone
            got, want, dw, _ = run(ctx, synthetic, SYN_SEQS, SYN_CIRCULAR, SYN_RECORDS, spec_of(dtype, layout, window, **kw))
            assert np.array_equal(got, want), (kw, window)
            if "max_length" in kw and window == "body":
                specials = ("bos" in kw) + ("eos" in kw)
                assert dw.lengths.max() == kw["max_length"] and dw.lengths.min() == 3 + specials       # the cut rows, and [1, 3] whole


@pytest.mark.parametrize("layout", ["ragged", "padded"])
@pytest.mark.parametrize("dtype", ["uint8", "int32", "int64"])
def test_codon_tokens(ctx, synthetic, dtype, layout):
    for window, kw in (("body", {}), ((("start", -6), ("end", 6)), {}), ((("start", -42), ("start", 3)), dict(bos=1, eos=2, max_length=12))):
        got, want, dw, t = run(ctx, synthetic, SYN_SEQS, SYN_CIRCULAR, SYN_RECORDS, spec_of(dtype, layout, window, unit="codon", **kw))
        assert np.array_equal(got, want), window
        if window == "body":
            assert dw.lengths.tolist() == [(r[2] - r[1] + 1) // 3 for r in SYN_RECORDS]
            assert 164 in want and CODON_OUTSIDE not in want                   # a codon with an N; nothing of a body is outside
        elif not kw:
            assert 164 in want and CODON_OUTSIDE in want                       # the second codon behind [6, 53] of 58 touches the end of the contig
    # the codons across the origin of the circle of 30, by hand: CAG ATC forward, and GAT CTG on the reverse strand
    got, want, _, t = run(ctx, synthetic, SYN_SEQS, SYN_CIRCULAR, SYN_RECORDS[7:9], spec_of(dtype, "ragged", "body", unit="codon"))
    assert got[1:5].tolist() == [CODON_IDS[c] for c in ("GAT", "CTG", "CAG", "ATC")]


# ---- 4. any subset or order of the records ---------------------------------------------------------------------------------------------
def test_record_order_and_subsets(ctx, synthetic):
    rng = np.random.default_rng(11)
    shuffled = [SYN_RECORDS[k] for k in rng.permutation(len(SYN_RECORDS))]
    assert [r[0] for r in shuffled] != sorted(r[0] for r in shuffled)
    for dtype, layout in (("uint8", "ragged"), ("int64", "padded")):
        got, want, dw, _ = run(ctx, synthetic, SYN_SEQS, SYN_CIRCULAR, shuffled, spec_of(dtype, layout, "body with flanks"))
        assert np.array_equal(got, want) and dw.gene_begin is None
        with pytest.raises(ValueError, match="contig order"):
            dw.windows
        got, want, dw, _ = run(ctx, synthetic, SYN_SEQS, SYN_CIRCULAR, SYN_RECORDS[9:3:-2] * 2, spec_of(dtype, layout, "upstream"))
        assert np.array_equal(got, want)
    with pytest.raises(TypeError, match="GeneWindows"):
        ctx.gene_windows(synthetic, gene_array(SYN_RECORDS), "body")


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_host_and_leave_the_context_usable(ctx, synthetic):
    from pyrodigal_amd import _cabi
    spec = spec_of("int32", "padded", "body with flanks", bos=1)
    genes = gene_array(SYN_RECORDS)
    lens = [r[2] - r[1] + 1 + 81 for r in SYN_RECORDS]
    G, W, S = len(SYN_RECORDS), max(lens), max(lens) + 2
    need = (G - 1) * S + W
    mem = keep(hip_mem.DeviceArray.from_numpy(np.full(4 * (need + 8), CANARY, np.uint8)))
    len_out = np.zeros(G, np.int64)

    def raw(ptr=mem.ptr, n_out=need, recs=genes, **change):
        o = spec.opts(W, S)
        for k, v in change.items():
            if k == "id_0":
                o.ids[0] = v
            else:
                setattr(o, k, v)
        rc = ctx.L.pga_gene_windows(ctx.h, synthetic.h, len(recs), ctypes.c_void_p(recs.ctypes.data), ctypes.byref(o), ctypes.c_void_p(ptr),
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
                           ("W below the longest row", dict(row_width=W - 1), "row_width = %d is less than the %d tokens of gene 1" % (W - 1, W)),
                           ("a record outside its contig", dict(recs=changed(2, begin=59, end=61)), "gene 2 lies outside"),
                           ("a record longer than its contig", dict(recs=changed(6, begin=1, end=33)), "gene 6 lies outside"),
                           ("a record of another contig", dict(recs=changed(3, contig=5)), "gene 3 names contig 5"),
                           ("e > L on a contig that is not circular", dict(recs=changed(1, begin=100, end=129)), "gene 1 ends beyond"),
                           ("a length that is no multiple of 3", dict(recs=changed(0, end=70)), "gene 0 is 61 bases"),
                           ("elem_bytes 2", dict(elem_bytes=2), "elem_bytes"),
                           ("an id beyond int32", dict(id_0=1 << 31), "ids[0]"),
                           ("a delta beyond 2^30", dict(from_delta=-(1 << 30) - 1), "from_delta"),
                           ("a codon window off the codons", dict(unit=_cabi.WINDOW_CODONS, from_delta=-42, to_delta=40), "to_delta = 40 is no multiple of 3"),
                           ("an anchor that is none", dict(to_anchor=2), "to_anchor"),
                           ("a unit that is none", dict(unit=2), "unit"),
                           ("max_length without room", dict(max_length=1), "max_length"),
                           ("a pointer that is not element-aligned", dict(ptr=mem.ptr + 1), "aligned")):
        rc, msg = raw(**kw)
        assert rc == _cabi.PGA_EINVAL and word in msg and msg.startswith("pga_gene_windows: "), (what, rc, msg)
    with pytest.raises(ValueError, match="not device memory"):
        ctx.gene_windows(synthetic, genes, spec, out=View(host.ctypes.data, (G, W), np.int32, (4 * S, 4)))
    with pytest.raises(ValueError, match="columns"):
        ctx.gene_windows(synthetic, genes, spec, out=View(mem.ptr, (G, W - 1), np.int32, (4 * S, 4)))
    with pytest.raises(ValueError, match="elements"):
        ctx.gene_windows(synthetic, genes, spec_of("int32", "ragged", "body"), out=View(mem.ptr, (sum(lens) - 81 * G - 1,), np.int32))
    assert np.all(host == 0) and np.all(mem.to_numpy(np.uint8) == CANARY)           # nothing was written anywhere
    rc, msg = raw()                                                                  # the context runs a good call afterwards
    assert rc == 0, msg
    assert len_out.tolist() == lens
    want, _, _ = gene_windows_ref(SYN_SEQS, SYN_CIRCULAR, SYN_RECORDS, spec.begin, spec.end, "base", spec.ids, bos=1, pad=spec.pad, dtype=np.int32)
    got = mem.to_numpy(np.int32)
    for g in range(G):
        assert np.array_equal(got[g * S:g * S + W], want[g]), g


# ---- 6. history --------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_earlier_calls(ctx, synthetic):
    spec = spec_of("uint8", "ragged", "body with flanks")
    first = run(ctx, synthetic, SYN_SEQS, SYN_CIRCULAR, SYN_RECORDS, spec)
    assert np.array_equal(first[0], first[1])
    seqs = [letters(n, 90 + n) for n in (5000, 1234, 9000)]
    records = [gene(0, 1 + 97 * k, 30, 1 if k % 3 else -1) for k in range(50)] + [gene(2, 8990, 40, -1)] + \
              [gene(2, 5 + 61 * k, 25, -1 if k % 2 else 1) for k in range(140)]
    other = keep(ctx.upload(seqs))
    other.set_circular([False, False, True])
    for dtype, layout in (("int64", "padded"), ("uint8", "ragged")):
        got, want, _, _ = run(ctx, other, seqs, [False, False, True], records, spec_of(dtype, layout, (("start", -60), ("start", 30))))
        assert np.array_equal(got, want)
    third = run(ctx, synthetic, SYN_SEQS, SYN_CIRCULAR, SYN_RECORDS, spec)
    assert np.array_equal(third[0], first[0]) and np.array_equal(third[0], third[1])


# ---- 7. through the finder -------------------------------------------------------------------------------------------------------------
GENOME = "GCF_001457455.1_NCTC11397_genomic_100kb"
LETTER_OF = {v: k for k, v in BASE_IDS.items()}
LETTER_OF[OUTSIDE] = "-"
COMPLEMENT = str.maketrans("ACGTN-", "TGCAN-")


@functools.lru_cache(maxsize=None)
def genome():
    return read_fasta(GENOME + ".fna.gz")[0][1].encode("ascii")


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib
    return lib


@pytest.fixture(scope="module")
def closed_model(lib):
    blob = gzip.open(golden_path(GENOME + ".tinf_closed.bin.gz")).read()
    return lib.TrainingInfo(raw=np.frombuffer(blob, np.uint8).copy())


def records_of_genes(all_genes):
    return [(i, g.begin, g.end, g.strand, int(g.partial_begin), int(g.partial_end)) for i, genes in enumerate(all_genes) for g in genes]


def context_by_slicing(seq, circular, g, before, after):
    """`before` bases in front of the gene's first base and `after` from it on, in reading direction: slices of the input, turned and
    complemented in Python; `-` beyond the ends of a linear contig, the contig laid out three times where it is a circle."""
    L = len(seq)
    assert before <= L and after <= L
    laid = (seq * 3 if circular else b"-" * L + seq + b"-" * L).decode().upper()
    laid = "".join(ch if ch in "ACGT-" else "N" for ch in laid)
    if g.strand == 1:
        at = L + g.begin - 1                                         # the gene's first base in `laid`
        return laid[at - before:at + after]
    at = L + (g.end - 1) % L if circular else L + g.end - 1
    return laid[at - after + 1:at + before + 1].translate(COMPLEMENT)[::-1]


def rows_as_letters(flat, lens):
    off = np.concatenate([[0], np.cumsum(lens)])
    return ["".join(LETTER_OF[v] for v in flat[off[g]:off[g + 1]].tolist()) for g in range(len(lens))]


def check_finder(finder, given, seqs, circles=None, lengths=None, **options):
    """find_windows_batch against Gene.sequence() (the body) and slices of the input (the start context) on the Genes it returns."""
    lengths = [len(s) for s in seqs] if lengths is None else lengths
    circles = [False] * len(seqs) if circles is None else circles
    found = {}
    for window, dtype in (("body", "uint8"), ((("start", -60), ("start", 30)), "int64")):
        spec = spec_of(dtype, "ragged", window)
        probe = finder.find_genes_batch(given, **options)
        lens = spec.lengths(gene_array([r[:4] for r in records_of_genes(probe)]))
        t = Target(DTYPES[dtype], "ragged", lens.tolist())
        genes, dw = finder.find_windows_batch(given, spec, out=t.out, **options)
        assert records_of_genes(genes) == records_of_genes(probe)               # the same Genes as find_genes_batch
        assert [len(g.sequence.data) for g in genes] == lengths and dw.lengths.tolist() == lens.tolist() and dw.tokens is t.out
        assert dw.gene_begin.tolist() == np.concatenate([[0], np.cumsum([len(g) for g in genes])]).tolist()
        got = t.read()
        assert np.all(got[:1].view(np.uint8) == CANARY) and np.all(got[1 + t.n:].view(np.uint8) == CANARY)
        rows = rows_as_letters(got[1:1 + t.n], lens)
        flat_genes = [(i, g) for i, x in enumerate(genes) for g in x]
        if window == "body":
            assert rows == [g.sequence() for _, g in flat_genes]
        else:
            assert rows == [context_by_slicing(genes[i].sequence.data, circles[i], g, 60, 30) for i, g in flat_genes]
        found[dtype] = genes
    return found["uint8"]


def test_find_windows_batch_on_the_genome(lib, closed_model):
    finder = lib.GeneFinder(closed_model, closed=True)
    genes = check_finder(finder, [genome()], [genome()])
    assert len(genes[0]) > 80 and {g.strand for g in genes[0]} == {1, -1}
    assert finder.stats["device_calls"] == 4
    with pytest.raises(TypeError, match="GeneWindows"):
        finder.find_windows_batch([genome()], "body")


def test_find_windows_batch_on_circles_trimmed_records_and_device_input(lib, closed_model):
    from pyrodigal_amd import DeviceSequences
    g = genome()
    circle = g[4000:12000]
    seqs = [g[20000:26000], circle + circle[:40], g[50000:50200].lower() + b"NNNNNNRYK" + g[50200:53000]]
    finder = lib.GeneFinder(closed_model, closed=True)
    # every contig a circle: windows wrap at the origin, and a gene across it reads on
    genes = check_finder(finder, seqs, seqs, circles=[True] * 3, circular=True)
    assert all(x.circular for x in genes)
    # a hand-made direct repeat: the record is called without it, as a circle, and its rows are in trimmed coordinates
    lengths = [len(seqs[0]), len(seqs[1]) - 40, len(seqs[2])]
    genes = check_finder(finder, seqs, seqs, circles=[False, True, False], lengths=lengths, trim_terminal_repeats=True)
    assert genes[1].terminal_repeat == 40 and genes[1].circular and not genes[0].circular
    # the input as a device tensor
    rows = np.full((len(seqs), max(map(len, seqs))), ord("N"), np.uint8)
    for i, s in enumerate(seqs):
        rows[i, :len(s)] = np.frombuffer(s, np.uint8)
    given = DeviceSequences(keep(hip_mem.DeviceArray.from_numpy(rows)), [len(s) for s in seqs])
    check_finder(finder, given, seqs)


def test_find_windows_batch_refuses_a_request_that_splits(lib, closed_model):
    blob = gzip.open(golden_path("SRR492066.training.bin.gz")).read()
    tinfs = [closed_model, lib.TrainingInfo(raw=np.frombuffer(blob, np.uint8).copy())]
    seqs = [genome()[k * 9000:k * 9000 + 8000] for k in range(4)]
    small = lib.GeneFinder(coalesce_bases=15000)
    with pytest.raises(ValueError, match="device calls.*find_windows_batch"):
        small.find_windows_batch(seqs, spec_of("int64", "ragged", "body"), training_infos=[tinfs[i % 2] for i in range(len(seqs))])


# ---- 8. torch --------------------------------------------------------------------------------------------------------------------------
TORCH_SCRIPT = r'''
import sys
import torch                                   # first: the library then binds to the HIP runtime of torch's wheel
if not torch.cuda.is_available():
    print("torch sees no GPU")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
import numpy as np
from pyrodigal_amd import GeneWindows, DeviceWindows, benchdata, lib

bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])
seqs = [benchdata.synthetic_contig(n, gc, 900 + i) for i, (n, gc) in enumerate(((20000, 0.4), (12345, 0.6), (61, 0.5), (30011, 0.5)))]
want_genes = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_genes_batch(seqs)
flat = [g for genes in want_genes for g in genes]
assert len(flat) > 30
side = torch.cuda.Stream()
for layout, dtype in (("ragged", "int32"), ("padded", "int64")):
    spec = GeneWindows(bos=5, pad=-100 if layout == "padded" else None, dtype=dtype, layout=layout)
    with torch.cuda.stream(side):
        genes, dw = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_windows_batch(seqs, spec)
    assert isinstance(dw, DeviceWindows) and dw.tokens.is_cuda and dw.tokens.dtype == getattr(torch, dtype) and dw.tokens.device.index == 0
    assert [[(g.begin, g.end, g.strand) for g in x] for x in genes] == [[(g.begin, g.end, g.strand) for g in x] for x in want_genes]
    lens = [1 + g.end - g.begin + 1 for g in flat]
    assert dw.lengths.tolist() == lens
    assert tuple(dw.tokens.shape) == ((len(flat), max(lens)) if layout == "padded" else (sum(lens),))
    host = dw.tokens.cpu().numpy()
    rows = [host[k, :lens[k]] for k in range(len(flat))] if layout == "padded" else np.split(host, np.cumsum(lens)[:-1])
    for g, row in zip(flat, rows):
        assert row[0] == 5 and "".join("ACGTN"[v] for v in row[1:].tolist()) == g.sequence(), "tokens differ"
    cu = dw.cu_seqlens()
    assert cu.is_cuda and cu.dtype == torch.int32 and cu.cpu().tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    assert len(dw.windows) == len(seqs) and dw.gene_begin.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in genes])]).tolist()
    a, b = int(dw.gene_begin[1]), int(dw.gene_begin[2])
    view = dw.windows[1]
    if layout == "padded":
        assert tuple(view.shape) == (b - a, max(lens)) and view.data_ptr() == dw.tokens[a].data_ptr()
        assert int((dw.tokens == -100).sum()) == len(flat) * max(lens) - sum(lens)
    else:
        assert tuple(view.shape) == (sum(lens[a:b]),) and view.data_ptr() == dw.tokens[int(dw.offsets[a]):].data_ptr()
print("torch gene windows ok: %d genes" % len(flat))
'''


def test_torch_tensor_in_a_fresh_process(tmp_path):
    """torch is imported by the child alone (this process holds the library's HIP runtime and gets no second one); `out=None`
    allocates the tensor under torch's current stream.  The child says so when torch sees no GPU, and the test is skipped."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "torch_gene_windows.py"
    script.write_text(TORCH_SCRIPT)
    done = subprocess.run([sys.executable, str(script), root], timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, "child ended with %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    if "torch sees no GPU" in done.stdout:
        pytest.skip("torch sees no GPU")
    assert "torch gene windows ok" in done.stdout
