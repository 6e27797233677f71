"""K-mers and codons of contigs and genes counted on the device (pga_count_kmers, KmerCounts, Context.kmer_counts,
GeneFinder.find_counts_batch).

Every expected value is an exact integer: the plain-Python restatement of the rule (tests/kmer_counts_ref.py) applied to letters and
records the test wrote by hand, or a count of the codons of `Gene.sequence()` for records the existing finder path returned -- never
the code under test.  Device memory comes from tests/hip_mem.py (no torch), but for the one torch test, which runs in a child
process."""
import collections
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hip_mem
from tests.kmer_counts_ref import kmer, kmer_counts_ref
from tests.util import read_fasta

pytestmark = pytest.mark.gpu

CANARY = 0xA5
CANARY32 = int(np.full(4, CANARY, np.uint8).view(np.int32)[0])


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi, benchdata
    c = _cabi.Context(0)
    c.set_models([b for _, b in benchdata.load_model_set()])
    yield c
    c.close()


@pytest.fixture(scope="module")
def P():
    from pyrodigal_amd import _cabi
    p = int(_cabi.load().pga_kmer_counts_chunk())
    assert p >= 64
    return p


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

    def __init__(self, ptr, shape, strides=None, typestr="<i4"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}


class Target:
    """An allocation full of a fill byte and an int32 tensor [R, n_bins], rows S = n_bins + extra_stride apart, that starts ONE
    element into it (4-byte aligned, nothing more), with `slack` elements behind: `expect()` is what the whole allocation must hold
    after a call."""

    def __init__(self, R, n_bins, extra_stride=3, slack=40, fill=CANARY):
        self.R, self.W, self.S = R, n_bins, n_bins + extra_stride
        self.n = (R - 1) * self.S + self.W if R else 0
        self.before = np.full(4 * (1 + self.n + slack), fill, np.uint8)
        self.mem = keep(hip_mem.DeviceArray.from_numpy(self.before))
        self.ptr = self.mem.ptr + 4
        self.out = View(self.ptr, (R, self.W), (4 * self.S, 4))

    def read(self):
        return self.mem.to_numpy(np.int32)

    def expect(self, want):
        e = self.before.view(np.int32).copy()
        for r in range(self.R):
            e[1 + r * self.S:1 + r * self.S + self.W] = want[r]
        return e


def gene_array(recs):
    from pyrodigal_amd import _cabi
    genes = np.zeros(len(recs), _cabi.GENE_DTYPE)
    if recs:
        for name, col in zip(("contig", "begin", "end", "strand"), zip(*recs)):
            genes[name] = col
    return genes


def letters(n, seed):
    return np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(seed).integers(0, 4, size=n)].copy()


def run(ctx, batch, seqs, circular, records, spec, **kw):
    """One call into a Target: (what the allocation holds, what it must hold, the DeviceCounts, the Target)."""
    want, windows = kmer_counts_ref(seqs, circular, records, spec.k, spec.rows, spec.step, spec.table, spec.n_bins)
    t = Target(len(want), spec.n_bins, **kw)
    dc = ctx.kmer_counts(batch, gene_array(records), spec, out=t.out)
    assert dc.counts is t.out and dc.windows.dtype == np.int64 and dc.windows.tolist() == windows.tolist()
    assert t.ptr % 16 == 4
    return t.read(), t.expect(want), dc, t


# ---- 1. contig rows around the piece size ------------------------------------------------------------------------------------------------
def seam_contig(n, k, P, seed):
    """`n` letters with lower case at P - k .. P + k, an `n` just in front of the seam and an IUPAC letter just behind it, so that
    windows with an N straddle the seam between two pieces, and others with lower-case letters do."""
    s = letters(n, seed)
    lo, hi = max(P - k, 0), min(P + k + 1, n)
    s[lo:hi] |= 0x20
    for at, ch in ((P - 1, "n"), (P + k - 2, "R"), (2 * P, "N")):
        if 0 <= at < n:
            s[at] = ord(ch)
    return s.tobytes()


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_contig_rows(ctx, P, k, canonical):
    from pyrodigal_amd import KmerCounts
    lengths = [1, k - 1, k, k + 1, P - 1, P, P + 1, P + k - 2, P + k - 1, 2 * P, 2 * P + 1]
    seqs = [seam_contig(n, k, P, 100 * k + i) for i, n in enumerate(lengths)] * 2 + [b"N" * (P + 5), b"n" * 7 + b"ACGTAC", b"ACGTACGTAC"]
    circular = [False] * len(lengths) + [True] * len(lengths) + [False, True, True]
    batch = keep(ctx.upload(seqs))
    batch.set_circular(circular)
    spec = KmerCounts(k, canonical=canonical)
    got, want, dc, t = run(ctx, batch, seqs, circular, [], spec)
    assert np.array_equal(got, want)                                 # the counts, and the canary everywhere else
    n = len(lengths)
    assert dc.windows[:n].tolist() == [max(x - k + 1, 0) for x in lengths]
    assert dc.windows[n:2 * n].tolist() == [x if x >= k else 0 for x in lengths]          # circles: L < k none, L = k all L
    rows = want[1:1 + t.n + 3].reshape(-1, t.S)[:, :t.W]
    assert not rows[2 * n].any() and rows[5].sum() < dc.windows[5]                        # all N; windows lost to the N at the seam
    assert rows[n + 2].sum() == k and rows[-1].sum() == 10                                # L = k on a circle: every rotation
    assert dc.gene_begin is None and len(dc.counts_of) == len(seqs)
    # the same without records at all, and into a tensor without strides whose rows are wider than the bins
    wide = keep(hip_mem.DeviceArray.from_numpy(np.full(4 * len(seqs) * (spec.n_bins + 2), CANARY, np.uint8)))
    ctx.kmer_counts(batch, None, spec, out=View(wide.ptr, (len(seqs), spec.n_bins + 2)))
    full = wide.to_numpy(np.int32).reshape(len(seqs), spec.n_bins + 2)
    assert np.array_equal(full[:, :spec.n_bins], rows) and np.all(full[:, spec.n_bins:] == CANARY32)


# ---- 2. gene rows: hand-written records ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gene_batch(P):
    """A long linear contig, a long circle, the circle of 30 written letter by letter, and a contig no record names."""
    big = letters(6 * P + 200, 7)
    big[1000:1003] = np.frombuffer(b"nRy", np.uint8)
    big[3 * P - 2:3 * P + 4] |= 0x20
    big[3 * P] = ord("N")
    circle = letters(3 * P + 61, 8)
    circle[5] = circle[-4] = ord("n")
    seqs = [big.tobytes(), circle.tobytes(), b"GATCAtgcaNNNNNnRYKacgtTGCAGTCA", letters(50, 9).tobytes()]
    return seqs, [False, True, True, False]


def gene_records(P, k, step):
    """(contig, begin, end, strand): the smallest genes, genes whose windows end around one and two pieces, records across the origin
    of a circle on both strands, then a duplicate and an order that is not the contigs'."""
    seqs, _ = gene_batch(P)
    L1 = len(seqs[1])
    recs = [(0, 1, 3, 1), (0, 4, 6, -1), (0, 10, 15, 1), (0, 10, 15, -1), (0, 7, 7 + 3 * k - 1, -1)]          # n = 3, 6, 3 k: n < k, n = k
    for i, nw in enumerate((P - 1, P, P + 1, 2 * P, 2 * P + 1)):
        if step == 3:
            n = 3 * (nw + (k + 2) // 3 - 1)                          # (n - k) // 3 + 1 == nw
        else:
            n = 3 * ((nw + k - 1 + 2) // 3)                          # the multiple of 3 at or above nw + k - 1
        begin = 1 + 7 * i + (i % 2)
        recs.append((0, begin, begin + n - 1, 1 if i % 2 else -1))
        recs.append((0, begin + 40, begin + 40 + n - 1, -1 if i % 2 else 1))
    recs += [(1, L1 - 50, L1 - 50 + 3 * (P // 3 + 40) - 1, 1), (1, L1 - 8, L1 - 8 + 3 * P - 1, -1), (1, L1, L1 + 2, 1), (1, L1 - 1, L1 + 4, -1),
             (2, 4, 15, 1), (2, 4, 15, -1), (2, 25, 36, 1), (2, 29, 34, -1), (2, 29, 34, 1), (2, 1, 30, -1)]
    assert all(r[2] - r[1] + 1 <= len(seqs[r[0]]) and (r[2] - r[1] + 1) % 3 == 0 for r in recs)
    order = np.random.default_rng(k + step).permutation(len(recs))
    return recs, [recs[j] for j in order] + [recs[6], recs[-4]]


def custom_table(k):
    """Every third code dropped, the rest onto 5 bins."""
    return [-1 if x % 3 == 1 else (x * 7) % 5 for x in range(4 ** k)]


@pytest.mark.parametrize("k, step, bins", [(3, 3, None), (3, 3, "amino"), (6, 3, None), (6, 3, "canonical"), (4, 1, "canonical"), (1, 1, None),
                                           (6, 1, None), (2, 3, "custom"), (5, 1, "custom"), (5, 3, None)])
def test_gene_rows_and_their_sums(ctx, P, k, step, bins):
    from pyrodigal_amd import KmerCounts
    seqs, circular = gene_batch(P)
    batch = keep(ctx.upload(seqs))
    batch.set_circular(circular)
    kw = dict(bins=KmerCounts.codon_bins(4)) if bins == "amino" else dict(bins=custom_table(k)) if bins == "custom" else dict(canonical=bins == "canonical")
    ordered, shuffled = gene_records(P, k, step)
    per_gene = None
    for rows in ("gene", "contig_genes"):
        spec = KmerCounts(k, rows=rows, step=step, **kw)
        got, want, dc, t = run(ctx, batch, seqs, circular, ordered, spec)
        assert np.array_equal(got, want), rows
        grid = want[1:1 + t.n + 3].reshape(-1, t.S)[:, :t.W].astype(np.int64)
        if rows == "gene":
            per_gene = grid
            assert dc.gene_begin.tolist() == [0, 15, 19, 25, 25] and not (k > 3 and (dc.windows[0] or grid[0].any()))      # n = 3 < k
            assert step != 3 or {int(w) for w in dc.windows[5:15]} == {P - 1, P, P + 1, 2 * P, 2 * P + 1}
            assert len(dc.counts_of) == 4
        else:
            sums = np.zeros_like(grid)
            for g, r in enumerate(ordered):
                sums[r[0]] += per_gene[g]
            assert np.array_equal(grid, sums) and not grid[3].any() and grid[:3].any(axis=1).all()        # a contig without records: zeros
            assert len(dc.counts_of) == 4 and dc.gene_begin is None
        got, want, dc, _ = run(ctx, batch, seqs, circular, shuffled, spec)                                  # any order, a record twice
        assert np.array_equal(got, want), rows
        if rows == "gene":
            assert dc.gene_begin is None
            with pytest.raises(ValueError, match="contig order"):
                dc.counts_of


def test_the_codons_across_the_origin_by_hand(ctx, P):
    from pyrodigal_amd import KmerCounts
    seqs, circular = gene_batch(P)
    batch = keep(ctx.upload(seqs))
    batch.set_circular(circular)
    spec = KmerCounts(3, rows="gene", step=3)
    got, want, _, t = run(ctx, batch, seqs, circular, [(2, 29, 34, -1), (2, 29, 34, 1)], spec, extra_stride=0)
    assert np.array_equal(got, want)
    rows = got[1:1 + 128].reshape(2, 64)
    named = lambda row: sorted(kmer(x, 3) for x in np.flatnonzero(row) for _ in range(row[x]))          # noqa: E731
    assert named(rows[0]) == ["CTG", "GAT"] and named(rows[1]) == ["ATC", "CAG"]                         # as the windows test reads them


def test_both_forms_of_the_kernel_give_the_same_counts(ctx, P, monkeypatch):
    """Few windows under many bins with shared rows takes the form without a histogram by itself, and short pieces go to a wave each
    where four histograms fit; every form can be forced (where they do not fit, a forced wave form stays with the workgroup)."""
    from pyrodigal_amd import KmerCounts
    seqs, circular = gene_batch(P)
    batch = keep(ctx.upload(seqs))
    batch.set_circular(circular)
    small = [(0, 1 + 30 * i, 30 * i + 3 * (20 + i), 1 if i % 3 else -1) for i in range(40)] + [(2, 25, 36, 1), (2, 29, 34, -1), (1, len(seqs[1]) - 1, len(seqs[1]) + 4, -1)]
    ordered, _ = gene_records(P, 6, 3)
    for form in (None, "lds-group", "lds-wave", "direct-group", "direct-wave"):
        if form is None:
            monkeypatch.delenv("PGA_KMER_COUNTS_FORM", raising=False)
        else:
            monkeypatch.setenv("PGA_KMER_COUNTS_FORM", form)
        for spec, records in ((KmerCounts(6, rows="contig_genes", step=3), small), (KmerCounts(6, rows="contig_genes", step=3, canonical=True), ordered),
                              (KmerCounts(3, rows="gene", step=3), ordered), (KmerCounts(4, canonical=True), [])):
            got, want, _, _ = run(ctx, batch, seqs, circular, records, spec)
            assert np.array_equal(got, want), (form, spec)


# ---- 3. output discipline ------------------------------------------------------------------------------------------------------------------
def test_no_rows_and_two_rules_into_one_tensor(ctx, P):
    from pyrodigal_amd import KmerCounts
    seqs, circular = gene_batch(P)
    batch = keep(ctx.upload(seqs))
    batch.set_circular(circular)
    got, want, dc, t = run(ctx, batch, seqs, circular, [], KmerCounts(3, rows="gene", step=3))            # R = 0
    assert t.R == 0 and np.array_equal(got, want) and dc.windows.shape == (0,) and dc.gene_begin.tolist() == [0] * 5
    ordered, _ = gene_records(P, 3, 3)
    a, b = KmerCounts(3, rows="gene", step=3), KmerCounts(3, rows="gene", step=1, bins=[x % 64 if x % 5 else -1 for x in range(64)])
    t = Target(len(ordered), 64)
    for spec in (a, b, a):                                                                              # set, never added to
        want, _ = kmer_counts_ref(seqs, circular, ordered, spec.k, spec.rows, spec.step, spec.table, spec.n_bins)
        ctx.kmer_counts(batch, gene_array(ordered), spec, out=t.out)
        assert np.array_equal(t.read(), t.expect(want))
    for fill in (0x00, 0xFF):                                                                           # whatever the tensor held before
        t = Target(4, 136, fill=fill)
        spec = KmerCounts(4, canonical=True)
        want, _ = kmer_counts_ref(seqs, circular, [], 4, "contig", 1, spec.table, 136)
        ctx.kmer_counts(batch, None, spec, out=t.out)
        assert np.array_equal(t.read(), t.expect(want))


def test_result_does_not_depend_on_what_memory_held(ctx, P):
    from pyrodigal_amd import KmerCounts
    seqs, circular = gene_batch(P)
    ordered, _ = gene_records(P, 6, 3)
    first = None
    for poison in (None, 0xFF, 0x00, None):
        ctx.debug_poison(poison)
        try:
            batch = keep(ctx.upload(seqs))
            batch.set_circular(circular)
            for spec in (KmerCounts(6, rows="contig_genes", step=3), KmerCounts(5, canonical=True)):
                got, want, _, _ = run(ctx, batch, seqs, circular, ordered, spec)
                assert np.array_equal(got, want), poison
        finally:
            ctx.debug_poison(None)
        first = got if first is None else first
        assert np.array_equal(got, first)


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_host_and_leave_the_context_usable(ctx, P):
    from pyrodigal_amd import KmerCounts, _cabi
    seqs, circular = gene_batch(P)
    batch = keep(ctx.upload(seqs))
    batch.set_circular(circular)
    spec = KmerCounts(3, rows="gene", step=3)
    records = [(0, 10, 69, 1), (0, 40, 114, -1), (1, 6, 53, 1), (2, 25, 36, 1), (2, 4, 15, -1), (3, 1, 30, 1)]
    genes = gene_array(records)
    R, S = len(records), 70
    need = (R - 1) * S + 64
    mem = keep(hip_mem.DeviceArray.from_numpy(np.full(4 * (need + 8), CANARY, np.uint8)))
    win_out = np.zeros(8, np.int64)

    def raw(ptr=mem.ptr, n_out=need, recs=genes, table=None, **change):
        o = spec.opts(S)
        tab = np.array(spec.table if table is None else table, np.int32)
        o.bin_of_code = tab.ctypes.data
        for name, v in change.items():
            setattr(o, name, v)
        rc = ctx.L.pga_count_kmers(ctx.h, batch.h, len(recs), ctypes.c_void_p(recs.ctypes.data), ctypes.byref(o), ctypes.c_void_p(ptr), n_out, None,
                                   ctypes.c_void_p(win_out.ctypes.data))
        return rc, ctx.L.pga_last_error(ctx.h).decode()

    def changed(g, **fields):
        out = genes.copy()
        for name, v in fields.items():
            out[name][g] = v
        return out

    host = np.zeros(need + 8, np.int32)
    below, above = list(spec.table), list(spec.table)
    below[5], above[63] = -2, 64
    for what, kw, word in (("k = 0", dict(k=0), "k must be 1 .. 6"),
                           ("k = 7", dict(k=7), "k must be 1 .. 6"),
                           ("step = 2", dict(step=2), "step must be 1 or 3"),
                           ("step = 3 for contig rows", dict(rows=_cabi.COUNT_CONTIG), "step must be 1 for contig rows"),
                           ("a row kind that is none", dict(rows=3), "rows must be"),
                           ("no bins", dict(n_bins=0), "n_bins"),
                           ("too many bins", dict(n_bins=4097), "n_bins"),
                           ("a table entry below -1", dict(table=below), "bin_of_code[5] = -2"),
                           ("a table entry beyond the bins", dict(table=above), "bin_of_code[63] = 64"),
                           ("no table", dict(bin_of_code=None), "bin_of_code is NULL"),
                           ("S below the bins", dict(row_stride=63), "row_stride = 63 is less than n_bins = 64"),
                           ("out one element too small", dict(n_out=need - 1), "n_out_elems"),
                           ("a record of another contig", dict(recs=changed(3, contig=4)), "gene 3 names contig 4"),
                           ("a record outside its contig", dict(recs=changed(5, begin=51, end=53)), "gene 5 lies outside"),
                           ("a record longer than its contig", dict(recs=changed(4, begin=1, end=33)), "gene 4 lies outside"),
                           ("e > L on a contig that is not circular", dict(recs=changed(5, begin=40, end=54)), "gene 5 ends beyond"),
                           ("a length that is no multiple of 3", dict(recs=changed(0, end=70)), "gene 0 is 61 bases"),
                           ("a host pointer", dict(ptr=host.ctypes.data), "not device memory"),
                           ("a pointer that is not 4-byte aligned", dict(ptr=mem.ptr + 2), "aligned")):
        rc, msg = raw(**kw)
        assert rc == _cabi.PGA_EINVAL and word in msg and msg.startswith("pga_count_kmers: "), (what, rc, msg)
    with pytest.raises(ValueError, match="not device memory"):
        ctx.kmer_counts(batch, genes, spec, out=View(host.ctypes.data, (R, 64), (4 * S, 4)))
    with pytest.raises(ValueError, match="columns"):
        ctx.kmer_counts(batch, genes, spec, out=View(mem.ptr, (R, 63), (4 * S, 4)))
    with pytest.raises(ValueError, match=r"\[6, S\] tensor"):
        ctx.kmer_counts(batch, genes, spec, out=View(mem.ptr, (R - 1, 64), (4 * S, 4)))
    with pytest.raises(TypeError, match="int32"):
        ctx.kmer_counts(batch, genes, spec, out=View(mem.ptr, (R, 64), (8 * S, 8), "<i8"))
    with pytest.raises(TypeError, match="KmerCounts"):
        ctx.kmer_counts(batch, genes, "codons")
    assert np.all(host == 0) and np.all(mem.to_numpy(np.uint8) == CANARY)           # nothing was written anywhere
    rc, msg = raw()                                                                  # the context runs a good call afterwards
    assert rc == 0, msg
    want, windows = kmer_counts_ref(seqs, circular, records, 3, "gene", 3, spec.table, 64)
    assert win_out[:R].tolist() == windows.tolist()
    got = mem.to_numpy(np.int32)
    for g in range(R):
        assert np.array_equal(got[g * S:g * S + 64], want[g]) and np.all(got[g * S + 64:(g + 1) * S] == CANARY32), g


def test_a_row_of_more_windows_than_an_int32_holds_is_refused(ctx):
    from pyrodigal_amd import KmerCounts, _cabi
    seq = np.frombuffer(b"ACGT", np.uint8)[np.arange(3_000_000) % 4].tobytes()
    batch = keep(ctx.upload([seq]))
    mem = keep(hip_mem.DeviceArray.from_numpy(np.full(4 * 8, CANARY, np.uint8)))
    spec = KmerCounts(1, rows="contig_genes")
    with pytest.raises(ValueError, match="contig 0 has 2160000000 window positions"):
        ctx.kmer_counts(batch, gene_array([(0, 1, 3_000_000, 1)] * 720), spec, out=View(mem.ptr, (1, 4)))
    assert np.all(mem.to_numpy(np.uint8) == CANARY)
    dc = ctx.kmer_counts(batch, gene_array([(0, 1, 3_000_000, 1), (0, 1, 3_000_000, -1)]), spec, out=View(mem.ptr, (1, 4)))      # 6 000 000 fit
    assert mem.to_numpy(np.int32)[:4].tolist() == [1_500_000] * 4 and dc.windows.tolist() == [6_000_000]


# ---- 5. through the finder ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib
    return lib


@pytest.fixture(scope="module")
def meta_bins(lib):
    from pyrodigal_amd import benchdata
    return lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])


@functools.lru_cache(maxsize=None)
def golden_contigs():
    return [rec[1].encode("ascii") for name in ("KK037166.fna.gz", "SRR492066.fna.gz") for rec in read_fasta(name)]


def records_of_genes(all_genes):
    return [(i, g.begin, g.end, g.strand, int(g.partial_begin), int(g.partial_end)) for i, genes in enumerate(all_genes) for g in genes]


def codon_rows(flat_genes):
    """A count of the codons of Gene.sequence(): [G, 64], codons with a letter that is not A, C, G, T left out."""
    rows = np.zeros((len(flat_genes), 64), np.int32)
    for g, gene in enumerate(flat_genes):
        text = gene.sequence()
        for codon, c in collections.Counter(text[t:t + 3] for t in range(0, len(text) - 2, 3)).items():
            if set(codon) <= set("ACGT"):
                rows[g, 16 * "ACGT".index(codon[0]) + 4 * "ACGT".index(codon[1]) + "ACGT".index(codon[2])] = c
    return rows


def check_finder(finder, given, seqs, circles=None, lengths=None, **options):
    """find_counts_batch on the Genes it returns: codon rows per gene against Gene.sequence(), their sums per contig, and canonical
    4-mer rows per contig against the reference on the input (the trimmed input where a record was trimmed)."""
    from pyrodigal_amd import KmerCounts
    lengths = [len(s) for s in seqs] if lengths is None else lengths
    circles = [False] * len(seqs) if circles is None else circles
    probe = finder.find_genes_batch(given, **options)
    flat = [g for genes in probe for g in genes]
    want_codons = codon_rows(flat)
    out = None
    for spec in (KmerCounts(3, rows="gene", step=3), KmerCounts(3, rows="contig_genes", step=3), KmerCounts(4, canonical=True)):
        t = Target(len(flat) if spec.rows == "gene" else len(seqs), spec.n_bins)
        genes, dc = finder.find_counts_batch(given, spec, out=t.out, **options)
        assert records_of_genes(genes) == records_of_genes(probe)                   # the same Genes as find_genes_batch
        assert [len(g.sequence.data) for g in genes] == lengths and dc.counts is t.out
        if spec.rows == "gene":
            want = want_codons
            assert dc.gene_begin.tolist() == np.concatenate([[0], np.cumsum([len(g) for g in genes])]).tolist()
            assert dc.windows.tolist() == [(g.end - g.begin + 1) // 3 for g in flat]
        elif spec.rows == "contig_genes":
            want = np.zeros((len(seqs), 64), np.int32)
            for (i, *_), row in zip(records_of_genes(genes), want_codons):
                want[i] += row
        else:
            want, windows = kmer_counts_ref([s[:n] for s, n in zip(seqs, lengths)], circles, [], 4, "contig", 1, spec.table, 136)
            assert dc.windows.tolist() == windows.tolist()
        assert np.array_equal(t.read(), t.expect(want)), spec
        out = genes
    return out


def test_find_counts_batch_on_the_golden_contigs(lib, meta_bins):
    from pyrodigal_amd import DeviceSequences
    seqs = golden_contigs()
    finder = lib.GeneFinder(meta=True, metagenomic_bins=meta_bins)
    genes = check_finder(finder, seqs, seqs)
    assert sum(len(g) for g in genes) > 30 and {g.strand for x in genes for g in x} == {1, -1}
    before = records_of_genes(finder.find_genes_batch(seqs))                        # a plain call is what it was, after counts calls
    assert before == records_of_genes(genes) == records_of_genes(lib.GeneFinder(meta=True, metagenomic_bins=meta_bins).find_genes_batch(seqs))
    # the input as a device tensor gives the same tensors
    rows = np.full((len(seqs), max(map(len, seqs))), ord("N"), np.uint8)
    for i, s in enumerate(seqs):
        rows[i, :len(s)] = np.frombuffer(s, np.uint8)
    given = DeviceSequences(keep(hip_mem.DeviceArray.from_numpy(rows)), [len(s) for s in seqs])
    assert records_of_genes(check_finder(finder, given, seqs)) == records_of_genes(genes)


def test_find_counts_batch_on_circles_and_trimmed_records(lib, meta_bins):
    g = golden_contigs()[0]
    circle = g[1000:9000]
    seqs = [g[:6000], circle + circle[:40], g[3000:3200].lower() + b"NNNNNNRYK" + g[3200:7000]]
    finder = lib.GeneFinder(meta=True, metagenomic_bins=meta_bins)
    genes = check_finder(finder, seqs, seqs, circles=[True] * 3, circular=True)
    assert all(x.circular for x in genes)
    lengths = [len(seqs[0]), len(seqs[1]) - 40, len(seqs[2])]
    genes = check_finder(finder, seqs, seqs, circles=[False, True, False], lengths=lengths, trim_terminal_repeats=True)
    assert genes[1].terminal_repeat == 40 and genes[1].circular and not genes[0].circular


def test_find_counts_batch_refuses_a_request_that_splits(lib):
    import gzip
    from pyrodigal_amd import KmerCounts
    from tests.util import golden_path
    tinfs = [lib.TrainingInfo(raw=np.frombuffer(gzip.open(golden_path(name)).read(), np.uint8).copy())
             for name in ("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz", "SRR492066.training.bin.gz")]
    g = golden_contigs()[0]
    seqs = [g[k * 2000:k * 2000 + 8000] for k in range(4)]
    small = lib.GeneFinder(coalesce_bases=15000)
    with pytest.raises(ValueError, match="device calls.*find_counts_batch"):
        small.find_counts_batch(seqs, KmerCounts(3, rows="gene", step=3), training_infos=[tinfs[i % 2] for i in range(len(seqs))])


# ---- 6. torch --------------------------------------------------------------------------------------------------------------------------
TORCH_SCRIPT = r'''
import sys
import torch                                   # first: the library then binds to the HIP runtime of torch's wheel
if not torch.cuda.is_available():
    print("torch sees no GPU")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
import numpy as np
from pyrodigal_amd import KmerCounts, DeviceCounts, benchdata, lib

bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])
seqs = [benchdata.synthetic_contig(n, gc, 900 + i) for i, (n, gc) in enumerate(((20000, 0.4), (12345, 0.6), (61, 0.5), (30011, 0.5)))]
want_genes = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_genes_batch(seqs)
flat = [g for genes in want_genes for g in genes]
assert len(flat) > 30
side = torch.cuda.Stream()
code = {a + b + c: 16 * i + 4 * j + k for i, a in enumerate("ACGT") for j, b in enumerate("ACGT") for k, c in enumerate("ACGT")}
for rows in ("gene", "contig_genes"):
    spec = KmerCounts(3, rows=rows, step=3)
    with torch.cuda.stream(side):
        genes, dc = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_counts_batch(seqs, spec)
        total = dc.counts.sum(dim=1)                # a consumer on the same stream
    assert isinstance(dc, DeviceCounts) and dc.counts.is_cuda and dc.counts.dtype == torch.int32 and dc.counts.device.index == 0
    assert [[(g.begin, g.end, g.strand) for g in x] for x in genes] == [[(g.begin, g.end, g.strand) for g in x] for x in want_genes]
    want = np.zeros((len(flat), 64), np.int64)
    for g, gene in enumerate(flat):
        text = gene.sequence()
        for t in range(0, len(text), 3):
            want[g, code[text[t:t + 3]]] += 1
    if rows == "contig_genes":
        per = np.zeros((len(seqs), 64), np.int64)
        g = 0
        for i, x in enumerate(genes):
            for _ in x:
                per[i] += want[g]
                g += 1
        want = per
    assert tuple(dc.counts.shape) == want.shape and np.array_equal(dc.counts.cpu().numpy(), want), "counts differ"
    assert np.array_equal(total.cpu().numpy(), dc.windows) and dc.windows.tolist() == want.sum(axis=1).tolist()
    if rows == "gene":
        a, b = int(dc.gene_begin[1]), int(dc.gene_begin[2])
        view = dc.counts_of[1]
        assert tuple(view.shape) == (b - a, 64) and view.data_ptr() == dc.counts[a].data_ptr()
    else:
        assert dc.counts_of[3].data_ptr() == dc.counts[3].data_ptr()
print("torch kmer counts ok: %d genes" % len(flat))
'''


def test_torch_tensor_in_a_fresh_process(tmp_path):
    """torch is imported by the child alone (this process holds the library's HIP runtime and gets no second one); `out=None`
    allocates the tensor under torch's current stream.  The child says so when torch sees no GPU, and the test is skipped."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "torch_kmer_counts.py"
    script.write_text(TORCH_SCRIPT)
    done = subprocess.run([sys.executable, str(script), root], timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, "child ended with %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    if "torch sees no GPU" in done.stdout:
        pytest.skip("torch sees no GPU")
    assert "torch kmer counts ok" in done.stdout
