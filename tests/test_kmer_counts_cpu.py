"""K-mer and codon counts without a GPU (pga_count_kmers, KmerCounts): the plain-Python restatement of the rule
(tests/kmer_counts_ref.py) against brute-force string counting, the folded bins, the amino-acid bins, what the constructor refuses,
value semantics, the host arithmetic of the window positions, and the ctypes mirror of pga_count_opts against the header."""
import collections
import ctypes
import os
import pickle
import subprocess

import numpy as np
import pytest

from pyrodigal_amd import KmerCounts, _cabi
from tests import tables_ref
from tests.kmer_counts_ref import canonical_table, identity_table, kmer, kmer_counts_ref, rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMPLEMENT = str.maketrans("ACGTN", "TGCAN")


def letters(n, seed):
    """Upper-case, lower-case and IUPAC letters: about one in twelve reads N."""
    return np.frombuffer(b"ACGTACGTACGTacgtacgtRYn", np.uint8)[np.random.default_rng(seed).integers(0, 23, size=n)].tobytes()


def normalise(seq):
    return "".join(ch if ch in "ACGT" else "N" for ch in seq.decode().upper())


def brute(text, k, step, n_starts=None):
    """Counter of the k-letter strings at 0, step, .. of `text` without an N; `n_starts`: how many starts (default: all that fit)."""
    starts = range(0, len(text) - k + 1, step) if n_starts is None else range(0, n_starts * step, step)
    return collections.Counter(text[t:t + k] for t in starts if "N" not in text[t:t + k])


def as_counter(row, k):
    return collections.Counter({kmer(x, k): int(c) for x, c in enumerate(row) if c})


# ---- the reference against string counting ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_reference_contig_rows_against_string_counting(k):
    seqs = [letters(n, 10 * k + n) for n in (0, 1, k - 1, k, k + 1, 37, 200)]
    for circular in (False, True):
        counts, windows = kmer_counts_ref(seqs, [circular] * len(seqs), [], k, "contig", 1, identity_table(k), 4 ** k)
        assert counts.shape == (len(seqs), 4 ** k) and counts.dtype == np.int32
        for i, s in enumerate(seqs):
            text, L = normalise(s), len(s)
            if L < k:
                assert windows[i] == 0 and not counts[i].any()
            elif circular:
                assert windows[i] == L and as_counter(counts[i], k) == brute(text + text[:k - 1], k, 1, L)
            else:
                assert windows[i] == L - k + 1 and as_counter(counts[i], k) == brute(text, k, 1)


@pytest.mark.parametrize("k, step", [(1, 1), (3, 3), (3, 1), (4, 1), (5, 3), (6, 3), (6, 1)])
def test_reference_gene_rows_against_string_counting(k, step):
    seq = letters(90, 5)
    text, L = normalise(seq), 90
    records = [(0, 4, 33, 1), (0, 4, 33, -1), (0, 1, 3, 1), (0, 88, 90, -1), (0, 1, 90, 1), (0, 70, 99, 1), (0, 85, 96, -1), (0, 13, 18, 1)]
    counts, windows = kmer_counts_ref([seq], [True], records, k, "gene", step, identity_table(k), 4 ** k)
    laid = text * 2
    for g, (_, b, e, strand) in enumerate(records):
        body = laid[b - 1:e]
        if strand == -1:
            body = body.translate(COMPLEMENT)[::-1]
        n = e - b + 1
        assert windows[g] == (0 if n < k else (n - k) // step + 1)
        assert as_counter(counts[g], k) == brute(body, k, step), (g, k, step)
    summed, w = kmer_counts_ref([seq, seq], [True, True], [(1,) + r[1:] for r in records], k, "contig_genes", step, identity_table(k), 4 ** k)
    assert not summed[0].any() and w[0] == 0 and np.array_equal(summed[1], counts.sum(axis=0)) and w[1] == windows.sum()


def test_reference_bins_and_dropped_codes():
    seq = b"ACGTTGCAAC"
    table = [0, -1, 1, 1]                                                      # A, and G with T; C is dropped
    counts, windows = kmer_counts_ref([seq], [False], [], 1, "contig", 1, table, 2)
    assert counts.tolist() == [[3, 4]] and windows.tolist() == [10]


# ---- folded bins ---------------------------------------------------------------------------------------------------------------------
def test_canonical_bins():
    assert [KmerCounts(k, canonical=True).n_bins for k in range(1, 7)] == [2, 10, 32, 136, 512, 2080]
    for k in range(1, 7):
        spec = KmerCounts(k, canonical=True)
        assert list(spec.table) == canonical_table(k)
        for x in range(4 ** k):
            assert rc(rc(x, k), k) == x == _cabi.kmer_rc(_cabi.kmer_rc(x, k), k) and rc(x, k) == _cabi.kmer_rc(x, k)
            assert spec.table[x] == spec.table[rc(x, k)]
        palindromes = [x for x in range(4 ** k) if rc(x, k) == x]
        assert len(palindromes) == (0 if k % 2 else 4 ** (k // 2))           # an odd k-mer's middle base is never its own complement
        assert len({spec.table[x] for x in palindromes}) == len(palindromes)
    assert rc(0b0001_1011, 4) == 0b0001_1011                                   # ACGT is its own reverse complement
    assert kmer(rc(0, 3), 3) == "TTT" and kmer(rc(6, 2), 2) == "CG" and kmer(6, 2) == "CG"


def test_labels():
    assert KmerCounts(1).labels == ("A", "C", "G", "T") and KmerCounts(1, canonical=True).labels == ("A", "C")
    assert KmerCounts(2, canonical=True).labels == ("AA", "AC", "AG", "AT", "CA", "CC", "CG", "GA", "GC", "TA")
    codons = KmerCounts(3, rows="gene", step=3).labels
    assert len(codons) == 64 and codons[:5] == ("AAA", "AAC", "AAG", "AAT", "ACA") and codons[-1] == "TTT"
    lab = KmerCounts(4, canonical=True).labels
    assert len(lab) == 136 and lab[0] == "AAAA" and all(a <= b.translate(COMPLEMENT)[::-1] for a, b in zip(lab, lab)) and list(lab) == sorted(lab)
    assert KmerCounts(3, bins=KmerCounts.codon_bins(11)).labels is None


# ---- amino-acid bins -------------------------------------------------------------------------------------------------------------------
def test_codon_bins():
    order = "ACDEFGHIKLMNPQRSTVWY*"
    assert _cabi.CODON_BIN_LETTERS == order
    for table in (11, 4) + tuple(t for t in tables_ref.TABLES if t not in (4, 11)):
        bins = KmerCounts.codon_bins(table)
        code = tables_ref.code(table)
        assert len(bins) == 64 and [order[b] for b in bins] == [code[kmer(x, 3)] for x in range(64)], table
    tga = 16 * 3 + 4 * 2 + 0
    assert order[KmerCounts.codon_bins(11)[tga]] == "*" and order[KmerCounts.codon_bins(4)[tga]] == "W"
    assert [x for x in range(64) if KmerCounts.codon_bins(11)[x] != KmerCounts.codon_bins(4)[x]] == [tga]
    gtg = 16 * 2 + 4 * 3 + 2
    assert order[KmerCounts.codon_bins(11)[gtg]] == "V"                        # the table's map, no initiator rule
    spec = KmerCounts(3, rows="gene", step=3, bins=KmerCounts.codon_bins(11))
    assert spec.n_bins == 21 and spec.custom and not spec.canonical
    for bad in (7, 0, "11", True, None):
        with pytest.raises(ValueError, match="translation table"):
            KmerCounts.codon_bins(bad)


# ---- the constructor ---------------------------------------------------------------------------------------------------------------------
def test_constructor_errors():
    for bad in (0, 7, -1):
        with pytest.raises(ValueError, match="k must be 1 .. 6"):
            KmerCounts(bad)
    for bad in (4.0, "4", True, None):
        with pytest.raises(TypeError, match="k must be an integer"):
            KmerCounts(bad)
    for bad in ("genes", "contigs", None, 1):
        with pytest.raises(ValueError, match="rows must be"):
            KmerCounts(4, rows=bad)
    for bad in (0, 2, 4, -3):
        with pytest.raises(ValueError, match="step must be 1 or 3"):
            KmerCounts(3, rows="gene", step=bad)
    for bad in (3.0, "3", False):
        with pytest.raises(TypeError, match="step must be an integer"):
            KmerCounts(3, rows="gene", step=bad)
    with pytest.raises(ValueError, match="contig rows count every window"):
        KmerCounts(3, rows="contig", step=3)
    with pytest.raises(TypeError, match="canonical must be a bool"):
        KmerCounts(4, canonical=1)
    with pytest.raises(ValueError, match="exclude each other"):
        KmerCounts(1, canonical=True, bins=[0, 1, 1, 0])
    with pytest.raises(ValueError, match="bins has 3 entries: k = 1 has 4 codes"):
        KmerCounts(1, bins=[0, 1, 2])
    with pytest.raises(ValueError, match="bins has 64 entries"):
        KmerCounts(4, bins=KmerCounts.codon_bins(11))
    with pytest.raises(TypeError, match="the bin of C must be an integer id"):
        KmerCounts(1, bins=[0, 1.5, 2, 3])
    with pytest.raises(ValueError, match="the bin of G, -2, lies outside -1 .. 4095"):
        KmerCounts(1, bins=[0, 1, -2, 3])
    with pytest.raises(ValueError, match="the bin of T, 4096, lies outside"):
        KmerCounts(1, bins=[0, 1, 2, 4096])
    with pytest.raises(ValueError, match="drops every k-mer"):
        KmerCounts(1, bins=[-1] * 4)
    with pytest.raises(TypeError):
        KmerCounts(4, "gene")                                                  # everything but k by keyword
    ok = KmerCounts(1, bins=np.array([0, -1, 4095, 0]))
    assert ok.n_bins == 4096 and ok.table == (0, -1, 4095, 0)
    d = KmerCounts()
    assert (d.k, d.rows, d.step, d.canonical, d.custom, d.n_bins, d.per_contig) == (4, "contig", 1, False, False, 256, "lengths")


def test_value_semantics():
    a, b = KmerCounts(4, canonical=True), KmerCounts(4, canonical=True)
    assert a == b and hash(a) == hash(b) and a is not b and len({a, b}) == 1
    others = [KmerCounts(4), KmerCounts(5, canonical=True), KmerCounts(4, rows="gene", canonical=True), KmerCounts(4, rows="gene", step=3, canonical=True),
              KmerCounts(4, bins=a.table), KmerCounts(3, rows="gene", step=3, bins=KmerCounts.codon_bins(11)),
              KmerCounts(3, rows="gene", step=3, bins=KmerCounts.codon_bins(4))]
    assert len(set(others + [a])) == len(others) + 1 and all(x != a for x in others) and a != "KmerCounts"
    for spec in others + [a]:
        back = pickle.loads(pickle.dumps(spec))
        assert back == spec and hash(back) == hash(spec) and back.labels == spec.labels and back.n_bins == spec.n_bins
        assert "KmerCounts" in repr(spec)
        o = back.opts(300)
        assert (o.rows, o.k, o.step, o.n_bins, o.row_stride) == (_cabi._COUNT_ROWS[spec.rows], spec.k, spec.step, spec.n_bins, 300)
        assert np.ctypeslib.as_array(ctypes.cast(o.bin_of_code, ctypes.POINTER(ctypes.c_int32)), (4 ** spec.k,)).tolist() == list(spec.table)


# ---- window positions: host arithmetic ---------------------------------------------------------------------------------------------------
def test_windows():
    genes = np.zeros(6, _cabi.GENE_DTYPE)
    genes["contig"] = [0, 0, 2, 2, 2, 3]
    genes["begin"] = [1, 10, 5, 5, 40, 1]
    genes["end"] = [3, 39, 10, 304, 51, 6]                                   # n = 3, 30, 6, 300, 12, 6
    genes["strand"] = [1, -1, 1, -1, 1, -1]
    lengths = [100, 3, 500, 6, 0]
    none = np.zeros(0, _cabi.GENE_DTYPE)
    assert KmerCounts(4).windows(none, lengths).tolist() == [97, 0, 497, 3, 0]
    assert KmerCounts(4).windows(none, lengths, [True, True, False, True, True]).tolist() == [100, 0, 497, 6, 0]        # L < k: none
    assert KmerCounts(6).windows(none, lengths, True).tolist() == [100, 0, 500, 6, 0]                                 # L = k on a circle: L
    assert KmerCounts(1).windows(none, lengths).tolist() == lengths
    assert KmerCounts(3, rows="gene", step=3).windows(genes, lengths).tolist() == [1, 10, 2, 100, 4, 2]
    assert KmerCounts(6, rows="gene", step=3).windows(genes, lengths).tolist() == [0, 9, 1, 99, 3, 1]                  # n < k: none
    assert KmerCounts(4, rows="gene", step=1).windows(genes, lengths).tolist() == [0, 27, 3, 297, 9, 3]
    assert KmerCounts(4, rows="gene", step=3).windows(genes, lengths).tolist() == [0, 9, 1, 99, 3, 1]
    assert KmerCounts(3, rows="contig_genes", step=3).windows(genes, lengths).tolist() == [11, 0, 106, 2, 0]
    w = KmerCounts(5, rows="gene").windows(genes, lengths)
    assert w.dtype == np.int64
    # what the reference counts as positions
    seqs = [letters(n, 40 + n) for n in lengths]
    recs = [tuple(int(genes[f][g]) for f in ("contig", "begin", "end", "strand")) for g in range(6)]
    for spec in (KmerCounts(4), KmerCounts(6), KmerCounts(6, rows="gene", step=3), KmerCounts(2, rows="contig_genes")):
        for circ in (False, True):
            _, windows = kmer_counts_ref(seqs, [circ] * 5, recs, spec.k, spec.rows, spec.step, spec.table, spec.n_bins)
            assert spec.windows(genes, lengths, circ).tolist() == windows.tolist()


# ---- the finder, the exports, the header -------------------------------------------------------------------------------------------------
def test_find_counts_batch_takes_a_kmer_counts_only():
    from pyrodigal_amd import GeneWindows, lib
    finder = lib.GeneFinder(meta=True)
    for bad in ("kmers", 4, None, GeneWindows(layout="ragged")):
        with pytest.raises(TypeError, match="`counts` must be a KmerCounts"):
            finder.find_counts_batch([b"ACGT" * 100], bad)
    with pytest.raises(TypeError, match="KmerCounts"):
        _cabi.counts_into(None, None, None, 0, 1, np.zeros(0, _cabi.GENE_DTYPE), "kmers")


def test_count_opts_matches_the_header(tmp_path):
    src = tmp_path / "count_sizes.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "pyrodigal_amd.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(pga_count_opts), offsetof(pga_count_opts, rows), offsetof(pga_count_opts, k),
           offsetof(pga_count_opts, step), offsetof(pga_count_opts, n_bins), offsetof(pga_count_opts, row_stride),
           offsetof(pga_count_opts, bin_of_code), PGA_COUNT_CONTIG, PGA_COUNT_GENE, PGA_COUNT_CONTIG_GENES);
    return 0;
}
""")
    exe = tmp_path / "count_sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    C = _cabi.CountOpts
    assert got == [ctypes.sizeof(C), C.rows.offset, C.k.offset, C.step.offset, C.n_bins.offset, C.row_stride.offset, C.bin_of_code.offset,
                   _cabi.COUNT_CONTIG, _cabi.COUNT_GENE, _cabi.COUNT_CONTIG_GENES]
    assert got[0] == 32 and {"pga_count_kmers", "pga_kmer_counts_chunk"} <= set(_cabi.EXPORTS)
    assert _cabi.load().pga_kmer_counts_chunk() >= 256
