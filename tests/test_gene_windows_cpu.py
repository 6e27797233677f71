"""Gene and flanking nucleotide windows without a GPU (pga_gene_windows, GeneWindows): what the constructor refuses,
the vocabularies, value semantics, the host arithmetic of the row lengths, the plain-Python restatement of the rule
(tests/gene_windows_ref.py) against string slicing, and the ctypes mirror of pga_window_opts against the header."""
import ctypes
import os
import pickle
import subprocess

import numpy as np
import pytest

from pyrodigal_amd import _cabi
from pyrodigal_amd._cabi import GeneWindows
from tests.gene_windows_ref import DEFAULT_BASE_IDS, DEFAULT_CODON_IDS, gene_windows_ref, offsets_of, row_tokens

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CODONS = [a + b + c for a in "ACGT" for b in "ACGT" for c in "ACGT"]


def gene_array(recs):
    genes = np.zeros(len(recs), _cabi.GENE_DTYPE)
    for name, col in zip(("contig", "begin", "end", "strand"), zip(*recs)):
        genes[name] = col
    return genes


# ---- the constructor -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, error, word", [
    (dict(unit="residue"), ValueError, "unit"),
    (dict(begin=("middle", 0)), ValueError, "anchor"),
    (dict(end=("end",)), ValueError, "anchor, delta"),
    (dict(begin=("start", 1.5)), TypeError, "delta"),
    (dict(begin=("start", -(1 << 30) - 1)), ValueError, "2\\^30"),
    (dict(end=("end", (1 << 30) + 1)), ValueError, "2\\^30"),
    (dict(unit="codon", begin=("start", -4)), ValueError, "multiple of 3"),
    (dict(unit="codon", end=("end", 2)), ValueError, "multiple of 3"),
    (dict(layout="padded", pad=None), ValueError, "pad"),
    (dict(layout="dense"), ValueError, "layout"),
    (dict(dtype="int16"), ValueError, "dtype"),
    (dict(vocabulary="ACG"), ValueError, "'T'"),
    (dict(vocabulary="ACGT"), ValueError, "unknown"),
    (dict(vocabulary="AACGTN"), ValueError, "twice"),
    (dict(vocabulary={"A": 0, "C": 1, "G": 2, "T": 3, "N": 4, "X": 5}), ValueError, "'X'"),
    (dict(vocabulary={"A": 0, "C": 1, "G": 2}, unknown=9), ValueError, "'T'"),
    (dict(vocabulary={"A": 0, "C": 1, "G": 2, "T": True}, unknown=9), TypeError, "integer"),
    (dict(unit="codon", vocabulary="ACGTN"), TypeError, "mapping"),
    (dict(unit="codon", vocabulary={c: k for k, c in enumerate(CODONS[:63])}, unknown=64), ValueError, "'TTT'"),
    (dict(unit="codon", vocabulary={c: k for k, c in enumerate(CODONS)}), ValueError, "'NNN'"),
    (dict(vocabulary=7), TypeError, "vocabulary"),
    (dict(dtype="uint8", pad=256), ValueError, "pad, 256"),
    (dict(dtype="uint8", unknown=300), ValueError, "300"),
    (dict(dtype="uint8", outside=-1), ValueError, "outside"),
    (dict(dtype="int32", bos=1 << 31), ValueError, "bos"),
    (dict(dtype="int32", vocabulary={"A": 0, "C": 1, "G": 2, "T": -(1 << 31) - 1, "N": 4}), ValueError, "'T'"),
    (dict(max_length=0), ValueError, "max_length"),
    (dict(bos=1, eos=2, max_length=2), ValueError, "max_length"),
])
def test_constructor_refuses(kw, error, word):
    kw.setdefault("pad", 0)
    with pytest.raises(error, match=word):
        GeneWindows(**kw)


def test_default_and_mapped_vocabularies():
    w = GeneWindows(pad=9)
    assert w.ids == (0, 1, 2, 3, 4, 4) == DEFAULT_BASE_IDS and (w.unknown, w.outside) == (4, 4)
    assert (w.begin, w.end, w.token_unit, w.dtype, w.layout, w.max_length) == (("start", 0), ("end", 0), "base", "int64", "padded", None)
    assert (GeneWindows.row, GeneWindows.unit, GeneWindows.per_contig) == ("gene", "tokens", "lengths")
    assert GeneWindows(pad=9, outside=7).ids == (0, 1, 2, 3, 4, 7) and GeneWindows(pad=9, unknown=8).ids == (0, 1, 2, 3, 8, 8)
    assert GeneWindows(vocabulary="-NTGCA", pad=0).ids == (5, 4, 3, 2, 1, 1)
    assert GeneWindows(vocabulary="tgca", unknown=11, outside=12, layout="ragged").ids == (3, 2, 1, 0, 11, 12)
    assert GeneWindows(vocabulary={"a": 10, b"C": 11, "G": 12, "T": 13, "N": 14}, pad=0).ids == (10, 11, 12, 13, 14, 14)
    c = GeneWindows(unit="codon", pad=-1)
    assert c.ids == DEFAULT_CODON_IDS and len(c.ids) == 66
    table = {codon: 100 + k for k, codon in enumerate(reversed(CODONS))}
    table["NNN"] = 7
    m = GeneWindows(unit="codon", vocabulary=table, outside=8, pad=0)
    assert m.ids[:64] == tuple(163 - k for k in range(64)) and m.ids[64:] == (7, 8)
    assert m.ids[16 * 0 + 4 * 3 + 2] == table["ATG"]                          # the public ACGT order
    o = m.opts(12, 20)
    assert (o.elem_bytes, o.layout, o.row_width, o.row_stride, o.unit) == (8, _cabi.TOKENS_PADDED, 12, 20, _cabi.WINDOW_CODONS)
    assert list(o.ids) == list(m.ids) and (o.bos, o.eos, o.max_length, o.pad) == (_cabi.TOKEN_NONE, _cabi.TOKEN_NONE, 0, 0)
    o = GeneWindows(("start", -60), ("end", 30), bos=5, eos=6, max_length=40, layout="ragged", dtype="uint8").opts()
    assert (o.from_anchor, o.from_delta, o.to_anchor, o.to_delta) == (_cabi.WINDOW_START, -60, _cabi.WINDOW_END, 30)
    assert (o.elem_bytes, o.layout, o.unit, o.bos, o.eos, o.max_length) == (1, _cabi.TOKENS_RAGGED, _cabi.WINDOW_BASES, 5, 6, 40)
    assert list(o.ids)[:6] == [0, 1, 2, 3, 4, 4]


def test_value_semantics_and_pickle():
    import pyrodigal_amd
    assert pyrodigal_amd.GeneWindows is GeneWindows and "GeneWindows" in pyrodigal_amd.__all__
    a = GeneWindows(("start", -60), ("start", 30), bos=5, pad=9, dtype="int32", max_length=50)
    b = GeneWindows(("start", -60), ("start", 30), bos=5, pad=9, dtype="int32", max_length=50)
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    for other in (GeneWindows(("start", -60), ("start", 33), bos=5, pad=9, dtype="int32", max_length=50),
                  GeneWindows(("start", -60), ("end", 30), bos=5, pad=9, dtype="int32", max_length=50),
                  GeneWindows(("start", -60), ("start", 30), bos=5, pad=9, dtype="int64", max_length=50),
                  GeneWindows(("start", -60), ("start", 30), bos=5, pad=9, dtype="int32", max_length=50, outside=5),
                  GeneWindows(("start", -60), ("start", 30), unit="codon", bos=5, pad=9, dtype="int32", max_length=50)):
        assert a != other
    assert a != _cabi.BaseLabels("frame")
    for spec in (a, GeneWindows(unit="codon", eos=70, layout="ragged", dtype="uint8")):
        back = pickle.loads(pickle.dumps(spec))
        assert back == spec and hash(back) == hash(spec) and back.ids == spec.ids and back.specials == spec.specials
        assert (back.unknown, back.outside, back.token_unit) == (spec.unknown, spec.outside, spec.token_unit)
        assert bytes(back.opts(3, 4)) == bytes(spec.opts(3, 4))
        assert "GeneWindows" in repr(back)


def test_lengths_against_hand_arithmetic():
    genes = gene_array([(0, 1, 90, 1), (0, 100, 102, -1), (1, 7, 36, -1), (0, 10, 609, 1)])          # n = 90, 3, 30, 600
    assert GeneWindows(pad=0).lengths(genes).tolist() == [90, 3, 30, 600]
    assert GeneWindows(pad=0).lengths(genes).dtype == np.int64
    assert GeneWindows(("start", -60), ("start", 30), pad=0).lengths(genes).tolist() == [90, 90, 90, 90]
    assert GeneWindows(("end", 0), ("end", 50), pad=0, bos=1).lengths(genes).tolist() == [51, 51, 51, 51]
    assert GeneWindows(("start", -10), ("end", 10), pad=0, bos=1, eos=2).lengths(genes).tolist() == [112, 25, 52, 622]
    # windows that are empty or inverted on the short genes: rows without bases, the specials alone
    assert GeneWindows(("start", 30), ("end", 0), pad=0).lengths(genes).tolist() == [60, 0, 0, 570]
    assert GeneWindows(("start", 30), ("end", -3), pad=0, eos=2).lengths(genes).tolist() == [58, 1, 1, 568]
    assert GeneWindows(("end", 0), ("start", 0), pad=0).lengths(genes).tolist() == [0, 0, 0, 0]
    assert GeneWindows(pad=0, max_length=40).lengths(genes).tolist() == [40, 3, 30, 40]
    assert GeneWindows(pad=0, max_length=40, bos=1, eos=2).lengths(genes).tolist() == [40, 5, 32, 40]
    assert GeneWindows(unit="codon", pad=0).lengths(genes).tolist() == [30, 1, 10, 200]
    assert GeneWindows(("start", -6), ("end", 3), unit="codon", pad=0, eos=1, max_length=12).lengths(genes).tolist() == [12, 5, 12, 12]
    assert GeneWindows(pad=0).lengths(genes[:0]).tolist() == []


# ---- the restatement against string slicing ---------------------------------------------------------------------------------------------
SEQ = b"ACGTNacgtnRYKMACGTTGCAAACCCGGGTTTWSACGTACGTAGCTAGCTAGGATCCTTAAGG"      # 64 letters: both cases, IUPAC codes, Ns
LETTERS = "ACGTN"


def slice_linear(seq, lo, hi):
    """Positions lo .. hi - 1 (0-based) of a linear contig as letters, `-` outside it."""
    return "".join(chr(seq[p]).upper() if 0 <= p < len(seq) else "-" for p in range(lo, hi))


def normalise(text):
    return "".join(ch if ch in "ACGT-" else "N" for ch in text)


def reverse_complement(text):
    return text.translate(str.maketrans("ACGTN-", "TGCAN-"))[::-1]


def as_letters(tokens):
    return "".join("ACGTN-"[v] for v in tokens)


def test_reference_on_hand_records():
    assert len(SEQ) == 64
    ids = (0, 1, 2, 3, 4, 5)
    fwd, rev = (0, 11, 40, 1), (0, 11, 40, -1)                              # [11, 40], n = 30
    assert offsets_of(fwd, ("start", -60), ("start", 30)) == (-60, 30) and offsets_of(rev, ("end", -3), ("end", 50)) == (27, 80)
    # the gene itself
    body = normalise(slice_linear(SEQ, 10, 40))
    assert body == "RYKMACGTTGCAAACCCGGGTTTWSACGTA".translate(str.maketrans("RYKMWS", "NNNNNN"))
    assert as_letters(row_tokens(SEQ, False, fwd, ("start", 0), ("end", 0), ids=ids)) == body
    assert as_letters(row_tokens(SEQ, False, rev, ("start", 0), ("end", 0), ids=ids)) == reverse_complement(body)
    # flanks that run over both ends of the linear contig
    assert as_letters(row_tokens(SEQ, False, fwd, ("start", -15), ("end", 30), ids=ids)) == normalise(slice_linear(SEQ, -5, 70))
    assert as_letters(row_tokens(SEQ, False, rev, ("start", -30), ("end", 15), ids=ids)) == reverse_complement(normalise(slice_linear(SEQ, -5, 70)))
    assert as_letters(row_tokens(SEQ, False, rev, ("end", 0), ("end", 12), ids=ids)) == reverse_complement(normalise(slice_linear(SEQ, -2, 10)))
    # the same windows on a circle: the contig three times over, then plain slicing
    thrice = SEQ * 3
    assert as_letters(row_tokens(SEQ, True, fwd, ("start", -15), ("end", 30), ids=ids)) == normalise(slice_linear(thrice, 64 - 5, 64 + 70))
    assert as_letters(row_tokens(SEQ, True, rev, ("start", -30), ("end", 15), ids=ids)) == reverse_complement(normalise(slice_linear(thrice, 64 - 5, 64 + 70)))
    assert as_letters(row_tokens(SEQ, True, fwd, ("start", -80), ("start", 0), ids=ids)) == normalise(slice_linear(SEQ * 4, 128 + 10 - 80, 128 + 10))
    across = (0, 50, 79, 1)                                                 # e > L on the circle
    assert as_letters(row_tokens(SEQ, True, across, ("start", 0), ("end", 0), ids=ids)) == normalise(slice_linear(thrice, 49, 79))
    # empty and inverted windows, specials, max_length
    assert row_tokens(SEQ, False, fwd, ("start", 30), ("end", 0), ids=ids) == []
    assert row_tokens(SEQ, False, fwd, ("end", 3), ("start", 0), ids=ids, bos=8, eos=9) == [8, 9]
    assert row_tokens(SEQ, False, fwd, ("start", 0), ("end", 0), ids=ids, bos=8, eos=9, max_length=6) == [8, 4, 4, 4, 4, 9]
    # codons: ACG TTG CAA ... from position 15, an N codon in front, an outside codon beyond the end
    gene = (0, 12, 23, 1)                                                   # YKM ACG TTG CAA
    codon = lambda text: 16 * "ACGT".index(text[0]) + 4 * "ACGT".index(text[1]) + "ACGT".index(text[2])
    cids = tuple(range(64)) + (64, 65)
    assert row_tokens(SEQ, False, gene, ("start", 0), ("end", 0), "codon", cids) == [64, codon("ACG"), codon("TTG"), codon("CAA")]
    assert row_tokens(SEQ, False, (0, 12, 23, -1), ("start", 0), ("end", 0), "codon", cids) == [codon("TTG"), codon("CAA"), codon("CGT"), 64]
    assert row_tokens(SEQ, False, (0, 59, 64, 1), ("start", 0), ("end", 6), "codon", cids) == [codon("TTA"), codon("AGG"), 65, 65]
    assert row_tokens(SEQ, True, (0, 59, 64, 1), ("start", 0), ("end", 6), "codon", cids) == [codon("TTA"), codon("AGG"), codon("ACG"), 64]
    straddle = (0, 63, 68, 1)                                               # GG|A CGT on the circle: a codon across the origin
    assert row_tokens(SEQ, True, straddle, ("start", 0), ("end", 0), "codon", cids) == [codon("GGA"), codon("CGT")]


def test_reference_tensors():
    records = [(0, 11, 40, 1), (0, 11, 13, -1), (0, 20, 49, -1)]
    kw = dict(begin=("start", 27), end=("end", 0), ids=(0, 1, 2, 3, 4, 5))
    flat, off, lens = gene_windows_ref([SEQ], [False], records, layout="ragged", dtype=np.uint8, **kw)
    assert lens.tolist() == [3, 0, 3] and off.tolist() == [0, 3, 3, 6] and flat.dtype == np.uint8
    assert as_letters(flat) == "GTA" + reverse_complement("GCA")          # positions 38 .. 40, and 20 .. 22 read backwards
    rows, _, _ = gene_windows_ref([SEQ], [False], records, layout="padded", pad=-7, width=5, dtype=np.int32, **kw)
    assert rows.tolist() == [[2, 3, 0, -7, -7], [-7] * 5, [3, 2, 1, -7, -7]]
    assert gene_windows_ref([SEQ], None, [], layout="padded", **kw)[0].shape == (0, 0)


# ---- the ctypes mirror against the header -------------------------------------------------------------------------------------------------
def test_window_opts_matches_the_header(tmp_path):
    src = tmp_path / "window_sizes.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "pyrodigal_amd.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %d %d %d %d\\n", sizeof(pga_window_opts), offsetof(pga_window_opts, unit), offsetof(pga_window_opts, from_delta),
           offsetof(pga_window_opts, max_length), offsetof(pga_window_opts, ids), offsetof(pga_window_opts, pad),
           PGA_WINDOW_BASES, PGA_WINDOW_CODONS, PGA_WINDOW_START, PGA_WINDOW_END);
    return 0;
}
""")
    exe = tmp_path / "window_sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    W = _cabi.WindowOpts
    assert got == [ctypes.sizeof(W), W.unit.offset, W.from_delta.offset, W.max_length.offset, W.ids.offset, W.pad.offset,
                   _cabi.WINDOW_BASES, _cabi.WINDOW_CODONS, _cabi.WINDOW_START, _cabi.WINDOW_END]
    assert got[0] == 24 + 16 + 24 + 8 * 66 + 24 and "pga_gene_windows" in _cabi.EXPORTS
