"""MinHash sketches of predicted proteins without a GPU (pga_sketch_proteins, pga_sketch_pairs, ProteinSketches): the
hash's check values, the pure-Python sketch_of / shared against the plain-Python restatement of the rule
(tests/protein_sketches_ref.py), what the constructor refuses, value semantics, the forms of `classes`, and the header: the new
functions, and the ctypes mirror of pga_sketch_opts against what a C program prints."""
import ctypes
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

from pyrodigal_amd import ProteinSketches, _cabi
from tests import protein_sketches_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCED = ("LVIM", "C", "A", "G", "ST", "P", "FYW", "EDNQ", "KR", "H")


def test_hash_check_values():
    assert ref.mix(0, 0) == 0xE220A8397B1DCDAF                   # the first output of splitmix64 from state 0
    assert ref.hash_of(0, 0) == 0x7110541CBD8EE6D7
    assert ref.keys_of(b"MKV", 3, "protein", ref.default_classes()) == [0x4D4B56]
    assert ref.hash_of(0x4D4B56, 0) == 0x2646C952006551D1
    assert ref.hash_of(0x4D4B56, 7) == 0x1D603BCD9D5FF562
    assert ProteinSketches(3).hash_of(0x4D4B56) == 0x2646C952006551D1 and ProteinSketches(3, seed=7).hash_of(0x4D4B56) == 0x1D603BCD9D5FF562
    assert ProteinSketches(3).hash_of(0) == 0x7110541CBD8EE6D7
    assert ProteinSketches(3).sketch_of("MKV") == ([0x2646C952006551D1], 1)
    assert ProteinSketches(3, seed=7).sketch_of(b"MKV") == ([0x1D603BCD9D5FF562], 1)
    for seed in (0, 7, 2 ** 32 - 1):
        for x in (0, 1, 2 ** 64 - 1, 0x4D4B56):
            h = ProteinSketches(1, seed=seed).hash_of(x)
            assert h == ref.hash_of(x, seed) and 0 <= h < 2 ** 63


def test_reference_by_hand():
    d = ref.default_classes()
    assert ref.sketch(b"", 3, 4, "protein", 0, d) == ([], 0) and ref.sketch(b"MK", 3, 4, "protein", 0, d) == ([], 0)
    assert ref.keys_of(b"MKXVL", 2, "protein", d) == [0x4D4B, 0x564C]                         # the windows over X are skipped
    assert ref.keys_of(b"ACGTNAC", 2, "gene") == [0b0001, 0b0110, 0b1011, 0b0001]
    row, w = ref.sketch(b"ACGTNAC", 2, 8, "gene")
    assert w == 4 and len(row) == 3 and row == sorted(row)                                     # AC twice: one hash
    assert ref.sketch(b"AAAAAAAA", 3, 8, "gene") == ([ref.hash_of(0)], 6)
    assert ref.keys_of(b"T" * 32, 32, "gene") == [2 ** 64 - 1]
    assert ref.keys_of(b"\x7f" * 8, 8, "protein", d) == [0x7F7F7F7F7F7F7F7F]
    # pairs: the Mash estimator over the s smallest of the union
    assert ref.pair([1, 2, 3], [1, 2, 3], 3) == (3, 3) and ref.pair([], [], 3) == (0, 0)
    assert ref.pair([1, 3, 5], [2, 4, 6], 3) == (0, 3)
    assert ref.pair([1, 2, 9], [3, 4, 9], 3) == (0, 3)                                         # the overlap lies beyond the 3 smallest
    assert ref.pair([1, 2, 9], [3, 4, 9], 5) == (1, 5) and ref.pair([1, 2], [2], 4) == (1, 2)
    shared, union = ref.pairs_ref([[1, 2], [2, 3]], [(0, 1), (0, 2), (-1, 0), (1, 1)], 4)
    assert shared.tolist() == [1, -1, -1, 2] and union.tolist() == [3, -1, -1, 2]
    out, count, windows, rows = ref.sketches_ref([b"MKV", b"", b"MKVMKV"], 3, 2, "protein", 0, d)
    assert out.dtype == np.int64 and out.shape == (3, 2) and count.tolist() == [1, 0, 2] and windows.tolist() == [1, 0, 4]
    assert out[0, 1] == out[1, 0] == ref.INT64_MAX and out[0, 0] == 0x2646C952006551D1


def test_sketch_of_and_shared_against_the_reference():
    rng = np.random.default_rng(5)
    amino = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWYX*", np.uint8)
    bases = np.frombuffer(b"ACGTN", np.uint8)
    rows = []
    for n in (0, 1, 4, 5, 6, 63, 64, 65, 129, 700):
        prot = rng.choice(amino, size=n).tobytes()
        dna = rng.choice(bases, size=n, p=[0.24, 0.24, 0.24, 0.24, 0.04]).tobytes()
        for k, s, seed in ((1, 1, 0), (3, 2, 7), (5, 32, 0), (8, 64, 2 ** 32 - 1)):
            spec = ProteinSketches(k, s, seed=seed)
            assert spec.sketch_of(prot) == ref.sketch(prot, k, s, "protein", seed, ref.default_classes())
            assert spec.sketch_of(prot.decode()) == spec.sketch_of(prot)
            red = ProteinSketches(k, s, seed=seed, classes=REDUCED)
            assert red.sketch_of(prot) == ref.sketch(prot, k, s, "protein", seed, ref.classes_of(REDUCED))
        for k, s in ((1, 3), (11, 32), (31, 33), (32, 64)):
            assert ProteinSketches(k, s, "gene").sketch_of(dna) == ref.sketch(dna, k, s, "gene")
        rows.append(ProteinSketches(3, 16).sketch_of(prot)[0])
    spec = ProteinSketches(3, 16)
    for a in rows:
        for b in rows:
            assert spec.shared(a, b) == ref.pair(a, b, 16)
    assert spec.shared(np.array(rows[-1], np.int64), rows[-1]) == (16, 16) and spec.shared([], []) == (0, 0)
    # a lower-case base is not a letter of the gene string (the device writes upper case), and a letter >= 128 is skipped
    assert ProteinSketches(1, 4, "gene").sketch_of(b"acgt") == ([], 0)
    assert ProteinSketches(1, 4).sketch_of(b"M\xc3K")[1] == 2


def test_constructor_refusals():
    for bad in ("residue", "", None, 0):
        with pytest.raises(ValueError, match="unit"):
            ProteinSketches(unit=bad)
    for name in ("k", "size", "seed"):
        for bad in (1.0, "3", None, True):
            with pytest.raises(TypeError, match=name):
                ProteinSketches(**{name: bad})
    for bad in (0, 9, -1):
        with pytest.raises(ValueError, match="k must be 1 .. 8"):
            ProteinSketches(bad)
    for bad in (0, 33):
        with pytest.raises(ValueError, match="k must be 1 .. 32"):
            ProteinSketches(bad, unit="gene")
    for bad in (0, 65, -3):
        with pytest.raises(ValueError, match="size"):
            ProteinSketches(size=bad)
    for bad in (-1, 2 ** 32):
        with pytest.raises(ValueError, match="seed"):
            ProteinSketches(seed=bad)
    for name in ("include_stop", "strict"):
        with pytest.raises(TypeError, match=name):
            ProteinSketches(**{name: 1})
    with pytest.raises(TypeError, match="unknown_residue"):
        ProteinSketches(unknown_residue=88)
    for bad in ("", "XX", "é", "\x00"):
        with pytest.raises(ValueError, match="unknown_residue"):
            ProteinSketches(unknown_residue=bad)
    with pytest.raises(TypeError):
        ProteinSketches(5, 32, "protein", 0)                     # (the options are keyword-only)
    assert (ProteinSketches(8).k, ProteinSketches(32, unit="gene").k, ProteinSketches(size=64).size, ProteinSketches(size=1).size) == (8, 32, 64, 1)


def test_value_semantics_and_pickling():
    a, b = ProteinSketches(), ProteinSketches(5, 32, "protein", seed=0, classes=None, include_stop=False, strict=True, unknown_residue="X")
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    assert (a.k, a.size, a.of, a.seed) == (5, 32, "protein", 0)
    others = [ProteinSketches(4), ProteinSketches(size=31), ProteinSketches(unit="gene"), ProteinSketches(seed=1), ProteinSketches(classes=REDUCED),
              ProteinSketches(include_stop=True), ProteinSketches(strict=False), ProteinSketches(unknown_residue="Z")]
    assert len({a, *others}) == 9 and all(a != x for x in others)
    for x in [a] + others:
        y = pickle.loads(pickle.dumps(x))
        assert y == x and hash(y) == hash(x) and repr(y) == repr(x) and type(y) is ProteinSketches and y.sketch_of("MKVLAAGW") == x.sketch_of("MKVLAAGW")
    assert (ProteinSketches.row, ProteinSketches.unit, ProteinSketches.per_contig) == ("gene", "sketches", "tables")
    o = ProteinSketches(11, 64, "gene", seed=2 ** 32 - 1, include_stop=True, strict=False, unknown_residue="Z").opts()
    assert (o.unit, o.k, o.size, o.seed, o.include_stop, o.strict, o.unknown_residue) == (_cabi.SKETCH_GENE, 11, 64, 2 ** 32 - 1, 1, 0, ord("Z"))
    assert ProteinSketches().opts().unit == _cabi.SKETCH_PROTEIN


def test_the_forms_of_classes():
    default = ProteinSketches()
    assert list(default.classes) == ref.default_classes("X") and list(default.opts().classes) == ref.default_classes("X")
    assert list(ProteinSketches(unknown_residue="Z").classes) == ref.default_classes("Z")
    red = ProteinSketches(classes=REDUCED)
    assert list(red.classes) == ref.classes_of(REDUCED) and list(red.opts().classes) == ref.classes_of(REDUCED)
    assert red.classes[ord("L")] == red.classes[ord("M")] == 0 and red.classes[ord("H")] == 9 and red.classes[ord("X")] == 255 and red.classes[ord("B")] == 255
    table = ref.classes_of(REDUCED)
    for form in (bytes(table), bytearray(table), list(table), tuple(table), np.array(table, np.uint8), iter(REDUCED), list(REDUCED)):
        assert ProteinSketches(classes=form) == red
    # a caller-given table decides alone: X is a letter like any other when the table names it
    assert ProteinSketches(1, 4, classes=("X", "M")).sketch_of("MXB")[1] == 2
    # two proteins that differ inside the classes get one sketch
    assert red.sketch_of("MKVLSTDEAGH") == red.sketch_of("LRIMTSEDAGH") != default.sketch_of("MKVLSTDEAGH")
    with pytest.raises(ValueError, match="named twice"):
        ProteinSketches(classes=("LVIM", "CL"))
    with pytest.raises(ValueError, match="128"):
        ProteinSketches(classes=bytes(127))
    with pytest.raises(ValueError, match="0 .. 254"):
        ProteinSketches(classes=[300] * 128)
    with pytest.raises(ValueError, match="ASCII"):
        ProteinSketches(classes=("é",))
    with pytest.raises(TypeError, match="classes"):
        ProteinSketches(classes="LVIM")
    with pytest.raises(TypeError, match="classes"):
        ProteinSketches(classes=("LVIM", 3))


def test_header_declares_the_functions_and_the_rule():
    text = open(os.path.join(ROOT, "include", "pyrodigal_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("pga_sketch_proteins", "pga_sketch_pairs"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code) and name in _cabi.EXPORTS
    assert "typedef struct pga_sketch_opts" in code
    for constant in ("0x9E3779B97F4A7C15", "0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "0xE220A8397B1DCDAF", "0x7110541CBD8EE6D7"):
        assert constant in text
    assert (ref.GOLDEN, ref.MUL1, ref.MUL2) == (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB)


def test_sketch_opts_mirror_matches_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    fields = ("unit", "k", "size", "seed", "include_stop", "strict", "unknown_residue", "_pad", "classes")
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "pyrodigal_amd.h"
int main(void) {
    printf("%%zu %%zu", sizeof(pga_sketch_opts), sizeof(((pga_sketch_opts*)0)->classes));
    %s
    printf(" %%d %%d\\n", PGA_SKETCH_PROTEIN, PGA_SKETCH_GENE);
    return 0;
}
""" % "\n    ".join('printf(" %%zu", offsetof(pga_sketch_opts, %s));' % f for f in fields))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _cabi.SketchOpts
    assert got == [ctypes.sizeof(S), 128] + [getattr(S, f).offset for f in fields] + [_cabi.SKETCH_PROTEIN, _cabi.SKETCH_GENE]
    assert ctypes.sizeof(S) == 160
