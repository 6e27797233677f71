"""Groups of identical proteins without a GPU (pga_group_proteins, ProteinGroups): what the constructor refuses, value
semantics, the digest in Python integers, the plain-Python restatement of the rule (tests/protein_groups_ref.py) on a hand-written
list, and the ctypes mirror of pga_group_opts against the header."""
import ctypes
import os
import pickle
import subprocess

import numpy as np
import pytest

from pyrodigal_amd import ProteinGroups, _cabi
from tests import protein_groups_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constructor_refusals():
    for bad in ("residue", "", None, 0, "Protein"):
        with pytest.raises(ValueError, match="unit"):
            ProteinGroups(bad)
    for name in ("include_stop", "strict"):
        with pytest.raises(TypeError, match=name):
            ProteinGroups(**{name: 1})
    with pytest.raises(TypeError, match="unknown_residue"):
        ProteinGroups(unknown_residue=88)
    for bad in ("", "XX", "é", "\x00"):
        with pytest.raises(ValueError, match="unknown_residue"):
            ProteinGroups(unknown_residue=bad)
    with pytest.raises(TypeError):
        ProteinGroups("protein", True)                           # (the options are keyword-only)


def test_value_semantics_and_pickling():
    a, b = ProteinGroups(), ProteinGroups("protein", include_stop=False, strict=True, unknown_residue="X")
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    others = [ProteinGroups("gene"), ProteinGroups(include_stop=True), ProteinGroups(strict=False), ProteinGroups(unknown_residue="Z")]
    assert len({a, *others}) == 5 and all(a != x for x in others)
    for x in [a] + others:
        y = pickle.loads(pickle.dumps(x))
        assert y == x and hash(y) == hash(x) and repr(y) == repr(x) and type(y) is ProteinGroups
    assert (ProteinGroups.row, ProteinGroups.unit, ProteinGroups.per_contig) == ("gene", "groups", "tables")
    o = ProteinGroups("gene", include_stop=True, strict=False, unknown_residue="Z").opts()
    assert (o.unit, o.include_stop, o.strict, o.unknown_residue) == (_cabi.GROUP_GENE, 1, 0, ord("Z"))
    assert ProteinGroups().opts().unit == _cabi.GROUP_PROTEIN


def test_digest_in_python_integers():
    M, b0, b1 = (1 << 61) - 1, 0x0123456789ABCDEF, 0x1BADB002C0FFEE11
    assert (ref.M, ref.B0, ref.B1) == (M, b0, b1)
    assert ProteinGroups.digest_of(b"") == (1, 1) == ref.digest(b"")
    assert ProteinGroups.digest_of(b"M") == ((b0 + 77) % M, (b1 + 77) % M) == ref.digest(b"M")
    assert ProteinGroups.digest_of("MK*") == ProteinGroups.digest_of(b"MK*") == ref.digest(b"MK*")
    want = tuple((((1 * b + 77) * b + 75) * b + 42) % M for b in (b0, b1))
    assert ref.digest(b"MK*") == want
    rng = np.random.default_rng(3)
    for n in (2, 63, 64, 65, 1000):
        s = rng.integers(33, 127, size=n).astype(np.uint8).tobytes()
        d = ProteinGroups.digest_of(s)
        assert d == ref.digest(s) and all(0 <= x < M for x in d)
        assert ProteinGroups.digest_of(s[:-1]) != d and ProteinGroups.digest_of(s + b"A") != d


def test_reference_groups_and_numbering_by_hand():
    strings = [b"MKV", b"", b"MKL", b"MKV", b"", b"MK", b"MKV", b"mkv", b"MKL"]
    group, reps, sizes = ref.groups_of(strings)
    assert group == [0, 1, 2, 0, 1, 3, 0, 4, 2]
    assert reps == [0, 1, 2, 5, 7] and sizes == [3, 2, 2, 1, 1]
    assert ref.groups_of([]) == ([], [], [])
    # the same strings in another order: numbering follows first appearance in the list passed
    group, reps, sizes = ref.groups_of(strings[::-1])
    assert group == [0, 1, 2, 3, 4, 2, 0, 4, 2] and reps == [0, 1, 2, 3, 4] and sizes == [2, 1, 3, 1, 2]


def test_reference_strings_by_hand():
    #            ATG AAA GTT TAA                  reverse complement of the same: TTA AAC TTT CAT
    seqs = [b"ccATGAAAGTTTAAcc", b"ggTTAAACTTTCATgg", b"AAGTTTAAccccATGA", b"ATGAANGTTTAA", b"GTGAAAGTTTAA"]
    circular = [False, False, True, False, False]
    tables = [11] * 5
    recs = [(0, 3, 14, 1, 0, 0), (1, 3, 14, -1, 0, 0), (2, 13, 24, 1, 0, 0), (3, 1, 12, 1, 0, 0), (4, 1, 12, 1, 0, 0), (4, 1, 12, 1, 1, 0)]
    prot = [ref.string_of(seqs, circular, r, "protein", tables) for r in recs]
    assert prot == [b"MKV", b"MKV", b"MKV", b"MXV", b"MKV", b"VKV"]
    assert [ref.string_of(seqs, circular, r, "protein", tables, include_stop=True) for r in recs[:2]] == [b"MKV*", b"MKV*"]
    assert ref.string_of(seqs, circular, recs[3], "protein", tables, strict=False, unknown_residue="Z") == b"MZV"
    gene = [ref.string_of(seqs, circular, r, "gene") for r in recs]
    assert gene == [b"ATGAAAGTTTAA"] * 3 + [b"ATGAANGTTTAA", b"GTGAAAGTTTAA", b"GTGAAAGTTTAA"]
    group, reps, sizes, digests, strings = ref.protein_groups_ref(seqs, circular, recs, "protein", tables)
    assert group.tolist() == [0, 0, 0, 1, 0, 2] and reps.tolist() == [0, 3, 5] and sizes.tolist() == [4, 1, 1]
    assert digests.dtype == np.int64 and digests.shape == (6, 2) and digests[0].tolist() == list(ProteinGroups.digest_of(b"MKV"))
    group, reps, sizes, digests, strings = ref.protein_groups_ref(seqs, circular, recs, "gene")
    assert group.tolist() == [0, 0, 0, 1, 2, 2] and reps.tolist() == [0, 3, 4] and sizes.tolist() == [3, 1, 2]
    empty = ref.protein_groups_ref(seqs, circular, [], "protein", tables)
    assert [x.shape for x in empty[:4]] == [(0,), (0,), (0,), (0, 2)]


def test_group_opts_mirror_matches_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "pyrodigal_amd.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %d %d\\n", sizeof(pga_group_opts), offsetof(pga_group_opts, unit), offsetof(pga_group_opts, include_stop),
           offsetof(pga_group_opts, strict), offsetof(pga_group_opts, unknown_residue), PGA_GROUP_PROTEIN, PGA_GROUP_GENE);
    return 0;
}
""")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    G = _cabi.GroupOpts
    assert got == [ctypes.sizeof(G), G.unit.offset, G.include_stop.offset, G.strict.offset, G.unknown_residue.offset,
                   _cabi.GROUP_PROTEIN, _cabi.GROUP_GENE]
