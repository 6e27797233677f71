"""Per-base gene labels without a GPU: the numpy restatement of the rule (tests/base_labels_ref.py) pinned to contigs worked out by
hand, the four presets over all 256 bytes, what the BaseLabels constructor checks, and the export."""
import os
import pickle

import numpy as np
import pytest

from tests.base_labels_ref import PRESETS, base_labels_ref, preset_map, raw_labels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (length, [(begin, end, strand, partial_begin, partial_end)], the raw byte of every base) -- each worked out by hand from the rule
HAND = {
    "forward": (12, [(2, 10, 1, 0, 0)], "00 41 42 44 01 02 04 81 82 84 00 00"),
    "reverse": (12, [(2, 10, -1, 0, 0)], "00 a0 90 88 20 10 08 60 50 48 00 00"),
    "forward, partial_begin: no start codon": (9, [(1, 9, 1, 1, 0)], "01 02 04 01 02 04 81 82 84"),
    "forward, partial_end: no stop codon": (9, [(1, 9, 1, 0, 1)], "41 42 44 01 02 04 01 02 04"),
    "reverse, partial_begin: no stop codon": (9, [(1, 9, -1, 1, 0)], "20 10 08 20 10 08 60 50 48"),
    "reverse, partial_end: no start codon": (9, [(1, 9, -1, 0, 1)], "a0 90 88 20 10 08 20 10 08"),
    "a 4-base same-strand overlap": (15, [(1, 9, 1, 0, 0), (6, 14, 1, 0, 0)], "41 42 44 01 02 45 c3 c6 85 02 04 81 82 84 00"),
    "an opposite-strand overlap": (15, [(1, 9, 1, 0, 0), (7, 15, -1, 0, 0)], "41 42 44 01 02 04 a1 92 8c 20 10 08 60 50 48"),
    "a position under three genes": (15, [(1, 9, 1, 0, 0), (5, 13, 1, 0, 0), (6, 14, -1, 0, 0)],
                                     "41 42 44 01 43 e6 d5 8b a6 14 89 e2 d4 48 00"),
    "across the origin, the start codon straddles it": (12, [(11, 19, 1, 0, 0)], "44 01 02 04 81 82 84 00 00 00 41 42"),
    "across the origin, the stop codon straddles it": (12, [(5, 13, 1, 0, 0)], "84 00 00 00 41 42 44 01 02 04 81 82"),
    "reverse across the origin, its start codon straddles it": (12, [(6, 14, -1, 0, 0)], "50 48 00 00 00 a0 90 88 20 10 08 60"),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_the_restatement_on_contigs_worked_out_by_hand(name):
    length, recs, want = HAND[name]
    want = bytes.fromhex(want)
    assert len(want) == length
    records = [(0,) + r for r in recs]
    assert raw_labels(length, records).tobytes() == want
    assert raw_labels(length, records[::-1]).tobytes() == want                     # a union: the order does not matter


def test_the_tensors_of_the_restatement():
    lengths = [12, 0, 9]
    records = [(0, 2, 10, 1, 0, 0), (2, 1, 9, -1, 1, 0)]
    frame = preset_map("frame")
    padded, off = base_labels_ref(lengths, records, frame, pad=-100, width=13)
    assert off.tolist() == [0, 12, 12, 21] and padded.shape == (3, 13) and padded.dtype == np.int64
    assert padded[0].tolist() == [0, 1, 2, 3, 1, 2, 3, 1, 2, 3, 0, 0, -100]
    assert padded[1].tolist() == [-100] * 13
    assert padded[2].tolist() == [6, 5, 4, 6, 5, 4, 6, 5, 4] + [-100] * 4
    ragged, _ = base_labels_ref(lengths, records, frame, layout="ragged", dtype=np.uint8)
    assert ragged.dtype == np.uint8 and ragged.tolist() == padded[0][:12].tolist() + padded[2][:9].tolist()


def test_presets_over_all_bytes():
    from pyrodigal_amd import BaseLabels
    from pyrodigal_amd._cabi import label_class_map
    for name in PRESETS:
        want = preset_map(name)
        assert list(label_class_map(name)) == want.tolist(), name
        assert list(BaseLabels(name, pad=255, dtype="int32").class_map) == want.tolist()
    # and by their definition, written out once more
    for raw in range(256):
        fwd, rev = [raw >> k & 1 for k in range(3)], [raw >> k & 1 for k in range(3, 6)]
        assert preset_map("raw")[raw] == raw
        assert preset_map("coding")[raw] == int(raw & 0x3f != 0)
        assert preset_map("strand")[raw] == (1 if any(fwd) else 0) + (2 if any(rev) else 0)
        n = sum(fwd) + sum(rev)
        assert preset_map("frame")[raw] == (0 if n == 0 else 7 if n > 1 else 1 + (fwd + rev).index(1))
    assert preset_map("frame")[0xc0] == 0 and preset_map("frame")[0x41] == 1 and preset_map("frame")[0xa0] == 6


def test_base_labels_validation():
    from pyrodigal_amd import BaseLabels
    d = BaseLabels()
    assert (d.classes, d.pad, d.dtype, d.layout, d.elem_bytes) == ("frame", -100, "int64", "padded", 8)
    assert BaseLabels("raw", dtype="int32").pad == -100
    with pytest.raises(ValueError, match="256"):
        BaseLabels(list(range(255)))
    with pytest.raises(ValueError, match="256"):
        BaseLabels(list(range(257)))
    with pytest.raises(ValueError, match="does not fit uint8"):
        BaseLabels([0] * 255 + [256], dtype="uint8", layout="ragged")
    with pytest.raises(ValueError, match="does not fit uint8"):
        BaseLabels("raw", dtype="uint8", pad=-1)
    with pytest.raises(ValueError, match="does not fit int32"):
        BaseLabels([1 << 31] + [0] * 255, dtype="int32")
    with pytest.raises(ValueError, match="does not fit int32"):
        BaseLabels("frame", dtype="int32", pad=-(1 << 31) - 1)
    with pytest.raises(ValueError, match="needs `pad`"):
        BaseLabels("frame", dtype="uint8")
    assert BaseLabels("frame", dtype="uint8", layout="ragged").pad == 0             # the ragged layout has no pad
    assert BaseLabels("frame", dtype="uint8", pad=255).pad == 255
    with pytest.raises(ValueError, match="one of"):
        BaseLabels("phase")
    with pytest.raises(ValueError, match="layout"):
        BaseLabels("frame", layout="packed")
    with pytest.raises(ValueError, match="dtype"):
        BaseLabels("frame", dtype="int16")
    with pytest.raises(TypeError):
        BaseLabels([0.5] * 256)
    assert BaseLabels("coding", dtype=np.int32).dtype == "int32"
    o = BaseLabels("strand", dtype="int32", pad=-1).opts(7, 9)
    assert (o.elem_bytes, o.layout, o.row_width, o.row_stride, o.pad) == (4, 1, 7, 9, -1)
    assert list(o.class_map) == preset_map("strand").tolist()


def test_base_labels_hash_equality_pickle():
    from pyrodigal_amd import BaseLabels
    a, b = BaseLabels("frame", dtype="int32"), BaseLabels("frame", dtype="int32")
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    assert a != BaseLabels("frame", dtype="int64") and a != BaseLabels("frame", dtype="int32", layout="ragged")
    assert a != BaseLabels("frame", dtype="int32", pad=-1) and a != BaseLabels("strand", dtype="int32") and a != "frame"
    for spec in (a, BaseLabels(list(range(256))[::-1], dtype="uint8", layout="ragged"), BaseLabels("raw", dtype="uint8", pad=255)):
        back = pickle.loads(pickle.dumps(spec))
        assert back == spec and hash(back) == hash(spec) and back.class_map == spec.class_map
        assert (back.pad, back.dtype, back.layout, back.classes) == (spec.pad, spec.dtype, spec.layout, spec.classes)
        assert "BaseLabels" in repr(back)


def test_export_is_named_and_declared():
    import pyrodigal_amd
    from pyrodigal_amd import _cabi
    assert "pga_label_bases" in _cabi.EXPORTS
    header = open(os.path.join(ROOT, "include", "pyrodigal_amd.h")).read()
    assert "int pga_label_bases(pga_ctx*, const pga_batch*, int64_t n_genes, const pga_gene*" in header
    assert "typedef struct pga_label_opts" in header and "class_map[256]" in header
    assert pyrodigal_amd.BaseLabels is _cabi.BaseLabels and pyrodigal_amd.DeviceLabels is _cabi.DeviceLabels
    assert "BaseLabels" in pyrodigal_amd.__all__
    assert hasattr(_cabi.Context, "label_bases")
