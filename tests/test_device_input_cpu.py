"""Sequences in device memory, the part that needs no device: `DeviceSequences` checks its arguments before any device call (a fake
object that only carries a `__cuda_array_interface__` dict stands in for a tensor), the alphabet forms, subsetting, and the numpy
restatement of the packing rule on hand-written cases."""
import numpy as np
import pytest

from pyrodigal_amd import _cabi
from pyrodigal_amd._cabi import DeviceSequences, normalise_alphabet
from tests.device_input_ref import pack_reference


class Fake:
    """Nothing but the interface dict: the pointer is never used here."""

    def __init__(self, shape, typestr="|u1", strides=None, ptr=0x7f0000001000):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}


@pytest.fixture(autouse=True)
def no_device_call(monkeypatch):
    """Every check here raises (or passes) without the library: loading it would be a device call's first step."""
    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_cabi, "load", boom)


def test_reexported_from_the_package():
    import pyrodigal_amd
    assert pyrodigal_amd.DeviceSequences is DeviceSequences and "DeviceSequences" in pyrodigal_amd.__all__


def test_bad_dtype():
    for t in ("<f4", "<u2", "<i2", "<u4", ">i4", "|b1"):
        with pytest.raises(TypeError, match="dtype"):
            DeviceSequences(Fake((10,), t), [10], alphabet="ACGT")
    with pytest.raises(TypeError, match="__cuda_array_interface__"):
        DeviceSequences(np.zeros(10, np.uint8), [10])


def test_accepted_dtypes():
    for t, eb in (("|u1", 1), ("|i1", 1), ("<i4", 4), ("<i8", 8)):
        ds = DeviceSequences(Fake((3, 7), t), [7, 0, 2], alphabet="ACGT")
        assert ds.elem_bytes == eb and ds.n_elems == 21 and list(ds.offsets) == [0, 7, 14] and ds.total == 9 and len(ds) == 3


def test_three_dimensions():
    with pytest.raises(ValueError, match="1-D or 2-D"):
        DeviceSequences(Fake((2, 3, 4)), [1, 1])
    with pytest.raises(ValueError, match="1-D or 2-D"):
        DeviceSequences(Fake(()), [])


def test_last_dimension_not_contiguous():
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        DeviceSequences(Fake((4, 8), "<i8", strides=(128, 16)), [8, 8, 8, 8], alphabet="ACGT")
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        DeviceSequences(Fake((8,), "|u1", strides=(2,)), [8])
    # rows may lie apart (a view of the first columns of a wider tensor): the last dimension is what must be dense
    ds = DeviceSequences(Fake((4, 8), "<i8", strides=(128, 8)), [8, 3, 0, 8], alphabet="ACGT")
    assert list(ds.offsets) == [0, 16, 32, 48] and ds.n_elems == 56


def test_length_beyond_the_row():
    with pytest.raises(ValueError, match="sequence 1.*11.*10 columns"):
        DeviceSequences(Fake((2, 10)), [10, 11])
    with pytest.raises(ValueError, match="3 entries for 2 rows"):
        DeviceSequences(Fake((2, 10)), [1, 2, 3])


def test_negative_length():
    with pytest.raises(ValueError, match="sequence 1.*negative"):
        DeviceSequences(Fake((2, 10)), [3, -1])
    with pytest.raises(ValueError, match="negative"):
        DeviceSequences(Fake((20,)), [3, -1])


def test_offsets_beyond_the_data():
    with pytest.raises(ValueError, match="sequence 1"):
        DeviceSequences(Fake((20,)), [5, 6], offsets=[0, 15])
    with pytest.raises(ValueError, match="sequence 0"):
        DeviceSequences(Fake((20,)), [5, 6], offsets=[-1, 0])
    with pytest.raises(ValueError, match="sequence 2"):
        DeviceSequences(Fake((20,)), [10, 10, 1])                     # back to back: the third starts at the end
    with pytest.raises(ValueError, match="offsets has 1 entries"):
        DeviceSequences(Fake((20,)), [5, 6], offsets=[0])
    ds = DeviceSequences(Fake((20,)), [5, 6, 0], offsets=[14, 14, 20])      # overlapping ranges and an empty one at the very end are fine
    assert ds.total == 11


def test_alphabet_entry_that_is_no_letter():
    for bad in ("ACG*", b"ACGT-", {0: "A", 1: "1"}, "AC T"):
        with pytest.raises(ValueError, match="not an ASCII letter"):
            DeviceSequences(Fake((4,)), [4], alphabet=bad)
    with pytest.raises(ValueError, match="at most 256"):
        normalise_alphabet("A" * 257)


def test_dict_id_of_256_or_above():
    with pytest.raises(ValueError, match="256"):
        DeviceSequences(Fake((4,), "<i4"), [4], alphabet={0: "A", 256: "C"})
    with pytest.raises(ValueError, match="-1"):
        DeviceSequences(Fake((4,), "<i4"), [4], alphabet={-1: "A"})


def test_token_ids_need_an_alphabet():
    for t in ("<i4", "<i8"):
        with pytest.raises(ValueError, match="alphabet"):
            DeviceSequences(Fake((4,), t), [4])


def test_alphabet_normalisation():
    assert normalise_alphabet(None) is None
    assert normalise_alphabet("ACGTn") == b"ACGTn"
    assert normalise_alphabet(b"acgt") == b"acgt"
    assert normalise_alphabet({3: "G", 0: "A", 5: b"t"}) == b"ANNGNt"
    assert normalise_alphabet({}) == b""
    assert normalise_alphabet({255: "A"}) == b"N" * 255 + b"A"
    assert normalise_alphabet(bytearray(b"AC")) == b"AC"
    with pytest.raises(ValueError, match="one letter"):
        normalise_alphabet({0: "AC"})


def test_lengths_and_offsets_go_through_tolist():
    class Tensorish:
        def __init__(self, v):
            self.v = v

        def tolist(self):
            return list(self.v)

    ds = DeviceSequences(Fake((30,)), Tensorish([3, 4]), offsets=np.array([10, 20]))
    assert list(ds.lengths) == [3, 4] and list(ds.offsets) == [10, 20] and ds.lengths.dtype == np.int64
    with pytest.raises(TypeError, match="integers"):
        DeviceSequences(Fake((30,)), [3.5])


def test_stream_forms():
    class S:
        cuda_stream = 0x1234

    assert DeviceSequences(Fake((4,)), [4]).stream == 0                # not a torch tensor: the null stream
    assert DeviceSequences(Fake((4,)), [4], stream=S()).stream == 0x1234
    assert DeviceSequences(Fake((4,)), [4], stream=77).stream == 77
    with pytest.raises(TypeError, match="stream"):
        DeviceSequences(Fake((4,)), [4], stream="null")


def test_subsetting_shares_the_memory():
    data = Fake((5, 9), "<i4")
    ds = DeviceSequences(data, [9, 0, 4, 1, 7], alphabet="ACGT", stream=5)
    sub = ds[1:4]
    assert isinstance(sub, DeviceSequences) and sub.data is data and sub.ptr == ds.ptr and sub.n_elems == ds.n_elems
    assert list(sub.offsets) == [9, 18, 27] and list(sub.lengths) == [0, 4, 1] and sub.total == 5 and len(sub) == 3
    assert sub.alphabet == b"ACGT" and sub.stream == 5 and sub.elem_bytes == 4
    t = ds.take([4, 4, 0])
    assert list(t.offsets) == [36, 36, 0] and list(t.lengths) == [7, 7, 9] and t.total == 23
    assert list(ds[::-1].offsets) == [36, 27, 18, 9, 0]
    assert len(ds[2:2]) == 0 and ds[2:2].total == 0
    one = ds[-1]
    assert len(one) == 1 and list(one.lengths) == [7]
    with pytest.raises(IndexError):
        ds.take([5])
    assert list(ds.lengths) == [9, 0, 4, 1, 7]                         # the parent is left as it was


def test_host_entry_points_refuse_device_input():
    from pyrodigal_amd import lib
    ds = DeviceSequences(Fake((4,)), [4])
    gf = lib.GeneFinder(meta=True)
    single = lib.GeneFinder()
    for call in (lambda: gf.find_genes(ds), lambda: single.train(ds), lambda: single.train_batch(ds), lambda: single.select_translation_table(ds)):
        with pytest.raises(TypeError, match="find_genes_batch"):
            call()


def test_pack_reference_by_hand():
    letters = np.frombuffer(b"ACGTNacgtn??", np.uint8)
    assert pack_reference(letters, [0, 4, 10, 2], [4, 6, 0, 3], None) == [b"ACGT", b"Nacgtn", b"", b"GTN"]
    tok = np.array([0, 1, 2, 3, 4, -1, 5, 255, 256, 1 << 31, -(1 << 63), 3], np.int64)
    assert pack_reference(tok, [0, 5], [5, 7], b"ACGTn") == [b"ACGTn", b"NNNNNNT"]
    tok32 = np.array([[0, 1, 9, 9], [3, -1, 2, 9]], np.int32)            # rows of a padded tensor: offsets are flat element indices
    assert pack_reference(tok32, [0, 4], [2, 3], b"ACGT") == [b"AC", b"TNG"]
    signed = np.array([-1, 0, 1], np.int8)                               # 1-byte elements are unsigned: -1 is 255
    assert pack_reference(signed, [0], [3], b"AC") == [b"NAC"]
    assert pack_reference(signed, [0], [3], b"A" * 255 + b"T") == [b"TAA"]
    assert pack_reference(signed, [0], [3], None) == [b"\xff\x00\x01"]
    assert pack_reference(letters, [3, 3, 0], [2, 2, 1], None) == [b"TN", b"TN", b"A"]       # overlapping, repeated, reordered
    with pytest.raises(ValueError):
        pack_reference(letters, [8], [5], None)
    with pytest.raises(ValueError):
        pack_reference(tok, [0], [1], None)
