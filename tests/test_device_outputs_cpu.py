"""The device-tensor outputs, the part that needs no device: every `out=` a caller may hand over is checked before any library call,
so a fake object that only carries a `__cuda_array_interface__` dict stands in for a tensor (as in test_device_input_cpu.py).  The
refusals are pinned word for word, per caller: the callers share one reader of the interface, and each keeps its own words.  Also
here: `gene_begin`, and pickles of the seven rules made before the rules shared one `__reduce__`."""
import os
import pickle

import numpy as np
import pytest

from pyrodigal_amd import _cabi
from pyrodigal_amd._cabi import (BaseLabels, DeviceSketches, GeneWindows, KmerCounts, ProteinGroups, ProteinSketches, ProteinTokens,
                                 StartCandidates)


class Fake:
    """Nothing but the interface dict: the pointer is never used here."""

    def __init__(self, shape, typestr="<i8", strides=None, ptr=0x7f0000001000):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}


@pytest.fixture(autouse=True)
def no_device_call(monkeypatch):
    """Every check here raises without the library: loading it would be a device call's first step."""
    def boom():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_cabi, "load", boom)


LENS = np.array([2, 0, 3], np.int64)            # three rows; G = 3
GENES = np.zeros(3, _cabi.GENE_DTYPE)
GENES["contig"] = (0, 0, 2)
TABLES = [11, 11, 11]
F8 = lambda *shape, **kw: Fake(shape, "<i8", **kw)      # noqa: E731
F4 = lambda *shape, **kw: Fake(shape, "<i4", **kw)      # noqa: E731
FF = lambda *shape, **kw: Fake(shape, "<f4", **kw)      # noqa: E731

TOKENS = ProteinTokens(_cabi.AMINO_ACIDS + "*X", layout="padded")
RAGGED = ProteinTokens(_cabi.AMINO_ACIDS + "*X", layout="ragged")
COUNTS = KmerCounts(1, rows="gene")                     # four bins
GROUPS = ProteinGroups()
SKETCHES = ProteinSketches(3, 2)                        # size = 2
STARTS = StartCandidates(("total", "sscore"), index_dtype="int64", layout="padded", pad=-1, score_pad=0.0)      # F = 2
STARTS_RAGGED = StartCandidates(("total", "sscore"), index_dtype="int64")


def device_output(out, spec=TOKENS):
    return _cabi._device_output(spec, out, None, 0, LENS, 5, "gene", "tokens")


def counts(out):
    return _cabi.counts_into(None, None, None, 0, 3, GENES, COUNTS, out)


def groups(out):
    return _cabi.groups_into(None, None, None, 0, 3, GENES, TABLES, GROUPS, out)


def sketches(out):
    return _cabi.sketches_into(None, None, None, 0, 3, GENES, TABLES, SKETCHES, out)


def starts(out, spec=STARTS):
    return _cabi._start_outputs(spec, out, None, 0, LENS)


def compare(pairs, out):
    d = DeviceSketches(F8(3, 2), F8(3), None, None, SKETCHES, 0, 3)
    return d.compare(pairs, out)


GOOD_STARTS = (F8(3, 3), F8(3, 3), FF(3, 3, 2))
CASES = {
    # ---- _device_output (tokens, labels, windows) ----
    "rows/type": lambda: device_output(np.zeros((3, 3), np.int64)),
    "rows/typestr": lambda: device_output(F4(3, 3)),
    "rows/rank": lambda: device_output(F8(9)),
    "rows/rank-ragged": lambda: device_output(F8(3, 3), RAGGED),
    "rows/rows": lambda: device_output(F8(2, 3)),
    "rows/columns": lambda: device_output(F8(3, 2)),
    "rows/elements-ragged": lambda: device_output(F8(4), RAGGED),
    "rows/last-dimension": lambda: device_output(F8(3, 3, strides=(48, 16))),
    "rows/row-stride": lambda: device_output(F8(3, 3, strides=(28, 8))),
    # ---- counts_into ----
    "counts/type": lambda: counts(np.zeros((3, 4), np.int32)),
    "counts/typestr": lambda: counts(F8(3, 4)),
    "counts/rank": lambda: counts(F4(12)),
    "counts/rows": lambda: counts(F4(2, 4)),
    "counts/columns": lambda: counts(F4(3, 3)),
    "counts/last-dimension": lambda: counts(F4(3, 4, strides=(32, 8))),
    "counts/row-stride": lambda: counts(F4(3, 4, strides=(18, 4))),
    "counts/row-overlap": lambda: counts(F4(3, 4, strides=(8, 4))),
    # ---- groups_into ----
    "groups/type": lambda: groups((np.zeros(3, np.int64), None, None, None)),
    "groups/typestr": lambda: groups((F4(3), None, None, None)),
    "groups/rank": lambda: groups((F8(3, 1), None, None, None)),
    "groups/rows": lambda: groups((F8(3), F8(2), None, None)),
    "groups/columns": lambda: groups((F8(3), None, None, F8(3, 1))),
    "groups/contiguous": lambda: groups((F8(3, strides=(16,)), None, None, None)),
    "groups/row-stride": lambda: groups((F8(3), None, None, F8(3, 2, strides=(20, 8)))),
    "groups/tuple": lambda: groups((F8(3), F8(3), F8(3))),
    "groups/none": lambda: groups((None, F8(3), F8(3), F8(3, 2))),
    # ---- sketches_into ----
    "sketches/type": lambda: sketches((np.zeros((3, 2), np.int64), F8(3), None)),
    "sketches/typestr": lambda: sketches((F8(3, 2), F4(3), None)),
    "sketches/rank": lambda: sketches((F8(6), F8(3), None)),
    "sketches/rows": lambda: sketches((F8(2, 2), F8(3), None)),
    "sketches/columns": lambda: sketches((F8(3, 1), F8(3), None)),
    "sketches/contiguous": lambda: sketches((F8(3, 2, strides=(16, 16)), F8(3), None)),
    "sketches/row-stride": lambda: sketches((F8(3, 2, strides=(20, 8)), F8(3), None)),
    "sketches/tuple": lambda: sketches((F8(3, 2), F8(3))),
    "sketches/none": lambda: sketches((F8(3, 2), None, None)),
    # ---- _start_outputs ----
    "starts/type": lambda: starts((np.zeros((3, 3), np.int64),) + GOOD_STARTS[1:]),
    "starts/typestr": lambda: starts((GOOD_STARTS[0], F4(3, 3), GOOD_STARTS[2])),
    "starts/typestr-scores": lambda: starts(GOOD_STARTS[:2] + (Fake((3, 3, 2), "<f8"),)),
    "starts/rank": lambda: starts((F8(9),) + GOOD_STARTS[1:]),
    "starts/rank-scores": lambda: starts(GOOD_STARTS[:2] + (FF(3, 3),)),
    "starts/fields": lambda: starts(GOOD_STARTS[:2] + (FF(3, 3, 3),)),
    "starts/rows": lambda: starts((F8(2, 3),) + GOOD_STARTS[1:]),
    "starts/columns": lambda: starts((F8(3, 2),) + GOOD_STARTS[1:]),
    "starts/columns-differ": lambda: starts((GOOD_STARTS[0], F8(3, 4), GOOD_STARTS[2])),
    "starts/candidates-ragged": lambda: starts((F8(4), F8(5), FF(5, 2)), STARTS_RAGGED),
    "starts/last-dimension": lambda: starts(GOOD_STARTS[:2] + (FF(3, 3, 2, strides=(48, 16, 8)),)),
    "starts/candidates": lambda: starts((F8(3, 3, strides=(48, 16)),) + GOOD_STARTS[1:]),
    "starts/row-stride": lambda: starts((F8(3, 3, strides=(28, 8)),) + GOOD_STARTS[1:]),
    "starts/tuple": lambda: starts(GOOD_STARTS[:2]),
    "starts/none": lambda: starts((GOOD_STARTS[0], None, GOOD_STARTS[2])),
    # ---- DeviceSketches.compare ----
    "compare/type": lambda: compare(np.zeros((4, 2), np.int64), (F8(4), F8(4))),
    "compare/typestr": lambda: compare(F4(4, 2), (F8(4), F8(4))),
    "compare/rank": lambda: compare(F8(8), (F8(4), F8(4))),
    "compare/pair-columns": lambda: compare(F8(4, 3), (F8(4), F8(4))),
    "compare/contiguous": lambda: compare(F8(4, 2, strides=(32, 8)), (F8(4), F8(4))),
    "compare/rows": lambda: compare(F8(4, 2), (F8(3), F8(4))),
    "compare/out-typestr": lambda: compare(F8(4, 2), (F8(4), F4(4))),
    "compare/tuple": lambda: compare(F8(4, 2), (F8(4),)),
    "compare/none": lambda: compare(F8(4, 2), (F8(4), None)),
}

# what the code said before the callers shared `_device_array`: (exception type, the whole message)
EXPECTED = {
    'rows/type': (TypeError, "out must have a __cuda_array_interface__ (a device tensor or array), not 'ndarray'"),
    'rows/typestr': (TypeError, 'out has dtype <i4: the rule writes int64 (<i8)'),
    'rows/rank': (ValueError, 'the padded layout needs a [3, W] tensor, not one of shape (9,)'),
    'rows/rank-ragged': (ValueError, 'the ragged layout needs a 1-D tensor, not one of shape (3, 3)'),
    'rows/rows': (ValueError, 'the padded layout needs a [3, W] tensor, not one of shape (2, 3)'),
    'rows/columns': (ValueError, 'out has 2 columns: gene 2 has 3 tokens'),
    'rows/elements-ragged': (ValueError, 'out has 4 elements: the genes have 5 tokens'),
    'rows/last-dimension': (ValueError, 'the last dimension of out is not contiguous'),
    'rows/row-stride': (ValueError, 'the rows of out do not lie a whole, positive number of elements apart'),
    'counts/type': (TypeError, "out must have a __cuda_array_interface__ (a device tensor or array), not 'ndarray'"),
    'counts/typestr': (TypeError, 'out has dtype <i8: the rule writes int32 (<i4)'),
    'counts/rank': (ValueError, 'the counts need a [3, S] tensor, not one of shape (12,)'),
    'counts/rows': (ValueError, 'the counts need a [3, S] tensor, not one of shape (2, 4)'),
    'counts/columns': (ValueError, 'out has 3 columns: the rule has 4 bins'),
    'counts/last-dimension': (ValueError, 'the last dimension of out is not contiguous'),
    'counts/row-stride': (ValueError, "the rows of out do not lie a whole number of elements apart, at least a row's width"),
    'counts/row-overlap': (ValueError, "the rows of out do not lie a whole number of elements apart, at least a row's width"),
    'groups/type': (TypeError, "out: group must have a __cuda_array_interface__ (a device tensor or array), not 'ndarray'"),
    'groups/typestr': (TypeError, 'out: group has dtype <i4: these tensors are int64 (<i8)'),
    'groups/rank': (ValueError, 'out: group needs shape [3] or longer, not [3, 1]'),
    'groups/rows': (ValueError, 'out: representatives needs shape [3] or longer, not [2]'),
    'groups/columns': (ValueError, 'out: digests needs shape [3, 2], not [3, 1]'),
    'groups/contiguous': (ValueError, 'out: group is not contiguous'),
    'groups/row-stride': (ValueError, 'out: digests is not contiguous'),
    'groups/tuple': (ValueError, 'out must be (group, representatives, sizes, digests), 3 objects were given'),
    'groups/none': (TypeError, 'out: group is required'),
    'sketches/type': (TypeError, "out: sketches must have a __cuda_array_interface__ (a device tensor or array), not 'ndarray'"),
    'sketches/typestr': (TypeError, 'out: counts has dtype <i4: these tensors are int64 (<i8)'),
    'sketches/rank': (ValueError, 'out: sketches needs shape [3, 2], not [6]'),
    'sketches/rows': (ValueError, 'out: sketches needs shape [3, 2], not [2, 2]'),
    'sketches/columns': (ValueError, 'out: sketches needs shape [3, 2], not [3, 1]'),
    'sketches/contiguous': (ValueError, 'out: sketches is not contiguous'),
    'sketches/row-stride': (ValueError, 'out: sketches is not contiguous'),
    'sketches/tuple': (ValueError, 'out must be (sketches, counts, windows), 2 objects were given'),
    'sketches/none': (TypeError, 'out: counts is required'),
    'starts/type': (TypeError, "positions must have a __cuda_array_interface__ (a device tensor or array), not 'ndarray'"),
    'starts/typestr': (TypeError, 'types has dtype <i4: the rule writes <i8'),
    'starts/typestr-scores': (TypeError, 'scores has dtype <f8: the rule writes <f4'),
    'starts/rank': (ValueError, 'positions must be [3, W], not of shape (9,)'),
    'starts/rank-scores': (ValueError, 'scores must be [3, W, 2], not of shape (3, 3)'),
    'starts/fields': (ValueError, 'scores must be [3, W, 2], not of shape (3, 3, 3)'),
    'starts/rows': (ValueError, 'the padded layout needs 3 rows: positions has 2'),
    'starts/columns': (ValueError, 'positions has 2 columns: gene 2 has 3 candidates'),
    'starts/columns-differ': (ValueError, 'types has 4 columns a stride of 4 apart: positions has 3, 3 apart'),
    'starts/candidates-ragged': (ValueError, 'positions has 4 candidates: the genes have 5'),
    'starts/last-dimension': (ValueError, 'the last dimension of scores is not contiguous'),
    'starts/candidates': (ValueError, 'the candidates of positions are not contiguous'),
    'starts/row-stride': (ValueError, 'the rows of positions do not lie a whole, positive number of candidates apart'),
    'starts/tuple': (TypeError, 'out must be a (positions, types, scores) triple of device arrays'),
    'starts/none': (TypeError, "types must have a __cuda_array_interface__ (a device tensor or array), not 'NoneType'"),
    'compare/type': (TypeError, "pairs must have a __cuda_array_interface__ (a device tensor or array), not 'ndarray'"),
    'compare/typestr': (TypeError, 'out: pairs has dtype <i4: these tensors are int64 (<i8)'),
    'compare/rank': (ValueError, 'pairs needs shape [P, 2], not [8]'),
    'compare/pair-columns': (ValueError, 'pairs needs shape [P, 2], not [4, 3]'),
    'compare/contiguous': (ValueError, 'out: pairs is not contiguous'),
    'compare/rows': (ValueError, 'out: shared needs shape [4] or longer, not [3]'),
    'compare/out-typestr': (TypeError, 'out: union has dtype <i4: these tensors are int64 (<i8)'),
    'compare/tuple': (ValueError, 'out must be (shared, union), 1 objects were given'),
    'compare/none': (TypeError, 'out: union is required'),
}


def test_every_case_is_pinned():
    assert sorted(CASES) == sorted(EXPECTED)


@pytest.mark.parametrize("case", sorted(CASES))
def test_refusal(case):
    kind, message = EXPECTED[case]
    with pytest.raises(kind) as e:
        CASES[case]()
    assert type(e.value) is kind and str(e.value) == message


def test_good_outputs_pass_the_checks():
    out, stream, _, width, stride, n_out = device_output(F8(3, 4, strides=(48, 8)))
    assert (width, stride, n_out) == (4, 6, 16) and stream is None
    assert device_output(F8(7), RAGGED)[3:] == (0, 0, 7)
    out, stream, ptrs, width, stride, n_elems = starts(GOOD_STARTS)
    assert (width, stride, n_elems) == (3, 3, [9, 9, 18]) and [p.value for p in ptrs] == [0x7f0000001000] * 3
    assert starts((F8(5), F8(6), FF(5, 2)), STARTS_RAGGED)[3:] == (0, 0, [5, 6, 10])


def test_gene_begin():
    genes = np.zeros(5, _cabi.GENE_DTYPE)
    genes["contig"] = (0, 0, 2, 2, 3)
    assert _cabi._gene_begin(genes, 4).tolist() == [0, 2, 2, 4, 5] and _cabi._gene_begin(genes, 4).dtype == np.int64
    genes["contig"] = (0, 2, 1, 2, 3)
    assert _cabi._gene_begin(genes, 4) is None
    assert _cabi._gene_begin(genes[:0], 3).tolist() == [0, 0, 0, 0]


RULES = {
    "ProteinTokens": ProteinTokens({"A": 7, "*": 3}, unknown=1, bos=2, eos=None, pad=9, dtype="int32", layout="ragged", max_length=40,
                                   include_stop=True, strict=False, unknown_residue="Z"),
    "BaseLabels": BaseLabels("strand", pad=5, dtype="uint8", layout="padded"),
    "GeneWindows": GeneWindows(("start", -30), ("start", 30), unit="codon", bos=70, pad=71, dtype="int32", max_length=12),
    "KmerCounts": KmerCounts(3, rows="contig_genes", step=3, bins=KmerCounts.codon_bins(4)),
    "ProteinGroups": ProteinGroups("gene", include_stop=True, strict=False, unknown_residue="Z"),
    "ProteinSketches": ProteinSketches(4, 16, "protein", seed=7, include_stop=True, strict=False, unknown_residue="Z"),
    "StartCandidates": StartCandidates(("sscore", "total"), dtype="float64", index_dtype="int32", layout="padded", pad=-1,
                                       score_pad=float("nan")),
}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_output_rules")      # pickles of RULES (protocol 2)


@pytest.mark.parametrize("name", sorted(RULES))
def test_old_pickles_load_equal(name):
    rule = RULES[name]
    with open(os.path.join(GOLDEN, name + ".pickle"), "rb") as f:      # made before the rules shared one `__reduce__`
        old = pickle.load(f)
    assert type(old) is type(rule) and old == rule and hash(old) == hash(rule) and old._key() == rule._key()
    assert vars(old) == vars(rule) or name == "StartCandidates"          # (NaN is not equal to itself: the key holds its bits)
    assert repr(old) == repr(rule)
    again = pickle.loads(pickle.dumps(rule))
    assert type(again) is type(rule) and again == rule and again._key() == rule._key()
