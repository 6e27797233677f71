"""The rules of pga_align_pairs and pga_cluster_edges pinned by hand-worked cases on their Python reference
(tests/protein_alignments_ref.py), clause by clause; the ProteinAlignments and VerifiedClusters rule classes; and every refusal of the
Python layer that needs no device (a fake object that only carries a `__cuda_array_interface__` dict stands in for a tensor)."""
import fractions
import pickle
import random

import numpy as np
import pytest

from pyrodigal_amd._cabi import (AlignOpts, DeviceClusters, DeviceProteins, ProteinAlignments, ProteinClusters, ProteinSketches, ProteinTokens,
                                 VerifiedClusters, align_into, edges_into)

from tests import protein_alignments_ref as ref


def toks(s):
    return [ord(c) for c in s]


# ---- clause 2: the distance ----
def test_kitten_sitting_and_friends():
    assert ref.edit_distance(toks("kitten"), toks("sitting")) == 3         # k>s, e>i, +g
    assert ref.edit_distance(toks("sitting"), toks("kitten")) == 3
    assert ref.edit_distance(toks("flaw"), toks("lawn")) == 2
    assert ref.edit_distance(toks("abc"), toks("abc")) == 0
    assert ref.edit_distance(toks("abc"), toks("xyz")) == 3
    assert ref.edit_distance([1 << 40], [0]) == 1 and ref.edit_distance([-1], [255]) == 1      # elements are whole integers


def test_empty_rows():
    assert ref.edit_distance([], []) == 0
    assert ref.edit_distance([], toks("abcd")) == 4 == ref.edit_distance(toks("abcd"), [])
    assert ref.align_pairs([[], []], [(0, 1)], 0, 1, 1) == ([0], [1])      # 0 * 1 <= 0 * 0: two empty rows are identical


def test_the_row_at_a_time_form_is_the_same_function():
    rng = random.Random(3)
    for _ in range(200):
        a = [rng.randrange(3) for _ in range(rng.randrange(0, 25))]
        b = [rng.randrange(3) for _ in range(rng.randrange(0, 25))]
        assert ref.edit_distance_rows(a, b) == ref.edit_distance(a, b)
    assert ref.edit_distance_rows(toks("kitten"), toks("sitting")) == 3 and ref.edit_distance_rows([], []) == 0


# ---- clause 3: the cap ----
def test_the_cap_is_max_distance_plus_one():
    rows = [toks("kitten"), toks("sitting"), toks("abcdefgh")]
    for k, want in ((0, 1), (1, 2), (2, 3), (3, 3), (4, 3), (255, 3)):
        assert ref.align_pairs(rows, [(0, 1)], k, 1, 2)[0] == [want]
    assert ref.edit_distance(rows[0], rows[2]) == 7
    assert ref.align_pairs(rows, [(0, 2)], 6, 1, 2) == ([7], [0])          # "more than 6"
    assert ref.align_pairs(rows, [(0, 2)], 7, 1, 8) == ([7], [1])          # 7 * 8 <= 7 * 8
    assert ref.align_pairs(rows, [(0, 0), (2, 2)], 0, 1, 1) == ([0, 0], [1, 1])


# ---- clause 4: the threshold ----
def test_the_threshold_met_exactly_and_missed_by_one():
    a = list(range(20))
    two, three = [90, 91] + a[2:], [90, 91, 92] + a[3:]
    rows = [a, two, three]
    assert ref.edit_distance(a, two) == 2 and ref.edit_distance(a, three) == 3
    # identity 18 / 20 = 9 / 10 exactly: 2 * 10 <= 1 * 20; one more edit misses: 3 * 10 > 20
    assert ref.align_pairs(rows, [(0, 1), (0, 2)], 5, 9, 10) == ([2, 3], [1, 0])
    # the same fraction not in lowest terms
    assert ref.align_pairs(rows, [(0, 1), (0, 2)], 5, 18, 20) == ([2, 3], [1, 0])
    # the longer row counts: 19 elements against 20, one deletion: 1 * 20 <= 1 * 20
    assert ref.align_pairs([a, a[:-1]], [(0, 1), (1, 0)], 3, 19, 20) == ([1, 1], [1, 1])
    assert ref.align_pairs([a[:-1], a[:-2]], [(0, 1)], 3, 19, 20) == ([1], [0])      # 1 * 20 > 1 * 19
    # within the identity and beyond max_distance: the distance decides
    assert ref.align_pairs(rows, [(0, 2)], 2, 1, 2) == ([3], [0])
    assert ref.align_pairs(rows, [(0, 2)], 3, 1, 2) == ([3], [1])


# ---- clause 1: indices ----
def test_out_of_range_pairs():
    rows = [toks("ab"), toks("ac")]
    assert ref.align_pairs(rows, [(-1, 0), (0, 2), (2, 2), (0, 1), (1, 1)], 4, 1, 2) == ([-1, -1, -1, 1, 0], [0, 0, 0, 1, 1])
    assert ref.align_pairs([], [(0, 0)], 4, 1, 2) == ([-1], [0])


# ---- components ----
def test_components_with_ignored_and_self_edges():
    edges = [(0, 1), (3, 3), (5, 2), (7, 0), (-1, 2), (4, 9), (1, 7)]
    r = ref.cluster_edges(edges, None, 8, None)
    assert r["n_used"] == 5                                                  # (-1, 2) and (4, 9) are ignored; (3, 3) counts and joins nothing
    assert r["cluster"] == [0, 0, 1, 2, 3, 1, 4, 0] and r["sizes"] == [3, 2, 1, 1, 1] and r["representatives"] == [0, 2, 3, 4, 6]
    r = ref.cluster_edges(edges, [1, 1, 0, 1, 1, 1, 0], 8, [0, 0, 0, 0, 0, 5, 0, 9])
    assert r["n_used"] == 3 and r["cluster"] == [0, 0, 1, 2, 3, 4, 5, 0] and r["representatives"] == [7, 2, 3, 4, 5, 6]
    r = ref.cluster_edges([], None, 3, [4, 4, 4])
    assert r == {"cluster": [0, 1, 2], "representatives": [0, 1, 2], "sizes": [1, 1, 1], "n_clusters": 3, "n_used": 0}
    r = ref.cluster_edges([(2, 1), (1, 0)], None, 3, [1, 7, 7])              # a tie at the top: the smaller index
    assert r["cluster"] == [0, 0, 0] and r["representatives"] == [1] and r["sizes"] == [3]
    assert ref.cluster_edges([(0, 1)], None, 0, None)["n_clusters"] == 0


# ---- ProteinAlignments ----
def test_defaults_and_the_options_struct():
    spec = ProteinAlignments()
    assert spec.max_distance == 32 and spec.min_identity == (9, 10)
    o = spec.opts(4)
    assert isinstance(o, AlignOpts) and (o.elem_bytes, o.max_distance, o.num, o.den) == (4, 32, 9, 10)
    assert "max_distance=32" in repr(spec)


def test_fractions_and_pairs_name_the_same_rule():
    a, b = ProteinAlignments(10, fractions.Fraction(3, 4)), ProteinAlignments(10, (3, 4))
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1 and a.min_identity == (3, 4)
    assert a != ProteinAlignments(10, (6, 8)) and a != ProteinAlignments(11, (3, 4))      # (the pair is kept as given)
    assert a != ProteinClusters()


def test_pickling_round_trips():
    spec = ProteinAlignments(max_distance=7, min_identity=(19, 20))
    whole = VerifiedClusters(ProteinClusters(ProteinSketches(4, 16), 4, (3, 4), 2), spec, ProteinTokens("ACDEFGHIKLMNPQRSTVWYX", dtype="int32", layout="padded"))
    for proto in range(2, pickle.HIGHEST_PROTOCOL + 1):
        back = pickle.loads(pickle.dumps(spec, proto))
        assert back == spec and back.opts(1).den == 20 and repr(back) == repr(spec)
        back = pickle.loads(pickle.dumps(whole, proto))
        assert back == whole and hash(back) == hash(whole) and back.alignments == spec and back.tokens.layout == "padded"


def test_floats_are_refused_with_the_reason():
    with pytest.raises(TypeError, match="integers"):
        ProteinAlignments(min_identity=0.9)
    with pytest.raises(TypeError, match="int"):
        ProteinAlignments(min_identity=(0.9, 1))


@pytest.mark.parametrize("kwargs", [dict(max_distance=-1), dict(max_distance=256), dict(min_identity=(0, 10)), dict(min_identity=(11, 10)),
                                    dict(min_identity=(1, (1 << 20) + 1))])
def test_ranges(kwargs):
    with pytest.raises(ValueError):
        ProteinAlignments(**kwargs)


@pytest.mark.parametrize("kwargs", [dict(max_distance=True), dict(max_distance=2.0), dict(max_distance="3"), dict(min_identity=9),
                                    dict(min_identity=(9, 10, 11)), dict(min_identity=(True, 2))])
def test_types(kwargs):
    with pytest.raises(TypeError):
        ProteinAlignments(**kwargs)


def test_the_edges_of_the_ranges_are_allowed():
    ProteinAlignments(0, (1, 1))
    ProteinAlignments(255, (1 << 20, 1 << 20))
    ProteinAlignments(np.int64(5), (np.int32(1), 2))


# ---- VerifiedClusters ----
def test_verified_clusters_defaults_and_refusals():
    v = VerifiedClusters()
    assert v.clusters == ProteinClusters() and v.alignments == ProteinAlignments()
    assert v.tokens == ProteinTokens("ACDEFGHIKLMNPQRSTVWYX", dtype="uint8", layout="ragged") and v.per_contig == "tables"
    assert v == VerifiedClusters() and v != VerifiedClusters(alignments=ProteinAlignments(5))
    with pytest.raises(ValueError, match="protein"):
        VerifiedClusters(ProteinClusters(ProteinSketches(5, 32, "gene")))
    with pytest.raises(TypeError, match="clusters must be a ProteinClusters"):
        VerifiedClusters(ProteinSketches())
    with pytest.raises(TypeError, match="alignments must be a ProteinAlignments"):
        VerifiedClusters(alignments=(9, 10))
    with pytest.raises(TypeError, match="tokens must be a ProteinTokens"):
        VerifiedClusters(tokens="ACDEFGHIKLMNPQRSTVWYX")


def test_the_package_exports_the_rules():
    import pyrodigal_amd
    assert pyrodigal_amd.ProteinAlignments is ProteinAlignments and pyrodigal_amd.VerifiedClusters is VerifiedClusters
    assert "ProteinAlignments" in pyrodigal_amd.__all__ and "VerifiedClusters" in pyrodigal_amd.__all__


# ---- the layer, without a device ----
class Fake:
    def __init__(self, shape, typestr="<i8", ptr=4096, strides=None):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}


def test_align_refusals_that_need_no_device():
    spec = ProteinAlignments()
    tok, pairs, out = Fake((100,), "|u1"), Fake((4, 2)), (Fake((4,)), Fake((4,)))
    good = dict(tokens=tok, row_begin=[0, 50], row_len=[50, 50], pairs=pairs, spec=spec, out=out)

    def call(**change):
        a = dict(good, **change)
        return align_into(None, None, 0, a["tokens"], a["row_begin"], a["row_len"], a["pairs"], a["spec"], a["out"])

    for kw, err, word in ((dict(spec=ProteinClusters()), TypeError, "must be a ProteinAlignments"),
                          (dict(tokens=np.zeros(4, np.uint8)), TypeError, "__cuda_array_interface__"),
                          (dict(tokens=Fake((100,), "<f4")), TypeError, "uint8, int32 or int64"),
                          (dict(tokens=Fake((10, 10), "<i4", strides=(80, 8))), ValueError, "contiguous last dimension"),
                          (dict(tokens=Fake((10, 10), "<i4", strides=(42, 4))), ValueError, "contiguous last dimension"),
                          (dict(row_len=[50]), ValueError, "row_begin has 2 entries and row_len 1"),
                          (dict(row_begin=[0, 1.5]), TypeError, "row_begin must hold integers"),
                          (dict(pairs=Fake((4, 3))), ValueError, "pairs needs shape"),
                          (dict(pairs=Fake((8,))), ValueError, "pairs needs shape"),
                          (dict(pairs=Fake((4, 2), "<i4")), TypeError, "int64"),
                          (dict(pairs=Fake((4, 2), strides=(32, 8))), ValueError, "not contiguous"),
                          (dict(out=(Fake((4,)),)), ValueError, "out must be"),
                          (dict(out=(None, Fake((4,)))), TypeError, "distance is required"),
                          (dict(out=(Fake((3,)), None)), ValueError, "distance needs shape"),
                          (dict(out=(Fake((4,)), Fake((4,), "<i4"))), TypeError, "int64")):
        with pytest.raises(err, match=word):
            call(**kw)
    with pytest.raises(ValueError, match="names no context"):
        DeviceProteins(tok, np.array([50, 50]), np.array([0, 50, 100]), None, 0).align(pairs, spec)


def test_cluster_edges_refusals_that_need_no_device():
    edges, out = Fake((5, 2)), (Fake((8,)), Fake((8,)), Fake((8,)))

    def call(edges=edges, n=8, keep=None, weights=None, out=out):
        return edges_into(None, None, 0, edges, n, keep, weights, out)

    for kw, err, word in ((dict(n=True), TypeError, "n must be an int"), (dict(n=2.0), TypeError, "n must be an int"),
                          (dict(n=-1), ValueError, "negative"),
                          (dict(edges=Fake((5, 3))), ValueError, "edges needs shape"), (dict(edges=Fake((5, 2), "<i4")), TypeError, "int64"),
                          (dict(keep=Fake((4,))), ValueError, "keep needs shape"), (dict(keep=Fake((5,), "|u1")), TypeError, "int64"),
                          (dict(weights=Fake((7,))), ValueError, "weights needs shape"),
                          (dict(out=out[:2]), ValueError, "out must be"), (dict(out=(None,) + out[1:]), TypeError, "cluster is required"),
                          (dict(out=(Fake((7,)),) + out[1:]), ValueError, "cluster needs shape"),
                          (dict(out=(out[0], Fake((7,)), None)), ValueError, "representatives needs shape")):
        with pytest.raises(err, match=word):
            call(**kw)
    dc = DeviceClusters(Fake((8,)), None, None, 8, edges, None, None, 5, ProteinClusters(), None, 0)
    with pytest.raises(ValueError, match="names no context"):
        dc.relink()
    dc = DeviceClusters(Fake((8,)), None, None, 8, None, None, None, 5, ProteinClusters(), None, 0, L=object(), ctx_h=1)
    with pytest.raises(ValueError, match="has no edges"):
        dc.relink()


def test_the_finder_refuses_another_rule():
    from pyrodigal_amd import lib
    finder = lib.GeneFinder(meta=True)
    with pytest.raises(TypeError, match="must be a VerifiedClusters"):
        finder.find_verified_clusters_batch([b"ACGT" * 100], ProteinClusters())
