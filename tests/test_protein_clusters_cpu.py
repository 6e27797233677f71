"""The rule of pga_cluster_sketches pinned by hand-worked cases on its Python reference (tests/protein_clusters_ref.py), clause by
clause, and the ProteinClusters rule class.  No device."""
import fractions
import pickle

import pytest

from pyrodigal_amd._cabi import ClusterOpts, ProteinClusters, ProteinSketches

from tests import protein_clusters_ref as ref

INT64_MAX = (1 << 63) - 1


def run(rows, weights=None, size=4, probes=4, num=1, den=2, min_union=0):
    return ref.cluster(rows, weights, size, probes, num, den, min_union)


# ---- clause 1: probes ----
def test_padding_is_never_a_probe_and_empty_rows_stay_apart():
    r = run([[], [], [5], []])
    assert r["candidates"] == [] and r["cluster"] == [0, 1, 2, 3] and r["sizes"] == [1, 1, 1, 1] and r["n_edges"] == 0


def test_a_counted_int64_max_is_a_probe_like_any_other():
    r = run([[INT64_MAX], [3], [INT64_MAX], []], size=2, probes=2)
    assert r["candidates"] == [(0, 2)] and r["edges"] == [(0, 2)] and (r["edge_shared"], r["edge_union"]) == ([1], [1])
    assert r["cluster"] == [0, 1, 0, 2]


def test_only_the_first_probes_entries_propose():
    rows = [[1, 2, 9], [3, 4, 9]]                              # the one common hash sits at position 2
    assert ref.shared_of(rows[0], rows[1], 8) == (1, 5)
    assert run(rows, size=8, probes=3, num=1, den=5)["edges"] == [(0, 1)]
    assert run(rows, size=8, probes=2, num=1, den=5)["candidates"] == []
    # probes counts positions of the row, not hashes shared: the common hash lies at position 0 of one row and 2 of the other
    rows = [[9, 20, 30], [1, 2, 9]]
    assert run(rows, probes=1)["candidates"] == [] and run(rows, probes=3)["candidates"] == [(0, 1)]


# ---- clauses 2 and 3: buckets, centres, candidates ----
def test_the_centre_is_the_heaviest_member_and_the_outer_pair_is_never_proposed():
    rows = [[7, 10], [7, 11], [7, 12]]
    r = run(rows, weights=[1, 5, 1], size=2, probes=1, num=1, den=2)
    assert r["candidates"] == [(0, 1), (1, 2)]                 # (0, 2) would pass -- (1, 2) of 2 -- and is not proposed
    assert ref.shared_of(rows[0], rows[2], 2) == (1, 2)
    assert r["cluster"] == [0, 0, 0] and r["representatives"] == [1] and r["sizes"] == [3]


def test_equal_and_absent_weights_name_the_lowest_index():
    rows = [[7, 10], [7, 11], [7, 12]]
    for w in (None, [4, 4, 4]):
        r = run(rows, weights=w, size=2, probes=1)
        assert r["candidates"] == [(0, 1), (0, 2)] and r["representatives"] == [0]
    r = run(rows, weights=[1, 6, 6], size=2, probes=1)         # a tie at the top: the smaller index of the two
    assert r["candidates"] == [(0, 1), (1, 2)] and r["representatives"] == [1]


def test_pairs_are_unordered_and_distinct():
    rows = [[1, 2, 3], [1, 2, 3]]
    r = run(rows, weights=[0, 9], probes=3)                    # proposed as (c, g) = (1, 0) by each of three buckets
    assert r["proposals"] == 3 and r["candidates"] == [(0, 1)] and r["edges"] == [(0, 1)]
    assert (r["edge_shared"], r["edge_union"]) == ([3], [3])


def test_at_most_records_times_probes_candidates():
    rows = [[h for h in range(1, 5)] for _ in range(6)]
    r = run(rows, probes=4)
    assert r["proposals"] == 5 * 4 and len(r["candidates"]) == 5 <= 6 * 4


# ---- clause 4: acceptance ----
def test_the_threshold_is_met_exactly_or_missed_by_one():
    a, b = [1, 2, 3, 4], [1, 2, 5, 6]                          # union 1 2 3 4 5 6, m = 4: 1 2 shared of 1 2 3 4
    assert ref.shared_of(a, b, 4) == (2, 4)
    assert run([a, b], num=1, den=2)["edges"] == [(0, 1)]      # 2 * 2 >= 1 * 4
    assert run([a, b], num=2, den=3)["edges"] == []            # 2 * 3 <  2 * 4
    assert run([a, b], num=2, den=3)["candidates"] == [(0, 1)]


def test_min_union_and_the_floor_of_one():
    a, b = [1, 2], [1, 3]                                      # m = 3 under size 4
    assert ref.shared_of(a, b, 4) == (1, 3)
    for mu, want in ((2, [(0, 1)]), (3, [(0, 1)]), (4, [])):
        assert run([a, b], num=1, den=3, min_union=mu)["edges"] == want
    # min_union = 0 still asks for m >= 1: no pair of rows has m = 0 and a common probe, so the floor only ever refuses 0 / 0
    assert ref.shared_of([], [], 4) == (0, 0)


# ---- clauses 5 and 6: edges and clusters ----
def test_edges_come_in_ascending_order_with_their_counts():
    rows = [[1, 50], [2, 60], [2, 61], [1, 51], [1, 52]]
    r = run(rows, size=2, probes=1, num=1, den=2)
    assert r["edges"] == [(0, 3), (0, 4), (1, 2)] and r["edge_shared"] == [1, 1, 1] and r["edge_union"] == [2, 2, 2]
    assert r["n_edges"] == 3


def test_clusters_are_numbered_by_their_smallest_member():
    rows = [[9, 90], [1, 10], [5, 50], [1, 11], [9, 91], [1, 12]]
    r = run(rows, weights=[1, 1, 1, 1, 7, 3], size=2, probes=1, num=1, den=2)
    assert r["cluster"] == [0, 1, 2, 1, 0, 1]
    assert r["representatives"] == [4, 5, 2] and r["sizes"] == [2, 3, 1] and r["n_clusters"] == 3


def test_single_linkage_chains():
    rows = [[i, i + 1] for i in range(6)]
    r = run(rows, size=2, probes=2, num=1, den=2)
    assert r["edges"] == [(i, i + 1) for i in range(5)] and set(zip(r["edge_shared"], r["edge_union"])) == {(1, 2)}
    assert r["cluster"] == [0] * 6 and ref.shared_of(rows[0], rows[5], 2) == (0, 2)


# ---- the rule class ----
def test_defaults_and_the_options_struct():
    spec = ProteinClusters()
    assert spec.sketches == ProteinSketches(5, 32) and spec.probes == 8 and spec.min_resemblance == (9, 10) and spec.min_union == 8
    o = spec.opts()
    assert isinstance(o, ClusterOpts) and (o.size, o.probes, o.num, o.den, o.min_union) == (32, 8, 9, 10, 8)
    assert spec.per_contig == "tables"


def test_fractions_and_pairs_name_the_same_rule():
    a = ProteinClusters(ProteinSketches(4, 16), 4, fractions.Fraction(3, 4), 2)
    b = ProteinClusters(ProteinSketches(4, 16), 4, (3, 4), 2)
    assert a == b and hash(a) == hash(b) and a.min_resemblance == (3, 4)
    assert a != ProteinClusters(ProteinSketches(4, 16), 4, (6, 8), 2)      # (the pair is kept as given: it is what the device gets)
    assert a != ProteinClusters(ProteinSketches(4, 16, seed=1), 4, (3, 4), 2)
    assert len({a, b}) == 1


def test_pickling_round_trips():
    spec = ProteinClusters(ProteinSketches(3, 8, "gene", seed=5), probes=3, min_resemblance=(7, 8), min_union=0)
    for proto in range(2, pickle.HIGHEST_PROTOCOL + 1):
        back = pickle.loads(pickle.dumps(spec, proto))
        assert back == spec and back.opts().den == 8 and back.sketches.of == "gene" and repr(back) == repr(spec)


def test_floats_are_refused_with_the_reason():
    with pytest.raises(TypeError, match="integers"):
        ProteinClusters(min_resemblance=0.9)
    with pytest.raises(TypeError, match="int"):
        ProteinClusters(min_resemblance=(0.9, 1))


@pytest.mark.parametrize("kwargs", [dict(probes=0), dict(probes=33), dict(min_resemblance=(0, 10)), dict(min_resemblance=(11, 10)),
                                    dict(min_resemblance=(1, (1 << 20) + 1)), dict(min_union=-1), dict(min_union=33)])
def test_ranges(kwargs):
    with pytest.raises(ValueError):
        ProteinClusters(ProteinSketches(5, 32), **kwargs)


@pytest.mark.parametrize("kwargs", [dict(probes=True), dict(probes=2.0), dict(min_union="8"), dict(sketches="protein"),
                                    dict(min_resemblance=9), dict(min_resemblance=(9, 10, 11))])
def test_types(kwargs):
    with pytest.raises(TypeError):
        ProteinClusters(**kwargs)


def test_the_edges_of_the_ranges_are_allowed():
    ProteinClusters(ProteinSketches(5, 64), probes=64, min_resemblance=(1 << 20, 1 << 20), min_union=64)
    ProteinClusters(ProteinSketches(5, 1), probes=1, min_resemblance=(1, 1), min_union=0)
