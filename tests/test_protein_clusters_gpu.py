"""Near-identical proteins clustered on the device from their sketches (pga_cluster_sketches, ProteinClusters, DeviceSketches.cluster,
Context.cluster_sketches, GeneFinder.find_clusters_batch).

Every expected value comes from the plain-Python restatement of the rule (tests/protein_clusters_ref.py) -- never from the code under
test -- and the device must give the same integers: cluster, representatives, sizes, edges, edge_shared, edge_union and both counts.
Most cases put sketch rows straight into device memory (tests/hip_mem.py, no torch), so the kernels see shapes no genome would give.
Every output lies inside an allocation full of a canary byte, and the whole allocation is compared."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hip_mem
from tests import protein_clusters_ref as ref

pytestmark = pytest.mark.gpu

CANARY = 0xA5
INT64_MAX = (1 << 63) - 1


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi, benchdata
    c = _cabi.Context(0)
    c.set_models([b for _, b in benchdata.load_model_set()])
    yield c
    c.close()


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

    def __init__(self, ptr, shape, typestr="<i8"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3, "strides": None}


class Target:
    """Six allocations full of a fill byte, and in each an int64 tensor that begins 8 bytes into it with `slack` elements behind:
    cluster [G], representatives [cap], sizes [cap], edges [ecap, 2], edge_shared [ecap], edge_union [ecap].  `given`: which of them
    are passed at all."""

    def __init__(self, G, cap, ecap, given=(True,) * 6, slack=5, fill=CANARY):
        self.shapes = [(G,), (cap,), (cap,), (ecap, 2), (ecap,), (ecap,)]
        self.given, self.ecap = tuple(given), ecap
        self.before = [np.full(8 * (1 + int(np.prod(s)) + slack), fill, np.uint8) for s in self.shapes]
        self.mem = [keep(hip_mem.DeviceArray.from_numpy(b)) for b in self.before]
        self.ptr = [m.ptr + 8 if on else None for m, on in zip(self.mem, self.given)]
        self.out = tuple(View(m.ptr + 8, s) if on else None for m, s, on in zip(self.mem, self.shapes, self.given))

    def read(self):
        return [m.to_numpy(np.int64) for m in self.mem]

    def expect(self, r):
        """what the whole allocations must hold after a call whose result is the reference's `r`"""
        w = min(self.ecap, r["n_edges"])
        want = (r["cluster"], r["representatives"], r["sizes"], r["edges"][:w], r["edge_shared"][:w], r["edge_union"][:w])
        out = [b.view(np.int64).copy() for b in self.before]
        for e, x, on in zip(out, want, self.given):
            if on:
                x = np.asarray(x, np.int64).reshape(-1)
                e[1:1 + len(x)] = x
        return out

    def untouched(self):
        return all(np.array_equal(m.to_numpy(np.uint8), b) for m, b in zip(self.mem, self.before))


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def device_rows(rows, s, weights=None, pad=INT64_MAX):
    """(sketch [G, s], count [G], weight [G] or None) of lists of real entries, on the device, as pga_sketch_proteins leaves them;
    `pad` is what lies behind the counts"""
    G = len(rows)
    sk, cnt = np.full((max(G, 1), s), pad, np.int64), np.zeros(max(G, 1), np.int64)
    for g, row in enumerate(rows):
        assert list(row) == sorted(set(row)) and len(row) <= s
        sk[g, :len(row)] = row
        cnt[g] = len(row)
    d_w = None if weights is None else keep(hip_mem.DeviceArray.from_numpy(np.asarray(weights, np.int64).reshape(G)))
    return keep(hip_mem.DeviceArray.from_numpy(sk)), keep(hip_mem.DeviceArray.from_numpy(cnt)), d_w


def raw(ctx, sketch, count, weight, n, opts, ptr, capacity, ecap):
    """the C call itself: (rc, message, n_clusters, n_edges)"""
    from pyrodigal_amd import _cabi
    o = _cabi.ClusterOpts()
    o.size, o.probes, o.num, o.den, o.min_union = opts
    nc, ne = ctypes.c_int64(-7), ctypes.c_int64(-7)
    vp = ctypes.c_void_p
    rc = ctx.L.pga_cluster_sketches(ctx.h, vp(sketch), vp(count), vp(weight), n, ctypes.byref(o), vp(ptr[0]), vp(ptr[1]), vp(ptr[2]), capacity,
                                    vp(ptr[3]), vp(ptr[4]), vp(ptr[5]), ecap, None, ctypes.byref(nc), ctypes.byref(ne))
    return rc, ctx.L.pga_last_error(ctx.h).decode(), nc.value, ne.value


def check(ctx, rows, s, probes, num, den, min_union, weights=None, given=(True,) * 6, ecap=None, pad=INT64_MAX, want=None):
    """One call on injected rows against the reference: every allocation whole, and both counts.  Returns the reference's result."""
    G = len(rows)
    r = ref.cluster(rows, weights, s, probes, num, den, min_union) if want is None else want
    assert len(r["candidates"]) <= G * probes
    d_sk, d_cnt, d_w = device_rows(rows, s, weights, pad)
    t = Target(G, G, G * probes if ecap is None else ecap, given)
    rc, msg, nc, ne = raw(ctx, d_sk.ptr, d_cnt.ptr, d_w.ptr if d_w else None, G, (s, probes, num, den, min_union), t.ptr, G, t.ecap if given[3] else 0)
    assert rc == 0, msg
    assert (nc, ne) == (r["n_clusters"], r["n_edges"])
    got, exp = t.read(), t.expect(r)
    for name, g, e in zip(("cluster", "representatives", "sizes", "edges", "edge_shared", "edge_union"), got, exp):
        assert np.array_equal(g, e), name
    stats = ctx.cluster_stats()
    assert stats == {"probes": sum(min(probes, len(x)) for x in rows), "candidates": len(r["candidates"]), "edges": ne, "clusters": nc}
    return r


# ---- 1. empty and single ---------------------------------------------------------------------------------------------------------------------
def test_no_record_one_record_and_empty_rows(ctx):
    t = Target(0, 0, 0)
    rc, msg, nc, ne = raw(ctx, None, None, None, 0, (32, 8, 9, 10, 8), [None] * 6, 0, 0)
    assert (rc, nc, ne) == (0, 0, 0), msg
    rc, msg, nc, ne = raw(ctx, None, None, None, 0, (32, 8, 9, 10, 8), t.ptr, 0, 0)
    assert (rc, nc, ne) == (0, 0, 0) and t.untouched(), msg
    r = check(ctx, [[4, 5, 6]], 4, 2, 1, 2, 0)
    assert r["cluster"] == [0] and r["representatives"] == [0] and r["sizes"] == [1] and r["edges"] == []
    r = check(ctx, [[]], 4, 4, 1, 2, 0)
    assert r["n_clusters"] == 1
    # every row empty: the padding is the same in all of them, and is no probe -- whatever it holds
    for pad in (INT64_MAX, 7, 0):
        r = check(ctx, [[]] * 70, 4, 4, 1, 4, 0, pad=pad)
        assert r["n_clusters"] == 70 and r["n_edges"] == 0 and r["candidates"] == []
    r = check(ctx, [[], []], 1, 1, 1, 1, 0)                       # two rows with count = 0 stay apart
    assert r["cluster"] == [0, 1]


def test_a_counted_int64_max_joins_two_rows_and_padding_joins_nobody(ctx):
    rows = [[INT64_MAX], [3], [INT64_MAX], [], [2, INT64_MAX], [1 << 62]]
    r = check(ctx, rows, 2, 2, 1, 2, 0)                            # rows 1, 3 and 5 are padded with INT64_MAX, inside the probes
    assert r["edges"] == [(0, 2), (0, 4)] and r["cluster"] == [0, 1, 0, 2, 0, 3]
    assert r["edge_shared"] == [1, 1] and r["edge_union"] == [1, 2]
    r = check(ctx, rows, 2, 2, 1, 2, 0, weights=[0, 0, 0, 0, 5, 0])
    assert r["edges"] == [(0, 4), (2, 4)] and r["representatives"][0] == 4
    # padding that equals a genuine hash of other rows
    r = check(ctx, [[3], [3, 9], [], [9]], 2, 2, 1, 2, 0, pad=3)
    assert r["edges"] == [(0, 1), (1, 3)] and r["cluster"] == [0, 0, 1, 0]


# ---- 2. the threshold ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1, 5, 32, 64])
def test_the_threshold_exactly_met_and_missed_by_one(ctx, s):
    if s == 1:
        # one hash per row: a proposed pair has (shared, m) = (1, 1), and num <= den lets no threshold miss it
        r = check(ctx, [[5], [6], [5]], 1, 1, 1, 1, 0)
        assert r["edges"] == [(0, 2)] and (r["edge_shared"], r["edge_union"]) == ([1], [1])
        r = check(ctx, [[5], [6], [5]], 1, 1, 1, 1, 1)
        assert r["edges"] == [(0, 2)]
        return
    t = s - 1                                                     # (shared, m) = (s - 1, s): in lowest terms
    rows = [list(range(s)), list(range(t)) + [1000], [5000], list(range(2000, 2000 + s)), list(range(2000, 2000 + t)) + [9000]]
    assert ref.shared_of(rows[0], rows[1], s) == (t, s) == ref.shared_of(rows[3], rows[4], s)
    for num, den, edges in ((t, s, [(0, 1), (3, 4)]), (2 * t, 2 * s, [(0, 1), (3, 4)]),     # shared * den == num * m
                            (1, 1, []), (2 * s - 1, 2 * s + 1, [])):                        # shared * den == num * m - 1
        assert t * den - num * s == (0 if edges else -1)
        r = check(ctx, rows, s, min(s, 3), num, den, 0)
        assert r["edges"] == edges and r["candidates"] == [(0, 1), (3, 4)]
    # a union smaller than the sketch: m = 3, and min_union at m - 1, m and m + 1
    rows = [[1, 2], [1, 3], [8]]
    assert ref.shared_of(rows[0], rows[1], s) == (1, 3)
    for mu, edges in ((2, [(0, 1)]), (3, [(0, 1)]), (4, [])):
        r = check(ctx, rows, s, 2, 1, 3, mu)
        assert r["edges"] == edges and r["candidates"] == [(0, 1)]


# ---- 3. probes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("j", [1, 3, 7])
def test_a_common_hash_at_position_j_needs_j_plus_one_probes(ctx, j):
    s = 16
    rows = [list(range(100, 100 + j)) + [900], list(range(200, 200 + j)) + [900], [901]]
    assert ref.shared_of(rows[0], rows[1], s) == (1, 2 * j + 1)
    found = check(ctx, rows, s, j + 1, 1, 64, 0)
    assert found["edges"] == [(0, 1)] and found["cluster"] == [0, 0, 1]
    missed = check(ctx, rows, s, j, 1, 64, 0)
    assert missed["candidates"] == [] and missed["cluster"] == [0, 1, 2]
    # at position j in one row only: the other row's probes would reach it, the pair needs both
    rows[1] = [900] + list(range(1000, 1000 + j))
    assert check(ctx, rows, s, j, 1, 64, 0)["candidates"] == []


# ---- 4. centres ------------------------------------------------------------------------------------------------------------------------------
def test_the_centre_of_a_bucket(ctx):
    rows = [[7, 10], [7, 11], [7, 12]]
    r = check(ctx, rows, 2, 1, 1, 2, 0, weights=[1, 5, 1])
    assert r["candidates"] == [(0, 1), (1, 2)] and ref.shared_of(rows[0], rows[2], 2) == (1, 2)      # the outer pair would pass
    assert r["representatives"] == [1] and r["sizes"] == [3]
    for w in ([4, 4, 4], None, [-3, -3, -3]):
        r = check(ctx, rows, 2, 1, 1, 2, 0, weights=w)
        assert r["candidates"] == [(0, 1), (0, 2)] and r["representatives"] == [0]
    r = check(ctx, rows, 2, 1, 1, 2, 0, weights=[1, 6, 6])        # a tie at the top
    assert r["candidates"] == [(0, 1), (1, 2)] and r["representatives"] == [1]
    # weights over the whole of int64, and a heaviest member that is not the smallest index of its cluster
    big = [-(1 << 63), INT64_MAX, INT64_MAX - 1]
    r = check(ctx, rows, 2, 1, 1, 2, 0, weights=big)
    assert r["candidates"] == [(0, 1), (1, 2)] and r["representatives"] == [1]
    r = check(ctx, rows + [[7, 13]], 2, 1, 1, 2, 0, weights=[-5, -(1 << 63), -1, -1])
    assert r["candidates"] == [(0, 2), (1, 2), (2, 3)] and r["representatives"] == [2]


# ---- 5. duplicates ---------------------------------------------------------------------------------------------------------------------------
def test_a_pair_proposed_many_times_and_the_wrong_way_round(ctx):
    probes = 8
    rows = [list(range(10, 18)), list(range(50, 58)), list(range(10, 18))]
    r = check(ctx, rows, 8, probes, 1, 1, 8, weights=[0, 0, 9])     # centre 2 in every one of 8 buckets: (c, g) = (2, 0)
    assert r["proposals"] == probes and r["candidates"] == [(0, 2)] == r["edges"]
    assert (r["edge_shared"], r["edge_union"]) == ([8], [8]) and r["cluster"] == [0, 1, 0] and r["representatives"] == [2, 1]


# ---- 6. a long chain -------------------------------------------------------------------------------------------------------------------------
def test_a_chain_of_three_thousand_and_two_interleaved(ctx):
    N = 3000
    rows = [[i, i + 1] for i in range(N)]
    r = ref.cluster(rows, None, 2, 2, 1, 2, 0)
    assert r["edges"] == [(i, i + 1) for i in range(N - 1)] and set(zip(r["edge_shared"], r["edge_union"])) == {(1, 2)}
    assert r["cluster"] == [0] * N and r["sizes"] == [N]          # one cluster of diameter N - 1
    check(ctx, rows, 2, 2, 1, 2, 0, want=r)
    rows = [[i, i + 2] for i in range(N)]                         # two chains, by the parity of the index
    r = ref.cluster(rows, None, 2, 2, 1, 2, 0)
    assert r["n_edges"] == N - 2 and r["cluster"] == [i % 2 for i in range(N)] and r["sizes"] == [N // 2, N // 2]
    check(ctx, rows, 2, 2, 1, 2, 0, want=r)
    check(ctx, rows, 2, 2, 1, 2, 0, weights=[(i * 7919) % 13 for i in range(N)])


# ---- 7. one huge bucket ----------------------------------------------------------------------------------------------------------------------
def test_five_thousand_rows_in_one_bucket(ctx):
    N = 5000
    rows = [[1, 1000 + i] for i in range(N)]
    r = check(ctx, rows, 2, 1, 1, 2, 0, weights=[1] * (N - 1) + [9])
    assert r["candidates"] == [(i, N - 1) for i in range(N - 1)] == r["edges"]
    assert r["sizes"] == [N] and r["representatives"] == [N - 1]
    r = check(ctx, rows, 2, 1, 2, 3, 0, weights=[1] * (N - 1) + [9])      # all 4 999 refused: 1 of 2 is less than 2 of 3
    assert len(r["candidates"]) == N - 1 and r["n_edges"] == 0 and r["n_clusters"] == N


# ---- 8. boundaries ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,probes", [(63, 1), (64, 1), (65, 1), (255, 1), (256, 1), (257, 1), (32, 2), (128, 2), (85, 3), (86, 3)])
def test_buckets_across_the_boundaries_of_waves_and_blocks(ctx, G, probes):
    """The sorted probes lie in buckets of 2, 3, 3, 3, ...: one covers positions 62 .. 64 and one 254 .. 256.  The records are in a
    shuffled order, so the sort has work to do; with more than one probe a record has unique hashes behind its bucket's."""
    rng = np.random.default_rng(G * 10 + probes)
    order = rng.permutation(G)
    rows = [None] * G
    for at in range(G):
        g = int(order[at])
        rows[g] = sorted({(at + 1) // 3} | {200000 + 10 * g + x for x in range(probes)})
    w = rng.integers(0, 4, size=G).tolist()
    r = check(ctx, rows, probes + 1, probes, 1, probes + 1, 0, weights=w)
    assert r["n_edges"] > 0 and max(r["sizes"]) in (2, 3)
    check(ctx, rows, probes + 1, probes, 1, probes + 1, 0)


# ---- 9. random rows --------------------------------------------------------------------------------------------------------------------------
def random_rows():
    s, G = 32, 300
    rng = np.random.default_rng(500)
    rows = [sorted(set(rng.integers(0, 150, size=int(rng.integers(0, 60))).tolist()))[:s] for _ in range(G)]
    return rows, rng.integers(0, 6, size=G).tolist(), s


@pytest.mark.parametrize("probes,num,den,min_union", [(2, 1, 4, 0), (8, 1, 6, 0), (8, 2, 7, 24), (32, 2, 7, 0)])
def test_random_rows(ctx, probes, num, den, min_union):
    rows, w, s = random_rows()
    r = ref.cluster(rows, w, s, probes, num, den, min_union)
    assert sum(1 for x in r["sizes"] if x > 1) >= 5              # the seed was chosen so that the reference alone shows all three
    assert len(r["candidates"]) > r["n_edges"]                    # a candidate that is refused
    assert r["proposals"] > len(r["candidates"])                  # a pair proposed more than once
    check(ctx, rows, s, probes, num, den, min_union, weights=w, want=r)


# ---- 10. capacity ----------------------------------------------------------------------------------------------------------------------------
def test_edge_capacity_and_outputs_left_out(ctx):
    rows, w, s = random_rows()
    r = ref.cluster(rows, w, s, 8, 1, 6, 0)
    E = r["n_edges"]
    assert E > 10
    for ecap in (0, 1, E - 1, E, E + 3):
        check(ctx, rows, s, 8, 1, 6, 0, weights=w, ecap=ecap, want=r)      # the prefix, the true count, the canary behind it
    check(ctx, rows, s, 8, 1, 6, 0, weights=w, given=(True, True, True, False, False, False), want=r)
    check(ctx, rows, s, 8, 1, 6, 0, weights=w, given=(True, False, False, True, True, True), want=r)
    check(ctx, rows, s, 8, 1, 6, 0, weights=w, given=(True, True, False, True, True, True), want=r)
    check(ctx, rows, s, 8, 1, 6, 0, weights=w, given=(True, False, True, False, False, False), want=r)
    check(ctx, rows, s, 8, 1, 6, 0, weights=w, given=(True, False, False, False, False, False), want=r)


# ---- 11. memory of earlier calls -------------------------------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_earlier_calls(ctx):
    rows, w, s = random_rows()
    small = rows[:40]
    r = ref.cluster(small, w[:40], s, 4, 1, 5, 0)
    check(ctx, small, s, 4, 1, 5, 0, weights=w[:40], want=r)
    check(ctx, rows, s, 32, 1, 8, 0, weights=w)                   # larger: the work arrays grow, and are left full of its numbers
    check(ctx, small, s, 4, 1, 5, 0, weights=w[:40], want=r)
    check(ctx, [[1, 1000 + i] for i in range(2000)], 2, 1, 1, 2, 0)       # another shape: one bucket, no weights
    check(ctx, small, s, 4, 1, 5, 0, weights=w[:40], want=r)
    check(ctx, small, s, 4, 1, 5, 0, want=ref.cluster(small, None, s, 4, 1, 5, 0))


# ---- 12. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_host_and_leave_the_context_usable(ctx):
    from pyrodigal_amd import ProteinClusters, ProteinSketches, _cabi
    rows, w, s = random_rows()
    G = len(rows)
    d_sk, d_cnt, d_w = device_rows(rows, s, w)
    t = Target(G, G, 50)
    host = np.zeros(G * s + 8, np.int64)
    good = dict(sketch=d_sk.ptr, count=d_cnt.ptr, weight=d_w.ptr, n=G, opts=(s, 8, 1, 6, 0), capacity=G, ecap=50)

    def call(**change):
        a = dict(good)
        ptr = list(t.ptr)
        for name, v in change.items():
            if name.startswith("p"):
                ptr[int(name[1:])] = v
            else:
                a[name] = v
        return raw(ctx, a["sketch"], a["count"], a["weight"], a["n"], a["opts"], ptr, a["capacity"], a["ecap"])

    for what, kw, word in (("size = 0", dict(opts=(0, 8, 1, 6, 0)), "size = 0"), ("size = 65", dict(opts=(65, 8, 1, 6, 0)), "size = 65"),
                           ("probes = 0", dict(opts=(s, 0, 1, 6, 0)), "probes = 0"), ("probes above size", dict(opts=(s, s + 1, 1, 6, 0)), "probes = 33"),
                           ("num = 0", dict(opts=(s, 8, 0, 6, 0)), "num / den"), ("num above den", dict(opts=(s, 8, 7, 6, 0)), "num / den"),
                           ("den above 2^20", dict(opts=(s, 8, 1, (1 << 20) + 1, 0)), "num / den"),
                           ("a negative min_union", dict(opts=(s, 8, 1, 6, -1)), "min_union = -1"), ("min_union above size", dict(opts=(s, 8, 1, 6, s + 1)), "min_union = 33"),
                           ("more than 2^31 - 1 records", dict(n=1 << 31), "2^31 - 1 records"), ("negative records", dict(n=-1), "bad arguments"),
                           ("more than 2^31 - 1 probes", dict(n=1 << 29), "2^31 - 1 probes"),
                           ("no sketches", dict(sketch=None), "d_sketch is NULL"), ("no counts", dict(count=None), "d_count is NULL"),
                           ("no d_cluster", dict(p0=None), "d_cluster is NULL"),
                           ("edges without their counts", dict(p4=None), "all three or not at all"), ("counts without edges", dict(p3=None, p5=None), "all three or not at all"),
                           ("a capacity below G", dict(capacity=G - 1), "capacity = 299"), ("a negative edge capacity", dict(ecap=-1), "edge_capacity = -1"),
                           ("misaligned sketches", dict(sketch=d_sk.ptr + 4), "d_sketch is not aligned"), ("misaligned weights", dict(weight=d_w.ptr + 2), "d_weight is not aligned"),
                           ("a misaligned d_cluster", dict(p0=t.ptr[0] + 4), "d_cluster is not aligned"), ("misaligned edges", dict(p3=t.ptr[3] + 1), "d_edges is not aligned"),
                           ("host sketches", dict(sketch=host.ctypes.data), "d_sketch is not device memory"),
                           ("host counts", dict(count=host.ctypes.data), "d_count is not device memory"),
                           ("host weights", dict(weight=host.ctypes.data), "d_weight is not device memory"),
                           ("a host d_cluster", dict(p0=host.ctypes.data), "d_cluster is not device memory"),
                           ("host representatives", dict(p1=host.ctypes.data), "d_representative is not device memory"),
                           ("host sizes", dict(p2=host.ctypes.data), "d_size is not device memory"),
                           ("host edges", dict(p3=host.ctypes.data), "d_edges is not device memory"),
                           ("a host d_edge_shared", dict(p4=host.ctypes.data), "d_edge_shared is not device memory"),
                           ("a host d_edge_union", dict(p5=host.ctypes.data), "d_edge_union is not device memory")):
        rc, msg, nc, ne = call(**kw)
        assert rc == _cabi.PGA_EINVAL and word in msg and msg.startswith("pga_cluster_sketches: "), (what, rc, msg)
        assert (nc, ne) == (-7, -7), what
    # the Python layer
    spec = ProteinClusters(ProteinSketches(5, s), 8, (1, 6), 0)
    sk, cnt, wt = View(d_sk.ptr, (G, s)), View(d_cnt.ptr, (G,)), View(d_w.ptr, (G,))
    with pytest.raises(ValueError, match="sketches needs shape"):
        ctx.cluster_sketches(View(d_sk.ptr, (G, s - 1)), cnt, spec, wt, out=t.out)
    with pytest.raises(ValueError, match="counts needs shape"):
        ctx.cluster_sketches(sk, View(d_cnt.ptr, (G - 1,)), spec, wt, out=t.out)
    with pytest.raises(ValueError, match="weights needs shape"):
        ctx.cluster_sketches(sk, cnt, spec, View(d_w.ptr, (G, 1)), out=t.out)
    with pytest.raises(TypeError, match="int64"):
        ctx.cluster_sketches(sk, cnt, spec, View(d_w.ptr, (G,), "<i4"), out=t.out)
    with pytest.raises(TypeError, match="cluster is required"):
        ctx.cluster_sketches(sk, cnt, spec, wt, out=(None,) + t.out[1:])
    with pytest.raises(ValueError, match="all three or not at all"):
        ctx.cluster_sketches(sk, cnt, spec, wt, out=t.out[:4] + (None, t.out[5]))
    with pytest.raises(ValueError, match="out must be"):
        ctx.cluster_sketches(sk, cnt, spec, wt, out=t.out[:5])
    with pytest.raises(ValueError, match="edges needs shape"):
        ctx.cluster_sketches(sk, cnt, spec, wt, out=t.out[:3] + (View(t.ptr[3], (100,)),) + t.out[4:])
    with pytest.raises(ValueError, match="not device memory"):
        ctx.cluster_sketches(sk, cnt, spec, wt, out=(View(host.ctypes.data, (G,)),) + t.out[1:])
    with pytest.raises(TypeError, match="ProteinClusters"):
        ctx.cluster_sketches(sk, cnt, ProteinSketches(5, s), wt, out=t.out)
    assert np.all(host == 0) and t.untouched()                    # nothing was written anywhere
    # the context runs a good call afterwards, through the Python layer: the tensors of out=, cut to what was written
    r = ref.cluster(rows, w, s, 8, 1, 6, 0)
    dc = ctx.cluster_sketches(sk, cnt, spec, wt, out=t.out)
    assert same(t.read(), t.expect(r)) and (dc.n_clusters, dc.n_edges) == (r["n_clusters"], r["n_edges"]) and r["n_edges"] > 50
    assert dc.cluster is t.out[0] and dc.spec == spec and dc.sketches is None
    dc = ctx.cluster_sketches(sk, cnt, spec, None, out=(t.out[0], None, None, None, None, None))
    assert dc.representatives is None and dc.edges is None and dc.n_clusters == ref.cluster(rows, None, s, 8, 1, 6, 0)["n_clusters"]


# ---- 13. through the finder ------------------------------------------------------------------------------------------------------------------
FINDER_SCRIPT = r'''
import sys
import torch                                   # first: the library then binds to the HIP runtime of torch's wheel
if not torch.cuda.is_available():
    print("torch sees no GPU")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
import numpy as np
from pyrodigal_amd import DeviceClusters, ProteinClusters, ProteinSketches, _cabi, benchdata, lib
from tests import protein_clusters_ref as ref
from tests import protein_sketches_ref as sk_ref
from tests.util import read_fasta

bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])
genome = read_fasta("GCF_001457455.1_NCTC11397_genomic_100kb.fna.gz")[0][1].encode("ascii")
finder = lib.GeneFinder(meta=True, metagenomic_bins=bins)
home = genome[:40000]
# the gene to plant: a long one on the forward strand, whole, well inside the first contig
first = finder.find_genes_batch([home])[0]
gene = max((g for g in first if g.strand == 1 and not g.partial_begin and not g.partial_end and g.begin > 700 and g.end < len(home) - 700),
           key=lambda g: g.end - g.begin)
b, e = gene.begin - 1, gene.end                                # 0-based [b, e)
assert (e - b) % 3 == 0 and e - b >= 1200
lo, hi = b - 600, e + 600
STOPS = (b"TAA", b"TAG", b"TGA")


def substituted(seq, at_codons):
    out = bytearray(seq)
    for c in at_codons:
        p = b + 3 * c - lo
        for base in b"ACGT":
            new = bytes([base]) + bytes(out[p + 1:p + 3])
            if base != out[p] and new not in STOPS:
                out[p] = base
                break
    return bytes(out)


piece = genome[lo:hi]
two_substitutions = substituted(piece, (100, 250))
start = bytearray(piece)
assert bytes(start[b - lo:b - lo + 3]) in (b"ATG", b"GTG", b"TTG")
start[b - lo] = ord("G") if start[b - lo] != ord("G") else ord("A")       # another start codon
truncated = piece[:len(piece) - 600 - ((e - b) // 30) * 3]                # the contig ends inside the gene: its last tenth is gone
stranger = genome[60000:60000 + len(piece)]
seqs = [home, two_substitutions, bytes(start), truncated, stranger]
spec = ProteinClusters(ProteinSketches(5, 32), probes=8, min_resemblance=(1, 2), min_union=8)


def planted(genes, i):
    """the gene of contig i (1 .. 3) that lies over the planted one"""
    over = [g for g in genes[i] if g.strand == 1 and min(g.end, e - lo) - max(g.begin - 1, b - lo) > (e - b) // 2]
    assert len(over) == 1, (i, [(g.begin, g.end) for g in over])
    return over[0]


side = torch.cuda.Stream()
with torch.cuda.stream(side):
    genes, dc = finder.find_clusters_batch(seqs, spec)
    biggest = dc.sizes.max()                                   # a consumer on the same stream
assert isinstance(dc, DeviceClusters) and dc.spec == spec and dc.sketches.spec == spec.sketches
flat = [g for c in genes for g in c]
G = len(flat)
begin = np.concatenate([[0], np.cumsum([len(c) for c in genes])])
assert dc.sketches.gene_begin.tolist() == begin.tolist() and tuple(dc.cluster.shape) == (G,)
# the reference, from the genes' own translations
strings = [g.translate(include_stop=False).encode("ascii") for g in flat]
sketch, count, windows, rows = sk_ref.sketches_ref(strings, 5, 32, "protein", 0, sk_ref.default_classes("X"))
want = ref.cluster(rows, windows.tolist(), 32, 8, 1, 2, 8)


def agrees(d, r, shift=0):
    assert (d.n_clusters, d.n_edges) == (r["n_clusters"], r["n_edges"])
    for t in (d.cluster, d.representatives, d.sizes, d.edges, d.edge_shared, d.edge_union):
        assert t.is_cuda and t.dtype == torch.int64
    assert d.cluster.cpu().tolist() == r["cluster"] and d.representatives.cpu().tolist() == r["representatives"]
    assert d.sizes.cpu().tolist() == r["sizes"] and [tuple(x) for x in d.edges.cpu().tolist()] == r["edges"]
    assert d.edge_shared.cpu().tolist() == r["edge_shared"] and d.edge_union.cpu().tolist() == r["edge_union"]


agrees(dc, want)
assert int(biggest) == max(want["sizes"])
# what it means: the near-copies in one cluster, the stranger's genes elsewhere
index = {id(g): k for k, g in enumerate(flat)}
copies = [index[id(gene_of)] for gene_of in [next(g for g in genes[0] if (g.begin, g.end, g.strand) == (gene.begin, gene.end, 1))]
          + [planted(genes, i) for i in (1, 2, 3)]]
cl = dc.cluster.cpu().tolist()
assert len({cl[k] for k in copies}) == 1, [cl[k] for k in copies]
assert len(genes[4]) > 0 and all(cl[k] != cl[copies[0]] for k in range(int(begin[4]), int(begin[5])))
assert want["sizes"][cl[copies[0]]] >= 4
# the same as the sketches of the same request, clustered
genes2, ds = finder.find_sketches_batch(seqs, spec.sketches)
assert [[(g.begin, g.end, g.strand) for g in c] for c in genes2] == [[(g.begin, g.end, g.strand) for g in c] for c in genes]
assert np.array_equal(ds.sketches.cpu().numpy(), sketch) and np.array_equal(ds.windows.cpu().numpy(), windows)
two = ds.cluster(spec)
agrees(two, want)
assert two.sketches is ds
for name in ("cluster", "representatives", "sizes", "edges", "edge_shared", "edge_union"):
    assert torch.equal(getattr(two, name), getattr(dc, name)), name
# two half-batches, their sketches concatenated, on a context of our own
ctx = _cabi.Context(0)
_, da = finder.find_sketches_batch(seqs[:2], spec.sketches)
_, db = finder.find_sketches_batch(seqs[2:], spec.sketches)
cat = lambda x, y: torch.cat([x, y]).contiguous()
merged = ctx.cluster_sketches(cat(da.sketches, db.sketches), cat(da.counts, db.counts), spec, cat(da.windows, db.windows))
agrees(merged, want)                                       # (the index shift is that of the concatenation: record g of the second half is da.n + g)
assert da.n + db.n == G and da.n == int(begin[2])
# equal weights, and out=
out = tuple(torch.full(shape, -5, dtype=torch.int64, device="cuda") for shape in ((G,), (G,), (G,), (7, 2), (7,), (7,)))
flatw = ctx.cluster_sketches(ds.sketches, ds.counts, spec, None, out=out)
r0 = ref.cluster(rows, None, 32, 8, 1, 2, 8)
assert flatw.cluster is out[0] and flatw.n_edges == r0["n_edges"] and flatw.cluster.cpu().tolist() == r0["cluster"]
assert flatw.representatives.cpu().tolist() == r0["representatives"] and out[1][flatw.n_clusters:].eq(-5).all()
w7 = min(7, r0["n_edges"])
assert [tuple(x) for x in flatw.edges.cpu().tolist()] == r0["edges"][:w7] and out[3][w7:].eq(-5).all()
ctx.close()
print("find_clusters_batch ok: %d genes, %d clusters, %d edges, the planted gene's cluster has %d members"
      % (G, dc.n_clusters, dc.n_edges, want["sizes"][cl[copies[0]]]))
'''


def test_find_clusters_batch_in_a_fresh_process(tmp_path):
    """torch is imported by the child alone (this process holds the library's HIP runtime and gets no second one); `out=` omitted
    allocates the tensors under torch's current stream.  The child says so when torch sees no GPU, and the test is skipped."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "torch_protein_clusters.py"
    script.write_text(FINDER_SCRIPT)
    done = subprocess.run([sys.executable, str(script), root], timeout=300, capture_output=True, text=True)
    assert done.returncode == 0, "child ended with %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    if "torch sees no GPU" in done.stdout:
        pytest.skip("torch sees no GPU")
    assert "find_clusters_batch ok" in done.stdout
