"""Edges verified by banded edit distance on the device, and the components of a caller's edges (pga_align_pairs, pga_cluster_edges,
ProteinAlignments, DeviceProteins.align, Context.align_pairs, DeviceClusters.relink, Context.cluster_edges,
GeneFinder.find_verified_clusters_batch).

Every expected value comes from the plain-Python restatement of the rules (tests/protein_alignments_ref.py: a full-matrix DP, no
band) -- never from the code under test -- and the device must give the same integers.  Rows are put straight into device memory
(tests/hip_mem.py, no torch), between filler elements that no row holds, so the kernel sees shapes no genome would give.  Every
output lies inside an allocation full of a canary byte, and the whole allocation is compared."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hip_mem
from tests import protein_alignments_ref as ref
from tests import protein_clusters_ref as cl_ref

pytestmark = pytest.mark.gpu

CANARY = 0xA5
DTYPES = {1: np.uint8, 4: np.int32, 8: np.int64}


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
    """A pointer into somebody's device memory with a shape: what the Python layer takes."""

    def __init__(self, ptr, shape, typestr="<i8", strides=None):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}


class Target:
    """Allocations full of a fill byte, and in each an int64 tensor of `shapes[k]` that begins 8 bytes into it with `slack` elements
    behind.  `given`: which of them are passed at all."""

    def __init__(self, shapes, given=None, slack=5, fill=CANARY):
        self.shapes = [tuple(s) for s in shapes]
        self.given = tuple(given) if given is not None else (True,) * len(shapes)
        self.before = [np.full(8 * (1 + int(np.prod(s)) + slack), fill, np.uint8) for s in self.shapes]
        self.mem = [keep(hip_mem.DeviceArray.from_numpy(b)) for b in self.before]
        self.ptr = [m.ptr + 8 if on else None for m, on in zip(self.mem, self.given)]
        self.out = tuple(View(m.ptr + 8, s) if on else None for m, s, on in zip(self.mem, self.shapes, self.given))

    def read(self):
        return [m.to_numpy(np.int64) for m in self.mem]

    def expect(self, want):
        """what the whole allocations must hold when tensor k got the values `want[k]` in its first elements"""
        out = [b.view(np.int64).copy() for b in self.before]
        for e, x, on in zip(out, want, self.given):
            if on:
                x = np.asarray(x, np.int64).reshape(-1)
                e[1:1 + len(x)] = x
        return out

    def untouched(self):
        return all(np.array_equal(m.to_numpy(np.uint8), b) for m, b in zip(self.mem, self.before))


def put_rows(rows, eb, lead=3, gap=2, tail=0, filler=0x5D):
    """The rows in one device allocation of elements of `eb` bytes: `lead` filler elements, then every row with `gap` filler elements
    behind it, `tail` more at the end.  Returns (the allocation, row_begin, row_len, n_elems)."""
    dt = DTYPES[eb]
    begin, flat, at = [], [], lead
    for row in rows:
        begin.append(at)
        flat += list(row) + [filler] * gap
        at += len(row) + gap
    n_elems = at - gap + tail if rows else lead + tail
    host = np.full(max(lead + len(flat) + tail, 1), filler, dt)
    host[lead:lead + len(flat)] = np.asarray(flat, np.int64).astype(dt) if flat else []
    return keep(hip_mem.DeviceArray.from_numpy(host)), np.asarray(begin, np.int64), np.asarray([len(r) for r in rows], np.int64), n_elems


def raw_align(ctx, tok, n_elems, begin, lens, pairs, P, opts, dist, passed, G=None):
    """the C call itself: (rc, message)"""
    from pyrodigal_amd import _cabi
    o = _cabi.AlignOpts()
    o.elem_bytes, o.max_distance, o.num, o.den = opts
    vp = ctypes.c_void_p
    G = len(lens) if G is None else G
    rc = ctx.L.pga_align_pairs(ctx.h, vp(tok), n_elems, vp(begin.ctypes.data if begin is not None else None),
                               vp(lens.ctypes.data if lens is not None else None), G, vp(pairs), P, ctypes.byref(o), vp(dist), vp(passed), None)
    return rc, ctx.L.pga_last_error(ctx.h).decode()


def decided_without_a_dp(rows, pairs, K):
    G = len(rows)
    return sum(1 for a, b in pairs if not (0 <= a < G and 0 <= b < G) or a == b or abs(len(rows[a]) - len(rows[b])) > K)


def check(ctx, rows, pairs, K, num=9, den=10, eb=1, with_pass=True, fast=False, want=None, **layout):
    """One call on injected rows against the reference: both allocations whole, and the statistics.  Returns (distance, passed)."""
    if want is None:
        want = ref.align_pairs(rows, pairs, K, num, den, ref.edit_distance_rows if fast else ref.edit_distance)
    d_tok, begin, lens, n_elems = put_rows(rows, eb, **layout)
    P = len(pairs)
    d_pairs = keep(hip_mem.DeviceArray.from_numpy(np.asarray(pairs, np.int64).reshape(P, 2)))
    t = Target([(P,), (P,)], (True, with_pass))
    rc, msg = raw_align(ctx, d_tok.ptr, n_elems, begin, lens, d_pairs.ptr, P, (eb, K, num, den), t.ptr[0], t.ptr[1])
    assert rc == 0, msg
    got, exp = t.read(), t.expect(want)
    bad = np.flatnonzero(got[0] != exp[0])
    assert len(bad) == 0, ("distance", [(int(i) - 1, int(got[0][i]), int(exp[0][i])) for i in bad[:8]])
    assert np.array_equal(got[1], exp[1]), "passed"
    quick = decided_without_a_dp(rows, pairs, K)
    assert ctx.align_stats() == {"pairs": P, "decided": quick, "aligned": P - quick, "passed": sum(want[1])}
    return want


def distinct(n, start=1000):
    return list(range(start, start + n))


# ---- 1. no pair, no row, a row with itself, indices out of range -----------------------------------------------------------------------------
def test_no_pair_no_row_and_indices_out_of_range(ctx):
    rows = [[1, 2, 3], [1, 2, 4]]
    d_tok, begin, lens, n_elems = put_rows(rows, 1)
    t = Target([(0,), (0,)])
    rc, msg = raw_align(ctx, d_tok.ptr, n_elems, begin, lens, None, 0, (1, 4, 9, 10), None, None)      # P = 0: no pointer is looked at
    assert rc == 0 and t.untouched(), msg
    assert ctx.align_stats() == {"pairs": 0, "decided": 0, "aligned": 0, "passed": 0}
    # G = 0 with pairs: every index is out of range, and there are no tokens to read
    t = Target([(3,), (3,)])
    d_pairs = keep(hip_mem.DeviceArray.from_numpy(np.asarray([(0, 0), (0, 1), (-1, 5)], np.int64)))
    rc, msg = raw_align(ctx, None, 0, None, None, d_pairs.ptr, 3, (1, 4, 9, 10), t.ptr[0], t.ptr[1], G=0)
    assert rc == 0, msg
    assert all(np.array_equal(g, e) for g, e in zip(t.read(), t.expect(([-1, -1, -1], [0, 0, 0]))))
    w = check(ctx, rows, [(0, 0), (1, 1), (-1, 0), (0, -1), (2, 0), (1, 2), (0, 1), (1, 0), (1 << 40, 0), (-(1 << 62), 1)], 4, 1, 2)
    assert w == ([0, 0, -1, -1, -1, -1, 1, 1, -1, -1], [1, 1, 0, 0, 0, 0, 1, 1, 0, 0])


# ---- 2. empty rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 1, 31, 32, 255])
def test_empty_rows(ctx, K):
    rows = [[], [], [7] * K, [7] * (K + 1), list(range(K))]
    w = check(ctx, rows, [(0, 1), (0, 2), (2, 0), (0, 3), (3, 0), (0, 4), (2, 4)], K, 1, 1 << 20)
    assert w[0][:5] == [0, K, K, K + 1, K + 1]


# ---- 3. equal rows ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 7, 32, 255])
def test_equal_rows_at_the_edges_of_waves_and_chunks(ctx, K):
    rng = np.random.default_rng(K)
    rows, pairs = [], []
    for n in (1, 63, 64, 65, 127, 128, 129, 513):
        r = rng.integers(0, 4, size=n).tolist()
        pairs.append((len(rows), len(rows) + 1))
        rows += [r, list(r)]
    w = check(ctx, rows, pairs, K, 1, 1, fast=True)
    assert w == ([0] * 8, [1] * 8)


# ---- 4. the distance exactly at the cap and one beyond it, for every kernel variant ------------------------------------------------------
def substituted(row, where, new=5000):
    out = list(row)
    for k, p in enumerate(where):
        out[p] = new + k
    return out


@pytest.mark.parametrize("K", [0, 1, 15, 16, 31, 32, 63, 64, 127, 128, 255])
def test_the_distance_at_the_cap_and_one_beyond(ctx, K):
    """Rows of distinct elements: e substitutions by new elements give the distance e exactly.  31 | 32, 63 | 64 and 127 | 128 are
    where the host changes the diagonals a lane holds (1, 2, 4, 8)."""
    n = 2 * K + 70
    a = distinct(n)
    spread = lambda e: [(k * n) // max(e, 1) for k in range(e)]      # noqa: E731
    rows = [a, substituted(a, spread(K)), substituted(a, spread(K + 1)), substituted(a, spread(max(K - 1, 0)))]
    w = check(ctx, rows, [(0, 1), (0, 2), (0, 3), (1, 0), (2, 0)], K, 1, 2, eb=4, fast=True)
    assert w[0] == [K, K + 1, max(K - 1, 0), K, K + 1] and w[1] == [1, 0, 1, 1, 0]


# ---- 5. lengths that differ by the cap, and the band's outermost diagonal -----------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5, 31, 32, 63, 64, 128, 255])
def test_length_differences_and_the_outermost_diagonal(ctx, K):
    n = 150
    a = distinct(n)
    head, tail = distinct(K, 7000), distinct(K + 1, 8000)
    rows = [a, head + a, a + head, a + tail, tail + a, head[:1] + a + head[1:]]
    pairs = [(0, 1), (1, 0), (0, 2), (2, 0),        # B is A behind K leading elements: the best path runs along the outermost diagonal; and A behind B
             (0, 3), (4, 0),                          # K + 1 more elements: decided by the lengths
             (1, 2),                                  # the same length, K leading against K trailing: 2 K edits, beyond the cap
             (0, 5)]
    w = check(ctx, rows, pairs, K, 1, 2, eb=4, fast=True)
    assert w[0] == [K, K, K, K, K + 1, K + 1, K + 1, K]
    assert decided_without_a_dp(rows, pairs, K) == 2


# ---- 6. single edits, substitutions only, inserts and deletes in turn -----------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8, 40])
def test_edits_at_the_ends_and_in_turn(ctx, K):
    n = 200
    a = distinct(n)
    first, last = substituted(a, [0]), substituted(a, [n - 1])
    subs = substituted(a, range(0, n, n // K)[:K])
    turn = list(a)                                     # delete one element, insert another further on, K // 2 times each
    for k in range(K // 2):
        del turn[5 + 8 * k]
        turn.insert(9 + 8 * k, 9000 + k)
    rows = [a, first, last, subs, turn, a[1:], a[:-1]]
    w = check(ctx, rows, [(0, 1), (0, 2), (1, 2), (0, 3), (0, 4), (4, 0), (0, 5), (0, 6), (5, 6)], K, 1, 2, eb=4, fast=True)
    assert w[0][:5] == [1, 1, min(2, K + 1), K, 2 * (K // 2)] and w[0][6:] == [1, 1, min(2, K + 1)]


# ---- 7. a pair whose only cheap path leaves the band -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [0, 3, 31, 32, 100])
def test_a_path_outside_the_band_is_not_found_and_nothing_smaller_is_reported(ctx, K):
    """A = S T, B = U S with |T| = |U| = K + 1: the lengths are equal, so the DP runs; the cheap alignment shifts S by K + 1 diagonals,
    costs 2 K + 2, and lies outside the band.  Inside the band nothing costs K or less either: the answer is "more than K"."""
    s = distinct(300)
    rows = [s + distinct(K + 1, 7000), distinct(K + 1, 8000) + s]
    assert ref.edit_distance_rows(rows[0], rows[1]) == 2 * K + 2
    w = check(ctx, rows, [(0, 1), (1, 0)], K, 1, 2, eb=4, fast=True)
    assert w == ([K + 1, K + 1], [0, 0])
    assert ctx.align_stats()["aligned"] == 2


# ---- 8. element types ---------------------------------------------------------------------------------------------------------------------------
def test_elements_are_compared_over_all_their_bits(ctx):
    base = [3, 1 << 40, 5, -7, (1 << 62) + 9, 0, 11] * 10
    high = list(base)
    high[1] = 0                                        # differs from 1 << 40 only in bit 40
    high[4 + 7 * 9] = 9                                # differs from (1 << 62) + 9 only in bit 62
    w = check(ctx, [base, high], [(0, 1)], 4, 1, 2, eb=8)
    assert w == ([2], [1])
    neg = [-1, -2, -(1 << 31), (1 << 31) - 1, 0, 255, -256] * 10
    other = list(neg)
    other[0], other[2] = 1, (1 << 31) - 1
    w = check(ctx, [neg, other, [-x - 1 for x in neg]], [(0, 1), (0, 2)], 4, 1, 2, eb=4)
    assert w[0][0] == 2
    # uint8 rows at odd element offsets, every lead 0 .. 7, rows 1 and 3 elements apart
    rng = np.random.default_rng(8)
    a = rng.integers(0, 256, size=97).tolist()
    b = list(a)
    b[0], b[50], b[96] = b[0] ^ 0x80, b[50] ^ 1, b[96] ^ 0x10
    for lead in range(8):
        for gap in (1, 3):
            w = check(ctx, [a, b, a[:-1]], [(0, 1), (0, 2), (2, 1)], 5, 1, 2, eb=1, lead=lead, gap=gap)
            assert w[0] == [3, 1, 3]


def test_a_row_that_ends_at_the_last_element(ctx):
    a = distinct(70, 0)
    for eb in (1, 4, 8):
        w = check(ctx, [a, substituted(a, [69], 200)], [(0, 1), (1, 0)], 2, 1, 2, eb=eb, gap=0, lead=1)      # row 1 ends at n_elems
        assert w[0] == [1, 1]


# ---- 9. the padded layout ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eb", [1, 4, 8])
def test_the_pad_of_a_padded_tensor_is_not_read(ctx, eb):
    from pyrodigal_amd import ProteinAlignments, _cabi
    rng = np.random.default_rng(40 + eb)
    G, W, S = 6, 90, 101                               # rows 101 elements apart, 90 of them the tensor's
    base = rng.integers(0, 20, size=80).tolist()
    rows = [base, base[:60], substituted(base, [3, 70], 100), base[:60] + [21], [], base[:79]]
    host = rng.integers(30, 120, size=G * S).astype(DTYPES[eb])      # garbage everywhere, different in every pad
    for g, r in enumerate(rows):
        host[g * S:g * S + len(r)] = r
    d_tok = keep(hip_mem.DeviceArray.from_numpy(host))
    typestr = "|u1" if eb == 1 else np.dtype(DTYPES[eb]).str
    tokens = View(d_tok.ptr, (G, W), typestr, (S * eb, eb))
    lens = np.asarray([len(r) for r in rows], np.int64)
    proteins = _cabi.DeviceProteins(tokens, lens, None, None, 0, ctx.L, ctx.h)
    pairs = [(0, 1), (0, 2), (1, 3), (4, 1), (0, 5), (4, 4), (5, 2), (6, 0)]
    spec = ProteinAlignments(20, (9, 10))
    want = ref.align_pairs(rows, pairs, 20, 9, 10)
    assert want[0] == [20, 2, 1, 21, 1, 0, 3, -1]
    d_pairs = keep(hip_mem.DeviceArray.from_numpy(np.asarray(pairs, np.int64)))
    t = Target([(len(pairs),), (len(pairs),)])
    out = proteins.align(View(d_pairs.ptr, (len(pairs), 2)), spec, out=t.out)
    assert out[0] is t.out[0] and all(np.array_equal(g, e) for g, e in zip(t.read(), t.expect(want)))
    # the same rows through Context.align_pairs, the offsets spelled out
    t = Target([(len(pairs),), (len(pairs),)], (True, False))
    ctx.align_pairs(tokens, np.arange(G) * S, lens, View(d_pairs.ptr, (len(pairs), 2)), spec, out=t.out)
    assert all(np.array_equal(g, e) for g, e in zip(t.read(), t.expect(want)))


# ---- 10. long rows ----------------------------------------------------------------------------------------------------------------------------
def test_five_thousand_elements_and_forty_edits(ctx):
    rng = np.random.default_rng(5000)
    a = rng.integers(0, 20, size=5000).tolist()
    b = list(a)
    for k in range(40):                                # spread over the row: substitutions, insertions and deletions in turn
        p = 60 + k * 120
        if k % 3 == 0:
            b[p] = (b[p] + 1 + k % 19) % 20
        elif k % 3 == 1:
            b.insert(p, 20)
        else:
            del b[p]
    d = ref.edit_distance_rows(a, b)
    assert 30 <= d <= 40
    for K in (d - 1, d, 64, 255):
        w = check(ctx, [a, b], [(0, 1), (1, 0)], K, 99, 100, want=([min(d, K + 1)] * 2, [1 if d <= K else 0] * 2))
        assert w[0][0] == min(d, K + 1)


# ---- 11. the threshold ------------------------------------------------------------------------------------------------------------------------
def test_the_threshold_met_exactly_and_missed_by_one_edit(ctx):
    a = distinct(20, 0)
    rows = [a, substituted(a, [0, 1], 90), substituted(a, [0, 1, 2], 90), a[:-1], a[:-2]]
    w = check(ctx, rows, [(0, 1), (0, 2), (0, 3), (3, 4)], 5, 9, 10)
    assert w == ([2, 3, 1, 1], [1, 0, 1, 1])           # 2 * 10 == 1 * 20; 3 * 10 > 1 * 20; one deletion is well inside
    w = check(ctx, rows, [(0, 1), (0, 2), (0, 3), (3, 4)], 5, 18, 20)
    assert w[1] == [1, 0, 1, 1]
    w = check(ctx, rows, [(0, 3), (3, 4)], 5, 19, 20)  # 1 * 20 == 1 * 20 over the longer row, 20; 1 * 20 > 1 * 19
    assert w == ([1, 1], [1, 0])
    w = check(ctx, rows, [(0, 2)], 2, 1, 2)            # within the identity and beyond max_distance
    assert w == ([3], [0])
    w = check(ctx, rows, [(0, 1), (0, 2)], 3, 1 << 20, 1 << 20)      # num == den: only identical rows pass
    assert w[1] == [0, 0]


def test_without_d_pass(ctx):
    a = distinct(100)
    check(ctx, [a, substituted(a, [5, 50]), a[3:]], [(0, 1), (1, 2), (2, 2), (0, 9)], 6, 1, 2, eb=4, with_pass=False)


# ---- 12. random pairs -------------------------------------------------------------------------------------------------------------------------
def random_pairs(K):
    rng = np.random.default_rng(7 + K)
    rows, pairs = [], []
    for _ in range(300):
        a = rng.integers(0, 4, size=int(rng.integers(0, 201))).tolist()
        b = list(a)
        for _ in range(int(rng.integers(0, 2 * K + 2))):
            op = int(rng.integers(0, 3))
            if op == 0 and b:
                b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 4))
            elif op == 1:
                b.insert(int(rng.integers(0, len(b) + 1)), int(rng.integers(0, 4)))
            elif b:
                del b[int(rng.integers(0, len(b)))]
        pairs.append((len(rows), len(rows) + 1))
        rows += [a, b]
    return rows, pairs


@pytest.mark.parametrize("K", [0, 1, 5, 31, 32])
def test_random_pairs(ctx, K):
    rows, pairs = random_pairs(K)
    ed = [ref.edit_distance_rows(rows[a], rows[b]) for a, b in pairs]
    if K == 0:
        assert sum(1 for d in ed if d == 0) >= 40 and sum(1 for d in ed if d > 0) >= 40
    else:
        assert sum(1 for d in ed if 0 < d <= K) >= 40 and sum(1 for d in ed if d > K) >= 40
    want = ([min(d, K + 1) for d in ed],
            [1 if d <= K and d * 10 <= max(len(rows[a]), len(rows[b])) else 0 for d, (a, b) in zip(ed, pairs)])
    check(ctx, rows, pairs, K, 9, 10, want=want)


# ---- 13. memory of earlier calls --------------------------------------------------------------------------------------------------------------
def test_the_result_does_not_depend_on_earlier_calls(ctx):
    a = distinct(90)
    small = ([a, substituted(a, [1, 40, 80]), a[2:]], [(0, 1), (1, 2), (0, 2)], 6, 1, 2)
    first = check(ctx, *small, eb=4)
    rows, pairs = random_pairs(5)
    check(ctx, rows, pairs, 5, 9, 10, fast=True)       # larger: more rows in the lease, and the wave's LDS full of its tokens
    assert check(ctx, *small, eb=4) == first
    big = distinct(700)
    check(ctx, [big, substituted(big, range(0, 700, 7))], [(0, 1)], 200, 1, 2, eb=8, fast=True)      # another shape: 8 diagonals a lane, int64
    assert check(ctx, *small, eb=4) == first


# ---- 14. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_host_and_leave_the_context_usable(ctx):
    from pyrodigal_amd import ProteinAlignments, _cabi
    a = distinct(50, 0)
    rows = [a, substituted(a, [7], 90), a[:40]]
    d_tok, begin, lens, n_elems = put_rows(rows, 4)
    pairs = [(0, 1), (1, 2), (2, 0)]
    d_pairs = keep(hip_mem.DeviceArray.from_numpy(np.asarray(pairs, np.int64)))
    t = Target([(3,), (3,)])
    host = np.zeros(64, np.int64)
    good = dict(tok=d_tok.ptr, n_elems=n_elems, begin=begin, lens=lens, pairs=d_pairs.ptr, P=3, opts=(4, 8, 9, 10), dist=t.ptr[0], passed=t.ptr[1], G=None)

    def call(**change):
        x = dict(good, **change)
        return raw_align(ctx, x["tok"], x["n_elems"], x["begin"], x["lens"], x["pairs"], x["P"], x["opts"], x["dist"], x["passed"], x["G"])

    def moved(arr, g, v):
        out = arr.copy()
        out[g] = v
        return out

    for what, kw, word in (("elem_bytes = 2", dict(opts=(2, 8, 9, 10)), "elem_bytes must be 1, 4 or 8, not 2"),
                           ("a negative max_distance", dict(opts=(4, -1, 9, 10)), "max_distance = -1"), ("max_distance = 256", dict(opts=(4, 256, 9, 10)), "max_distance = 256"),
                           ("num = 0", dict(opts=(4, 8, 0, 10)), "num / den"), ("num above den", dict(opts=(4, 8, 11, 10)), "num / den"),
                           ("den above 2^20", dict(opts=(4, 8, 1, (1 << 20) + 1)), "num / den"),
                           ("more than 2^31 - 1 pairs", dict(P=1 << 31), "2^31 - 1 pairs"), ("negative pairs", dict(P=-1), "bad arguments"),
                           ("negative rows", dict(G=-1), "bad arguments"), ("negative elements", dict(n_elems=-1), "bad arguments"),
                           ("no row_begin", dict(begin=None), "bad arguments"), ("no row_len", dict(lens=None, G=3), "bad arguments"),
                           ("a row that begins before the tensor", dict(begin=moved(begin, 1, -1)), "row 1 is elements -1"),
                           ("a row that ends behind the tensor", dict(n_elems=n_elems - 1), "row 2 is elements"),
                           ("a negative length", dict(lens=moved(lens, 0, -1)), "row 0 has length -1"),
                           ("a length above 2^30", dict(lens=moved(lens, 2, (1 << 30) + 1), n_elems=1 << 40), "row 2 has length"),
                           ("no tokens", dict(tok=None), "d_tokens is NULL"), ("no pairs", dict(pairs=None), "d_pairs is NULL"),
                           ("no d_distance", dict(dist=None), "d_distance is NULL"),
                           ("misaligned tokens", dict(tok=d_tok.ptr + 2), "d_tokens is not aligned to its 4-byte"),
                           ("misaligned pairs", dict(pairs=d_pairs.ptr + 4), "d_pairs is not aligned"),
                           ("a misaligned d_distance", dict(dist=t.ptr[0] + 1), "d_distance is not aligned"),
                           ("a misaligned d_pass", dict(passed=t.ptr[1] + 4), "d_pass is not aligned"),
                           ("host tokens", dict(tok=host.ctypes.data), "d_tokens is not device memory"),
                           ("host pairs", dict(pairs=host.ctypes.data), "d_pairs is not device memory"),
                           ("a host d_distance", dict(dist=host.ctypes.data), "d_distance is not device memory"),
                           ("a host d_pass", dict(passed=host.ctypes.data), "d_pass is not device memory")):
        rc, msg = call(**kw)
        assert rc == _cabi.PGA_EINVAL and word in msg and msg.startswith("pga_align_pairs: "), (what, rc, msg)
    rc, msg = raw_align(ctx, d_tok.ptr, n_elems, begin, lens, d_pairs.ptr, 3, (4, 8, 9, 10), t.ptr[0], t.ptr[1], G=1 << 31)
    assert rc == _cabi.PGA_EINVAL and "2^31 - 1 rows" in msg
    # the Python layer, on device memory
    spec = ProteinAlignments(8, (9, 10))
    tokens = View(d_tok.ptr, (n_elems,), "<i4")
    with pytest.raises(ValueError, match="not device memory"):
        ctx.align_pairs(tokens, begin, lens, View(d_pairs.ptr, (3, 2)), spec, out=(View(host.ctypes.data, (3,)), None))
    with pytest.raises(ValueError, match="row 2 is elements"):
        ctx.align_pairs(View(d_tok.ptr, (n_elems - 1,), "<i4"), begin, lens, View(d_pairs.ptr, (3, 2)), spec, out=t.out)
    assert np.all(host == 0) and t.untouched()         # nothing was written anywhere
    # the context runs a good call afterwards, through the Python layer
    want = ref.align_pairs(rows, pairs, 8, 9, 10)
    out = ctx.align_pairs(tokens, begin.tolist(), lens.tolist(), View(d_pairs.ptr, (3, 2)), spec, out=t.out)
    assert out == t.out and all(np.array_equal(g, e) for g, e in zip(t.read(), t.expect(want))) and want[0] == [1, 9, 9]


# ==== pga_cluster_edges ==========================================================================================================================
def raw_edges(ctx, edges, keep_, E, n, weight, ptr, capacity):
    """the C call itself: (rc, message, n_clusters, n_used)"""
    nc, nu = ctypes.c_int64(-7), ctypes.c_int64(-7)
    vp = ctypes.c_void_p
    rc = ctx.L.pga_cluster_edges(ctx.h, vp(edges), vp(keep_), E, n, vp(weight), vp(ptr[0]), vp(ptr[1]), vp(ptr[2]), capacity, None,
                                 ctypes.byref(nc), ctypes.byref(nu))
    return rc, ctx.L.pga_last_error(ctx.h).decode(), nc.value, nu.value


def check_edges(ctx, edges, n, mask=None, weights=None, given=(True, True, True), cap=None):
    """One call on injected edges against the reference: every allocation whole, and both counts.  Returns the reference's result."""
    r = ref.cluster_edges(edges, mask, n, weights)
    E = len(edges)
    d_e = keep(hip_mem.DeviceArray.from_numpy(np.asarray(edges, np.int64).reshape(E, 2)))
    d_k = None if mask is None else keep(hip_mem.DeviceArray.from_numpy(np.asarray(mask, np.int64).reshape(E)))
    d_w = None if weights is None else keep(hip_mem.DeviceArray.from_numpy(np.asarray(weights, np.int64).reshape(n)))
    cap = n if cap is None else cap
    t = Target([(n,), (cap,), (cap,)], given)
    rc, msg, nc, nu = raw_edges(ctx, d_e.ptr if E else None, d_k.ptr if d_k and E else None, E, n, d_w.ptr if d_w else None, t.ptr, cap)
    assert rc == 0, msg
    assert (nc, nu) == (r["n_clusters"], r["n_used"])
    for name, g, e in zip(("cluster", "representatives", "sizes"), t.read(), t.expect((r["cluster"], r["representatives"], r["sizes"]))):
        assert np.array_equal(g, e), name
    return r


def test_no_record_no_edge_and_every_edge(ctx):
    t = Target([(0,), (0,), (0,)])
    rc, msg, nc, nu = raw_edges(ctx, None, None, 0, 0, None, [None] * 3, 0)
    assert (rc, nc, nu) == (0, 0, 0), msg
    d_e = keep(hip_mem.DeviceArray.from_numpy(np.asarray([(0, 1)], np.int64)))
    rc, msg, nc, nu = raw_edges(ctx, d_e.ptr, None, 1, 0, None, t.ptr, 0)        # no record: the edge is out of range, and nothing runs
    assert (rc, nc, nu) == (0, 0, 0) and t.untouched(), msg
    r = check_edges(ctx, [], 5)
    assert r["cluster"] == [0, 1, 2, 3, 4] and r["n_used"] == 0
    r = check_edges(ctx, [], 1, weights=[3])
    assert r["representatives"] == [0]
    edges = [(0, 1), (3, 3), (5, 2), (7, 0), (-1, 2), (4, 9), (1, 7), (8, 0), (0, 1 << 33), (2, 2)]
    r = check_edges(ctx, edges, 8)
    assert r["n_used"] == 6 and r["cluster"] == [0, 0, 1, 2, 3, 1, 4, 0]        # out of range: ignored; an edge of a record with itself: counted
    r = check_edges(ctx, edges, 8, mask=[1, 1, 0, -5, 1, 1, 0, 1, 1, 1 << 40], weights=[0, 0, 0, 0, 0, 5, 0, 9])
    assert r["n_used"] == 4 and r["cluster"] == [0, 0, 1, 2, 3, 4, 5, 0] and r["representatives"][0] == 7
    r = check_edges(ctx, edges, 8, mask=[0] * 10)
    assert r["n_used"] == 0 and r["n_clusters"] == 8


def test_a_chain_of_three_thousand_in_any_order(ctx):
    N = 3000
    edges = [(i + 1, i) if i % 3 else (i, i + 1) for i in range(N - 1)]
    order = np.random.default_rng(3).permutation(N - 1)
    edges = [edges[int(k)] for k in order]
    r = check_edges(ctx, edges, N, weights=[(i * 7919) % 13 for i in range(N)])
    assert r["cluster"] == [0] * N and r["sizes"] == [N] and r["n_used"] == N - 1
    r = check_edges(ctx, edges, N, mask=[0 if min(e) % 1000 == 999 else 1 for e in edges])      # cut in three
    assert r["sizes"] == [1000, 1000, 1000] and r["representatives"] == [0, 1000, 2000]


def test_weights_ties_capacities_and_outputs_left_out(ctx):
    rng = np.random.default_rng(11)
    n = 400
    edges = [tuple(int(x) for x in rng.integers(-3, n + 3, size=2)) for _ in range(260)]
    mask = rng.integers(0, 3, size=260).tolist()
    for w in (None, [4] * n, rng.integers(0, 3, size=n).tolist(), rng.integers(-(1 << 62), 1 << 62, size=n).tolist()):
        r = check_edges(ctx, edges, n, mask, w)
        assert max(r["sizes"]) > 2 and r["n_used"] < sum(1 for k in mask if k)
    w = rng.integers(0, 3, size=n).tolist()
    check_edges(ctx, edges, n, mask, w, cap=n + 9)
    for given in ((True, False, False), (True, True, False), (True, False, True)):
        check_edges(ctx, edges, n, mask, w, given=given)
    # earlier calls: a larger one and another shape in between
    first = check_edges(ctx, edges[:50], 60, None, w[:60])
    check_edges(ctx, [(i, i + 1) for i in range(4999)], 5000)
    assert check_edges(ctx, edges[:50], 60, None, w[:60]) == first
    check_edges(ctx, [], 2000, weights=list(range(2000)))
    assert check_edges(ctx, edges[:50], 60, None, w[:60]) == first


def test_cluster_edges_refusals(ctx):
    from pyrodigal_amd import _cabi
    n, E = 50, 20
    edges = [(i, i + 1) for i in range(E)]
    d_e = keep(hip_mem.DeviceArray.from_numpy(np.asarray(edges, np.int64)))
    d_k = keep(hip_mem.DeviceArray.from_numpy(np.ones(E, np.int64)))
    d_w = keep(hip_mem.DeviceArray.from_numpy(np.arange(n, dtype=np.int64)))
    t = Target([(n,), (n,), (n,)])
    host = np.zeros(2 * n, np.int64)
    good = dict(edges=d_e.ptr, keep=d_k.ptr, E=E, n=n, weight=d_w.ptr, capacity=n)

    def call(**change):
        x, ptr = dict(good), list(t.ptr)
        for name, v in change.items():
            if name.startswith("p"):
                ptr[int(name[1:])] = v
            else:
                x[name] = v
        return raw_edges(ctx, x["edges"], x["keep"], x["E"], x["n"], x["weight"], ptr, x["capacity"])

    for what, kw, word in (("negative records", dict(n=-1), "bad arguments"), ("negative edges", dict(E=-1), "bad arguments"),
                           ("more than 2^31 - 1 records", dict(n=1 << 31, capacity=1 << 31), "2^31 - 1 records"),
                           ("more than 2^31 - 1 edges", dict(E=1 << 31), "2^31 - 1 edges"),
                           ("a capacity below n", dict(capacity=n - 1), "capacity = 49"), ("a negative capacity", dict(capacity=-1), "capacity = -1"),
                           ("no edges", dict(edges=None), "d_edges is NULL"), ("no d_cluster", dict(p0=None), "d_cluster is NULL"),
                           ("misaligned edges", dict(edges=d_e.ptr + 4), "d_edges is not aligned"), ("a misaligned d_keep", dict(keep=d_k.ptr + 2), "d_keep is not aligned"),
                           ("misaligned weights", dict(weight=d_w.ptr + 1), "d_weight is not aligned"), ("a misaligned d_size", dict(p2=t.ptr[2] + 4), "d_size is not aligned"),
                           ("host edges", dict(edges=host.ctypes.data), "d_edges is not device memory"), ("a host d_keep", dict(keep=host.ctypes.data), "d_keep is not device memory"),
                           ("host weights", dict(weight=host.ctypes.data), "d_weight is not device memory"),
                           ("a host d_cluster", dict(p0=host.ctypes.data), "d_cluster is not device memory"),
                           ("host representatives", dict(p1=host.ctypes.data), "d_representative is not device memory"),
                           ("host sizes", dict(p2=host.ctypes.data), "d_size is not device memory")):
        rc, msg, nc, nu = call(**kw)
        assert rc == _cabi.PGA_EINVAL and word in msg and msg.startswith("pga_cluster_edges: "), (what, rc, msg)
        assert (nc, nu) == (-7, -7), what
    assert np.all(host == 0) and t.untouched()
    # the Python layer afterwards: out= cut to the clusters
    r = ref.cluster_edges(edges, None, n, list(range(n)))
    cluster, reps, sizes, U, used = ctx.cluster_edges(View(d_e.ptr, (E, 2)), n, None, View(d_w.ptr, (n,)), out=t.out)
    assert (U, used) == (r["n_clusters"], E) and cluster is t.out[0]
    for g, e in zip(t.read(), t.expect((r["cluster"], r["representatives"], r["sizes"]))):
        assert np.array_equal(g, e)
    assert r["representatives"][0] == E


def test_relink_with_every_edge_reproduces_the_clusters_of_the_sketches(ctx):
    """The cross-check: on the edges of a DeviceClusters, with keep=None and the same weights, pga_cluster_edges gives that object's
    cluster, representatives and sizes again, exactly -- and the reference's, from the edges read back."""
    from pyrodigal_amd import ProteinClusters, ProteinSketches
    s, G = 32, 300
    rng = np.random.default_rng(500)
    rows = [sorted(set(rng.integers(0, 150, size=int(rng.integers(0, 60))).tolist()))[:s] for _ in range(G)]
    w = rng.integers(0, 6, size=G).tolist()
    sk, cnt = np.full((G, s), (1 << 63) - 1, np.int64), np.zeros(G, np.int64)
    for g, row in enumerate(rows):
        sk[g, :len(row)] = row
        cnt[g] = len(row)
    d_sk, d_cnt, d_w = (keep(hip_mem.DeviceArray.from_numpy(x)) for x in (sk, cnt, np.asarray(w, np.int64)))
    spec = ProteinClusters(ProteinSketches(5, s), 8, (1, 6), 0)
    want = cl_ref.cluster(rows, w, s, 8, 1, 6, 0)
    assert want["n_edges"] > 50 and sum(1 for x in want["sizes"] if x > 1) >= 5
    first = Target([(G,), (G,), (G,), (G * 8, 2), (G * 8,), (G * 8,)])
    dc = ctx.cluster_sketches(View(d_sk.ptr, (G, s)), View(d_cnt.ptr, (G,)), spec, View(d_w.ptr, (G,)), out=first.out)
    assert (dc.n_clusters, dc.n_edges) == (want["n_clusters"], want["n_edges"])
    E = dc.n_edges
    dc.edges = View(first.ptr[3], (E, 2))               # (a View has no slices: the first E edges, as the layer would cut a tensor)
    again = Target([(G,), (G,), (G,)])
    cluster, reps, sizes, U, used = dc.relink(None, View(d_w.ptr, (G,)), out=again.out)
    assert (U, used) == (want["n_clusters"], E)
    for k in range(3):
        assert np.array_equal(again.read()[k], first.read()[k])
    for g, e in zip(again.read(), again.expect((want["cluster"], want["representatives"], want["sizes"]))):
        assert np.array_equal(g, e)
    # a mask of the caller's own over those edges, against the reference
    edges = [tuple(x) for x in first.read()[3][1:1 + 2 * E].reshape(E, 2).tolist()]
    assert edges == want["edges"]
    mask = [1 if sh * 3 >= m else 0 for sh, m in zip(want["edge_shared"], want["edge_union"])]
    assert 0 < sum(mask) < E
    d_k = keep(hip_mem.DeviceArray.from_numpy(np.asarray(mask, np.int64)))
    r = ref.cluster_edges(edges, mask, G, w)
    cluster, reps, sizes, U, used = dc.relink(View(d_k.ptr, (E,)), View(d_w.ptr, (G,)), out=again.out)
    assert (U, used) == (r["n_clusters"], sum(mask)) and r["n_clusters"] > want["n_clusters"]
    got = again.read()
    assert got[0][1:1 + G].tolist() == r["cluster"] and got[1][1:1 + U].tolist() == r["representatives"] and got[2][1:1 + U].tolist() == r["sizes"]


# ==== through the finder =========================================================================================================================
FINDER_SCRIPT = r'''
import sys
import torch                                   # first: the library then binds to the HIP runtime of torch's wheel
if not torch.cuda.is_available():
    print("torch sees no GPU")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
import numpy as np
from pyrodigal_amd import (DeviceClusters, DeviceProteins, DeviceVerifiedClusters, ProteinAlignments, ProteinClusters, ProteinSketches,
                           VerifiedClusters, benchdata, lib)
from tests import protein_alignments_ref as ref
from tests import protein_clusters_ref as cl_ref
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
K, NUM, DEN = 255, 19, 20
spec = VerifiedClusters(ProteinClusters(ProteinSketches(5, 32), probes=8, min_resemblance=(1, 2), min_union=8), ProteinAlignments(K, (NUM, DEN)))


def planted(genes, i):
    """the gene of contig i (1 .. 3) that lies over the planted one"""
    over = [g for g in genes[i] if g.strand == 1 and min(g.end, e - lo) - max(g.begin - 1, b - lo) > (e - b) // 2]
    assert len(over) == 1, (i, [(g.begin, g.end) for g in over])
    return over[0]


side = torch.cuda.Stream()
with torch.cuda.stream(side):
    genes, dv = finder.find_verified_clusters_batch(seqs, spec)
    biggest = dv.sizes.max()                                   # a consumer on the same stream
assert isinstance(dv, DeviceVerifiedClusters) and dv.spec == spec
assert isinstance(dv.candidates, DeviceClusters) and dv.candidates.spec == spec.clusters and isinstance(dv.proteins, DeviceProteins)
flat = [g for c in genes for g in c]
G = len(flat)
begin = np.concatenate([[0], np.cumsum([len(c) for c in genes])])
assert dv.proteins.gene_begin.tolist() == begin.tolist() and tuple(dv.cluster.shape) == (G,)
for t in (dv.cluster, dv.representatives, dv.sizes, dv.edge_distance, dv.edge_passed, dv.candidates.edges):
    assert t.is_cuda and t.dtype == torch.int64
# the tokens are the proteins
vocab = "ACDEFGHIKLMNPQRSTVWYX"
strings = [g.translate(include_stop=False) for g in flat]
tok = dv.proteins.tokens.cpu().numpy()
off = dv.proteins.offsets
assert dv.proteins.tokens.dtype == torch.uint8 and off[-1] == len(tok) == sum(len(s) for s in strings)
rows = [tok[off[g]:off[g + 1]].tolist() for g in range(G)]
assert rows == [[vocab.index(ch) for ch in s] for s in strings]
# the sketch stage, from the genes' own translations
sketch, count, windows, sk_rows = sk_ref.sketches_ref([s.encode("ascii") for s in strings], 5, 32, "protein", 0, sk_ref.default_classes("X"))
cand = cl_ref.cluster(sk_rows, windows.tolist(), 32, 8, 1, 2, 8)
edges = [tuple(x) for x in dv.candidates.edges.cpu().tolist()]
assert edges == cand["edges"] and dv.candidates.cluster.cpu().tolist() == cand["cluster"] and dv.candidates.n_edges == len(edges) > 0
# every tensor of the result equals the reference run on the tokens and candidate edges read back
distance, passed = ref.align_pairs(rows, edges, K, NUM, DEN, ref.edit_distance_rows)
assert dv.edge_distance.cpu().tolist() == distance and dv.edge_passed.cpu().tolist() == passed
want = ref.cluster_edges(edges, passed, G, windows.tolist())
assert dv.cluster.cpu().tolist() == want["cluster"] and dv.representatives.cpu().tolist() == want["representatives"]
assert dv.sizes.cpu().tolist() == want["sizes"] and (dv.n_clusters, dv.n_passed) == (want["n_clusters"], sum(passed))
assert int(biggest) == max(want["sizes"])
# what it means
index = {id(g): k for k, g in enumerate(flat)}
original = index[id(next(g for g in genes[0] if (g.begin, g.end, g.strand) == (gene.begin, gene.end, 1)))]
two, other_start, cut = (index[id(planted(genes, i))] for i in (1, 2, 3))
cl, before = want["cluster"], cand["cluster"]
assert 1 <= ref.edit_distance_rows(rows[original], rows[two]) <= 2 and cl[two] == cl[original]
# the case in which the verification makes a difference: the sketch stage accepts the shortened copy, the alignment refuses it
assert before[cut] == before[original] == before[two]
touching = [k for k, (x, y) in enumerate(edges) if cut in (x, y)]
assert touching and all(before[x] == before[original] for k in touching for x in edges[k])
lost = len(rows[original]) - len(rows[cut])
assert lost * DEN > (DEN - NUM) * len(rows[original])          # a tenth is gone, a twentieth may differ
for k in touching:
    x, y = edges[k]
    full = ref.edit_distance_rows(rows[x], rows[y])
    assert full * DEN > (DEN - NUM) * max(len(rows[x]), len(rows[y])) and passed[k] == 0
assert cl[cut] != cl[original] and want["sizes"][cl[cut]] == 1
assert all(cl[k] != cl[original] for k in range(int(begin[4]), int(begin[5]))) and len(genes[4]) > 0
# out=, and the same request again
out = tuple(torch.full((G + 3,), -5, dtype=torch.int64, device="cuda") for _ in range(3))
genes2, dv2 = finder.find_verified_clusters_batch(seqs, spec, out=out)
assert dv2.cluster is out[0] and out[0][:G].cpu().tolist() == want["cluster"] and out[0][G:].eq(-5).all()
assert dv2.representatives.cpu().tolist() == want["representatives"] and out[1][dv2.n_clusters:].eq(-5).all()
assert torch.equal(dv2.edge_passed, dv.edge_passed) and torch.equal(dv2.edge_distance, dv.edge_distance)
genes3, dv3 = finder.find_verified_clusters_batch(seqs, spec, out=(out[0], None, None))
assert dv3.representatives is None and dv3.sizes is None and dv3.n_clusters == want["n_clusters"]
# against the clusters of the sketch stage alone
genes4, dc = finder.find_clusters_batch(seqs, spec.clusters)
assert torch.equal(dc.cluster, dv.candidates.cluster) and torch.equal(dc.edges, dv.candidates.edges) and dv.n_clusters > dc.n_clusters
print("find_verified_clusters_batch ok: %d genes, %d candidate edges, %d passed, %d -> %d clusters, the shortened copy lost %d of %d residues"
      % (G, len(edges), sum(passed), dc.n_clusters, dv.n_clusters, lost, len(rows[original])))
'''


def test_find_verified_clusters_batch_in_a_fresh_process(tmp_path):
    """torch is imported by the child alone (this process holds the library's HIP runtime and gets no second one); `out=` omitted
    allocates the tensors under torch's current stream.  The child says so when torch sees no GPU, and the test is skipped."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "torch_verified_clusters.py"
    script.write_text(FINDER_SCRIPT)
    done = subprocess.run([sys.executable, str(script), root], timeout=300, capture_output=True, text=True)
    assert done.returncode == 0, "child ended with %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    if "torch sees no GPU" in done.stdout:
        pytest.skip("torch sees no GPU")
    assert "find_verified_clusters_batch ok" in done.stdout
