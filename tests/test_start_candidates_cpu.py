"""Start candidates without a device: the plain-Python rule (tests/start_candidates_ref.py) on node arrays written by hand, and what
StartCandidates checks, hashes, pickles and hands to the library."""
import ctypes
import pickle

import numpy as np
import pytest

from tests.start_candidates_ref import FIELDS, candidates, row, start_candidates_ref

# One contig, nine nodes in ndx order.  Two forward ORFs end at stop_val 100 (nodes 0, 2, 4; its stop node 6) and at 70 (node 3);
# a reverse ORF has stop_val 100 as well (nodes 5, 7, 8, its stop node 1): reverse starts lie to the right of their stop.
NODES = {
    "ndx":      [10, 40, 46, 50, 61, 130, 100, 160, 190],
    "stop_val": [100, 40, 100, 70, 100, 100, 100, 100, 100],
    "type":     [0, 3, 1, 0, 2, 0, 3, 1, 0],
    "strand":   [1, -1, 1, 1, 1, -1, 1, -1, -1],
    "edge":     [1, 0, 0, 0, 0, 0, 0, 0, 1],
    "cscore":   [1.5, 0.0, 2.25, -3.0, 0.1, 7.0, 0.0, 8.0, 9.0],
    "sscore":   [0.5, 0.0, -1.0, 0.25, 0.2, 1.0, 0.0, 2.0, 3.0],
    "rscore":   [0.1, 0.0, 0.2, 0.3, 0.4, 0.5, 0.0, 0.6, 0.7],
    "uscore":   [1.0, 0.0, 2.0, 3.0, 4.0, 5.0, 0.0, 6.0, 7.0],
    "tscore":   [-1.0, 0.0, -2.0, -3.0, -4.0, -5.0, 0.0, -6.0, -7.0],
    "gc_cont":  np.array([0.5, 0.0, 0.25, 0.125, 0.75, 0.375, 0.0, 0.625, 0.875], np.float32),
}


def test_row_order_on_both_strands_by_hand():
    # forward: ascending ndx, the outermost (longest) ORF first
    assert candidates(NODES, 0) == ([0, 2, 4], 0) and candidates(NODES, 2) == ([0, 2, 4], 1) and candidates(NODES, 4) == ([0, 2, 4], 2)
    # reverse: descending ndx -- the start farthest from the stop reads first
    assert candidates(NODES, 5) == ([8, 7, 5], 2) and candidates(NODES, 7) == ([8, 7, 5], 1) and candidates(NODES, 8) == ([8, 7, 5], 0)
    # the same stop_val on the other strand, and another stop_val on the same strand, stay out; a row of one
    assert candidates(NODES, 3) == ([3], 0)
    with pytest.raises(AssertionError):
        candidates(NODES, 6)                                          # a stop node is no record


def test_values_by_hand():
    positions, types, scores, chosen = row(NODES, 2)
    assert positions == [11, 47, 62] and types == [3, 1, 2] and chosen == 1          # node 0 is an edge node: 3, whatever its type
    assert scores[0] == [2.0, 1.5, 0.5, 0.1, 1.0, -1.0, 0.5] and scores[1][:3] == [1.25, 2.25, -1.0]
    assert scores[2][0] == 0.1 + 0.2 and scores[2][0] != 0.3                          # added in double, as it is
    positions, types, scores, chosen = row(NODES, 7, ("gc_cont", "tscore"))
    assert positions == [191, 161, 131] and types == [3, 1, 0] and chosen == 1
    assert scores == [[0.875, -7.0], [0.625, -6.0], [0.375, -5.0]]


def test_layouts():
    records = [(0, 4), (0, 3), (0, 8)]
    pos, typ, sco, lens, chosen, ys = start_candidates_ref([NODES], records, ("total", "uscore"))
    assert lens.tolist() == [3, 1, 3] and chosen.tolist() == [2, 0, 0] and ys == [[0, 2, 4], [3], [8, 7, 5]]
    assert pos.tolist() == [11, 47, 62, 51, 191, 161, 131] and typ.tolist() == [3, 1, 2, 0, 3, 1, 0] and sco.shape == (7, 2)
    assert sco[3].tolist() == [-2.75, 3.0]
    pos, typ, sco, lens, _, _ = start_candidates_ref([NODES], records, ("total",), "padded", pad=-1, score_pad=np.nan, width=4,
                                                     index_dtype=np.int32, dtype=np.float32)
    assert pos.dtype == np.int32 and pos.tolist() == [[11, 47, 62, -1], [51, -1, -1, -1], [191, 161, 131, -1]]
    assert typ.tolist() == [[3, 1, 2, -1], [0, -1, -1, -1], [3, 1, 0, -1]] and sco.shape == (3, 4, 1) and sco.dtype == np.float32
    assert np.isnan(sco[1, 1:, 0]).all() and sco[0, 2, 0] == np.float32(0.1 + 0.2)   # one rounding of the double
    empty = start_candidates_ref([NODES], [], ("total",), "padded", pad=-1, score_pad=0.0)
    assert empty[0].shape == (0, 0) and empty[2].shape == (0, 0, 1)


def test_constructor_checks():
    from pyrodigal_amd import StartCandidates, _cabi
    s = StartCandidates()
    assert s.fields == FIELDS == _cabi.START_FIELDS and (s.dtype, s.index_dtype, s.layout) == ("float32", "int64", "ragged")
    assert StartCandidates("tscore").fields == ("tscore",) and StartCandidates(dtype=np.float64).dtype == "float64"
    for kw, word in ((dict(fields=()), "columns"), (dict(fields=FIELDS + ("total",)), "columns"), (dict(fields=("total", "mot_score")), "mot_score"),
                     (dict(fields=("cscore", "total", "cscore")), "twice"), (dict(dtype="float16"), "dtype"), (dict(dtype="int32"), "dtype"),
                     (dict(index_dtype="uint8"), "index_dtype"), (dict(index_dtype="float32"), "index_dtype"), (dict(layout="dense"), "layout"),
                     (dict(layout="padded"), "needs"), (dict(layout="padded", pad=0), "needs"), (dict(layout="padded", score_pad=0.0), "needs"),
                     (dict(layout="padded", pad=1 << 31, score_pad=0.0, index_dtype="int32"), "int32"),
                     (dict(layout="padded", pad=1 << 63, score_pad=0.0), "int64"),
                     (dict(layout="padded", pad=0, score_pad=1e39), "float32")):
        with pytest.raises(ValueError, match=word):
            StartCandidates(**kw)
    with pytest.raises(TypeError):
        StartCandidates(layout="padded", pad=0.5, score_pad=0.0)
    with pytest.raises(TypeError):
        StartCandidates(layout="padded", pad=0, score_pad="nan")
    StartCandidates(layout="padded", pad=(1 << 31) - 1, score_pad=1e39, index_dtype="int32", dtype="float64")     # both fit
    StartCandidates(layout="padded", pad=-1, score_pad=float("-inf"))


def test_hashing_and_pickling():
    from pyrodigal_amd import StartCandidates
    a = StartCandidates(("total", "tscore"), layout="padded", pad=-1, score_pad=float("nan"), index_dtype="int32")
    b = StartCandidates(["total", "tscore"], layout="padded", pad=-1, score_pad=float("nan"), index_dtype="int32")
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1          # NaN pads compare by their bits
    for other in (StartCandidates(("tscore", "total"), layout="padded", pad=-1, score_pad=float("nan"), index_dtype="int32"),
                  StartCandidates(("total", "tscore"), layout="padded", pad=-1, score_pad=0.0, index_dtype="int32"),
                  StartCandidates(("total", "tscore"), layout="padded", pad=-2, score_pad=float("nan"), index_dtype="int32"),
                  StartCandidates(("total", "tscore"), index_dtype="int32"), StartCandidates(("total", "tscore"), dtype="float64")):
        assert a != other
    c = pickle.loads(pickle.dumps(a))
    assert c == a and hash(c) == hash(a) and np.isnan(c.score_pad) and c.fields == a.fields and c.pad == -1
    assert a != "total" and "StartCandidates" in repr(a)


def test_opts():
    from pyrodigal_amd import StartCandidates, _cabi
    o = StartCandidates(("gc_cont", "total", "rscore"), dtype="float64", index_dtype="int32", layout="padded", pad=-7, score_pad=-1.5).opts(9, 12)
    assert (o.index_bytes, o.score_bytes, o.layout, o.n_fields, o.row_width, o.row_stride) == (4, 8, _cabi.TOKENS_PADDED, 3, 9, 12)
    assert list(o.fields)[:3] == [6, 0, 3] and o.index_pad == -7 and o.score_pad == -1.5
    o = StartCandidates().opts()
    assert (o.index_bytes, o.score_bytes, o.layout, o.n_fields, o.row_width, o.row_stride) == (8, 4, _cabi.TOKENS_RAGGED, 7, 0, 0)
    assert list(o.fields) == list(range(7))
    assert ctypes.sizeof(_cabi.StartOpts) == 80 and _cabi.StartOpts.index_pad.offset == 64 and _cabi.StartOpts.score_pad.offset == 72


def test_struct_matches_the_header(tmp_path):
    import os
    import subprocess
    from pyrodigal_amd import _cabi
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "sizes.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"pyrodigal_amd.h\"\nint main(void) { printf(\"%zu %zu %zu %zu %zu\\n\", "
                   "sizeof(pga_start_opts), offsetof(pga_start_opts, row_width), offsetof(pga_start_opts, fields), "
                   "offsetof(pga_start_opts, index_pad), offsetof(pga_start_opts, score_pad)); return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    S = _cabi.StartOpts
    assert got == [ctypes.sizeof(S), S.row_width.offset, S.fields.offset, S.index_pad.offset, S.score_pad.offset]


def test_find_starts_batch_refuses_circles_before_any_device_call():
    from pyrodigal_amd import StartCandidates, lib
    finder = lib.GeneFinder(meta=True)
    for kw in (dict(circular=True), dict(circular=[True, False]), dict(trim_terminal_repeats=True)):
        with pytest.raises(ValueError, match="not written for circular sequences"):
            finder.find_starts_batch([b"ACGT" * 100, b"ACGT" * 50], StartCandidates(), **kw)
    with pytest.raises(TypeError, match="StartCandidates"):
        finder.find_starts_batch([b"ACGT" * 100], "total")
