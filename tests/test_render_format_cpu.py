"""The number formatting of the device renderer (pyrodigal_amd/csrc/render_fmt.h), built host-only through
tests/render_fmt_shim.cpp and compared with CPython's '%.Nf' -- what the host writers (Genes.write_*) print."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "render_fmt_shim.cpp")
HDR = os.path.join(os.path.dirname(HERE), "pyrodigal_amd", "csrc", "render_fmt.h")
LIB = os.path.join(HERE, "librender_fmt_shim.so")


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC], check=True)
    L = ctypes.CDLL(LIB)
    L.render_fmt_many.restype = ctypes.c_int64
    L.render_fmt_many.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.render_near_midpoint.restype = ctypes.c_int
    L.render_near_midpoint.argtypes = [ctypes.c_double, ctypes.c_int, ctypes.c_double]
    return L


def fmt(L, xs, nd):
    x = np.ascontiguousarray(xs, np.float64)
    out = np.zeros(32 * max(len(x), 1), np.uint8)
    ok = np.zeros(max(len(x), 1), np.uint8)
    n = L.render_fmt_many(x.ctypes.data, len(x), nd, out.ctypes.data, ok.ctypes.data)
    return out[:n].tobytes().decode("ascii").split("\n")[:-1], ok[:len(x)].astype(bool)


def check(L, xs, nd):
    got, ok = fmt(L, xs, nd)
    assert ok.all()
    want = [("%%.%df" % nd) % v for v in xs]
    bad = [(float(v), g, w) for v, g, w in zip(xs, got, want) if g != w]
    assert not bad, bad[:10]


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_exact_halves_and_neighbours(shim, nd):
    halves = [0.125, 2.675, 1.005, 0.0005, 0.5, 1.5, 2.5, 0.25, 0.75, 0.05, 0.15, 0.35, 99.995, 99.985, 12.345, 1e-3, 5e-4]
    xs = []
    for h in halves:
        for v in (h, -h):
            xs += [v, math.nextafter(v, math.inf), math.nextafter(v, -math.inf)]
    check(shim, xs, nd)


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_signed_zero_results(shim, nd):
    xs = [0.0, -0.0, -1e-300, -5e-324, -0.04, -0.004, -0.0004, -0.049999, -0.0049999, -0.00049999, -0.05, -0.005, -0.0005,
          5e-324, 1e-300, 2.2250738585072014e-308, -2.2250738585072014e-308]
    check(shim, xs, nd)
    got, _ = fmt(shim, [-0.0, -0.0004], nd)
    assert got == ["-" + "0." + "0" * nd] * 2


@pytest.mark.parametrize("nd", [1, 2, 3])
def test_random_doubles(shim, nd):
    rng = np.random.default_rng(1000 + nd)
    n = 1_000_000
    mant = rng.random(n) + 1.0
    ex = rng.integers(-30, 21, n)
    xs = np.ldexp(mant, ex) * np.where(rng.random(n) < 0.5, -1.0, 1.0)
    check(shim, xs.tolist(), nd)


def test_float32_grid_widened(shim):
    # gc_cont is a float32 widened to double, as the host does: every float32 in [0, 1] on a fine grid, and their neighbours
    grid = np.linspace(0, 1, 200_001, dtype=np.float32)
    up = np.nextafter(grid, np.float32(2))
    dn = np.nextafter(grid, np.float32(-1))
    xs = np.unique(np.concatenate([grid, up, dn])).astype(np.float64)
    xs = xs[(xs >= 0) & (xs <= 1)]
    check(shim, xs.tolist(), 3)


def test_values_outside_the_exact_path_are_flagged(shim):
    _, ok = fmt(shim, [math.inf, -math.inf, math.nan, 2.0 ** 53, -(2.0 ** 60), 2.0 ** 53 - 1], 2)
    assert ok.tolist() == [False, False, False, False, False, True]


def test_midpoint_margin(shim):
    assert shim.render_near_midpoint(99.985, 2, 1e-9)
    assert shim.render_near_midpoint(73.125, 2, 1e-9)
    assert not shim.render_near_midpoint(73.12, 2, 1e-9)
    assert not shim.render_near_midpoint(50.0, 2, 1e-9)
    assert shim.render_near_midpoint(math.nan, 2, 1e-9)
