"""The host arithmetic of a finder call (pyrodigal_amd/csrc/find_plan.h), built host-only through tests/find_plan_shim.cpp and
compared with a short restatement of the reference's rules: dense set ids, the (contig, model) chains of the GC windows, the
winning chain per contig, who is re-scored, the layout of the gathered winners."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "find_plan_shim.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "pyrodigal_amd", "csrc")
HDRS = [os.path.join(CSRC, "find_plan.h"), os.path.join(CSRC, "find_pods.h")]
LIB = os.path.join(HERE, "libfind_plan_shim.so")
NAN = float("nan")


@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-o", LIB, SRC], check=True)
    L = ctypes.CDLL(LIB)
    for name in ("find_plan_chains", "find_plan_rescore", "find_plan_gather"):
        getattr(L, name).restype = ctypes.c_int64
    return L


def ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def i32(x):
    return None if x is None else np.ascontiguousarray(x, np.int32)


def i64(x):
    return np.ascontiguousarray(x, np.int64)


# ---- the restatement --------------------------------------------------------------------------------------------------
def window(gc):
    return min(0.65, 0.88495 * gc - 0.0102337), max(0.35, 0.86596 * gc + 0.1131991)


def ref_chains(lens, cnt, cbase, sbase, model_gc, model_tt, model_group, NG, meta, moc=None, cgrp=None, set_of=None):
    """chains as (off, topo_off, n, model, contig, first, group, soff), group-major, (contig, model) order within a group"""
    NC = len(lens)
    gc = [cnt[i] / lens[i] if lens[i] > 0 else 0.0 for i in range(NC)]
    if set_of is not None:
        pooled = {}
        for i in range(NC):
            a, b = pooled.get(set_of[i], (0, 0))
            pooled[set_of[i]] = (a + cnt[i], b + lens[i])
        gc = [pooled[set_of[i]][0] / pooled[set_of[i]][1] if pooled[set_of[i]][1] > 0 else 0.0 for i in range(NC)]
    per_group = [[] for _ in range(NG)]
    for i in range(NC):
        if not meta:
            g = cgrp[i] if cgrp is not None else 0
            per_group[g].append((i, moc[i] if moc is not None else 0, 1))
            continue
        low, high = window(gc[i])
        prev = -1
        for m in range(len(model_gc)):
            if low <= model_gc[m] <= high:
                per_group[model_group[m]].append((i, m, 1 if model_tt[m] != prev else 0))
                prev = model_tt[m]
    out, off, soff = [], 0, 0
    for g in range(NG):
        for i, m, first in per_group[g]:
            n = cbase[g][i + 1] - cbase[g][i]
            out.append((off, cbase[g][i], n, m, i, first, g, soff))
            off += n
            soff += sbase[g][i + 1] - sbase[g][i]
    return out


def ref_winners(NC, NM, meta, chains, score, ipath, set_of=None):
    win = [-1] * NC
    if not meta:
        for k in reversed(range(len(chains))):
            win[chains[k][4]] = k
        return win, None
    ok = [k for k, ch in enumerate(chains) if ch[2] > 0 and ipath[k] >= 0]
    if set_of is None:
        for i in range(NC):
            best = -100.0
            for k in sorted((k for k in ok if chains[k][4] == i), key=lambda k: chains[k][3]):      # model order, strictly better
                if score[k] > best:
                    best, win[i] = score[k], k
        return win, None
    choice = {}
    for s in sorted(set(set_of)):
        best, w = -100.0, -1
        for m in range(NM):
            terms = [score[k] for i in range(NC) if set_of[i] == s for k in ok if chains[k][4] == i and chains[k][3] == m]
            if terms and sum_in_order(terms) > best:
                best, w = sum_in_order(terms), m
        choice[s] = (w, best)
    for i in range(NC):
        w = choice[set_of[i]][0]
        for k in ok:
            if w >= 0 and chains[k][4] == i and chains[k][3] == w:
                win[i] = k
    return win, choice


def sum_in_order(terms):
    s = terms[0]
    for v in terms[1:]:
        s += v
    return s


# ---- calling the shim --------------------------------------------------------------------------------------------------
def run_chains(L, lens, cnt, cbase, sbase, enabled, model_gc, model_tt, model_group, NG, meta, moc=None, cgrp=None, set_of=None, NS=0):
    NC, NM = len(lens), len(model_gc)
    cap = NC * max(NM, 1) + 1
    rows = np.zeros((cap, 8), np.int64)
    c0, n0, s0, tot = np.zeros(NG + 1, np.int64), np.zeros(NG + 1, np.int64), np.zeros(NG + 1, np.int64), np.zeros(2, np.int64)
    a = [i32(lens), i32(cnt), i32(np.asarray(cbase).ravel()), i32(np.asarray(sbase).ravel()), np.ascontiguousarray(np.asarray(enabled).ravel(), np.uint8),
         np.ascontiguousarray(model_gc, np.float64), i32(model_tt), i32(model_group), i32(moc), i32(cgrp), i32(set_of)]
    n = L.find_plan_chains(NC, NM, NG, int(meta), *[ptr(x) for x in a], NS, ptr(rows), ctypes.c_int64(cap), ptr(c0), ptr(n0), ptr(s0), ptr(tot))
    return n, [tuple(int(v) for v in r) for r in rows[:max(n, 0)]], c0, n0, s0, tot


def run_winners(L, NC, NM, meta, chains, score, ipath, set_of=None, NS=0):
    rows = i64(np.asarray(chains, np.int64).reshape(-1, 8))
    ms = np.full((NC, max(NM, 1)), NAN)
    sm, ss, win = np.full(NC, -1, np.int32), np.full(NC, NAN), np.zeros(NC, np.int32)
    sc, ip = np.ascontiguousarray(score, np.float64), i32(ipath)
    L.find_plan_winners(NC, NM, int(meta), ptr(rows), len(chains), ptr(sc), ptr(ip), ptr(i32(set_of)), NS, ptr(ms), ptr(sm), ptr(ss), ptr(win))
    return [int(w) for w in win], ms, sm, ss


# three contigs (the middle one empty), three models: tables 11, 4, 11 in groups 0, 1, 0
LENS, CNT = [1000, 0, 1000], [500, 0, 850]
CBASE, SBASE = [[0, 10, 10, 14], [0, 6, 6, 9]], [[0, 4, 4, 6], [0, 2, 2, 3]]
TT, GRP = [11, 4, 11], [0, 1, 0]
ALL_ON = [[1, 1, 1], [1, 1, 1]]


def test_dense_set_ids(shim):
    lab = i32([7, -1, 7, 3, -1, 3, 0])
    out = np.zeros(len(lab), np.int32)
    assert shim.find_plan_dense_sets(ptr(lab), len(lab), ptr(out)) == 5      # an unlabelled contig is a set of its own
    assert out.tolist() == [0, 1, 0, 2, 3, 2, 4]
    assert shim.find_plan_dense_sets(None, 0, None) == 0


def test_window_ends_are_inclusive(shim):
    low, high = window(0.5)
    eps = 1e-12
    for mgc, want in (([low, high, 0.3], [0, 1]), ([low - eps, high + eps, 0.3], [])):
        n, rows, *_ = run_chains(shim, LENS, CNT, CBASE, SBASE, ALL_ON, mgc, TT, GRP, 2, True)
        assert sorted(r[3] for r in rows if r[4] == 0) == want
        assert rows == ref_chains(LENS, CNT, CBASE, SBASE, mgc, TT, GRP, 2, True)


def test_empty_contig_and_no_model_in_window(shim):
    # a contig of length 0 has gc 0: the window is [-0.0102337, 0.35]; contig 2 (gc 0.85) finds no model in [0.65, 0.849...]
    mgc = [0.45, 0.2, 0.9]
    n, rows, c0, n0, s0, tot = run_chains(shim, LENS, CNT, CBASE, SBASE, ALL_ON, mgc, TT, GRP, 2, True)
    assert rows == ref_chains(LENS, CNT, CBASE, SBASE, mgc, TT, GRP, 2, True)
    assert [(r[4], r[3]) for r in rows] == [(0, 0), (1, 1)] and rows[1][2] == 0            # the empty contig's chain has no nodes
    assert c0.tolist() == [0, 1, 2] and n0.tolist() == [0, 10, 10] and s0.tolist() == [0, 4, 4] and tot.tolist() == [10, 4]
    n, rows, *_ = run_chains(shim, LENS, CNT, CBASE, SBASE, ALL_ON, [0.9, 0.95, 0.99], TT, GRP, 2, True)
    assert n == 0 and rows == []


def test_first_flag_follows_the_table(shim):
    # models in one window with tables 11, 11, 4, 11: a change of table starts a fresh extraction
    mgc, tt, grp = [0.5, 0.5, 0.5, 0.5], [11, 11, 4, 11], [0, 0, 1, 0]
    n, rows, *_ = run_chains(shim, [1000], [500], [[0, 8], [0, 5]], [[0, 3], [0, 2]], [[1], [1]], mgc, tt, grp, 2, True)
    assert rows == ref_chains([1000], [500], [[0, 8], [0, 5]], [[0, 3], [0, 2]], mgc, tt, grp, 2, True)
    assert {r[3]: r[5] for r in rows} == {0: 1, 1: 0, 2: 1, 3: 1}
    assert [r[0] for r in rows] == [0, 8, 16, 24] and [r[7] for r in rows] == [0, 3, 6, 9]      # group-major offsets


def test_host_and_device_disagree(shim):
    n, *_ = run_chains(shim, LENS, CNT, CBASE, SBASE, [[0, 1, 1], [1, 1, 1]], [0.45, 0.2, 0.9], TT, GRP, 2, True)
    assert n == -1


def test_single_mode_chains(shim):
    n, rows, *_ = run_chains(shim, LENS, CNT, CBASE, SBASE, ALL_ON, [0.5, 0.5, 0.5], TT, GRP, 2, False, moc=[1, 0, 2], cgrp=[1, 0, 0])
    assert rows == ref_chains(LENS, CNT, CBASE, SBASE, [0.5, 0.5, 0.5], TT, GRP, 2, False, moc=[1, 0, 2], cgrp=[1, 0, 0])
    assert [(r[4], r[3], r[5], r[6]) for r in rows] == [(1, 0, 1, 0), (2, 2, 1, 0), (0, 1, 1, 1)]
    n, rows, *_ = run_chains(shim, LENS, CNT, [CBASE[0]], [SBASE[0]], [[1, 1, 1]], [0.5], [11], [0], 1, False)
    assert [(r[4], r[3], r[6]) for r in rows] == [(0, 0, 0), (1, 0, 0), (2, 0, 0)]


def test_set_pooled_gc(shim):
    # contigs 0 and 2 pool to (500 + 850) / 2000 = 0.675, window [0.587.., 0.697..]: alone, contig 0 would take model 0
    mgc, set_of = [0.45, 0.2, 0.69], [0, 1, 0]
    n, rows, *_ = run_chains(shim, LENS, CNT, CBASE, SBASE, ALL_ON, mgc, TT, GRP, 2, True, set_of=set_of, NS=2)
    assert rows == ref_chains(LENS, CNT, CBASE, SBASE, mgc, TT, GRP, 2, True, set_of=set_of)
    assert [(r[4], r[3]) for r in rows] == [(0, 2), (2, 2), (1, 1)]


def chain(contig, model, group=0, n=5, off=0, first=1):
    return (off, 0, n, model, contig, first, group, 0)


def test_single_mode_takes_the_first_chain(shim):
    chains = [chain(1, 0), chain(0, 0), chain(1, 3)]
    win, *_ = run_winners(shim, 3, 4, False, chains, [-500.0, NAN, 9.0], [-1, -1, 4])
    assert win == [1, 0, -1] == ref_winners(3, 4, False, chains, None, None)[0]


def test_meta_winner_rules(shim):
    # contig 0: equal best scores in different groups -> the lower model; contig 1: exactly -100 loses; contig 2: the better chain has
    # no path (ipath < 0), the other one no nodes; contig 3: a later, strictly better model
    chains = [chain(0, 2, 0), chain(1, 0, 0), chain(2, 0, 0), chain(3, 0, 0), chain(0, 1, 1), chain(2, 1, 1, n=0), chain(3, 1, 1)]
    score = [7.5, -100.0, 50.0, 1.0, 7.5, 60.0, 1.0000001]
    ipath = [0, 0, -1, 2, 3, 1, 0]
    win, *_ = run_winners(shim, 4, 3, True, chains, score, ipath)
    assert win == [4, -1, -1, 6] == ref_winners(4, 3, True, chains, score, ipath)[0]
    # just above -100 wins
    assert run_winners(shim, 1, 1, True, [chain(0, 0)], [math.nextafter(-100.0, 0.0)], [0])[0] == [0]


def test_set_winners(shim):
    # set 0 = contigs 0, 1, 3; set 1 = contig 2 alone.  Under model 0 only contig 0 contributes (contig 1 has no path there), under
    # model 1 contigs 0 and 1, under model 2 contig 3 alone: S = [4, 3 + 2.5, 5.5] -> the lower of the equal models, 1
    chains = [chain(0, 0), chain(0, 1), chain(1, 0), chain(1, 1), chain(3, 2), chain(2, 0), chain(3, 0, n=0)]
    score = [4.0, 3.0, 99.0, 2.5, 5.5, -100.0, 1000.0]
    ipath = [0, 0, -1, 0, 0, 0, 0]
    set_of = [0, 0, 1, 0]
    win, ms, sm, ss = run_winners(shim, 4, 3, True, chains, score, ipath, set_of=set_of, NS=2)
    ref, choice = ref_winners(4, 3, True, chains, score, ipath, set_of=set_of)
    assert win == ref == [1, 3, -1, -1]                 # contig 3 did not contribute under the set's model: no genes; set 1: -100 loses
    assert choice[0] == (1, 5.5) and choice[1][0] == -1
    assert sm.tolist() == [1, 1, -1, 1] and ss[[0, 1, 3]].tolist() == [5.5, 5.5, 5.5] and math.isnan(ss[2])
    want = np.full((4, 3), NAN)
    want[0, 0], want[0, 1], want[1, 1], want[3, 2], want[2, 0] = 4.0, 3.0, 2.5, 5.5, -100.0
    assert np.array_equal(ms, want, equal_nan=True)     # only contributions are reported


def run_rescore(L, NC, NG, meta, chains, win, conv, grp, tot):
    rows = i64(np.asarray(chains, np.int64).reshape(-1, 8))
    rs = np.zeros((NC + 1, 4), np.int64)
    c0, n0, fin = np.zeros(NG + 1, np.int64), np.zeros(NG + 1, np.int64), np.zeros(NC, np.int64)
    cv = np.ascontiguousarray(np.asarray(conv).ravel(), np.uint8)
    n = L.find_plan_rescore(NC, NG, int(meta), ptr(rows), len(chains), ptr(i32(win)), ptr(cv), ptr(i32(grp)), len(grp), ctypes.c_int64(tot), ptr(rs), ptr(c0), ptr(n0), ptr(fin))
    return [tuple(int(v) for v in r) for r in rs[:n]], c0.tolist(), n0.tolist(), fin.tolist()


def test_rescore_rule_and_gather_layout(shim):
    # models 0, 2 in group 0, model 1 in group 1.  Winners: contig 0 a `first` chain (stands), contig 1 a later chain on a contig whose
    # conv flag is clear (stands), contig 2 a later chain with the flag set in ITS group (fresh pass), contig 3 none, contig 4 a later
    # chain of group 1 with the flag set (fresh pass, behind group 0's)
    grp = [0, 1, 0]
    chains = [chain(0, 0, 0, 5, 0), chain(1, 2, 0, 6, 5, first=0), chain(2, 2, 0, 7, 11, first=0), chain(4, 1, 1, 3, 18, first=0), chain(2, 1, 1, 2, 21)]
    win = [0, 1, 2, -1, 3]
    conv = [[0, 0, 1, 0, 0], [0, 1, 0, 0, 1]]       # (contig 1's flag is set in group 1 only: not its winner's group)
    rs, c0, n0, fin = run_rescore(shim, 5, 2, True, chains, win, conv, grp, 23)
    assert rs == [(23, 11, 2, 2), (30, 18, 4, 1)] and c0 == [0, 1, 2] and n0 == [23, 30, 33]
    assert fin == [0, 5, 23, -1, 30]
    # single mode never re-scores
    rs1, _, _, fin1 = run_rescore(shim, 5, 2, False, chains, win, conv, grp, 23)
    assert rs1 == [] and fin1 == [0, 5, 11, -1, 18]
    # the gathered winners: group-major, then contig
    rows = i64(np.asarray(chains, np.int64).reshape(-1, 8))
    wr, oo, wo = np.zeros((5, 6), np.int64), np.zeros(5, np.int64), np.zeros(3, np.int64)
    total = shim.find_plan_gather(5, 2, ptr(rows), len(chains), ptr(i32(win)), ptr(i64(fin)), ptr(wr), ptr(oo), ptr(wo))
    assert total == 21 and wo.tolist() == [0, 18, 21] and oo.tolist() == [0, 5, 11, 0, 18]
    assert wr[:4].tolist() == [[0, 0, 0, 0, 0, 5], [0, 5, 5, 5, 0, 6], [0, 11, 11, 23, 0, 7], [1, 18, 18, 30, 0, 3]]
