"""A plain restatement of the traceback tail over the oracle's node array (`Oracle.nodes()`), with counters: what the kernels of
pyrodigal_amd/csrc/tail.inl and the start tweaks of finder.hip have to compute, written from the rules and not from the kernels.
A helper module, not a test.

  ref: lib.pyx:1253-1311   (_disentangle_overlaps, _max_forward_pointers, the forward pointers)
       Prodigal dprog.c    eliminate_bad_genes (call sites lib.pyx:5308, 5369)
       lib.pyx:3231-3270   (Genes._extract)
       lib.pyx:3272-3401   (Genes._tweak_final_starts)

Everything walks the path node by node as the reference does; nothing here knows about prefix sums, running maxima or windows.
What it knows about the kernels is only how they COUNT: path positions `r` from the head of the path (r = 0) to the best gene
end, and gene indices from 0.  The counters say which populations an input holds, so that a test can assert that it reached
both sides of a rule (tests/test_tail_cpu.py) before the device is compared on it (tests/test_tail_shapes_gpu.py)."""
from collections import Counter

import numpy as np

from oracle import oracle as orc

T_STOP = 3
OPER_DIST = 60
EDGE_CLASSES = ("triple", "rb_fs", "fs_fs", "rs_rs")
UNITS = (64, 256, 1024)          # a wave, a round of k_tp_small / k_tp_extract, a round or a chunk of the genome forms


class Nodes:
    """The fields of a node array as Python lists (a walk over numpy scalars is ten times slower)."""

    def __init__(self, nd):
        self.n = len(nd)
        for k in ("ndx", "strand", "stop_val", "traceb", "tracef", "ov_mark", "elim", "edge", "cscore", "sscore", "rscore", "uscore", "tscore"):
            setattr(self, k, nd[k].tolist())
        self.stop = (nd["type"] == T_STOP).tolist()
        self.star_ptr = nd["star_ptr"].tolist()


# ---- path and splices ------------------------------------------------------------------------------------------------------------

def walk(traceb, mx):
    """The nodes from `mx` back to the head of the path."""
    out, p = [], mx
    while p != -1:
        out.append(p)
        p = traceb[p]
    return out


def untangle(N, mx):
    """Both untangling passes and the forward pointers over the raw traceb (the state after dprog_raw + find_max_index).

    Returns a dict: path (final, from mx to the head), raw_path, traceb / tracef / ov_mark (lists over all nodes), spliced (the set
    of nodes spliced in), edge_class ({position of p in raw_path: class} for the edge p -> raw traceb[p]), ipath (-1 if mx has no
    traceb, as dprog returns), counters."""
    tb, ov = list(N.traceb), list(N.ov_mark)
    tf = [-1] * N.n
    c = Counter()
    if mx < 0:
        return dict(path=[], raw_path=[], traceb=tb, tracef=tf, ov_mark=ov, spliced=set(), edge_class={}, ipath=-1, counters=c)
    raw = walk(tb, mx)
    pos = {p: k for k, p in enumerate(raw)}
    cls, spliced = {}, set()
    p = mx
    while tb[p] != -1:                       # first pass: triple overlaps
        nx = tb[p]
        if N.strand[p] == -1 and N.stop[p] and N.strand[nx] == 1 and N.stop[nx] and ov[p] != -1 and N.ndx[p] > N.ndx[nx]:
            tmp = N.star_ptr[p][ov[p]]
            k = tmp
            while N.ndx[k] != N.stop_val[tmp]:
                k -= 1
            c["triple_resets_a_mark"] += int(ov[k] != -1)                 # else the reset of the spliced-in stop's ov_mark is a no-op
            tb[p], tb[tmp], ov[k], tb[k] = tmp, k, -1, nx
            cls[pos[p]] = "triple"
            spliced.update((tmp, k))
        else:                                # what keeps an edge between a reverse and a forward stop from being one
            if N.strand[p] == -1 and N.stop[p] and N.strand[nx] == 1 and N.stop[nx]:
                if ov[p] == -1 and N.ndx[p] > N.ndx[nx]:
                    c["no_triple_for_the_mark_alone"] += 1                # only `ov_mark != -1` keeps this edge from a splice
                if ov[p] != -1 and N.ndx[p] <= N.ndx[nx]:
                    c["no_triple_for_the_position_alone"] += 1            # only `ndx[p] > ndx[nx]` does
                    c["triple_positions_equal"] += int(N.ndx[p] == N.ndx[nx])
        p = tb[p]
    p = mx
    while tb[p] != -1:                       # second pass: simple overlaps
        nx = tb[p]
        p_rb = N.strand[p] == -1 and not N.stop[p]
        p_fs = N.strand[p] == 1 and N.stop[p]
        p_rs = N.strand[p] == -1 and N.stop[p]
        n_fs = N.strand[nx] == 1 and N.stop[nx]
        n_rs = N.strand[nx] == -1 and N.stop[nx]
        ins, what = -1, None
        if p_rb and n_fs:
            k = p
            while N.ndx[k] != N.stop_val[p]:
                k -= 1
            ins, what = k, "rb_fs"
        if p_fs and n_fs:
            ins, what = N.star_ptr[nx][N.ndx[p] % 3], "fs_fs"
        if p_rs and n_rs:
            ins, what = N.star_ptr[p][N.ndx[nx] % 3], "rs_rs"
        if what is not None:
            assert p in pos and pos[p] not in cls and ins >= 0, (p, what, ins)     # a spliced-in node never triggers a splice
            tb[p] = ins
            tb[ins] = nx
            cls[pos[p]] = what
            spliced.add(ins)
            if N.ndx[p] % 3 != N.ndx[nx] % 3 and what != "rb_fs":
                c["frame_differs_" + what] += 1                                   # `np % 3` and `nn % 3` pick different starts
        p = tb[p]
    p = mx
    while tb[p] != -1:
        tf[tb[p]] = p
        p = tb[p]
    path = walk(tb, mx)
    for k, what in cls.items():
        c[what] += 1
        if k + 1 in cls:
            c["adjacent_splices"] += 1
        if k == 0:
            c["splice_first_edge"] += 1
        if k == len(raw) - 2:
            c["splice_head_edge"] += 1
    c["path"] = len(path)
    c["raw_path"] = len(raw)
    return dict(path=path, raw_path=raw, traceb=tb, tracef=tf, ov_mark=ov, spliced=spliced, edge_class=cls,
                ipath=(-1 if tb[mx] == -1 else mx), counters=c)


# ---- intergenic terms (ref: _connection.h:43-91) ------------------------------------------------------------------------------------

def igm_same(N, a, b, st_wt):
    dist = abs(N.ndx[a] - N.ndx[b])
    ovl = N.ndx[a] + 2 * N.strand[a] >= N.ndx[b]
    r = 0.0
    if N.ndx[a] + 2 == N.ndx[b] or N.ndx[a] == N.ndx[b] + 1:
        x = b if N.strand[a] == 1 else a
        if N.rscore[x] < 0:
            r -= N.rscore[x]
        if N.uscore[x] < 0:
            r -= N.uscore[x]
    if dist > 3 * OPER_DIST:
        r -= 0.15 * st_wt
    elif (dist <= OPER_DIST and not ovl) or dist * 4 < OPER_DIST:
        r += (2.0 - float(dist) / OPER_DIST) * 0.15 * st_wt
    return r


def igm(N, a, b, st_wt):
    return igm_same(N, a, b, st_wt) if N.strand[a] == N.strand[b] else -0.15 * st_wt


# ---- elimination ----------------------------------------------------------------------------------------------------------------------

def eliminate(N, U, st_wt):
    """eliminate_bad_genes over the untangled path `U`: returns (sscore, elim, counters); N.sscore / N.elim are left alone."""
    ss, el = list(N.sscore), list(N.elim)
    c = Counter()
    path = U["path"]
    if U["ipath"] == -1:
        return ss, el, c
    order = path[::-1]                                   # from the head
    got = Counter()
    for p, f in zip(order[:-1], order[1:]):
        if N.strand[p] == 1 and N.stop[p]:
            ss[f] += igm(N, p, f, st_wt)
            got[f] |= 1
        if N.strand[p] == -1 and not N.stop[p]:
            ss[p] += igm(N, p, f, st_wt)
            got[p] |= 2
    c["term_after_fwd_stop"] = sum(1 for v in got.values() if v == 1)
    c["term_rev_start"] = sum(1 for v in got.values() if v == 2)
    c["both_terms"] = sum(1 for v in got.values() if v == 3)
    for p, f in zip(order[:-1], order[1:]):
        hit = 0
        if N.strand[p] == 1 and not N.stop[p] and N.cscore[p] + ss[p] < 0:
            c["mark_fwd_start"] += 1
            hit = 1
        if N.strand[p] == -1 and N.stop[p] and N.cscore[f] + ss[f] < 0:
            c["mark_rev_stop"] += 1
            hit = 1
        if N.strand[p] == -1 and N.stop[p] and N.cscore[p] + ss[p] < 0 <= N.cscore[f] + ss[f]:
            c["rev_stop_own_score_negative"] += 1       # the rule reads the START's score (f), not the stop's (p)
        if hit:
            el[p] = el[f] = 1
            c["mark_on_spliced"] += int(p in U["spliced"]) + int(f in U["spliced"])
    c["eliminated"] = sum(1 for p in path if el[p] == 1)
    return ss, el, c


# ---- gene list ------------------------------------------------------------------------------------------------------------------------

def extract(N, U, el):
    """Genes._extract over the final path.  Returns (genes as a GENE_DTYPE array, setters, counters): setters[g] = the path positions
    r (0 = head) of the nodes that set gene g's begin, end, start node and stop node (-1: never set, the field is 0)."""
    genes, setters = [], []
    c = Counter()
    if U["ipath"] == -1:
        return np.zeros(0, orc.GENE_DTYPE), setters, c
    order = U["path"][::-1]
    b = e = s = t = 0
    rb = re = rs = rt = -1
    for r, p in enumerate(order):
        if el[p] == 1:
            continue
        if N.strand[p] == 1:
            if not N.stop[p]:
                b, s, rb, rs = N.ndx[p] + 1, p, r, r
            else:
                e, t, re, rt = N.ndx[p] + 3, p, r, r
                genes.append((b, e, s, t)); setters.append((rb, re, rs, rt))
        else:
            if not N.stop[p]:
                e, s, re, rs = N.ndx[p] + 1, p, r, r
                genes.append((b, e, s, t)); setters.append((rb, re, rs, rt))
            else:
                b, t, rb, rt = N.ndx[p] - 1, p, r, r
    for (rb, re, rs, rt) in setters:
        if min(rb, re, rs, rt) < 0:
            c["gene_with_unset_field"] += 1
            continue
        if abs(rs - rt) > 1:
            c["setter_not_adjacent"] += 1                   # an eliminated pair lies between a gene's two nodes
        for u in UNITS:
            if rs // u != rt // u:
                c["straddle_%d" % u] += 1
    for r in range(len(order) - 1):
        if el[order[r]] == 1 and el[order[r + 1]] == 1:
            for u in UNITS:
                if r // u != (r + 1) // u:
                    c["elim_pair_across_%d" % u] += 1
    c["genes"] = len(genes)
    c["path_parity"] = len(order) & 1
    out = np.zeros(len(genes), orc.GENE_DTYPE)
    for k, name in enumerate(("begin", "end", "start_ndx", "stop_ndx")):
        out[name] = [g[k] for g in genes]
    return out, setters, c


# ---- start tweaks ---------------------------------------------------------------------------------------------------------------------

def tweak_one(N, prev, cur, nxt, w, maxov, c=None):
    """One gene (begin, end, start_ndx, stop_ndx) against the given neighbours (tuples or None): the new record.  `c`: a Counter."""
    c = c if c is not None else Counter()
    ndx = cur[2]
    sc = N.sscore[ndx] + N.cscore[ndx]
    ig = 0.0
    prev_fwd = prev is not None and N.strand[prev[2]] == 1
    prev_rev = prev is not None and N.strand[prev[2]] == -1
    next_fwd = nxt is not None and N.strand[nxt[2]] == 1
    next_rev = nxt is not None and N.strand[nxt[2]] == -1
    if N.strand[ndx] == 1 and prev_fwd:
        ig = igm_same(N, prev[3], ndx, w)
    if N.strand[ndx] == 1 and prev_rev:
        ig = -0.15 * w
    if N.strand[ndx] == -1 and next_fwd:
        ig = -0.15 * w
    if N.strand[ndx] == -1 and next_rev:
        ig = igm_same(N, ndx, nxt[3], w)
    if ndx - 100 < 0:
        c["window_clipped_low"] += 1
    if ndx + 100 > N.n:
        c["window_clipped_high"] += 1
    mi, ms, mg = [-1, -1], [0.0, 0.0], [0.0, 0.0]
    for j in range(ndx - 100, ndx + 100):
        if j < 0 or j >= N.n or j == ndx:
            continue
        if N.stop[j] or N.stop_val[j] != N.stop_val[ndx]:
            continue
        tg = 0.0
        if N.strand[j] == 1 and prev_fwd:
            d = N.ndx[prev[3]] - N.ndx[j]
            if d == maxov:
                c["diff_equals_maxov"] += 1
            if d > maxov:
                c["cut_maxov_fwd"] += 1
                continue
            tg = igm_same(N, prev[3], j, w)
        if N.strand[j] == 1 and prev_rev:
            if N.ndx[prev[2]] - N.ndx[j] >= 0:
                c["cut_prev_rev_start"] += 1
                if N.ndx[prev[2]] - N.ndx[j] == 0:
                    c["cut_prev_rev_start_equal"] += 1
                continue
            tg = -0.15 * w
        if N.strand[j] == -1 and next_fwd:
            if N.ndx[j] - N.ndx[nxt[2]] >= 0:
                c["cut_next_fwd_start"] += 1
                if N.ndx[j] - N.ndx[nxt[2]] == 0:
                    c["cut_next_fwd_start_equal"] += 1
                continue
            tg = -0.15 * w
        if N.strand[j] == -1 and next_rev:
            d = N.ndx[j] - N.ndx[nxt[3]]
            if d == maxov:
                c["diff_equals_maxov"] += 1
            if d > maxov:
                c["cut_maxov_rev"] += 1
                continue
            tg = igm_same(N, j, nxt[3], w)
        cs = N.cscore[j] + N.sscore[j]
        if mi[0] == -1:
            mi[0], ms[0], mg[0] = j, cs, tg
        elif cs + tg > ms[0]:
            mi[1], ms[1], mg[1] = mi[0], ms[0], mg[0]
            mi[0], ms[0], mg[0] = j, cs, tg
        elif mi[1] == -1 or cs + tg > ms[1]:
            mi[1], ms[1], mg[1] = j, cs, tg
    if mi[1] != -1:
        c["second_best_filled"] += 1
    for k in range(2):
        m = mi[k]
        if m == -1:
            continue
        dist = abs(N.ndx[m] - N.ndx[ndx])
        if dist == 15:
            c["candidate_15_away"] += 1
        if (N.tscore[m] < N.tscore[ndx] and ms[k] - N.tscore[m] >= sc - N.tscore[ndx] + w and N.rscore[m] > N.rscore[ndx]
                and N.uscore[m] > N.uscore[ndx] and N.cscore[m] > N.cscore[ndx] and dist > 15):
            ms[k] += N.tscore[ndx] - N.tscore[m]
            c["far_%d" % k] += 1
        elif dist <= 15 and N.rscore[m] + N.tscore[m] > N.rscore[ndx] + N.tscore[ndx] and N.edge[ndx] == 0 and N.edge[m] == 0:
            if N.cscore[ndx] > N.cscore[m]:
                ms[k] += N.cscore[ndx] - N.cscore[m]
            if N.uscore[ndx] > N.uscore[m]:
                ms[k] += N.uscore[ndx] - N.uscore[m]
            if ig > mg[k]:
                ms[k] += ig - mg[k]
                c["near_ig_term"] += 1
            c["near_%d" % k] += 1
        else:
            ms[k] = -1000.0
            c["reject_%d" % k] += 1
    pick = -1
    for k in range(2):
        if mi[k] == -1:
            continue
        if pick == -1 and ms[k] + mg[k] > sc + ig:
            pick = k
        elif pick >= 0 and ms[k] + mg[k] > ms[pick] + mg[pick]:
            pick = k
    if pick == -1:
        return cur
    c["pick_%d" % pick] += 1
    m = mi[pick]
    if N.strand[m] == 1:
        c["move_fwd"] += 1
        return (N.ndx[m] + 1, cur[1], m, cur[3])
    c["move_rev"] += 1
    return (cur[0], N.ndx[m] + 1, m, cur[3])


def _as_array(recs):
    out = np.zeros(len(recs), orc.GENE_DTYPE)
    for k, name in enumerate(("begin", "end", "start_ndx", "stop_ndx")):
        out[name] = [g[k] for g in recs]
    return out


def tweak(N, genes, w, maxov):
    """The start tweaks of a gene list, two ways.  Returns (in_order, parallel, counters) as GENE_DTYPE arrays:
    in_order   every gene against its predecessor as already tweaked and its successor untouched -- the reference's loop;
    parallel   every gene against its ORIGINAL neighbours -- what k_tail_tweak* write before the fix-up.
    The rule counters are those of the in-order pass.  `differs`: the indices at which the two results differ; `redone`: the genes
    whose predecessor moved a reverse start, which the fix-up has to take again."""
    orig = [tuple(int(x) for x in g) for g in genes.tolist()]
    ng = len(orig)
    c = Counter()
    par = [tweak_one(N, orig[i - 1] if i > 0 else None, orig[i], orig[i + 1] if i < ng - 1 else None, w, maxov) for i in range(ng)]
    fin = []
    for i in range(ng):
        fin.append(tweak_one(N, fin[i - 1] if i > 0 else None, orig[i], orig[i + 1] if i < ng - 1 else None, w, maxov, c))
    moved = lambda rec, i: rec[2] != orig[i][2] and N.strand[rec[2]] == -1
    redone = [i for i in range(1, ng) if moved(fin[i - 1], i - 1)]
    differs = [i for i in range(ng) if fin[i] != par[i]]
    c["genes"] = ng
    c["redone"] = len(redone)
    c["differs"] = len(differs)
    c["redone_behind_63"] = sum(1 for i in redone if (i - 1) % 64 == 63)
    for i in differs:
        assert i in redone
        k = (i - 1) % 64                                  # the fix-up's windows hold genes 1 .. 64, 65 .. 128, ...
        c["differs_window_first" if k == 0 else "differs_window_last" if k == 63 else "differs_window_interior"] += 1
        if i >= 65:
            c["differs_past_first_window"] += 1
        if i + 1 < ng and (moved(fin[i], i) != moved(par[i], i) or (moved(fin[i], i) and fin[i][2] != par[i][2])):
            c["change_travels_on"] += 1                   # gene i + 1 now sees another predecessor than the parallel pass assumed
            if k == 63:
                c["change_travels_across_window"] += 1    # the only input on which phase 2 of the fix-up changes anything
    return _as_array(fin), _as_array(par), dict(counters=c, redone=redone, differs=differs)


# ---- the whole tail of one contig under one model, next to the oracle's staged calls ---------------------------------------------------

def staged_raw(seq, tinf, closed=False, is_meta=False, max_overlap=60, min_gene=90):
    """An oracle of `seq` after dprog_raw + find_max_index under `tinf`: (oracle, raw nodes, best gene end)."""
    o = orc.Oracle(seq)
    o.extract(tinf.trans_table, orc.Params(closed=closed, min_gene=min_gene))
    o.sort()
    o.reset_scores()
    o.score_nodes(tinf, closed, is_meta)
    o.overlapping_starts(tinf, 1, max_overlap)
    o.dprog_raw(tinf, True)
    mx = o.find_max_index() if o.num_nodes else -1
    return o, o.nodes(), mx


def run(seq, tinf, closed=False, is_meta=False, max_overlap=60, with_tweak=True, check=True, min_gene=90):
    """The tail of `seq` under `tinf` by this module; with `check`, every stage is compared with the oracle's staged call of the same
    name (dprog, eliminate_bad_genes, extract_genes, tweak_final_starts).  Returns a dict of the stages' results and counters."""
    o, raw, mx = staged_raw(seq, tinf, closed, is_meta, max_overlap, min_gene)
    N = Nodes(raw)
    U = untangle(N, mx)
    ss, el, ce = eliminate(N, U, tinf.st_wt)
    N.sscore, N.elim = ss, el
    genes, setters, cg = extract(N, U, el)
    out = dict(N=N, U=U, sscore=ss, elim=el, genes=genes, setters=setters, n_nodes=N.n,
               counters=dict(untangle=U["counters"], eliminate=ce, extract=cg))
    if check:
        ipath = o.dprog(tinf, True)
        assert ipath == U["ipath"], (ipath, U["ipath"])
        on = o.nodes()
        for k in ("traceb", "tracef", "ov_mark"):
            assert on[k].tolist() == U[k], k
        if N.n:
            o.eliminate_bad_genes(ipath, tinf)
        on = o.nodes()
        assert on["elim"].tolist() == el
        assert np.array_equal(on["sscore"].view(np.uint64), np.array(ss, np.float64).view(np.uint64))
        o.extract_genes(ipath)
        assert o.genes().tobytes() == genes.tobytes()
    if with_tweak:
        fin, par, tw = tweak(N, genes, tinf.st_wt, max_overlap)
        out.update(final=fin, parallel=par, redone=tw["redone"], differs=tw["differs"])
        out["counters"]["tweak"] = tw["counters"]
        if check:
            o.tweak_final_starts(tinf, max_overlap)
            assert o.genes().tobytes() == fin.tobytes()
    return out


def total(results, stage):
    """The sum of a stage's counters over several results of `run`."""
    c = Counter()
    for r in results:
        c.update(r["counters"].get(stage, {}))
    return c
