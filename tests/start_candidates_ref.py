"""The rule of pga_start_plan_create / pga_start_plan_write (include/pyrodigal_amd.h) restated in plain Python, from the header's text:
the candidates of a gene record, their order, and the values of every candidate.  `nodes` is one contig's node arrays as the
``want_nodes=1`` path reports them: a dict of sequences ndx, stop_val, type, strand, edge, cscore, sscore, rscore, uscore, tscore,
gc_cont.  A record is (contig, start_ndx, ...)."""
import numpy as np

FIELDS = ("total", "cscore", "sscore", "rscore", "uscore", "tscore", "gc_cont")
STOP = 3


def candidates(nodes, x):
    """The node indices of the candidates of start node x, in row order, and the index of x among them."""
    assert int(nodes["type"][x]) != STOP
    strand, stop_val = int(nodes["strand"][x]), int(nodes["stop_val"][x])
    same = [y for y in range(len(nodes["ndx"]))
            if int(nodes["type"][y]) != STOP and int(nodes["strand"][y]) == strand and int(nodes["stop_val"][y]) == stop_val]
    same.sort(key=lambda y: int(nodes["ndx"][y]), reverse=strand != 1)     # reading direction, outermost first
    return same, same.index(x)


def value(nodes, y, field):
    """One score column of candidate node y, as a Python float (a double)."""
    if field == "total":
        return float(nodes["cscore"][y]) + float(nodes["sscore"][y])       # added in double
    return float(nodes[field][y])                                          # (gc_cont is a float32: exact in a double)


def row(nodes, x, fields=FIELDS):
    """(positions, types, scores [n][F], chosen) of the record whose start node is x."""
    ys, chosen = candidates(nodes, x)
    positions = [int(nodes["ndx"][y]) + 1 for y in ys]
    types = [3 if int(nodes["edge"][y]) else int(nodes["type"][y]) & 3 for y in ys]
    scores = [[value(nodes, y, f) for f in fields] for y in ys]
    return positions, types, scores, chosen


def start_candidates_ref(nodes_of_contig, records, fields=FIELDS, layout="ragged", pad=0, score_pad=0.0, width=None, index_dtype=np.int64,
                         dtype=np.float64):
    """The three tensors of the rule ([T], [T], [T, F] ragged; [G, W], [G, W], [G, W, F] padded, W = `width` or the longest row), the
    candidates of every row and the chosen index of every row, and the node indices of every row.  float32 is the double rounded once."""
    rows = [row(nodes_of_contig[r[0]], r[1], fields) for r in records]
    ys = [candidates(nodes_of_contig[r[0]], r[1])[0] for r in records]
    lens = np.array([len(r[0]) for r in rows], np.int64)
    chosen = np.array([r[3] for r in rows], np.int64)
    F = len(fields)
    if layout == "ragged":
        pos = np.array([p for r in rows for p in r[0]], np.int64).astype(index_dtype)
        typ = np.array([t for r in rows for t in r[1]], np.int64).astype(index_dtype)
        sco = np.array([s for r in rows for s in r[2]], np.float64).reshape(-1, F).astype(dtype)
        return pos, typ, sco, lens, chosen, ys
    w = (int(lens.max()) if len(rows) else 0) if width is None else width
    pos = np.full((len(rows), w), pad, np.int64)
    typ = np.full((len(rows), w), pad, np.int64)
    sco = np.full((len(rows), w, F), score_pad, np.float64)
    for g, r in enumerate(rows):
        pos[g, :lens[g]], typ[g, :lens[g]] = r[0], r[1]
        sco[g, :lens[g]] = np.array(r[2], np.float64).reshape(-1, F)
    return pos.astype(index_dtype), typ.astype(index_dtype), sco.astype(dtype), lens, chosen, ys
