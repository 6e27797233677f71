"""Connection scoring on score arrays that tie: the caller's own cscore / sscore / rscore / uscore over a real node topology.

Scores that the scoring stage computes from a sequence never tie (the oracle counts 0 ties and 0 zero-joins on them), so the
tie rules of the reference -- candidate sources scanned in ascending order and joined with `>=` against a target that starts
at 0.0 (ref: _connection.h:135/197 and siblings: the later source wins, a sum of exactly 0.0 still connects), the frame of a
triple overlap chosen with a strict `>` against 0.0, the best gene end the largest index among equals (ref: lib.pyx:1239-1251)
-- are only decided on injected arrays.  `pga_score_connections` takes such arrays as they are, so they are legal input.

The oracle extracts and sorts the nodes of a sequence, the four score arrays are overwritten with values of one family,
`overlapping_starts(flag = 1)` makes star_ptr consistent with them, and `dprog_raw` gives the expected score / traceb / ov_mark.
`Oracle.dp_events()` then tells how often each rule was decided, so that a test can assert that it checked what it set out to.
"""
import numpy as np

from oracle import oracle as orc
from tests.util import synthetic_contig

FAMILIES = ("zero", "pm1", "quant", "mag")
SCORE_FIELDS = ("cscore", "sscore", "rscore", "uscore")          # the order in which the arrays are drawn


def draw(family, rng, n):
    """One array of `n` finite scores of a family."""
    if family == "zero":
        return np.zeros(n)
    if family == "pm1":
        return rng.choice([-1.0, 1.0], n)
    if family == "quant":
        return rng.integers(-8, 13, n) * 0.25
    if family == "mag":
        # magnitudes from 1e-12 to 1e8: small terms vanish in large sums (ties by absorption), and a sum taken in another order rounds
        # to another double
        return rng.standard_normal(n) * 10.0 ** rng.integers(-12, 9, n)
    raise ValueError(family)


def blank_training(st_wt, tt=11):
    t = orc.Training()
    t.set_trans_table(tt)
    t._f64(16)[0] = st_wt
    return t


def extracted(seq, closed=False, tt=11):
    """The oracle of a sequence with its nodes extracted and sorted (scores all zero)."""
    o = orc.Oracle(seq)
    o.extract(tt, orc.Params(closed=closed))
    o.sort()
    return o


def inject_into(o, family, st_wt, seed, tt=11, star_flag=1):
    """`inject` on an oracle whose nodes are extracted and sorted already; may be repeated on the same oracle."""
    o.reset_scores()
    t = blank_training(st_wt, tt)
    live = o.nodes(copy=False)
    rng = np.random.default_rng(seed)
    for f in SCORE_FIELDS:
        live[f] = draw(family, rng, len(live))
    assert all(np.isfinite(live[f]).all() for f in SCORE_FIELDS)
    o.overlapping_starts(t, star_flag, 60)
    events = o.dp_events()                        # ovl_ties belongs to this call
    before = o.nodes()
    o.dprog_raw(t, True)
    ref = o.nodes()
    ref_max = o.find_max_index()
    events.update({k: v for k, v in o.dp_events().items() if k != "ovl_ties"})
    return before, ref, ref_max, events


def inject(seq, family, st_wt, seed, closed=False, tt=11, star_flag=1):
    """Nodes of `seq` with injected scores before the connection scoring, after it, the best gene end and the event counters.

    star_flag = 1 leaves in star_ptr what the gene prediction pass has there: per stop node the overlapping starts that beat,
    strictly, every candidate before them.  The frames of one stop node then never have equal values, so the frame of a triple
    overlap is never decided by a tie (frame_ties stays 0 whatever the scores).  star_flag = 0 leaves the first candidate of every
    frame, whatever its score, as the training pass does; a caller of the scorer may pass such an array, and with it frames tie."""
    return inject_into(extracted(seq, closed, tt), family, st_wt, seed, tt, star_flag)


def node_index(nodes, kind, ndx):
    """Index of the node of a kind ("fb" / "fs" / "rb" / "rs": strand and start / stop) at a position; exactly one must exist."""
    strand, is_stop = (1 if kind[0] == "f" else -1), kind[1] == "s"
    hit = np.flatnonzero((nodes["ndx"] == ndx) & (nodes["strand"] == strand) & ((nodes["type"] == 3) == is_stop))
    assert len(hit) == 1, (kind, ndx, hit)
    return int(hit[0])


def inject_assigned(o, named, default, st_wt, max_overlap=60, tt=11, final=True, reverse=False):
    """`inject_into` with a designed assignment instead of a family: `named` = [(kind, ndx, {field: value})] for the nodes a design
    names, `default` = {"start": {field: value}, "stop": {...}} for every other node.  Returns (before, ref, ref_max, events, edges); `final = False`
    runs the training pass on gc_score = (|cscore| / 16, |sscore|, 0.25) of the same assignment under the bias (1, 1, 1): every frame score
    is positive, so genes connect."""
    o.reset_scores()
    t = blank_training(st_wt, tt)
    live = o.nodes(copy=False)
    is_stop = live["type"] == 3
    for f in SCORE_FIELDS:
        live[f] = np.where(is_stop, default["stop"][f], default["start"][f])
    for kind, ndx, values in named:
        k = node_index(live, kind, ndx)
        for f, v in values.items():
            live[f][k] = v
    if not final:
        t.bias[:] = (1.0, 1.0, 1.0)
        live["gc_score"] = np.stack([np.abs(live["cscore"]) / 16, np.abs(live["sscore"]), np.full(len(live), 0.25)], axis=1)
    o.overlapping_starts(t, 1 if final else 0, max_overlap)
    events, edges = o.dp_events(), o.dp_edges()
    before = o.nodes()
    o.dprog_raw(t, final)
    ref = o.nodes()
    ref_max = o.find_max_index()
    events.update({k: v for k, v in o.dp_events().items() if k != "ovl_ties"})
    for k, v in o.dp_edges().items():              # the scoring pass clears its own counters, not those of overlapping_starts
        if k.startswith("igm_"):                   # igm_same is priced in both passes
            edges[k] = tuple(a + b for a, b in zip(edges[k], v))
        elif not k.startswith("ovl_"):
            edges[k] = v
    return before, ref, ref_max, events, edges


def inject_training(seq, family, bias, seed, closed=False, st_wt=4.35, tt=11):
    """The training pass (final = 0): gc_score drawn from `family` (pm1 or quant), the frame bias set to `bias`, star_ptr as
    `overlapping_starts(flag = 0)` leaves it.  Returns (before, ref, ref_max, events); ref is the state after `dprog_raw(t, False)`."""
    assert family in ("pm1", "quant")
    o = extracted(seq, closed, tt)
    o.reset_scores()
    t = blank_training(st_wt, tt)
    t.bias[:] = bias
    live = o.nodes(copy=False)
    rng = np.random.default_rng(seed)
    live["gc_score"] = draw(family, rng, 3 * len(live)).reshape(-1, 3)
    o.overlapping_starts(t, 0, 60)
    before = o.nodes()
    o.dprog_raw(t, False)
    ref = o.nodes()
    ref_max = o.find_max_index()
    return before, ref, ref_max, o.dp_events()


def contig_with_nodes(n, gc, seed):
    """A synthetic contig, trimmed from the right until the oracle extracts exactly `n` nodes from it (open ends, table 11)."""
    length = 64
    while True:                                   # long enough to hold more than n nodes
        seq = synthetic_contig(length, gc, seed)
        if extracted(seq).num_nodes > n + 8 or length > (n + 64) * 4096:
            break
        length *= 2
    found = trimmed_to_nodes(seq, n)
    assert found is not None, (n, gc, seed)
    return found


def trimmed_to_nodes(seq, n, closed=False, tt=11):
    """`seq` trimmed from the right until the oracle extracts exactly `n` nodes from it; None if no cut gives that count."""
    length = len(seq)
    lo, hi = 0, length                            # the count grows with the length but for a few nodes: bisect near, then go base by base
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if extracted(seq[:mid], closed, tt).num_nodes > n else (mid, hi)
    for cut in range(min(length, hi + 256), 0, -1):
        k = extracted(seq[:cut], closed, tt).num_nodes
        if k == n:
            return seq[:cut]
        if k < n - 8:                             # the count falls by a few nodes at a time: far below n it does not come back
            break
    return None
