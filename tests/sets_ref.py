"""The rule for contig sets in meta mode, restated over the CPU oracle's stage calls: one GC window and one model
per set of contigs.  Reference for tests/test_sets_cpu.py, tests/test_sets_gpu.py and tests/test_cli_sets_gpu.py."""
import math

import numpy as np

from oracle import oracle as orc
from tests.circular_ref import meta_bins  # noqa: F401  (the 13 bins of tests/golden/models, for the tests)
from tests.util import synthetic_contig


def gc_count(seq):
    """G + C letters of a sequence, either case (what the digitizer counts)."""
    s = bytes(seq).upper()
    return s.count(b"G") + s.count(b"C")


def window(gc):
    """The GC window of meta mode (ref: lib.pyx:5335-5336): the two expressions of po_find_genes_meta."""
    return min(0.65, 0.88495 * gc - 0.0102337), max(0.35, 0.86596 * gc + 0.1131991)


def models_in(gc, models):
    low, high = window(gc)
    return [m for m, t in enumerate(models) if not (t.gc < low or t.gc > high)]


def dense_sets(labels):
    """Labels (None: on its own) to dense ids in order of first appearance; every unlabelled contig a set of its own."""
    ids, seen, out = 0, {}, []
    for lab in labels:
        if lab is None:
            out.append(ids)
            ids += 1
        else:
            if lab not in seen:
                seen[lab] = ids
                ids += 1
            out.append(seen[lab])
    return out


def walk(seq, models, window_models, params, stop_at=None, **oracle_kw):
    """The reference's loop (po_find_genes_meta) of one contig over `window_models`, in model order: extract on a change of table,
    reset, score with is_meta, overlapping starts, connection scoring; the state one model leaves for the next is kept.  Returns
    (oracle, {model: path score} for the models under which the contig has nodes and a path).  With `stop_at` the loop ends after
    that model's visit and runs the tail there (eliminate_bad_genes, extract_genes, tweak_final_starts): the oracle then holds the
    genes of that visit."""
    o = orc.Oracle(seq, **oracle_kw)
    scores, tt = {}, -1
    for m in window_models:
        t = models[m]
        if t.trans_table != tt:
            tt = t.trans_table
            o.extract(tt, params)
            o.sort()
        o.reset_scores()
        o.score_nodes(t, closed=bool(params.closed), is_meta=True)
        o.overlapping_starts(t, 1, params.max_overlap)
        ipath = o.dprog(t, True)
        if o.num_nodes > 0 and ipath >= 0:
            scores[m] = float(o.nodes(copy=False)["score"][ipath])
            if m == stop_at:
                o.eliminate_bad_genes(ipath, t)
                o.extract_genes(ipath)
                o.tweak_final_starts(t, params.max_overlap)
        if m == stop_at:
            break
    return o, scores


class Member:
    """One contig of a call: `model` (W of its set when the contig contributed under it, else -1), `genes` and `nodes` (the
    oracle's arrays: the genes of W's visit, the nodes of the fresh re-score under W; empty without a model), `scores`
    ({model: path score}), `set_model` / `set_score` (W and S_W of its set; -1 / NaN) and `window` (the models of its set's window)."""


def find_genes_sets(seqs, labels, models, closed=False, **oracle_kw):
    """The rule: returns one Member per contig."""
    params = orc.Params(closed=closed)
    seqs = [s.encode("ascii") if isinstance(s, str) else bytes(s) for s in seqs]
    ids = dense_sets(labels)
    ns = max(ids) + 1 if ids else 0
    # 1. the window of every set: integers summed exactly, one division
    gsum, lsum = [0] * ns, [0] * ns
    for s, a in zip(seqs, ids):
        gsum[a] += gc_count(s)
        lsum[a] += len(s)
    win = [models_in(gsum[a] / lsum[a] if lsum[a] > 0 else 0.0, models) for a in range(ns)]
    # 2. every member under every model of the window
    out = []
    for s, a in zip(seqs, ids):
        mb = Member()
        mb.seq, mb.set, mb.window = s, a, win[a]
        _, mb.scores = walk(s, models, win[a], params, **oracle_kw)
        out.append(mb)
    # 3. the choice: sums in batch order, the largest above -100, the lowest index among equals
    S = [dict() for _ in range(ns)]
    for mb in out:
        for m, v in mb.scores.items():
            S[mb.set][m] = S[mb.set][m] + v if m in S[mb.set] else v
    W = []
    for a in range(ns):
        best, w = -100.0, -1
        for m in sorted(S[a]):
            if S[a][m] > best:
                best, w = S[a][m], m
        W.append(w)
    # 4. the result of every member
    for mb in out:
        w = W[mb.set]
        mb.set_model, mb.set_score = w, (S[mb.set][w] if w >= 0 else math.nan)
        mb.set_sums = S[mb.set]
        if w >= 0 and w in mb.scores:
            o, _ = walk(mb.seq, models, mb.window, params, stop_at=w, **oracle_kw)
            mb.genes = o.genes()
            t = models[w]
            o.extract(t.trans_table, params)
            o.sort()
            o.reset_scores()
            o.score_nodes(t, closed=bool(params.closed), is_meta=True)
            mb.model, mb.nodes = w, o.nodes()
        else:
            mb.model, mb.genes, mb.nodes = -1, np.zeros(0, orc.GENE_DTYPE), np.zeros(0, orc.NODE_DTYPE)
    return out


def per_contig_winner(seq, models, closed=False, **oracle_kw):
    """Today's meta mode on one contig (Oracle.find_genes_meta): (model, oracle)."""
    o = orc.Oracle(seq, **oracle_kw)
    return o.find_genes_meta(models, orc.Params(closed=closed)), o


# ---- the inputs of the GPU tests: chosen here so that the conditions test_sets_cpu.py asserts hold in the reference alone --------------

def case_interleaved():
    """(a) a set of 3 contigs of 2-8 kbp, interleaved with unlabelled contigs and with a second set; members not adjacent."""
    seqs = [synthetic_contig(7919, 0.47, 4101), synthetic_contig(3001, 0.62, 4102), synthetic_contig(2003, 0.44, 4103),
            synthetic_contig(4099, 0.36, 4104), synthetic_contig(5003, 0.52, 4105), synthetic_contig(2503, 0.66, 4106),
            synthetic_contig(3511, 0.41, 4107)]
    labels = ["A", None, "A", "B", "A", None, "B"]
    return seqs, labels


def case_mixed_gc():
    """(b) members near GC 0.35 and near GC 0.65: the pooled window (around 0.5) holds the one translation-table-4 bin, which no
    member's own window reaches."""
    seqs = [synthetic_contig(6007, 0.35, 4201), synthetic_contig(6011, 0.65, 4202), synthetic_contig(2999, 0.34, 4203),
            synthetic_contig(3203, 0.66, 4204)]
    return seqs, ["mix"] * 4


def case_many_short():
    """(c) a set of 300 members of 300-600 bp (more than one workgroup of the segmented sum; the short-contig meta penalties), after
    one unlabelled contig."""
    seqs = [synthetic_contig(2500, 0.5, 4300)] + [synthetic_contig(300 + (k * 37) % 301, 0.40 + 0.2 * ((k * 7) % 11) / 10, 4301 + k) for k in range(300)]
    return seqs, [None] + ["many"] * 300


def case_no_nodes():
    """(d) a set whose members have no nodes at all (too short, or unknown bases only), a set whose one member has nodes but no
    path, and a set that has genes."""
    seqs = [b"ACGTACGTAC", b"N" * 30, b"AT", synthetic_contig(2200, 0.5, 4401), b"", b"ACGT" * 20, b"A" * 50, synthetic_contig(1800, 0.48, 4402)]
    return seqs, ["empty", "empty", "empty", "full", "empty", "nopath", "empty", "full"]


def case_no_model():
    """(d) a set with no model in its window: low-GC contigs under the four bins of GC 0.61 and above.  Returns (seqs, labels, the
    indices of those bins)."""
    seqs = [synthetic_contig(2100, 0.36, 4501), synthetic_contig(1500, 0.33, 4502), synthetic_contig(2400, 0.64, 4503)]
    return seqs, ["low", "low", None], [9, 10, 11, 12]
