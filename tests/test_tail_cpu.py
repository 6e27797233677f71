"""The inputs of tests/test_tail_shapes_gpu.py hold what they claim to hold, checked with the CPU oracle alone: tests/tail_ref.py
restates the traceback tail (ref: lib.pyx:1253-1311, 3231-3401, Prodigal dprog.c eliminate_bad_genes) and counts, as it goes, which
side of every rule an input reaches; tests/tail_shapes.py builds the inputs.  Every run below first compares tail_ref with the
oracle's staged calls (dprog, eliminate_bad_genes, extract_genes, tweak_final_starts): traceb, tracef, ov_mark, elim, the start
scores as bit patterns, the gene list before and after the tweak.  Then the populations are asserted per series, so that the GPU
test compares the device on inputs that are known to reach both sides of each rule.  The rules have one text each
(pyrodigal_amd/csrc/tail_rules.h); what differs between the forms is who enumerates, once per enumeration:

  splices, elimination      k_tp_small (chains of at most 4 096 nodes), k_tp_slots .. k_tp_elim_b (PGA_TP_STEPS or longer chains),
                            the serial walks untangle / eliminate_bad_genes (PGA_TAIL=device, host): the splice and the
                            elimination series are short enough for the first and run under every form
  gene list                 tp_extract_rounds with 64 and 256 threads (k_tp_small), with 256 and 1 024 (k_tp_extract),
                            k_tp_extract_sum / _chunk, the serial extract_genes: one contig of the gene-list series each
  start tweaks              a thread per gene (tweak_one: k_tail_tweak, k_tail_tweak_packed, the host), a wavefront per gene
                            (tweak_one_wave: k_tail_tweak_wave, k_tail_tweak_fixup): the tweak batch runs under all

Populations that were sought and not found are asserted to be ABSENT, so that nobody takes them for covered."""
import functools

import pytest

from oracle import oracle as orc
from tests import dp_inject
from tests import tail_ref as tr
from tests import tail_shapes as ts


@functools.lru_cache(maxsize=None)
def single(key, model=None, closed=False, max_overlap=60):
    """tail_ref.run (checked against the oracle) of a named contig in single mode."""
    tinf = ts.nctc() if model is None else ts.altered(*model)
    return tr.run(contig(key), tinf, closed=closed, max_overlap=max_overlap, min_gene=ts.MIN_GENE[max_overlap])


def contig(key):
    kind, k = key
    if kind == "splice":
        return ts.splice_series()[k]
    if kind == "tweak":
        return ts.tweak_contig(k)
    if kind == "gene_list":
        return ts.GENE_LIST[k][0]()
    if kind == "nodes":
        return ts.with_nodes(k)
    if kind == "long_tweak":
        return ts.cut(*(ts.LONG_TWEAK_200 if k == 200 else ts.LONG_TWEAK))
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def meta(series, closed=False, max_overlap=60):
    """tail_ref.run of every contig of a series under the model that wins it in meta mode; the final genes are the oracle's."""
    models = ts.meta_models()
    out = []
    for s in getattr(ts, series)():
        o = orc.Oracle(s)
        phase = o.find_genes_meta(models, orc.Params(closed=closed, max_overlap=max_overlap, min_gene=ts.MIN_GENE[max_overlap]))
        assert phase >= 0
        r = tr.run(s, models[phase], closed=closed, is_meta=True, max_overlap=max_overlap, min_gene=ts.MIN_GENE[max_overlap])
        assert r["final"].tobytes() == o.genes().tobytes()
        out.append(r)
    return out


def report(name, c, keys=None):
    print("%-28s %s" % (name, {k: c[k] for k in (keys or sorted(c))}))


SPLICE_KEYS = tr.EDGE_CLASSES + ("adjacent_splices", "splice_first_edge", "splice_head_edge", "frame_differs_fs_fs",
                                 "frame_differs_rs_rs", "no_triple_for_the_mark_alone", "no_triple_for_the_position_alone")


# ---- splices ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("closed", [False, True])
def test_splice_series_holds_every_class(closed):
    runs = [single(("splice", k), closed=closed) for k in range(len(ts.SPLICE_SLICES))]
    c = tr.total(runs, "untangle")
    report("splices closed=%d" % closed, c, SPLICE_KEYS + ("path",))
    assert all(r["n_nodes"] <= 4096 for r in runs)                        # k_tp_small takes them, k_tp_slots under PGA_TP_STEPS
    assert all(c[k] >= 3 for k in tr.EDGE_CLASSES), c
    # (with closed ends slice 0's last gene, an edge gene, is gone, and the best gene end with it; the elimination series has such edges open and closed)
    assert c["adjacent_splices"] >= 3 and c["splice_first_edge"] >= (0 if closed else 1) and c["splice_head_edge"] >= 1, c
    # the frame that picks the start of an overlapping gene is the OTHER node's: the two differ
    assert c["frame_differs_fs_fs"] >= 3 and c["frame_differs_rs_rs"] >= 3, c
    # a reverse stop in front of a forward stop that is NOT a triple overlap only because its ov_mark says so
    assert c["no_triple_for_the_mark_alone"] >= 3, c
    # per slice: the spliced-in nodes are on the final path and nowhere else
    for r in runs:
        U = r["U"]
        assert len(U["path"]) == len(U["raw_path"]) + len(U["spliced"]) and not set(U["raw_path"]) & U["spliced"]


@pytest.mark.parametrize("max_overlap", [30, 200])
def test_splice_series_under_other_overlaps(max_overlap):
    runs = [single(("splice", k), max_overlap=max_overlap) for k in range(len(ts.SPLICE_SLICES))]
    c = tr.total(runs, "untangle")
    report("splices max_overlap=%d" % max_overlap, c, SPLICE_KEYS)
    assert all(c[k] >= 3 for k in ("rb_fs", "fs_fs", "rs_rs")), c
    assert c["triple"] >= (3 if max_overlap == 200 else 1), c              # a triple overlap needs room for three genes


def test_splice_and_elimination_series_in_meta_mode():
    for series in ("splice_series", "elimination_series"):
        for closed in (False, True):
            runs = meta(series, closed)
            c = tr.total(runs, "untangle")
            report("%s meta closed=%d" % (series, closed), c, SPLICE_KEYS)
            assert all(c[k] >= 3 for k in tr.EDGE_CLASSES), (series, closed, c)


# ---- elimination --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("closed", [False, True])
def test_elimination_series_holds_both_rules(closed):
    runs = meta("elimination_series", closed)
    c = tr.total(runs, "eliminate")
    report("elimination closed=%d" % closed, c)
    assert all(r["n_nodes"] <= 2048 for r in runs)                         # k_tp_small with 64 threads
    assert c["mark_fwd_start"] >= 10 and c["mark_rev_stop"] >= 10 and c["mark_on_spliced"] >= 1, c
    assert c["term_after_fwd_stop"] >= 100 and c["term_rev_start"] >= 100, c
    # the reverse-stop rule reads the score of the START behind the stop: stops whose own score is negative while the start's is not
    assert c["rev_stop_own_score_negative"] >= 10, c
    u = tr.total(runs, "untangle")
    assert u["splice_head_edge"] >= 1 and u["splice_first_edge"] >= 1, u
    # `ndx[p] > ndx[nx]` never decides alone whether an edge is a triple overlap: sought on the genome, its reverse complement and 300
    # contigs of random sequence, not found
    assert u["no_triple_for_the_position_alone"] == 0


@pytest.mark.parametrize("closed", [False, True])
def test_mark_reset_series(closed):
    """Everywhere else the `ov_mark = -1` of the first untangling pass writes what is there already."""
    tinf = ts.meta_models()[ts.MARK_RESET_MODEL]
    runs = [tr.run(s, tinf, closed=closed) for s in ts.mark_reset_series()]
    u = tr.total(runs, "untangle")
    report("mark reset closed=%d" % closed, u, SPLICE_KEYS + ("triple_resets_a_mark",))
    assert u["triple_resets_a_mark"] >= 2 and all(r["n_nodes"] <= 2048 for r in runs), u
    others = [single(("splice", k), closed=closed) for k in range(len(ts.SPLICE_SLICES))] + [single(("gene_list", k)) for k in ts.GENE_LIST]
    assert tr.total(others, "untangle")["triple_resets_a_mark"] == 0


def test_no_node_receives_both_score_terms():
    """The first term goes to the node behind a forward stop, the second to a reverse start.  A reverse start directly behind a
    forward stop is exactly what the rb_fs splice removes (it puts the reverse stop between them), so after untangling no node
    receives both, on any input: asserted on every series so that a change of the untangling that made it possible would show."""
    everything = [single(("splice", k)) for k in range(len(ts.SPLICE_SLICES))] + meta("elimination_series") + \
                 [single(("gene_list", k)) for k in ts.GENE_LIST] + [single(("tweak", k), ts.TWEAK_MODEL) for k in ts.TWEAK_LEFT]
    assert tr.total(everything, "eliminate")["both_terms"] == 0


# ---- gene list ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ts.GENE_LIST))
def test_gene_list_series_paths_are_longer_than_their_unit(name):
    make, nodes, unit, _ = ts.GENE_LIST[name]
    r = single(("gene_list", name))
    path = r["counters"]["untangle"]["path"]
    report("gene list %s" % name, r["counters"]["extract"] + r["counters"]["eliminate"])
    print("   nodes %d path %d genes %d" % (r["n_nodes"], path, len(r["genes"])))
    assert r["n_nodes"] == nodes and path > unit and len(r["genes"]) > unit // 2
    if name == "wave":
        assert r["n_nodes"] <= 2048
    if name == "round":
        assert r["n_nodes"] == 4096 and path > 256
    if name == "steps":
        assert 4096 < r["n_nodes"] < 32768
    if name == "chunk":
        assert r["n_nodes"] >= 32768 and r["counters"]["eliminate"]["eliminated"] >= 4
        assert r["counters"]["eliminate"]["mark_fwd_start"] >= 1 and r["counters"]["eliminate"]["mark_rev_stop"] >= 1
        # genes are emitted in more than one chunk, and an eliminated pair lies in a chunk that is not the first
        order = r["U"]["path"][::-1]
        assert any(r["elim"][p] == 1 for p in order[1024:])
    # every gene's setters come from the final path and give back the gene
    for g, (rb, re, rs, rt) in zip(r["genes"], r["setters"]):
        order = r["U"]["path"][::-1]
        assert order[rs] == g["start_ndx"] and order[rt] == g["stop_ndx"]


def test_a_gene_never_straddles_a_unit():
    """A path is a sequence of (start, stop) pairs: its head opens a gene, every splice restores the node that a shortcut of the
    connection scoring left out, and both elimination rules mark a pair.  So the path has an even number of nodes, the two nodes of
    a gene sit at positions 2k and 2k + 1 from the head, and no gene -- live or eliminated -- has its nodes in different units of 64,
    256 or 1 024 positions.  The running maxima that the gene list carries from one wave, round or chunk into the next are therefore
    never read by a gene of a valid path (the gene COUNT carried alongside is read by every later gene).  Sought on the genome and
    its reverse complement under five models and three overlaps, and on every series here: not found, and asserted absent."""
    everything = [single(("splice", k), closed=c) for k in range(len(ts.SPLICE_SLICES)) for c in (False, True)] + \
        meta("elimination_series") + meta("elimination_series", True) + [single(("gene_list", k)) for k in ts.GENE_LIST] + \
        [single(("tweak", k), ts.TWEAK_MODEL) for k in ts.TWEAK_LEFT]
    c = tr.total(everything, "extract")
    assert c["genes"] > 2000
    for k in ("path_parity", "gene_with_unset_field", "setter_not_adjacent") + tuple("straddle_%d" % u for u in tr.UNITS) + \
            tuple("elim_pair_across_%d" % u for u in tr.UNITS):
        assert c[k] == 0, (k, c[k])
    for r in everything:
        assert all(rs + 1 == rt or rt + 1 == rs for _, _, rs, rt in r["setters"])


def test_trimming_one_gene_shifts_every_gene_by_a_pair():
    tinf = ts.nctc()
    for name in ("wave", "round"):
        full = single(("gene_list", name))
        less = tr.run(ts.minus_one_gene(contig(("gene_list", name)), tinf), tinf)
        assert len(less["genes"]) == len(full["genes"]) - 1
        assert less["counters"]["untangle"]["path"] == full["counters"]["untangle"]["path"] - 2


# ---- start tweaks ---------------------------------------------------------------------------------------------------------------------------

TWEAK_REQUIRED = ("far_0", "far_1", "near_0", "near_1", "reject_0", "reject_1", "pick_0", "pick_1", "cut_maxov_fwd", "cut_maxov_rev",
                  "cut_prev_rev_start", "cut_next_fwd_start", "window_clipped_low", "window_clipped_high", "move_fwd", "move_rev",
                  "redone", "differs", "second_best_filled", "near_ig_term", "candidate_15_away")
TWEAK_NOT_FOUND = ("diff_equals_maxov", "change_travels_on", "change_travels_across_window")


def tweak_batch_runs(max_overlap=60, closed=False):
    """The tweak batch of the GPU test: the tweak series and the splice series under TWEAK_MODEL."""
    return [single(("tweak", k), ts.TWEAK_MODEL, closed, max_overlap) for k in ts.TWEAK_LEFT] + \
           [single(("splice", k), ts.TWEAK_MODEL, closed, max_overlap) for k in range(len(ts.SPLICE_SLICES))]


@pytest.mark.parametrize("closed", [False, True])
def test_tweak_series_differs_at_every_place_of_a_window(closed):
    places = tr.Counter()
    for name, (left, index) in ts.TWEAK_LEFT.items():
        r = single(("tweak", name), ts.TWEAK_MODEL, closed)
        c = r["counters"]["tweak"]
        report("tweak %s closed=%d" % (name, closed), c, ("genes", "redone", "differs", "redone_behind_63"))
        assert r["differs"] == [index], (name, r["differs"])
        assert index in r["redone"]
        i = index
        assert r["final"][i] != r["parallel"][i]                          # a fix-up that returned the parallel pass would be wrong here
        places.update({k: v for k, v in c.items() if k.startswith("differs_") or k == "redone_behind_63"})
    assert places["differs_window_first"] >= 1 and places["differs_window_last"] >= 2 and places["differs_window_interior"] >= 3, places
    assert places["differs_past_first_window"] >= 3 and places["redone_behind_63"] >= 2, places
    # first of a window behind at least 65 genes, last of a window beyond the first, interior beyond the first
    assert ts.TWEAK_LEFT["first_of_window"][1] % 64 == 1 and ts.TWEAK_LEFT["first_of_window"][1] >= 65
    assert ts.TWEAK_LEFT["last_of_window"][1] % 64 == 0 and ts.TWEAK_LEFT["last_of_window"][1] >= 65
    assert ts.TWEAK_LEFT["interior"][1] % 64 not in (0, 1) and ts.TWEAK_LEFT["interior"][1] >= 65


@pytest.mark.parametrize("max_overlap", ts.MAX_OVERLAPS)
def test_tweak_batch_holds_every_branch(max_overlap):
    c = tr.total(tweak_batch_runs(max_overlap), "tweak")
    report("tweak batch max_overlap=%d" % max_overlap, c)
    # (no candidate within 100 nodes of a start lies more than 200 bases beyond the neighbour's stop: those two cuts need 30 or 60)
    missing = [k for k in TWEAK_REQUIRED if c[k] == 0 and not (max_overlap == 200 and k.startswith("cut_maxov"))]
    assert not missing, (missing, c)
    assert c["redone"] >= 10 and c["move_rev"] >= 10 and c["move_fwd"] >= 10, c
    for k in TWEAK_NOT_FOUND:           # sought on the genome and its reverse complement under every model of ALTERED and every overlap
        assert c[k] == 0, "%s turned up: assert it and take it off the not-found list of DESIGN 4.5" % k


def test_equal_positions_at_the_neighbour_cuts():
    """`start of the reverse predecessor - candidate >= 0` and its mirror image: a candidate exactly AT the neighbour's start.  The
    elimination series holds the forward-successor case; the reverse-predecessor case was sought and not found."""
    c = tr.total(meta("elimination_series") + tweak_batch_runs(), "tweak")
    report("equal cuts", c, ("cut_prev_rev_start_equal", "cut_next_fwd_start_equal"))
    assert c["cut_next_fwd_start_equal"] >= 1
    assert c["cut_prev_rev_start_equal"] == 0


def test_long_contig_holds_the_differing_gene():
    r = single(("long_tweak", 0), ts.TWEAK_MODEL)
    report("long tweak", r["counters"]["tweak"], ("genes", "redone", "differs", "move_rev", "move_fwd"))
    assert r["n_nodes"] == 32768 and len(r["differs"]) == 1 and len(r["redone"]) >= 10
    assert r["differs"][0] >= 65
    r = single(("long_tweak", 200), ts.TWEAK_MODEL, False, 200)
    assert r["n_nodes"] >= 32768 and r["differs"] == [432] and len(r["redone"]) >= 10


# ---- launch edges and tools -----------------------------------------------------------------------------------------------------------------

def test_contigs_of_exact_node_counts():
    for n in ts.NODE_CUTS:
        assert dp_inject.extracted(ts.with_nodes(n)).num_nodes == n
    assert ts.find_cut(1, 0, 2049, 40000) == ts.NODE_CUTS[2049][2]        # the search that made the table
    assert dp_inject.extracted(dp_inject.contig_with_nodes(257, 0.5, 31)).num_nodes == 257      # the synthetic form, as before


def test_place_gene_finds_a_slice_of_the_series_again():
    tinf = ts.altered(*ts.TWEAK_MODEL)
    got = ts.place_gene(ts.tweak_contig("last_of_window"), tinf, 65)
    assert got is not None and got[1]["differs"] == [65]
    assert ts.TWEAK_LEFT["last_of_window"][0] + got[0] == ts.TWEAK_LEFT["first_of_window"][0]


def test_companion_batches_hold_the_degenerate_contigs():
    for k in (62, 254, 1024):
        batch = ts.companions(k) if k < 1000 else ts.repeated(k)
        assert len(batch) == k and all(d in batch for d in ts.DEGENERATE)
    assert len(set(ts.repeated(1024))) <= 16
