"""The restatement of the training (tests/train_ref.py) against the oracle on every genome of tests/train_shapes.py, and the
populations those genomes hold: which side of every rule of pyrodigal_amd/csrc/train.inl they reach, on both strands.  No device:
tests/test_train_shapes_gpu.py compares the kernels on the same genomes, and a population asserted here is what makes a wrong
comparison, window or bound there change a byte."""
from collections import Counter
from functools import lru_cache

import numpy as np
import pytest

from oracle import oracle as orc
from tests import train_ref as tr
from tests import train_shapes as ts


def oracle_blob(g, upto):
    o = g.opts
    p = orc.Params(closed=o.get("closed", False), min_gene=o.get("min_gene", 90))
    return orc.Oracle(g.seq, mask=o.get("mask", False)).train(p, force_nonsd=o.get("force_nonsd", False), start_weight=o.get("start_weight", 4.35),
                                                             tt=o.get("translation_table", 11), upto=upto).tobytes()


@lru_cache(maxsize=None)
def compared(name):
    """One series restated and held to the oracle, once: (what differs, how many genomes trained, {side: Counter} of its populations)."""
    genomes = ts.fixture_slices() if name == "fixtures" else ts.series(name)
    bad, trained, counted = [], 0, {1: Counter(), -1: Counter()}
    for g in genomes:
        out, c = tr.train(g.seq, **g.opts)
        counted[g.side].update(c)
        if out is None:
            if ts.n_nodes(g.seq, g.opts.get("translation_table", 11), g.opts.get("closed", False), g.opts.get("min_gene", 90)) != 0:
                bad.append((g.tag, g.side, "no nodes"))
            continue
        trained += 1
        bad += [(g.tag, g.side, upto, d) for upto in (1, 2, 3, 0) for d in [tr.differing_fields(out[upto], oracle_blob(g, upto))] if d]
    return bad, trained, len(genomes), counted


@pytest.fixture(scope="module")
def populations():
    """{side: Counter} over every series (not the fixture slices): counted here, whichever tests of the module run."""
    total = {1: Counter(), -1: Counter()}
    for name in ts.SERIES:
        for side in (1, -1):
            total[side].update(compared(name)[3][side])
    return total


@pytest.mark.parametrize("name", list(ts.SERIES) + ["fixtures"])
def test_the_restatement_equals_the_oracle(name):
    bad, trained, n, _ = compared(name)
    assert bad == []
    assert trained >= n - 8


# ---- the GC frame plot: the device's windowed sum is the reference's running sums ---------------------------------------------------

def test_the_windowed_sum_is_the_frame_plot_of_the_reference():
    rng = np.random.default_rng(9100)
    for L in range(1, 401):
        for gc in (0.0, 0.2, 0.5, 0.8, 1.0, float(rng.random())):
            dig = rng.choice(4, size=L, p=[(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]).astype(np.uint8)
            if L % 7 == 0:
                dig[rng.integers(L)] = 6                                   # an unknown base counts as GC
            a, b = tr.gc_totals_windowed(dig), tr.gc_totals_running(dig)
            assert np.array_equal(a, b), (L, gc)
            gp = tr.gc_frame_plot(a)
            assert (gp[:3 * (L // 3)] >= 0).all() and (gp[3 * (L // 3):] == -1).all()


# ---- the populations ----------------------------------------------------------------------------------------------------------------
# what a node decides: non-empty on the forward and on the reverse strand
NODE_POPULATIONS = (
    ["ups_window_1_cut_%d" % k for k in range(3)] + ["ups_window_15_cut_%d" % k for k in range(31)]       # every cut of the two windows
    + ["motif_candidate_dropped_len_%d" % k for k in (3, 4, 5, 6)] + ["motif_search_without_candidates"]
    + ["stage2_falls_back_at_minus_four", "stage2_falls_back_below_no_mot_alone", "stage2_keeps_its_motif", "stage1_update_with_submotifs"]
    + ["pick_rbs_w0_above", "pick_rbs_r1_zero", "pick_rbs_w0_below", "pick_rbs_r0_zero", "pick_rbs_larger_bin"]
    + ["first_start_taken_at_zero_or_above", "first_start_refused_below_zero", "later_start_replaces_the_best"]
    + ["orf_confident", "orf_not_confident", "orf_without_a_usable_start", "confident_start_rbs_bin_nonzero"]
    + ["ctr_tie_ab", "ctr_tie_ac", "ctr_tie_bc", "bias_walk_reaches_last_codon"]
    + ["gene_ends_within_5_of_the_downstream_end", "gene_starts_within_5_of_the_upstream_end"]
    + ["start_abuts_the_stop_before_it", "start_abuts_a_stop_that_has_overlapping_starts"])
# what a genome decides: non-empty among the forward genomes and among their reverse complements
GENOME_POPULATIONS = (
    ["plot_tie_ab", "plot_tie_ac", "plot_tie_bc", "plot_tie_abc"]
    + ["sd_rounds_halve_and_keep", "sd_rounds_all_halve", "motif_rounds_halve_and_keep", "motif_rounds_all_halve"]
    + ["halves_at_equality", "keeps_one_node_below_equality", "nodes_at_least_2000", "nodes_below_2000"]
    + ["rbs_sum_zero", "rbs_sum_nonzero", "type_sum_zero", "type_sum_nonzero", "motif_round_sum_zero", "motif_round_sum_nonzero"]
    + ["coverage_%d_at_length_%d" % (v, ln) for v in (0, 1, 2) for ln in (5, 6)]
    + ["sd_term_%s_decides_alone" % t for t in "ABCD"] + ["uses_sd_0", "uses_sd_1", "forced_nonsd_against_the_rule"]
    + ["ups_row_nonzero_low", "ups_row_nonzero_middle", "ups_row_nonzero_high", "ups_row_zero_middle", "no_mot_at_minus_four"]
    + ["genome_without_nodes", "path_with_genes"])
# Of the populations the issue lists, sought and not found; asserted absent so that a change which makes one reachable fails here
# (DESIGN.md 4.7.1 says why each is out of reach of a generator): an exact tie between two starts of one ORF and a start worth exactly
# 0.0 (the length factor of the coding score differs between any two starts by a difference of logarithms), RBS weights exactly 1.0
# apart (differences of logarithms of count ratios), and a training path that holds no gene (every start-stop pair scores above zero in
# the training pass).
ABSENT = (("later_start_equals_the_best", True), ("first_start_exactly_zero", True), ("pick_rbs_weights_exactly_one_apart", True),
          ("path_without_genes", False))
MAX_ABSENT = 4
# Outside that count of four, and asserted at zero all the same.  Two things are kept apart from ABSENT, and the count of four is
# exact only because they are:
#   * one exact equality that the issue does not list, an ORF whose best start is worth exactly the threshold (17.5, 35, ...): it is
#     what `best >= sthresh` written as `>` would need, and is out of reach for the reason the first two of ABSENT are;
#   * one population that the issue does list but that is no population: the stage-1 update starts at the motif's own position, which
#     the search only takes at j >= 0, so its `j < 0` skip can never fire (the same holds for the `bsc == -4.0` term of stage 2, which
#     train_ref asserts where it restates it).
UNLISTED_EQUALITY = ("orf_best_exactly_at_sthresh",)
NEVER = ("stage1_update_skips_before_the_sequence",)


def test_the_series_hold_every_population_on_both_strands(populations):
    both = populations[1] + populations[-1]
    missing = [(k, s) for k in NODE_POPULATIONS for s in (1, -1) if both[(k, s)] == 0]
    missing += [(k, side) for k in GENOME_POPULATIONS for side in (1, -1) if populations[side][(k, None)] == 0]
    assert missing == []
    assert len(ABSENT) <= MAX_ABSENT                                        # 4 of the issue's populations are asserted absent
    for k, per_strand in ABSENT:
        assert [both[(k, s)] for s in ((1, -1) if per_strand else (None,))] == [0] * (2 if per_strand else 1), k
    for k in UNLISTED_EQUALITY + NEVER:                                     # and, beyond them, one equality and one invariant
        assert both[(k, 1)] == 0 and both[(k, -1)] == 0, k
    assert both[("orf_confident", 1)] and both[("orf_not_confident", -1)]  # (the counters next to the equality do count)


# ---- the batch: what bounds a stop's walk ---------------------------------------------------------------------------------------------

@lru_cache(maxsize=None)
def sorted_nodes(seq, tt):
    o = orc.Oracle(seq)
    o.extract(tt, orc.Params(closed=False, min_gene=90))
    o.sort()
    nd = o.nodes()
    return tuple(nd[k].tolist() for k in ("ndx", "stop_val", "strand", "type"))


@pytest.mark.parametrize("G", ts.BATCH_SIZES)
def test_no_walk_of_a_stop_takes_a_node_of_a_neighbouring_genome(G):
    """k_ts_best walks from a stop over the nodes [lo, n) of its genome.  In a batch the genomes' nodes lie back to back, and without
    those two bounds a walk would go on into a neighbour.  It would take nothing there: walking down, the first forward node of a frame
    that the genome before holds is a stop (every start has its stop above it; an ORF open at the end has an edge stop), and walking
    up, the first reverse node of a frame that the next genome holds is a stop likewise, so the `type[j] == PGA_T_STOP` break ends the
    walk before any start.  `lo` and `n` of k_ts_best are therefore protected by that break and by no test of the device; this test
    holds the argument to the oracle's nodes of every batch, where many walks do step onto a neighbour."""
    members, _ = ts.batch(G)
    ndx, stop_val, strand, type_, bounds = [], [], [], [], []
    for m in members:
        a = sorted_nodes(m.seq, m.translation_table)
        bounds.append((len(ndx), len(ndx) + len(a[0])))
        ndx += a[0]; stop_val += a[1]; strand += a[2]; type_ += a[3]
    n_all, stepped_over = len(ndx), {1: 0, -1: 0}
    for lo, n in bounds:
        for s in range(lo, n):
            if type_[s] != tr.T_STOP:
                continue
            inside, end = tr.walk_of_a_stop(ndx, stop_val, strand, type_, s, lo, n)
            assert tr.walk_of_a_stop(ndx, stop_val, strand, type_, s, 0, n_all)[0] == inside, (G, s)
            stepped_over[strand[s]] += int(not lo <= end < n and 0 <= end < n_all)
    assert G < 63 or (stepped_over[1] > 0 and stepped_over[-1] > 0)          # (G = 2 is one genome with nodes and one without)


def test_the_halving_at_equality_changes_a_model():
    """Reaching sum * 2000 == n is not enough: where the one confident ORF scores far above every threshold, halving or not changes
    nothing.  The "halving" genomes hold a second ORF that only the halved threshold admits: restated with `<` for `<=`, the training
    gives another model, on either strand."""
    genomes = [g for g in ts.series("threshold") if g.tag == ("halving",)]
    assert [g.side for g in genomes] == [1, -1]
    for g in genomes:
        inputs = tr.Inputs(g.seq, closed=True)
        assert inputs.n == 2000
        right, c = tr.train(g.seq, inputs=inputs, **g.opts)
        wrong, _ = tr.train(g.seq, inputs=inputs, variant=("halving_lt",), **g.opts)
        assert c[("halves_at_equality", None)] > 0 and c[("uses_sd_0", None)] == 1
        assert right[3] != wrong[3] or right[0] != wrong[0], g.side


def test_the_sixteen_combinations_of_the_sd_terms():
    """determine_sd_usage as a truth table: A implies C, so twelve combinations exist; the rule is 0 exactly where A or (B and (C or D))."""
    w = [0.0] * 28
    seen = set()
    for w0 in (-1.0, -0.5, -0.25, 0.0, 0.5):
        for b in (0.99, 1.0):
            for d in (1.99, 2.0):
                for kb in (13, 15, 16):
                    for kd in (22, 24, 27):
                        w = [0.0] * 28
                        w[0], w[kb], w[kd] = w0, b, d
                        t = tr.sd_terms(w)
                        seen.add(t)
                        assert tr.determine_sd_usage(w, Counter()) == (0 if (w0 >= 0.0 or (b < 1.0 and (w0 >= -0.5 or d < 2.0))) else 1)
    assert len(seen) == 12
