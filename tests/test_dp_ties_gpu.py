"""GPU parity of every connection-scoring kernel where scores tie (tests/dp_inject.py): the caller's score arrays, drawn so that
candidate connections offer equal values, through `pga_score_connections` / `pga_score_connections_training` against the CPU
oracle's serial loop.  The reference scans the sources in ascending order and joins with `>=` against a target that starts at 0.0
(ref: _connection.h:135/197 and siblings): the later source wins a tie and a sum of exactly 0.0 still connects; the frame of a
triple overlap is chosen with a strict `>`; the best gene end is the largest index among equals (ref: lib.pyx:1239-1251).  Scores
computed from a sequence never tie (0 ties, 0 zero-joins on every real-score input the oracle was asked about), so no other
test decides these rules.  Scores bit-identical, traceb / ov_mark / max index equal, as in test_dp_gpu.py; each case asserts from
the oracle's event counters that the rule was decided on its input (floors far below what the oracle counts: conditions on the
input, not tolerances)."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import dp_inject
from tests.util import read_fasta, synthetic_contig

pytestmark = pytest.mark.gpu

ENV = ("PGA_DP_KERNEL", "PGA_DP_WAVES", "PGA_DPW_SCHED", "PGA_DPW_SCHED_MISS", "PGA_DPW_TOPO_LDS", "PGA_DP_SEG", "PGA_DP_SEG_MIN",
       "PGA_DP_SEG_LEN", "PGA_DP_SEG_WARM", "PGA_DP_SEG_SLOTS", "PGA_DP_SEG_READBACK", "PGA_DP_SEG_WAVE", "PGA_DP_SEG_WSLOTS",
       "PGA_DP_SEG_WAVE_MIN")

VARIANTS = {                                     # the switches of test_dp_gpu.py
    "default": {},
    "wave": {"PGA_DP_KERNEL": "wave"},
    "wavedyn": {"PGA_DP_KERNEL": "wave", "PGA_DPW_SCHED": "0"},
    "wavemiss": {"PGA_DP_KERNEL": "wave", "PGA_DPW_SCHED_MISS": "1"},
    "tree1": {"PGA_DP_KERNEL": "tree1"},
    "tree3": {"PGA_DP_KERNEL": "tree3"},
    "scan1": {"PGA_DP_KERNEL": "scan", "PGA_DP_WAVES": "1"},
    "scan4": {"PGA_DP_KERNEL": "scan", "PGA_DP_WAVES": "4"},
    "scan16": {"PGA_DP_KERNEL": "scan", "PGA_DP_WAVES": "16"},
}


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def clean_env():
    saved = {k: os.environ.pop(k, None) for k in ENV}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def run(ctx, before, st_wt):
    return ctx.score_connections(before["ndx"], before["stop_val"], before["type"], before["strand"], before["cscore"], before["sscore"],
                                 before["rscore"], before["uscore"], before["star_ptr"], st_wt, True)


def same(out, ref, ref_max, what=""):
    score, traceb, ov, mi, _ = out
    bad = np.flatnonzero(traceb != ref["traceb"])
    assert len(bad) == 0, (what, len(bad), bad[:8], traceb[bad[:8]], ref["traceb"][bad[:8]])
    assert np.array_equal(score.view(np.uint64), ref["score"].view(np.uint64)), (what, "score not bit-identical")
    reached = ref["traceb"] != -1      # ov_mark is only defined once a connection was made
    assert np.array_equal(ov[reached], ref["ov_mark"][reached]), what
    assert mi == ref_max, what


def _floors(case, n, family, st_wt, ev):
    assert ev["ties"] >= (100 if n >= 600 else 20), (case, family, st_wt, ev)
    if family == "zero" and st_wt == 0.0:
        assert ev["zero_joins"] >= n / 2, (case, ev)
    if ev["frame_ties"]:
        assert case == "frames"


@pytest.fixture(scope="module")
def cases():
    """(name, family, st_wt, before, ref, ref_max, events) of every scorer-level case, from the oracle, once for all variants.
    Chains of 63 .. 129 nodes end at, one short of and one past the 64-node batches; about 700 nodes; 1 250 nodes slide the 1 000-node
    window, so that block, suffix and prefix maxima carry ties; 5 518 nodes lie in the band where the topology kernel stages a contig
    in LDS beyond 64 KB; two reference topologies.  quant and mag tie rarely on the small shapes and run from 700 nodes up."""
    from pyrodigal_amd import benchdata
    out = []

    def add(name, o, families, st_wts=(4.35, 0.0), tt=11, **kw):
        for family in families:
            for st_wt in st_wts:
                before, ref, ref_max, ev = dp_inject.inject_into(o, family, st_wt, seed=1, tt=tt, **kw)
                _floors(name, len(ref), family, st_wt, ev)
                out.append((name, family, st_wt, before, ref, ref_max, ev))

    for n in (63, 64, 65, 128, 129):
        o = dp_inject.extracted(dp_inject.contig_with_nodes(n, 0.5, 40 + n))
        assert o.num_nodes == n
        add("n%d" % n, o, ("zero", "pm1"))
    for n in (700, 1250):
        o = dp_inject.extracted(dp_inject.contig_with_nodes(n, 0.5, 40 + n))
        assert o.num_nodes == n
        add("n%d" % n, o, dp_inject.FAMILIES)
    o = dp_inject.extracted(synthetic_contig(150000, 0.5, 31))
    assert 5300 <= o.num_nodes <= 6144
    add("lds", o, dp_inject.FAMILIES)
    add("SRR492066", dp_inject.extracted(read_fasta("SRR492066.fna.gz")[0][1]), ("pm1",))
    # the topology of test_reverse_start_two_bases_before_a_reverse_stop, under its model's translation table
    tt = orc.Training(benchdata.load_model_set()[7][1]).trans_table
    o = dp_inject.extracted(read_fasta("sweep_830022_178.fna.gz")[0][1], closed=True, tt=tt)
    assert o.num_nodes == 3989
    add("sweep_830022_178", o, ("pm1",), tt=tt)
    # frames of a triple overlap that tie: only with star_ptr holding the first candidate of every frame (dp_inject.inject); seed 23 from
    # a search over seeds 0..39 on the oracle
    o = dp_inject.extracted(read_fasta("GCF_001457455.1_NCTC11397_genomic_100kb.fna.gz")[0][1], closed=True)
    before, ref, ref_max, ev = dp_inject.inject_into(o, "pm1", 0.0, seed=23, star_flag=0)
    assert ev["frame_ties"] >= 1 and ev["ties"] >= 100, ev
    out.append(("frames", "pm1", 0.0, before, ref, ref_max, ev))
    # what the module as a whole must have decided
    assert any(c[1] == "zero" and c[6]["best_end_ties"] >= 1 for c in out)
    assert any(c[6]["ovl_ties"] >= 1 for c in out) and any(c[6]["frame_ties"] >= 1 for c in out)
    return out


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_every_kernel_family_on_tied_scores(ctx, cases, variant):
    os.environ.update(VARIANTS[variant])
    for name, family, st_wt, before, ref, ref_max, ev in cases:
        what = (variant, name, family, st_wt)
        same(run(ctx, before, st_wt), ref, ref_max, what)
        if name == "lds":                         # ... and the topology from global memory
            os.environ["PGA_DPW_TOPO_LDS"] = "0"
            same(run(ctx, before, st_wt), ref, ref_max, what + ("PGA_DPW_TOPO_LDS=0",))
            del os.environ["PGA_DPW_TOPO_LDS"]


# ---- the segmented path: speculative walks, exact re-scoring and node-by-node verification where scores tie ----

@pytest.fixture(scope="module")
def genome():
    """The full genome's topology (153 296 nodes, closed ends), extracted once."""
    o = dp_inject.extracted(read_fasta("GCF_001457455.1_NCTC11397_genomic.fna.gz")[0][1], closed=True)
    assert o.num_nodes == 153296
    return o


@pytest.fixture(scope="module")
def genome_cases(genome):
    out = {}
    for family in ("quant", "zero"):
        before, ref, ref_max, ev = dp_inject.inject_into(genome, family, 4.35, seed=1)
        assert ev["ties"] >= 100_000, ev
        out[family] = (before, ref, ref_max)
    return out


SEG_PLANS = {
    "default": {},
    "len256_warm64": {"PGA_DP_SEG_MIN": "300", "PGA_DP_SEG_LEN": "256", "PGA_DP_SEG_WARM": "64"},
    "len64_warm64": {"PGA_DP_SEG_MIN": "300", "PGA_DP_SEG_LEN": "64", "PGA_DP_SEG_WARM": "64"},
    "len1024_warm128": {"PGA_DP_SEG_MIN": "300", "PGA_DP_SEG_LEN": "1024", "PGA_DP_SEG_WARM": "128"},
    # the scorer-level call never hands its segments to the wave-batch kernel, whatever this says (tests/test_finder_ties_gpu.py has
    # that walk under a model that ties); the plan must not depend on it
    "seg_wave_1": {"PGA_DP_SEG_WAVE": "1"},
}


@pytest.mark.parametrize("family", ["quant", "zero"])
@pytest.mark.parametrize("plan", list(SEG_PLANS))
def test_segmented_scoring_is_exact_on_tied_scores(ctx, genome_cases, plan, family):
    """A tie decided differently inside a warm-up is a reason for the verification to reject nodes; whatever it rejects, the
    result is the serial loop's.  The counts are printed, not asserted: ties may legitimately reject more than real scores do."""
    before, ref, ref_max = genome_cases[family]
    os.environ.update(SEG_PLANS[plan])
    same(run(ctx, before, 4.35), ref, ref_max, (plan, family))
    st = ctx.dp_stats()
    print(f"{plan} {family}: segments {st['segments']} rejected {st['rejected']} serial {st['serial']}")
    assert st["chains"] == 1


# ---- the training pass (final = 0) ----

@pytest.mark.parametrize("kernel", ["default", "wave"])
@pytest.mark.parametrize("name,closed", [("SRR492066", False), ("GCF_001457455.1_NCTC11397_genomic_100kb", True)])
def test_training_pass_on_tied_frame_scores(ctx, name, closed, kernel):
    os.environ.update(VARIANTS[kernel])
    seq = read_fasta(name + ".fna.gz")[0][1]
    ties = 0
    for family, bias in (("pm1", (1.0, 1.0, 1.0)), ("quant", (1.0, 1.0, 1.0)), ("pm1", (0.5, 1.0, 2.0)), ("quant", (0.5, 1.0, 2.0))):
        before, ref, ref_max, ev = dp_inject.inject_training(seq, family, bias, seed=1, closed=closed)
        assert ev["ties"] >= 100, (family, bias, ev)
        ties += ev["ties"]
        out = ctx.score_connections_training(before["ndx"], before["stop_val"], before["type"], before["strand"], before["gc_score"],
                                             np.array(bias), before["star_ptr"], 4.35)
        same(out, ref, ref_max, (name, family, bias))
    assert ties >= 1000
