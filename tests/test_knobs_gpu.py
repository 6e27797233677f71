"""The run-time knobs are read once per call (pyrodigal_amd/csrc/knobs.h): in one process, on one context, a knob that is set between
two calls takes effect in the next call and stops taking effect when it is unset again -- and the results never move."""
import os

import numpy as np
import pytest

from tests.util import synthetic_contig

pytestmark = pytest.mark.gpu

KNOBS = ("PGA_STAGE_SHIFT", "PGA_STAGE_FULL", "PGA_DP_SEG", "PGA_DP_SEG_MIN", "PGA_DP_SEG_LEN", "PGA_DP_KERNEL", "PGA_SS_MM", "PGA_SS_STARTS_ONLY")


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi, benchdata
    c = _cabi.Context(0)
    c.set_models([blob for _, blob in benchdata.load_model_set()])
    yield c
    c.close()


@pytest.fixture(autouse=True)
def clean_env():
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    yield
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def unset_set_unset(ctx, seqs, name, value, observe):
    """three calls -- the knob unset, set, unset again; returns what `observe` saw after each, having checked that the results are the same"""
    runs, seen = [], []
    for setting in (None, value, None):
        if setting is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = setting
        runs.append(ctx.find_genes_batch(seqs, meta=True))
        seen.append(observe())
    assert len(runs[0].genes) > 10
    for r in runs[1:]:
        assert r.genes.tobytes() == runs[0].genes.tobytes(), name
        assert np.array_equal(r.contigs["model"], runs[0].contigs["model"]), name
        assert np.array_equal(r.contigs["score"].view(np.uint64), runs[0].contigs["score"].view(np.uint64)), name
    return seen


# (forty extraction tiles of ordinary sequence, a node every 25 positions or so: one staging slot per 32 positions cannot hold them)
SHORT = [synthetic_contig(20_000 + 700 * c, 0.33 + 0.06 * c, 52_000 + c) for c in range(6)]


def test_stage_shift_moves_the_extraction_passes_and_back(ctx):
    assert unset_set_unset(ctx, SHORT, "PGA_STAGE_SHIFT", "5", lambda: ctx.extract_stats()["passes"]) == [1, 2, 1]


def test_ss_mm_changes_no_result(ctx):
    unset_set_unset(ctx, SHORT, "PGA_SS_MM", "0", lambda: None)


def test_dp_seg_moves_the_segments_and_back(ctx):
    os.environ["PGA_DP_SEG_MIN"] = "256"         # a contig of a few thousand nodes is cut (as tests/test_dp_segments_gpu.py forces the path)
    seen = unset_set_unset(ctx, [synthetic_contig(100_000, 0.5, 52_100)], "PGA_DP_SEG", "0", lambda: ctx.dp_stats()["segments"])
    assert seen[0] > 0 and seen[1] == 0 and seen[2] == seen[0]
