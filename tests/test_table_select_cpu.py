"""Translation-table choice by coding density, without a GPU: the rule of pyrodigal_amd.tables on hand-made densities, the
argument checks of select_translation_table / translation_table="auto" that fail before any device call, and -g auto."""
import subprocess
import sys
import os

import pytest

from pyrodigal_amd import tables
from pyrodigal_amd.tables import choose_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# densities that are exact binary fractions, so that differences land exactly on the thresholds
D11, D4 = 0.625, 0.75        # gain 0.125


def test_defaults_are_the_usual_test():
    assert tables.DEFAULT_CANDIDATES == (11, 4)
    assert tables.DEFAULT_MIN_GAIN == 0.05 and tables.DEFAULT_MIN_DENSITY == 0.7
    assert choose_table({11: 0.80, 4: 0.90}) == 4
    assert choose_table({11: 0.88, 4: 0.90}) == 11          # too little gain
    assert choose_table({11: 0.50, 4: 0.65}) == 11          # gain, but not dense enough
    assert choose_table({11: 0.90, 4: 0.10}) == 11


def test_min_gain_is_strict():
    assert choose_table({11: D11, 4: D4}, min_gain=0.125, min_density=0.5) == 11     # exactly min_gain: not more
    assert choose_table({11: D11, 4: D4}, min_gain=0.0625, min_density=0.5) == 4
    assert choose_table({11: D11, 4: D11}, min_gain=0.0, min_density=0.0) == 11      # no gain at all


def test_min_density_is_strict():
    assert choose_table({11: D11, 4: D4}, min_gain=0.0625, min_density=0.75) == 11   # exactly min_density: not more
    assert choose_table({11: D11, 4: D4}, min_gain=0.0625, min_density=0.6875) == 4
    assert choose_table({11: 0.25, 4: 1.0}, min_gain=1.0, min_density=0.0) == 11       # thresholds at the ends of [0, 1]
    assert choose_table({11: 0.0, 4: 1.0}, min_gain=0.5, min_density=1.0) == 11


def test_ties_go_to_the_candidate_listed_first():
    d = {11: 0.5, 4: 0.875, 25: 0.875}
    assert choose_table(d, (11, 4, 25)) == 4
    assert choose_table(d, (11, 25, 4)) == 25


def test_three_and_four_candidates():
    d = {11: 0.5, 4: 0.75, 25: 0.875, 1: 0.8125}
    assert choose_table(d, (11, 4, 25)) == 25
    assert choose_table(d, (11, 4, 25, 1)) == 25
    assert choose_table(d, (11, 4, 1)) == 1
    assert choose_table(d, (11, 4, 25, 1), min_density=0.875) == 11        # nobody above 0.875
    assert choose_table(d, (11, 4, 25, 1), min_density=0.8125) == 25
    # the default is the first candidate, whatever its number
    assert choose_table(d, (25, 11, 4, 1)) == 25
    assert choose_table(d, (4, 11, 25)) == 25
    assert choose_table(d, (4, 11, 25), min_gain=0.125) == 4                # 0.875 - 0.75 is exactly 0.125


def test_single_candidate():
    assert choose_table({4: 0.1}, (4,)) == 4
    assert choose_table({11: 0.99}, (11,)) == 11


def test_candidate_and_threshold_checks():
    assert tables.check_candidates([11, 4]) == (11, 4)
    for bad in ((), (11, 11), (11, 4, 1, 2, 3), (7,), (11, 0), ("11",), (11.0,), (True,), "11", 11):
        with pytest.raises(ValueError):
            tables.check_candidates(bad)
    for g, d in ((-0.01, 0.7), (1.5, 0.7), (0.05, -1), (0.05, 1.0001), (float("nan"), 0.7)):
        with pytest.raises(ValueError):
            tables.check_thresholds(g, d)
    assert tables.check_thresholds(0, 1) == (0.0, 1.0)


def test_density_is_one_double_division():
    assert tables.coding_density(2_000_001, 2_463_666) == 2_000_001 / 2_463_666
    assert tables.coding_density(1, 3) == 1.0 / 3.0


def test_selection_result_is_read_only():
    s = tables.TableSelection(4, None, {11: 600, 4: 900}, 1000)
    assert s.translation_table == 4 and s.length == 1000
    assert dict(s.coding_bases) == {11: 600, 4: 900}
    assert s.coding_density[4] == 0.9 and s.coding_density[11] == 0.6
    with pytest.raises(AttributeError):
        s.translation_table = 11
    with pytest.raises(TypeError):
        s.coding_density[4] = 0.0
    import pyrodigal_amd
    assert pyrodigal_amd.TableSelection is tables.TableSelection


@pytest.fixture(scope="module")
def lib():
    try:
        from pyrodigal_amd import lib as L
    except ImportError:
        import __graft_entry__
        __graft_entry__.build_cython_host()
        from pyrodigal_amd import lib as L
    return L


def test_select_argument_errors_before_any_device_call(lib):
    genome = "ATG" * 10_000
    f = lib.GeneFinder()
    for kw in ({"candidates": ()}, {"candidates": (11, 11)}, {"candidates": (11, 7)}, {"candidates": (11, 4, 1, 2, 3)},
               {"min_gain": 1.5}, {"min_gain": -0.1}, {"min_density": 2.0}, {"min_density": -1e-9}):
        with pytest.raises(ValueError):
            f.select_translation_table([genome], **kw)
    with pytest.raises(ValueError):
        f.select_translation_table(["ACGT" * 100])                 # shorter than MIN_SINGLE_GENOME
    with pytest.raises(RuntimeError):
        lib.GeneFinder(meta=True).select_translation_table([genome])
    assert f.select_translation_table([]) == []


def test_auto_argument_errors_before_any_device_call(lib):
    f = lib.GeneFinder()
    for bad in ("Auto", "11", "", 7):
        with pytest.raises(ValueError):
            f.train("ATG" * 10_000, translation_table=bad)
        with pytest.raises(ValueError):
            f.train_batch(["ATG" * 10_000], translation_table=bad)
    with pytest.raises(ValueError):
        f.train("ACGT" * 100, translation_table="auto")
    with pytest.raises(ValueError):
        f.train_batch(["ACGT" * 100], translation_table="auto")
    with pytest.raises(ValueError):
        f.train_batch(["ATG" * 10_000, "ATG" * 10_000], translation_table=["auto", 7])
    with pytest.raises(RuntimeError):
        lib.GeneFinder(meta=True).train("ATG" * 10_000, translation_table="auto")
    assert f.training_info is None


def test_cli_accepts_auto_and_refuses_bad_tables():
    from pyrodigal_amd.cli import argument_parser
    p = argument_parser()
    assert p.parse_args(["-g", "auto"]).g == "auto"
    assert p.parse_args(["-g", "4"]).g == 4
    assert p.parse_args([]).g == 11
    for bad in ("7", "AUTO", "x"):
        r = subprocess.run([sys.executable, "-m", "pyrodigal_amd", "-g", bad, "-i", "x"], cwd=ROOT, capture_output=True, timeout=120)
        assert r.returncode != 0
