"""Direct terminal repeats without a GPU: the rule in plain Python (tests/terminal_repeat_ref.py) on hand-made
strings, the command line's options, refusals and report writer, and the bindings."""
import ctypes
import io
import os
import re
import subprocess
import sys

import pytest

from pyrodigal_amd import _cabi, cli, pipeline
from tests import terminal_repeat_ref as tref
from tests.util import synthetic_contig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pga_batch_terminal_repeats", "pga_batch_trim_terminal_repeats", "pga_terminal_repeat_chunk")


# ---------------------------------------------------------------------------------------------- the rule

def slow_match(seq, min_length, max_length):
    """find_match, letter by letter."""
    L = len(seq)
    for r in range(min(max_length, L // 2), min_length - 1, -1):
        if all(tref.letters_match(seq[j], seq[L - r + j]) for j in range(r)):
            return r
    return 0


def test_letters():
    assert tref.letters_match(ord("A"), ord("a")) and tref.letters_match(ord("t"), ord("T")) and tref.letters_match(ord("g"), ord("g"))
    assert not tref.letters_match(ord("A"), ord("C"))
    for ch in b"NnRYxX-*.":
        assert not tref.letters_match(ch, ch)             # an unknown letter matches nothing, not even itself


def test_overlap_of_exactly_min_length_and_one_shorter():
    t = b"ACGGTCATTGCAGCTTAGGCATCAAGTCCGATTAGACCAGT" + synthetic_contig(82, 0.5, 9)
    assert tref.terminal_repeat(t + t[:20]) == (20, 20, t)
    s = t + t[:19]
    assert tref.terminal_repeat(s) == (0, 0, s)
    assert tref.terminal_repeat(s, min_length=19) == (19, 19, t)
    assert tref.terminal_repeat(t + t[:20], min_length=21) == (0, 0, t + t[:20])


def test_window_is_capped_by_half_the_length_and_by_max_length():
    t = synthetic_contig(60, 0.5, 1)
    assert tref.terminal_repeat(t + t) == (60, 60, t)                          # r == L / 2 is still inside the window
    s = (t * 3)[:150]                                                          # period 60: the overlaps are 90 (> L / 2 = 75) and 30
    assert tref.find_match(s) == 30 and tref.find_match(s[:149]) == 29 and tref.find_match(s[:139]) == 0
    t = synthetic_contig(400, 0.5, 2)
    s = t + t[:100]
    assert tref.find_match(s, 20, 100) == 100 and tref.find_match(s, 20, 99) == 0
    assert tref.terminal_repeat(b"ACGT" * 9) == (0, 0, b"ACGT" * 9)            # L / 2 = 18 < min_length: nothing is searched
    assert tref.terminal_repeat(b"") == (0, 0, b"") and tref.terminal_repeat(b"A", 1, 1, 100) == (0, 0, b"A")
    assert tref.terminal_repeat(b"AA", 1, 1, 100) == (1, 1, b"A")


def test_unknown_letters_and_case():
    t = synthetic_contig(300, 0.5, 3)
    s = bytearray(t + t[:40])
    for pos in (0, 17, 39, 300, 317, 339):
        n = bytes(s[:pos]) + b"N" + bytes(s[pos + 1:])
        assert tref.find_match(n) == 0 and slow_match(n, 20, 65536) == 0, pos
    both = bytearray(s)
    both[5] = both[305] = ord("N")                                             # N against N: no match either
    assert tref.find_match(bytes(both)) == 0
    assert tref.terminal_repeat(t + t[:40].lower()) == (40, 40, t)
    assert tref.terminal_repeat(t.lower() + t[:40]) == (40, 40, t.lower())


def test_the_longest_match_wins_on_a_periodic_end():
    unit = b"ACGGTCA"
    t = unit * 8 + synthetic_contig(500, 0.5, 4)
    s = t + unit * 5                                                           # 35 planted, but the record starts with 56 periodic bases
    assert tref.find_match(s) == 35
    s = t + unit * 8
    assert tref.find_match(s) == 56
    s = synthetic_contig(7, 0.5, 5) * 40                                       # periodic throughout: the longest multiple inside L / 2
    assert tref.find_match(s) == 140 - 140 % 7 and slow_match(s, 20, 65536) == 140
    for seed in range(20):                                                     # the fast search is the letter-by-letter one
        s = synthetic_contig(3, 0.5, seed) * 30 + synthetic_contig(int(seed), 0.5, 50 + seed) + synthetic_contig(3, 0.5, seed) * 15
        assert tref.find_match(s, 5, 40) == slow_match(s, 5, 40)


def test_percent_rule_at_equality_is_kept():
    rep = b"AAAC" * 10                                                         # 30 of 40 bases are A: 100 * 30 == 75 * 40
    mid = synthetic_contig(300, 0.5, 6)
    mid = b"G" + mid[1:-1] + b"T"                                              # (no longer match by accident)
    s = rep + mid + rep
    assert tref.terminal_repeat(s) == (40, 40, rep + mid)
    assert tref.terminal_repeat(s, max_base_percent=74) == (40, 0, s)
    rep = b"AAAAC" * 8                                                         # 32 of 40
    s = rep + mid + rep
    assert tref.terminal_repeat(s) == (40, 0, s)                               # found, filtered: a shorter match is not tried
    assert tref.terminal_repeat(s, max_base_percent=80) == (40, 40, rep + mid)
    poly = b"a" * 50
    assert tref.terminal_repeat(poly + mid + poly.upper()) == (50, 0, poly + mid + poly.upper())
    assert tref.terminal_repeat(poly + mid + poly, max_base_percent=100)[:2] == (50, 50)      # 100: the filter is off
    for bad in ((0, 10, 75), (11, 10, 75), (20, 1048577, 75), (20, 65536, 24), (20, 65536, 101)):
        with pytest.raises(ValueError):
            tref.terminal_repeat(s, *bad)


def test_regions_and_status():
    assert tref.clip_regions([(0, 10), (90, 120), (100, 130), (95, 100)], 100) == [(0, 10), (90, 100), (95, 100)]
    assert [tref.status(m, t) for m, t in ((0, 0), (40, 0), (40, 40))] == ["none", "low_complexity", "trimmed"]
    assert [pipeline.terminal_repeat_status(m, t) for m, t in ((0, 0), (40, 0), (40, 40))] == ["none", "low_complexity", "trimmed"]


# ---------------------------------------------------------------------------------------------- command line

def run(*argv):
    return subprocess.run([sys.executable, "-m", "pyrodigal_amd", *argv], cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_command_line_refusals(tmp_path):
    r = run("-i", "x.fa", "-s", str(tmp_path / "s.txt"), "--circular-detect")
    assert r.returncode != 0 and "-s cannot be combined" in r.stderr and "--circular-detect" in r.stderr
    r = run("-i", "x.fa", "-p", "meta", "--meta-bins", "a.bin", "--bin-map", "bins.tsv", "--circular-detect")
    assert r.returncode != 0 and "--bin-map cannot be combined" in r.stderr and "--circular-detect" in r.stderr
    r = run("-i", "x.fa", "--circular-report", str(tmp_path / "r.tsv"))
    assert r.returncode != 0 and "--circular-report needs --circular-detect" in r.stderr
    for bad in (["--min-repeat", "0"], ["--min-repeat", "30", "--max-repeat", "29"], ["--max-repeat", "1048577"]):
        r = run("-i", "x.fa", "--circular-detect", *bad)
        assert r.returncode != 0 and "--min-repeat" in r.stderr
    assert not os.path.exists(tmp_path / "s.txt") and not os.path.exists(tmp_path / "r.tsv")


def test_command_line_options():
    d = cli.argument_parser().parse_args([])
    assert not d.circular_detect and d.min_repeat == 20 and d.max_repeat == 65536 and d.circular_report is None
    assert cli.terminal_repeat_option(d) is None
    a = cli.argument_parser().parse_args(["--circular-detect"])
    opt = cli.terminal_repeat_option(a)
    assert (opt.min_length, opt.max_length, opt.max_base_percent) == (20, 65536, 75)
    a = cli.argument_parser().parse_args(["--circular-detect", "--min-repeat", "50", "--max-repeat", "2000", "--circular-report", "r.tsv",
                                          "--circular-from-header"])
    opt = cli.terminal_repeat_option(a)
    assert (opt.min_length, opt.max_length, opt.max_base_percent) == (50, 2000, 75) and a.circular_report == "r.tsv"
    assert a.circular_from_header and cli.circular_option(a) is pipeline.header_says_circular      # the options combine
    search, params = _cabi.terminal_repeat_options(3, opt)
    assert search.tolist() == [1, 1, 1] and params == (50, 2000, 75)
    r = run("--help")
    assert r.returncode == 0 and all(o in r.stdout for o in ("--circular-detect", "--min-repeat", "--max-repeat", "--circular-report"))


def test_option_forms_of_the_bindings():
    opts = _cabi.terminal_repeat_options
    assert opts(4, None) is None and opts(4, False) is None and opts(4, [False, None, False, False]) is None
    search, params = opts(2, True)
    assert search.tolist() == [1, 1] and params == (20, 65536, 75)
    shared = cli.TerminalRepeatOption(30, 40, 100)
    search, params = opts(4, [True, False, shared, shared])
    assert search.tolist() == [1, 0, 1, 1] and params == (30, 40, 100)
    with pytest.raises(ValueError, match="3 entries for 4"):
        opts(4, [True] * 3)
    with pytest.raises(ValueError, match="two different"):
        opts(2, [cli.TerminalRepeatOption(30, 40, 100), cli.TerminalRepeatOption(31, 40, 100)])
    with pytest.raises(TypeError):
        opts(2, [True, "yes"])


def test_report_writer():
    records = [("contig_1", 20127, 127, 127), ("polyA tail", 5060, 60, 0), ("linear", 300, 0, 0), ("", 0, 0, 0)]
    out = io.StringIO()
    cli.write_circular_report(out, records)
    assert out.getvalue() == ("contig_1\t20127\t127\t127\ttrimmed\n"
                              "polyA tail\t5060\t60\t0\tlow_complexity\n"
                              "linear\t300\t0\t0\tnone\n"
                              "\t0\t0\t0\tnone\n")
    out = io.StringIO()
    cli.write_circular_report(out, [])
    assert out.getvalue() == ""


# ---------------------------------------------------------------------------------------------- bindings

def test_new_names_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "pyrodigal_amd.h")) as f:
        declared = set(re.findall(r"\b(pga_[a-z0-9_]+)\s*\(", f.read()))
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in NEW:
        assert re.fullmatch(r"pga_[a-z_]+", name)
        assert name in declared and name in _cabi.EXPORTS and getattr(L, name)
    with open(os.path.join(ROOT, "pyrodigal_amd", "lib.pyx")) as f:
        pyx = f.read()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        doc = f.read()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, pyx) and "`%s`" % name in doc
    chunk = _cabi.load().pga_terminal_repeat_chunk()
    assert chunk >= 64 and chunk % 4 == 0


def test_python_names():
    import pyrodigal_amd
    from pyrodigal_amd import lib
    assert "TerminalRepeats" in pyrodigal_amd.__all__ and pyrodigal_amd.TerminalRepeats is lib.TerminalRepeats
    t = lib.TerminalRepeats()
    assert (t.min_length, t.max_length, t.max_base_percent) == (20, 65536, 75)
    assert lib.TerminalRepeats(30, 40, 100) == lib.TerminalRepeats(30, 40, 100) != lib.TerminalRepeats(30, 41, 100)
    for bad in ((0, 10, 75), (11, 10, 75), (20, 1048577, 75), (20, 100, 24), (20, 100, 101)):
        with pytest.raises(ValueError):
            lib.TerminalRepeats(*bad)
    assert _cabi.terminal_repeat_options(2, lib.TerminalRepeats(30, 40, 100))[1] == (30, 40, 100)
    for f in (_cabi.Batch.terminal_repeats, _cabi.Batch.trim_terminal_repeats):
        assert callable(f)
