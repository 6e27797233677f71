"""The command line (python -m pyrodigal_amd) without a GPU: option parsing, --help, and the exits it refuses with."""
import os
import subprocess
import sys

from pyrodigal_amd import cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(*argv):
    return subprocess.run([sys.executable, "-m", "pyrodigal_amd", *argv], cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_options_parse_like_the_reference():
    a = cli.argument_parser().parse_args(["-i", "x.fa", "-o", "o.gff", "-a", "p.faa", "-d", "n.fna", "-s", "s.txt", "-f", "gbk",
                                          "-p", "meta", "-g", "4", "-c", "-m", "-n", "-j", "3", "--min-gene", "120",
                                          "--min-edge-gene", "70", "--max-overlap", "50", "--no-stop-codon",
                                          "--meta-bins", "a.bin", "b.bin", "--batch-bases", "1000"])
    assert (a.i, a.o, a.a, a.d, a.s, a.f, a.p, a.g) == ("x.fa", "o.gff", "p.faa", "n.fna", "s.txt", "gbk", "meta", 4)
    assert a.c and a.m and a.n and a.no_stop_codon
    assert (a.jobs, a.min_gene, a.min_edge_gene, a.max_overlap, a.batch_bases) == (3, 120, 70, 50, 1000)
    assert a.meta_bins == ["a.bin", "b.bin"]
    d = cli.argument_parser().parse_args([])
    assert (d.f, d.p, d.g, d.min_gene, d.min_edge_gene, d.max_overlap, d.t, d.o) == ("gff", "single", 11, 90, 60, 60, None, None)


def test_help_without_the_hip_library():
    r = run("--help")
    assert r.returncode == 0
    for opt in ("-i", "-o", "-a", "-d", "-s", "-f", "-p", "-t", "-g", "-c", "-m", "-n", "-j", "--min-gene", "--min-edge-gene",
                "--max-overlap", "--no-stop-codon", "--meta-bins", "--batch-bases"):
        assert opt in r.stdout
    # parsing alone never loads the compiled modules
    code = ("import sys; from pyrodigal_amd import cli; cli.argument_parser().parse_args(['-i', 'x']); "
            "assert 'pyrodigal_amd.lib' not in sys.modules and 'pyrodigal_amd._cabi' not in sys.modules")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT, timeout=60).returncode == 0


def test_bad_choices_exit_nonzero():
    assert run("-p", "both", "-i", "x").returncode != 0
    assert run("-g", "7", "-i", "x").returncode != 0
    assert run("-f", "json", "-i", "x").returncode != 0


def test_meta_with_training_file_exits_nonzero(tmp_path):
    r = run("-p", "meta", "-t", str(tmp_path / "t.bin"), "--meta-bins", "a.bin", "-i", "x")
    assert r.returncode != 0
    assert "training file" in r.stderr


def test_meta_without_bins_exits_nonzero():
    r = run("-p", "meta", "-i", "x")
    assert r.returncode != 0
    assert "--meta-bins" in r.stderr
