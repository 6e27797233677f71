"""Circular contigs without a GPU: the cut rule in C (pga_circular_cut) against its numpy restatement, the rule on the CPU oracle
against the results recorded for the committed fixtures, the host writers, the command line's argument checks."""
import ctypes
import io
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pyrodigal_amd import _cabi, cli
from tests import circular_ref as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib as L
    return L


def c_cut(L, genes):
    b = np.ascontiguousarray([g[0] for g in genes], np.int32)
    e = np.ascontiguousarray([g[1] for g in genes], np.int32)
    return _cabi.load().pga_circular_cut(L, len(genes), ctypes.c_void_p(b.ctypes.data), ctypes.c_void_p(e.ctypes.data))


# ---------------------------------------------------------------------------------------------- step 2 of the rule

def test_cut_hand_cases():
    assert c_cut(100, []) == 50 and cref.cut_of([], 100) == 50                   # one gap [0, L)
    assert c_cut(100, [(1, 100)]) == 50 and cref.cut_of([(1, 100)], 100) == 50   # no gap at all
    assert c_cut(1, []) == 0 and c_cut(0, []) == 0 and c_cut(2, []) == 1 and c_cut(3, [(1, 3)]) == 1
    # gaps only at the ends: none has its middle in the middle half, so all gaps count and the wider one wins
    assert c_cut(1000, [(11, 970)]) == cref.cut_of([(11, 970)], 1000) == 985
    assert c_cut(1000, [(31, 990)]) == cref.cut_of([(31, 990)], 1000) == 15
    # ties in width: the one closer to L / 2, then the lower one
    genes = [(1, 300), (311, 480), (491, 520), (531, 1000)]                      # gaps [300,310) [480,490) [520,530)
    assert c_cut(1000, genes) == cref.cut_of(genes, 1000) == 485
    genes = [(1, 470), (481, 520), (531, 1000)]                                  # mids 475 and 525: 25 from the middle both
    assert c_cut(1000, genes) == cref.cut_of(genes, 1000) == 475
    # a wide gap outside the middle half loses to a narrow one inside
    genes = [(201, 500), (511, 1000)]
    assert c_cut(1000, genes) == cref.cut_of(genes, 1000) == 505
    # overlapping genes, either order, and genes that stick out of the contig are clipped
    genes = [(400, 900), (1, 450), (420, 430), (880, 1200)]
    assert c_cut(1000, genes) == 500
    assert c_cut(-1, []) < 0 and c_cut(10, [(1, 2)][:0]) == 5


@pytest.mark.parametrize("seed", range(6))
def test_cut_random_interval_sets(seed, lib):
    rng = np.random.default_rng(seed)
    for it in range(400):
        L = int(rng.choice([1, 2, 3, 4, 7, 10, 64, 100, 1000, 65537, 10 ** 6])) if it % 2 else int(rng.integers(1, 3000))
        kind = it % 5
        n = int(rng.integers(0, 12))
        if kind == 0 and n:                                  # equal gaps between equal genes: ties in width
            w = int(rng.integers(1, max(2, L // (2 * n) + 1)))
            b = np.arange(n) * 2 * w + 1 + int(rng.integers(0, w + 1))
            e = b + w - 1
            keep = e <= L
            b, e = b[keep], e[keep]
        elif kind == 1:                                      # gaps only at the ends
            lo, hi = sorted(int(x) for x in rng.integers(1, L + 1, 2))
            b, e = np.array([lo]), np.array([hi])
        elif kind == 2:                                      # everything covered, in overlapping pieces
            b = np.concatenate([[1], rng.integers(1, L + 1, n)])
            e = np.concatenate([[L], np.minimum(b[1:] + rng.integers(0, L, n), L)])
        else:                                                # anything, overlaps allowed
            b = rng.integers(1, L + 1, n)
            e = np.minimum(b + rng.integers(0, max(1, L // 3), n), L)
        genes = list(zip(b.tolist(), e.tolist()))
        want = cref.cut_of(genes, L)
        assert c_cut(L, genes) == want, (L, genes)
        assert lib.circular_cut(L, b, e) == want
        assert 0 <= want < max(L, 1)


# ---------------------------------------------------------------------------------------------- the rule on the oracle

def test_rule_on_the_oracle_reproduces_the_recorded_results():
    bins = cref.meta_bins()
    assert len(bins) == 13
    srr = cref.fixture("SRR492066")
    c = cref.Circular(srr, cref.single_model("SRR492066.training.bin.gz"), False)
    assert len(srr) == 79939 and len(c.linear) == 76 and c.linear[0] == (1, 177, -1) and c.linear[-1] == (79328, 79939, -1)
    assert len(c.genes) == 75 and c.genes[-1] == (79328, 80116, -1) and c.cut == 52426
    assert sorted(c.genes[:-1]) == sorted(c.linear[1:-1])
    c = cref.Circular(srr, bins, True)
    assert len(c.linear) == 79 and len(c.genes) == 78 and c.genes[-1] == (79328, 80116, -1)
    kk = cref.fixture("KK037166")
    c = cref.Circular(kk, bins, True)
    assert len(kk) == 20000 and len(c.linear) == 20 and c.linear[0] == (2, 169, -1)
    assert len(c.genes) == 20 and c.genes[-1] == (19933, 20169, -1) and c.cut == 11007
    assert cref.Circular(kk, bins, True, closed=True).cut == 11007 and cref.Circular(kk, bins, True, closed=True).genes == c.genes
    mi = cref.fixture("MIIJ01000039")
    c = cref.Circular(mi, bins, True)
    assert len(mi) == 869782 and len(c.linear) == 425 and c.linear[-1] == (869621, 869782, 1)
    assert len(c.genes) == 424 and max(e for _, e, _ in c.genes) <= len(mi)
    kb = cref.fixture("GCF_001457455.1_NCTC11397_genomic_100kb")
    c = cref.Circular(kb, cref.single_model("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz"), False)
    assert len(kb) == 100000 and len(c.linear) == 102 and len(c.genes) == 102
    planted, orf = cref.planted_orf()
    c = cref.Circular(planted, bins, True)
    assert len(planted) == 31230 and len(orf) == 1206
    assert c.linear[0] == (1, 606, 1) and c.linear[-1] == (30631, 31230, 1) and c.genes[-1] == (30631, 31836, 1)
    assert (planted + planted)[30630:31836].decode() == orf


def test_rule_on_the_closed_chromosome():
    seq = cref.fixture("GCF_001457455.1_NCTC11397_genomic")
    c = cref.Circular(seq, cref.single_model("GCF_001457455.1_NCTC11397_genomic.tinf_closed.bin.gz"), False)
    assert len(seq) == 2463666 and len(c.linear) == 2343 and c.linear[0] == (1, 1659, 1)
    assert len(c.genes) == 2343 and c.genes[-1] == (2463649, 2465325, 1)
    assert sorted(c.genes[:-1]) == sorted(c.linear[1:])
    srr = cref.fixture("SRR492066")
    single = cref.single_model("SRR492066.training.bin.gz")
    assert cref.Circular(srr, single, False, closed=True).cut == 52426
    assert cref.Circular(srr, single, False, closed=True).genes == cref.Circular(srr, single, False).genes


# ---------------------------------------------------------------------------------------------- host writers

def gene_record(contig, begin, end, strand, start_type=0):
    g = np.zeros(1, _cabi.GENE_DTYPE)
    g["contig"], g["begin"], g["end"], g["strand"], g["start_type"] = contig, begin, end, strand, start_type
    g["cscore"], g["sscore"], g["gc_cont"] = 12.5, 3.25, 0.5
    return g.tobytes()


def test_host_writers_across_the_origin(lib):
    orf = "ATG" + "GCTGAAAAACTG" * 5 + "TAA"                      # 66 bases
    filler = "ACGTTGCA" * 30
    seq = orf[40:] + filler + orf[:40]                            # the gene starts 40 bases before the record's end
    L = len(seq)
    tinf = lib.TrainingInfo(0.5)
    recs = gene_record(0, L - 39, L + 26, 1) + gene_record(0, 50, 139, -1)
    genes = lib._genes_from_records(seq, recs, tinf, 7, circular=True, cut=L // 2)
    assert genes.circular and genes.cut == L // 2 and len(genes) == 2
    g = genes[0]
    assert (g.begin, g.end) == (L - 39, L + 26) and g.sequence() == orf and g.translate() == "M" + "AEKL" * 5 + "*"
    rev = lib._genes_from_records(seq, gene_record(0, L - 39, L + 26, -1), tinf, 7, circular=True, cut=0)[0]
    comp = orf.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    assert rev.sequence() == comp
    out = io.StringIO()
    genes.write_gff(out, "plasmid")
    text = out.getvalue()
    assert '# Sequence Data: seqnum=7;seqlen=%d;seqhdr="plasmid";topology=circular\n' % L in text
    assert "\tCDS\t%d\t%d\t" % (L - 39, L + 26) in text
    out = io.StringIO()
    genes.write_genes(out, "plasmid")
    assert out.getvalue().split("\n")[0].startswith(">plasmid_1 # %d # %d # 1 # " % (L - 39, L + 26))
    assert "".join(out.getvalue().split(">")[1].split("\n")[1:]) == orf
    out = io.StringIO()
    genes.write_translations(out, "plasmid")
    assert "".join(out.getvalue().split(">")[1].split("\n")[1:]) == "M" + "AEKL" * 5 + "*"
    out = io.StringIO()
    genes.write_genbank(out, "plasmid")
    gb = out.getvalue()
    assert re.search(r"^LOCUS       plasmid +%d bp    DNA     circular BCT \d\d-[A-Z]{3}-\d\d$" % L, gb, re.M)
    assert "     CDS             join(%d..%d,1..26)\n" % (L - 39, L) in gb
    assert "     CDS             complement(50..139)\n" in gb
    out = io.StringIO()
    lib._genes_from_records(seq, gene_record(0, L - 39, L + 26, -1), tinf, 7, circular=True, cut=0).write_genbank(out, "plasmid")
    assert "     CDS             complement(join(%d..%d,1..26))\n" % (L - 39, L) in out.getvalue()
    with pytest.raises(ValueError, match="circular"):
        genes.write_scores(io.StringIO(), "plasmid")
    # a linear sequence is written as before
    lin = lib._genes_from_records(seq, gene_record(0, 50, 139, 1), tinf, 7)
    out = io.StringIO()
    lin.write_gff(out, "contig")
    assert 'seqhdr="contig"\n' in out.getvalue() and "topology" not in out.getvalue()
    out = io.StringIO()
    lin.write_genbank(out, "contig")
    assert "DNA     linear   BCT" in out.getvalue() and not lin.circular and lin.cut is None


# ---------------------------------------------------------------------------------------------- command line, bindings

def run(*argv):
    return subprocess.run([sys.executable, "-m", "pyrodigal_amd", *argv], cwd=ROOT, capture_output=True, text=True, timeout=120)


def test_command_line_options_and_checks(tmp_path):
    a = cli.argument_parser().parse_args(["-i", "x.fa", "--circular"])
    assert a.circular and a.circular_ids is None and not a.circular_from_header
    d = cli.argument_parser().parse_args([])
    assert not d.circular and d.circular_ids is None and not d.circular_from_header
    assert cli.circular_option(d) is None and cli.circular_option(a) is True
    for extra in (["--circular"], ["--circular-ids", "ids.txt"], ["--circular-from-header"]):
        r = run("-i", "x.fa", "-s", str(tmp_path / "s.txt"), *extra)
        assert r.returncode != 0 and "-s cannot be combined" in r.stderr
    r = run("--help")
    assert r.returncode == 0 and all(o in r.stdout for o in ("--circular", "--circular-ids", "--circular-from-header"))


def test_circular_ids_and_header_predicate(tmp_path):
    assert cli.parse_circular_ids(["plasmid1 extra words\n", "\n", "# a comment\n", b"chr2\r\n", "  chr3  \n"]) == {"plasmid1", "chr2", "chr3"}
    ids = tmp_path / "ids.txt"
    ids.write_text("p1\np2 circular plasmid\n")
    a = cli.argument_parser().parse_args(["--circular-ids", str(ids)])
    assert cli.circular_option(a) == {"p1", "p2"}
    from pyrodigal_amd import pipeline
    says = pipeline.header_says_circular
    assert says("x", "length=5 circular=true") and says("x", "Topology=Circular") and says("x", "[CIRCULAR=TRUE]")
    assert not says("x", "circular=false") and not says("x", "") and not says("x", None) and not says("circular=true", "linear")
    both = cli.circular_option(cli.argument_parser().parse_args(["--circular-ids", str(ids), "--circular-from-header"]))
    assert both("p1", "") and both("zz", "topology=circular") and not both("zz", "") and both.seen == {"p1"}
    seen = set()
    assert pipeline.circular_flags({"p1", "nobody"}, ["a", "p1"], ["", ""], seen) == [False, True] and seen == {"p1"}
    assert pipeline.circular_flags({"nobody"}, ["a", "p1"], ["", ""]) is None
    assert pipeline.circular_flags(True, ["a", "b"], ["", ""]) == [True, True]
    assert pipeline.circular_flags(None, ["a"], [""]) is None and pipeline.circular_flags(False, ["a"], [""]) is None
    assert pipeline.circular_flags(says, ["a", "b"], ["circular=true", "x"]) == [True, False]


def test_exports_and_header_agree():
    with open(os.path.join(ROOT, "include", "pyrodigal_amd.h")) as f:
        declared = set(re.findall(r"\b(pga_[a-z0-9_]+)\s*\(", f.read()))
    assert declared == set(_cabi.EXPORTS)
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in ("pga_batch_set_circular", "pga_circular_cuts", "pga_circular_cut"):
        assert name in _cabi.EXPORTS and getattr(L, name)
    # the structs the render and finder ABI tests pin did not move
    assert ctypes.sizeof(_cabi.Result) == 88 and ctypes.sizeof(_cabi.Gene) == 88 and ctypes.sizeof(_cabi.ContigResult) == 40
