"""Region masks without a GPU: the `Masks` / `Mask` classes, pickling of the new fields, interval validation, the BED-like
parser of --mask-regions, the command line's argument checks, the boundary (header and binding agree), and the FASTA reader
handing the case of the letters through."""
import copy
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest

from pyrodigal_amd import cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib as L
    return L


def test_mask_intersects_like_the_reference(lib):
    """ref: lib.pyx:344-365, the four cases of the docstring."""
    mask = lib.Mask(3, 5)
    assert mask.intersects(2, 5) is True
    assert mask.intersects(1, 4) is True
    assert mask.intersects(1, 3) is False       # range end is exclusive
    assert mask.intersects(5, 7) is False       # mask end is exclusive
    assert mask.intersects(3, 4) and mask.intersects(4, 5) and not mask.intersects(0, 3)


def test_masks_is_a_container_of_masks(lib):
    import pyrodigal_amd
    assert pyrodigal_amd.Masks is lib.Masks and "Masks" in pyrodigal_amd.__all__
    m = lib.Masks([(1, 2), lib.Mask(5, 9), [20, 30]])
    assert len(m) == 3 and bool(m)
    assert isinstance(m[0], lib.Mask) and (m[0].begin, m[0].end) == (1, 2) and (m[-1].begin, m[-1].end) == (20, 30)
    with pytest.raises(IndexError):
        m[3]
    with pytest.raises(IndexError):
        m[-4]
    assert [(x.begin, x.end) for x in m] == [(1, 2), (5, 9), (20, 30)]
    assert m == [(1, 2), (5, 9), (20, 30)] and m == [lib.Mask(1, 2), lib.Mask(5, 9), lib.Mask(20, 30)]
    assert m == lib.Masks(m) and m != [(1, 2)] and m != [(1, 2), (5, 9), (20, 31)] and not (m == 7)
    assert lib.Masks() == [] and [] == lib.Masks() and not lib.Masks() and len(lib.Masks()) == 0
    assert m[1:] == [(5, 9), (20, 30)] and isinstance(m[1:], lib.Masks)
    assert m.intersects(8, 12) and not m.intersects(9, 20)
    c = m.copy()
    assert c == m and c is not m and copy.copy(m) == m
    c.clear()
    assert c == [] and len(m) == 3
    assert pickle.loads(pickle.dumps(m)) == m and isinstance(pickle.loads(pickle.dumps(m)), lib.Masks)
    assert "Masks" in repr(m) and "(5, 9)" in repr(m)
    with pytest.raises((TypeError, ValueError)):
        lib.Masks([(1, 2, 3)])


def test_sequence_and_finder_pickle_the_new_fields(lib):
    s = lib.Sequence("ACGTacgtACGT", mask=True, mask_size=7, regions=[(8, 10), lib.Mask(1, 3)], mask_lowercase=True)
    assert s.regions == [(8, 10), (1, 3)] and s.mask_lowercase and s.mask and s.mask_size == 7
    t = pickle.loads(pickle.dumps(s))
    assert (t.data, t.mask, t.mask_size, t.mask_lowercase) == (s.data, True, 7, True) and t.regions == s.regions
    plain = lib.Sequence("ACGT")
    assert plain.regions is None and not plain.mask_lowercase
    assert plain.__reduce__() == (lib.Sequence, (b"ACGT", False, 50))          # as before the new fields
    assert lib.Sequence(s).regions == s.regions                                 # re-wrapping keeps the regions
    assert lib.Sequence("ACGT", regions=[]).regions is None
    f = lib.GeneFinder(meta=True, mask_lowercase=True, min_mask=20)
    g = pickle.loads(pickle.dumps(f))
    assert g.mask_lowercase and g.min_mask == 20 and "mask_lowercase=True" in repr(f)
    d = lib.GeneFinder(meta=True)
    assert not d.mask_lowercase and "mask_lowercase" not in repr(d) and "mask_lowercase" not in d.__reduce__()[1][1]
    assert not pickle.loads(pickle.dumps(d)).mask_lowercase


@pytest.mark.parametrize("bad", [(4, 4), (-1, 3), (2, 13), (9, 3), (12, 13)])
def test_an_interval_outside_its_sequence_is_refused_with_its_name(lib, bad):
    with pytest.raises(ValueError, match=re.escape("[%d, %d)" % bad)):
        lib.Sequence("ACGTACGTACGT", regions=[(0, 12), bad])
    finder = lib.GeneFinder(meta=True)
    # the host layer checks before anything goes to the device, and names the sequence of a batch
    with pytest.raises(ValueError, match=r"sequence 1: region \[%d, %d\)" % bad):
        finder.find_genes_batch(["ACGTACGTACGT", "ACGTACGTACGT"], regions=[None, [bad]])
    with pytest.raises(ValueError, match=re.escape("[%d, %d)" % bad)):
        finder.find_genes("ACGTACGTACGT", regions=[bad])
    with pytest.raises(ValueError, match="entries for 2 sequences"):
        finder.find_genes_batch(["ACGT", "ACGT"], regions=[None])


def test_regions_for_the_binding_are_packed_per_sequence():
    from pyrodigal_amd import _cabi, lib
    off, iv = _cabi.pack_regions([None, [(5, 9), lib.Mask(1, 2)], [], np.array([[7, 8]])], 4)
    assert off.tolist() == [0, 0, 2, 2, 3] and iv.reshape(-1, 2).tolist() == [[5, 9], [1, 2], [7, 8]]
    assert off.dtype == np.int32 and iv.dtype == np.int32
    assert _cabi.pack_regions(None, 3) is None and _cabi.pack_regions([None, []], 2) is None
    with pytest.raises(ValueError, match="2 entries for 3 sequences"):
        _cabi.pack_regions([None, None], 3)


def test_bed_parser():
    text = ["# a comment\n", "track name=features\n", "browser position x\n", "\n",
            "contig_1\t10\t20\n", "contig_1\t5\t7\tname\t0\t+\n", "contig 2\t0\t1\r\n", b"contig_1\t100\t200\n"]
    assert cli.parse_mask_regions(text) == {"contig_1": [(10, 20), (5, 7), (100, 200)], "contig 2": [(0, 1)]}
    assert cli.parse_mask_regions([]) == {}
    for no, bad in ((1, "contig_1 10 20\n"), (2, "contig_1\t10\n"), (2, "contig_1\tten\t20\n"), (3, "contig_1\t20\t10\n"),
                    (1, "contig_1\t-1\t10\n"), (1, "\t1\t2\n"), (4, "contig_1\t5\t5\n")):
        lines = ["#\n"] * (no - 1) + [bad]
        with pytest.raises(ValueError, match=r"regions\.bed, line %d:" % no):
            cli.parse_mask_regions(lines, "regions.bed")


def test_command_line_checks_its_mask_arguments(tmp_path):
    a = cli.argument_parser().parse_args(["-i", "x.fa", "--mask-lowercase", "--mask-regions", "r.bed"])
    assert a.mask_lowercase and a.mask_regions == "r.bed"
    d = cli.argument_parser().parse_args([])
    assert not d.mask_lowercase and d.mask_regions is None

    def run(*argv):
        return subprocess.run([sys.executable, "-m", "pyrodigal_amd", *argv], cwd=ROOT, capture_output=True, text=True, timeout=120)
    r = run("--help")
    assert r.returncode == 0 and "--mask-lowercase" in r.stdout and "--mask-regions" in r.stdout
    bed = tmp_path / "bad.bed"
    bed.write_text("seq\t1\t5\nseq\tfive\t9\n")
    r = run("-i", "x.fa", "--mask-regions", str(bed))
    assert r.returncode != 0 and "line 2" in r.stderr and "--mask-regions" in r.stderr
    r = run("-i", "x.fa", "--mask-regions", str(tmp_path / "missing.bed"))
    assert r.returncode != 0 and "--mask-regions" in r.stderr
    r = run("-i", "x.fa", "--mask-regions")
    assert r.returncode != 0


def test_header_and_binding_agree_on_the_new_exports():
    from pyrodigal_amd import _cabi
    text = open(os.path.join(ROOT, "include", "pyrodigal_amd.h")).read()
    for name in ("pga_batch_set_regions", "pga_batch_set_mask_case"):
        assert name in _cabi.EXPORTS and re.search(r"\bint\s+%s\s*\(" % name, text)


def test_the_fasta_reader_hands_the_case_through(tmp_path):
    """tests/golden/fasta/* hold no lower-case letter, so the reader's treatment of case is pinned here: soft-masked input must
    reach the device as it was written."""
    import gzip
    from pyrodigal_amd import _cabi
    recs = [("soft", "ACGTacgtnnNNacgtACGT" * 9), ("upper", "ACGT" * 40), ("lower", "acgtn" * 33)]
    plain, packed = tmp_path / "in.fa", tmp_path / "in.fa.gz"
    body = "".join(">%s desc\n%s\n" % (i, "\n".join(s[k:k + 60] for k in range(0, len(s), 60))) for i, s in recs)
    plain.write_text(body)
    with gzip.open(packed, "wt") as f:
        f.write(body)
    for path in (plain, packed):
        with _cabi.FastaReader(str(path)) as r:
            got = [(i, s.decode()) for batch in r.batches() for i, _, s in batch]
        assert got == recs
