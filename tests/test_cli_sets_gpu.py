"""python -m pyrodigal_amd --bin-map end to end on the GPU: one model per bin, against GeneFinder.find_genes_batch(..., sets=...) and
the host writers; several device calls packed from whole sets, output in file order."""
import io
import os
import subprocess
import sys

import pytest

from tests import sets_ref as sr
from tests.util import synthetic_contig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib as L
    return L


def records():
    seqs, labels = sr.case_interleaved()
    seqs = list(seqs) + [synthetic_contig(1500, 0.5, 4701), synthetic_contig(2600, 0.58, 4702)]
    labels = list(labels) + [None, "B"]
    return [("rec%d" % i, s) for i, s in enumerate(seqs)], labels


def test_bin_map_against_the_library_call(lib, tmp_path):
    recs, labels = records()
    fasta = tmp_path / "in.fna"
    with open(fasta, "wb") as f:
        for sid, s in recs:
            f.write(b">" + sid.encode() + b" a description\n")
            for k in range(0, len(s), 70):
                f.write(s[k:k + 70] + b"\n")
    bin_map = tmp_path / "bins.tsv"
    with open(bin_map, "w") as f:
        f.write("# contig\tbin\n")
        for (sid, _), lab in zip(recs, labels):
            if lab is not None:
                f.write("%s\tbin.%s\n" % (sid, lab))
        f.write("not_in_the_file\tbin.A\n")
    paths = []
    for i, b in enumerate(sr.meta_bins()):
        p = tmp_path / ("model_%02d.bin" % i)
        p.write_bytes(b.tobytes())
        paths.append(p)
    mbins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=p.read_bytes()), p.name) for p in paths])
    genes = lib.GeneFinder(meta=True, metagenomic_bins=mbins).find_genes_batch([s for _, s in recs], sets=labels)
    gff, faa, fna = io.StringIO(), io.StringIO(), io.StringIO()
    for (sid, _), g in zip(recs, genes):
        assert g.metagenomic_bin is not None
        g.write_gff(gff, sid)
        g.write_translations(faa, sid)
        g.write_genes(fna, sid)
    # the sets do not fit one device call: A (rec0, rec2, rec4) is larger than a call, the others share calls -- and the text is in
    # file order all the same, every record under its own seqnum
    for batch_bases in ("9000", str(64 << 20)):
        o, a, d = tmp_path / "o.gff", tmp_path / "a.faa", tmp_path / "d.fna"
        r = subprocess.run([sys.executable, "-m", "pyrodigal_amd", "-i", str(fasta), "-p", "meta", "--meta-bins", *map(str, paths),
                            "--bin-map", str(bin_map), "-o", str(o), "-a", str(a), "-d", str(d), "--batch-bases", batch_bases],
                           cwd=ROOT, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stderr.decode().count("Warning: --bin-map: no sequence 'not_in_the_file' in the input") == 1
        assert o.read_bytes() == gff.getvalue().encode()
        assert a.read_bytes() == faa.getvalue().encode()
        assert d.read_bytes() == fna.getvalue().encode()
    text = gff.getvalue()
    assert [text.index('seqhdr="rec%d"' % i) for i in range(len(recs))] == sorted(text.index('seqhdr="rec%d"' % i) for i in range(len(recs)))
    assert all('seqnum=%d;seqlen=%d;seqhdr="rec%d"' % (i + 1, len(s), i) in text for i, (_, s) in enumerate(recs))
    # without the map the records go their own ways
    r = subprocess.run([sys.executable, "-m", "pyrodigal_amd", "-i", str(fasta), "-p", "meta", "--meta-bins", *map(str, paths)],
                       cwd=ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0 and r.stdout != gff.getvalue().encode()
