"""python -m pyrodigal_amd end to end on the GPU: a multi-record .gz file in several batches, each output byte for byte what a
Python loop over GeneFinder.find_genes and the Genes.write_* writers produces."""
import gzip
import io
import os
import subprocess
import sys
import warnings

import pytest

from pyrodigal_amd import benchdata
from tests.util import golden_path, read_fasta, synthetic_contig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib as L
    return L


@pytest.fixture(scope="module")
def records():
    recs = [(h.split()[0], s) for h, s in read_fasta("SRR492066.fna.gz")]
    recs += [("syn_%d" % i, synthetic_contig(n, gc, 40 + i).decode()) for i, (n, gc) in
             enumerate([(70_000, 0.45), (5_000, 0.55), (120_000, 0.35), (300, 0.5), (40_000, 0.6)])]
    recs += [(h.split()[0], s) for h, s in read_fasta("KK037166.fna.gz")]
    return recs


def write_fasta(path, records):
    with gzip.open(path, "wt") as f:
        for i, (sid, s) in enumerate(records):
            f.write(">%s description %d\n" % (sid, i))
            for k in range(0, len(s), 80):
                f.write(s[k:k + 80] + "\n")
    return str(path)


@pytest.fixture(scope="module")
def fasta(records, tmp_path_factory):
    return write_fasta(tmp_path_factory.mktemp("cli") / "input.fna.gz", records)


def cli(*argv):
    r = subprocess.run([sys.executable, "-m", "pyrodigal_amd", *argv, "--batch-bases", "150000"], cwd=ROOT, capture_output=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    return r


def host(finder, records, gbk=False, scores=False, include_stop=True):
    out, faa, fna, sc = io.StringIO(), io.StringIO(), io.StringIO(), io.StringIO()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for sid, s in records:
            g = finder.find_genes(s)
            if gbk:
                g.write_genbank(out, sid)
            else:
                g.write_gff(out, sid)
            g.write_translations(faa, sid, include_stop=include_stop)
            g.write_genes(fna, sid)
            if scores:
                g.write_scores(sc, sid)
    return out.getvalue().encode(), faa.getvalue().encode(), fna.getvalue().encode(), sc.getvalue().encode()


def outputs(tmp_path, *extra):
    o, a, d = tmp_path / "o", tmp_path / "a.faa", tmp_path / "d.fna"
    cli("-o", str(o), "-a", str(a), "-d", str(d), *extra)
    return o.read_bytes(), a.read_bytes(), d.read_bytes()


def test_single_training_and_training_file(lib, records, fasta, tmp_path):
    t = tmp_path / "model.bin"
    got = outputs(tmp_path, "-i", fasta, "-t", str(t), "--no-stop-codon")          # -t names a missing file: train, write it
    finder = lib.GeneFinder()
    tinf = finder.train(*[s for _, s in records])
    assert t.read_bytes() == bytes(tinf.raw)
    want = host(lib.GeneFinder(tinf), records, include_stop=False)
    assert got == want[:3]
    got2 = outputs(tmp_path, "-i", fasta, "-t", str(t), "--no-stop-codon", "-j", "1")   # -t names an existing file: read it
    assert got2 == want[:3]
    # no -t: train on all records, write to stdout
    r = cli("-i", fasta)
    assert r.stdout == host(lib.GeneFinder(tinf), records)[0]


def unbinned_header(genes, sid, b):
    """What Prodigal writes for a meta-mode contig without genes: the GFF header lines, with bin 5's model data."""
    t = b.training_info
    return ('##gff-version  3\n# Sequence Data: seqnum=%d;seqlen=%d;seqhdr="%s"\n# Model Data: version=pyrodigal_amd.v%s;'
            'run_type=Metagenomic;model="%s";gc_cont=%.2f;transl_table=%d;uses_sd=%d\n'
            % (genes._num_seq, len(genes.sequence), sid, lib_version(), b.description, t.gc * 100, t.translation_table, int(t.uses_sd)))


def lib_version():
    from pyrodigal_amd import __version__
    return __version__


def test_meta_bins(lib, records, tmp_path):
    # short and gene-less records among the others: no bin wins them, their GFF is the header with bin 5's data
    records = records[:2] + [("tiny", "ACGTTGCA" * 8 + "A"), ("no_genes", "ATGAAATAA" * 500)] + records[2:]
    fasta = write_fasta(tmp_path / "meta.fna.gz", records)
    paths = []
    for name, blob in benchdata.load_model_set():
        p = tmp_path / name.replace(".gz", "")
        p.write_bytes(blob)
        paths.append(p)
    got = outputs(tmp_path, "-i", fasta, "-p", "meta", "--meta-bins", *map(str, paths))
    bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=p.read_bytes()), p.name) for p in paths])
    finder = lib.GeneFinder(meta=True, metagenomic_bins=bins)
    gff, faa, fna = io.StringIO(), io.StringIO(), io.StringIO()
    unbinned = 0
    for sid, s in records:
        g = finder.find_genes(s)
        if g.metagenomic_bin is None:
            assert len(g) == 0
            unbinned += 1
            gff.write(unbinned_header(g, sid, bins[5]))
        else:
            g.write_gff(gff, sid)
        g.write_translations(faa, sid)
        g.write_genes(fna, sid)
    assert unbinned >= 1
    assert got == (gff.getvalue().encode(), faa.getvalue().encode(), fna.getvalue().encode())


def test_genbank_and_scores_through_the_host_writers(lib, records, fasta, tmp_path):
    tinf = lib.TrainingInfo.load(golden_path("SRR492066.training.bin.gz"))
    t = tmp_path / "m.bin"
    with open(t, "wb") as f:
        tinf.dump(f)
    s = tmp_path / "s.txt"
    got = outputs(tmp_path, "-i", fasta, "-t", str(t), "-f", "gbk", "-s", str(s))
    want = host(lib.GeneFinder(tinf, keep_nodes=True), records, gbk=True, scores=True)
    assert got == want[:3]
    assert s.read_bytes() == want[3]
