"""python -m pyrodigal_amd with -f gbk and -s on the GPU: both now rendered on the device, byte for byte what a Python loop over
GeneFinder.find_genes and Genes.write_genbank / write_gff / write_scores writes (a meta-mode contig no bin won: the fallback
bin's header and an empty body)."""
import gzip
import io
import os
import subprocess
import sys
import warnings

import pytest

from pyrodigal_amd import benchdata
from tests.util import read_fasta, synthetic_contig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib as L
    return L


@pytest.fixture(scope="module")
def records():
    recs = [(h.split()[0], s) for h, s in read_fasta("SRR492066.fna.gz")]
    recs += [("syn_%d" % i, synthetic_contig(n, gc, 60 + i).decode()) for i, (n, gc) in
             enumerate([(90_000, 0.45), (4_000, 0.55), (150_000, 0.35), (250, 0.5), (30_000, 0.6)])]
    recs += [("tiny", "ACGTTGCA" * 8 + "A"), ("no_genes", "ATGAAATAA" * 500)]
    recs += [(h.split()[0], s) for h, s in read_fasta("KK037166.fna.gz")]
    return recs


def write_fasta(path, records):
    with gzip.open(path, "wt") as f:
        for i, (sid, s) in enumerate(records):
            f.write(">%s description %d\n" % (sid, i))
            for k in range(0, len(s), 80):
                f.write(s[k:k + 80] + "\n")
    return str(path)


def cli(*argv):
    r = subprocess.run([sys.executable, "-m", "pyrodigal_amd", *argv, "--batch-bases", "60000", "-j", "2"], cwd=ROOT,
                       capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr.decode()
    return r


def host(make_finder, records, gbk, unbinned=None):
    """(main output, start file) of the host writers, record by record, from a fresh finder (a finder numbers the sequences it
    sees across calls); `unbinned`: the bin whose header a contig no bin won gets"""
    from pyrodigal_amd import __version__
    finder = make_finder()
    out, sc = io.StringIO(), io.StringIO()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k, (sid, s) in enumerate(records):
            g = finder.find_genes(s)
            if g.meta and g.metagenomic_bin is None:
                t = unbinned.training_info
                head = ('# Sequence Data: seqnum=%d;seqlen=%d;seqhdr="%s"\n' % (k + 1, len(s), sid))
                if gbk:
                    g.write_genbank(out, sid)
                else:
                    out.write('##gff-version  3\n' + head + '# Model Data: version=pyrodigal_amd.v%s;run_type=Metagenomic;model="%s";'
                              'gc_cont=%.2f;transl_table=%d;uses_sd=%d\n' % (__version__, unbinned.description, t.gc * 100,
                                                                              t.translation_table, int(t.uses_sd)))
                sc.write(head + '# Run Data: version=pyrodigal_amd.v%s;gc_cont=%.2f;transl_table=%d;uses_sd=%d\n'
                         'Beg\tEnd\tStd\tTotal\tCodPot\tStrtSc\tCodon\tRBSMot\tSpacer\tRBSScr\tUpsScr\tTypeScr\tGCCont\n\n'
                         % (__version__, t.gc * 100, t.translation_table, int(t.uses_sd)))
                continue
            if gbk:
                g.write_genbank(out, sid)
            else:
                g.write_gff(out, sid)
            g.write_scores(sc, sid)
    return out.getvalue().encode(), sc.getvalue().encode()


def same(got, want):
    for name, a, w in zip(("main output", "start file"), got, want):
        if a != w:
            al, wl = a.split(b"\n"), w.split(b"\n")
            k = next((i for i in range(min(len(al), len(wl))) if al[i] != wl[i]), min(len(al), len(wl)))
            pytest.fail("%s differs at line %d:\n cli  %r\n host %r" % (name, k, al[k] if k < len(al) else None, wl[k] if k < len(wl) else None))


def run(tmp_path, *extra):
    o, s = tmp_path / "o", tmp_path / "s.txt"
    cli("-o", str(o), "-s", str(s), *extra)
    return o.read_bytes(), s.read_bytes()


def test_single_mode_trained_and_training_file(lib, records, tmp_path):
    fasta = write_fasta(tmp_path / "in.fna.gz", records)
    t = tmp_path / "model.bin"
    got = run(tmp_path, "-i", fasta, "-t", str(t), "-f", "gbk")                  # trains, writes the training file
    tinf = lib.TrainingInfo.load(open(t, "rb"))
    finder = lambda: lib.GeneFinder(tinf, keep_nodes=True)
    same(got, host(finder, records, gbk=True))
    same(run(tmp_path, "-i", fasta, "-t", str(t)), host(finder, records, gbk=False))       # GFF and -s, the file read back
    closed = lambda: lib.GeneFinder(tinf, keep_nodes=True, closed=True)
    same(run(tmp_path, "-i", fasta, "-t", str(t), "-c", "-f", "gbk"), host(closed, records, gbk=True))


def test_meta_bins(lib, records, tmp_path):
    fasta = write_fasta(tmp_path / "meta.fna.gz", records)
    paths = []
    for name, blob in benchdata.load_model_set():
        p = tmp_path / name.replace(".gz", "")
        p.write_bytes(blob)
        paths.append(p)
    bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=p.read_bytes()), p.name) for p in paths])
    finder = lambda: lib.GeneFinder(meta=True, metagenomic_bins=bins, keep_nodes=True)
    assert any(g.metagenomic_bin is None for g in finder().find_genes_batch([s for _, s in records]))
    for fmt in ("gff", "gbk"):
        got = run(tmp_path, "-i", fasta, "-p", "meta", "-f", fmt, "--meta-bins", *map(str, paths))
        same(got, host(finder, records, gbk=fmt == "gbk", unbinned=bins[5]))
