"""Translation-table choice by coding density on the GPU (GeneFinder.select_translation_table, pga_find_coding_bases,
pga_batch_replicate, train(..., translation_table="auto"), -g auto), against the host loop it replaces: train under every
candidate table, find_genes_batch(training_infos=...), a numpy union of the genes' [begin, end]."""
import gzip
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from pyrodigal_amd import tables
from tests.util import golden_path, read_fasta, synthetic_contig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GCF = "GCF_001457455.1_NCTC11397_genomic.fna.gz"
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib as L
    return L


def seq_of(name):
    return read_fasta(name)[0][1].encode()


def coverage(genes, length):
    """Positions 1 .. length inside [begin, end] of at least one gene (numpy union)."""
    cov = np.zeros(length, bool)
    for b, e in genes:
        b, e = max(int(b), 1), min(int(e), length)
        if b <= e:
            cov[b - 1:e] = True
    return int(cov.sum())


def host_yardstick(lib, contigs, table, **opts):
    """Today's API: train(*contigs) with the table, find_genes_batch per contig, the union of every contig's genes."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tinf = lib.GeneFinder(**opts).train(*contigs, translation_table=table)
    found = lib.GeneFinder(**opts).find_genes_batch(contigs, training_infos=[tinf] * len(contigs))
    bases = sum(coverage([(g.begin, g.end) for g in genes], len(c)) for c, genes in zip(contigs, found))
    return tinf, bases


def genomes():
    gcf = seq_of(GCF)
    cuts = [0, 700_000, 1_300_000, 2_000_000, len(gcf)]
    return {
        "GCF": [gcf],
        "GCF_100kb": [seq_of("GCF_001457455.1_NCTC11397_genomic_100kb.fna.gz")],
        "MIIJ01000039": [seq_of("MIIJ01000039.fna.gz")],
        "SRR492066": [seq_of("SRR492066.fna.gz")],
        "GCF_4_contigs": [gcf[a:b] for a, b in zip(cuts, cuts[1:])],
    }


def recode_tgg(lib, seq):
    """The genome that needs table 4: in every complete gene called under table 11, every in-frame TGG becomes TGA on the gene's
    own strand (CCA -> TCA on the + strand for genes on the - strand)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        f = lib.GeneFinder()
        f.train(seq, translation_table=11)
        genes = f.find_genes(seq)
    s = bytearray(seq)
    n = 0
    for g in genes:
        if g.partial_begin or g.partial_end:
            continue
        if g.strand == 1:
            for p in range(g.begin - 1, g.end - 3, 3):
                if s[p:p + 3] == b"TGG":
                    s[p + 2] = ord("A"); n += 1
        else:
            for p in range(g.end - 3, g.begin - 1, -3):
                if s[p:p + 3] == b"CCA":
                    s[p] = ord("T"); n += 1
    return bytes(s), n


@pytest.fixture(scope="module")
def table4_genome(lib):
    seq, n = recode_tgg(lib, seq_of(GCF))
    assert n > 1000
    return seq


@pytest.fixture(scope="module")
def yardsticks(lib):
    out = {}
    for name, contigs in genomes().items():
        length = sum(len(c) for c in contigs)
        out[name] = (contigs, length, {t: host_yardstick(lib, contigs, t) for t in (11, 4)})
    return out


def test_select_matches_the_host_loop(lib, yardsticks):
    names = list(yardsticks)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = lib.GeneFinder().select_translation_table([yardsticks[n][0] for n in names])
    assert len(got) == len(names)
    for name, sel in zip(names, got):
        contigs, length, host = yardsticks[name]
        bases = {t: host[t][1] for t in (11, 4)}
        dens = {t: bases[t] / length for t in (11, 4)}
        assert sel.length == length, name
        assert dict(sel.coding_bases) == bases, name
        assert all(sel.coding_density[t] == dens[t] for t in (11, 4)), name          # bit for bit
        assert sel.translation_table == tables.choose_table(dens), name
        assert sel.translation_table == 11, (name, dens)                               # the unmodified fixtures
        assert bytes(sel.training_info.raw) == bytes(host[sel.translation_table][0].raw), name
        assert 0.5 < dens[11] < 1.0, (name, dens)


def test_auto_train_and_train_batch(lib, yardsticks):
    contigs, _, host = yardsticks["GCF_4_contigs"]
    f = lib.GeneFinder()
    t = f.train(*contigs, translation_table="auto")
    assert f.training_info is t and bytes(t.raw) == bytes(host[11][0].raw)
    small = yardsticks["SRR492066"][0][0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = lib.GeneFinder().train_batch([contigs, small, small], translation_table=["auto", 4, "auto"])
        want4 = lib.GeneFinder().train(small, translation_table=4)
    assert bytes(got[0].raw) == bytes(host[11][0].raw)
    assert bytes(got[1].raw) == bytes(want4.raw)
    assert bytes(got[2].raw) == bytes(yardsticks["SRR492066"][2][11][0].raw)


def test_recoded_genome_picks_table_4(lib, table4_genome):
    length = len(table4_genome)
    host = {t: host_yardstick(lib, [table4_genome], t) for t in (11, 4)}
    dens = {t: host[t][1] / length for t in (11, 4)}
    # the construction must flip the rule, or the rest of this test would pass vacuously
    assert dens[4] - dens[11] > 0.05 and dens[4] > 0.7, dens
    sel, = lib.GeneFinder().select_translation_table([table4_genome])
    assert sel.translation_table == 4
    assert dict(sel.coding_bases) == {t: host[t][1] for t in (11, 4)}
    assert all(sel.coding_density[t] == dens[t] for t in (11, 4))
    assert bytes(sel.training_info.raw) == bytes(host[4][0].raw)
    assert sel.training_info.translation_table == 4
    f = lib.GeneFinder()
    assert bytes(f.train(table4_genome, translation_table="auto").raw) == bytes(host[4][0].raw)
    # the other thresholds of the rule, and a third candidate
    assert lib.GeneFinder().select_translation_table([table4_genome], min_density=0.99)[0].translation_table == 11
    three, = lib.GeneFinder().select_translation_table([table4_genome], candidates=(11, 25, 4))
    assert set(three.coding_bases) == {11, 25, 4} and three.coding_bases[4] == host[4][1]
    assert three.translation_table == tables.choose_table(three.coding_density, (11, 25, 4))


# ---- pga_find_coding_bases at the edges, through the C-ABI ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def models(ctx):
    m11 = gzip.open(golden_path("SRR492066.training.bin.gz")).read()
    m4 = ctx.train(seq_of("GCF_001457455.1_NCTC11397_genomic_100kb.fna.gz"), translation_table=4)
    return [m11, m4]


def edge_contigs():
    gcf = seq_of(GCF)
    masked = bytearray(gcf[300_000:420_000])
    for a in (5_000, 40_000, 90_000):
        masked[a:a + 400] = b"N" * 400
    masked[:120] = b"N" * 120
    return [
        gcf[:150_000],                                  # partial genes at both ends when the ends are open
        b"", b"AC", b"ATG",                            # no gene; shorter than three bases
        b"A" * 5_000,                                  # no gene with closed ends
        bytes(masked),                                 # runs of N (mask=True keeps genes out of them)
        synthetic_contig(400_000, 0.5, 81),            # segmented connection scoring, as smoke() uses
        gcf[1_000_000:1_080_000].translate(_COMP)[::-1],
        gcf[2_400_000:],
    ]


def numpy_coverage(res, contigs):
    return [coverage([(g["begin"], g["end"]) for g in res.genes_of(i)], len(c)) for i, c in enumerate(contigs)]


@pytest.mark.parametrize("closed,mask", [(False, False), (True, False), (False, True)])
def test_find_coding_bases_against_the_genes(ctx, models, closed, mask):
    contigs = edge_contigs()
    ctx.set_models(models)
    moc = np.arange(len(contigs), dtype=np.int32) % 2          # tables 11 and 4 in one call
    b = ctx.upload(contigs)
    try:
        kw = dict(closed=closed, mask=mask)
        cov, ng, sc = ctx.find_coding_bases(b, moc, **kw)
        res = ctx.find_genes(b, meta=False, model_of_contig=moc, **kw)
    finally:
        b.close()
    want = numpy_coverage(res, contigs)
    assert cov.tolist() == want
    assert ng.tolist() == res.contigs["n_genes"].tolist()
    assert sc.tolist() == res.contigs["score"].tolist()
    assert cov[1] == cov[2] == cov[3] == 0
    if closed:
        assert cov[4] == 0          # (open ends: poly-A has no stop in any frame, an edge gene covers it whole)
    g = res.genes
    if not closed:
        assert (g["partial_begin"] != 0).any() and (g["partial_end"] != 0).any()
    # genes that overlap on opposite strands are in the data
    opp = 0
    for i in range(len(contigs)):
        gi = res.genes_of(i)
        for s, e, st in zip(gi["begin"][:-1], gi["end"][:-1], gi["strand"][:-1]):
            nxt = gi[(gi["begin"] > s) & (gi["begin"] <= e) & (gi["strand"] != st)]
            opp += len(nxt)
    assert opp > 0
    if mask:
        assert res.masks is not None and sum(len(m) for m in res.masks) >= 3


def test_find_coding_bases_host_tail(ctx, models, tmp_path):
    """PGA_TAIL=host (the tail on host threads) counts on the host: the same numbers."""
    contigs = edge_contigs()
    ctx.set_models(models)
    moc = np.arange(len(contigs), dtype=np.int32) % 2
    b = ctx.upload(contigs)
    try:
        cov, ng, sc = ctx.find_coding_bases(b, moc)
    finally:
        b.close()
    script = tmp_path / "child.py"
    script.write_text(
        "import json, sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "from pyrodigal_amd import _cabi\n"
        "from tests.test_table_select_gpu import edge_contigs, models_blobs\n"
        "c = _cabi.Context(0)\n"
        "contigs = edge_contigs()\n"
        "c.set_models(models_blobs(c))\n"
        "b = c.upload(contigs)\n"
        "cov, ng, sc = c.find_coding_bases(b, np.arange(len(contigs), dtype=np.int32) %% 2)\n"
        "print(json.dumps([cov.tolist(), ng.tolist(), sc.tolist()]))\n"
        "b.close(); c.close()\n" % ROOT)
    r = subprocess.run([sys.executable, str(script)], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PGA_TAIL="host"))
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == [cov.tolist(), ng.tolist(), sc.tolist()]


def models_blobs(c):
    return [gzip.open(golden_path("SRR492066.training.bin.gz")).read(),
            c.train(seq_of("GCF_001457455.1_NCTC11397_genomic_100kb.fna.gz"), translation_table=4)]


def test_batch_replicate(ctx, models):
    contigs = [seq_of("SRR492066.fna.gz"), synthetic_contig(30_000, 0.4, 5), seq_of(GCF)[500_000:560_000]]
    ctx.set_models(models[:1])
    src = ctx.upload(contigs)
    order = [2, 0, 0, 1, 2]
    rep = ctx.replicate(src, order)
    try:
        a = ctx.find_genes(src, meta=False, model_of_contig=np.zeros(3, np.int32))
        r = ctx.find_genes(rep, meta=False, model_of_contig=np.zeros(len(order), np.int32))
        cov, _, _ = ctx.find_coding_bases(rep, np.zeros(len(order), np.int32))
    finally:
        rep.close()
        src.close()
    for e, i in enumerate(order):
        ga, gr = a.genes_of(i), r.genes_of(e)
        for k in ("begin", "end", "strand", "start_ndx", "stop_ndx", "cscore", "sscore"):
            assert np.array_equal(ga[k], gr[k]), (e, k)
        assert r.contigs[e]["score"] == a.contigs[i]["score"]
        assert cov[e] == coverage([(g["begin"], g["end"]) for g in ga], len(contigs[i]))
    bad = ctx.upload(contigs)
    try:
        with pytest.raises(ValueError):
            ctx.replicate(bad, [0, 3])
    finally:
        bad.close()


# ---- command line -----------------------------------------------------------------------------------------------------------

def write_fasta(path, sid, seq):
    with open(path, "w") as f:
        f.write(">%s\n" % sid)
        s = seq.decode()
        for k in range(0, len(s), 80):
            f.write(s[k:k + 80] + "\n")
    return str(path)


def cli(*argv):
    r = subprocess.run([sys.executable, "-m", "pyrodigal_amd", *argv], cwd=ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    return r


def test_cli_auto(lib, table4_genome, tmp_path):
    fa = write_fasta(tmp_path / "t4.fna", "recoded", table4_genome)
    model = tmp_path / "new.bin"
    cli("-i", fa, "-o", str(tmp_path / "t4.gff"), "-g", "auto", "-t", str(model))
    gff = (tmp_path / "t4.gff").read_text()
    heads = [l for l in gff.splitlines() if l.startswith("# Model Data")]
    assert heads and all("transl_table=4;" in l for l in heads)
    with open(model, "rb") as fh:
        assert lib.TrainingInfo.load(fh).translation_table == 4
    # an unmodified genome: -g auto is -g 11, byte for byte
    fa2 = write_fasta(tmp_path / "m.fna", "MIIJ01000039", seq_of("MIIJ01000039.fna.gz"))
    cli("-i", fa2, "-o", str(tmp_path / "auto.gff"), "-g", "auto", "-a", str(tmp_path / "auto.faa"))
    cli("-i", fa2, "-o", str(tmp_path / "t11.gff"), "-g", "11", "-a", str(tmp_path / "t11.faa"))
    assert (tmp_path / "auto.gff").read_bytes() == (tmp_path / "t11.gff").read_bytes()
    assert (tmp_path / "auto.faa").read_bytes() == (tmp_path / "t11.faa").read_bytes()
