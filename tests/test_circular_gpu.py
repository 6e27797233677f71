"""Circular contigs on the device (pga_batch_set_circular) against the rule restated over the CPU oracle
(tests/circular_ref.py): the cut, every gene field and the node arrays bit for bit; linear contigs of a mixed batch untouched."""
import gzip
import io
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from oracle import oracle as orc
from tests import circular_ref as cref
from tests.test_finder_gpu import NODE_F64, NODE_INT, compare_contig
from tests.util import golden_path, synthetic_contig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL, FULL_T = "GCF_001457455.1_NCTC11397_genomic", "GCF_001457455.1_NCTC11397_genomic.tinf_closed.bin.gz"
KB100, KB100_T = "GCF_001457455.1_NCTC11397_genomic_100kb", "GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz"
SRR_T = "SRR492066.training.bin.gz"
FIXED_ROTATIONS = lambda L: [1, 2, 3, L // 7, L // 3, L // 2, 5 * L // 6, L - 1]


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib as L
    return L


@pytest.fixture(scope="module")
def bins():
    return cref.meta_bins()


def compare_circular(res, i, seq, models, meta, closed=False, **oracle_kw):
    """Contig i of `res` was called as a circle: everything against the restatement.  Returns the restatement."""
    want = cref.Circular(seq, models, meta, closed=closed, **oracle_kw)
    L = len(seq)
    assert res.cuts[i] == want.cut
    cr = res.contigs[i]
    if meta:
        assert cr["model"] == want.model
    og, on = want.oracle.genes(), want.oracle.nodes()
    gg = res.genes_of(i)
    assert len(gg) == len(want.genes)
    order = np.asarray(want.order, np.int64)
    assert [(int(b), int(e), int(s)) for b, e, s in zip(gg["begin"], gg["end"], gg["strand"])] == want.genes
    assert np.all(gg["contig"] == i) and np.all(gg["begin"] >= 1) and np.all(gg["begin"] <= max(L, 1))
    assert not gg["partial_begin"].any() and not gg["partial_end"].any()
    assert np.all(np.diff(gg["begin"]) >= 0)
    if len(gg):
        assert np.array_equal(gg["start_ndx"], og["start_ndx"][order]) and np.array_equal(gg["stop_ndx"], og["stop_ndx"][order])
        s = on[og["start_ndx"][order]]
        for k in ("cscore", "sscore", "rscore", "uscore", "tscore", "mot_score"):
            assert np.array_equal(gg[k].view(np.uint64), s[k].view(np.uint64)), k
        assert np.array_equal(gg["gc_cont"].view(np.uint32), s["gc_cont"].view(np.uint32))
        assert np.array_equal(gg["start_type"], np.where(s["edge"] != 0, 3, s["type"]))
        assert np.array_equal(gg["rbs"], s["rbs"])
        for k in ("mot_ndx", "mot_len", "mot_spacer"):
            assert np.array_equal(gg[k].astype(np.int64), s[k].astype(np.int64)), k
    if res.nodes is not None and (not meta or cr["model"] >= 0):
        nd = res.nodes[i]                       # the nodes of R, in R's coordinates
        assert nd["n"] == len(on)
        for k in NODE_INT:
            assert np.array_equal(nd[k].astype(np.int64), on[k].astype(np.int64)), k
        for k in NODE_F64:
            assert np.array_equal(nd[k].view(np.uint64), on[k].view(np.uint64)), k
        assert np.array_equal(nd["gc_cont"].view(np.uint32), on["gc_cont"].view(np.uint32))
        assert np.array_equal(nd["rbs"], on["rbs"])
        if not meta:
            assert np.array_equal(nd["star_ptr"], on["star_ptr"])
    return want


# ---------------------------------------------------------------------------------------------- the table of the issue

def test_closed_chromosome_single(ctx):
    seq, models = cref.fixture(FULL), cref.single_model(FULL_T)
    ctx.set_models([m.buf for m in models])
    res = ctx.find_genes_batch([seq], meta=False, want_nodes=True, circular=True)
    want = compare_circular(res, 0, seq, models, False)
    gg = res.genes_of(0)
    assert len(gg) == 2343 and len(want.linear) == 2343
    assert (int(gg["begin"][-1]), int(gg["end"][-1]), int(gg["strand"][-1])) == (2463649, 2465325, 1)
    assert want.linear[0] == (1, 1659, 1)
    assert sorted(want.linear[1:]) == sorted(want.genes[:-1])          # every other gene identical


def test_srr492066_single_and_meta(ctx, bins):
    seq = cref.fixture("SRR492066")
    models = cref.single_model(SRR_T)
    ctx.set_models([m.buf for m in models])
    res = ctx.find_genes_batch([seq], meta=False, want_nodes=True, circular=[True])
    want = compare_circular(res, 0, seq, models, False)
    assert want.cut == 52426 and len(want.linear) == 76 and len(want.genes) == 75 and want.genes[-1] == (79328, 80116, -1)
    ctx.set_models([m.buf for m in bins])
    res = ctx.find_genes_batch([seq], meta=True, want_nodes=True, circular=True)
    want = compare_circular(res, 0, seq, bins, True)
    assert len(want.linear) == 79 and len(want.genes) == 78 and want.genes[-1] == (79328, 80116, -1)


def test_meta_fixtures_and_planted_orf(ctx, bins):
    planted, _ = cref.planted_orf()
    seqs = [cref.fixture("KK037166"), cref.fixture("MIIJ01000039"), planted]
    ctx.set_models([m.buf for m in bins])
    res = ctx.find_genes_batch(seqs, meta=True, want_nodes=True, circular=True)
    kk, mi, pl = [compare_circular(res, i, s, bins, True) for i, s in enumerate(seqs)]
    assert len(kk.linear) == 20 and len(kk.genes) == 20 and kk.genes[-1] == (19933, 20169, -1) and kk.cut == 11007
    assert len(mi.linear) == 425 and len(mi.genes) == 424 and all(e <= len(seqs[1]) for _, e, _ in mi.genes)
    assert pl.linear[0] == (1, 606, 1) and pl.linear[-1] == (30631, 31230, 1) and pl.genes[-1] == (30631, 31836, 1)


def test_100kb_single_has_nothing_across_the_origin(ctx):
    seq, models = cref.fixture(KB100), cref.single_model(KB100_T)
    ctx.set_models([m.buf for m in models])
    res = ctx.find_genes_batch([seq], meta=False, want_nodes=True, circular=True)
    want = compare_circular(res, 0, seq, models, False)
    assert len(want.linear) == 102 and len(want.genes) == 102


# ---------------------------------------------------------------------------------------------- mixed batches

def mixed_batch():
    seqs = [b"", b"A", b"AT", b"ATG"] + [synthetic_contig(n, 0.5, 900 + n) for n in (61, 89, 90, 180, 1500, 3000)]
    seqs += [synthetic_contig(20000, 0.35 + 0.3 * (c % 7) / 6, 3000 + c) for c in range(64)]
    seqs += [cref.fixture("SRR492066"), cref.fixture("KK037166")]
    # the short ones twice, so that each length is met both as a circle and as a line
    seqs = seqs[:10] + seqs[:10] + seqs[10:]
    flags = [True] * 10 + [False] * 10 + [c % 2 == 0 for c in range(64)] + [True, True]
    return seqs, flags


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("meta", [True, False])
def test_mixed_batch(ctx, bins, meta, closed):
    seqs, flags = mixed_batch()
    models = bins if meta else cref.single_model(SRR_T)
    ctx.set_models([m.buf for m in models])
    plain = ctx.find_genes_batch(seqs, meta=meta, closed=closed, want_nodes=True)
    res = ctx.find_genes_batch(seqs, meta=meta, closed=closed, want_nodes=True, circular=flags)
    assert plain.cuts is None
    n_circ = 0
    for i, s in enumerate(seqs):
        if flags[i]:
            n_circ += len(compare_circular(res, i, s, models, meta, closed=closed).genes)
        else:
            assert res.cuts[i] == -1
            assert res.genes_of(i).tobytes() == plain.genes_of(i).tobytes()
            for k in ("model", "n_nodes", "n_genes", "n_unknown", "gc", "score"):
                assert res.contigs[i][k] == plain.contigs[i][k], k
            for k, a in plain.nodes[i].items():
                assert np.array_equal(np.asarray(a), np.asarray(res.nodes[i][k])), k
            compare_contig(res, i, s, orc.Oracle(s), models, meta, closed=closed)
    assert n_circ > 75                  # SRR492066 alone has 75 (78 in meta mode): other circles have genes too
    # the contig records tile one gene array, in batch order
    at = 0
    for c in res.contigs:
        assert c["gene_begin"] == at
        at += c["n_genes"]
    assert at == len(res.genes)


def test_closed_finder_gives_the_same_cuts_on_the_fixtures(ctx, bins):
    """With `closed` set pass 1 only moves the cut; on these two inputs it does not."""
    srr, kk = cref.fixture("SRR492066"), cref.fixture("KK037166")
    single = cref.single_model(SRR_T)
    ctx.set_models([m.buf for m in single])
    res = ctx.find_genes_batch([srr], meta=False, closed=True, circular=True)
    a = compare_circular(res, 0, srr, single, False, closed=True)
    assert a.cut == 52426 and a.genes == cref.Circular(srr, single, False, closed=False).genes
    ctx.set_models([m.buf for m in bins])
    res = ctx.find_genes_batch([kk], meta=True, closed=True, circular=True)
    b = compare_circular(res, 0, kk, bins, True, closed=True)
    assert b.cut == 11007 and b.genes == cref.Circular(kk, bins, True, closed=False).genes


def test_two_models_in_one_batch(ctx):
    m0, m1 = cref.single_model(SRR_T)[0], cref.single_model(KB100_T)[0]
    seqs = [cref.fixture("SRR492066"), cref.fixture(KB100), cref.fixture("KK037166"), synthetic_contig(20000, 0.5, 5)]
    moc, flags = [0, 1, 1, 0], [True, True, False, True]
    ctx.set_models([m0.buf, m1.buf])
    b = ctx.upload(seqs).set_circular(flags)
    try:
        res = ctx.find_genes(b, meta=False, want_nodes=True, model_of_contig=moc)
        rep = ctx.replicate(b, [1, 0])                       # the flags travel with the contigs
        res2 = ctx.find_genes(rep, meta=False, model_of_contig=[1, 0])
        rep.close()
    finally:
        b.close()
    for i, s in enumerate(seqs):
        model = [m0, m1][moc[i]]
        if flags[i]:
            compare_circular(res, i, s, [model], False)
        else:
            compare_contig(res, i, s, orc.Oracle(s), [model], False)
        assert res.contigs[i]["model"] == moc[i]
    assert list(res2.cuts) == [res.cuts[1], res.cuts[0]]
    for a, b_ in ((0, 1), (1, 0)):
        x, y = res2.genes_of(a), res.genes_of(b_)
        assert all(np.array_equal(x[k], y[k]) for k in ("begin", "end", "strand", "start_ndx", "stop_ndx"))


# ---------------------------------------------------------------------------------------------- masks follow the letters

def test_unknown_run_that_touches_both_ends(ctx, bins):
    body = synthetic_contig(24000, 0.5, 61)
    seqs = [b"N" * 40 + body + b"N" * 30, b"N" * 200 + cref.fixture("KK037166") + b"N" * 100]
    ctx.set_models([m.buf for m in bins])
    res = ctx.find_genes_batch(seqs, meta=True, want_nodes=True, mask=True, circular=True)
    for i, s in enumerate(seqs):
        compare_circular(res, i, s, bins, True, mask=True, mask_size=50)
        assert np.array_equal(res.masks[i], orc.Oracle(s, mask=True, mask_size=50).masks())     # reported in the record's coordinates


def test_named_region_that_contains_the_cut_and_lower_case_runs(ctx, bins):
    left, right = synthetic_contig(12000, 0.5, 62), synthetic_contig(11000, 0.5, 63)
    seq = left + b"N" * 1500 + right
    region = [(len(left), len(left) + 1500)]
    ctx.set_models([m.buf for m in bins])
    res = ctx.find_genes_batch([seq], meta=True, want_nodes=True, mask=False, regions=[region], circular=True)
    want = compare_circular(res, 0, seq, bins, True, mask=True, mask_size=50)
    assert region[0][0] < want.cut < region[0][1]            # the region is split in two on the rotated contig
    assert np.array_equal(res.masks[0], np.asarray(region, np.int32))
    soft = left + b"n" * 1500 + right[:5000] + b"n" * 60 + right[5060:] + b"n" * 20
    res = ctx.find_genes_batch([soft, seq], meta=True, want_nodes=True, mask=False, mask_lowercase=True, circular=[True, False])
    compare_circular(res, 0, soft, bins, True, mask=True, mask_size=50)
    assert res.cuts[1] == -1


# ---------------------------------------------------------------------------------------------- rotations

@pytest.mark.parametrize("name, model, meta", [(KB100, KB100_T, False), ("SRR492066", SRR_T, False), ("SRR492066", None, True),
                                                ("KK037166", None, True)])
def test_fixed_rotations(ctx, bins, name, model, meta):
    """The device equals the restatement for every rotation; on these inputs the gene set does not depend on where the record is
    cut (checked on the reference for exactly these rotations: not a property of the rule)."""
    seq = cref.fixture(name)
    L = len(seq)
    models = bins if meta else cref.single_model(model)
    ctx.set_models([m.buf for m in models])
    ks = FIXED_ROTATIONS(L)
    seqs = [seq] + [seq[k:] + seq[:k] for k in ks]
    res = ctx.find_genes_batch(seqs, meta=meta, circular=True)
    base = compare_circular(res, 0, seq, models, meta)
    for i, k in enumerate(ks, 1):
        compare_circular(res, i, seqs[i], models, meta)
        g = res.genes_of(i)
        back = sorted(((int(b) - 1 + k) % L + 1, (int(b) - 1 + k) % L + 1 + int(e) - int(b), int(s)) for b, e, s in zip(g["begin"], g["end"], g["strand"]))
        assert back == sorted(base.genes), k


# ---------------------------------------------------------------------------------------------- text

WRITERS = {"gff": "write_gff", "faa": "write_translations", "fna": "write_genes"}


def host_text(genes_list, ids, fmt):
    out = io.StringIO()
    for genes, sid in zip(genes_list, ids):
        getattr(genes, WRITERS[fmt])(out, sid)
    return out.getvalue().encode("utf-8")


def test_device_text_equals_host_writers(ctx, lib):
    planted, orf = cref.planted_orf()
    srr = cref.fixture("SRR492066")
    seqs, ids, flags = [srr, planted, srr], ["SRR492066", "planted", "linear"], [True, True, False]
    tinf = lib.TrainingInfo(raw=cref.single_model(SRR_T)[0].tobytes())
    finder = lib.GeneFinder(tinf)
    genes_list = finder.find_genes_batch(seqs, circular=flags)
    assert [g.circular for g in genes_list] == flags and genes_list[2].cut is None and genes_list[0].cut == 52426
    ctx.set_models([tinf.raw])
    b = ctx.upload(seqs).set_circular(flags)
    try:
        r = ctx.find_genes(b, meta=False)
        out = ctx.render_genes(b, r, ids, ("gff", "faa", "fna"))
        with pytest.raises(Exception, match="circular"):
            ctx.render_genes(b, r, ids, ("gbk",))
        with pytest.raises(Exception, match="circular"):
            ctx.render_genes(b, r, ids, ("scores",))
        letters, off = ctx.translate_genes(b, r)
    finally:
        b.close()
    for fmt in WRITERS:
        want = host_text(genes_list, ids, fmt)
        assert out[fmt].fallback == 0
        assert out[fmt].data == want, fmt
    gff = out["gff"].data.decode()
    assert '# Sequence Data: seqnum=1;seqlen=79939;seqhdr="SRR492066";topology=circular\n' in gff
    assert 'seqhdr="linear"\n' in gff
    assert "SRR492066\tpyrodigal_amd" in gff and "\tCDS\t79328\t80116\t" in gff
    # the proteins of the spanning genes: read from the doubled record; the planted one is the planted ORF's
    from pyrodigal_amd.lib import Sequence
    for i in (0, 1):
        s = seqs[i]
        g = genes_list[i][len(genes_list[i]) - 1]
        assert g.end > len(s)
        k = int(r.contigs[i]["gene_begin"]) + len(genes_list[i]) - 1
        doubled = lib._genes_from_records(Sequence(s + s), r.genes[k:k + 1].tobytes(), tinf, 1)[0]      # the same record on S + S: no wrap
        assert (doubled.begin, doubled.end) == (g.begin, g.end)
        assert g.translate() == doubled.translate() and g.sequence() == doubled.sequence()
        assert bytes(letters[off[k]:off[k + 1]]).decode() == g.translate()
    g = genes_list[1][len(genes_list[1]) - 1]
    assert (g.begin, g.end, g.strand) == (30631, 31836, 1) and g.sequence() == orf
    table = {"GCT": "A", "GAA": "E", "AAA": "K", "CTG": "L", "GGT": "G", "GAT": "D", "ACC": "T", "ATC": "I", "CGT": "R", "CAG": "Q"}
    assert g.translate() == "M" + "".join(table[orf[k:k + 3]] for k in range(3, len(orf) - 3, 3)) + "*"
    # GenBank and the start file on the host
    gb = io.StringIO()
    genes_list[0].write_genbank(gb, "SRR492066")
    assert "bp    DNA     circular BCT" in gb.getvalue() and "complement(join(79328..79939,1..177))" in gb.getvalue()
    with pytest.raises(ValueError, match="circular"):
        genes_list[0].write_scores(io.StringIO(), "SRR492066")


def test_command_line_from_header(lib, tmp_path):
    srr, kk = cref.fixture("SRR492066").decode(), cref.fixture("KK037166").decode()
    path = tmp_path / "two.fna"
    with open(path, "w") as f:
        f.write(">plasmid1 length=79939 Circular=TRUE\n%s\n>contig2 some linear thing\n%s\n" % (srr, kk))
    tfile = tmp_path / "model.bin"
    with gzip.open(golden_path(SRR_T), "rb") as src, open(tfile, "wb") as dst:
        dst.write(src.read())
    o, a, d = tmp_path / "o.gff", tmp_path / "a.faa", tmp_path / "d.fna"
    run = subprocess.run([sys.executable, "-m", "pyrodigal_amd", "-i", str(path), "-t", str(tfile), "-o", str(o), "-a", str(a), "-d", str(d),
                          "--circular-from-header"], cwd=ROOT, capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr.decode()
    with open(tfile, "rb") as fh:
        finder = lib.GeneFinder(lib.TrainingInfo.load(fh))
    genes = [finder.find_genes(srr, circular=True), finder.find_genes(kk)]
    out, faa, fna = io.StringIO(), io.StringIO(), io.StringIO()
    for g, sid in zip(genes, ("plasmid1", "contig2")):
        g.write_gff(out, sid); g.write_translations(faa, sid); g.write_genes(fna, sid)
    assert o.read_bytes() == out.getvalue().encode() and a.read_bytes() == faa.getvalue().encode() and d.read_bytes() == fna.getvalue().encode()
    assert b"topology=circular" in o.read_bytes() and b"\t79328\t80116\t" in o.read_bytes()
    # -f gbk: a batch with a circular record goes through the host writer
    run = subprocess.run([sys.executable, "-m", "pyrodigal_amd", "-i", str(path), "-t", str(tfile), "-o", str(o), "-f", "gbk",
                          "--circular-ids", str(tmp_path / "ids.txt")], cwd=ROOT, capture_output=True, timeout=600)
    assert run.returncode != 0 and b"--circular-ids" in run.stderr            # the file is missing
    (tmp_path / "ids.txt").write_text("plasmid1\nnobody\n")
    run = subprocess.run([sys.executable, "-m", "pyrodigal_amd", "-i", str(path), "-t", str(tfile), "-o", str(o), "-f", "gbk",
                          "--circular-ids", str(tmp_path / "ids.txt")], cwd=ROOT, capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr.decode()
    assert b"no sequence 'nobody'" in run.stderr
    gb = io.StringIO()
    for g, sid in zip(genes, ("plasmid1", "contig2")):
        g.write_genbank(gb, sid)
    assert o.read_bytes() == gb.getvalue().encode()


def test_thread_pool_pattern(lib):
    tinf = lib.TrainingInfo(raw=cref.single_model(SRR_T)[0].tobytes())
    seqs = [cref.fixture("SRR492066"), cref.fixture("KK037166")] + [synthetic_contig(20000, 0.45, 700 + i) for i in range(6)]
    lone = lib.GeneFinder(tinf)
    key = lambda genes: (genes.circular, genes.cut, [(g.begin, g.end, g.strand, g.partial_begin, g.partial_end, g.score) for g in genes])
    want = {(i, c): key(lone.find_genes(s, circular=c)) for i, s in enumerate(seqs) for c in (False, True)}
    finder = lib.GeneFinder(tinf, contexts=2)
    got, errors = {}, []
    start = threading.Barrier(32)

    def work(t):
        try:
            start.wait()
            for rep in range(4):
                i, c = (t + rep) % len(seqs), (t + rep) % 2 == 0
                got[(t, rep)] = ((i, c), key(finder.find_genes(seqs[i], circular=c)))
        except BaseException as e:          # noqa: reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(32)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(got) == 128
    for (k, res) in got.values():
        assert res == want[k], k
    assert want[(0, True)] != want[(0, False)]
