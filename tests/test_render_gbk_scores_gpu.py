"""Device rendering of GenBank records and start-score files (Context.render_genes "gbk" / "scores", render.hip): byte for byte
what Genes.write_genbank and Genes.write_scores write, contig after contig; and the node arrays a find keeps on the device for
them (want_nodes="device")."""
import datetime
import io
import warnings

import numpy as np
import pytest

from pyrodigal_amd import benchdata
from tests.util import golden_path, read_fasta, synthetic_contig

pytestmark = pytest.mark.gpu

DATE = datetime.date(2026, 3, 7)


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib as L
    return L


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


def unbinned_scores(i, seq, sid, tinf, header=True):
    """cli's text for a meta-mode contig no bin won: the header with the fallback model's data, an empty body."""
    if not header:
        return "\n"
    from pyrodigal_amd import __version__
    return ('# Sequence Data: seqnum=%d;seqlen=%d;seqhdr="%s"\n# Run Data: version=pyrodigal_amd.v%s;gc_cont=%.2f;transl_table=%d;'
            'uses_sd=%d\nBeg\tEnd\tStd\tTotal\tCodPot\tStrtSc\tCodon\tRBSMot\tSpacer\tRBSScr\tUpsScr\tTypeScr\tGCCont\n\n'
            % (i + 1, len(seq), sid, __version__, tinf.gc * 100, tinf.translation_table, int(tinf.uses_sd)))


def host_texts(genes_list, ids, seqs, gbk, scores, unbinned_tinf=None):
    """Per contig: (write_genbank text, write_scores text) of the host writers."""
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # a translation table with other stop codons warns on the host
        for i, (g, sid) in enumerate(zip(genes_list, ids)):
            a, b = io.StringIO(), io.StringIO()
            g.write_genbank(a, sid, **gbk)
            if g.meta and g.metagenomic_bin is None:
                b.write(unbinned_scores(i, seqs[i], sid, unbinned_tinf, **scores))
            else:
                g.write_scores(b, sid, **scores)
            out.append((a.getvalue().encode(), b.getvalue().encode()))
    return out


def device_render(ctx, seqs, ids, blobs, formats, meta=False, model_of_contig=None, find_kw=None, **kw):
    ctx.set_models(blobs)
    b = ctx.upload([s if isinstance(s, bytes) else s.encode() for s in seqs])
    try:
        r = ctx.find_genes(b, meta=meta, model_of_contig=model_of_contig, want_nodes="device", **(find_kw or {}))
        assert r.nodes is None
        return r, ctx.render_genes(b, r, ids, formats, meta=meta, model_of_contig=model_of_contig, **kw)
    finally:
        b.close()


def first_difference(got, want):
    a, w = got.split(b"\n"), want.split(b"\n")
    k = next((i for i in range(min(len(a), len(w))) if a[i] != w[i]), min(len(a), len(w)))
    return "line %d:\n device %r\n host   %r" % (k, a[k] if k < len(a) else None, w[k] if k < len(w) else None)


def check(out, want, names=("gbk", "scores")):
    for k, name in enumerate(("gbk", "scores")):
        if name not in names:
            continue
        t = out[name]
        assert t.fallback == 0
        whole = b"".join(w[k] for w in want)
        if t.data != whole:
            pytest.fail("%s differs at %s" % (name, first_difference(t.data, whole)))
        assert t.contig_offsets[0] == 0 and t.contig_offsets[-1] == len(whole)
        for i, w in enumerate(want):
            assert t.contig(i) == w[k], (name, i)


FORMATS = {"gbk": {"date": DATE}, "scores": {}}


def run_single(lib, ctx, seqs, ids, tinf, formats=FORMATS, find_kw=None):
    genes_list = lib.GeneFinder(tinf, **(find_kw or {})).find_genes_batch(seqs)
    _, out = device_render(ctx, seqs, ids, [tinf.raw], formats, find_kw=find_kw)
    check(out, host_texts(genes_list, ids, seqs, formats["gbk"], formats["scores"]))
    return genes_list, out


@pytest.mark.parametrize("name", ["SRR492066", "MIIJ01000039", "KK037166"])
def test_single_mode_fixtures(lib, ctx, name):
    from oracle import oracle as orc
    recs = read_fasta(name + ".fna.gz")
    seqs = [s for _, s in recs]
    ids = [h.split()[0] for h, _ in recs]
    tinf = lib.TrainingInfo(raw=orc.Oracle(seqs[0]).train().tobytes())
    run_single(lib, ctx, seqs, ids, tinf)


def test_non_sd_model_spells_the_motifs(lib, ctx):
    seq = read_fasta("KK037166.fna.gz")[0][1]
    tinf = lib.GeneFinder().train(seq, force_nonsd=True)
    assert not tinf.uses_sd
    genes_list, out = run_single(lib, ctx, [seq], ["KK037166"], tinf)
    rows = out["scores"].data.decode().split("\n")
    motifs = {r.split("\t")[7] for r in rows if r and not r.startswith(("#", "Beg"))}
    assert any(m not in ("None",) and set(m) <= set("ACGT") for m in motifs), "no row took the motif-string branch"


def test_closed_genome_100kb(lib, ctx):
    recs = read_fasta("GCF_001457455.1_NCTC11397_genomic_100kb.fna.gz")
    tinf = lib.TrainingInfo.load(golden_path("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz"))
    run_single(lib, ctx, [s for _, s in recs], [h.split()[0] for h, _ in recs], tinf, find_kw={"closed": True})


def test_long_contig_segmented(lib, ctx):
    """A whole genome in one contig: its chain is cut into segments."""
    recs = read_fasta("GCF_001457455.1_NCTC11397_genomic.fna.gz")
    tinf = lib.TrainingInfo.load(golden_path("GCF_001457455.1_NCTC11397_genomic.tinf_closed.bin.gz"))
    seqs = [max((s for _, s in recs), key=len)]
    run_single(lib, ctx, seqs, ["genome"], tinf, find_kw={"closed": True})
    assert ctx.dp_stats()["segments"] > ctx.dp_stats()["chains"] >= 1


def test_host_tail(lib, ctx, monkeypatch):
    """The tail walked by host threads moves start scores on the host copy: the arena kept on the device gets them back."""
    tinf = lib.TrainingInfo.load(golden_path("SRR492066.training.bin.gz"))
    seqs = [synthetic_contig(120_000, 0.5, 17), read_fasta("SRR492066.fna.gz")[0][1]]
    monkeypatch.setenv("PGA_TAIL", "host")
    run_single(lib, ctx, seqs, ["a", "b"], tinf)


def with_unknowns(seq, seed):
    """N runs, lowercase stretches and a few other IUPAC letters."""
    rng = np.random.default_rng(seed)
    s = bytearray(seq)
    for _ in range(len(s) // 20_000 + 1):
        p, k = int(rng.integers(0, max(1, len(s) - 200))), int(rng.integers(1, 120))
        s[p:p + k] = b"N" * len(s[p:p + k])
    for _ in range(len(s) // 5_000 + 1):
        p = int(rng.integers(0, len(s)))
        s[p] = ord("RYKMSWN"[int(rng.integers(0, 7))])
    p = int(rng.integers(0, max(1, len(s) - 3000)))
    s[p:p + 3000] = bytes(s[p:p + 3000]).lower()
    return bytes(s)


def odd_contigs():
    seqs = [with_unknowns(synthetic_contig(n, gc, 300 + i), i) for i, (n, gc) in enumerate([(150_000, 0.5), (60_000, 0.4), (30_000, 0.6)])]
    seqs += [synthetic_contig(n, 0.5, 700 + n) for n in (61, 62, 120, 299, 300)]            # short contigs
    seqs += [b"ACGTTGCA" * 6, b"acgtnnRYacgt" * 10, synthetic_contig(5_000, 0.5, 3).lower()]   # no nodes, IUPAC, lower case
    seqs.append(read_fasta("KK037166.fna.gz")[0][1].encode())
    return seqs


WRITER_OPTIONS = [
    {"gbk": {"date": DATE}, "scores": {}},
    {"gbk": {"date": DATE, "division": "PLN", "translation_table": 4, "strict_translation": False}, "scores": {"header": False}},
    {"gbk": {"date": datetime.date(1999, 12, 31), "division": "", "translation_table": 11}, "scores": {"header": True}},
]


@pytest.mark.parametrize("opts", WRITER_OPTIONS)
def test_writer_options_and_odd_contigs(lib, ctx, opts):
    seqs = odd_contigs()
    ids = ["ctg%d" % i for i in range(len(seqs))]
    ids[3] = "a_rather_long_identifier_of_more_than_23_characters"
    ids[4] = "ünïcode_id"
    tinf = lib.TrainingInfo.load(golden_path("SRR492066.training.bin.gz"))
    for mask in (False, True):
        genes_list = lib.GeneFinder(tinf, mask=mask).find_genes_batch(seqs)
        assert any(g.nodes is not None and len(g.nodes) == 0 for g in genes_list)
        r, out = device_render(ctx, seqs, ids, [tinf.raw], opts, find_kw={"mask": mask})
        check(out, host_texts(genes_list, ids, seqs, opts["gbk"], opts["scores"]))
        assert out["gbk"].data.count(b"\n//\n") == len(seqs)


def test_translation_table_4_model(lib, ctx):
    models = benchdata.load_model_set()
    tinf = next(lib.TrainingInfo(raw=b) for _, b in models if lib.TrainingInfo(raw=b).translation_table == 4)
    seqs = [synthetic_contig(90_000, 0.3, 41), synthetic_contig(40_000, 0.35, 42)]
    _, out = run_single(lib, ctx, seqs, ["m4a", "m4b"], tinf)
    assert b"/transl_table=4\n" in out["gbk"].data and b"transl_table=4;" in out["scores"].data


def meta_contigs(n, seed):
    rng = np.random.default_rng(seed)
    lens = np.exp(rng.uniform(np.log(61), np.log(200_000), n)).astype(int)
    lens[:3] = [61, 200_000, 2_000]
    seqs = []
    for i, L in enumerate(lens):
        s = synthetic_contig(int(L), float(rng.uniform(0.3, 0.7)), seed * 1000 + i)
        if i % 7 == 0:
            s = with_unknowns(s, i)
        seqs.append(s)
    seqs.append(b"ATGAAATAA" * 500)                    # nodes but (almost surely) no genes
    seqs.append(b"ACGT" * 10)                          # no nodes
    return seqs


@pytest.mark.parametrize("closed,mask", [(False, False), (True, True), (False, True)])
def test_meta_mode_bins(lib, ctx, closed, mask):
    models = benchdata.load_model_set()
    tinfs = [lib.TrainingInfo(raw=b) for _, b in models]
    bins = lib.MetagenomicBins([lib.MetagenomicBin(t, name) for t, (name, _) in zip(tinfs, models)])
    seqs = meta_contigs(120, 11 + closed + 2 * mask)
    genes_list = lib.GeneFinder(meta=True, metagenomic_bins=bins, closed=closed, mask=mask).find_genes_batch(seqs)
    ids = ["meta_%d" % i for i in range(len(seqs))]
    blobs = [b for _, b in models]
    kw = dict(meta=True, descriptions=[n for n, _ in models], find_kw={"closed": closed, "mask": mask})
    assert any(g.metagenomic_bin is None for g in genes_list)
    assert len({id(g.training_info) for g in genes_list if g.metagenomic_bin is not None}) > 4
    # a contig no bin won: write_scores refuses it, and so does the renderer unless it is told whose header to print
    with pytest.raises(ValueError, match="no model"):
        device_render(ctx, seqs, ids, blobs, {"scores": {}}, **kw)
    for opts in ({"gbk": {"date": DATE}, "scores": {}}, {"gbk": {"date": DATE, "division": "ENV"}, "scores": {"header": False}}):
        _, out = device_render(ctx, seqs, ids, blobs, opts, unbinned_model=5, **kw)
        check(out, host_texts(genes_list, ids, seqs, opts["gbk"], opts["scores"], unbinned_tinf=tinfs[5]))


def test_model_per_contig(lib, ctx):
    models = benchdata.load_model_set()
    tinfs = [lib.TrainingInfo(raw=b) for _, b in models[:4]]
    seqs = [synthetic_contig(80_000 + 5000 * i, 0.35 + 0.05 * i, 900 + i) for i in range(8)]
    choice = [tinfs[i % 4] for i in range(8)]
    genes_list = lib.GeneFinder().find_genes_batch(seqs, training_infos=choice)
    ids = ["g%d" % i for i in range(8)]
    moc = np.array([i % 4 for i in range(8)], np.int32)
    _, out = device_render(ctx, seqs, ids, [t.raw for t in tinfs], FORMATS, model_of_contig=moc)
    check(out, host_texts(genes_list, ids, seqs, FORMATS["gbk"], FORMATS["scores"]))


# ---- want_nodes="device" -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def single_setup(lib):
    tinf = lib.TrainingInfo.load(golden_path("SRR492066.training.bin.gz"))
    seqs = [read_fasta("SRR492066.fna.gz")[0][1].encode(), synthetic_contig(70_000, 0.45, 5), synthetic_contig(300, 0.5, 6)]
    return tinf, seqs, ["s0", "s1", "s2"]


def test_device_nodes_leave_the_genes_unchanged(ctx, single_setup):
    tinf, seqs, _ = single_setup
    ctx.set_models([tinf.raw])
    b = ctx.upload(seqs)
    try:
        r0 = ctx.find_genes(b, meta=False)
        g0, c0 = r0.genes.copy(), r0.contigs.copy()
        r1 = ctx.find_genes(b, meta=False, want_nodes=True)
        rd = ctx.find_genes(b, meta=False, want_nodes="device")
    finally:
        b.close()
    assert rd.nodes is None and r0.nodes is None and r1.nodes is not None
    # every field bit for bit (the records' padding bytes carry nothing)
    for want, got in ((g0, rd.genes), (g0, r1.genes), (c0, rd.contigs), (c0, r1.contigs)):
        assert len(want) == len(got)
        for name in want.dtype.names:
            assert want[name].tobytes() == got[name].tobytes(), name


def test_scores_need_the_nodes_of_this_result(lib, ctx, single_setup):
    tinf, seqs, ids = single_setup
    ctx.set_models([tinf.raw])
    b = ctx.upload(seqs)
    try:
        r0 = ctx.find_genes(b, meta=False)                                   # no nodes kept
        with pytest.raises(ValueError, match="no node arrays"):
            ctx.render_genes(b, r0, ids, "scores")
        ctx.render_genes(b, r0, ids, ("gff", "gbk"), date=DATE)              # the other formats need none
        r1 = ctx.find_genes(b, meta=False, want_nodes="device")
        first = ctx.render_genes(b, r1, ids, "scores")["scores"].data
        r2 = ctx.find_genes(b, meta=False, want_nodes="device")              # another find on the context: r1's nodes are gone
        with pytest.raises(ValueError, match="no node arrays"):
            ctx.render_genes(b, r1, ids, "scores")
        assert ctx.render_genes(b, r2, ids, "scores")["scores"].data == first
        ctx.train(bytes(seqs[0]))                                            # training runs the finder too
        with pytest.raises(ValueError, match="no node arrays"):
            ctx.render_genes(b, r2, ids, "scores")
        ctx.set_models([tinf.raw])
        # a result whose node arrays also came home (want_nodes=True) renders the same text
        r3 = ctx.find_genes(b, meta=False, want_nodes=True)
        assert ctx.render_genes(b, r3, ids, "scores")["scores"].data == first
        ctx.set_models([tinf.raw])                                           # loading models drops them
        with pytest.raises(ValueError, match="no node arrays"):
            ctx.render_genes(b, r3, ids, "scores")
    finally:
        b.close()
    genes_list = lib.GeneFinder(tinf).find_genes_batch([bytes(s) for s in seqs])
    assert first == b"".join(w[1] for w in host_texts(genes_list, ids, seqs, {"date": DATE}, {}))
