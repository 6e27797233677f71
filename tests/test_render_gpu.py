"""Device rendering of gene calls into GFF / protein FASTA / gene FASTA (Context.render_genes, render.hip): byte for byte what
the host writers Genes.write_gff / write_translations / write_genes emit, contig after contig, with no line left to the host."""
import gzip
import io
import warnings

import numpy as np
import pytest

from pyrodigal_amd import benchdata
from tests.util import golden_path, read_fasta, synthetic_contig

pytestmark = pytest.mark.gpu

WRITERS = {"gff": "write_gff", "faa": "write_translations", "fna": "write_genes"}


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


def host_text(genes_list, ids, fmt, **opts):
    out = io.StringIO()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # a translation table with other stop codons warns on the host
        for genes, sid in zip(genes_list, ids):
            getattr(genes, WRITERS[fmt])(out, sid, **opts)
    return out.getvalue().encode("utf-8")


def device_render(ctx, seqs, ids, blobs, formats, meta=False, model_of_contig=None, descriptions=None, find_kw=None, **kw):
    ctx.set_models(blobs)
    b = ctx.upload([s if isinstance(s, bytes) else s.encode() for s in seqs])
    try:
        r = ctx.find_genes(b, meta=meta, model_of_contig=model_of_contig, **(find_kw or {}))
        return r, ctx.render_genes(b, r, ids, formats, meta=meta, model_of_contig=model_of_contig, descriptions=descriptions, **kw)
    finally:
        b.close()


def check_all(out, genes_list, ids, formats):
    for fmt, opts in formats.items():
        want = host_text(genes_list, ids, fmt, **opts)
        got = out[fmt]
        assert got.fallback == 0
        if got.data != want:
            a = got.data.split(b"\n"); w = want.split(b"\n")
            k = next(i for i in range(min(len(a), len(w))) if a[i] != w[i]) if any(x != y for x, y in zip(a, w)) else min(len(a), len(w))
            pytest.fail("%s differs at line %d:\n device %r\n host   %r" % (fmt, k, a[k] if k < len(a) else None, w[k] if k < len(w) else None))
        # per-contig offsets split the text exactly as the writers wrote it contig by contig
        assert got.contig_offsets[0] == 0 and got.contig_offsets[-1] == len(want)
        for i in range(len(ids)):
            assert got.contig(i) == host_text([genes_list[i]], [ids[i]], fmt, **opts)


DEFAULTS = {"gff": {}, "faa": {}, "fna": {}}


@pytest.mark.parametrize("name", ["SRR492066", "KK037166", "MIIJ01000039", "GCF_001457455.1_NCTC11397_genomic_100kb"])
def test_single_mode_fixtures(lib, ctx, name):
    from oracle import oracle as orc
    recs = read_fasta(name + ".fna.gz")
    seqs = [s for _, s in recs]
    ids = [h.split()[0] for h, _ in recs]
    tinf = lib.TrainingInfo(raw=orc.Oracle(seqs[0]).train().tobytes())
    genes_list = lib.GeneFinder(tinf).find_genes_batch(seqs)
    _, out = device_render(ctx, seqs, ids, [tinf.raw], DEFAULTS)
    check_all(out, genes_list, ids, DEFAULTS)


def test_reference_goldens_through_the_renderer(lib, ctx):
    from oracle import oracle as orc
    for name in ("SRR492066", "KK037166", "MIIJ01000039"):
        hdr, seq = read_fasta(name + ".fna.gz")[0]
        tinf = lib.TrainingInfo(raw=orc.Oracle(seq).train().tobytes())
        _, out = device_render(ctx, [seq], [hdr.split()[0]], [tinf.raw], ("faa", "fna"))
        assert out["faa"].data == gzip.open(golden_path(name + ".single.faa.gz"), "rb").read()
        assert out["fna"].data == gzip.open(golden_path(name + ".single.fna.gz"), "rb").read()


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


WRITER_OPTIONS = [
    {"gff": {"header": False, "include_translation_table": True, "full_id": False, "version_separator": "-"},
     "faa": {"width": 1, "include_stop": False, "strict_translation": False, "full_id": True},
     "fna": {"width": 1, "full_id": True}},
    {"gff": {"include_translation_table": True}, "faa": {"width": 80, "translation_table": 4, "strict_translation": False},
     "fna": {"width": 80}},
    {"faa": {"width": 70, "include_stop": False}, "fna": {"width": 60}},
    {"faa": {"width": 60, "translation_table": 11}, "fna": {"width": 70}},
]


@pytest.mark.parametrize("opts", WRITER_OPTIONS)
def test_writer_options(lib, ctx, opts):
    from oracle import oracle as orc
    seqs = [with_unknowns(synthetic_contig(n, gc, 300 + i), i) for i, (n, gc) in enumerate([(150_000, 0.5), (60_000, 0.4), (30_000, 0.6)])]
    seqs.append(read_fasta("KK037166.fna.gz")[0][1].encode())
    ids = ["ctg%d" % i for i in range(len(seqs))]
    tinf = lib.TrainingInfo(raw=orc.Oracle(read_fasta("SRR492066.fna.gz")[0][1]).train().tobytes())
    for mask in (False, True):
        genes_list = lib.GeneFinder(tinf, mask=mask).find_genes_batch(seqs)
        _, out = device_render(ctx, seqs, ids, [tinf.raw], opts, find_kw={"mask": mask})
        check_all(out, genes_list, ids, opts)


def meta_contigs(n, seed):
    rng = np.random.default_rng(seed)
    lens = np.exp(rng.uniform(np.log(61), np.log(400_000), n)).astype(int)
    lens[:3] = [61, 400_000, 2_000]
    seqs = []
    for i, L in enumerate(lens):
        s = synthetic_contig(int(L), float(rng.uniform(0.3, 0.7)), seed * 1000 + i)
        if i % 7 == 0:
            s = with_unknowns(s, i)
        seqs.append(s)
    seqs.append(b"ATGAAATAA" * 500)                    # nodes but (almost surely) no genes
    return seqs


@pytest.mark.parametrize("closed,mask", [(False, False), (True, True)])
def test_meta_mode_bins(lib, ctx, closed, mask):
    models = benchdata.load_model_set()
    tinfs = [lib.TrainingInfo(raw=b) for _, b in models]
    assert any(t.translation_table == 4 for t in tinfs) and any(not t.uses_sd for t in tinfs)
    bins = lib.MetagenomicBins([lib.MetagenomicBin(t, name) for t, (name, _) in zip(tinfs, models)])
    finder = lib.GeneFinder(meta=True, metagenomic_bins=bins, closed=closed, mask=mask)
    seqs = meta_contigs(240, 7 + closed)
    genes_list = finder.find_genes_batch(seqs)
    ids = ["meta_%d" % i for i in range(len(seqs))]
    kw = dict(meta=True, descriptions=[n for n, _ in models], find_kw={"closed": closed, "mask": mask})
    blobs = [b for _, b in models]
    # a contig without genes has no bin: write_gff refuses it, and so does the renderer; the FASTA writers write nothing for it
    unbinned = [i for i, g in enumerate(genes_list) if g.metagenomic_bin is None]
    assert unbinned and all(len(genes_list[i]) == 0 for i in unbinned)
    with pytest.raises(RuntimeError):
        host_text(genes_list, ids, "gff")
    with pytest.raises(ValueError):
        device_render(ctx, seqs, ids, blobs, {"gff": {}}, **kw)
    _, out = device_render(ctx, seqs, ids, blobs, {"faa": {}, "fna": {}}, **kw)
    check_all(out, genes_list, ids, {"faa": {}, "fna": {}})
    # ... unless the caller names the model such a contig reports (Prodigal: bin 5): its GFF is the header with that model's data
    _, out = device_render(ctx, seqs, ids, blobs, {"gff": {}}, unbinned_model=5, **kw)
    assert out["gff"].fallback == 0
    want = []
    for i, (g, sid) in enumerate(zip(genes_list, ids)):
        if g.metagenomic_bin is None:
            t = tinfs[5]
            want.append('##gff-version  3\n# Sequence Data: seqnum=%d;seqlen=%d;seqhdr="%s"\n# Model Data: version=pyrodigal_amd.v%s;'
                        'run_type=Metagenomic;model="%s";gc_cont=%.2f;transl_table=%d;uses_sd=%d\n'
                        % (i + 1, len(seqs[i]), sid, lib._VERSION, models[5][0], t.gc * 100, t.translation_table, int(t.uses_sd)))
        else:
            want.append(host_text([g], [sid], "gff").decode())
        assert out["gff"].contig(i) == want[-1].encode()
    assert out["gff"].data == "".join(want).encode()
    # GFF over the contigs that got a bin
    keep = [i for i, g in enumerate(genes_list) if g.metagenomic_bin is not None]
    seqs = [seqs[i] for i in keep]
    genes_list = lib.GeneFinder(meta=True, metagenomic_bins=bins, closed=closed, mask=mask).find_genes_batch(seqs)
    ids = ["meta_%d" % i for i in range(len(seqs))]
    if not closed:
        assert any(g[0].partial_begin for g in genes_list if len(g)) and any(g[-1].partial_end for g in genes_list if len(g))
    used = {id(g.training_info) for g in genes_list}
    assert len(used) > 4
    _, out = device_render(ctx, seqs, ids, blobs, DEFAULTS, **kw)
    check_all(out, genes_list, ids, DEFAULTS)


def test_model_per_contig(lib, ctx):
    models = benchdata.load_model_set()
    tinfs = [lib.TrainingInfo(raw=b) for _, b in models[:4]]
    seqs = [synthetic_contig(80_000 + 5000 * i, 0.35 + 0.05 * i, 900 + i) for i in range(8)]
    choice = [tinfs[i % 4] for i in range(8)]
    genes_list = lib.GeneFinder().find_genes_batch(seqs, training_infos=choice)
    ids = ["g%d" % i for i in range(8)]
    moc = np.array([i % 4 for i in range(8)], np.int32)
    _, out = device_render(ctx, seqs, ids, [t.raw for t in tinfs], DEFAULTS, model_of_contig=moc)
    check_all(out, genes_list, ids, DEFAULTS)


def test_flagged_lines_are_rendered_by_the_host(lib, ctx):
    """A margin that flags (nearly) every GFF line: the host renders them and splices them in, the text is unchanged."""
    from oracle import oracle as orc
    recs = read_fasta("MIIJ01000039.fna.gz")
    seqs = [s for _, s in recs]
    ids = [h.split()[0] for h, _ in recs]
    tinf = lib.TrainingInfo(raw=orc.Oracle(seqs[0]).train().tobytes())
    genes_list = lib.GeneFinder(tinf).find_genes_batch(seqs)
    _, out = device_render(ctx, seqs, ids, [tinf.raw], {"gff": {}}, fallback_margin=1.0)
    assert out["gff"].fallback > 0
    assert out["gff"].data == host_text(genes_list, ids, "gff")


def test_bad_arguments(lib, ctx):
    tinf = lib.TrainingInfo.load(golden_path("SRR492066.training.bin.gz"))
    seqs = [synthetic_contig(50_000, 0.3, 5)]
    with pytest.raises(ValueError):
        device_render(ctx, seqs, ["a"], [tinf.raw], {"faa": {"width": 0}})
    with pytest.raises(ValueError):
        device_render(ctx, seqs, ["a"], [tinf.raw], {"faa": {"translation_table": 7}})
    with pytest.raises(ValueError):
        device_render(ctx, seqs, ["a", "b"], [tinf.raw], DEFAULTS)
