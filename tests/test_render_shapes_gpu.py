"""The device renderer (Context.render_genes, render.hip) on the records of tests/render_shapes.py: every line, record and number
at its edges, byte for byte against the host writers, with the exact count of lines left to the host; and the refusals of
pga_render_genes that keep the kernels inside the sequence.  tests/test_render_shapes_cpu.py proves what the cases contain."""
import numpy as np
import pytest

from tests import render_shapes as rs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


def render(ctx, case, formats=None, genes=None, contigs=None, moc=None, **kw):
    ctx.set_models(case.blobs)
    b = ctx.upload(case.seqs)
    try:
        if case.circular is not None:
            b.set_circular(case.circular)
        res = rs.Records(case.contigs if contigs is None else contigs, case.genes if genes is None else genes)
        return ctx.render_genes(b, res, case.ids, case.formats if formats is None else formats, meta=case.meta,
                                model_of_contig=case.moc if moc is None else moc, descriptions=case.descriptions,
                                first_seqnum=case.first_seqnum, seqnums=case.seqnums, **kw)
    finally:
        b.close()


def first_difference(got, want):
    a, w = got.split(b"\n"), want.split(b"\n")
    k = next((i for i in range(min(len(a), len(w))) if a[i] != w[i]), min(len(a), len(w)))
    return "line %d:\n device %r\n host   %r" % (k, a[k][:300] if k < len(a) else None, w[k][:300] if k < len(w) else None)


def check(case, out):
    for fmt in case.formats:
        per_contig, want = rs.host_text(case, fmt)
        got = out[fmt]
        flags = rs.expected_flags(case, fmt) if fmt in ("gff", "faa", "fna") else []
        assert case.built_flagged or not flags
        assert got.fallback == len(flags), (case.name, fmt, got.fallback, len(flags))
        assert got.data == want, "%s %s differs at %s" % (case.name, fmt, first_difference(got.data, want))
        off = np.concatenate([[0], np.cumsum([len(t) for t in per_contig])])
        assert np.array_equal(got.contig_offsets, off), (case.name, fmt)
        for c in (0, len(per_contig) // 2, len(per_contig) - 1):
            assert got.contig(c) == per_contig[c]


@pytest.mark.parametrize("name", rs.case_names())
def test_case(ctx, name):
    case = rs.case_by_name(name)
    check(case, render(ctx, case))


def unit_lines(case, text):
    """The gene lines of a GFF text, in record order."""
    return [ln for ln in text.split(b"\n") if ln and not ln.startswith(b"#")]


@pytest.mark.parametrize("name", [c.name for c in rs.number_cases()])
def test_numbers_without_a_margin_are_printed_by_the_device(ctx, monkeypatch, name):
    """fallback_margin = 0: only what the exact printer does not cover is left to the host, so every other line -- every half, signed
    zero and carry among them -- is the device's own fmt_fixed."""
    case = rs.case_by_name(name)
    flags = rs.expected_flags(case, "gff", margin=0.0)
    out = render(ctx, case, formats={"gff": case.formats["gff"]}, fallback_margin=0.0)["gff"]
    assert out.fallback == len(flags)
    want = rs.host_text(case, "gff")[1]
    assert out.data == want, first_difference(out.data, want)
    # the same call without the host splice: the flagged lines hold the device's guess, all others are the host's text
    from pyrodigal_amd import _cabi
    monkeypatch.setattr(_cabi, "_splice_fallback", lambda self, name, opts, data, coff, *a, **k: (data, coff))
    raw = render(ctx, case, formats={"gff": case.formats["gff"]}, fallback_margin=0.0)["gff"].data
    got, ref = unit_lines(case, raw), unit_lines(case, want)
    assert len(got) == len(ref) == len(case.genes)
    skip = set(flags)
    bad = [k for k in range(len(ref)) if k not in skip and got[k] != ref[k]]
    assert not bad, (bad[:5], got[bad[0]], ref[bad[0]])
    assert all(got[k] != ref[k] for k in skip)


def test_a_confidence_of_50_is_no_midpoint(ctx):
    """A margin of 0.01 covers every hundredth, so every line whose confidence went through exp is flagged -- but for conf == 50.0,
    which the midpoint test leaves out."""
    case = rs.confidence_case()
    flags = rs.expected_flags(case, "gff", margin=0.01)
    scores = rs.confidence_scores()
    names = [n for n in scores for _ in (1, -1)]
    unflagged = {names[k] for k in range(len(case.genes)) if k not in flags}
    assert unflagged == {"at_41", "zero", "tiny"}          # 99.99 without exp; exp(0) and exp(1e-300) are exactly 1
    out = render(ctx, case, fallback_margin=0.01)["gff"]
    assert out.fallback == len(flags)
    assert out.data == rs.host_text(case, "gff")[1]


@pytest.mark.parametrize("header", [True, False])
def test_scores(ctx, header):
    """The start-score file of the scores family against Genes.write_scores restated (render_shapes.scores_text) over the host copy
    of the same context's nodes."""
    seqs, ids = rs.scores_contigs()
    t = rs.base_model()
    ctx.set_models([t.tobytes()])
    b = ctx.upload(list(seqs))
    try:
        nodes = ctx.find_genes(b, meta=False, want_nodes=True).nodes
        r = ctx.find_genes(b, meta=False, want_nodes="device")
        out = ctx.render_genes(b, r, list(ids), {"scores": {"header": header}})["scores"]
    finally:
        b.close()
    per_contig = [rs.scores_text(nodes[c], t, c + 1, len(seqs[c]), ids[c], header).encode() for c in range(len(seqs))]
    assert [nodes[c]["n"] == 0 for c in range(len(seqs))] == [True] + [False] * (len(seqs) - 2) + [True]
    assert out.fallback == 0
    want = b"".join(per_contig)
    assert out.data == want, first_difference(out.data, want)
    assert np.array_equal(out.contig_offsets, np.concatenate([[0], np.cumsum([len(x) for x in per_contig])]))


def test_circular_batches_refuse_genbank_and_scores(ctx):
    case = rs.circular_case()
    for fmt in ("gbk", "scores"):
        with pytest.raises(ValueError, match="circular"):
            render(ctx, case, formats={fmt: {}})


# ---- refusals: ValueError before any kernel runs ------------------------------------------------------------------------------------------

def refusal_case():
    return rs.circular_case()


def edited(case, k, **fields):
    g = case.genes.copy()
    for name, v in fields.items():
        g[name][k] = v
    return g


def linear_gene(case):
    return int(case.contigs["gene_begin"][1])


def test_refuses_begin_0(ctx):
    case = refusal_case()
    with pytest.raises(ValueError, match="outside its contig"):
        render(ctx, case, genes=edited(case, linear_gene(case), begin=0))


def test_refuses_end_before_begin(ctx):
    case = refusal_case()
    k = linear_gene(case)
    with pytest.raises(ValueError, match="outside its contig"):
        render(ctx, case, genes=edited(case, k, begin=10, end=9))


def test_refuses_end_beyond_a_linear_contig(ctx):
    case = refusal_case()
    with pytest.raises(ValueError, match="outside its contig"):
        render(ctx, case, genes=edited(case, linear_gene(case), end=len(case.seqs[1]) + 1))


def test_refuses_a_gene_longer_than_the_circle(ctx):
    case = refusal_case()
    n = len(case.seqs[0])
    with pytest.raises(ValueError, match="outside its contig"):
        render(ctx, case, genes=edited(case, 0, begin=3, end=3 + n))
    with pytest.raises(ValueError, match="outside its contig"):
        render(ctx, case, genes=edited(case, 0, begin=n + 1, end=n + 5))          # begins beyond the circle


def test_refuses_rbs_28(ctx):
    case = refusal_case()
    for side in (0, 1):
        g = case.genes.copy()
        g["rbs"][3, side] = 28
        with pytest.raises(ValueError, match="outside its contig"):
            render(ctx, case, genes=g)


def test_refuses_a_wrong_contig(ctx):
    case = refusal_case()
    for wrong in (1, -1, 2):
        with pytest.raises(ValueError, match="outside its contig"):
            render(ctx, case, genes=edited(case, 0, contig=wrong))


def test_refuses_gene_begin_off_by_one(ctx):
    case = refusal_case()
    for c, d in ((1, 1), (1, -1), (0, 1)):
        ct = case.contigs.copy()
        ct["gene_begin"][c] += d
        with pytest.raises(ValueError, match="do not tile"):
            render(ctx, case, contigs=ct)


def test_refuses_n_genes_that_do_not_sum(ctx):
    case = refusal_case()
    for d in (1, -1):
        ct = case.contigs.copy()
        ct["n_genes"][1] += d
        with pytest.raises(ValueError, match="do not tile"):
            render(ctx, case, contigs=ct)
    ct = case.contigs.copy()
    ct["n_genes"][0] = -1
    with pytest.raises(ValueError, match="do not tile"):
        render(ctx, case, contigs=ct)


def test_refuses_a_model_out_of_range(ctx):
    case = refusal_case()
    for m in (len(case.blobs), -2):
        with pytest.raises(ValueError, match="model index"):
            render(ctx, case, moc=np.array([0, m], np.int32))
    with pytest.raises(ValueError, match="no model"):
        render(ctx, case, moc=np.array([0, -1], np.int32))


def test_refuses_a_width_of_0(ctx):
    case = refusal_case()
    for fmt in ("faa", "fna"):
        with pytest.raises(ValueError, match="width"):
            render(ctx, case, formats={fmt: {"width": 0}})
