"""Every translation table, and three and four tables in one call, through the device kernels: extraction, start scoring at the
sequence ends, training and single mode against the CPU oracle bit for bit; the table groups of a meta call (their node arrays,
their interleaved coding tables, the choice across groups) against the oracle and tests/sets_ref.py; the refusals of a fifth
table; and the device and host translations against the plain translator of tests/tables_ref.py."""
import datetime
import io
import re
import warnings

import numpy as np
import pytest

from oracle import oracle as orc
from tests import sets_ref, tables_ref
from tests.test_find_genes_models_gpu import _against_oracle, _same_contig
from tests.test_finder_gpu import compare_contig
from tests.test_sets_gpu import compare_member
from tests.test_stages_gpu import check, oracle_stage
from tests.test_translation_tables_cpu import NODE_CLASSES, class_probe, group_conditions, node_classes, topo_bytes
from tests.util import golden_path, read_fasta, synthetic_contig

pytestmark = pytest.mark.gpu

TABLES = tables_ref.TABLES
GENOME = "GCF_001457455.1_NCTC11397_genomic_100kb"
DATE = datetime.date(2026, 3, 7)


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


# ---- extraction ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def extraction_batch():
    probe = class_probe()
    seqs = [probe, tables_ref.revcomp(probe)]
    seqs += [synthetic_contig(n, 0.35 + 0.03 * k, 400 + k) for k, n in enumerate((3071, 3072, 3073, 3074, 3075, 6143, 6144, 6145, 6146))]
    seqs += tables_ref.boundary_contigs()[0]
    quiet = (b"GCC" * 150 + b"ATG" + b"GCC" * 150 + b"GTG") * 13            # no stop of any table in any frame of either strand
    seqs += [synthetic_contig(2000, 0.5, 11) + b"ATG" + quiet + b"TAA" + synthetic_contig(2500, 0.45, 12), quiet[:3080],
             b"CAT" + quiet[:6200][::-1]]
    seqs += [synthetic_contig(9000, 0.25, 14), synthetic_contig(9000, 0.78, 13)]
    return seqs


@pytest.mark.parametrize("closed", [False, True])
@pytest.mark.parametrize("tt", TABLES)
def test_extraction_under_every_table(ctx, extraction_batch, tt, closed):
    from pyrodigal_amd import _cabi
    out = ctx.nodes_stage(extraction_batch, _cabi.STAGE_EXTRACT, translation_table=tt, closed=closed)
    total = 0
    for seq, nd in zip(extraction_batch, out):
        on = oracle_stage(seq, 1, tt=tt, closed=closed)
        check(nd, on, 1)
        total += len(on)
    assert total > 1000


def test_device_extraction_falls_into_the_same_fifteen_classes(ctx):
    from pyrodigal_amd import _cabi
    probe = class_probe()
    got = {}
    for tt in TABLES:
        nd = ctx.nodes_stage([probe], _cabi.STAGE_EXTRACT, translation_table=tt)[0]
        got[tt] = topo_bytes({k: nd[k] for k in ("ndx", "stop_val", "type", "strand", "edge")})
    assert node_classes(got) == NODE_CLASSES


# ---- the sequence ends in start scoring ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def end_models():
    sd = orc.Training.load(golden_path("SRR492066.training.bin.gz"))
    nonsd = orc.Oracle(read_fasta("KK037166.fna.gz")[0][1]).train()
    assert sd.uses_sd == 1 and nonsd.uses_sd == 0
    return sd, nonsd


def under_table(tinf, tt):
    t = tinf.copy()
    t.set_trans_table(tt)
    return t


@pytest.mark.parametrize("tt", TABLES)
def test_start_scores_at_the_sequence_ends_under_every_table(ctx, end_models, tt):
    seqs, where = tables_ref.end_contigs()
    for base in end_models:
        tinf = under_table(base, tt)
        ctx.set_models([tinf.buf])
        for stage in (2, 3):
            out = ctx.nodes_stage(seqs, stage)
            open_frames = closed_frames = 0
            for seq, nd, (codon, at, strand) in zip(seqs, out, where):
                on = oracle_stage(seq, stage, tinf=tinf)
                check(nd, on, stage)
                stop_here = (on["type"] == 3) & (on["ndx"] == at) & (on["strand"] == strand) & (on["edge"] == 0)
                closed_frames += int(stop_here.any())
                open_frames += int(((on["type"] == 3) & (on["strand"] == strand) & (on["edge"] == 1)).any())
            # both sides of the edge rule: frames the table closes at the last codon, and frames that run off the end
            assert closed_frames == 6 * len(tables_ref.stop_codons(tt)) and open_frames >= len(seqs) - closed_frames


@pytest.mark.parametrize("tt", [min(c) for c in NODE_CLASSES])
def test_sequence_ends_through_the_finder(ctx, end_models, tt):
    """One table of every class in single mode: the start list form of the start scorer."""
    seqs, _ = tables_ref.end_contigs()
    for base in end_models:
        tinf = under_table(base, tt)
        ctx.set_models([tinf.buf])
        res = ctx.find_genes_batch(seqs, meta=False, want_nodes=True)
        for i, s in enumerate(seqs):
            compare_contig(res, i, s, orc.Oracle(s), [tinf], meta=False)


# ---- training and single mode -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def genome():
    return read_fasta(GENOME + ".fna.gz")[0][1]


_TRAINED = {}


def device_training(ctx, genome, tt):
    if tt not in _TRAINED:
        _TRAINED[tt] = ctx.train(genome, translation_table=tt)
    return _TRAINED[tt]


@pytest.mark.parametrize("tt", TABLES)
def test_training_and_single_mode_under_every_table(ctx, genome, tt):
    want = orc.Oracle(genome).train(tt=tt)
    assert want.trans_table == tt and want.uses_sd == 1
    blob = device_training(ctx, genome, tt)
    assert blob == want.tobytes()
    ctx.set_models([blob])
    res = ctx.find_genes_batch([genome], meta=False, want_nodes=True)
    n = compare_contig(res, 0, genome, orc.Oracle(genome), [want], meta=False)
    assert 88 <= n <= 163


def test_one_training_call_with_all_tables(ctx, lib, genome):
    """One genome per table in one call of the host layer, which hands the device four tables at a time."""
    got = lib.GeneFinder().train_batch([genome] * len(TABLES), translation_table=list(TABLES))
    assert [t.translation_table for t in got] == list(TABLES)
    for tt, t in zip(TABLES, got):
        assert t.raw.tobytes() == device_training(ctx, genome, tt), tt
    # and four tables in one device call, each twice, interleaved
    tts = [23, 6, 2, 33, 6, 33, 23, 2]
    for tt, blob in zip(tts, ctx.train_batch([genome] * len(tts), translation_table=tts)):
        assert blob == device_training(ctx, genome, tt), tt


# ---- three and four table groups in one call ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[(4, 11, 15, 22), (4, 11, 22)], ids=["four_tables", "three_tables"])
def group_case(request):
    models = tables_ref.group_models(request.param)
    assert tables_ref.group_order(models) == list(request.param)
    return models


@pytest.mark.parametrize("closed,mask", [(False, False), (True, False), (False, True)], ids=["open", "closed", "masked"])
def test_meta_mode_with_several_table_groups(ctx, group_case, closed, mask):
    models = group_case
    seqs = tables_ref.group_contigs(unknown_runs=mask)
    wins, later, alone, no_model = group_conditions(seqs, models, closed, mask)
    ng = len(wins)
    assert min(wins) >= 2 and later >= 5 and no_model >= 1 and alone == ({2, 3} if ng == 4 else {2})
    ctx.set_models([m.buf for m in models])
    res = ctx.find_genes_batch(seqs, meta=True, closed=closed, want_nodes=True, mask=mask)
    total = 0
    for i, s in enumerate(seqs):
        total += compare_contig(res, i, s, orc.Oracle(s, mask=mask), models, meta=True, closed=closed)
    assert total > 100
    order = tables_ref.group_order(models)
    got = [sum(1 for m in res.contigs["model"] if m >= 0 and order.index(models[m].trans_table) == g) for g in range(ng)]
    assert got == wins


def test_sets_across_table_groups(ctx):
    """Contigs that different tables win on their own, pooled into one set: the set's one model, against tests/sets_ref.py."""
    models = tables_ref.group_models()
    seqs = tables_ref.group_contigs()
    own = tables_ref.group_winners(seqs, models)
    pick = [i for i, s in enumerate(seqs) if len(s) in (2500, 6200, 9300)]          # three contigs written in each of the four codes
    labels = []
    for i in pick:                                           # the four of 6200 bases one set, those of 2500 two pairs, the rest alone
        n = len(seqs[i])
        labels.append("mixed" if n == 6200 else "pair%d" % (sum(1 for x in labels if x and x.startswith("pair")) // 2) if n == 2500 else None)
    mixed = [own[i][1] for i, lab in zip(pick, labels) if lab == "mixed"]
    assert len(mixed) == 4 and len(set(mixed)) >= 3 and -1 not in mixed
    sub = [seqs[i] for i in pick]
    want = sets_ref.find_genes_sets(sub, labels, models)
    ctx.set_models([m.buf for m in models])
    res = ctx.find_genes_batch(sub, meta=True, want_nodes=True, sets=labels)
    assert sum(compare_member(res, i, mb, len(models)) for i, mb in enumerate(want)) > 20
    # one model for the four, whichever table each would have taken alone (a member without a path under it stays without genes)
    members = [i for i, lab in enumerate(labels) if lab == "mixed"]
    chosen = {int(res.set_models[i]) for i in members}
    assert len(chosen) == 1 and -1 not in chosen
    assert sum(1 for i in members if res.contigs[i]["model"] == min(chosen)) >= 3


def test_single_mode_with_a_model_per_contig_across_four_tables(ctx):
    models = tables_ref.group_models()
    seqs = [s for s in tables_ref.group_contigs() if len(s) <= 14000]
    moc = [(3 * i + 1) % len(models) for i in range(len(seqs))]
    assert set(moc) == set(range(len(models)))
    ctx.set_models([m.buf for m in models])
    got = ctx.find_genes_batch(seqs, meta=False, want_nodes=True, model_of_contig=moc)
    assert list(got.contigs["model"]) == moc and len(got.genes) > 50
    checked = set()
    for m, tinf in enumerate(models):
        mine = [i for i, x in enumerate(moc) if x == m]
        ctx.set_models([tinf.buf])
        want = ctx.find_genes_batch([seqs[i] for i in mine], meta=False, want_nodes=True)
        for j, i in enumerate(mine):
            _same_contig(got, i, want, j)
            if tinf.trans_table not in checked and got.contigs[i]["n_genes"] > 0:
                _against_oracle(got, i, seqs[i], tinf.tobytes())
                checked.add(tinf.trans_table)
    assert checked == {4, 11, 15, 22}


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def five_tables():
    base = orc.Training.load(golden_path("SRR492066.training.bin.gz"))
    return [under_table(base, tt) for tt in (11, 4, 22, 15, 11, 2)]


def test_a_fifth_table_is_refused_and_the_context_keeps_its_models(ctx, genome):
    kept = tables_ref.group_models()
    seq = tables_ref.coded_contig(6200, 0.5, 9003, 4)
    ctx.set_models([m.buf for m in kept])
    before = ctx.find_genes_batch([seq], meta=True)
    assert len(before.genes) > 0
    with pytest.raises(ValueError, match="more than 4 distinct translation tables"):
        ctx.set_models([m.buf for m in five_tables()])
    after = ctx.find_genes_batch([seq], meta=True)
    assert after.contigs["model"][0] == before.contigs["model"][0] and after.genes.tobytes() == before.genes.tobytes()
    compare_contig(after, 0, seq, orc.Oracle(seq), kept, meta=True)
    with pytest.raises(ValueError, match="more than 4 distinct translation tables"):
        ctx.train_batch([genome[:20000]] * 5, translation_table=[11, 4, 22, 15, 2])
    assert len(ctx.find_genes_batch([seq], meta=True).genes) == len(before.genes)


def test_a_fifth_table_through_the_host_layer(lib):
    tinfs = [lib.TrainingInfo(raw=t.tobytes()) for t in five_tables()]
    bins = lib.MetagenomicBins([lib.MetagenomicBin(t, "bin%d" % k) for k, t in enumerate(tinfs)])
    seq = tables_ref.coded_contig(6200, 0.3, 9003, 4)
    finder = lib.GeneFinder(meta=True, metagenomic_bins=bins)
    with pytest.raises(ValueError, match="more than 4 distinct translation tables"):
        finder.find_genes(seq)
    with pytest.raises(ValueError, match="more than 4 distinct translation tables"):
        finder.find_genes_batch([seq, seq])
    # a model per sequence has no such limit: the host layer splits the sequences into device calls of four tables
    seqs = [tables_ref.coded_contig(5000 + 100 * k, 0.3, 9200 + k, t.translation_table) for k, t in enumerate(tinfs)]
    single = lib.GeneFinder()
    got = single.find_genes_batch(seqs, training_infos=tinfs)
    assert single.stats["device_calls"] == 2
    for s, t, g in zip(seqs, tinfs, got):
        want = lib.GeneFinder(t).find_genes(s)
        assert g.training_info is t and len(want) > 0
        assert [(x.begin, x.end, x.strand, x.start_type, x.score) for x in g] == [(x.begin, x.end, x.strand, x.start_type, x.score) for x in want]


# ---- translation and rendering ------------------------------------------------------------------------------------------------------

OPTIONS = [dict(include_stop=True, strict=True, unknown_residue="X"), dict(include_stop=False, strict=True, unknown_residue="X"),
           dict(include_stop=True, strict=False, unknown_residue="X"), dict(include_stop=False, strict=False, unknown_residue="?")]


class Called:
    """The translation contig resident on the device and its gene calls under one model."""


@pytest.fixture(scope="module")
def called(ctx, lib):
    seq, planted = tables_ref.translation_contig()
    base = orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic.tinf_closed.bin.gz"))
    batch = ctx.upload([seq])
    out = {}
    for tt in (4, 11):
        c = Called()
        c.seq, c.planted, c.batch, c.tinf = seq, planted, batch, under_table(base, tt)
        ctx.set_models([c.tinf.buf])
        c.res = ctx.find_genes(batch, meta=False)
        c.host = lib.GeneFinder(lib.TrainingInfo(raw=c.tinf.tobytes())).find_genes(seq)
        o = orc.Oracle(seq)
        o.find_genes_single(c.tinf, orc.Params())
        assert len(c.res.genes) == o.num_genes == len(c.host) and np.array_equal(c.res.genes["begin"], o.genes()["begin"])
        assert [(g.begin, g.end, g.strand, g.partial_begin, g.partial_end) for g in c.host] == \
               [tuple(int(g[k]) for k in ("begin", "end", "strand", "partial_begin", "partial_end")) for g in c.res.genes]
        out[tt] = c
    yield out
    batch.close()


def expected(c, tt, include_stop=True, strict=True, unknown_residue="X"):
    return [tables_ref.translate(c.seq, int(g["begin"]), int(g["end"]), int(g["strand"]), bool(g["partial_begin"]), bool(g["partial_end"]),
                                 tt, include_stop=include_stop, strict=strict, unknown_residue=unknown_residue) for g in c.res.genes]


def device_proteins(ctx, c, tt, **opt):
    letters, off = ctx.translate_genes(c.batch, c.res, tables=[tt], **opt)
    text = letters.tobytes().decode("ascii")
    return [text[off[g]:off[g + 1]] for g in range(len(c.res.genes))]


@pytest.mark.parametrize("tt", TABLES)
def test_device_and_host_translation_under_every_table(ctx, called, tt):
    for c in called.values():
        assert len(c.res.genes) >= 8
        for opt in OPTIONS:
            want = expected(c, tt, **opt)
            assert device_proteins(ctx, c, tt, **opt) == want
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                # a table with other stop codons than the genes' own warns
                assert [g.translate(translation_table=tt, **opt) for g in c.host] == want


def fasta_proteins(text):
    return ["".join(rec.split("\n")[1:]) for rec in text.split(">")[1:]]


def genbank_proteins(text):
    return [re.sub(r"\s+", "", m) for m in re.findall(r'/translation="([^"]*)"', text)]


@pytest.mark.parametrize("tt", TABLES)
def test_rendered_proteins_under_every_table(ctx, called, tt):
    for c in called.values():
        ctx.set_models([c.tinf.buf])
        for include_stop, strict in ((True, True), (False, False)):
            formats = {"faa": {"translation_table": tt, "include_stop": include_stop, "strict_translation": strict},
                       "gbk": {"translation_table": tt, "strict_translation": strict, "date": DATE}}
            b = ctx.upload([c.seq])
            try:
                r = ctx.find_genes(b, meta=False)
                out = ctx.render_genes(b, r, ["ctg"], formats)
            finally:
                b.close()
            faa, gbk = io.StringIO(), io.StringIO()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                c.host.write_translations(faa, "ctg", **formats["faa"])
                c.host.write_genbank(gbk, "ctg", **formats["gbk"])
            assert out["faa"].fallback == 0 and out["gbk"].fallback == 0
            assert out["faa"].data == faa.getvalue().encode() and out["gbk"].data == gbk.getvalue().encode()
            assert fasta_proteins(out["faa"].data.decode()) == expected(c, tt, include_stop=include_stop, strict=strict)
            assert genbank_proteins(out["gbk"].data.decode()) == expected(c, tt, include_stop=False, strict=strict)


def test_the_cases_that_tell_the_tables_apart(ctx, called):
    c = called[4]
    index = {(int(g["begin"]), int(g["end"]), int(g["strand"])): k for k, g in enumerate(c.res.genes)}
    genes = c.res.genes
    assert genes[0]["partial_begin"] and genes[-1]["partial_end"]
    loose = {tt: device_proteins(ctx, c, tt, include_stop=True, strict=False, unknown_residue="?") for tt in (1, 3, 5, 11, 12, 13, 26)}
    at = tables_ref.SPECIAL_AT
    seen = set()
    for begin, end, strand, start, special in c.planted:
        k = index.get((begin, end, strand))
        if k is None:
            continue
        seen.add((strand, start, special))
        first = {tt: p[k][0] for tt, p in loose.items()}
        if start == "TTG":
            assert first[1] == "L" and first[11] == "M" and first[3] == "L" and first[12] == "M"
        if start == "GTG":
            assert first[1] == "V" and first[11] == "M" and first[12] == "V" and first[5] == "M"
        if special:                                           # CTN AGN TAN TGN ATN GCN NCT ANG
            assert loose[11][k][at] == "L" and loose[3][k][at] == "T" and loose[12][k][at] == "?" and loose[26][k][at] == "?"
            assert loose[5][k][at + 1] == "S" and loose[11][k][at + 1] == "?" and loose[13][k][at + 1] == "?"
            assert loose[11][k][at + 2:at + 8] == "???A??"
            strict = device_proteins(ctx, c, 11, include_stop=True, strict=True, unknown_residue="X")
            assert strict[k][at:at + 8] == "XXXXXXXX"
    assert {(s, x) for s, x, _ in seen} >= {(s, x) for s in (1, -1) for x in ("GTG", "TTG")}
    assert {s for s, _, sp in seen if sp} == {1, -1}
    # a gene called under table 4 holds in-frame TGA: under table 11 it shows a stop inside
    assert any("*" in p[:-1] for p in loose[11]) and not any("*" in p[:-1] for p in device_proteins(ctx, c, 4))
    # the gene cut off at the left end keeps its first codon's table reading, the one cut off at the right end its last codon
    assert device_proteins(ctx, c, 11, include_stop=False)[-1] == expected(c, 11, include_stop=False)[-1] == expected(c, 11)[-1]
