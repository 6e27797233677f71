"""The codon rules of every translation table, in the CPU oracle, against the independent statement of tests/tables_ref.py; and the
partition of the 24 tables into the classes that extract the same nodes, which tests/test_translation_tables_gpu.py relies on."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import tables_ref
from tests.util import synthetic_contig

TOPO = ["ndx", "stop_val", "type", "strand", "edge"]
STOP = 3
# the tables that extract the same nodes from CLASS_PROBE: same stop codons and same start codons wherever the probe can tell
NODE_CLASSES = [{1}, {2}, {3, 10}, {4, 5, 13, 25}, {6}, {9, 21, 24}, {11, 26}, {12}, {14}, {15, 16}, {22}, {23}, {29, 30}, {32}, {33}]

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def class_probe():
    return synthetic_contig(6145, 0.45, 5)


def codon_probe():
    return synthetic_contig(30_000, 0.45, 17)


def codon_at(seq, ndx, strand):
    """The codon a node stands on, as its strand reads it: a forward node's index is the codon's first base, a reverse node's
    index the sequence position of the codon's first base too, which is its last in sequence order."""
    if strand == 1:
        return seq[ndx:ndx + 3].decode()
    return seq[ndx - 2:ndx + 1].translate(_COMP)[::-1].decode()


def node_classes(topo_of_table):
    """{table: bytes of the node arrays} -> the sets of tables that share them, ordered by their smallest table."""
    groups = {}
    for tt in sorted(topo_of_table):
        groups.setdefault(topo_of_table[tt], set()).add(tt)
    return sorted(groups.values(), key=min)


def topo_bytes(nodes):
    return b"".join(np.ascontiguousarray(nodes[k]).astype(np.int64).tobytes() for k in TOPO)


def oracle_nodes(seq, tt, closed):
    o = orc.Oracle(seq)
    o.extract(tt, orc.Params(closed=closed))
    o.sort()
    return o.nodes()


def test_tables_ref_names_the_tables_the_library_accepts():
    from pyrodigal_amd import tables
    assert set(tables_ref.TABLES) == set(tables.TRANSLATION_TABLES) and len(tables_ref.TABLES) == 24
    from pyrodigal_amd import cli                                    # cli.py restates the set; lib.pyx does too (GPU file)
    assert set(cli.TRANSLATION_TABLES) == set(tables_ref.TABLES)


def test_tables_ref_is_consistent_with_itself():
    assert tables_ref.STANDARD["ATG"] == "M" and tables_ref.STANDARD["TGG"] == "W" and tables_ref.STANDARD["AAA"] == "K"
    assert sorted(tables_ref.STANDARD.values()).count("*") == 3
    assert tables_ref.code(11) == tables_ref.code(1) == tables_ref.STANDARD
    assert tables_ref.stop_codons(11) == {"TAA", "TAG", "TGA"} and tables_ref.stop_codons(4) == {"TAA", "TAG"}
    assert tables_ref.stop_codons(2) == {"TAA", "TAG", "AGA", "AGG"}
    assert tables_ref.stop_codons(22) == {"TAA", "TGA", "TCA"} and tables_ref.stop_codons(23) == {"TAA", "TAG", "TGA", "TTA"}
    one_stop = {tt for tt in tables_ref.TABLES if len(tables_ref.stop_codons(tt)) == 1}
    assert one_stop == {6, 14, 29, 30, 33}
    assert tables_ref.start_codons(11) == {"ATG", "GTG", "TTG"} and tables_ref.start_codons(1) == {"ATG"}
    assert tables_ref.start_codons(12) == {"ATG", "TTG"} and tables_ref.start_codons(9) == {"ATG", "GTG"}


def test_the_translator_on_a_hand_made_gene():
    #      M/L   L/T/S  S/X    stop   (reverse complement appended: the same gene on the other strand)
    gene = "TTG" "CTN" "AGN" "TAA"
    rev = gene.translate(str.maketrans("ACGTN", "TGCAN"))[::-1]
    for seq, strand in ((gene, 1), (rev, -1)):
        t = lambda tt, **kw: tables_ref.translate(seq, 1, 12, strand, False, False, tt, **kw)        # noqa: E731
        assert t(11) == "MXX*" and t(1) == "LXX*" and t(11, include_stop=False) == "MXX"
        assert t(11, strict=False) == "MLX*" and t(3, strict=False) == "LTX*" and t(12, strict=False, unknown_residue="?") == "M??*"
        assert t(5, strict=False) == "MLS*" and t(13, strict=False) == "MLX*" and t(6) == "LXXQ"
        # a partial start keeps its table reading, a partial stop keeps its last codon
        pb, pe = (True, False) if strand == 1 else (False, True)
        assert tables_ref.translate(seq, 1, 12, strand, pb, pe, 11) == "LXX*"
        assert tables_ref.translate(seq, 1, 12, strand, pe, pb, 11, include_stop=False) == "MXX*"
    # an unknown first or second base is never resolved
    assert tables_ref.translate("NCTANGGNC", 1, 9, 1, True, True, 11, strict=False) == "XXX"


@pytest.mark.parametrize("tt", tables_ref.TABLES)
def test_oracle_stop_and_start_codons_of_every_table(tt):
    seq = codon_probe()
    on = oracle_nodes(seq, tt, closed=True)
    inner = on[on["edge"] == 0]
    assert len(inner) > 100
    stops = inner[inner["type"] == STOP]
    seen = {codon_at(seq, int(n["ndx"]), int(n["strand"])) for n in stops}
    assert seen == tables_ref.stop_codons(tt)
    for strand in (1, -1):                                          # every stop codon on either strand
        assert {codon_at(seq, int(n["ndx"]), strand) for n in stops[stops["strand"] == strand]} == tables_ref.stop_codons(tt)
    seen_starts = set()
    for ty, codon in enumerate(("ATG", "GTG", "TTG")):
        got = {codon_at(seq, int(n["ndx"]), int(n["strand"])) for n in inner[inner["type"] == ty]}
        assert got == ({codon} if codon in tables_ref.start_codons(tt) else set()), (ty, got)
        seen_starts |= got
    assert seen_starts == tables_ref.start_codons(tt)


def test_the_probe_holds_every_codon_any_table_reads_as_a_stop_or_a_start():
    seq = codon_probe().decode()
    rev = seq.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    for codon in ("TAA", "TAG", "TGA", "AGA", "AGG", "TCA", "TTA", "ATG", "GTG", "TTG"):
        for s in (seq, rev):
            assert all(codon in {s[i:i + 3] for i in range(f, len(s) - 2, 3)} for f in range(3)), codon


def test_the_tables_fall_into_fifteen_classes_of_equal_nodes():
    seq = class_probe()
    got = node_classes({tt: topo_bytes(oracle_nodes(seq, tt, closed=False)) for tt in tables_ref.TABLES})
    assert got == NODE_CLASSES
    # what the classes follow from: equal stop sets and, of the start codons, equal ones
    for cls in NODE_CLASSES:
        assert len({(tables_ref.stop_codons(tt), tables_ref.start_codons(tt)) for tt in cls}) == 1
    keys = {(tables_ref.stop_codons(min(c)), tables_ref.start_codons(min(c))) for c in NODE_CLASSES}
    assert len(keys) == 15


# ---- the inputs of tests/test_translation_tables_gpu.py: what makes them tell a wrong kernel from a right one, from the oracle alone -----

@pytest.mark.parametrize("tt", tables_ref.TABLES)
def test_end_contigs_close_the_frame_exactly_under_the_tables_that_read_a_stop(tt):
    seqs, where = tables_ref.end_contigs()
    assert {len(s) % 3 for s in seqs} == {0, 1, 2} and all(600 <= len(s) <= 900 for s in seqs)
    closed_frames = 0
    for s, (codon, at, strand) in zip(seqs, where):
        assert codon_at(s, at, strand) == codon
        on = oracle_nodes(s, tt, closed=False)
        hit = on[(on["type"] == STOP) & (on["edge"] == 0) & (on["ndx"] == at) & (on["strand"] == strand)]
        assert (len(hit) == 1) == (codon in tables_ref.stop_codons(tt)), (codon, at, strand)
        closed_frames += len(hit)
    assert closed_frames == 6 * len(tables_ref.stop_codons(tt))


@pytest.mark.parametrize("tt", [11, 2, 22, 23, 6, 14])
def test_boundary_contigs_hold_their_stop_on_the_tile_border(tt):
    seqs, where = tables_ref.boundary_contigs()
    assert len(seqs) == 70
    for s, (codon, ats, strand) in zip(seqs, where):
        for closed in (False, True):
            on = oracle_nodes(s, tt, closed=closed)
            for at in ats:
                first = at if strand == 1 else at - 2                 # the codon's first base in sequence order
                assert min(abs(first + 2 - tables_ref.TILE), abs(first + 2 - 2 * tables_ref.TILE)) <= 4
                assert codon_at(s, at, strand) == codon
                hit = on[(on["type"] == STOP) & (on["edge"] == 0) & (on["ndx"] == at) & (on["strand"] == strand)]
                assert (len(hit) == 1) == (codon in tables_ref.stop_codons(tt)), (codon, at, strand, closed)


def group_conditions(seqs, models, closed=False, mask=False):
    """What a several-table call must show to reach every group's buffers: (contigs won per group, contigs won by a group other
    than the first one in their window, groups that are alone in the window of a contig they win, contigs without a model)."""
    won = tables_ref.group_winners(seqs, models, closed=closed, mask=mask)
    ng = len(tables_ref.group_order(models))
    wins = [sum(1 for _, g, _ in won if g == k) for k in range(ng)]
    later = sum(1 for _, g, seen in won if g >= 0 and g != seen[0])
    alone = {seen[0] for _, g, seen in won if g >= 0 and len(seen) == 1}
    return wins, later, alone, sum(1 for s, (_, _, seen) in zip(seqs, won) if not seen and len(s) > 1000)


@pytest.mark.parametrize("tables", [(4, 11, 15, 22), (4, 11, 22)])
def test_every_table_group_wins_contigs(tables):
    models = tables_ref.group_models(tables)
    assert tables_ref.group_order(models) == list(tables)
    sizes = [sum(1 for m in models if m.trans_table == tt) for tt in tables]
    assert sizes == ([3, 1, 5, 2] if len(tables) == 4 else [3, 1, 2])
    assert len({tables_ref.stop_codons(tt) for tt in tables}) == len(tables) and 22 in tables
    assert any(m.uses_sd == 0 for m in models) and any(m.uses_sd == 1 for m in models)
    for closed, mask in ((False, False), (True, False), (False, True)):
        seqs = tables_ref.group_contigs(unknown_runs=mask)
        assert 40 <= len(seqs) <= 50 and b"" in seqs and b"ATG" in seqs and b"N" * 400 in seqs
        wins, later, alone, no_model = group_conditions(seqs, models, closed, mask)
        assert min(wins) >= 2, wins
        assert later >= 5
        assert no_model >= 1
        assert alone == ({2, 3} if len(tables) == 4 else {2})


def test_translation_contig_genes_are_called_as_planted():
    from tests.util import golden_path
    seq, planted = tables_ref.translation_contig()
    assert 15_000 < len(seq) < 25_000
    base = orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic.tinf_closed.bin.gz"))
    t = base.copy()
    t.set_trans_table(4)
    o = orc.Oracle(seq)
    o.find_genes_single(t, orc.Params())
    genes, nodes = o.genes(), o.nodes()
    called = {(int(g["begin"]), int(g["end"]), int(nodes[g["start_ndx"]]["strand"])) for g in genes}
    kinds = {(p[2], p[3]) for p in planted if p[:3] in called}
    assert kinds == {(s, c) for s in (1, -1) for c in ("ATG", "GTG", "TTG")}
    assert {p[2] for p in planted if p[4] and p[:3] in called} == {1, -1}
    assert nodes[genes[0]["start_ndx"]]["edge"] == 1 and nodes[genes[-1]["stop_ndx"]]["edge"] == 1      # partial at either end
    for begin, end, strand, start, special in planted:
        nuc = tables_ref.gene_letters(seq, begin, end, strand)
        assert nuc[:3] == start and nuc[-3:] in ("TAA", "TAG")
        if special:
            assert nuc[3 * tables_ref.SPECIAL_AT:3 * tables_ref.SPECIAL_AT + 24] == "".join(tables_ref.SPECIAL_CODONS)
    assert any("TGA" in {tables_ref.gene_letters(seq, *p[:3])[i:i + 3] for i in range(0, p[1] - p[0], 3)} for p in planted)
    o11 = orc.Oracle(seq)
    o11.find_genes_single(base, orc.Params())
    assert o11.num_genes >= 8
