"""The inputs of tests/test_start_score_gpu.py hold what they claim to hold: checked with the CPU oracle alone (tests/start_shapes.py
builds them).  Every population a threshold of the start scorer separates is asserted here, so that the GPU test compares node
fields on inputs that are known to reach both sides of it."""
import math

import numpy as np
import pytest

from oracle import oracle as orc
from tests import sets_ref as sr
from tests import start_shapes as ss
from tests.orf_shapes import T_STOP

UPS_COMP = 80 + 28 * 8                      # offset of ups_comp[32][4] in struct _training
DIGIT = {65: 0, 71: 1, 67: 2, 84: 3}        # A G C T
COMP = {65: 84, 84: 65, 67: 71, 71: 67}


@pytest.fixture(scope="module")
def models():
    return ss.base_models()


def staged(seq, stage, tinf=None, closed=False, is_meta=False, min_gene=90, min_edge_gene=60):
    """oracle_stage of tests/test_stages_gpu.py (that module is marked gpu as a whole)."""
    o = orc.Oracle(seq)
    o.extract(tinf.trans_table if tinf is not None else 11, orc.Params(closed=closed, min_gene=min_gene, min_edge_gene=min_edge_gene))
    o.sort()
    if stage >= 2:
        o.reset_scores()
        o.score_nodes(tinf, closed, is_meta)
    return o.nodes()


# ---- end_series ---------------------------------------------------------------------------------------------------------------------------

def test_end_series_covers_every_distance():
    assert set(ss.END_U) == set(range(48)) | set(range(60, 67))
    series = ss.end_series()
    assert len(series) == 2 * len(ss.END_SEEDS) * len(ss.END_U)
    for closed in (False, True):
        for kind, u, strand, s in series:
            nd = staged(s, 1, closed=closed)             # (after extraction: scoring with open ends turns the starts at u <= 2 into edge nodes)
            d = ss.start_distance(nd, len(s))
            hit = np.flatnonzero((d == u) & (nd["strand"] == strand) & (nd["edge"] == 0))
            assert len(hit) == 1, (kind, u, strand)
            assert ss.orf_lengths(nd)[hit[0]] == 3 * (ss.END_CODONS + 1)
    # with open ends some of these ORFs reach the end of the contig (an edge node shares them) and some meet a stop codon first
    shared = {kind: 0 for kind in ss.END_SEEDS}
    for kind, u, strand, s in series:
        nd = staged(s, 1)
        i = int(np.flatnonzero((ss.start_distance(nd, len(s)) == u) & (nd["strand"] == strand) & (nd["edge"] == 0))[0])
        shared[kind] += int(np.any((nd["edge"] == 1) & (nd["type"] != T_STOP) & (nd["stop_val"] == nd["stop_val"][i]) & (nd["strand"] == strand)))
    assert all(0 < v < 2 * len(ss.END_U) for v in shared.values()), shared


@pytest.mark.parametrize("closed", [False, True])
def test_end_series_sd_bins(models, closed):
    """Under the SD model: bins other than 0 at five or more distances below 20 -- where the forward strand skips windows and the reverse
    strand searches them with bases missing -- and from 20 on, on both strands."""
    for strand in (1, -1):
        hit = set()
        for kind, u, st, s in ss.end_series():
            if st != strand:
                continue
            nd = staged(s, 2, models["sd"], closed=closed)
            d = ss.start_distance(nd, len(s))
            for i in np.flatnonzero((d >= 0) & (nd["strand"] == strand) & (nd["rbs"].max(axis=1) > 0)):
                hit.add(int(d[i]))
        assert len([u for u in hit if u < 20]) >= 5 and any(20 <= u < 70 for u in hit), (strand, sorted(hit))


@pytest.mark.parametrize("closed", [False, True])
def test_end_series_motifs(models, closed):
    """Under the model with a full motif table: every motif length, motifs and `no motif` below 21 bases from the end.  Under the non-SD
    model of the coding-score tests every start is `no motif` or a 4- or 5-base motif (its table holds nothing else)."""
    for strand in (1, -1):
        lens, near_len, near_none, far = set(), set(), set(), set()
        for kind, u, st, s in ss.end_series():
            if st != strand:
                continue
            nd = staged(s, 2, models["motif"], closed=closed)
            d = ss.start_distance(nd, len(s))
            for i in np.flatnonzero((d >= 0) & (nd["strand"] == strand) & (nd["edge"] == 0)):
                lens.add(int(nd["mot_len"][i]))
                if kind == "far" and d[i] == u and (nd["mot_len"][i], nd["mot_spacer"][i], nd["mot_ndx"][i]) == (6, 15, ss.FAR_MOTIF_INDEX):
                    assert nd["mot_score"][i] == ss.FAR_MOTIF_WEIGHT
                    far.add(u)
                if d[i] < 21:
                    near_len.add(int(nd["mot_len"][i]))
                    if nd["mot_score"][i] == models["motif"].no_mot:
                        near_none.add(int(d[i]))
            kk = staged(s, 2, models["nonsd"], closed=closed)
            assert set(kk["mot_len"].tolist()) <= {0, 4, 5}
        assert {3, 4, 5, 6} <= lens and len(near_len - {0}) >= 3 and len(near_none) >= 5, (strand, lens, near_len, near_none)
        # the candidate 21 bases upstream wins from the first distance at which it lies inside the contig
        assert far == {u for u in ss.END_U if u >= 21}, (strand, sorted(far))


# ---- orf_series ---------------------------------------------------------------------------------------------------------------------------

def test_orf_series_lengths(models):
    series = ss.orf_series()
    assert {len(s) for tag, _, s in series if tag[0] == "length"} == set(ss.CONTIG_LENGTHS)
    assert {len(s) for tag, _, s in series if tag[0] == "edge"} == {L for L, _ in ss.EDGE_CASES}
    for min_gene, min_edge in ((90, 60), (ss.ORF_MIN_GENE, ss.ORF_MIN_EDGE_GENE)):
        seen = {1: set(), -1: set()}
        for closed in (False, True):
            for tag, strand, s in series:
                if tag[0] != "length":
                    continue
                nd = staged(s, 1, closed=closed, min_gene=min_gene, min_edge_gene=min_edge)
                ok = (nd["type"] != T_STOP) & (nd["edge"] == 0) & (nd["strand"] == strand)
                have = set(ss.orf_lengths(nd)[ok].tolist()) & set(ss.ORF_LENGTHS)
                assert {117, 120, 123, 249, 252} <= have, (tag, strand, closed)
                seen[strand] |= have
        assert seen[1] == seen[-1] == set(ss.ORF_LENGTHS)
    assert min(ss.ORF_LENGTHS) + 3 == ss.ORF_MIN_GENE          # one base more and the shortest ORF has no start node


@pytest.mark.parametrize("model", ss.MODEL_NAMES)
def test_orf_series_meta_penalties(models, model):
    """Meta mode: starts with a negative coding score whose ORF has no stop codon, in contigs up to and above 1500 bases (sscore loses
    10.31 - 0.004 L or st_wt), and edge nodes with a negative coding score on both sides of 5 sqrt(L) -- the equality included."""
    tinf = models[model]
    below, above = 0, 0
    for tag, strand, s in ss.orf_series():
        nd = staged(s, 2, tinf, is_meta=True)
        if tag[0] == "length":
            n = sum(1 for i in ss.open_orf_starts(nd) if nd["cscore"][i] < 0)
            below, above = below + (n if len(s) <= 1500 else 0), above + (n if len(s) > 1500 else 0)
            assert n > 0, (tag, strand)
        else:
            _, L, orf, gc = tag
            e = np.flatnonzero((nd["type"] != T_STOP) & (nd["edge"] == 1) & (nd["strand"] == strand) & (ss.orf_lengths(nd) == orf))
            assert len(e) == 1 and nd["cscore"][e[0]] < 0, tag
            mml = math.sqrt(L) * 5.0
            assert mml == int(mml) and (nd["sscore"][e[0]] == 0.0) == (orf >= mml), tag
    assert below >= 4 and above >= 4                 # either strand of 1499 and 1500; of 1501 and longer
    assert any(orf == 5 * math.sqrt(L) for L, orfs in ss.EDGE_CASES for orf in orfs)


# ---- scan_series --------------------------------------------------------------------------------------------------------------------------

def upstream_sum(tinf, seq, nodes, i):
    """ref: lib.pyx:1618-1650, term by term in the reference's order."""
    ups = tinf.buf[UPS_COMP:UPS_COMP + 32 * 4 * 8].view(np.float64).reshape(32, 4)
    L, strand = len(seq), int(nodes["strand"][i])
    start = int(nodes["ndx"][i]) if strand == 1 else L - 1 - int(nodes["ndx"][i])
    u, cnt = 0.0, 0
    for k in list(range(1, 3)) + list(range(15, 45)):
        if k > start:
            break
        p = start - k
        b = DIGIT[seq[p]] if strand == 1 else DIGIT[COMP[seq[L - 1 - p]]]
        u += 0.4 * tinf.st_wt * float(ups[cnt][b])
        cnt += 1
    return u


def scan_populations(nodes, strand):
    """(start nodes of the ORF open at the contig's upstream end that are no edge nodes, their node distance from that end)"""
    n = len(nodes)
    e = np.flatnonzero((nodes["edge"] == 1) & (nodes["type"] != T_STOP) & (nodes["strand"] == strand))
    plain = (nodes["type"] != T_STOP) & (nodes["strand"] == strand) & (nodes["edge"] == 0)
    sv = max(nodes["stop_val"][e].tolist(), key=lambda v: int(np.count_nonzero(plain & (nodes["stop_val"] == v))))     # the planted ORF
    same = np.flatnonzero(plain & (nodes["stop_val"] == sv))
    return same, (same if strand == 1 else n - 1 - same)


@pytest.mark.parametrize("variant", list(ss.SCAN_PREFIXES))
@pytest.mark.parametrize("strand", [1, -1])
def test_scan_series_500_nodes(models, variant, strand):
    tinf = models["sd"]
    seq = ss.scan_contig(variant, strand)
    nd = staged(seq, 2, tinf)
    same, dist = scan_populations(nd, strand)
    assert len(same) > 550 and np.all(ss.orf_lengths(nd)[same][(dist >= 490) & (dist <= 510)] >= 250)
    assert any(497 <= d <= 499 for d in dist) and any(500 <= d <= 503 for d in dist)
    # The node the ORF shares is an edge node from extraction on ("edge"), or a start at ndx <= 2 that scoring converts ("conv0",
    # "conv2"): on the reverse strand that node comes after the starts that look for it, so a first scoring pass does not see it.
    first = staged(seq, 1)
    firsts = first[(first["type"] != T_STOP) & (first["strand"] == strand) & ((first["ndx"] <= 2) | (first["ndx"] >= len(seq) - 3))]
    assert (variant == "edge") == bool(np.any(firsts["edge"] == 1) and np.all(firsts["edge"][firsts["stop_val"] == nd["stop_val"][same[0]]] == 1))
    seen = variant == "edge" or strand == 1
    near, far = same[(dist >= 497) & (dist <= 499)], same[(dist >= 500) & (dist <= 503)]
    for pop, minus in ((near, seen), (far, False)):
        for i in pop:
            u = upstream_sum(tinf, seq, nd, i)
            if minus:
                u += -1.00 * tinf.st_wt
            assert np.float64(u).view(np.uint64) == nd["uscore"][i:i + 1].view(np.uint64)[0], (variant, strand, int(i))
    # the same upstream bases in both populations: the two differ by that term alone
    assert len({np.float64(upstream_sum(tinf, seq, nd, i)).view(np.uint64) for i in list(near) + list(far)}) == 1
    # without open ends nothing is shared
    closed = staged(seq, 2, tinf, closed=True)
    assert not np.any(closed["edge"][closed["type"] != T_STOP])
    planted = np.flatnonzero((closed["type"] != T_STOP) & (closed["strand"] == strand) & (closed["stop_val"] == nd["stop_val"][same[0]]) &
                             (ss.orf_lengths(closed) >= 250))
    assert len(planted) > 500
    for i in planted[::25]:
        assert np.float64(upstream_sum(tinf, seq, closed, i)).view(np.uint64) == closed["uscore"][i:i + 1].view(np.uint64)[0]


# ---- tile_series --------------------------------------------------------------------------------------------------------------------------

def tile_starts(batch, models):
    by_table = {}
    for tt in {m.trans_table for m in models}:
        by_table[tt] = []
        for s in batch:
            o = orc.Oracle(s)
            o.extract(tt, orc.Params())
            by_table[tt].append(int(np.count_nonzero(o.nodes()["type"] != T_STOP)))
    return [by_table[m.trans_table] for m in models]


@pytest.mark.parametrize("mode", ["model_of_contig", "meta"])
def test_tile_series_cuts(models, mode):
    batch, lm = ss.tile_series(), ss.listed_models(models)
    assert 600 < len(batch) < 720 and max(len(s) for s in batch) < 25000
    assert batch.count(b"") >= 2 and b"ATG" in batch and b"N" * 500 in batch
    assert sum(1 for s in batch if 120 <= len(s) <= 400) == 600
    starts = tile_starts(batch, lm)
    assert sum(1 for n in starts[0] if n == 0) >= 5 and max(starts[0]) > 1024
    if mode == "meta":
        of = {m: [] for m in range(len(lm))}
        for c, s in enumerate(batch):
            if len(s) >= 3:
                for m in sr.models_in(sr.gc_count(s) / len(s), lm):
                    of[m].append(c)
    else:
        moc = ss.model_of_contig(len(batch))
        of = {m: [c for c in range(len(batch)) if moc[c] == m] for m in range(len(lm))}
    assert all(starts[ss.LISTED_UNUSED][c] == 0 for c in of[ss.LISTED_UNUSED])         # a model without an item between models with items
    assert all(any(starts[m][c] for c in of[m]) for m in range(len(lm)) if m != ss.LISTED_UNUSED)
    assert {lm[m].trans_table for m in of if of[m]} == {4, 11} and {lm[m].uses_sd for m in of if of[m]} == {0, 1}
    most = 0
    for tile in ss.TILE_SIZES:
        lay = ss.tile_layout(starts, of, tile)
        longer = [(m, c) for m, (chains, _) in lay.items() for c, _, n in chains if n > tile]
        assert longer, tile                                                              # cut in any order of the model's chains
        cut = [(m, c) for m, (chains, _) in lay.items() for c, a, n in chains if a // tile != (a + n - 1) // tile]
        assert len(cut) > len(longer), tile                                              # ... and short chains across a boundary
        # a long chain shares its first and its last tile with other chains
        assert any(a % tile != 0 and (a + n) % tile != 0 and chains[-1][0] != c for m, (chains, _) in lay.items() for c, a, n in chains if n > tile)
        most = max(most, max(max(t) for _, t in lay.values() if t))
    assert most > 100
    if mode == "model_of_contig":
        # SsMmChain::rdelta (an item's place among the records of k_start_prologue, which lie in contig order, minus its place in the
        # model-major order): other than 0 for nearly every chain and of either sign, so an item read without it reads another start.
        # Per translation table, as the launches go: a contig has records where its model's table is extracted.
        lay = ss.tile_layout(starts, of, 1024)
        for tt in (4, 11):
            ms = [m for m in range(len(lm)) if lm[m].trans_table == tt]
            rank, at = {}, 0
            for c in range(len(batch)):
                if moc[c] in ms:
                    rank[c], at = at, at + starts[moc[c]][c]
            rdelta, base = [], 0
            for m in ms:
                rdelta += [rank[c] - (base + a) for c, a, _ in lay[m][0]]
                base += sum(n for _, _, n in lay[m][0])
            if len(ms) > 1:
                assert sum(1 for r in rdelta if r != 0) >= 0.9 * len(rdelta) and len(rdelta) > 300
                assert min(rdelta) < -500 and max(rdelta) > 500
            else:
                assert not any(rdelta) and len(rdelta) > 50            # one model: the model-major order is the contig order
