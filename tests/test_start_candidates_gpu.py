"""Every candidate start site of a gene's ORF left on the device as tensors (pga_start_plan_create / pga_start_plan_write,
StartCandidates, Context.start_candidates, GeneFinder.find_starts_batch).

Every expected value is exact: the plain-Python rule (tests/start_candidates_ref.py) applied to the host node arrays of the existing
``want_nodes=True`` path -- never the code under test -- and compared bit for bit, float64 as it is and float32 after one
``astype(np.float32)``.  Device memory comes from tests/hip_mem.py (no torch) with the canary scheme of test_gene_windows_gpu.py, but for
the one torch test, which runs in a child process.

Two cases that a test of key collisions and open ends would want cannot occur on a linear contig; the test asserts the nearest
thing that can:
* a forward and a reverse ORF with the SAME stop_val: a forward stop codon begins at stop_val with a T, the triplet of a reverse stop
  ends there with an A (TTA, CTA, TCA), and an ORF that ends at the edge of the contig lies on the far side of any stop codon of the
  other strand with that value.  The nearest keys that can occur are a forward ORF with stop_val S and a reverse one with S + 1
  (... C TAA ...: CTA is the reverse TAG), which differ in both fields of the key;
* an edge start node whose stop_val lies outside [0, L): with open ends the extraction pulls the last codon of every frame inside
  the contig before it meets a start, so only stop nodes carry such values, and a stop node is no record.  The open-end case asserts
  the edge starts of both ends, whose ORFs end at the contig's edges, and a gene that runs off the end."""
import ctypes
import gzip
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hip_mem
from tests.start_candidates_ref import FIELDS, start_candidates_ref
from tests.util import golden_path, synthetic_contig

pytestmark = pytest.mark.gpu

CANARY = 0xA5
INDEX = {"int32": np.int32, "int64": np.int64}
SCORE = {"float32": np.float32, "float64": np.float64}
PAD, SCORE_PAD = -100, -1.0e9
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rc(s):
    return s.translate(COMP)[::-1]


# ---- the batch: 12 contigs of a few kbp at most, written here --------------------------------------------------------------------------
BIG, MID = b"ATG" * 300 + b"TAA", b"ATG" * 100 + b"TAA"          # an ORF of ATG repeats closed by a stop: a candidate every codon
LONG_ROWS = synthetic_contig(200, 0.5, 1) + BIG + synthetic_contig(150, 0.5, 2) + rc(MID) + synthetic_contig(120, 0.5, 3) + MID + \
    synthetic_contig(100, 0.5, 4) + rc(BIG) + synthetic_contig(210, 0.5, 5)
# a forward ORF that ends ... GCC TAA and a reverse ORF whose stop is the CTA of that C TAA: stop_val S and S + 1
JUNCTION = synthetic_contig(90, 0.5, 6) + b"TAA" + b"ATG" + b"GCA" * 20 + b"ATG" + b"GCA" * 30 + b"GCC" + b"TA" + b"AGC" * 35 + b"CAT" + \
    b"AGC" * 5 + b"CAT" + b"TTA" + synthetic_contig(80, 0.5, 7)
NO_NODES = b"ACGT" * 12 + b"AC"                                  # 50 bases: too short for any node
# open in all six frames, with starts near both ends: edge start nodes on either side, and genes that run off the ends
OPEN_ENDS = b"GCA" * 40 + b"ATGGCA" * 5 + b"GCA" * 40 + rc(b"ATGGCA" * 5) + b"GCA" * 3
SEQS = [LONG_ROWS, JUNCTION, JUNCTION, NO_NODES, OPEN_ENDS] + \
    [synthetic_contig(n, gc, 40 + k) for k, (n, gc) in enumerate(((4000, 0.5), (2500, 0.35), (3100, 0.65), (1999, 0.5), (4500, 0.45), (2800, 0.6),
                                                                 (3333, 0.55)))]


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi, benchdata
    c = _cabi.Context(0)
    c.set_models([b for _, b in benchdata.load_model_set()])
    yield c
    c.close()


@pytest.fixture(scope="module")
def other():
    """A second context for the calls that replace the recorded result: `ctx` keeps the arena of `called` for the whole module."""
    from pyrodigal_amd import _cabi, benchdata
    c = _cabi.Context(0)
    c.set_models([b for _, b in benchdata.load_model_set()])
    yield c
    c.close()


@pytest.fixture(scope="module")
def called(ctx):
    """The batch, its meta-mode result with the host node arrays (the reference's input), the arena on record on `ctx`."""
    assert len(SEQS) == 12
    batch = ctx.upload(SEQS)
    res = ctx.find_genes(batch, meta=True, want_nodes=True)
    yield batch, res
    batch.close()


LIVE = []


@pytest.fixture(autouse=True)
def release_device_objects():
    yield
    while LIVE:
        LIVE.pop().close()


def keep(x):
    LIVE.append(x)
    return x


class View:
    def __init__(self, ptr, shape, dtype, strides=None):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": np.dtype(dtype).str, "data": (ptr, False), "version": 3,
                                         "strides": strides}


class Target:
    """An allocation full of a fill byte and a tensor that starts ONE element into it (element-aligned, nothing more), rows a stride
    S > W apart, with `slack` elements behind the tensor: `expect()` is what the whole allocation must hold after a call.  `inner`:
    elements of one candidate (F for the scores)."""

    def __init__(self, dtype, layout, lengths, inner=None, width=None, fill=CANARY, extra_stride=5, slack=24):
        self.dtype, self.layout, self.eb, self.inner = np.dtype(dtype), layout, np.dtype(dtype).itemsize, inner or 1
        self.G, self.W = len(lengths), max(lengths, default=0) if width is None else width
        self.S = self.W + extra_stride
        self.n = ((self.G - 1) * self.S + self.W if self.G else 0) if layout == "padded" else int(sum(lengths))
        self.before = np.full((1 + self.n * self.inner + slack) * self.eb, fill, np.uint8)
        self.mem = keep(hip_mem.DeviceArray.from_numpy(self.before))
        self.ptr = self.mem.ptr + self.eb
        tail, tail_strides = ((inner,), (self.eb,)) if inner else ((), ())
        if layout == "padded":
            self.out = View(self.ptr, (self.G, self.W) + tail, dtype, (self.S * self.inner * self.eb, self.inner * self.eb) + tail_strides)
        else:
            self.out = View(self.ptr, (self.n,) + tail, dtype)

    def read(self):
        return self.mem.to_numpy(np.uint8)

    def expect(self, want):
        e = self.before.view(self.dtype).copy()
        k = self.inner
        if self.layout == "padded":
            for g in range(self.G):
                e[1 + g * self.S * k:1 + (g * self.S + self.W) * k] = want[g].ravel()
        else:
            e[1:1 + self.n * k] = want.ravel()
        return e.view(np.uint8)


def node_table(res):
    return [res.nodes[i] for i in range(len(res.nodes))]


def record_of(nodes, contig, x):
    """The gene record of start node x of a contig: what the finder would report with that start (begin / end as write_scores
    prints them)."""
    nd = nodes[contig]
    fwd = int(nd["strand"][x]) == 1
    ndx, sv = int(nd["ndx"][x]), int(nd["stop_val"][x])
    stops = [y for y in range(nd["n"]) if int(nd["type"][y]) == 3 and int(nd["strand"][y]) == int(nd["strand"][x]) and int(nd["ndx"][y]) == sv]
    return (contig, ndx + 1 if fwd else sv - 1, sv + 3 if fwd else ndx + 1, x, stops[0] if stops else 0, 1 if fwd else -1)


def gene_array(recs):
    from pyrodigal_amd import _cabi
    genes = np.zeros(len(recs), _cabi.GENE_DTYPE)
    if recs:
        for name, col in zip(("contig", "begin", "end", "start_ndx", "stop_ndx", "strand"), zip(*recs)):
            genes[name] = col
    return genes


def groups(nd):
    """{(stop_val, strand): [start nodes in ndx order]} of one contig."""
    out = {}
    for y in range(nd["n"]):
        if int(nd["type"][y]) != 3:
            out.setdefault((int(nd["stop_val"][y]), int(nd["strand"][y])), []).append(y)
    return out


def spec_of(index_dtype="int64", dtype="float32", layout="ragged", fields=FIELDS):
    from pyrodigal_amd import StartCandidates
    return StartCandidates(fields, dtype=dtype, index_dtype=index_dtype, layout=layout, pad=PAD if layout == "padded" else None,
                           score_pad=SCORE_PAD if layout == "padded" else None)


def run(ctx, batch, nodes, genes, spec, width=None):
    """One call into three Targets, the whole allocations compared with the rule's tensors; returns the DeviceStarts and the
    reference's (lengths, chosen, node indices)."""
    records = [(int(g["contig"]), int(g["start_ndx"])) for g in genes]
    pos, typ, sco, lens, chosen, ys = start_candidates_ref(nodes, records, spec.fields, spec.layout, PAD, SCORE_PAD, width, INDEX[spec.index_dtype],
                                                           SCORE[spec.dtype])
    tp, tt = (Target(INDEX[spec.index_dtype], spec.layout, lens.tolist(), None, width) for _ in range(2))
    ts = Target(SCORE[spec.dtype], spec.layout, lens.tolist(), len(spec.fields), width)
    ds = ctx.start_candidates(batch, genes, spec, out=(tp.out, tt.out, ts.out))
    assert ds.positions is tp.out and ds.types is tt.out and ds.scores is ts.out
    assert ds.lengths.dtype == np.int64 and ds.lengths.tolist() == lens.tolist() and ds.chosen.tolist() == chosen.tolist()
    assert (ds.offsets is None) if spec.layout == "padded" else (ds.offsets.tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist())
    assert tp.ptr % 16 == tp.eb or tp.eb == 16                        # element-aligned only
    for t, want, what in ((tp, pos, "positions"), (tt, typ, "types"), (ts, sco, "scores")):
        assert t.layout == "ragged" or t.S > t.W
        assert np.array_equal(t.read(), t.expect(want)), what          # the values, the pads, and the canary everywhere else
    return ds, lens, chosen, ys


# ---- 1. rows of one, of more than 64 and of more than 256 candidates; every start as a record -------------------------------------------
@pytest.mark.parametrize("layout", ["ragged", "padded"])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("index_dtype", ["int32", "int64"])
def test_every_start_of_the_long_orfs_is_a_record(ctx, called, index_dtype, dtype, layout):
    batch, res = called
    nodes = node_table(res)
    gr = groups(nodes[0])
    sizes = {strand: sorted(len(v) for (sv, s), v in gr.items() if s == strand) for strand in (1, -1)}
    for strand in (1, -1):                                             # the input holds the cases: asserted from the host nodes
        assert sizes[strand][-1] > 256 and 64 < sizes[strand][-2] <= 256, sizes
    assert min(sizes[1] + sizes[-1]) == 1
    recs = []
    for (sv, strand), ys in sorted(gr.items()):
        if len(ys) > 64 or len(ys) == 1:
            recs += [record_of(nodes, 0, y) for y in ys]               # every start node of the ORF: chosen takes every index
    ds, lens, chosen, _ = run(ctx, batch, nodes, gene_array(recs), spec_of(index_dtype, dtype, layout))
    assert lens.max() > 256 and lens.min() == 1 and len(recs) > 2 * (256 + 64)
    for strand in (1, -1):
        rows = [k for k, r in enumerate(recs) if r[5] == strand and lens[k] == sizes[strand][-1]]
        assert sorted(chosen[rows].tolist()) == list(range(sizes[strand][-1]))
    assert ds.gene_begin.tolist() == [0] + [len(recs)] * 12


def test_a_row_of_one_a_single_record_and_none(ctx, called):
    batch, res = called
    nodes = node_table(res)
    single = [ys[0] for ys in groups(nodes[0]).values() if len(ys) == 1][0]
    for layout in ("ragged", "padded"):
        ds, lens, chosen, _ = run(ctx, batch, nodes, gene_array([record_of(nodes, 0, single)]), spec_of("int32", "float64", layout))
        assert lens.tolist() == [1] and chosen.tolist() == [0]
        ds, lens, _, _ = run(ctx, batch, nodes, gene_array([]), spec_of("int64", "float32", layout))       # G = 0: nothing is written
        assert lens.tolist() == [] and ds.gene_begin.tolist() == [0] * 13 and ds.records().shape == (0,)


# ---- 2. keys the search must keep apart --------------------------------------------------------------------------------------------------
def test_neighbouring_keys_and_contigs(ctx, called):
    batch, res = called
    nodes = node_table(res)
    assert nodes[3]["n"] == 0 and all(nodes[i]["n"] > 0 for i in (0, 1, 2, 4, 11))       # a contig without nodes between records
    g1, g2 = groups(nodes[1]), groups(nodes[2])
    assert g1 == g2                                                    # the same (stop_val, strand) keys on neighbouring contigs
    fwd = {sv for sv, s in g1 if s == 1}
    near = sorted(sv for sv, s in g1 if s == -1 and sv - 1 in fwd)
    assert near and not fwd & {sv for sv, s in g1 if s == -1}          # S on + and S + 1 on -; the same value on both cannot occur
    S = near[0] - 1
    assert JUNCTION[S - 1:S + 3] == b"CTAA" and len(g1[(S, 1)]) >= 2 and len(g1[(S + 1, -1)]) >= 2
    recs = []
    for c in (2, 1):                                                   # the later contig first: records in any order
        recs += [record_of(nodes, c, y) for y in g1[(S, 1)] + g1[(S + 1, -1)]]
    first, last = groups(nodes[0]), groups(nodes[11])
    recs += [record_of(nodes, 0, min(first.values(), key=len)[0]), record_of(nodes, 11, sorted(last.items())[-1][1][-1]),
             record_of(nodes, 11, sorted(last.items())[0][1][0]), record_of(nodes, 0, sorted(first.items())[0][1][0])]
    for layout in ("ragged", "padded"):
        ds, lens, _, ys = run(ctx, batch, nodes, gene_array(recs), spec_of("int64", "float64", layout))
        assert ds.gene_begin is None                                   # not in contig order
        with pytest.raises(ValueError, match="contig order"):
            ds.starts
    k = len(g1[(S, 1)]) + len(g1[(S + 1, -1)])
    assert ys[:k] == ys[k:2 * k]                                       # the same node indices on the two contigs, each from its own rows


def test_open_ends(ctx, called):
    batch, res = called
    nodes = node_table(res)
    nd, L = nodes[4], len(OPEN_ENDS)
    edge = [y for y in range(nd["n"]) if nd["edge"][y] and nd["type"][y] != 3]
    assert {int(nd["strand"][y]) for y in edge} == {1, -1}             # edge start nodes at either end ...
    assert min(int(nd["ndx"][y]) for y in edge) <= 2 and max(int(nd["ndx"][y]) for y in edge) >= L - 3
    assert all(0 <= int(nd["stop_val"][y]) < L for y in range(nd["n"]) if nd["type"][y] != 3)       # ... (see the module's docstring)
    assert max(int(nd["stop_val"][y]) for y in edge) >= L - 5 and min(int(nd["stop_val"][y]) for y in edge) <= 4    # whose ORFs end at the edges
    mine = res.genes_of(4)
    assert len(mine) and (mine["partial_begin"].any() or mine["partial_end"].any())      # a gene that runs off the end
    recs = [record_of(nodes, 4, y) for ys in groups(nd).values() for y in ys]
    for layout in ("ragged", "padded"):
        run(ctx, batch, nodes, gene_array(recs), spec_of("int32", "float32", layout))
        run(ctx, batch, nodes, mine, spec_of("int64", "float64", layout))
    typ = start_candidates_ref(nodes, [(4, int(g["start_ndx"])) for g in mine])[1]
    assert 3 in typ.tolist()                                           # an Edge start among the candidates of the contig's genes


# ---- 3. fields ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fields", [("tscore", "total", "gc_cont"), ("gc_cont",), ("total",), ("uscore", "rscore", "sscore", "cscore"),
                                    FIELDS[::-1]], ids=lambda f: "+".join(f))
def test_field_subsets_in_any_order(ctx, called, fields):
    batch, res = called
    for dtype, layout in (("float32", "padded"), ("float64", "ragged")):
        run(ctx, batch, node_table(res), res.genes_of(5), spec_of("int64", dtype, layout, fields))


# ---- 4. the finder's own genes, subsets, orders; meta and single mode ----------------------------------------------------------------------
def test_the_genes_of_the_batch_in_any_subset_or_order(ctx, called):
    batch, res = called
    nodes = node_table(res)
    genes = np.array(res.genes)
    assert len(genes) > 30 and {1, -1} <= set(genes["strand"].tolist()) and len(set(genes["contig"].tolist())) >= 9
    ds, lens, chosen, ys = run(ctx, batch, nodes, genes, spec_of("int64", "float32", "ragged"))
    assert ds.gene_begin.tolist() == np.searchsorted(genes["contig"], np.arange(13)).tolist()
    assert lens.max() > 1 and (chosen > 0).any()
    run(ctx, batch, nodes, genes, spec_of("int32", "float64", "padded"), width=int(lens.max()) + 3)          # W above the longest row
    run(ctx, batch, nodes, genes[::-1].copy(), spec_of("int64", "float64", "padded"))
    run(ctx, batch, nodes, genes[3::7].copy(), spec_of("int32", "float32", "ragged"))
    # the result itself, and records(): the gene's record with its start replaced, node index and all
    t = [Target(np.int64, "ragged", lens.tolist()), Target(np.int64, "ragged", lens.tolist()), Target(np.float32, "ragged", lens.tolist(), 7)]
    ds = ctx.start_candidates(batch, res, spec_of(), out=tuple(x.out for x in t))
    recs = ds.records()
    assert recs.dtype == genes.dtype and len(recs) == lens.sum() and ds.records() is recs
    flat = [y for row in ys for y in row]
    assert recs["start_ndx"].tolist() == flat and recs["stop_ndx"].tolist() == np.repeat(genes["stop_ndx"], lens).tolist()
    rows = np.repeat(np.arange(len(genes)), lens)
    want_pos = [int(nodes[int(genes["contig"][g])]["ndx"][y]) + 1 for g, y in zip(rows, flat)]
    fwd = recs["strand"] == 1
    assert np.where(fwd, recs["begin"], recs["end"]).tolist() == want_pos
    assert np.where(fwd, recs["end"], recs["begin"]).tolist() == np.where(fwd, genes["end"][rows], genes["begin"][rows]).tolist()
    at = np.cumsum(lens) - lens + chosen
    assert np.array_equal(recs[at], genes)                             # the chosen candidate's record is the gene's own
    # ... and the records are records: every candidate as a record of its own gives its row again, with its own chosen
    run(ctx, batch, nodes, recs[:300].copy(), spec_of("int64", "float64", "padded"))
    assert len(ds.starts) == 12                                        # (the views themselves: the torch test)


def test_records_give_the_start_codon_of_every_candidate(ctx, called):
    from pyrodigal_amd import GeneWindows
    batch, res = called
    genes = np.array(res.genes)
    nodes = node_table(res)
    ds, lens, _, _ = run(ctx, batch, nodes, genes, spec_of("int32", "float32", "ragged"))
    recs = ds.records()
    win = GeneWindows(("start", -3), ("start", 3), pad=9, dtype="uint8", layout="padded")
    t = Target(np.uint8, "padded", [6] * len(recs))
    ctx.gene_windows(batch, recs, win, out=t.out)
    got = t.read()[1:1 + t.n + t.S - t.W].reshape(len(recs), t.S)[:, :6]
    _, typ, _, _, _, _ = start_candidates_ref(nodes, [(int(g["contig"]), int(g["start_ndx"])) for g in genes])
    codons = ["".join("ACGTN"[v] for v in row[3:6]) for row in got.tolist()]
    assert len(codons) == len(typ) and set(typ.tolist()) >= {0, 1, 2}
    for codon, kind in zip(codons, typ.tolist()):
        assert kind == 3 or codon == ("ATG", "GTG", "TTG")[kind], (codon, kind)


def test_single_mode(other):
    blob = gzip.open(golden_path(os.path.join("models", "synth_gc47_tt11.tinf.bin.gz"))).read()
    from pyrodigal_amd import benchdata
    try:
        other.set_models([blob])
        batch = keep(other.upload(SEQS[5:9] + [LONG_ROWS]))
        res = other.find_genes(batch, meta=False, want_nodes=True)
        nodes = node_table(res)
        genes = np.array(res.genes)
        assert len(genes) > 0
        for layout in ("ragged", "padded"):
            run(other, batch, nodes, genes, spec_of("int64", "float64", layout))          # the *_dp fields, as pga_result.nodes has them
        gr = groups(nodes[4])
        recs = [record_of(nodes, 4, y) for ys in gr.values() if len(ys) > 256 for y in ys[::17]]
        run(other, batch, nodes, gene_array(recs), spec_of("int32", "float32", "padded"))
    finally:
        other.set_models([b for _, b in benchdata.load_model_set()])


# ---- 5. the text path ----------------------------------------------------------------------------------------------------------------------
def test_rows_agree_with_write_scores():
    from pyrodigal_amd import lib, benchdata
    bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])
    finder = lib.GeneFinder(meta=True, metagenomic_bins=bins)
    seqs = [SEQS[0], SEQS[1], SEQS[4], SEQS[5], SEQS[6]]
    probe = finder.find_genes_batch(seqs)
    text = {}
    for i, g in enumerate(probe):                                      # {(contig, stop coordinate, strand): its rows in file order}
        f = io.StringIO()
        g.write_scores(f, "seq%d" % i, header=False)
        for line in f.getvalue().splitlines():
            c = line.split("\t")
            if len(c) == 13 and c[0] != "Beg":
                text.setdefault((i, int(c[1]) if c[2] == "+" else int(c[0]), c[2]), []).append(c)
    flat = [(i, g) for i, genes in enumerate(probe) for g in genes]
    spec = spec_of("int64", "float64", "ragged")
    # the lengths come from the text here, to size the targets: the values are compared below
    lens = [len(text[(i, g.end if g.strand == 1 else g.begin, "+" if g.strand == 1 else "-")]) for i, g in flat]
    t = [Target(np.int64, "ragged", lens), Target(np.int64, "ragged", lens), Target(np.float64, "ragged", lens, 7)]
    genes, ds = finder.find_starts_batch(seqs, spec, out=tuple(x.out for x in t))
    assert [(g.begin, g.end, g.strand) for x in genes for g in x] == [(g.begin, g.end, g.strand) for _, g in flat]
    assert ds.lengths.tolist() == lens and len(flat) > 10
    pos, typ = (x.read().view(np.int64)[1:1 + sum(lens)] for x in t[:2])
    sco = t[2].read().view(np.float64)[1:1 + 7 * sum(lens)].reshape(-1, 7)
    at = 0
    for (i, g), n in zip(flat, lens):
        rows = text[(i, g.end if g.strand == 1 else g.begin, "+" if g.strand == 1 else "-")]
        rows = rows if g.strand == 1 else rows[::-1]                  # the file runs in ndx order, a reverse row from the far end
        for k, c in enumerate(rows):
            assert int(pos[at + k]) == (int(c[0]) if g.strand == 1 else int(c[1]))
            assert ("ATG", "GTG", "TTG", "Edge")[int(typ[at + k])] == c[6]
            s = sco[at + k]
            assert ["%.2f" % s[0], "%.2f" % s[1], "%.2f" % s[2], "%.2f" % s[3], "%.2f" % s[4], "%.2f" % s[5], "%.3f" % s[6]] == \
                [c[3], c[4], c[5], c[9], c[10], c[11], c[12]], (i, k, c)
        at += n
    chosen_pos = pos[np.cumsum(lens) - np.array(lens) + ds.chosen]
    assert chosen_pos.tolist() == [g.begin if g.strand == 1 else g.end for _, g in flat]


# ---- 6. memory independence ----------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_what_memory_held(other):
    got = []
    try:
        for byte in (0x5A, 0xC3):
            other.debug_poison(byte)
            batch = keep(other.upload(SEQS[:6]))
            res = other.find_genes(batch, meta=True, want_nodes=True)
            genes = np.array(res.genes)
            ds, lens, _, _ = run(other, batch, node_table(res), genes, spec_of("int64", "float64", "padded"))
            t = [Target(np.int32, "ragged", lens.tolist()), Target(np.int32, "ragged", lens.tolist()), Target(np.float32, "ragged", lens.tolist(), 2)]
            other.start_candidates(batch, genes, spec_of("int32", "float32", "ragged", ("total", "tscore")), out=tuple(x.out for x in t))
            got.append([x.read() for x in t])
    finally:
        other.debug_poison(None)
    assert all(np.array_equal(a, b) for a, b in zip(*got))


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(ctx, other, called):
    from pyrodigal_amd import _cabi
    batch, res = called
    nodes = node_table(res)
    genes = np.array(res.genes_of(5))
    spec = spec_of("int32", "float32", "padded", ("total", "rscore"))
    lens = [len(start_candidates_ref(nodes, [(5, int(g["start_ndx"]))])[0]) for g in genes]
    G, W = len(genes), max(lens)
    S = W + 2
    need = (G - 1) * S + W
    mems = [keep(hip_mem.DeviceArray.from_numpy(np.full(4 * (need * k + 8), CANARY, np.uint8))) for k in (1, 1, 2)]
    count, chosen = np.zeros(G, np.int32), np.zeros(G, np.int32)

    def create(c=ctx, b=batch, recs=genes):
        h = ctypes.c_void_p()
        rc = c.L.pga_start_plan_create(c.h, b.h, len(recs), ctypes.c_void_p(recs.ctypes.data), ctypes.byref(h), ctypes.c_void_p(count.ctypes.data),
                                       ctypes.c_void_p(chosen.ctypes.data))
        return rc, c.L.pga_last_error(c.h).decode(), h

    def write(h, c=ctx, ptrs=None, n=None, **change):
        o = spec.opts(W, S)
        for k, v in change.items():
            if k.startswith("field_"):
                o.fields[int(k[6:])] = v
            else:
                setattr(o, k, v)
        ptrs = [m.ptr for m in mems] if ptrs is None else ptrs
        n = [need, need, 2 * need] if n is None else n
        rc = c.L.pga_start_plan_write(c.h, h, ctypes.byref(o), ctypes.c_void_p(ptrs[0]), ctypes.c_void_p(ptrs[1]), ctypes.c_void_p(ptrs[2]),
                                      n[0], n[1], n[2], None)
        return rc, c.L.pga_last_error(c.h).decode()

    def changed(k, **fields):
        g = genes.copy()
        for name, v in fields.items():
            g[name][k] = v
        return g

    stop_node = int(np.nonzero(nodes[5]["type"] == 3)[0][0])
    side = "begin" if genes["strand"][0] == 1 else "end"              # the coordinate of gene 0's start
    for what, recs, word in (("start_ndx is a stop node", changed(1, start_ndx=stop_node), "gene 1: start_ndx = %d is a stop node" % stop_node),
                             ("the wrong strand", changed(2, strand=-genes["strand"][2]), "gene 2: strand"),
                             ("a shifted begin", changed(0, **{side: genes[side][0] + 3}), "gene 0: %s = " % side),
                             ("start_ndx outside the nodes", changed(0, start_ndx=nodes[5]["n"]), "gene 0: start_ndx"),
                             ("stop_ndx outside the nodes", changed(0, stop_ndx=-1), "gene 0: stop_ndx"),
                             ("a record of the contig without nodes", changed(3, contig=3), "gene 3: start_ndx"),
                             ("a record of no contig", changed(3, contig=12), "gene 3 names contig 12")):
        rc, msg, h = create(recs=recs)
        assert rc == _cabi.PGA_EINVAL and word in msg and msg.startswith("pga_start_plan_create: ") and not h.value, (what, rc, msg)
    # no arena on record: a find that kept nothing; and a circular batch
    b2 = keep(other.upload(SEQS[5:7]))
    r2 = other.find_genes(b2, meta=True, want_nodes=False)
    rc, msg, h = create(other, b2, np.array(r2.genes))
    assert rc == _cabi.PGA_EINVAL and "no node arrays of this result on the device" in msg and not h.value
    with pytest.raises(ValueError, match="no node arrays"):
        other.start_candidates(b2, r2, spec_of())
    b3 = keep(other.upload(SEQS[5:7]))
    b3.set_circular([True, False])
    r3 = other.find_genes(b3, meta=True, want_nodes="device")
    rc, msg, h = create(other, b3, np.array(r3.genes))
    assert rc == _cabi.PGA_EINVAL and "not written for circular contigs" in msg and not h.value
    # a plan used after a second find_genes on its context
    r4 = other.find_genes(b2, meta=True, want_nodes="device")
    g4 = np.array(r4.genes)
    count, chosen = np.zeros(len(g4), np.int32), np.zeros(len(g4), np.int32)
    rc, msg, h4 = create(other, b2, g4)
    assert rc == 0, msg
    other.find_genes(b2, meta=True, want_nodes="device")
    o4 = spec_of("int32", "float32", "ragged", ("total", "rscore")).opts()
    rc = other.L.pga_start_plan_write(other.h, h4, ctypes.byref(o4), ctypes.c_void_p(mems[0].ptr), ctypes.c_void_p(mems[1].ptr),
                                      ctypes.c_void_p(mems[2].ptr), need, need, 2 * need, None)
    assert rc == _cabi.PGA_EINVAL and "no longer on record" in other.L.pga_last_error(other.h).decode()
    other.L.pga_start_plan_free(other.h, h4)
    # the write step, on a good plan
    count, chosen = np.zeros(G, np.int32), np.zeros(G, np.int32)
    rc, msg, h = create()
    assert rc == 0 and count.tolist() == lens, msg
    host = np.zeros(2 * need + 8, np.int32)
    for what, kw, word in (("W one below the longest row", dict(row_width=W - 1), "row_width = %d is less than the %d candidates of gene %d" % (W - 1, W, int(np.argmax(lens)))),
                           ("S below W", dict(row_stride=W - 1), "row_stride"),
                           ("a host pointer for positions", dict(ptrs=[host.ctypes.data, mems[1].ptr, mems[2].ptr]), "d_positions is not device memory"),
                           ("a host pointer for types", dict(ptrs=[mems[0].ptr, host.ctypes.data, mems[2].ptr]), "d_types is not device memory"),
                           ("a host pointer for scores", dict(ptrs=[mems[0].ptr, mems[1].ptr, host.ctypes.data]), "d_scores is not device memory"),
                           ("positions one element too small", dict(n=[need - 1, need, 2 * need]), "n_positions"),
                           ("types one element too small", dict(n=[need, need - 1, 2 * need]), "n_types"),
                           ("scores one element too small", dict(n=[need, need, 2 * need - 1]), "n_scores"),
                           ("index_bytes 2", dict(index_bytes=2), "index_bytes"), ("score_bytes 2", dict(score_bytes=2), "score_bytes"),
                           ("a layout that is none", dict(layout=2), "layout"), ("no fields", dict(n_fields=0), "n_fields"),
                           ("eight fields", dict(n_fields=8), "n_fields"), ("an unknown field", dict(field_1=7), "fields[1] = 7"),
                           ("a repeated field", dict(field_1=0), "fields[1] repeats fields[0]"),
                           ("an index pad beyond int32", dict(index_pad=1 << 31), "index_pad"),
                           ("a score pad beyond float32", dict(score_pad=1e39), "score_pad"),
                           ("a pointer that is not element-aligned", dict(ptrs=[mems[0].ptr + 2, mems[1].ptr, mems[2].ptr]), "d_positions is not aligned")):
        rc, msg = write(h, **kw)
        assert rc == _cabi.PGA_EINVAL and word in msg and msg.startswith("pga_start_plan_write: "), (what, rc, msg)
    with pytest.raises(TypeError, match="dtype"):                      # a wrong dtype in out=
        ctx.start_candidates(batch, genes, spec, out=(View(mems[0].ptr, (G, W), np.int64), View(mems[1].ptr, (G, W), np.int32),
                                                      View(mems[2].ptr, (G, W, 2), np.float32)))
    with pytest.raises(TypeError, match="dtype"):
        ctx.start_candidates(batch, genes, spec, out=(View(mems[0].ptr, (G, W), np.int32), View(mems[1].ptr, (G, W), np.int32),
                                                      View(mems[2].ptr, (G, W, 2), np.float64)))
    with pytest.raises(ValueError, match="not device memory"):
        ctx.start_candidates(batch, genes, spec, out=(View(host.ctypes.data, (G, W), np.int32), View(mems[1].ptr, (G, W), np.int32),
                                                      View(mems[2].ptr, (G, W, 2), np.float32)))
    with pytest.raises(ValueError, match="columns"):
        ctx.start_candidates(batch, genes, spec, out=(View(mems[0].ptr, (G, W - 1), np.int32), View(mems[1].ptr, (G, W - 1), np.int32),
                                                      View(mems[2].ptr, (G, W - 1, 2), np.float32)))
    assert np.all(host == 0) and all(np.all(m.to_numpy(np.uint8) == CANARY) for m in mems)      # nothing was written anywhere
    rc, msg = write(h)                                                 # the plan and the context run a good call afterwards
    assert rc == 0, msg
    pos, typ, sco, _, _, _ = start_candidates_ref(nodes, [(5, int(g["start_ndx"])) for g in genes], spec.fields, "padded", PAD, SCORE_PAD, W,
                                                  np.int32, np.float32)
    got = [m.to_numpy(d) for m, d in zip(mems, (np.int32, np.int32, np.float32))]
    for g in range(G):
        assert np.array_equal(got[0][g * S:g * S + W], pos[g]) and np.array_equal(got[1][g * S:g * S + W], typ[g])
        assert np.array_equal(got[2][2 * g * S:2 * (g * S + W)], sco[g].ravel())
    ctx.L.pga_start_plan_free(ctx.h, h)


# ---- 8. find_starts_batch ------------------------------------------------------------------------------------------------------------------
def test_find_starts_batch_from_host_and_device_sequences_without_kept_nodes():
    from pyrodigal_amd import DeviceSequences, _cabi, benchdata, lib
    models = benchdata.load_model_set()
    bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in models])
    seqs = SEQS[4:9]
    # the reference: the raw layer's nodes of the same sequences under the same models
    c = _cabi.Context(0)
    try:
        c.set_models([b for _, b in models])
        batch = c.upload(seqs)
        res = c.find_genes(batch, meta=True, want_nodes=True)
        nodes, raw = node_table(res), np.array(res.genes)
        batch.close()
    finally:
        c.close()
    spec = spec_of("int64", "float64", "padded", ("total", "sscore", "gc_cont"))
    pos, typ, sco, lens, chosen, ys = start_candidates_ref(nodes, [(int(g["contig"]), int(g["start_ndx"])) for g in raw], spec.fields, "padded",
                                                           PAD, SCORE_PAD, None, np.int64, np.float64)
    rows = np.full((len(seqs), max(map(len, seqs))), ord("N"), np.uint8)
    for i, s in enumerate(seqs):
        rows[i, :len(s)] = np.frombuffer(s, np.uint8)
    device = DeviceSequences(keep(hip_mem.DeviceArray.from_numpy(rows)), [len(s) for s in seqs])
    for keep_nodes in (True, False):
        finder = lib.GeneFinder(meta=True, metagenomic_bins=bins, keep_nodes=keep_nodes)
        want_genes = finder.find_genes_batch(seqs)
        for given in (seqs, device):
            t = [Target(np.int64, "padded", lens.tolist()), Target(np.int64, "padded", lens.tolist()), Target(np.float64, "padded", lens.tolist(), 3)]
            genes, ds = finder.find_starts_batch(given, spec, out=tuple(x.out for x in t))
            assert [[(g.begin, g.end, g.strand) for g in x] for x in genes] == [[(g.begin, g.end, g.strand) for g in x] for x in want_genes]
            assert [(g.begin, g.end) for x in genes for g in x] == list(zip(raw["begin"].tolist(), raw["end"].tolist()))
            assert ds.lengths.tolist() == lens.tolist() and ds.chosen.tolist() == chosen.tolist() and ds.offsets is None
            assert ds.gene_begin.tolist() == np.concatenate([[0], np.cumsum([len(x) for x in genes])]).tolist()
            for x, want in zip(t, (pos, typ, sco)):
                assert np.array_equal(x.read(), x.expect(want))
            assert (genes[0].nodes is not None) == keep_nodes
            assert ds._plan is None                                    # nothing of the finder's pooled context stays with the result
            finder.find_genes_batch(seqs[:1])                          # another request on the finder's contexts, before the records are asked for
            recs = ds.records()
            assert recs["start_ndx"].tolist() == [y for row in ys for y in row]
            assert np.where(recs["strand"] == 1, recs["begin"], recs["end"]).tolist() == pos[pos != PAD].tolist()
    # a failed request leaves no plan behind on the finder's contexts: the wrong dtype and a tensor too small are refused after the
    # plan exists (the caller cannot know T beforehand), and the requests behind them run
    import gc
    for k in range(3):
        bad = [Target(np.int64, "padded", lens.tolist()), Target(np.int64, "padded", lens.tolist()), Target(np.float32, "padded", lens.tolist(), 3)]
        with pytest.raises(TypeError, match="dtype"):
            finder.find_starts_batch(seqs, spec, out=tuple(x.out for x in bad))
        small = [Target(np.int64, "padded", lens.tolist(), None, int(lens.max()) - 1), Target(np.int64, "padded", lens.tolist(), None, int(lens.max()) - 1),
                 Target(np.float64, "padded", lens.tolist(), 3, int(lens.max()) - 1)]
        with pytest.raises(ValueError, match="columns") as caught:
            finder.find_starts_batch(seqs, spec, out=tuple(x.out for x in small))
        # while the exception and its traceback still live: the plan of the failed call is closed already
        assert caught.value is not None and not [o for o in gc.get_objects() if type(o) is _cabi._StartPlan and o.h is not None]
        del caught
        gc.collect()
        assert all(np.all(x.read() == CANARY) for x in bad + small)    # and nothing was written
    # a list that flags no contig asks for nothing circular, as in find_genes_batch
    t = [Target(np.int64, "padded", lens.tolist()), Target(np.int64, "padded", lens.tolist()), Target(np.float64, "padded", lens.tolist(), 3)]
    genes, ds = finder.find_starts_batch(seqs, spec, out=tuple(x.out for x in t), circular=[False] * len(seqs))
    assert ds.lengths.tolist() == lens.tolist() and ds._plan is None
    for x, want in zip(t, (pos, typ, sco)):
        assert np.array_equal(x.read(), x.expect(want))
    with pytest.raises(ValueError, match="not written for circular sequences"):
        finder.find_starts_batch(seqs, spec, circular=[False] * (len(seqs) - 1) + [True])
    with pytest.raises(ValueError, match="not written for circular sequences"):
        finder.find_starts_batch(seqs, spec, circular=True)
    with pytest.raises(ValueError, match="not written for circular sequences"):
        finder.find_starts_batch(seqs, spec, trim_terminal_repeats=True)


def test_find_starts_batch_refuses_a_request_that_splits():
    from pyrodigal_amd import lib
    closed = lib.TrainingInfo(raw=np.frombuffer(gzip.open(golden_path("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz")).read(), np.uint8).copy())
    srr = lib.TrainingInfo(raw=np.frombuffer(gzip.open(golden_path("SRR492066.training.bin.gz")).read(), np.uint8).copy())
    seqs = [synthetic_contig(8000, 0.5, 70 + k) for k in range(4)]
    small = lib.GeneFinder(coalesce_bases=15000)
    with pytest.raises(ValueError, match="device calls.*find_starts_batch"):
        small.find_starts_batch(seqs, spec_of(), training_infos=[(closed, srr)[i % 2] for i in range(len(seqs))])


TORCH_SCRIPT = r'''
import sys
import torch                                   # first: the library then binds to the HIP runtime of torch's wheel
if not torch.cuda.is_available():
    print("torch sees no GPU")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
import numpy as np
from pyrodigal_amd import StartCandidates, DeviceStarts, benchdata, lib

bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])
seqs = [benchdata.synthetic_contig(n, gc, 900 + i) for i, (n, gc) in enumerate(((20000, 0.4), (12345, 0.6), (61, 0.5), (30011, 0.5)))]
want_genes = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_genes_batch(seqs)
flat = [(i, g) for i, genes in enumerate(want_genes) for g in genes]
assert len(flat) > 30
side = torch.cuda.Stream()
for layout, dtype, index_dtype in (("ragged", "float32", "int32"), ("padded", "float64", "int64")):
    spec = StartCandidates(("total", "tscore"), dtype=dtype, index_dtype=index_dtype, layout=layout, pad=-1 if layout == "padded" else None,
                           score_pad=float("nan") if layout == "padded" else None)
    with torch.cuda.stream(side):
        genes, ds = lib.GeneFinder(meta=True, metagenomic_bins=bins, keep_nodes=False).find_starts_batch(seqs, spec)
    assert isinstance(ds, DeviceStarts) and all(t.is_cuda and t.device.index == 0 for t in (ds.positions, ds.types, ds.scores))
    assert ds.positions.dtype == ds.types.dtype == getattr(torch, index_dtype) and ds.scores.dtype == getattr(torch, dtype)
    assert [[(g.begin, g.end, g.strand) for g in x] for x in genes] == [[(g.begin, g.end, g.strand) for g in x] for x in want_genes]
    lens = ds.lengths.tolist()
    G, W, T = len(flat), max(lens), sum(lens)
    assert tuple(ds.positions.shape) == ((G, W) if layout == "padded" else (T,)) and tuple(ds.scores.shape) == tuple(ds.positions.shape) + (2,)
    pos, sco = ds.positions.cpu().numpy(), ds.scores.cpu().numpy()
    chosen = ds.chosen.tolist()
    for k, (i, g) in enumerate(flat):
        row = pos[k, :lens[k]] if layout == "padded" else pos[int(ds.offsets[k]):int(ds.offsets[k + 1])]
        assert int(row[chosen[k]]) == (g.begin if g.strand == 1 else g.end), "the chosen start is not the gene's"
        assert list(row) == sorted(row, reverse=g.strand != 1) and len(set(row.tolist())) == len(row)
    if layout == "padded":
        assert int((ds.positions == -1).sum()) == G * W - T and int(torch.isnan(ds.scores).sum()) == 2 * (G * W - T)
    cu = ds.cu_seqlens()
    assert cu.is_cuda and cu.dtype == torch.int32 and cu.cpu().tolist() == np.concatenate([[0], np.cumsum(lens)]).tolist()
    a, b = int(ds.gene_begin[1]), int(ds.gene_begin[2])
    p, t, s = ds.starts[1]
    if layout == "padded":
        assert tuple(p.shape) == (b - a, W) and p.data_ptr() == ds.positions[a].data_ptr() and s.data_ptr() == ds.scores[a].data_ptr()
    else:
        assert tuple(s.shape) == (sum(lens[a:b]), 2) and p.data_ptr() == ds.positions[int(ds.offsets[a]):].data_ptr()
    recs = ds.records()
    assert len(recs) == T and recs["begin"].min() >= 1
print("torch start candidates ok: %d genes" % len(flat))
'''


def test_torch_tensors_in_a_fresh_process(tmp_path):
    """torch is imported by the child alone (this process holds the library's HIP runtime and gets no second one); `out=None`
    allocates the tensors under torch's current stream.  The child says so when torch sees no GPU, and the test is skipped."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "torch_start_candidates.py"
    script.write_text(TORCH_SCRIPT)
    done = subprocess.run([sys.executable, str(script), root], timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, "child ended with %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    if "torch sees no GPU" in done.stdout:
        pytest.skip("torch sees no GPU")
    assert "torch start candidates ok" in done.stdout
