"""Every ORF walk of the coding score (k_coding_score_quads / k_coding_score, pyrodigal_amd/csrc/pipeline.hip) against the CPU
oracle's ordered f64 sums, bit for bit: at the edges of the twelve length classes, at the rounds of the walks, at the ends of a
contig and of the batch, across the cuts of a task, in tasks with 256 entries and in every column of every quad of table
columns.  tests/orf_shapes.py builds the inputs; tests/test_coding_score_cpu.py shows with the oracle alone that they hold what
they are meant to hold.  The run-time knobs move ORFs between the walks; only values the code accepts are set."""
import pytest

from oracle import oracle as orc
from tests import orf_shapes as osh
from tests import sets_ref as sr
from tests.test_sets_gpu import check_call
from tests.test_stages_gpu import check, oracle_stage
from tests.util import golden_path, read_fasta, synthetic_contig

pytestmark = pytest.mark.gpu

KNOBS = ("PGA_CS_LDS", "PGA_CS_WAVE", "PGA_CS_QCLASSES", "PGA_CS_TASK_NODES")
VARIANTS = {
    "default": {},                                                  # LDS form: orf_wave above 2048, orf_quarter 257 .. 2048, orf_serial (tables in LDS) below
    "global": {"PGA_CS_LDS": "0"},                                  # k_coding_score: orf_serial (tables in global memory) up to CS_LONG = 192, orf_wave above
    "wave64": {"PGA_CS_WAVE": "64"},                                # everything above 64 codons to orf_wave
    "nowave": {"PGA_CS_WAVE": "100000"},                            # nothing to orf_wave: the longest ORFs through orf_quarter
    "qclasses4": {"PGA_CS_QCLASSES": "4"},                          # 193 .. 256 from orf_serial to orf_quarter
    "pieces256": {"PGA_CS_TASK_NODES": "256"},                      # contigs cut into pieces of 256 nodes
    "pieces256+wave64": {"PGA_CS_TASK_NODES": "256", "PGA_CS_WAVE": "64"},
}


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def models():
    """An SD and a non-SD model, as in tests/test_stages_gpu.py."""
    sd = orc.Training.load(golden_path("SRR492066.training.bin.gz"))
    nonsd = orc.Oracle(read_fasta("KK037166.fna.gz")[0][1]).train()
    assert sd.uses_sd == 1 and nonsd.uses_sd == 0
    return {"sd": sd, "nonsd": nonsd}


@pytest.fixture
def knobs(monkeypatch):
    """Sets the knobs of a variant (the library reads them at every launch); all of them are gone again after the test."""
    def use(variant):
        for k in KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in (VARIANTS[variant] if isinstance(variant, str) else variant).items():
            monkeypatch.setenv(k, v)
    yield use
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


_INPUT, _REF = {}, {}


def contig(name):
    if "designed" not in _INPUT:
        _INPUT["designed"] = osh.designed()
        _INPUT["short"] = osh.designed_short_edges()
        _INPUT["gc35"], _INPUT["gc65"] = osh.model_contigs()[1:]
    return _INPUT[name]


def reference(key, seq, stage, tinf, model, closed, **kw):
    """The oracle's nodes of one input, computed once and shared (never written to)."""
    key = (key, stage, model, closed)
    if key not in _REF:
        _REF[key] = oracle_stage(seq, stage, tinf=tinf, closed=closed, **kw)
        _REF[key].setflags(write=False)
    return _REF[key]


def orfs_across_cuts(nodes, L, piece):
    """Per strand: the ORFs whose stop node and one of whose start nodes lie in different pieces of `piece` nodes."""
    idx, _, st = osh.orf_spans(nodes, L)
    return {s: sum(1 for i in idx[st == s] if any(k // piece != i // piece for k in osh.start_codons_of(nodes, L, i).values())) for s in (1, -1)}


# (a) -----------------------------------------------------------------------------------------------------------------------------------

def run_class_edges(ctx, models, knobs, closed, model, variant, stage=2):
    tinf = models[model]
    ctx.set_models([tinf.tobytes()])
    knobs(variant)
    names = ["designed", "gc35", "gc65"]
    out = ctx.nodes_stage([contig(n) for n in names], stage, closed=closed)
    for n, nd in zip(names, out):
        check(nd, reference(n, contig(n), stage, tinf, model, closed), stage)
    # the inputs hold what they were built to hold (from the oracle's nodes)
    seq, on = contig("designed"), reference("designed", contig("designed"), stage, tinf, model, closed)
    _, sp, st = osh.orf_spans(on, len(seq))
    for strand in (1, -1):
        assert set(osh.SPANS) - {16, 17} <= set(sp[st == strand].tolist())
    if stage == 2:
        # spans of 15 .. 18 codons have nodes only under smaller minimum gene lengths (max_overlap may not exceed min_gene)
        g = osh.SHORT_MIN_GENE
        short = ctx.nodes_stage([contig("short")], stage, closed=closed, min_gene=g, min_edge_gene=g, max_overlap=g)
        sn = reference("short", contig("short"), stage, tinf, model, closed, min_gene=g, min_edge_gene=g)
        check(short[0], sn, stage)
        _, sp, st = osh.orf_spans(sn, len(contig("short")))
        for strand in (1, -1):
            assert set(osh.SHORT_SPANS) <= set(sp[st == strand].tolist())
    if "PGA_CS_TASK_NODES" in VARIANTS[variant]:
        assert -(-len(on) // 256) == 26
        across = orfs_across_cuts(on, len(seq), 256)
        assert across[1] >= 6 and across[-1] >= 6


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("model", ["sd", "nonsd"])
@pytest.mark.parametrize("closed", [False, True])
def test_every_class_edge_under_every_walk(ctx, models, knobs, closed, model, variant):
    run_class_edges(ctx, models, knobs, closed, model, variant)


def test_every_class_edge_with_overlapping_starts(ctx, models, knobs):
    run_class_edges(ctx, models, knobs, False, "sd", "default", stage=3)


# (b) -----------------------------------------------------------------------------------------------------------------------------------

END_CODONS = (33, 34, 35, 36, 37, 300, 1100)          # every ncod mod 5 of the serial walks; the quarter and the wave walk
END_INSIDE = (0, 1, 2, 3, 5, 14, 15, 16, 17)          # bases between the contig's end and the ORF's outermost planted codon


def end_batch():
    """ORFs that run off the left end (forward) and off the right end (reverse) of their contig; such contigs first and last in
    the batch, directly before a 3-base contig and before an empty one."""
    if "ends" not in _INPUT:
        edge = [osh.end_contig(n, k, strand, 1000 * n + 10 * k + (strand == 1))
                for n in END_CODONS for k in END_INSIDE for strand in (1, -1)]
        batch = []
        for i, s in enumerate(edge):
            batch.append(s)
            if i % 7 == 1 and i + 1 < len(edge):
                batch.append(b"ATG")
            if i % 7 == 4 and i + 1 < len(edge):
                batch.append(b"")
        _INPUT["ends"] = batch
    return _INPUT["ends"]


@pytest.mark.parametrize("variant", ["default", "global", "wave64"])
def test_orfs_at_the_ends_of_a_contig_and_of_the_batch(ctx, models, knobs, variant):
    tinf = models["sd"]
    ctx.set_models([tinf.tobytes()])
    batch = end_batch()
    assert len(batch[0]) > 100 and len(batch[-1]) > 100 and b"ATG" in batch and b"" in batch
    refs = [reference(("end", i), s, 2, tinf, "sd", False) for i, s in enumerate(batch)]
    # every such contig has the ORF it was built for, with a start node where the ORF was cut
    at = 0
    for n in END_CODONS:
        for k in END_INSIDE:
            for strand in (1, -1):
                while len(batch[at]) < 100:
                    at += 1
                on, L = refs[at], len(batch[at])
                idx, sp, st = osh.orf_spans(on, L)
                hit = [i for i, x, t in zip(idx, sp, st) if t == strand and x == n + k // 3]
                assert hit and any(max(osh.start_codons_of(on, L, i), default=-1) == n + k // 3 - 1 for i in hit), (n, k, strand)
                at += 1
    knobs(variant)
    for order in (1, -1):
        out = ctx.nodes_stage(batch[::order], 2, closed=False)
        for nd, on in zip(out, refs[::order]):
            check(nd, on, 2)


# (c) -----------------------------------------------------------------------------------------------------------------------------------

def task_entries(node_counts, task_nodes):
    """pga_cs_tasks for one model: (entries, nodes, largest entry) of every task, contigs in batch order."""
    tasks, count, nodes, big = [], 0, 0, 0
    for nc in node_counts:
        for f0 in range(0, nc, task_nodes):
            piece = min(task_nodes, nc - f0)
            if count > 0 and (nodes + piece > task_nodes or count == 256):
                tasks.append((count, nodes, big)); count = nodes = big = 0
            count += 1; nodes += piece; big = max(big, piece)
    if count:
        tasks.append((count, nodes, big))
    return tasks


@pytest.mark.parametrize("task_nodes", [None, 8192])
def test_tasks_with_256_entries(ctx, models, knobs, task_nodes):
    tinf = models["sd"]
    ctx.set_models([tinf.tobytes()])
    if "many" not in _INPUT:
        small = [synthetic_contig(150 + (k * 37) % 251, 0.35 + 0.03 * ((k * 7) % 11), 9000 + k) for k in range(700)]
        _INPUT["many"] = small[:350] + [contig("designed")] + small[350:]
    batch = _INPUT["many"]
    refs = [reference(("many", i), s, 2, tinf, "sd", False) for i, s in enumerate(batch)]
    tasks = task_entries([len(on) for on in refs], task_nodes or 5120)
    full = [t for t in tasks if t[0] == 256]
    assert len(full) >= 2 and all(n < (task_nodes or 5120) for _, n, _ in full)    # full of entries before full of nodes
    assert any(c > 1 and big > 1000 for c, _, big in tasks)                         # the large contig shares a task with small ones
    # the restatement above is what the library's own planner does with these node counts
    from pyrodigal_amd import _cabi
    counts = [len(on) for on in refs]
    plan = _cabi.cs_task_summary(counts, [0] * len(counts), [1] * len(counts), task_nodes or 5120)
    assert (plan["tasks"], plan["entries"], plan["largest_task"]) == (len(tasks), sum(t[0] for t in tasks), max(t[1] for t in tasks))
    knobs({} if task_nodes is None else {"PGA_CS_TASK_NODES": str(task_nodes)})
    out = ctx.nodes_stage(batch, 2, closed=False)
    for nd, on in zip(out, refs):
        check(nd, on, 2)


# (d) -----------------------------------------------------------------------------------------------------------------------------------

_SETS = {}


def model_set_reference(size):
    if size not in _SETS:
        seqs, ms = osh.model_contigs(), osh.model_set(size)
        _SETS[size] = (seqs, ms, sr.find_genes_sets(seqs, list(range(len(seqs))), ms))
    return _SETS[size]


@pytest.mark.parametrize("variant", ["default", "global", "wave64", "pieces256"])
@pytest.mark.parametrize("size", osh.MODEL_SET_SIZES, ids=str)
def test_every_column_of_every_quad(ctx, knobs, size, variant):
    """Each contig a set of its own: the winner, the winner's node arrays (cscore among them) and the path score under every model
    of the window, as bit patterns.  A wrong value in any column of any quad changes that model's path score."""
    seqs, ms, want = model_set_reference(size)
    n = sum(size) if isinstance(size, tuple) else size
    assert want[0].window == list(range(3, 3 + n)) and len(want[0].scores) == n     # cc.y = the size of the set
    assert want[1].window == [0] and want[2].window == [1, 2]                       # other columns in the same launch
    ctx.set_models([m.buf for m in ms])
    knobs(variant)
    res, genes = check_call(ctx, seqs, list(range(len(seqs))), want, len(ms))
    assert genes > 0 and all(mb.model >= 0 for mb in want)
    assert [int(m) for m in res.contigs["model"]] == [mb.model for mb in want]


def test_winners_cover_the_columns():
    slots = []
    for size in osh.MODEL_SET_SIZES:
        _, ms, want = model_set_reference(size)
        tt = ms[want[0].model].trans_table
        slots.append([m for m in want[0].window if ms[m].trans_table == tt].index(want[0].model))
    assert len({s % 4 for s in slots}) >= 3 and any(s // 4 == 1 for s in slots)     # the column in its quad; m0 = 4
