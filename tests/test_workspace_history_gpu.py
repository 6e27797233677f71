"""A call's result depends on its arguments only -- not on what earlier calls left in the context's workspace, in the process-wide
cache of destroyed contexts or in the letters' allocation of the last batch.

Every SUBJECT call (S1 .. S11 below) runs once on a context without history (after pga_release_cached()), where it is compared with
the CPU oracle or the reference's fixtures the way the other GPU tests compare, and its complete deterministic output is kept as
bytes.  Then it runs behind DIRTYING calls (D1 .. D6) on the same context, with pga_debug_poison between the two: the dirtying call
leaves every integer buffer full of values that are valid for ANOTHER input, the poison fills every floating-point buffer (whole
capacity, and every block acquired later) with 0xFF (NaN: loses every comparison), 0x7F (huge: wins a max) or 0xFE (hugely negative:
wins a min).  The bytes must be the ones kept.

Pairs.  Every subject runs after D1 with the three bytes, after D4 (its own near miss) and after D6 (D1 on a context that is
destroyed: the blocks come back through the cache under other names) with 0xFF.  D2 (one 400 kbp contig, single mode, table 4) runs
before S1, S3, S4 and S10: the calls that share its long-chain connection-scoring buffers and its single-mode path.  D3 (a
training run) runs before S3, S8, S9 and S11: training shares the `tr_*` / `dp_*` buffers with train / train_batch and the stage
calls, and leaves the device arrays of its last stage behind.  D5 (a call smaller than the subject) runs before S1, S2, S4 and S6,
the meta-mode calls whose buffers then partly grow into fresh blocks.  Left out: D2 / D3 / D5 before S5, S7 (their buffers --
`circ_*`, `tr_ct*`, the rotated batch -- are only touched by circular calls, which D1 and D4 make); D2 / D5 before S11
(pga_score_connections allocates per call and keeps nothing); D3 before the meta-mode subjects (covered by D1's larger call on the
same buffers).

Float state that legitimately lives from one call to the next, and is therefore never poisoned BETWEEN those two calls here:
  * the winners' node arrays of a find call made with want_nodes (`ca_*`, `o_arena` and the group arrays, pga_internal.h DevNodes):
    pga_render_genes(..., "scores") reads them until the next finder call on the context;
  * nothing else: `hs_*`, `h_chain_results`, `dp_*`, `dpw_*`, `tr_*` are scratch of one call.
Not compared: timings (t_total_ms, t_dp_ms, pga_dp_timings), and `ov_mark` of nodes no connection reached in pga_score_connections
(documented as undefined: tests/test_dp_gpu.py)."""
import contextlib
import functools
import gzip
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import circular_ref as cref
from tests import sets_ref as sr
from tests import terminal_repeat_ref as tref
from tests.util import golden_path, read_fasta, synthetic_contig

pytestmark = pytest.mark.gpu

KNOBS = ("PGA_DP_KERNEL", "PGA_DP_SEG", "PGA_DP_SEG_MIN", "PGA_DP_SEG_LEN", "PGA_DP_SEG_WARM", "PGA_DP_SEG_WAVE", "PGA_DPW_SCHED",
         "PGA_TAIL", "PGA_SS_FULL_STOPS", "PGA_SS_STARTS_ONLY")
SEG = {"PGA_DP_SEG_MIN": "2500", "PGA_DP_SEG_LEN": "512", "PGA_DP_SEG_WARM": "768"}     # as tests/test_dp_segments_gpu.py forces the path
WAVE = {"PGA_DP_KERNEL": "wave"}
POISONS = (0xFF, 0x7F, 0xFE)
KB100, KB100_T = "GCF_001457455.1_NCTC11397_genomic_100kb", "GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz"
SRR_T = "SRR492066.training.bin.gz"


@contextlib.contextmanager
def knobs(env):
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def new_context():
    from pyrodigal_amd import _cabi
    return _cabi.Context(0)


def blob(*arrays):
    """Arrays (or bytes) as one byte string, lengths included."""
    out = []
    for a in arrays:
        b = a if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a).tobytes()
        out.append(len(b).to_bytes(8, "little") + bytes(b))
    return b"".join(out)


def snap_nodes(nodes):
    return b"" if nodes is None else blob(*[np.asarray(nd[k]) for nd in nodes for k in sorted(nd) if k != "n"], np.asarray([nd["n"] for nd in nodes]))


def snap(res):
    """Everything deterministic of a BatchResult: the records field by field (no padding bytes), node arrays, masks, cuts, the sets'
    choice and the trimmed lengths."""
    parts = [res.genes[k] for k in res.genes.dtype.names] + [res.contigs[k] for k in res.contigs.dtype.names]
    parts += [np.asarray([res.node_passes, res.n_chains], np.int64), snap_nodes(res.nodes)]
    parts += [b"" if res.masks is None else blob(*res.masks)]
    for extra in (res.cuts, res.set_models, res.set_scores, res.model_scores, res.terminal_repeats):
        parts.append(b"-" if extra is None else blob(extra))
    return blob(*parts)


def _cache(fn):
    memo = {}

    def get(*a):
        if a not in memo:
            memo[a] = fn(*a)
        return memo[a]
    return get


@_cache
def bench_models():
    from pyrodigal_amd import benchdata
    return [b for _, b in benchdata.load_model_set()]


@_cache
def bench_bins():
    return [orc.Training(b) for b in bench_models()]


@_cache
def bins13():
    return cref.meta_bins()


@_cache
def two_table_models():
    """A table-11 and a table-4 model."""
    t4 = [m for m in bins13() if m.trans_table == 4]
    assert len(t4) == 1
    return [orc.Training.load(golden_path(SRR_T)), t4[0]]


@_cache
def planted(length, gc, seed):
    from pyrodigal_amd import benchdata
    return benchdata.planted_contig(length, gc, seed)


def with_runs(seq, runs, letter=b"N"):
    s = bytearray(seq)
    for at, n in runs:
        s[at:at + n] = letter * n
    return bytes(s)


# ------------------------------------------------------------------------------------------------------------------ subjects

class Subject:
    env = {}
    keeps_workspace = True      # False: the call allocates per call and leaves no buffer in the context

    def run(self, ctx, verify=False):
        with knobs(self.env):
            return self.call(ctx, verify)


@_cache
def s1_contigs():
    seqs = [b"", b"ATG", b"N" * 500, b"A" * 50]                      # (b"A" * 50: not one node)
    seqs += [synthetic_contig(n, 0.5, 8000 + n) for n in (3071, 3072, 3073)]
    k = 0
    while len(seqs) < 70:
        length = 61 if k == 0 else 6000 if k == 1 else 61 + (k * 1931) % 5940
        seqs.append(synthetic_contig(length, 0.30 + 0.40 * ((k * 7) % 41) / 40, 8100 + k))
        k += 1
    return seqs


class Meta70(Subject):
    """S1 / S2: meta mode as the benchmark runs it -- 70 contigs (more than one 64-lane batch, not a multiple of it), the 16 models."""

    def __init__(self, closed, want_nodes, env):
        self.closed, self.want_nodes, self.env = closed, want_nodes, env

    def call(self, ctx, verify):
        from tests.test_finder_gpu import compare_contig
        ctx.set_models(bench_models())
        seqs = s1_contigs()
        res = ctx.find_genes_batch(seqs, meta=True, closed=self.closed, want_nodes=self.want_nodes)
        if verify:
            n = sum(compare_contig(res, i, s, orc.Oracle(s), bench_bins(), meta=True, closed=self.closed) for i, s in enumerate(seqs))
            assert n > 50 and res.contigs[3]["n_nodes"] == 0
        return snap(res)

    def near(self, ctx):
        ctx.set_models(bench_models()[:5] if self.want_nodes else bench_models())
        with knobs({} if self.env else WAVE):          # the other connection scorer, the other `closed`, node arrays the other way round
            ctx.find_genes_batch(s1_contigs(), meta=True, closed=not self.closed, want_nodes=not self.want_nodes)


@_cache
def s3_contigs():
    seqs = []
    for k in range(12):
        n = 2000 + 1171 * k
        s = planted(n, 0.38 + 0.02 * k, 8300 + k) if k % 2 else synthetic_contig(n, 0.38 + 0.02 * k, 8300 + k)
        seqs.append(with_runs(s, [(300 + 97 * k, 49 + k % 3), (1200, 120)] if k % 3 else []))
    seqs += [b"N" * 70 + synthetic_contig(4000, 0.5, 8372) + b"N" * 55, b""]
    return seqs, [k % 2 for k in range(len(seqs))]


class SingleModels(Subject):
    """S3: single mode with model_of_contig over a table-11 and a table-4 model, masking on."""

    def call(self, ctx, verify):
        from tests.test_finder_gpu import compare_contig
        models = two_table_models()
        ctx.set_models([m.buf for m in models])
        seqs, moc = s3_contigs()
        b = ctx.upload(seqs)
        try:
            res = ctx.find_genes(b, meta=False, want_nodes=True, mask=True, model_of_contig=moc)
        finally:
            b.close()
        if verify:
            n = sum(compare_contig(res, i, s, orc.Oracle(s, mask=True, mask_size=50), [models[moc[i]]], meta=False) for i, s in enumerate(seqs))
            assert n > 20 and list(res.contigs["model"]) == moc
        return snap(res)

    def near(self, ctx):
        ctx.set_models([m.buf for m in two_table_models()])
        seqs, moc = s3_contigs()
        b = ctx.upload(seqs)
        try:
            ctx.find_genes(b, meta=False, want_nodes=False, mask=False, model_of_contig=[1 - m for m in moc])
        finally:
            b.close()


class LongContig(Subject):
    """S4: one dense planted contig of 120 kbp, its chains cut into segments (or walked whole by the wave-batch scorer)."""

    def __init__(self, env):
        self.env = env

    def call(self, ctx, verify):
        from tests.test_finder_gpu import compare_contig
        ctx.set_models(bench_models())
        seq = planted(120_000, 0.5, 8400)
        res = ctx.find_genes_batch([seq], meta=True)
        st = ctx.dp_stats()
        if verify:
            assert compare_contig(res, 0, seq, orc.Oracle(seq), bench_bins(), meta=True) > 100
            if "PGA_DP_SEG_MIN" in self.env:
                assert st["chains"] >= 1 and st["segments"] > st["chains"]
        return blob(snap(res), np.asarray([st["chains"], st["segments"], st["serial"]] + st["rejected"]))

    def near(self, ctx):
        ctx.set_models(bench_models())
        with knobs({"PGA_DP_SEG": "0"}):                # the serial walk of the same chains
            ctx.find_genes_batch([planted(120_000, 0.5, 8400)], meta=True, closed=True)


@_cache
def s5_inputs():
    seqs, regions, flags = [], [], []
    for k in range(9):
        n = 5000 + 1777 * k
        s = synthetic_contig(n, 0.36 + 0.035 * k, 8500 + k)
        reg = None
        if k % 3 == 0:
            s = with_runs(s, [(n // 2, 150)])
            reg = [(n // 2, n // 2 + 150)]
        if k % 3 == 1:
            s = with_runs(s, [(n // 3, 64), (n - 20, 20)], b"n")
        seqs.append(s); regions.append(reg); flags.append(k % 2 == 0)
    seqs += [b"", b"ATG", cref.fixture("KK037166")]
    regions += [None, None, None]
    flags += [True, False, True]
    return seqs, regions, flags


class CircularMixed(Subject):
    """S5: a mixed circular and linear batch with named regions and lower-case masking."""

    def call(self, ctx, verify):
        from tests.test_circular_gpu import compare_circular
        from tests.test_finder_gpu import compare_contig
        bins = bins13()
        ctx.set_models([m.buf for m in bins])
        seqs, regions, flags = s5_inputs()
        res = ctx.find_genes_batch(seqs, meta=True, want_nodes=True, regions=regions, mask_lowercase=True, circular=flags)
        if verify:
            n = 0
            for i, s in enumerate(seqs):
                # (the call masks what the regions name and what is written in lower case, not the unknown bases a fixture holds)
                kw = {"mask": True, "mask_size": 50} if (i < 9 and i % 3 != 2) else {}
                if flags[i]:
                    n += len(compare_circular(res, i, s, bins, True, **kw).genes)
                else:
                    assert res.cuts[i] == -1
                    n += compare_contig(res, i, s, orc.Oracle(s, **kw), bins, meta=True)
            assert n > 20
        return snap(res)

    def near(self, ctx):
        ctx.set_models([m.buf for m in bins13()])
        seqs, regions, flags = s5_inputs()
        ctx.find_genes_batch(seqs, meta=True, want_nodes=False, regions=regions, mask_lowercase=False)       # every contig linear


class Sets(Subject):
    """S6: set labels in meta mode, the members interleaved with unlabelled contigs."""

    def call(self, ctx, verify):
        from tests.test_sets_gpu import compare_member
        bins = bins13()
        ctx.set_models([m.buf for m in bins])
        seqs, labels = sr.case_interleaved()
        res = ctx.find_genes_batch(seqs, meta=True, want_nodes=True, sets=labels)
        if verify:
            want = sr.find_genes_sets(seqs, labels, bins)
            assert sum(compare_member(res, i, mb, len(bins)) for i, mb in enumerate(want)) > 0
        return snap(res)

    def near(self, ctx):
        ctx.set_models([m.buf for m in bins13()])
        ctx.find_genes_batch(sr.case_interleaved()[0], meta=True, want_nodes=True)         # no labels: every contig on its own


class TerminalRepeats(Subject):
    """S7: detection of terminal repeats, the trimmed letters, and the trimmed batch's call."""

    def call(self, ctx, verify):
        from tests.test_circular_gpu import compare_circular
        from tests.test_finder_gpu import compare_contig
        from tests.test_terminal_repeat_gpu import batch_letters, mixed_inputs, printed
        bins = bins13()
        ctx.set_models([m.buf for m in bins])
        S, T, flags, ks = mixed_inputs()
        b = ctx.upload(S)
        t = b
        try:
            match, trim = b.terminal_repeats()
            t = b.trim_terminal_repeats(trim)
            letters = batch_letters(ctx, t, [len(x) for x in T])
            res = ctx.find_genes(t, meta=True)
        finally:
            if t is not b:
                t.close()
            b.close()
        if verify:
            assert [tref.terminal_repeat(s)[:2] for s in S] == list(zip(match.tolist(), trim.tolist())) and trim.tolist() == ks
            assert letters == [printed(x) for x in T]
            for i, s in enumerate(T):
                if flags[i]:
                    compare_circular(res, i, s, bins, True)
                else:
                    compare_contig(res, i, s, orc.Oracle(s), bins, meta=True)
        return blob(match, trim, blob(*letters), snap(res))

    def near(self, ctx):
        from tests.test_terminal_repeat_gpu import mixed_inputs
        ctx.set_models([m.buf for m in bins13()])
        ctx.find_genes_batch(mixed_inputs()[0], meta=True)          # the untrimmed records, as lines


@_cache
def s8_contigs():
    return [read_fasta("SRR492066.fna.gz")[0][1].encode(), with_runs(synthetic_contig(20011, 0.62, 8801), [(5000, 80), (9000, 30)]),
            b"ATGAAATAA", b""]


class Stages(Subject):
    """S8: pga_nodes_stage at each stage."""

    def call(self, ctx, verify):
        from pyrodigal_amd import _cabi
        from tests.test_stages_gpu import check, oracle_stage
        tinf = orc.Training.load(golden_path(SRR_T))
        ctx.set_models([tinf.buf])
        seqs = s8_contigs()
        out = []
        for stage in (_cabi.STAGE_EXTRACT, _cabi.STAGE_SCORE, _cabi.STAGE_OVERLAP):
            nodes = ctx.nodes_stage(seqs, stage)
            if verify:
                for s, nd in zip(seqs, nodes):
                    check(nd, oracle_stage(s, stage, tinf), stage)
            out.append(snap_nodes(nodes))
        r = ctx.nodes_stage(seqs, _cabi.STAGE_SEQUENCE, mask=True)
        if verify:
            for i, s in enumerate(seqs):
                assert np.array_equal(r.masks[i], orc.Oracle(s, mask=True, mask_size=50).masks())
            assert r.contigs["n_unknown"].tolist() == [s.count(b"N") for s in seqs]
        out.append(snap(r))
        return blob(*out)

    def near(self, ctx):
        from pyrodigal_amd import _cabi
        ctx.set_models([two_table_models()[1].buf])
        for stage in (_cabi.STAGE_OVERLAP, _cabi.STAGE_EXTRACT):
            ctx.nodes_stage(s8_contigs(), stage, closed=True, mask=True)


@_cache
def s9_genomes():
    return [(read_fasta("KK037166.fna.gz")[0][1], 11), (read_fasta("SRR492066.fna.gz")[0][1], 4), (read_fasta(KB100 + ".fna.gz")[0][1], 11)]


class Training(Subject):
    """S9: train on the 100 kb fixture, train_batch of three small genomes over two tables."""

    def call(self, ctx, verify):
        one = ctx.train(read_fasta(KB100 + ".fna.gz")[0][1], closed=True)
        gs = s9_genomes()
        many = ctx.train_batch([g[0] for g in gs], translation_table=[g[1] for g in gs])
        if verify:
            assert one == gzip.open(golden_path(KB100_T)).read()
            for got, (seq, tt) in zip(many, gs):
                assert got == orc.Oracle(seq).train(orc.Params(), tt=tt).tobytes()
        return blob(one, *many)

    def near(self, ctx):
        gs = s9_genomes()
        ctx.train(gs[2][0], closed=False, translation_table=4)
        ctx.train_batch([g[0] for g in gs[::-1]], translation_table=[11, 11, 4], force_nonsd=True)


class CodingBases(Subject):
    """S10: pga_find_coding_bases over replicated contigs under a table-11 and a table-4 model (what the table selection runs)."""

    def call(self, ctx, verify):
        models = two_table_models()
        ctx.set_models([m.buf for m in models])
        seqs = s3_contigs()[0][:-1]
        n = len(seqs)
        b = ctx.upload(seqs)
        rep = None
        try:
            rep = ctx.replicate(b, list(range(n)) * 2)
            moc = [0] * n + [1] * n
            cov, ng, sc = ctx.find_coding_bases(rep, moc, mask=True)
        finally:
            if rep is not None:
                rep.close()
            b.close()
        if verify:
            for k in range(2 * n):
                s = seqs[k % n]
                o = orc.Oracle(s, mask=True, mask_size=50)
                o.find_genes_single(models[moc[k]], orc.Params())
                g = o.genes()
                c = np.zeros(len(s) + 1, bool)
                for x, y in zip(g["begin"], g["end"]):
                    c[max(int(x), 1) - 1:min(int(y), len(s))] = True
                assert (int(cov[k]), int(ng[k])) == (int(c.sum()), len(g)), k
            assert cov.sum() > 10000
        return blob(cov, ng, sc)

    def near(self, ctx):
        ctx.set_models([m.buf for m in two_table_models()])
        seqs = s3_contigs()[0]
        b = ctx.upload(seqs)
        try:
            ctx.find_coding_bases(b, [1] * len(seqs), mask=False, closed=True)
        finally:
            b.close()


@_cache
def s11_nodes():
    """Node arrays of SRR492066 and the oracle's connection scoring of them: the final pass and the training pass."""
    seq = read_fasta("SRR492066.fna.gz")[0][1]
    tinf = orc.Training.load(golden_path(SRR_T))
    o = orc.Oracle(seq)
    o.extract(tinf.trans_table, orc.Params()); o.sort(); o.reset_scores()
    o.score_nodes(tinf, False, False)
    o.overlapping_starts(tinf, 1, 60)
    o.dprog_raw(tinf, True)
    final = (o.nodes(), o.find_max_index(), tinf.st_wt)
    t = orc.Training()
    t.set_trans_table(11); t._f64(16)[0] = 4.35
    o = orc.Oracle(seq)
    o.extract(11, orc.Params()); o.sort()
    o.record_gc_bias(t)
    bias = t.bias.copy()
    o.overlapping_starts(t, 0, 60)
    before = o.nodes()
    o.dprog_raw(t, False)
    return final, (before, bias, o.nodes(), o.find_max_index())


class Connections(Subject):
    """S11: pga_score_connections (final) and pga_score_connections_training on the node arrays of one fixture."""
    keeps_workspace = False

    def __init__(self, env):
        self.env = env

    def call(self, ctx, verify):
        (ref, ref_max, st_wt), (before, bias, tref_, tmax) = s11_nodes()
        a = ctx.score_connections(ref["ndx"], ref["stop_val"], ref["type"], ref["strand"], ref["cscore"], ref["sscore"], ref["rscore"],
                                  ref["uscore"], ref["star_ptr"], st_wt, True)
        b = ctx.score_connections_training(before["ndx"], before["stop_val"], before["type"], before["strand"], before["gc_score"], bias,
                                           before["star_ptr"], 4.35)
        out = []
        for (score, traceb, ov, mi, _), want, wmax in ((a, ref, ref_max), (b, tref_, tmax)):
            reached = traceb != -1
            if verify:
                assert np.array_equal(traceb, want["traceb"]) and mi == wmax
                assert np.array_equal(score.view(np.uint64), want["score"].view(np.uint64))
                assert np.array_equal(ov[reached], want["ov_mark"][reached]) and reached.sum() > 100
            out.append(blob(score, traceb, np.where(reached, ov, 0), np.asarray([mi])))
        return blob(*out)

    def near(self, ctx):
        with knobs({} if self.env else WAVE):
            Connections.call(self, ctx, False)


SUBJECTS = {
    "S1-open": Meta70(False, False, {}), "S1-closed": Meta70(True, False, {}),
    "S1-open-wave": Meta70(False, False, WAVE), "S1-closed-wave": Meta70(True, False, WAVE),
    "S2-open": Meta70(False, True, {}), "S2-closed-wave": Meta70(True, True, WAVE),
    "S3": SingleModels(), "S4-segments": LongContig(SEG), "S4-wave": LongContig(WAVE), "S5": CircularMixed(), "S6": Sets(),
    "S7": TerminalRepeats(), "S8": Stages(), "S9": Training(), "S10": CodingBases(), "S11": Connections({}), "S11-wave": Connections(WAVE),
}
_BASE = {}


def baseline(name):
    """The subject on a context without history, checked against the oracle; its bytes."""
    if name not in _BASE:
        from pyrodigal_amd import _cabi
        _cabi.load().pga_release_cached()
        ctx = new_context()
        try:
            _BASE[name] = SUBJECTS[name].run(ctx, verify=True)
        finally:
            ctx.close()
    return _BASE[name]


# ------------------------------------------------------------------------------------------------------------ dirtying calls

@_cache
def d1_inputs():
    seqs = [synthetic_contig(3500 + (k * 37) % 1000, 0.33 + 0.36 * ((k * 11) % 29) / 28, 9000 + k) for k in range(300)]
    regions = [[(100, 400), (1000, 1090)] if k % 4 == 0 else None for k in range(300)]
    return seqs, regions, [k % 3 == 0 for k in range(300)]


def d1(ctx):
    """Bigger in every direction: 300 contigs, 16 models, node arrays, circular flags, regions."""
    seqs, regions, flags = d1_inputs()
    ctx.set_models(bench_models())
    with knobs({}):
        ctx.find_genes_batch(seqs, meta=True, want_nodes=True, regions=regions, circular=flags, mask=True)
        with knobs(WAVE):
            ctx.find_genes_batch(seqs[:150], meta=True, want_nodes=True)       # the wave-batch scorer's buffers as well


def d2(ctx):
    """One 400 kbp planted contig, single mode, table 4."""
    ctx.set_models([two_table_models()[1].buf])
    with knobs({}):
        ctx.find_genes_batch([planted(400_000, 0.45, 9100)], meta=False, want_nodes=True)


def d3(ctx):
    """A training run on another genome."""
    with knobs({}):
        ctx.train(planted(200_000, 0.55, 9200), translation_table=11)


def d5(ctx):
    """A call smaller than any subject."""
    ctx.set_models(bench_models()[4:9])
    with knobs({}):
        ctx.find_genes_batch([synthetic_contig(900 + 100 * k, 0.5, 9300 + k) for k in range(5)], meta=True, want_nodes=True)


def poisoned_subject(name, dirty, byte):
    want = baseline(name)
    ctx = new_context()
    try:
        dirty(ctx)
        n, nbytes = ctx.debug_poison(byte)
        assert (n > 0 and nbytes > 0) or (dirty == SUBJECTS[name].near and not SUBJECTS[name].keeps_workspace)
        assert SUBJECTS[name].run(ctx) == want
    finally:
        ctx.close()


# --------------------------------------------------------------------------------------------------------------------- tests

def device_error_ends_the_session(fn):
    """A stale index read as an address would show as a device error: nothing more is started on a device that reported one."""
    @functools.wraps(fn)
    def wrapper(*a, **kw):
        from pyrodigal_amd import _cabi
        try:
            return fn(*a, **kw)
        except _cabi.PgaError as e:
            pytest.exit("device error in %s%r: %s" % (fn.__name__, a or tuple(kw.values()), e), returncode=3)
    return wrapper


@pytest.mark.parametrize("name", list(SUBJECTS))
@device_error_ends_the_session
def test_no_history_result_equals_the_oracle(name):
    assert len(baseline(name)) > 0


@device_error_ends_the_session
def test_poison_reports_what_it_filled_and_can_be_switched_off():
    ctx = new_context()
    try:
        d5(ctx)
        n, nbytes = ctx.debug_poison(0xFF)
        assert n > 10 and nbytes > n * 64
        assert ctx.debug_poison(None) == (0, 0)
        with pytest.raises(ValueError):
            ctx.debug_poison(256)
    finally:
        ctx.close()


@pytest.mark.parametrize("byte", POISONS, ids=["nan", "huge", "neghuge"])
@pytest.mark.parametrize("name", list(SUBJECTS))
@device_error_ends_the_session
def test_after_a_bigger_call(name, byte):
    poisoned_subject(name, d1, byte)


@pytest.mark.parametrize("name", list(SUBJECTS))
@device_error_ends_the_session
def test_after_the_near_miss(name):
    poisoned_subject(name, SUBJECTS[name].near, 0xFF)


@pytest.mark.parametrize("name", list(SUBJECTS))
@device_error_ends_the_session
def test_after_a_destroyed_context(name):
    """D6: the blocks of D1's context return through the process-wide cache, by size and not by name."""
    want = baseline(name)
    a = new_context()
    try:
        d1(a)
    finally:
        a.close()
    ctx = new_context()
    try:
        ctx.debug_poison(0xFF)            # (a new context owns nothing yet: what it takes from the cache is filled as it is taken)
        assert SUBJECTS[name].run(ctx) == want
        n, nbytes = ctx.debug_poison(0xFF)
        assert (n > 0 and nbytes > 0) or not SUBJECTS[name].keeps_workspace
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["S1-open", "S1-closed-wave", "S3", "S4-segments", "S4-wave", "S10"])
@device_error_ends_the_session
def test_after_one_long_contig(name):
    poisoned_subject(name, d2, 0x7F)


@pytest.mark.parametrize("name", ["S3", "S8", "S9", "S11", "S11-wave"])
@device_error_ends_the_session
def test_after_a_training_run(name):
    poisoned_subject(name, d3, 0xFE)


@pytest.mark.parametrize("name", ["S1-open", "S1-open-wave", "S2-open", "S2-closed-wave", "S4-segments", "S6"])
@device_error_ends_the_session
def test_after_a_smaller_call(name):
    poisoned_subject(name, d5, 0xFF)


@pytest.mark.parametrize("name", ["S1-open", "S1-closed-wave"])
@device_error_ends_the_session
def test_five_runs_in_a_row(name):
    """The first run grows every buffer, the others none."""
    want = baseline(name)
    ctx = new_context()
    try:
        for k in range(5):
            ctx.debug_poison(POISONS[k % 3])
            assert SUBJECTS[name].run(ctx) == want, k
        assert ctx.debug_poison(0xFF)[0] > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("lean, full", [("S1-open", "S2-open"), ("S1-closed-wave", "S2-closed-wave")])
@device_error_ends_the_session
def test_lean_path_after_the_full_path(lean, full):
    """S1, S2, S1 without poison: the full path has just written the stop nodes' fields that the lean path leaves out -- with the
    values that are right for this input (what a sweep over one batch hides); then once more over NaN."""
    want_lean, want_full = baseline(lean), baseline(full)
    ctx = new_context()
    try:
        assert SUBJECTS[lean].run(ctx) == want_lean
        assert SUBJECTS[full].run(ctx) == want_full
        assert SUBJECTS[lean].run(ctx) == want_lean
        assert ctx.debug_poison(0xFF)[0] > 0
        assert SUBJECTS[lean].run(ctx) == want_lean
    finally:
        ctx.close()
