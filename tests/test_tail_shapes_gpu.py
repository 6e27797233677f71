"""GPU parity of the traceback tail (the kernels of pyrodigal_amd/csrc/tail.inl over the rules of tail_rules.h) on the
input series of tests/tail_shapes.py, whose populations tests/test_tail_cpu.py proves on the CPU: every splice class, both
elimination rules, paths longer than a wave, a round and a chunk of the gene list, the gene whose in-order start tweak differs
from the parallel one at every place of the fix-up's 64-gene windows, and the node and contig counts at which the launch forms
switch (ref: lib.pyx:1253-1311, 3231-3401, Prodigal dprog.c eliminate_bad_genes).

Everything is compared with the CPU oracle, field by field (compare_contig of test_finder_gpu.py) -- never only one form with
another, since the forms share their rules (tail_rules.h: a wrong rule is wrong in every form).  Every series runs under every form that can take it, and each test asserts from
what is observable (the node count of the longest contig, the number of contigs) that the intended form ran:

  default                              k_tp_small up to 4 096 nodes (64 threads up to 2 048), the many-launch form beyond
  PGA_TP_STEPS=1                       the many-launch form for short chains too; PGA_TP_JUMP8=0: pointer doubling only
  PGA_TP_EXTRACT_ONE=1                 from 32 768 nodes: k_tp_extract with 1 024 threads instead of the chunked gene list
  PGA_TWEAK_SLOTS=1                    from 256 contigs: k_tail_tweak instead of k_tail_tweak_packed
  PGA_TAIL=device, PGA_TAIL=host       one thread per contig; host threads
  PGA_GATHER_ALL_DP=1, PGA_FULL_GATHER=1   without node arrays: k_emit_genes reads gathered copies, not the scorers' arrays"""
import pytest

from oracle import oracle as orc
from tests import tail_shapes as ts
from tests.test_finder_gpu import compare_contig

pytestmark = pytest.mark.gpu

ENV = ("PGA_TAIL", "PGA_TP_STEPS", "PGA_TP_JUMP8", "PGA_TP_EXTRACT_ONE", "PGA_TWEAK_SLOTS", "PGA_GATHER_ALL_DP", "PGA_FULL_GATHER")
FORMS = {
    "default": {},
    "steps": {"PGA_TP_STEPS": "1"},
    "steps_doubling": {"PGA_TP_STEPS": "1", "PGA_TP_JUMP8": "0"},
    "extract_one": {"PGA_TP_EXTRACT_ONE": "1"},
    "tweak_slots": {"PGA_TWEAK_SLOTS": "1"},
    "device": {"PGA_TAIL": "device"},
    "host": {"PGA_TAIL": "host"},
    "gather_all_dp": {"PGA_GATHER_ALL_DP": "1"},
    "full_gather": {"PGA_FULL_GATHER": "1"},
}
SHORT_FORMS = ("default", "steps", "steps_doubling", "device", "host")     # what differs for chains of at most 4 096 nodes
LONG_FORMS = ("default", "extract_one", "steps_doubling", "device", "host")  # ... and from 32 768 nodes


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def use(monkeypatch, form):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)


class Recorded:
    """What the oracle says about one contig under one set of parameters, computed once and kept unchanged: stands in for
    orc.Oracle in compare_contig, so that a contig that occurs in many batches (or 200 times in one) costs one oracle run."""

    def __init__(self, seq, params):
        self.seq, self.params, self.done = seq, params, False

    def _run(self, call):
        if not self.done:
            o = orc.Oracle(self.seq)
            self.phase = call(o)
            self._genes, self._nodes = o.genes(), o.nodes()
            self._genes.setflags(write=False)
            self._nodes.setflags(write=False)
            self.done = True
        return self.phase

    def _same(self, params):                # compare_contig passes the ends and the overlap; the shortest gene goes with the overlap
        assert (params.closed, params.max_overlap) == (self.params.closed, self.params.max_overlap)
        return self.params

    def find_genes_meta(self, models, params):
        return self._run(lambda o: o.find_genes_meta(models, self._same(params)))

    def find_genes_single(self, tinf, params):
        return self._run(lambda o: o.find_genes_single(tinf, self._same(params)))

    def genes(self):
        return self._genes

    def nodes(self):
        return self._nodes


_RECORDED = {}


def recorded(seq, tag, closed, max_overlap):
    key = (seq, tag, closed, max_overlap)
    if key not in _RECORDED:
        _RECORDED[key] = Recorded(seq, orc.Params(closed=closed, max_overlap=max_overlap, min_gene=ts.MIN_GENE[max_overlap]))
    return _RECORDED[key]


MODELS = {}


def models_of(tag):
    """tag: "nctc", "tweak", "mark_reset" (single mode, one model) or "meta" (the model set)."""
    if tag not in MODELS:
        MODELS[tag] = {"nctc": lambda: [ts.nctc()], "tweak": lambda: [ts.altered(*ts.TWEAK_MODEL)], "meta": ts.meta_models,
                       "mark_reset": lambda: [ts.meta_models()[ts.MARK_RESET_MODEL]]}[tag]()
    return MODELS[tag]


def check(ctx, seqs, tag, closed=False, max_overlap=60, want_nodes=True):
    """One find_genes_batch call, every contig against the oracle: (result, genes)."""
    models = models_of(tag)
    meta = tag == "meta"
    ctx.set_models([m.buf for m in models])
    res = ctx.find_genes_batch(seqs, meta=meta, closed=closed, max_overlap=max_overlap, min_gene=ts.MIN_GENE[max_overlap], want_nodes=want_nodes)
    n = 0
    for i, s in enumerate(seqs):
        n += compare_contig(res, i, s, recorded(s, tag, closed, max_overlap), models, meta, closed, max_overlap)
    return res, n


def check_all_ways(ctx, seqs, tag, overlaps=(60,)):
    """With and without node arrays (the lean gather reads the scorers' own arrays), open and closed, forwards and reversed:
    (the result of the first call -- open ends, forwards --, genes of all calls)."""
    total, first = 0, None
    for closed in (False, True):
        for want_nodes in (True, False):
            for batch in (seqs, seqs[::-1]):
                res, n = check(ctx, batch, tag, closed, 60, want_nodes)
                first = first or res
                total += n
    for mo in overlaps:
        if mo != 60:
            total += check(ctx, seqs, tag, False, mo, True)[1] + check(ctx, seqs[::-1], tag, True, mo, False)[1]
    return first, total


def longest(res):
    return max(int(c["n_nodes"]) for c in res.contigs)


def chains(res):
    return sum(1 for c in res.contigs if c["n_nodes"] > 0)


# ---- splices and elimination -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", SHORT_FORMS)
def test_splice_series(ctx, monkeypatch, form):
    """Every splice class at least three times, splices on adjacent edges, on the first edge and on the edge into the head: single
    mode (the DP pass's fields) and meta mode (the re-scored fields), under every overlap."""
    use(monkeypatch, form)
    seqs = ts.splice_series() + list(ts.DEGENERATE)
    res, n = check_all_ways(ctx, seqs, "nctc", ts.MAX_OVERLAPS)
    assert 2048 < longest(res) <= 4096 and n >= 8 * 240                   # k_tp_small with 256 threads, or k_tp_slots .. under PGA_TP_STEPS
    res, n = check_all_ways(ctx, seqs, "meta")
    assert 2048 < longest(res) <= 4096 and n >= 8 * 240


@pytest.mark.parametrize("form", SHORT_FORMS)
def test_elimination_series(ctx, monkeypatch, form):
    """Both marking rules some twenty times each, marks on spliced-in nodes, splices on first and head edges: thirty contigs in meta
    mode, each chain short enough for k_tp_small with 64 threads."""
    use(monkeypatch, form)
    seqs = ts.elimination_series()
    seqs = seqs[:11] + list(ts.DEGENERATE[:2]) + seqs[11:] + list(ts.DEGENERATE[2:])
    res, n = check_all_ways(ctx, seqs, "meta", ts.MAX_OVERLAPS)
    assert longest(res) <= 2048 and n > 5000
    res, n = check_all_ways(ctx, seqs, "nctc")
    assert longest(res) <= 2048
    # two triple overlaps whose spliced-in reverse stop has an ov_mark to reset: single mode, where the tail's ov_mark is returned
    res, n = check_all_ways(ctx, ts.mark_reset_series() + seqs[:4], "mark_reset")
    assert longest(res) <= 2048


# ---- gene list ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", SHORT_FORMS)
@pytest.mark.parametrize("name", ["wave", "round"])
def test_gene_list_one_launch(ctx, monkeypatch, name, form):
    """A path longer than 64 positions in a chain of at most 2 048 nodes (k_tp_small with 64 threads: two rounds), and one longer
    than 256 in a chain of exactly 4 096 (256 threads: two rounds); each also without its first gene."""
    use(monkeypatch, form)
    seq = ts.GENE_LIST[name][0]()
    for batch in ([seq], [ts.minus_one_gene(seq, ts.nctc())], [seq] + ts.companions(9)):
        res, n = check_all_ways(ctx, batch, "nctc")
        assert longest(res) <= 2048 if name == "wave" else 2048 < longest(res) <= 4096
    assert longest(check(ctx, [seq], "nctc")[0]) == ts.GENE_LIST[name][1]


@pytest.mark.parametrize("form", ["default", "steps_doubling", "device", "host"])
def test_gene_list_many_launches(ctx, monkeypatch, form):
    """A path of 390 positions in a chain of 13 419 nodes: k_tp_extract with 256 threads, two rounds."""
    use(monkeypatch, form)
    seq = ts.GENE_LIST["steps"][0]()
    res, n = check_all_ways(ctx, [seq] + ts.companions(9), "nctc")
    assert longest(res) == ts.GENE_LIST["steps"][1] and n > 8 * 195


@pytest.mark.parametrize("form", LONG_FORMS)
def test_gene_list_chunks(ctx, monkeypatch, form):
    """A path of 1 164 positions with eliminated pairs in its second chunk, in a chain of 33 954 nodes: the chunked gene list, and
    under PGA_TP_EXTRACT_ONE k_tp_extract with 1 024 threads in two rounds."""
    use(monkeypatch, form)
    seq = ts.GENE_LIST["chunk"][0]()
    for closed, want_nodes in ((False, True), (True, False)):
        res, n = check(ctx, [seq, ts.ONE_GENE, b""], "nctc", closed, 60, want_nodes)
        assert longest(res) >= 32768 and chains(res) <= 64 and n > 570


# ---- start tweaks ------------------------------------------------------------------------------------------------------------------------------

def tweak_batch():
    return ts.tweak_series() + ts.splice_series()


def test_tweaks_one_thread_per_gene(ctx, monkeypatch):
    """k_tail_tweak and the fix-up with two wavefronts: fewer than 256 contigs, none of 32 768 nodes."""
    for form in ("default", "device", "host"):
        use(monkeypatch, form)
        res, n = check_all_ways(ctx, tweak_batch(), "tweak", ts.MAX_OVERLAPS)
        assert len(res.contigs) < 256 and longest(res) < 32768 and n > 5000


@pytest.mark.parametrize("form", ["default", "tweak_slots"])
def test_tweaks_packed(ctx, monkeypatch, form):
    """k_tail_tweak_packed: 256 contigs or more (PGA_TWEAK_SLOTS=1 keeps k_tail_tweak for them)."""
    use(monkeypatch, form)
    seqs = ts.companions(250)
    seqs = seqs[:100] + tweak_batch() + seqs[100:]
    res, n = check_all_ways(ctx, seqs, "tweak", ts.MAX_OVERLAPS)
    assert len(res.contigs) >= 256 and longest(res) < 32768


def test_tweaks_one_wavefront_per_gene(ctx, monkeypatch):
    """k_tail_tweak_wave and the fix-up with sixteen wavefronts: the tweak series next to a contig of 32 768 nodes, and the differing
    gene inside such a contig (gene 249 of 501, 18 genes redone)."""
    long_one = ts.cut(*ts.LONG_TWEAK)
    for mo in ts.MAX_OVERLAPS:                          # (genes of 200 bases or more leave half as many nodes: a longer contig)
        batch = tweak_batch() + [long_one if mo < 200 else ts.cut(*ts.LONG_TWEAK_200)]
        res, n = check(ctx, batch, "tweak", False, mo, mo == 60)
        assert longest(res) == (32768 if mo < 200 else 33022) and len(res.contigs) <= 1024 and n > 1100
    # the elimination series in meta mode next to such a contig: a candidate exactly at the start of the gene behind it
    res, n = check(ctx, ts.elimination_series() + [ts.with_nodes(32768)], "meta", False, 60, False)
    assert longest(res) == 32768
    longer = ts.cut(ts.LONG_TWEAK[0], ts.LONG_TWEAK[1], 515000)           # with closed ends long_one has 32 750 nodes, this one 33 069
    res, n = check(ctx, [longer], "tweak", True, 60, True)
    assert longest(res) >= 32768 and n > 480
    use(monkeypatch, "extract_one")
    res, n = check(ctx, [long_one] + ts.tweak_series(), "tweak", False, 60, False)
    assert longest(res) == 32768


# ---- gene records ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["gather_all_dp", "full_gather"])
def test_gene_records_from_gathered_fields(ctx, monkeypatch, form):
    """Without node arrays k_emit_genes reads the scorers' own arrays (the other tests' want_nodes=False).  PGA_GATHER_ALL_DP gathers
    the DP pass's fields all the same (the tail and the records' topology and single-mode scores then come from the gathered
    copies, the final-pass fields from the scorers), PGA_FULL_GATHER the final pass's too (every field from the gathered copies):
    the splice series, the smallest input with every record field in both modes, single mode (the DP pass's scores) and meta mode
    (the final pass's), open and closed ends."""
    use(monkeypatch, form)
    seqs = ts.splice_series()
    for tag in ("nctc", "meta"):
        for closed in (False, True):
            res, n = check(ctx, seqs, tag, closed, 60, want_nodes=False)
            assert len(seqs) == 5 and n >= 240


# ---- launch edges ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["default", "steps"])
@pytest.mark.parametrize("n_nodes", [2048, 2049, 4096, 4097])
def test_node_counts_at_the_one_launch_thresholds(ctx, monkeypatch, n_nodes, form):
    """64 threads up to 2 048 nodes, 256 up to 4 096, the many-launch form beyond: a contig of exactly that many nodes alone and as
    the longest of a batch, in single and in meta mode."""
    use(monkeypatch, form)
    seq = ts.with_nodes(n_nodes)
    for batch in ([seq], ts.companions(20) + [seq] + ts.elimination_series()[:6]):
        for tag in ("nctc", "meta"):                    # (open ends: the node counts are those of open ends; the winning models read table 11)
            for want_nodes in (True, False):
                for b in (batch, batch[::-1]):
                    res, n = check(ctx, b, tag, False, 60, want_nodes)
                    assert longest(res) == n_nodes


@pytest.mark.parametrize("n_nodes", [32767, 32768])
def test_node_counts_at_the_genome_threshold(ctx, monkeypatch, n_nodes):
    """From 32 768 nodes: the chunked gene list, k_tail_tweak_wave, wide workgroups for k_tp_extract and the fix-up."""
    for form in ("default", "extract_one"):
        use(monkeypatch, form)
        for tag, closed, want_nodes in (("nctc", False, True), ("tweak", False, False)):
            res, n = check(ctx, [ts.with_nodes(n_nodes)] + ts.tweak_series()[:2], tag, closed, 60, want_nodes)
            assert longest(res) == n_nodes and n > 450


def segments_batch(k, long_one):
    """A batch with exactly k chains (open ends): the long contig, k - 3 short ones, and the degenerate contigs, of which two have nodes."""
    short = [s for s in ts.companions(k + 8, seed=5200) if s not in ts.DEGENERATE][:k - 3]
    return short[:k // 2] + [long_one] + short[k // 2:] + list(ts.DEGENERATE)


@pytest.mark.parametrize("k", [63, 64, 65])
def test_chain_counts_at_the_chunked_gene_list_threshold(ctx, k):
    """The chunked gene list takes up to 64 chains; one more and k_tp_extract takes the batch, 1 024 threads wide."""
    for tag, long_one in (("nctc", ts.GENE_LIST["chunk"][0]()), ("tweak", ts.cut(*ts.LONG_TWEAK))):
        res, n = check(ctx, segments_batch(k, long_one), tag, False, 60, tag == "nctc")
        assert longest(res) >= 32768 and chains(res) == k


@pytest.mark.parametrize("k", [255, 256])
def test_contig_counts_at_the_packed_tweak_threshold(ctx, k):
    seqs = ts.companions(k - 6) + ts.tweak_series()
    for closed, want_nodes in ((False, True), (True, False)):
        res, n = check(ctx, seqs, "tweak", closed, 60, want_nodes)
        assert len(res.contigs) == k and longest(res) < 32768


@pytest.mark.parametrize("k", [1024, 1025])
def test_contig_counts_at_the_wavefront_tweak_threshold(ctx, k):
    """Up to 1 024 contigs next to a genome-sized one take k_tail_tweak_wave, more take k_tail_tweak_packed; either way the long
    contig's 18 redone genes go through the fix-up with sixteen wavefronts."""
    seqs = ts.repeated(k - 2) + [ts.cut(*ts.LONG_TWEAK), ts.tweak_contig("first_of_window")]
    seqs = seqs[-2:] + seqs[:-2] if k == 1025 else seqs
    res, n = check(ctx, seqs, "tweak", False, 60, False)
    assert len(res.contigs) == k and longest(res) == 32768
    assert len({s for s in seqs}) <= 18
