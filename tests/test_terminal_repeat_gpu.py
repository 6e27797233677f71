"""Direct terminal repeats on the device (pga_batch_terminal_repeats / pga_batch_trim_terminal_repeats): the detection
against the rule in plain Python (tests/terminal_repeat_ref.py), the trimmed batch letter by letter, and the call on a record with a
repeat against the existing circular call on the hand-trimmed record."""
import gzip
import io
import os
import re
import subprocess
import sys
import threading
import types

import numpy as np
import pytest

from tests import circular_ref as cref
from tests import terminal_repeat_ref as tref
from tests.util import golden_path, synthetic_contig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KB100, KB100_T = "GCF_001457455.1_NCTC11397_genomic_100kb", "GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz"
SRR_T = "SRR492066.training.bin.gz"
MIIJ_ROTATION = 817235           # MIIJ01000039 rotated to start inside its gene 816877..817593: the circle has a gene across the origin


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


@pytest.fixture(scope="module")
def bins():
    return cref.meta_bins()


@pytest.fixture(scope="module")
def chunk():
    from pyrodigal_amd import _cabi
    return int(_cabi.load().pga_terminal_repeat_chunk())


def other_base(ch):
    return b"ACGT"[(b"ACGT".index(bytes([ch]).upper()) + 1) % 4]


def mutate(seq, pos, ch=None):
    b = bytearray(seq)
    b[pos] = other_base(b[pos]) if ch is None else ch
    return bytes(b)


def with_repeat(length, k, seed, gc=0.5):
    """T + T[:k] for a random T of `length` bases."""
    t = synthetic_contig(length, gc, seed)
    return t + t[:k]


# ---------------------------------------------------------------------------------------------- detection

def detection_batch(C):
    """(contigs, planted): planted[i] is the k of a plain T + T[:k] contig, None for every other shape."""
    seqs, planted = [], []

    def add(s, k=None):
        seqs.append(s)
        planted.append(k)

    for n, k in enumerate((19, 20, 21, C - 1, C, C + 1, 2 * C + 3)):
        add(with_repeat(max(120, 2 * k - 150 if k > 200 else 500 + 37 * n), k, 100 + n), k)
    for a in range(16):                                   # the suffix window S[L - k:] starts at every alignment in the batch
        base = sum(len(s) for s in seqs)
        add(with_repeat(300 + (a - base - 300) % 16, 40 + a, 200 + a), 40 + a)
    add((synthetic_contig(100, 0.5, 301) * 3)[:215])      # period 100: the overlaps are 115 (> L / 2) and 15 (< min_length)
    t = synthetic_contig(150, 0.5, 302)
    add(t + t, 150)                                       # L / 2 == k
    t = synthetic_contig(19, 0.5, 303)
    add(t + t)                                            # shorter than 2 * min_length
    add(with_repeat(20, 19, 304))
    add(b""); add(b"A"); add(b"AC")
    add(with_repeat(700, 60, 305), 60)                    # (max_length = 30 of the second parameter set lies below these)
    for pos in (0, 79, 33):                               # an N in the repeat: first, last, a middle position; in either copy
        s = with_repeat(900, 80, 306 + pos)
        add(mutate(s, pos, ord("N")))
        add(mutate(s, len(s) - 80 + pos, ord("n")))
    s = with_repeat(1200, C + 90, 310)
    add(s[:-(C + 90)] + s[-(C + 90):].lower())            # a soft-masked copy
    add(s[:500].lower() + s[500:])
    t = b"A" * 70 + synthetic_contig(800, 0.5, 311)
    add(t + t[:50])                                       # a poly-A repeat: found, and filtered
    t = b"A" * 30 + b"ACGT" * 5 + synthetic_contig(600, 0.5, 312)
    add(t + t[:40])                                       # 33 of 40 are A: above 75 percent
    add(b"AAAC" * 10 + synthetic_contig(600, 0.5, 313) + b"AAAC" * 10)      # 30 of 40: exactly 75 percent, kept
    for period, seed in ((3, 314), (7, 315)):             # tandem repeats over the whole window, one mismatch at the far end
        unit = synthetic_contig(period, 0.5, seed)
        s = (unit * (6000 // period + 1))[:6000]
        add(mutate(s, len(s) - 1))
        add(mutate(s, 0))
        add(s)
    for n in range(6):
        add(synthetic_contig(120 + 977 * n, 0.35 + 0.05 * n, 320 + n))      # nothing to find
    r = C + 37                                            # two ends that differ in exactly one letter
    for pos in (0, C - 1, C, r - 1):
        s = with_repeat(1500, r, 330 + pos % 7)
        add(mutate(s, len(s) - r + pos))
        add(mutate(s, pos))
    return seqs, planted


PARAMETER_SETS = [(20, 65536, 75), (20, 30, 75), (19, 2000, 100), (1, 1048576, 25), (45, 1030, 60)]


@pytest.fixture(scope="module")
def detection(ctx, chunk):
    seqs, planted = detection_batch(chunk)
    want = {p: [tref.terminal_repeat(s, *p)[:2] for s in seqs] for p in PARAMETER_SETS}
    b = ctx.upload(seqs)
    yield seqs, planted, want, b
    b.close()


def test_the_inputs_are_what_they_claim(detection, chunk):
    seqs, planted, want, b = detection
    assert 50 <= len(seqs) <= 80 and all(len(s) <= 6200 for s in seqs)
    ref = want[PARAMETER_SETS[0]]
    for s, k, (match, trim) in zip(seqs, planted, ref):
        if k is not None:
            assert (match, trim) == ((k, k) if k >= 20 else (0, 0)), (len(s), k)
    base = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    aligned = {int(base[i] + len(s) - k) % 16 for i, (s, k) in enumerate(zip(seqs, planted)) if k is not None and k >= 20}
    assert aligned == set(range(16))
    assert sum(1 for m, t in ref if m > 0 and t == 0) >= 2 and sum(1 for m, t in ref if m == 0) >= 20
    assert {chunk - 1, chunk, chunk + 1, 2 * chunk + 3} <= {m for m, _ in ref}


@pytest.mark.parametrize("params", PARAMETER_SETS)
def test_detection_equals_the_reference(detection, params):
    seqs, planted, want, b = detection
    match, trim = b.terminal_repeats(None, *params)
    got = list(zip(match.tolist(), trim.tolist()))
    assert got == want[params], [(i, len(seqs[i]), g, w) for i, (g, w) in enumerate(zip(got, want[params])) if g != w]


def test_search_flags_skip_contigs(detection):
    seqs, planted, want, b = detection
    ref = want[PARAMETER_SETS[0]]
    search = [i % 3 != 1 for i in range(len(seqs))]
    assert any(ref[i][0] > 0 for i in range(len(seqs)) if not search[i])
    match, trim = b.terminal_repeats(search)
    assert list(zip(match.tolist(), trim.tolist())) == [ref[i] if search[i] else (0, 0) for i in range(len(seqs))]
    match, trim = b.terminal_repeats([False] * len(seqs))
    assert not match.any() and not trim.any()


def test_one_differing_letter_is_no_match_at_that_length(detection, chunk):
    seqs, planted, want, b = detection
    r = chunk + 37
    match, _ = b.terminal_repeats(None, r, r, 100)        # only r itself is asked for
    ones = [i for i, s in enumerate(seqs) if len(s) == 1500 + r]
    assert len(ones) == 8 and not match[ones].any()
    intact = with_repeat(1500, r, 330)
    one = b.ctx.upload([intact])
    try:
        assert one.terminal_repeats(None, r, r, 100)[0].tolist() == [r]
    finally:
        one.close()


def test_bad_parameters(detection):
    seqs, planted, want, b = detection
    for bad in ((0, 10, 75), (11, 10, 75), (20, 1048577, 75), (20, 100, 24), (20, 100, 101)):
        with pytest.raises(Exception, match="pga_batch_terminal_repeats"):
            b.terminal_repeats(None, *bad)
    with pytest.raises(ValueError, match="search"):
        b.terminal_repeats([True])


# ---------------------------------------------------------------------------------------------- trimming

def batch_letters(ctx, b, lens):
    """The letters of a resident batch, read back through the gene FASTA of one made-up gene per contig that covers all of it
    (upper case, N for an unknown letter)."""
    from pyrodigal_amd import _cabi
    n = len(lens)
    contigs = np.zeros(n, _cabi.CONTIG_DTYPE)
    genes = np.zeros(sum(1 for x in lens if x > 0), _cabi.GENE_DTYPE)
    k = 0
    for i, x in enumerate(lens):
        contigs[i]["gene_begin"] = k
        if x > 0:
            contigs[i]["n_genes"] = 1
            genes[k]["contig"], genes[k]["begin"], genes[k]["end"], genes[k]["strand"] = i, 1, x, 1
            k += 1
    text = ctx.render_genes(b, types.SimpleNamespace(contigs=contigs, genes=genes), ["c%d" % i for i in range(n)], ("fna",))["fna"]
    out = []
    for i in range(n):
        lines = text.contig(i).decode().splitlines()
        out.append("".join(l for l in lines if not l.startswith(">")).encode())
    return out


def printed(seq):
    return bytes(c if c in b"ACGT" else ord("N") for c in seq.upper())


def test_trimmed_batch_holds_the_trimmed_letters(ctx, detection):
    seqs, planted, want, b = detection
    ctx.set_models([cref.single_model(SRR_T)[0].buf])
    match, trim = b.terminal_repeats()
    assert (trim > 0).sum() >= 20 and (trim == 0).sum() >= 20
    t = b.trim_terminal_repeats(trim)
    try:
        assert t is not b and t.n == b.n
        assert t.circular.tolist() == (trim > 0).astype(np.uint8).tolist()
        lens = [len(s) - int(x) for s, x in zip(seqs, trim)]
        got = batch_letters(ctx, t, lens)
        for i, s in enumerate(seqs):
            assert got[i] == printed(s[:lens[i]]), i
        # ... and the batch it came from is as it was
        assert batch_letters(ctx, b, [len(s) for s in seqs]) == [printed(s) for s in seqs]
        again, _ = b.terminal_repeats()
        assert again.tolist() == match.tolist()
    finally:
        t.close()
    # one contig trimmed, at an odd place in the batch
    only = np.zeros(b.n, np.int32)
    i = int(np.flatnonzero(trim > 0)[7])
    only[i] = trim[i]
    t = b.trim_terminal_repeats(only)
    try:
        lens = [len(s) - int(x) for s, x in zip(seqs, only)]
        assert batch_letters(ctx, t, lens) == [printed(s[:n]) for s, n in zip(seqs, lens)]
        assert t.circular.tolist() == (only > 0).astype(np.uint8).tolist()
    finally:
        t.close()


def test_all_zero_trim_is_the_same_batch(detection):
    seqs, planted, want, b = detection
    assert b.trim_terminal_repeats(np.zeros(b.n, np.int32)) is b


def test_bad_trim_values(detection):
    seqs, planted, want, b = detection
    i = next(i for i, s in enumerate(seqs) if len(s) == 300)
    for bad in (-1, 151):
        t = np.zeros(b.n, np.int32)
        t[i] = bad
        with pytest.raises(Exception, match="contig %d " % i):
            b.trim_terminal_repeats(t)
    t = np.zeros(b.n, np.int32)
    t[i] = 150                                            # half of it is the most a record can lose
    out = b.trim_terminal_repeats(t)
    assert out is not b
    out.close()
    with pytest.raises(ValueError, match="trim"):
        b.trim_terminal_repeats([0])


def test_regions_across_the_new_end_are_clipped(ctx, bins):
    left, right = synthetic_contig(9000, 0.5, 401), synthetic_contig(9000, 0.5, 402)
    t = left + b"N" * 300 + right
    k = 200
    s = t + t[:k]
    plain = synthetic_contig(8000, 0.5, 403)
    regions = [[(len(left), len(left) + 300), (len(t) - 100, len(t) + 50), (len(t) + 10, len(s))], [(100, 400)]]
    ctx.set_models([m.buf for m in bins])
    got = ctx.find_genes_batch([s, plain], meta=True, regions=regions, trim_terminal_repeats=True)
    want = ctx.find_genes_batch([t, plain], meta=True, regions=[tref.clip_regions(regions[0], len(t)), regions[1]], circular=[True, False])
    assert got.terminal_repeats.tolist() == [k, 0]
    assert tref.clip_regions(regions[0], len(t)) == [(len(left), len(left) + 300), (len(t) - 100, len(t))]
    assert got.genes.tobytes() == want.genes.tobytes() and got.cuts.tolist() == want.cuts.tolist()
    for i in range(2):
        assert np.array_equal(got.masks[i], want.masks[i])
    assert got.masks[0].tolist() == [[len(left), len(left) + 300], [len(t) - 100, len(t)]]


# ---------------------------------------------------------------------------------------------- the call

def same_call(got, want):
    """Two BatchResults of the C-ABI: every record, contig field and cut."""
    assert got.genes.tobytes() == want.genes.tobytes()
    for k in ("model", "n_nodes", "gene_begin", "n_genes", "n_unknown", "gc", "score"):
        assert np.array_equal(got.contigs[k], want.contigs[k]), k
    assert (got.cuts is None and want.cuts is None) or got.cuts.tolist() == want.cuts.tolist()


def gene_key(genes):
    out = io.StringIO()
    if genes.training_info is not None:
        genes.write_gff(out, "s")
    text = re.sub(r"seqnum=\d+;", "", out.getvalue())    # (the finder counts its sequences: not a property of the call)
    return (genes.circular, genes.cut, bytes(genes.sequence.data), text,
            [(g.begin, g.end, g.strand, g.partial_begin, g.partial_end, g.start_type, g.rbs_motif, g.rbs_spacer, g.gc_cont, g.score,
              g.cscore, g.sscore, g.rscore, g.uscore, g.tscore, g.translate(), g.sequence()) for g in genes])


def end_to_end(ctx, finder, models, meta, S_list, T_list, flags, trims, **kw):
    ctx.set_models([m.buf for m in models])
    got = ctx.find_genes_batch(S_list, meta=meta, trim_terminal_repeats=True, **kw)
    want = ctx.find_genes_batch(T_list, meta=meta, circular=flags, **kw)
    same_call(got, want)
    assert got.terminal_repeats.tolist() == trims
    a = finder.find_genes_batch(S_list, trim_terminal_repeats=True, translate=True)
    b = finder.find_genes_batch(T_list, circular=flags, translate=True)
    for x, y, t, s in zip(a, b, trims, T_list):
        assert gene_key(x) == gene_key(y)
        assert bytes(x.sequence.data) == s and x.terminal_repeat == t and x.circular == (t > 0)
        assert y.terminal_repeat is None and y.terminal_repeat_match is None
    return got, a


def meta_finder(lib, bins, **kw):
    mbins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=m.tobytes()), "bin %d" % i) for i, m in enumerate(bins)])
    return lib.GeneFinder(meta=True, metagenomic_bins=mbins, **kw)


def test_miij_with_a_gene_across_the_origin(ctx, lib, bins):
    s = cref.fixture("MIIJ01000039")
    t = s[MIIJ_ROTATION:] + s[:MIIJ_ROTATION]
    S = t + t[:127]
    assert tref.terminal_repeat(S)[:2] == (127, 127)
    oracle = cref.Circular(t, bins, True)                  # the CPU oracle alone: the circle has a gene across its origin
    assert [g for g in oracle.genes if g[1] > len(t)] == [(869424, 870140, -1)]
    got, genes = end_to_end(ctx, meta_finder(lib, bins), bins, True, [S], [t], [True], [127])
    gg = got.genes_of(0)
    assert [(int(b), int(e), int(st)) for b, e, st in zip(gg["begin"], gg["end"], gg["strand"])] == oracle.genes
    assert int(got.cuts[0]) == oracle.cut
    last = genes[0][len(genes[0]) - 1]
    assert (last.begin, last.end) == (869424, 870140) and last.end > len(genes[0].sequence)
    assert genes[0].terminal_repeat_match == 127


def test_100kb_single(ctx, lib):
    t = cref.fixture(KB100)
    models = cref.single_model(KB100_T)
    finder = lib.GeneFinder(lib.TrainingInfo(raw=models[0].tobytes()))
    end_to_end(ctx, finder, models, False, [t + t[:55]], [t], [True], [55])


def mixed_inputs():
    ts = [synthetic_contig(3000 + 2833 * n, 0.4 + 0.04 * n, 500 + n) for n in range(6)]          # 3 to 17 kbp
    ks = [33, 0, 1500, 127, 0, 20]
    S = [t + t[:k] for t, k in zip(ts, ks)]
    S += [b"", b"AC", synthetic_contig(20000, 0.5, 510), cref.fixture("KK037166")]
    T = ts + S[6:]
    return S, T, [k > 0 for k in ks] + [False] * 4, ks + [0] * 4


def test_six_synthetic_contigs_and_a_mixed_batch_meta(ctx, lib, bins):
    S, T, flags, ks = mixed_inputs()
    assert [tref.terminal_repeat(s)[1] for s in S] == ks
    got, genes = end_to_end(ctx, meta_finder(lib, bins), bins, True, S, T, flags, ks)
    assert sum(len(g) for g in genes) > 50
    # independent of circular=: a record either option names is a circle, whether or not a repeat is found
    finder = meta_finder(lib, bins)
    a = finder.find_genes_batch(S, trim_terminal_repeats=[True] * 5 + [False] * 5, circular=[False] * 8 + [True] * 2)
    b = finder.find_genes_batch(T[:5] + S[5:], circular=[k > 0 for k in ks[:5]] + [False] * 3 + [True] * 2)
    assert [gene_key(x) for x in a] == [gene_key(y) for y in b]
    assert [x.terminal_repeat for x in a] == ks[:5] + [None] * 5
    assert a[5].circular is False and len(a[5].sequence) == len(S[5]) and a[9].circular is True


def test_mixed_batch_single_with_training_infos(ctx, lib):
    S, T, flags, ks = mixed_inputs()
    m0, m1 = cref.single_model(SRR_T)[0], cref.single_model(KB100_T)[0]
    t0, t1 = lib.TrainingInfo(raw=m0.tobytes()), lib.TrainingInfo(raw=m1.tobytes())
    tinfs = [t0 if i % 2 == 0 else t1 for i in range(len(S))]
    finder = lib.GeneFinder(t0)
    tr = lib.TerminalRepeats()
    a = finder.find_genes_batch(S, training_infos=tinfs, trim_terminal_repeats=[tr] * len(S), translate=True)
    b = finder.find_genes_batch(T, training_infos=tinfs, circular=flags, translate=True)
    assert [gene_key(x) for x in a] == [gene_key(y) for y in b]
    assert [x.terminal_repeat for x in a] == ks and [x.terminal_repeat_match for x in a] == ks
    assert all(x.training_info is t for x, t in zip(a, tinfs))
    # the C-ABI with a model per contig
    ctx.set_models([m0.buf, m1.buf])
    moc = [i % 2 for i in range(len(S))]
    same_call(ctx.find_genes_batch(S, meta=False, model_of_contig=moc, trim_terminal_repeats=True),
              ctx.find_genes_batch(T, meta=False, model_of_contig=moc, circular=flags))
    # parameters: a longer minimum leaves the short repeats alone; a low-complexity repeat is reported and kept
    a = finder.find_genes_batch(S[:4], trim_terminal_repeats=lib.TerminalRepeats(min_length=100))
    assert [(x.terminal_repeat, x.terminal_repeat_match) for x in a] == [(0, 0), (0, 0), (1500, 1500), (127, 127)]
    poly = b"A" * 80 + synthetic_contig(5000, 0.5, 520)
    g = finder.find_genes(poly + poly[:60], trim_terminal_repeats=True)
    assert (g.terminal_repeat, g.terminal_repeat_match, g.circular, len(g.sequence)) == (0, 60, False, len(poly) + 60)


def test_option_forms_and_refusals(lib, bins):
    finder = meta_finder(lib, bins)
    s = synthetic_contig(3000, 0.5, 530)
    with pytest.raises(ValueError, match="entries"):
        finder.find_genes_batch([s, s], trim_terminal_repeats=[True])
    with pytest.raises(ValueError, match="two different"):
        finder.find_genes_batch([s, s], trim_terminal_repeats=[lib.TerminalRepeats(20), lib.TerminalRepeats(21)])
    with pytest.raises(ValueError, match="sets"):
        finder.find_genes_batch([s, s], sets=["a", "a"], trim_terminal_repeats=True)
    with pytest.raises(ValueError):
        lib.TerminalRepeats(min_length=0)
    with pytest.raises(ValueError):
        lib.TerminalRepeats(max_base_percent=10)
    out = finder.find_genes_batch([s, s], trim_terminal_repeats=[lib.TerminalRepeats(20), lib.TerminalRepeats(20)])      # equal: one set
    assert [g.terminal_repeat for g in out] == [0, 0]
    assert finder.find_genes(s).terminal_repeat is None and finder.find_genes(s, trim_terminal_repeats=False).terminal_repeat is None
    g = finder.find_genes(s + s[:25], trim_terminal_repeats=True)
    with pytest.raises(ValueError, match="circular"):
        g.write_scores(io.StringIO(), "s")


def test_a_call_that_does_not_ask_is_untouched(ctx, bins):
    S, T, flags, ks = mixed_inputs()
    ctx.set_models([m.buf for m in bins])
    b = ctx.upload(S)
    try:
        before = ctx.find_genes(b, meta=True, want_nodes=True)
        match, trim = b.terminal_repeats()
        assert trim.tolist() == ks
        after = ctx.find_genes(b, meta=True, want_nodes=True)
        same_call(before, after)
        assert before.cuts is None and after.cuts is None and after.terminal_repeats is None
        for x, y in zip(before.nodes, after.nodes):
            assert all(np.array_equal(x[k], y[k]) for k in x)
    finally:
        b.close()
    once = ctx.find_genes_batch(S, meta=True)
    same_call(before, once)


# ---------------------------------------------------------------------------------------------- text

WRITERS = {"gff": "write_gff", "faa": "write_translations", "fna": "write_genes"}


def test_device_text_equals_host_writers(ctx, lib):
    srr = cref.fixture("SRR492066")
    planted, orf = cref.planted_orf()
    S, ids = [srr + srr[:300], planted + planted[:64], srr], ["dtr", "planted", "linear"]
    tinf = lib.TrainingInfo(raw=cref.single_model(SRR_T)[0].tobytes())
    genes_list = lib.GeneFinder(tinf).find_genes_batch(S, trim_terminal_repeats=True)
    assert [g.terminal_repeat for g in genes_list] == [300, 64, 0] and [g.circular for g in genes_list] == [True, True, False]
    assert genes_list[0].cut == 52426 and any(g.end > len(planted) for g in genes_list[1])
    ctx.set_models([tinf.raw])
    b = ctx.upload(S)
    try:
        t = b.trim_terminal_repeats(b.terminal_repeats()[1])
        r = ctx.find_genes(t, meta=False)
        out = ctx.render_genes(t, r, ids, ("gff", "faa", "fna"))
        with pytest.raises(Exception, match="circular"):
            ctx.render_genes(t, r, ids, ("gbk",))
        t.close()
    finally:
        b.close()
    for fmt, writer in WRITERS.items():
        want = io.StringIO()
        for genes, sid in zip(genes_list, ids):
            getattr(genes, writer)(want, sid)
        assert out[fmt].fallback == 0
        assert out[fmt].data == want.getvalue().encode(), fmt
    assert b'seqlen=79939;seqhdr="dtr";topology=circular\n' in out["gff"].data
    gb = io.StringIO()
    genes_list[0].write_genbank(gb, "dtr")
    assert "79939 bp    DNA     circular BCT" in gb.getvalue() and "complement(join(79328..79939,1..177))" in gb.getvalue()


# ---------------------------------------------------------------------------------------------- threads

def test_thread_pool_pattern(lib):
    tinf = lib.TrainingInfo(raw=cref.single_model(SRR_T)[0].tobytes())
    srr = cref.fixture("SRR492066")
    seqs = [srr + srr[:90], cref.fixture("KK037166")] + [with_repeat(9000 + 500 * i, 40 * (i % 2), 700 + i, 0.45) for i in range(4)]
    lone = lib.GeneFinder(tinf)
    key = lambda g: (g.terminal_repeat, g.terminal_repeat_match) + gene_key(g)
    options = (False, True, lib.TerminalRepeats(min_length=50))
    want = {(i, o): key(lone.find_genes(s, trim_terminal_repeats=options[o])) for i, s in enumerate(seqs) for o in range(3)}
    assert want[(0, 1)][0] == 90 and want[(0, 0)][0] is None and want[(3, 1)][0] == 40 and want[(3, 2)][0] == 0
    finder = lib.GeneFinder(tinf, contexts=2)
    got, errors = {}, []
    start = threading.Barrier(24)

    def work(t):
        try:
            start.wait()
            for rep in range(3):
                i, o = (t + rep) % len(seqs), (t + 2 * rep) % 3
                got[(t, rep)] = ((i, o), key(finder.find_genes(seqs[i], trim_terminal_repeats=options[o])))
        except BaseException as e:          # noqa: reported below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(24)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(got) == 72
    for k, res in got.values():
        assert res == want[k], k


# ---------------------------------------------------------------------------------------------- files and the command line

def three_records(tmp_path):
    """An assembler-style file (a circle written with its overlap, a linear contig whose header says circular, a record with poly-A
    ends) and the same file trimmed by hand."""
    srr, kk = cref.fixture("SRR492066").decode(), cref.fixture("KK037166").decode()
    poly = "A" * 80 + synthetic_contig(5000, 0.5, 520).decode()
    records = [("dtr1 flag=1 multi=9.0 len=80029", srr + srr[:90]), ("lin circular=true", kk), ("polyA", poly + poly[:60])]
    trimmed = [("dtr1 flag=1 multi=9.0 len=80029", srr), ("lin circular=true", kk), ("polyA", poly + poly[:60])]
    paths = []
    for name, recs in (("asm.fna", records), ("trimmed.fna", trimmed)):
        paths.append(tmp_path / name)
        with open(paths[-1], "w") as f:
            for h, s in recs:
                f.write(">%s\n" % h)
                f.writelines(s[k:k + 80] + "\n" for k in range(0, len(s), 80))
    tfile = tmp_path / "model.bin"
    with gzip.open(golden_path(SRR_T), "rb") as src, open(tfile, "wb") as dst:
        dst.write(src.read())
    report = "dtr1\t80029\t90\t90\ttrimmed\nlin\t20000\t0\t0\tnone\npolyA\t5140\t60\t0\tlow_complexity\n"
    return paths[0], paths[1], tfile, report


def test_command_line_detects_what_the_hand_trimmed_run_is_told(tmp_path):
    asm, trimmed, tfile, report = three_records(tmp_path)
    (tmp_path / "ids.txt").write_text("dtr1\nlin\n")
    o1, a1, d1, o2, a2, d2, rep = (tmp_path / n for n in ("1.gff", "1.faa", "1.fna", "2.gff", "2.faa", "2.fna", "report.tsv"))
    run = subprocess.run([sys.executable, "-m", "pyrodigal_amd", "-i", str(asm), "-t", str(tfile), "-o", str(o1), "-a", str(a1), "-d", str(d1),
                          "--circular-detect", "--circular-from-header", "--circular-report", str(rep)], cwd=ROOT, capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr.decode()
    run = subprocess.run([sys.executable, "-m", "pyrodigal_amd", "-i", str(trimmed), "-t", str(tfile), "-o", str(o2), "-a", str(a2), "-d", str(d2),
                          "--circular-ids", str(tmp_path / "ids.txt")], cwd=ROOT, capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr.decode()
    assert o1.read_bytes() == o2.read_bytes() and a1.read_bytes() == a2.read_bytes() and d1.read_bytes() == d2.read_bytes()
    gff = o1.read_bytes()
    assert gff.count(b"topology=circular") == 2 and b'seqlen=79939;seqhdr="dtr1";topology=circular' in gff
    assert b"\t79328\t80116\t" in gff and b'seqlen=5140;seqhdr="polyA"\n' in gff
    assert rep.read_text() == report


def test_files_through_the_pipeline(tmp_path):
    from pyrodigal_amd import pipeline
    asm, trimmed, tfile, report = three_records(tmp_path)
    blobs = [np.frombuffer(tfile.read_bytes(), np.uint8)]
    import datetime
    date = datetime.date(2024, 5, 17)
    got, want = {k: io.BytesIO() for k in ("gff", "gbk")}, {k: io.BytesIO() for k in ("gff", "gbk")}
    stats = pipeline.render_fasta(str(asm), blobs, gbk_options={"date": date}, trim_terminal_repeats=True, **got)
    ref = pipeline.render_fasta(str(trimmed), blobs, gbk_options={"date": date}, circular={"dtr1"}, **want)
    assert got["gff"].getvalue() == want["gff"].getvalue() and got["gbk"].getvalue() == want["gbk"].getvalue()
    assert b"79939 bp    DNA     circular BCT 17-MAY-24" in got["gbk"].getvalue() and b"complement(join(79328..79939,1..177))" in got["gbk"].getvalue()
    assert stats["terminal_repeats"] == [("dtr1", 80029, 90, 90), ("polyA", 5140, 60, 0)]
    assert [r[:2] for r in stats["terminal_repeat_records"]] == [("dtr1", 80029), ("lin", 20000), ("polyA", 5140)]
    assert stats["genes"] == ref["genes"] and "terminal_repeats" not in ref
    # a batch without any repeat keeps the device's GenBank renderer; the stricter minimum finds nothing
    class Longer:
        min_length, max_length, max_base_percent = 100, 65536, 75
    out = io.BytesIO()
    stats = pipeline.render_fasta(str(trimmed), blobs, gbk=out, gbk_options={"date": date}, trim_terminal_repeats=Longer)
    lin = io.BytesIO()
    pipeline.render_fasta(str(trimmed), blobs, gbk=lin, gbk_options={"date": date})
    assert out.getvalue() == lin.getvalue() and stats["terminal_repeats"] == []
    with pytest.raises(ValueError, match="start-score"):
        pipeline.render_fasta(str(asm), blobs, scores=io.BytesIO(), trim_terminal_repeats=True)
    # the generator form
    trims = []
    for ids, descs, lens, r in pipeline.find_genes_fasta(str(asm), blobs, meta=False, trim_terminal_repeats=True):
        trims += r.terminal_repeats.tolist()
        assert r.cuts[0] == 52426 and r.cuts[1] == -1
    assert trims == [90, 0, 0]
