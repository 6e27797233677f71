"""Masked regions from three sources -- runs of unknown bases, runs of lower-case letters, the caller's own intervals -- merged
on the device (DESIGN.md "Region masks").

Exact tests: a region takes part in the mask test exactly as a masked run of N at the same coordinates would, so wherever the
bases under the regions ARE unknown the CPU oracle (which only knows N-runs) is the reference, node field for node field.
Property tests: for real bases under a mask there is no oracle; what must hold is stated in each test."""
import io
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from oracle import oracle as orc
from tests.mask_ref import runs_of, union          # (the reference of every reported list, shared with tests/mask_shapes.py)
from tests.test_finder_gpu import _with_unknown_runs, compare_contig
from tests.util import golden_path, read_fasta, synthetic_contig

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
def models():
    m = [orc.Training.load(golden_path("SRR492066.training.bin.gz")),
         orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz")),
         orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic.tinf_closed.bin.gz"))]
    for src, gc, tt in [(0, 0.36, 11), (1, 0.47, 11), (2, 0.42, 4), (0, 0.33, 4), (1, 0.64, 11)]:
        t = m[src].copy(); t.set_gc(gc); t.set_trans_table(tt); m.append(t)
    return m


def masking_inputs():
    """The inputs of tests/test_finder_gpu.py::test_region_masking_single_and_meta."""
    return [_with_unknown_runs(30000, 0.45, 70, [9, 10, 11, 49, 50, 51, 120, 400, 1500]),
            _with_unknown_runs(12000, 0.6, 71, [50] * 12),
            b"N" * 70 + synthetic_contig(4000, 0.5, 72) + b"N" * 55,
            synthetic_contig(3000, 0.5, 73),
            synthetic_contig(5000, 0.5, 74) + b"NNN",
            b"N" * 400, b""]


def recs(genes):
    """Everything a Gene reports, for bit-for-bit comparisons of two calls through the host layer."""
    return [(g.begin, g.end, g.strand, g.partial_begin, g.partial_end, g.start_type, g.rbs_motif, g.rbs_spacer, g.gc_cont, g.cscore,
             g.rscore, g.sscore, g.tscore, g.uscore, g.score) for g in genes]


def same_calls(a, b):
    """Two gene record arrays of one sequence (possibly at different places of their batches) hold the same calls."""
    return len(a) == len(b) and all(np.array_equal(a[k], b[k]) for k in ("begin", "end", "strand", "start_ndx", "stop_ndx", "start_type"))


def check_against_oracle(ctx, models, seqs, oracle_kw, **device_kw):
    """Both modes, closed and open, every node field and gene of every contig."""
    for meta in (True, False):
        use = models if meta else [models[1]]
        ctx.set_models([m.buf for m in use])
        for closed in (False, True):
            res = ctx.find_genes_batch(seqs, meta=meta, closed=closed, want_nodes=True, **device_kw)
            n = 0
            for i, s in enumerate(seqs):
                n += compare_contig(res, i, s, orc.Oracle(s, **oracle_kw), use, meta=meta, closed=closed)
            assert n > 0
    return res


# ---------------------------------------------------------------------------------------------- exact, against the oracle

@pytest.mark.parametrize("min_mask", [50, 10])
def test_named_regions_equal_unknown_runs(ctx, models, min_mask):
    seqs = masking_inputs()
    regions = [orc.Oracle(s, mask=True, mask_size=min_mask).masks() for s in seqs]
    res = check_against_oracle(ctx, models, seqs, dict(mask=True, mask_size=min_mask), mask=False, regions=regions)
    for i in range(len(seqs)):
        assert np.array_equal(res.masks[i], regions[i])


@pytest.mark.parametrize("min_mask", [50, 10])
def test_the_union_is_exact_for_split_duplicated_and_shuffled_regions(ctx, models, min_mask):
    seqs = masking_inputs()
    rng = np.random.default_rng(5)
    regions = []
    for s in seqs:
        pieces = []
        for b, e in orc.Oracle(s, mask=True, mask_size=min_mask).masks().tolist():
            if e - b >= 4:                      # two overlapping pieces
                cut = int(rng.integers(b + 1, e - 1))
                pieces += [(b, min(e, cut + 1 + int(rng.integers(0, 3)))), (cut, e)]
            else:
                pieces.append((b, e))
            if rng.random() < 0.5:
                pieces.append(pieces[-1])       # a duplicate
        rng.shuffle(pieces)
        regions.append([tuple(p) for p in pieces])
    res = check_against_oracle(ctx, models, seqs, dict(mask=True, mask_size=min_mask), mask=False, regions=regions)
    for i, s in enumerate(seqs):
        assert np.array_equal(res.masks[i], orc.Oracle(s, mask=True, mask_size=min_mask).masks())


def test_the_union_joins_unknown_runs_and_named_regions(ctx, models):
    seqs = [_with_unknown_runs(30000, 0.45, 80, [30, 35, 49, 50, 51, 64, 200, 31, 48, 1000]),
            _with_unknown_runs(15000, 0.55, 81, [30, 49] * 4 + [50, 80] * 3),
            synthetic_contig(4000, 0.5, 82) + b"N" * 40]          # reaches the end: masked under either rule
    regions = []
    for s in seqs:
        long_runs = {tuple(x) for x in orc.Oracle(s, mask=True, mask_size=50).masks().tolist()}
        short = [tuple(x) for x in orc.Oracle(s, mask=True, mask_size=30).masks().tolist() if tuple(x) not in long_runs]
        regions.append(short)
    assert sum(len(r) for r in regions) >= 8
    res = check_against_oracle(ctx, models, seqs, dict(mask=True, mask_size=30), mask=True, min_mask=50, regions=regions)
    for i, s in enumerate(seqs):
        assert np.array_equal(res.masks[i], orc.Oracle(s, mask=True, mask_size=30).masks())


@pytest.mark.parametrize("min_mask", [10, 50])
def test_lower_case_runs_equal_unknown_runs(ctx, models, min_mask):
    seqs = masking_inputs()                      # ... with the run that reaches the end of its sequence and the b"N" * 400 contig
    soft = [s.upper().replace(b"N", b"n") for s in seqs]
    assert any(b"n" in s for s in soft) and not any(b"N" in s for s in soft)
    for meta in (True, False):
        use = models if meta else [models[1]]
        ctx.set_models([m.buf for m in use])
        for closed in (False, True):
            res = ctx.find_genes_batch(soft, meta=meta, closed=closed, want_nodes=True, mask=False, mask_lowercase=True, min_mask=min_mask)
            for i, s in enumerate(seqs):
                o = orc.Oracle(s, mask=True, mask_size=min_mask)
                compare_contig(res, i, s, o, use, meta=meta, closed=closed)
                assert np.array_equal(res.masks[i], o.masks())


def test_reported_lists_are_the_merged_union(ctx, lib, models):
    body = synthetic_contig(6000, 0.5, 90)
    cases = [   # (sequence, regions, mask_lowercase runs expected from the letters)
        (body, [(10, 20), (20, 30), (30, 31), (100, 200), (150, 160), (199, 260), (5000, 6000)]),   # touching, nested, overlapping
        (synthetic_contig(3000, 0.45, 91), None),                                                 # none
        (b"", None), (b"A", [(0, 1)]), (b"AC", [(0, 1), (1, 2)]), (b"G", None), (b"TT", [(1, 2)]),
        (synthetic_contig(900, 0.5, 92), [(0, 900)]),                                             # a whole contig
        (synthetic_contig(900, 0.5, 93), [(0, 450), (450, 900), (3, 4)]),                          # a whole contig from pieces
        (body[:2000] + b"N" * 60 + body[2000:4000].lower() + body[4000:], [(1990, 2010), (4059, 4100)]),
    ]
    seqs = [c[0] for c in cases]
    regions = [c[1] for c in cases]
    ctx.set_models([m.buf for m in models])
    for mask, lower, mm in ((False, False, 50), (True, True, 50), (True, False, 10), (False, True, 1)):
        want = []
        for s, r in cases:
            a = np.frombuffer(s, np.uint8)
            iv = list(r or [])
            if mask:
                iv += runs_of(~np.isin(a, np.frombuffer(b"ACGTacgt", np.uint8)), mm).tolist()
            if lower:
                iv += runs_of((a >= 97) & (a <= 122), mm).tolist()
            want.append(union(iv))
        res = ctx.find_genes_batch(seqs, meta=True, mask=mask, min_mask=mm, regions=regions, mask_lowercase=lower)
        assert [m.tolist() for m in res.masks] == [w.tolist() for w in want]
        for s, r, w in zip(seqs, regions, want):
            got = lib.Sequence(s, mask=mask, mask_size=mm, regions=r, mask_lowercase=lower).masks
            assert isinstance(got, lib.Masks) and got == [tuple(x) for x in w.tolist()]
    # the C-ABI names the sequence and the interval it refuses
    for bad in ([(5, 5)], [(-1, 4)], [(10, 901)], [(8, 3)]):
        with pytest.raises(ValueError, match=r"sequence 7: interval \[-?\d+, \d+\)"):
            ctx.find_genes_batch(seqs, meta=True, regions=[None] * 7 + [bad] + [None] * 2)


def test_training_under_named_regions_is_training_under_unknown_runs(ctx, lib):
    s = bytearray(read_fasta("GCF_001457455.1_NCTC11397_genomic_100kb.fna.gz")[0][1].encode())
    for at, n in ((4000, 60), (20500, 400), (47000, 50), (61234, 1000), (88000, 120), (99950, 50)):
        s[at:at + n] = b"N" * n
    s = bytes(s)
    o = orc.Oracle(s, mask=True)
    want = o.train().tobytes()
    regions = o.masks()
    assert len(regions) == 6 and want != orc.Oracle(s).train().tobytes()
    assert ctx.train(s, mask=True) == want
    assert ctx.train(s, mask=False, regions=regions) == want
    s2 = bytearray(read_fasta("SRR492066.fna.gz")[0][1].encode())
    for at, n in ((3000, 70), (30000, 300), (60000, 55)):
        s2[at:at + n] = b"N" * n
    s2 = bytes(s2)
    o2 = orc.Oracle(s2, mask=True)
    both = [want, o2.train().tobytes()]
    assert ctx.train_batch([s, s2], mask=True) == both
    assert ctx.train_batch([s, s2], mask=False, regions=[regions, o2.masks()]) == both
    # ... and through the host layer; two contigs of one genome carry their regions through the join
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert lib.GeneFinder().train(s, regions=regions).raw.tobytes() == want
        assert [t.raw.tobytes() for t in lib.GeneFinder().train_batch([s, s2], regions=[regions, o2.masks()])] == both
        a, b = s[:50000], s[50000:]
        ra = [(x, y) for x, y in regions.tolist() if y <= 50000]
        rb = [(x - 50000, y - 50000) for x, y in regions.tolist() if x >= 50000]
        assert len(ra) + len(rb) == 6
        joined = a + b"TTAATTAATTAA" + b + b"TTAATTAATTAA"
        assert lib.GeneFinder().train(a, b, regions=[ra, rb]).raw.tobytes() == orc.Oracle(joined, mask=True).train().tobytes()


# ---------------------------------------------------------------------------------------------- properties: real bases under a mask

def seeded_regions(genome_len, genes, n=80, seed=11, spacing=25000, longest=2000):
    """n regions of 50 .. longest bp, one per slot of the genome, every second one inside a gene; at least `spacing` apart."""
    rng = np.random.default_rng(seed)
    slot = genome_len // n
    room = slot - spacing - longest
    assert room > 500
    begins = np.array([g.begin - 1 for g in genes]); ends = np.array([g.end for g in genes])
    out, in_genes = [], 0
    for k in range(n):
        lo = k * slot
        length = int(rng.integers(50, longest + 1))
        b = lo + int(rng.integers(0, room))
        if k % 2 == 0:
            ok = np.flatnonzero((begins >= lo) & (begins + 10 < lo + room) & (ends - begins >= 100))
            if len(ok):
                g = int(ok[int(rng.integers(0, len(ok)))])
                b = int(begins[g]) + 10
                length = min(length, int(ends[g] - begins[g]) - 20)
                in_genes += 1
        out.append((b, b + length))
    assert in_genes >= n // 2 - 2
    return out


def test_real_bases_under_a_mask(lib):
    """The reference can only mask runs of N; the oracle for masked regions whose bases are known is tests/extract_ref.py, the sweep
    restated with the mask list as an argument (tests/test_extract_shapes_gpu.py::test_named_regions_over_known_bases holds the
    device against it, the boundary case of DESIGN.md 4.9 included).  What must hold on a whole genome, whatever the nodes are:
    no gene touches a region, the calls change, nothing else in the batch changes, the sequence statistics and the printed letters
    are those of the unmasked input, and lower-casing the regions is the same as naming them."""
    genome = read_fasta("GCF_001457455.1_NCTC11397_genomic.fna.gz")[0][1].upper().encode()
    others = [read_fasta("SRR492066.fna.gz")[0][1].upper().encode(), synthetic_contig(60000, 0.5, 17)]
    tinf = lib.TrainingInfo.load(golden_path("GCF_001457455.1_NCTC11397_genomic.tinf_closed.bin.gz"))
    finder = lib.GeneFinder(tinf)
    plain = finder.find_genes_batch([genome] + others)
    regions = seeded_regions(len(genome), list(plain[0]))
    srt = sorted(regions)
    assert len(regions) == 80 and all(50 <= e - b <= 2000 for b, e in regions)
    assert all(srt[k + 1][0] - srt[k][1] >= 25000 for k in range(len(srt) - 1))       # the boundary note of DESIGN.md cannot apply
    masked = finder.find_genes_batch([genome] + others, regions=[regions, None, None])
    assert masked[0].sequence.masks == srt
    for g in masked[0]:
        assert not any(b < g.end and g.begin - 1 < e for b, e in regions), (g.begin, g.end)
    calls = lambda genes: [(g.begin, g.end, g.strand) for g in genes]
    assert calls(masked[0]) != calls(plain[0])
    hit = [g for g in plain[0] if any(b < g.end and g.begin - 1 < e for b, e in regions)]
    assert len(hit) >= 38                                                            # the unmasked call did run genes across them
    for k in (1, 2):                                                                 # the rest of the batch: bit-identical
        assert recs(masked[k]) == recs(plain[k]) and masked[k].score == plain[k].score
        assert masked[k].sequence.masks == []
    for k in range(3):
        assert masked[k].sequence.gc == plain[k].sequence.gc and masked[k].sequence.unknown == plain[k].sequence.unknown
    out = io.StringIO()
    masked[0].write_genes(out, "genome")
    text = genome.decode()
    comp = str.maketrans("ACGT", "TGCA")
    lines = out.getvalue().split(">")[1:]
    assert len(lines) == len(masked[0])
    for g, rec in zip(masked[0], lines):
        letters = "".join(rec.split("\n")[1:])
        want = text[g.begin - 1:g.end]
        assert letters == (want if g.strand == 1 else want.translate(comp)[::-1])
    soft = bytearray(genome)
    for b, e in regions:
        soft[b:e] = bytes(soft[b:e]).lower()
    lower = lib.GeneFinder(tinf, mask_lowercase=True, min_mask=50).find_genes(bytes(soft))
    assert recs(lower) == recs(masked[0]) and lower.sequence.masks == srt


# ---------------------------------------------------------------------------------------------- scale

def long_soft_masked_contig(total=50_000_000, n=250_000, seed=23):
    """A contig with n lower-case runs (20 .. 49 letters, one per 100 bases of its first half: soft-masked repeats cluster) and as
    many named intervals: most overlap the runs at random, the rest fall anywhere.  Returns (letters, named, is_lower)."""
    rng = np.random.default_rng(seed)
    seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, total, dtype=np.uint8)]
    b = np.arange(n) * 100 + rng.integers(0, 30, n)
    ln = rng.integers(20, 50, n)
    at = np.repeat(b, ln) + np.arange(int(ln.sum())) - np.repeat(np.cumsum(ln) - ln, ln)
    lower = np.zeros(total, bool)
    lower[at] = True
    seq[lower] |= 0x20
    near = n * 4 // 5
    nb = np.concatenate([np.maximum(b[:near] + rng.integers(-40, 40, near), 0), rng.integers(0, total - 100, n - near)])
    named = np.stack([nb, nb + rng.integers(1, 60, n)], axis=1).astype(np.int32)
    return seq.tobytes(), named[rng.permutation(n)], lower


def test_scale_one_long_contig(ctx, models):
    seq, named, lower = long_soft_masked_contig()
    runs = runs_of(lower, 20)
    assert len(runs) == 250_000 and len(named) == 250_000
    want = union(np.concatenate([runs, named]))
    assert 250_000 < len(want) < 400_000                        # many of the named intervals joined a run
    ctx.set_models([models[2].buf])
    res = ctx.find_genes_batch([seq], meta=False, mask=False, min_mask=20, mask_lowercase=True, regions=[named])
    assert np.array_equal(res.masks[0], want)
    assert ctx.dp_stats()["segments"] > 0                       # the call completed on the segmented connection-scoring path
    assert res.contigs[0]["n_genes"] > 0 and res.contigs[0]["n_unknown"] == 0      # the lower-case letters still read as their bases


def test_scale_many_contigs_few_with_regions(ctx, models):
    seqs = [synthetic_contig(4000 + 37 * (c % 50), 0.35 + 0.3 * (c % 31) / 30, 3000 + c) for c in range(1000)]
    rng = np.random.default_rng(31)
    regions = [None] * 1000
    for c in rng.choice(1000, 10, replace=False):
        b = rng.integers(0, len(seqs[c]) - 300, 40)
        regions[c] = np.stack([b, b + rng.integers(1, 300, 40)], axis=1)
    ctx.set_models([m.buf for m in models])
    plain = ctx.find_genes_batch(seqs, meta=True)
    res = ctx.find_genes_batch(seqs, meta=True, regions=regions)
    changed = 0
    for c in range(1000):
        if regions[c] is None:
            assert len(res.masks[c]) == 0
            assert res.genes_of(c).tobytes() == plain.genes_of(c).tobytes()
            assert res.contigs[c]["model"] == plain.contigs[c]["model"] and res.contigs[c]["score"] == plain.contigs[c]["score"]
        else:
            assert np.array_equal(res.masks[c], union(regions[c]))
            changed += not same_calls(res.genes_of(c), plain.genes_of(c))
    assert changed > 0


# ---------------------------------------------------------------------------------------------- plumbing

def test_replicate_keeps_the_mask_sources(ctx, models):
    seqs = [synthetic_contig(9000, 0.5, 41), synthetic_contig(7000, 0.45, 42).lower()[:3000] + synthetic_contig(4000, 0.45, 43)]
    regions = [[(100, 900), (850, 1200), (5000, 5001)], [(6000, 6100)]]
    ctx.set_models([m.buf for m in models])
    b = ctx.upload(seqs).set_masks(regions, mask_lowercase=True)
    try:
        src = ctx.find_genes(b, meta=True)
        assert [m.tolist() for m in src.masks] == [[[100, 1200], [5000, 5001]], [[0, 3000], [6000, 6100]]]
        rep = ctx.replicate(b, [1, 0, 1])
        try:
            got = ctx.find_genes(rep, meta=True)
            for k, s in enumerate((1, 0, 1)):
                assert np.array_equal(got.masks[k], src.masks[s])
                assert len(src.genes_of(s)) > 0 and same_calls(got.genes_of(k), src.genes_of(s))
        finally:
            rep.close()
        b.set_masks(None, False)                                   # detached again: the plain call
        assert ctx.find_genes(b, meta=True).masks is None
    finally:
        b.close()


def test_host_tail_agrees(ctx, models, monkeypatch):
    monkeypatch.setenv("PGA_TAIL", "host")
    seqs = masking_inputs()
    regions = [orc.Oracle(s, mask=True, mask_size=50).masks() for s in seqs]
    check_against_oracle(ctx, models, seqs, dict(mask=True, mask_size=50), mask=False, regions=regions)


def test_thread_pool_keeps_each_callers_regions(lib):
    from multiprocessing.pool import ThreadPool
    tinf = lib.TrainingInfo.load(golden_path("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz"))
    seqs = [synthetic_contig(20000 + 500 * k, 0.5, 600 + k) for k in range(64)]
    regions = [None if k % 4 == 3 else [(1000 + 100 * k, 1500 + 150 * k), (9000, 9000 + 10 * (k + 1))] for k in range(64)]
    one = lib.GeneFinder(tinf, contexts=1)
    want = [one.find_genes(s, regions=r) for s, r in zip(seqs, regions)]
    finder = lib.GeneFinder(tinf)
    with ThreadPool(32) as pool:
        got = pool.starmap(finder.find_genes, zip(seqs, regions))
    assert finder.stats["max_calls_per_device_call"] > 1
    for k in range(64):
        assert recs(got[k]) == recs(want[k])
        assert got[k].sequence.masks == ([] if regions[k] is None else union(regions[k]).tolist())
    assert any(recs(want[k]) != recs(one.find_genes(seqs[k])) for k in range(64))


def test_command_line_agrees_with_the_api(lib, tmp_path):
    recs = [("soft", synthetic_contig(60000, 0.5, 71).decode()), ("named", synthetic_contig(45000, 0.45, 72).decode()),
            ("plain", synthetic_contig(30000, 0.55, 73).decode())]
    soft = bytearray(recs[0][1].encode())
    for b, e in ((2000, 2300), (30000, 30049), (41000, 43000)):
        soft[b:e] = bytes(soft[b:e]).lower()
    recs[0] = ("soft", soft.decode())
    named = [(500, 700), (650, 900), (20000, 21000)]
    fasta = tmp_path / "in.fna"
    with open(fasta, "w") as f:
        for sid, s in recs:
            f.write(">%s some description\n" % sid)
            for k in range(0, len(s), 70):
                f.write(s[k:k + 70] + "\n")
    bed = tmp_path / "regions.bed"
    bed.write_text("# comment\ntrack name=x\nnamed\t500\t700\tfeature\t0\t+\nnamed\t20000\t21000\nnamed\t650\t900\nabsent\t1\t5\n")
    model = tmp_path / "model.bin"
    tinf = lib.TrainingInfo.load(golden_path("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz"))
    with open(model, "wb") as fh:
        tinf.dump(fh)
    for fmt in ("gff", "gbk"):
        finder = lib.GeneFinder(tinf, mask_lowercase=True)             # (a fresh one: its sequence numbers start at 1, like a run's)
        o, a, d = tmp_path / ("o." + fmt), tmp_path / "a.faa", tmp_path / "d.fna"
        r = subprocess.run([sys.executable, "-m", "pyrodigal_amd", "-i", str(fasta), "-t", str(model), "-f", fmt, "-o", str(o), "-a", str(a),
                            "-d", str(d), "--mask-regions", str(bed), "--mask-lowercase"], cwd=ROOT, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()
        assert "absent" in r.stderr.decode() and "Warning" in r.stderr.decode()
        out, faa, fna = io.StringIO(), io.StringIO(), io.StringIO()
        n_masked = 0
        for sid, s in recs:
            g = finder.find_genes(s, regions=named if sid == "named" else None)
            n_masked += len(g.sequence.masks)
            (g.write_genbank if fmt == "gbk" else g.write_gff)(out, sid)
            g.write_translations(faa, sid)
            g.write_genes(fna, sid)
        assert n_masked == 4
        assert o.read_bytes() == out.getvalue().encode()
        assert a.read_bytes() == faa.getvalue().encode() and d.read_bytes() == fna.getvalue().encode()
    unmasked = io.StringIO()
    for sid, s in recs:
        lib.GeneFinder(tinf).find_genes(s).write_gff(unmasked, sid)
    assert unmasked.getvalue().encode() != (tmp_path / "o.gff").read_bytes()
    # single mode without -t: the training honours the masks too
    o2 = tmp_path / "trained.gff"
    r = subprocess.run([sys.executable, "-m", "pyrodigal_amd", "-i", str(fasta), "-o", str(o2), "--mask-regions", str(bed), "--mask-lowercase"],
                       cwd=ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    trainer = lib.GeneFinder(mask_lowercase=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        trainer.train(*[s for _, s in recs], regions=[None, named, None])
    out = io.StringIO()
    for sid, s in recs:
        trainer.find_genes(s, regions=named if sid == "named" else None).write_gff(out, sid)
    assert o2.read_bytes() == out.getvalue().encode()
