"""Bottom-s MinHash sketches of predicted proteins, or of the genes' bases, on the device, and their pairwise comparison
(pga_sketch_proteins, pga_sketch_pairs, ProteinSketches, Context.protein_sketches, DeviceSketches.compare,
GeneFinder.find_sketches_batch).

Every expected value comes from the plain-Python restatement of the rule (tests/protein_sketches_ref.py) over the strings of
tests/protein_groups_ref.string_of -- never from the code under test -- and the device must give the same integers, bit for bit.
Device memory comes from tests/hip_mem.py (no torch), but for the finder test, which runs in a child process.  Every output lies inside
an allocation full of a canary byte, and the whole allocation is compared."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hip_mem, tables_ref
from tests import protein_groups_ref as groups_ref
from tests import protein_sketches_ref as ref

pytestmark = pytest.mark.gpu

CANARY = 0xA5
SIZES = (1, 2, 31, 32, 33, 63, 64)
K_OF = {"protein": (1, 3, 5, 8), "gene": (1, 11, 31, 32)}
REDUCED = ("LVIM", "C", "A", "G", "ST", "P", "FYW", "EDNQ", "KR", "H")


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi, benchdata
    c = _cabi.Context(0)
    c.set_models([b for _, b in benchdata.load_model_set()])
    yield c
    c.close()


LIVE = []        # what a test put on the device: closed when the test ends, passed or failed, while the module's context still exists


@pytest.fixture(autouse=True)
def release_device_objects():
    yield
    while LIVE:
        LIVE.pop().close()


def keep(x):
    LIVE.append(x)
    return x


class View:
    """A pointer into somebody's device memory with a shape: what `out=` takes."""

    def __init__(self, ptr, shape, typestr="<i8"):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (ptr, False), "version": 3, "strides": None}


class Target:
    """Allocations full of a fill byte, and in each an int64 tensor of one of `shapes` that begins 8 bytes into it, with `slack`
    elements behind.  `given`: which of them are passed at all.  `expect()` is what the whole allocations must hold after a call."""

    def __init__(self, shapes, given=None, slack=5, fill=CANARY):
        self.shapes = [tuple(s) for s in shapes]
        self.given = tuple(given) if given is not None else (True,) * len(shapes)
        self.before = [np.full(8 * (1 + int(np.prod(s)) + slack), fill, np.uint8) for s in self.shapes]
        self.mem = [keep(hip_mem.DeviceArray.from_numpy(b)) for b in self.before]
        self.out = tuple(View(m.ptr + 8, s) if on else None for m, s, on in zip(self.mem, self.shapes, self.given))

    def read(self):
        return [m.to_numpy(np.int64) for m in self.mem]

    def expect(self, *want):
        out = [b.view(np.int64).copy() for b in self.before]
        for e, w, on in zip(out, want, self.given):
            if on:
                w = np.asarray(w, np.int64).reshape(-1)
                e[1:1 + len(w)] = w
        return out

    def untouched(self):
        return all(np.array_equal(m.to_numpy(np.uint8), b) for m, b in zip(self.mem, self.before))


def sketch_target(G, s, windows=True, fill=CANARY):
    return Target([(G, s), (G,), (G,)], given=(True, True, windows), fill=fill)


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def gene_array(recs):
    from pyrodigal_amd import _cabi
    genes = np.zeros(len(recs), _cabi.GENE_DTYPE)
    if len(recs):
        for name, col in zip(("contig", "begin", "end", "strand", "partial_begin", "partial_end"), zip(*recs)):
            genes[name] = col
    return genes


class Case:
    def __init__(self, seqs, circular, tables, records, **named):
        self.seqs, self.circular, self.tables, self.records = seqs, circular, np.array(tables, np.int32), records
        self.named = named                                     # record indices by name


def upload(ctx, case):
    batch = keep(ctx.upload(case.seqs))
    if any(case.circular):
        batch.set_circular(case.circular)
    return batch


def run(ctx, batch, case, k, s, unit="protein", records=None, windows=True, fill=CANARY, seed=0, classes=None, **options):
    """One call into a Target: (what the allocations hold, what they must hold, the DeviceSketches, the reference's tuple)."""
    from pyrodigal_amd import ProteinSketches
    records = case.records if records is None else records
    tables = options.pop("tables", case.tables)
    table = None if classes is None else (ref.classes_of(classes) if isinstance(classes[0], str) else list(classes))
    want = ref.protein_sketches_ref(case.seqs, case.circular, records, k, s, unit, seed, table, tables, **options)
    t = sketch_target(len(records), s, windows, fill)
    ds = ctx.protein_sketches(batch, gene_array(records), ProteinSketches(k, s, unit, seed=seed, classes=classes, **options), tables=tables, out=t.out)
    assert ds.sketches is t.out[0] and ds.counts is t.out[1] and ds.windows is t.out[2]
    assert all(m.ptr % 8 == 0 for m in t.mem)
    return t.read(), t.expect(*want[:3]), ds, want


def lay_out(parts):
    """[(name or None, letters, strand, partial_begin, partial_end)] -> (one contig's text, [(name, begin, end, strand, pb, pe)]): the
    parts one after the other, a reverse-strand part written as its reverse complement."""
    text, recs = "", []
    for name, letters, strand, pb, pe in parts:
        if name is not None:
            recs.append((name, len(text) + 1, len(text) + len(letters), strand, pb, pe))
        text += letters if strand == 1 else tables_ref.revcomp(letters.encode()).decode()
    return text, recs


# ---- 1. window-count and sketch-size edges -----------------------------------------------------------------------------------------------
WINDOW_COUNTS = (0, 1, 2, 3, 30, 31, 32, 33, 34, 62, 63, 64, 65, 66, 127, 128, 129, 130)


@functools.lru_cache(maxsize=None)
def edges(unit, k):
    """One contig of records whose strings are random and have w windows of k letters for every w of WINDOW_COUNTS (w = 0: k - 1
    letters, no window) -- units are residues (codons flagged partial at both ends: n codons give n residues, none of them M or a
    stop) or bases --, on alternating strands; then the empty string (protein) or a single base (gene), a run of one codon, a unit
    of 10 residues (30 bases) 20 times over, and one record of 4 101 residues (12 303 bases)."""
    u = 3 if unit == "protein" else 1
    parts = []

    def put(name, letters, strand):
        parts.append((name, letters, strand, 1, 1))
        parts.append((None, "CC", 1, 0, 0))

    for i, w in enumerate(WINDOW_COUNTS):
        n = w + k - 1
        if n == 0:
            continue                                             # (k = 1, w = 0: the empty string, below)
        put("w%d" % w, tables_ref.quiet_codons(n, 9000 + 50 * k + i)[:u * n], 1 if i % 2 else -1)
    put("empty", "G", 1)                                          # one base holds no codon; under the gene unit it is one letter
    put("run", "GCC" * 50 if unit == "protein" else "C" * 70, -1)
    put("repeat", tables_ref.quiet_codons(10, 77) * 20, 1)
    put("long", tables_ref.quiet_codons(4101, 78), -1)
    text, recs = lay_out(parts)
    return Case([text.encode("ascii")], [False], [11], [(0,) + r[1:] for r in recs], **{r[0]: [g] for g, r in enumerate(recs)})


@pytest.mark.parametrize("unit,k", [(unit, k) for unit in ("protein", "gene") for k in K_OF[unit]])
def test_window_counts_and_sketch_sizes(ctx, unit, k):
    case = edges(unit, k)
    batch = upload(ctx, case)
    strings = [groups_ref.string_of(case.seqs, case.circular, r, unit, case.tables) for r in case.records]
    distinct = [len(ref.sketch(x, k, 1 << 30, unit, 0, ref.default_classes())[0]) for x in strings]
    valid = [ref.sketch(x, k, 1, unit, 0, ref.default_classes())[1] for x in strings]
    # the inputs are what they are meant to be (by the reference alone)
    for w in WINDOW_COUNTS:
        if w + k - 1 > 0:
            assert valid[case.named["w%d" % w][0]] == w
    assert len(strings[case.named["empty"][0]]) == (0 if unit == "protein" else 1)
    assert len(strings[case.named["long"][0]]) == (4101 if unit == "protein" else 12303)
    if unit == "protein":
        assert distinct[case.named["run"][0]] == 1 and valid[case.named["run"][0]] == 50 - k + 1
    if k <= 10:
        assert distinct[case.named["repeat"][0]] <= 10 < valid[case.named["repeat"][0]]
    for s in SIZES:
        if k >= 5:
            assert {s - 1, s, s + 1} <= set(distinct), (s, sorted(set(distinct)))          # fewer than s, exactly s, s + 1 distinct hashes
        got, want, ds, r = run(ctx, batch, case, k, s, unit)
        assert same(got, want), (s, [n for n, g, w in zip(("sketch", "count", "windows"), got, want) if not np.array_equal(g, w)])
        assert r[1].tolist() == [min(s, d) for d in distinct] and r[2].tolist() == valid


# ---- 2. strands, the origin, tables, options, letters that are skipped --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def varied():
    """One ORF (ATG, 60 quiet codons, TAA) on both strands, across the origin of a circle, as an edge record, with an ambiguous
    codon, with a run of N, with GTG for ATG, with TGA inside under tables 4 and 11, and with one residue of LVIM exchanged for
    another of them; and 12 other ORFs."""
    code = tables_ref.code(11)
    body = tables_ref.quiet_codons(60, 1)
    codons = [body[3 * i:3 * i + 3] for i in range(60)]
    orf = "ATG" + body + "TAA"
    unknown = orf[:3 * 21] + "NNN" + orf[3 * 22:]
    n_run = orf[:40] + "N" * 7 + orf[47:]
    tga = orf[:3 * 11] + "TGA" + orf[3 * 12:]
    gtg = "GTG" + orf[3:]
    at, twin = next((i, x) for i, c in enumerate(codons) for x in tables_ref._QUIET_CODONS
                    if 10 < i < 50 and code[c] in "LVIM" and code[x] in "LVIM" and code[x] != code[c])
    cousin = "ATG" + "".join(codons[:at] + [twin] + codons[at + 1:]) + "TAA"
    seqs, recs, names = [], [], {}

    def lay(parts):
        text, placed = lay_out(parts)
        for name, b, e, strand, pb, pe in placed:
            names.setdefault(name, []).append(len(recs))
            recs.append((len(seqs), b, e, strand, pb, pe))
        seqs.append(text.encode("ascii"))

    gap = lambda s: (None, tables_ref.quiet_codons(7, 50 + s), 1, 0, 0)          # noqa: E731
    others = [("other", "ATG" + tables_ref.quiet_codons(60, 100 + d) + "TAA", 1 if d % 2 else -1, 0, 0) for d in range(12)]
    lay([gap(0), ("copy", orf, 1, 0, 0), gap(1), ("copy", orf, -1, 0, 0), gap(2), ("unknown", unknown, 1, 0, 0), gap(3), ("unknown", unknown, -1, 0, 0),
         gap(4), ("n_run", n_run, -1, 0, 0), gap(5), ("gtg", gtg, 1, 0, 0), gap(6), ("cousin", cousin, -1, 0, 0), gap(7), ("lower", orf.lower(), 1, 0, 0), gap(8)]
        + [x for d in others for x in (d, gap(9))])
    # the ORF's inside as an edge record: no M, no stop
    names["edge"] = [len(recs), len(recs) + 1]
    c, b, e = recs[names["copy"][0]][:3]
    recs.append((c, b + 3, e - 3, 1, 1, 1))
    c, b, e = recs[names["copy"][1]][:3]
    recs.append((c, b + 3, e - 3, -1, 1, 1))
    # across the origin of a circle: the contig begins with the ORF's last bases and ends with its first 76
    rest = tables_ref.quiet_codons(30, 60)
    seqs.append((orf[76:] + rest + orf[:76]).encode("ascii"))
    L = len(seqs[-1])
    names["origin"] = [len(recs), len(recs) + 1]
    recs.append((1, L - 75, L + len(orf) - 76, 1, 0, 0))
    rc = tables_ref.revcomp(seqs[-1]).decode()                    # ... and the same circle read from the other strand
    seqs.append(rc.encode("ascii"))
    recs.append((2, L - (len(orf) - 76) + 1, L + 76, -1, 0, 0))
    lay([gap(11), ("tga4", tga, 1, 0, 0), gap(12), ("copy4", orf, -1, 0, 0), gap(13)])         # read under table 4
    lay([gap(14), ("tga11", tga, 1, 0, 0), gap(15)])                                         # the same letters under table 11
    return Case(seqs, [False, True, True, False, False], [11, 11, 11, 4, 11], recs, **names)


def rows_by_name(case, got, s):
    sk = got[0][1:1 + len(case.records) * s].reshape(-1, s)
    return {name: [sk[g].tolist() for g in idx] for name, idx in case.named.items()}, got[1][1:1 + len(case.records)], got[2][1:1 + len(case.records)]


@pytest.mark.parametrize("unit", ["protein", "gene"])
def test_strands_origin_tables_and_skipped_letters(ctx, unit):
    case = varied()
    batch = upload(ctx, case)
    k, s = (5, 32) if unit == "protein" else (11, 32)
    got, want, ds, r = run(ctx, batch, case, k, s, unit)
    assert same(got, want)
    by, count, windows = rows_by_name(case, got, s)
    one = by["copy"][0]
    # what the reference says is what the issue says
    assert by["copy"][1] == one and by["origin"] == [one, one] and by["lower"] == [one]
    n = len(r[3 + 1][case.named["copy"][0]])
    assert n == (61 if unit == "protein" else 186) and windows[case.named["copy"][0]] == n - k + 1
    w_unknown, w_nrun = windows[case.named["unknown"][0]], windows[case.named["n_run"][0]]
    if unit == "protein":
        assert by["copy4"] == [one] and by["tga4"] != by["tga11"] and by["edge"][0] == by["edge"][1] != one
        assert w_unknown == n - k + 1 - k and windows[case.named["unknown"][1]] == w_unknown      # the k windows over X are skipped
        assert b"X" in r[4][case.named["unknown"][0]] and b"W" in r[4][case.named["tga4"][0]] and r[4][case.named["edge"][0]][:1] != b"M"
    else:
        assert by["tga4"] == by["tga11"] and w_unknown == n - k + 1 - (k + 2) and w_nrun == n - k + 1 - (k + 6)     # NNN; seven N
    # the translation's options and the seed, against the reference
    seen = {}
    for name, kw in (("include_stop", dict(include_stop=True)), ("lenient", dict(strict=False)), ("Z", dict(unknown_residue="Z")),
                     ("table 4", dict(tables=np.array([11, 11, 11, 4, 4], np.int32))), ("seed 7", dict(seed=7)), ("seed max", dict(seed=2 ** 32 - 1)),
                     ("k 3, s 64", None), ("reduced", dict(classes=REDUCED))):
        if kw is None:
            g2, w2, _, r2 = run(ctx, batch, case, 3, 64, unit)
        else:
            g2, w2, _, r2 = run(ctx, batch, case, k, s, unit, **kw)
        assert same(g2, w2), name
        seen[name] = g2
    if unit == "protein":
        assert not same(seen["include_stop"], got) and not same(seen["table 4"], got)
        stop_rows, _, stop_windows = rows_by_name(case, seen["include_stop"], s)
        assert stop_windows[case.named["copy"][0]] == windows[case.named["copy"][0]] + 1        # the * is a letter
        assert stop_windows[case.named["edge"][0]] == windows[case.named["edge"][0]]            # an edge record has no stop to include
        red, _, _ = rows_by_name(case, seen["reduced"], s)
        assert red["cousin"] == red["copy"][:1] and by["cousin"] != by["copy"][:1]              # two different proteins, one sketch
    else:
        assert same(seen["include_stop"], got) and same(seen["table 4"], got) and same(seen["reduced"], got)      # not read for bases
    assert not same(seen["seed 7"], got) and not same(seen["seed max"], got) and not same(seen["seed 7"], seen["seed max"])


def test_subsets_orders_null_windows_and_repeated_calls(ctx):
    from pyrodigal_amd import ProteinGroups
    case = varied()
    batch = upload(ctx, case)
    n = len(case.records)
    full, want, ds, r = run(ctx, batch, case, 5, 32)
    assert same(full, want)
    rows = full[0][1:1 + 32 * n].reshape(n, 32)
    orders = {"reversed": list(range(n))[::-1], "shuffled": np.random.default_rng(11).permutation(n).tolist(), "subset": list(range(1, n, 3)),
              "twice": list(range(n)) + list(range(n)), "one": [n // 2], "none": []}
    for name, order in orders.items():
        for unit, k in (("protein", 5), ("gene", 11)):
            got, want, ds, r = run(ctx, batch, case, k, 32, unit, records=[case.records[g] for g in order])
            assert same(got, want), (name, unit)
        assert ds.gene_begin is None or name in ("subset", "one", "none")
    got, want, ds, r = run(ctx, batch, case, 5, 32, records=[case.records[g] for g in orders["shuffled"]])
    assert np.array_equal(got[0][1:1 + 32 * n].reshape(n, 32), rows[orders["shuffled"]])     # a row is its record's, wherever it stands
    # d_windows = NULL: the third allocation stays as it was
    got, want, ds, r = run(ctx, batch, case, 5, 32, windows=False)
    assert same(got, want) and ds.windows is None and np.all(got[2] == np.int64(int.from_bytes(bytes([CANARY] * 8), "little", signed=True)))
    assert same(got[:2], full[:2])
    # the same call again, and after an unrelated call, over memory that held something else: the same bytes
    again, _, _, _ = run(ctx, batch, case, 5, 32)
    assert same(again, full)
    t = Target([(n,)])
    ctx.protein_groups(batch, gene_array(case.records), ProteinGroups("gene"), tables=case.tables, out=(t.out[0], None, None, None))
    run(ctx, batch, case, 11, 64, "gene", seed=3)
    for fill in (0x00, 0xFF):
        other, want, _, _ = run(ctx, batch, case, 5, 32, fill=fill)
        assert same(other, want)
        assert np.array_equal(other[0][1:1 + 32 * n], full[0][1:1 + 32 * n]) and np.array_equal(other[1][1:1 + n], full[1][1:1 + n])


# ---- 3. pairs ----------------------------------------------------------------------------------------------------------------------------
def device_rows(rows, s):
    """(sketch [G, s], count [G]) of lists of real entries, on the device, as pga_sketch_proteins leaves them"""
    G = len(rows)
    sk, cnt = np.full((max(G, 1), s), ref.INT64_MAX, np.int64), np.zeros(max(G, 1), np.int64)
    for g, row in enumerate(rows):
        assert list(row) == sorted(set(row)) and len(row) <= s
        sk[g, :len(row)] = row
        cnt[g] = len(row)
    return keep(hip_mem.DeviceArray.from_numpy(sk)), keep(hip_mem.DeviceArray.from_numpy(cnt))


def compare(ctx, d_sk, d_cnt, G, s, pairs, fill=CANARY):
    """pga_sketch_pairs into a Target: (what the two allocations hold, the Target)"""
    pairs = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2))
    P = len(pairs)
    d_pairs = keep(hip_mem.DeviceArray.from_numpy(pairs))
    t = Target([(P,), (P,)], fill=fill)
    rc = ctx.L.pga_sketch_pairs(ctx.h, ctypes.c_void_p(d_sk.ptr), ctypes.c_void_p(d_cnt.ptr), G, s, ctypes.c_void_p(d_pairs.ptr), P,
                                ctypes.c_void_p(t.mem[0].ptr + 8), ctypes.c_void_p(t.mem[1].ptr + 8), None)
    assert rc == 0, ctx.L.pga_last_error(ctx.h).decode()
    return t.read(), t


@pytest.mark.parametrize("s", [1, 5, 32, 64])
def test_pairs_by_hand(ctx, s):
    big = 1 << 62
    rows = {
        "full": list(range(10, 10 + s)), "same": list(range(10, 10 + s)), "apart": list(range(1000, 1000 + s)), "empty": [],
        "short": list(range(10, 10 + (s + 1) // 2)), "one": [10], "tail": list(range(1, s)) + [big], "tail2": list(range(2000, 1999 + s)) + [big],
        "low": [3], "high": [ref.INT64_MAX - 1], "even": list(range(0, 2 * s, 2)), "third": list(range(0, 3 * s, 3)),
    }
    names = list(rows)
    d_sk, d_cnt = device_rows([rows[n] for n in names], s)
    G = len(names)
    pairs = [(names.index(a), names.index(b)) for a in names for b in names]
    want = ref.pairs_ref([rows[n] for n in names], pairs, s)
    got, t = compare(ctx, d_sk, d_cnt, G, s, pairs)
    assert same(got, t.expect(*want))
    expect = dict(zip(((names[a], names[b]) for a, b in pairs), zip(want[0].tolist(), want[1].tolist())))
    # what the reference says is what the issue says
    assert expect["full", "same"] == (s, s) == expect["full", "full"] and expect["full", "apart"] == (0, s) and expect["empty", "empty"] == (0, 0)
    assert expect["empty", "full"] == (0, s) and expect["one", "low"] == (0, min(s, 2)) and expect["short", "one"] == (1, (s + 1) // 2)
    if s > 1:
        # both rows end in the same hash, and it lies beyond the s smallest of their union: not counted
        assert expect["tail", "tail2"] == (0, s) and expect["tail", "tail"] == (s, s)
        assert expect["short", "full"] == ((s + 1) // 2, s)                                  # a union of exactly s
        assert 0 < expect["even", "third"][0] < s and expect["even", "third"][1] == s       # a union larger than s
    assert expect["low", "high"] == (0, min(s, 2))                                             # a union smaller than s


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65])
def test_pairs_of_random_rows_and_indices_out_of_range(ctx, P):
    s, G = 32, 40
    rng = np.random.default_rng(100 + P)
    rows = [sorted(set(rng.integers(0, 150, size=int(rng.integers(0, 60))).tolist()))[:s] for _ in range(G)]
    d_sk, d_cnt = device_rows(rows, s)
    pairs = rng.integers(0, G, size=(P, 2)).tolist()
    for p, bad in zip(range(2, P, 7), [(-1, 0), (0, -1), (G, 0), (3, G), (1 << 40, 2), (2, -(1 << 62)), (G + 5, -3)] * 3):
        pairs[p] = list(bad)
    want = ref.pairs_ref(rows, pairs, s)
    got, t = compare(ctx, d_sk, d_cnt, G, s, pairs)
    assert same(got, t.expect(*want))                             # -1 where an index is out of range, the neighbours as they must be
    if P >= 63:
        assert (want[0] == -1).sum() >= 7 and (want[0] > 0).sum() >= 10 and len({tuple(x) for x in zip(*want)}) > 10
    # no record at all: every index is out of range, and no row is read
    got, t = compare(ctx, hip_mem_null(), hip_mem_null(), 0, s, pairs)
    assert same(got, t.expect(np.full(P, -1), np.full(P, -1)))


class _Null:
    ptr = 0


def hip_mem_null():
    return _Null()


def test_compare_on_sketches_of_the_device(ctx):
    """DeviceSketches.compare over rows the sketch kernel wrote, rows with count < s among them."""
    case = edges("protein", 5)
    batch = upload(ctx, case)
    got, want, ds, r = run(ctx, batch, case, 5, 32)
    assert same(got, want)
    G = len(case.records)
    assert (r[1] < 32).any() and (r[1] == 32).any() and (r[1] == 0).any()
    pairs = [(a, b) for a in range(G) for b in range(a, G)]
    d_pairs = keep(hip_mem.DeviceArray.from_numpy(np.array(pairs, np.int64)))
    t = Target([(len(pairs),), (len(pairs),)])
    out = ds.compare(View(d_pairs.ptr, (len(pairs), 2)), out=t.out)
    assert out[0] is t.out[0] and out[1] is t.out[1]
    wanted = ref.pairs_ref(r[3], pairs, 32)
    assert same(t.read(), t.expect(*wanted))
    assert ds.spec.shared(r[3][3], r[3][3]) == (int(wanted[0][pairs.index((3, 3))]), int(wanted[1][pairs.index((3, 3))]))
    with pytest.raises(ValueError, match="pairs needs shape"):
        ds.compare(View(d_pairs.ptr, (len(pairs) * 2,)), out=t.out)
    with pytest.raises(ValueError, match="shared needs shape"):
        ds.compare(View(d_pairs.ptr, (len(pairs), 2)), out=(View(t.mem[0].ptr + 8, (len(pairs) - 1,)), t.out[1]))


# ---- 4. meaning ----------------------------------------------------------------------------------------------------------------------------
def test_a_near_copy_resembles_and_a_stranger_does_not(ctx):
    """A 300-residue protein, a copy with 3 substitutions and an unrelated protein: the reference alone fixes the expected integers."""
    code = tables_ref.code(11)
    def codons(seed):
        text = tables_ref.quiet_codons(299, seed)
        return [text[3 * i:3 * i + 3] for i in range(299)]

    first, stranger = codons(501), codons(502)
    copy = list(first)
    for at in (50, 150, 250):
        copy[at] = next(x for x in tables_ref._QUIET_CODONS if code[x] != code[first[at]])
    text, recs = lay_out([x for name, cs in (("first", first), ("copy", copy), ("stranger", stranger))
                          for x in ((name, "ATG" + "".join(cs) + "TAA", 1, 0, 0), (None, "CCCC", 1, 0, 0))])
    case = Case([text.encode("ascii")], [False], [11], [(0,) + r[1:] for r in recs])
    batch = upload(ctx, case)
    got, want, ds, r = run(ctx, batch, case, 5, 32)
    assert same(got, want)
    strings = r[4]
    assert [len(x) for x in strings] == [300] * 3 and sum(a != b for a, b in zip(strings[0], strings[1])) == 3
    pairs = [(0, 1), (0, 2), (1, 2), (0, 0)]
    shared, union = ref.pairs_ref(r[3], pairs, 32)
    d_pairs = keep(hip_mem.DeviceArray.from_numpy(np.array(pairs, np.int64)))
    t = Target([(4,), (4,)])
    ds.compare(View(d_pairs.ptr, (4, 2)), out=t.out)
    assert same(t.read(), t.expect(shared, union))                # exactly the reference's integers
    assert union.tolist() == [32] * 4 and shared[3] == 32
    assert shared[0] / union[0] > shared[1] / union[1] and shared[0] / union[0] > shared[2] / union[2]
    print("near copy: %d / %d, strangers: %d / %d and %d / %d" % (shared[0], union[0], shared[1], union[1], shared[2], union[2]))


# ---- 5. composition ----------------------------------------------------------------------------------------------------------------------
def test_sketch_the_unique_proteins_only(ctx):
    """protein_groups, then protein_sketches over its representatives: the rows of everybody, by group."""
    from pyrodigal_amd import ProteinGroups, ProteinSketches
    case = varied()
    batch = upload(ctx, case)
    genes = gene_array(case.records)
    G = len(genes)
    tg = Target([(G,), (G,), (G,), (G, 2)])
    dg = ctx.protein_groups(batch, genes, ProteinGroups(), tables=case.tables, out=tg.out)
    group, reps = tg.read()[0][1:1 + G], tg.read()[1][1:1 + dg.n_groups]
    assert 1 < dg.n_groups < G
    everybody, want, _, r = run(ctx, batch, case, 5, 32)
    assert same(everybody, want)
    U = dg.n_groups
    unique = [case.records[g] for g in reps]
    got, want, ds, ru = run(ctx, batch, case, 5, 32, records=unique)
    assert same(got, want) and ds.spec == ProteinSketches(5, 32)
    rows_u, rows_all = got[0][1:1 + 32 * U].reshape(U, 32), everybody[0][1:1 + 32 * G].reshape(G, 32)
    assert np.array_equal(rows_u[group], rows_all)                # row for row
    assert np.array_equal(got[1][1:1 + U][group], everybody[1][1:1 + G]) and np.array_equal(got[2][1:1 + U][group], everybody[2][1:1 + G])


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_host_and_leave_the_context_usable(ctx):
    from pyrodigal_amd import ProteinSketches, _cabi
    case = varied()
    batch = upload(ctx, case)
    genes = gene_array(case.records)
    G, s = len(genes), 32
    t = sketch_target(G, s)
    ptrs = [m.ptr + 8 for m in t.mem]
    host = np.zeros(G * s + 8, np.int64)

    def raw(sketch=ptrs[0], count=ptrs[1], windows=ptrs[2], recs=genes, tables=case.tables, spec=ProteinSketches(5, s), **change):
        o = spec.opts()
        for name, v in change.items():
            setattr(o, name, v)
        tables = np.ascontiguousarray(tables, np.int32)
        rc = ctx.L.pga_sketch_proteins(ctx.h, batch.h, len(recs), ctypes.c_void_p(recs.ctypes.data), ctypes.c_void_p(tables.ctypes.data), ctypes.byref(o),
                                       ctypes.c_void_p(sketch), ctypes.c_void_p(count), ctypes.c_void_p(windows), None)
        return rc, ctx.L.pga_last_error(ctx.h).decode()

    def changed(g, **fields):
        out = genes.copy()
        for name, v in fields.items():
            out[name][g] = v
        return out

    bad_table = case.tables.copy()
    bad_table[3] = 7
    gene_unit = ProteinSketches(11, s, "gene")
    for what, kw, word in (("a host pointer for the sketches", dict(sketch=host.ctypes.data), "d_sketch is not device memory"),
                           ("a host pointer for the counts", dict(count=host.ctypes.data), "d_count is not device memory"),
                           ("a host pointer for the windows", dict(windows=host.ctypes.data), "d_windows is not device memory"),
                           ("a misaligned pointer", dict(count=ptrs[1] + 4), "d_count is not aligned"),
                           ("misaligned windows", dict(windows=ptrs[2] + 2), "d_windows is not aligned"),
                           ("no d_sketch", dict(sketch=None), "d_sketch is NULL"),
                           ("no d_count", dict(count=None), "d_count is NULL"),
                           ("a record outside its contig", dict(recs=changed(5, end=len(case.seqs[0]) + 1)), "gene 5 lies outside"),
                           ("a record of another contig", dict(recs=changed(4, contig=5)), "gene 4 lies outside"),
                           ("a record across the origin of a linear contig", dict(recs=changed(0, begin=len(case.seqs[0]) - 5, end=len(case.seqs[0]) + 6)), "gene 0"),
                           ("a unit that is none", dict(unit=2), "unit must be"),
                           ("k = 0", dict(k=0), "k = 0"), ("k = 9 for proteins", dict(k=9), "k = 9"), ("k = 33 for bases", dict(spec=gene_unit, k=33), "k = 33"),
                           ("size = 0", dict(size=0), "size = 0"), ("size = 65", dict(size=65), "size = 65"),
                           ("an unknown residue that is no character", dict(unknown_residue=200), "unknown_residue"),
                           ("a table that is none", dict(tables=bad_table), "contig 3: 7 is not a valid translation table")):
        rc, msg = raw(**kw)
        assert rc == _cabi.PGA_EINVAL and word in msg and msg.startswith("pga_sketch_proteins: "), (what, rc, msg)
    # pga_sketch_pairs
    d_pairs = keep(hip_mem.DeviceArray.from_numpy(np.array([[0, 1], [2, 3]], np.int64)))
    tp = Target([(2,), (2,)])

    def raw_pairs(sketch=ptrs[0], count=ptrs[1], n=G, size=s, pairs=d_pairs.ptr, P=2, shared=tp.mem[0].ptr + 8, union=tp.mem[1].ptr + 8):
        rc = ctx.L.pga_sketch_pairs(ctx.h, ctypes.c_void_p(sketch), ctypes.c_void_p(count), n, size, ctypes.c_void_p(pairs), P, ctypes.c_void_p(shared),
                                    ctypes.c_void_p(union), None)
        return rc, ctx.L.pga_last_error(ctx.h).decode()

    for what, kw, word in (("size = 0", dict(size=0), "size = 0"), ("size = 65", dict(size=65), "size = 65"), ("no pairs", dict(pairs=None), "d_pairs is NULL"),
                           ("no sketches", dict(sketch=None), "d_sketch is NULL"), ("no counts", dict(count=None), "d_count is NULL"),
                           ("no d_shared", dict(shared=None), "d_shared is NULL"), ("no d_union", dict(union=None), "d_union is NULL"),
                           ("host sketches", dict(sketch=host.ctypes.data), "d_sketch is not device memory"),
                           ("host pairs", dict(pairs=host.ctypes.data), "d_pairs is not device memory"),
                           ("host d_shared", dict(shared=host.ctypes.data), "d_shared is not device memory"),
                           ("misaligned d_union", dict(union=tp.mem[1].ptr + 12), "d_union is not aligned"),
                           ("a negative count", dict(P=-1), "bad arguments"), ("negative records", dict(n=-1), "bad arguments")):
        rc, msg = raw_pairs(**kw)
        assert rc == _cabi.PGA_EINVAL and word in msg and msg.startswith("pga_sketch_pairs: "), (what, rc, msg)
    # the Python layer
    with pytest.raises(ValueError, match="not device memory"):
        ctx.protein_sketches(batch, genes, ProteinSketches(5, s), tables=case.tables, out=(View(host.ctypes.data, (G, s)),) + t.out[1:])
    with pytest.raises(ValueError, match="sketches needs shape"):
        ctx.protein_sketches(batch, genes, ProteinSketches(5, s), tables=case.tables, out=(View(ptrs[0], (G, s - 1)),) + t.out[1:])
    with pytest.raises(ValueError, match="counts needs shape"):
        ctx.protein_sketches(batch, genes, ProteinSketches(5, s), tables=case.tables, out=(t.out[0], View(ptrs[1], (G - 1,)), None))
    with pytest.raises(TypeError, match="int64"):
        ctx.protein_sketches(batch, genes, ProteinSketches(5, s), tables=case.tables, out=(View(ptrs[0], (G, s), "<i4"),) + t.out[1:])
    with pytest.raises(TypeError, match="counts is required"):
        ctx.protein_sketches(batch, genes, ProteinSketches(5, s), tables=case.tables, out=(t.out[0], None, None))
    with pytest.raises(ValueError, match="3 objects|out must be"):
        ctx.protein_sketches(batch, genes, ProteinSketches(5, s), tables=case.tables, out=t.out[:2])
    with pytest.raises(ValueError, match="tables="):
        ctx.protein_sketches(batch, genes, ProteinSketches(5, s))
    with pytest.raises(TypeError, match="ProteinSketches"):
        ctx.protein_sketches(batch, genes, "protein", tables=case.tables)
    assert np.all(host == 0)
    assert t.untouched() and tp.untouched()                       # nothing was written anywhere
    rc, msg = raw()                                               # the context runs a good call afterwards
    assert rc == 0, msg
    want = ref.protein_sketches_ref(case.seqs, case.circular, case.records, 5, s, "protein", 0, None, case.tables)
    assert same(t.read(), t.expect(*want[:3]))
    rc, msg = raw_pairs()
    assert rc == 0, msg
    assert same(tp.read(), tp.expect(*ref.pairs_ref(want[3], [(0, 1), (2, 3)], s)))
    rc, msg = raw(spec=gene_unit, tables=bad_table)               # (the tables are not read for bases)
    assert rc == 0, msg
    rc, msg = raw_pairs(P=0, pairs=None, shared=None, union=None)  # no pair: nothing is needed
    assert rc == 0, msg
    assert ctx.protein_sketch_passes() == -1                      # (counted only by a build that was asked to)


# ---- 7. through the finder ----------------------------------------------------------------------------------------------------------------
FINDER_SCRIPT = r'''
import sys
import torch                                   # first: the library then binds to the HIP runtime of torch's wheel
if not torch.cuda.is_available():
    print("torch sees no GPU")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
import numpy as np
from pyrodigal_amd import DeviceSketches, DeviceSequences, ProteinGroups, ProteinSketches, benchdata, lib
from tests import protein_sketches_ref as ref
from tests.util import read_fasta

bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])
s = read_fasta("GCF_001457455.1_NCTC11397_genomic_100kb.fna.gz")[0][1].encode("ascii")
rc = s.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]
seqs = [s, rc, s[1000:50000]]
REDUCED = ("LVIM", "C", "A", "G", "ST", "P", "FYW", "EDNQ", "KR", "H")


def check(given, spec, classes=None, given_out=False, **options):
    finder = lib.GeneFinder(meta=True, metagenomic_bins=bins)
    want_genes = finder.find_genes_batch(given, **options)
    G = sum(len(c) for c in want_genes)
    out = None
    if given_out:
        out = (torch.full((G, spec.size), -5, dtype=torch.int64, device="cuda"), torch.full((G,), -5, dtype=torch.int64, device="cuda"),
               torch.full((G,), -5, dtype=torch.int64, device="cuda"))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        genes, ds = finder.find_sketches_batch(given, spec, out=out, **options)
        most = ds.counts.max() if G else None                      # a consumer on the same stream
    assert isinstance(ds, DeviceSketches) and ds.spec == spec
    if given_out:
        assert ds.sketches is out[0] and ds.counts is out[1] and ds.windows is out[2]
    key = lambda x: [[(g.begin, g.end, g.strand) for g in c] for c in x]
    assert key(genes) == key(want_genes)
    flat = [g for c in genes for g in c]
    assert len(flat) == G
    strings = [(g.translate(include_stop=spec.include_stop, strict=spec.strict, unknown_residue=spec.unknown_residue) if spec.of == "protein" else g.sequence()).encode("ascii")
               for g in flat]
    table = ref.default_classes(spec.unknown_residue) if classes is None else ref.classes_of(classes)
    sketch, count, windows, rows = ref.sketches_ref(strings, spec.k, spec.size, spec.of, spec.seed, table)
    for t in (ds.sketches, ds.counts, ds.windows):
        assert t.is_cuda and t.dtype == torch.int64 and t.device.index == 0
    assert tuple(ds.sketches.shape) == (G, spec.size) and tuple(ds.counts.shape) == (G,) and tuple(ds.windows.shape) == (G,)
    assert np.array_equal(ds.sketches.cpu().numpy(), sketch) and np.array_equal(ds.counts.cpu().numpy(), count)
    assert np.array_equal(ds.windows.cpu().numpy(), windows)
    assert int(most) == int(count.max())
    assert ds.gene_begin.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in genes])]).tolist()
    assert spec.sketch_of(strings[0]) == (rows[0], int(windows[0]))
    # pairs of neighbours and of a gene with its copy on the other strand, compared on the device
    pairs = torch.tensor([[g, (g + 1) % G] for g in range(G)] + [[0, 0], [G, 0], [-1, 2]], dtype=torch.int64, device="cuda")
    shared, union = ds.compare(pairs)
    want = ref.pairs_ref(rows, pairs.cpu().tolist(), spec.size)
    assert shared.cpu().tolist() == want[0].tolist() and union.cpu().tolist() == want[1].tolist()
    return G, ds, genes


G, ds, genes = check(seqs, ProteinSketches())
assert G > 150
assert check(seqs, ProteinSketches(11, 64, "gene", seed=7), given_out=True)[0] == G
assert check(seqs, ProteinSketches(3, 16, include_stop=True, strict=False, classes=REDUCED), classes=REDUCED)[0] == G
rows = np.full((len(seqs), max(map(len, seqs))), ord("N"), np.uint8)
for i, q in enumerate(seqs):
    rows[i, :len(q)] = np.frombuffer(q, np.uint8)
given = DeviceSequences(torch.from_numpy(rows).cuda(), [len(q) for q in seqs])
G2, ds2, _ = check(given, ProteinSketches())
assert G2 == G and torch.equal(ds2.sketches, ds.sketches)
assert check(seqs, ProteinSketches(), circular=True)[0] > 0
# with the groups of the same request: the sketches of the representatives are everybody's, by group
finder = lib.GeneFinder(meta=True, metagenomic_bins=bins)
_, dg = finder.find_groups_batch(seqs, ProteinGroups())
assert dg.n_groups < G
unique = ds.sketches[dg.representatives]
assert tuple(unique.shape) == (dg.n_groups, 32) and torch.equal(unique[dg.group], ds.sketches)
print("find_sketches_batch ok: %d genes, %d unique proteins" % (G, dg.n_groups))
'''


def test_find_sketches_batch_in_a_fresh_process(tmp_path):
    """torch is imported by the child alone (this process holds the library's HIP runtime and gets no second one); `out=` omitted
    allocates the tensors under torch's current stream.  The child says so when torch sees no GPU, and the test is skipped."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "torch_protein_sketches.py"
    script.write_text(FINDER_SCRIPT)
    done = subprocess.run([sys.executable, str(script), root], timeout=300, capture_output=True, text=True)
    assert done.returncode == 0, "child ended with %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    if "torch sees no GPU" in done.stdout:
        pytest.skip("torch sees no GPU")
    assert "find_sketches_batch ok" in done.stdout
