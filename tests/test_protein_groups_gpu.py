"""Gene records with the same protein, or the same bases, grouped on the device (pga_group_proteins, ProteinGroups,
Context.protein_groups, GeneFinder.find_groups_batch).

Every expected value comes from the plain-Python restatement of the rule (tests/protein_groups_ref.py): the strings by
tests/tables_ref.translate and tests/gene_windows_ref, the groups by a dict, the digest by Python integers -- never from the code under
test.  Device memory comes from tests/hip_mem.py (no torch), but for the finder test, which runs in a child process."""
import ctypes
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hip_mem, tables_ref
from tests import protein_groups_ref as ref

pytestmark = pytest.mark.gpu

CANARY = 0xA5
KNOB = "PGA_PROTEIN_GROUPS_KEY_BITS"


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi, benchdata
    c = _cabi.Context(0)
    c.set_models([b for _, b in benchdata.load_model_set()])
    yield c
    c.close()


@pytest.fixture(autouse=True)
def no_knob(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)


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
    """Four allocations full of a fill byte, and in each an int64 tensor that begins 8 bytes into it, with `slack` elements behind:
    group [G], representatives [capacity], sizes [capacity], digests [G, 2].  `which`: the optional three that are given at all.
    `expect()` is what the four whole allocations must hold after a call."""

    NAMES = ("group", "representatives", "sizes", "digests")

    def __init__(self, G, capacity=None, which=(True, True, True), slack=5, fill=CANARY):
        self.G, self.capacity = G, G if capacity is None else capacity
        self.elems = (G, self.capacity, self.capacity, 2 * G)
        self.given = (True,) + tuple(which)
        self.before = [np.full(8 * (1 + n + slack), fill, np.uint8) for n in self.elems]
        self.mem = [keep(hip_mem.DeviceArray.from_numpy(b)) for b in self.before]
        shapes = ((G,), (self.capacity,), (self.capacity,), (G, 2))
        self.out = tuple(View(m.ptr + 8, s) if on else None for m, s, on in zip(self.mem, shapes, self.given))

    def read(self):
        return [m.to_numpy(np.int64) for m in self.mem]

    def expect(self, group, reps, sizes, digests):
        out = [b.view(np.int64).copy() for b in self.before]
        for e, want, on in zip(out, (group, reps, sizes, np.asarray(digests).reshape(-1)), self.given):
            if on:
                e[1:1 + len(want)] = want
        return out


def gene_array(recs):
    from pyrodigal_amd import _cabi
    genes = np.zeros(len(recs), _cabi.GENE_DTYPE)
    if len(recs):
        for name, col in zip(("contig", "begin", "end", "strand", "partial_begin", "partial_end"), zip(*recs)):
            genes[name] = col
    return genes


def run(ctx, batch, case, records=None, unit="protein", which=(True, True, True), fill=CANARY, **options):
    """One call into a Target: (what the allocations hold, what they must hold, the DeviceGroups, the reference's tuple)."""
    from pyrodigal_amd import ProteinGroups
    records = case.records if records is None else records
    tables = options.pop("tables", case.tables)
    want = ref.protein_groups_ref(case.seqs, case.circular, records, unit, tables, **options)
    t = Target(len(records), which=which, fill=fill)
    dg = ctx.protein_groups(batch, gene_array(records), ProteinGroups(unit, **options), tables=tables, out=t.out)
    assert dg.group is t.out[0] and dg.n_groups == len(want[1]) and dg.digests is t.out[3]
    assert all(m.ptr % 8 == 0 for m in t.mem)
    return t.read(), t.expect(*want[:4]), dg, want


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def upload(ctx, case):
    batch = keep(ctx.upload(case.seqs))
    if any(case.circular):
        batch.set_circular(case.circular)
    return batch


class Case:
    def __init__(self, seqs, circular, tables, records, **named):
        self.seqs, self.circular, self.tables, self.records = seqs, circular, np.array(tables, np.int32), records
        self.named = named                                     # record indices by name


# ---- 1. planted copies -----------------------------------------------------------------------------------------------------------------
def spacer(n, seed):
    return tables_ref.quiet_codons(n, seed)                     # (no table reads a stop or, in frame, anything special in it)


@functools.lru_cache(maxsize=None)
def planted():
    """One ORF (ATG, 40 codons that no table ends a gene at, TAA) in every disguise the issue names, and 40 other ORFs of the same
    shape, so that more than 32 distinct strings meet under a 5-bit key."""
    code = tables_ref.code(11)
    body = tables_ref.quiet_codons(40, 1)
    orf = "ATG" + body + "TAA"
    codons = [body[3 * i:3 * i + 3] for i in range(40)]
    k, twin = next((i, x) for i, c in enumerate(codons) for x in tables_ref._QUIET_CODONS if x != c and code[x] == code[c])
    synonym = "ATG" + "".join(codons[:k] + [twin] + codons[k + 1:]) + "TAA"
    unknown = orf[:20] + "N" + orf[21:]
    tga = orf[:3 * 11] + "TGA" + orf[3 * 12:]
    gtg = "GTG" + orf[3:]
    seqs, recs, names = [], [], {}

    def lay(contig_parts):
        """[(name or None, letters, strand, partial_begin, partial_end)] -> one contig, and the records of the named parts"""
        c, text = len(seqs), ""
        for name, letters, strand, pb, pe in contig_parts:
            if name is not None:
                names.setdefault(name, []).append(len(recs))
                recs.append((c, len(text) + 1, len(text) + len(letters), strand, pb, pe))
            text += letters if strand == 1 else tables_ref.revcomp(letters.encode()).decode()
        seqs.append(text.encode("ascii"))

    gap = lambda s: (None, spacer(7, 50 + s), 1, 0, 0)          # noqa: E731
    decoys = [("decoy", "ATG" + tables_ref.quiet_codons(40, 100 + d) + "TAA", 1 if d % 2 else -1, 0, 0) for d in range(40)]
    lay([gap(0), ("copy", orf, 1, 0, 0), gap(1), ("copy", orf, 1, 0, 0), gap(2), ("synonym", synonym, 1, 0, 0), gap(3),
         ("lower", orf.lower(), 1, 0, 0), gap(4), ("unknown", unknown, 1, 0, 0), gap(5), ("gtg", gtg, 1, 0, 0), gap(6)]
        + [x for d in decoys for x in (d, gap(7))])
    lay([gap(8), ("copy", orf, -1, 0, 0), gap(9), ("gtg", gtg, -1, 0, 0), gap(10)])
    # across the origin of a circle: the contig begins with the ORF's last 50 bases and ends with its first 76
    rest = spacer(30, 60)
    seqs.append((orf[76:] + rest + orf[:76]).encode("ascii"))
    L = len(seqs[-1])
    names.setdefault("copy", []).append(len(recs))
    recs.append((2, L - 75, L + len(orf) - 76, 1, 0, 0))
    lay([gap(11), ("tga", tga, 1, 0, 0), gap(12), ("copy4", orf, -1, 0, 0), gap(13)])         # read under table 4
    lay([gap(14), ("tga11", tga, 1, 0, 0), gap(15)])                                        # the same letters under table 11
    # the GTG copies once more, flagged partial at their own start: V in place of M from the same bases
    for g in list(names["gtg"]):
        c, b, e, strand, _, _ = recs[g]
        names.setdefault("gtg_edge", []).append(len(recs))
        recs.append((c, b, e, strand, 1 if strand == 1 else 0, 0 if strand == 1 else 1))
    return Case(seqs, [False, False, True, False, False], [11, 11, 11, 4, 11], recs, **names)


def groups_by_name(case, group):
    return {name: sorted({int(group[g]) for g in idx}) for name, idx in case.named.items()}


@pytest.mark.parametrize("unit", ["protein", "gene"])
def test_planted_copies(ctx, unit):
    case = planted()
    got, want, dg, r = run(ctx, upload(ctx, case), case, unit=unit)
    assert same(got, want), [n for n, g, w in zip(Target.NAMES, got, want) if not np.array_equal(g, w)]
    by = groups_by_name(case, r[0])
    # what the reference says is what the issue says
    assert len(by["copy"]) == 1 and by["lower"] == by["copy"] and len(by["decoy"]) == 40
    assert by["unknown"] != by["copy"] and by["tga"] != by["copy"] and by["gtg_edge"] != by["copy"]
    if unit == "protein":
        assert by["tga11"] != by["tga"] and by["synonym"] == by["copy"] and by["gtg"] == by["copy"] and by["copy4"] == by["copy"] and by["gtg_edge"] != by["gtg"]
        assert b"W" in r[4][case.named["tga"][0]] and r[4][case.named["gtg_edge"][0]][:1] == b"V"
    else:
        assert by["synonym"] != by["copy"] and by["gtg"] != by["copy"] and by["gtg_edge"] == by["gtg"] and by["tga11"] == by["tga"]
    assert ctx.protein_groups_stats()["rounds"] == 1


# ---- 2. length edges -----------------------------------------------------------------------------------------------------------------------
EDGE_LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 4100)


@functools.lru_cache(maxsize=None)
def length_edges(unit):
    """For every n: a string of n units twice (once on the reverse strand), one that differs in the last unit only, one in the first
    only, and one of n + 1 units that begins with the string.  Units are residues (codons, flagged partial at both ends: n codons
    give n residues, none of them M or a stop) or bases."""
    u = 3 if unit == "protein" else 1
    other = {"protein": lambda c: "TGG" if c != "TGG" else "AAA", "gene": lambda c: "ACGT"["CGTA".index(c)]}[unit]
    text, recs, sets = "", [], []

    def put(letters, strand=1):
        nonlocal text
        at = len(text)
        text += (letters if strand == 1 else tables_ref.revcomp(letters.encode()).decode()) + "CC"
        if not letters:                                          # no unit at all: one base, which holds no codon
            assert unit == "protein"
            recs.append((0, at + 1, at + 1, strand, 1, 1))
        else:
            recs.append((0, at + 1, at + len(letters), strand, 1, 1))
        return len(recs) - 1

    for n in EDGE_LENGTHS:
        if n == 0 and unit == "gene":
            continue
        s = tables_ref.quiet_codons(n + 1, 7000 + n)[:u * (n + 1)]
        base, longer = s[:u * n], s
        entry = {"n": n, "equal": [put(base), put(base, -1)], "near": [put(longer)]}
        if n > 0:
            entry["near"] += [put(base[:-u] + other(base[-u:])), put(other(base[:u]) + base[u:])]
        sets.append(entry)
    return Case([text.encode("ascii")], [False], [11], recs), sets


@pytest.mark.parametrize("unit", ["protein", "gene"])
def test_length_edges(ctx, unit):
    case, sets = length_edges(unit)
    got, want, dg, r = run(ctx, upload(ctx, case), case, unit=unit)
    assert same(got, want), [n for n, g, w in zip(Target.NAMES, got, want) if not np.array_equal(g, w)]
    group = got[0][1:1 + len(case.records)]
    for e in sets:
        a, b = e["equal"]
        assert len(r[4][a]) == e["n"] and group[a] == group[b], e["n"]                      # equal ones always merge
        assert all(group[x] != group[a] for x in e["near"]), e["n"]                          # near-copies never do
    assert ctx.protein_groups_stats()["rounds"] == 1


# ---- 3. options ------------------------------------------------------------------------------------------------------------------------
def test_options_change_which_records_group(ctx):
    with_codon = lambda c: "ATG" + tables_ref.quiet_codons(10, 21) + c + tables_ref.quiet_codons(19, 22) + "TAA"      # noqa: E731
    orf, gcn, gct, tga, tgg = (with_codon(c) for c in ("AAA", "GCN", "GCT", "TGA", "TGG"))
    seqs = [("CC" + orf + "CC" + orf[:-3] + "CC" + gcn + "CC" + gct + "CC").encode(), ("C" + tga + "C").encode(), ("CCCC" + tgg).encode()]
    n = len(orf)
    recs = [(0, 3, 2 + n, 1, 0, 0), (0, 5 + n, 4 + 2 * n - 3, 1, 0, 1),                                 # with its stop; cut off in front of it
            (0, 2 * n + 4, 3 * n + 3, 1, 0, 0), (0, 3 * n + 6, 4 * n + 5, 1, 0, 0), (1, 2, 1 + n, 1, 0, 0), (2, 5, 4 + n, 1, 0, 0)]
    case = Case(seqs, [False] * 3, [11, 11, 11], recs)
    batch = upload(ctx, case)
    seen = {}
    for name, kw in (("default", {}), ("include_stop", dict(include_stop=True)), ("lenient", dict(strict=False)),
                     ("table 4", dict(tables=np.array([11, 4, 4], np.int32))), ("Z", dict(unknown_residue="Z"))):
        got, want, dg, r = run(ctx, batch, case, **kw)
        assert same(got, want), name
        seen[name] = got[0][1:7].tolist()
    assert seen["default"] == [0, 0, 1, 2, 3, 4]                  # the cut record reads what the whole one reads without its stop
    assert seen["include_stop"] == [0, 1, 2, 3, 4, 5]             # ... and lacks the * the whole one ends in
    assert seen["lenient"] == [0, 0, 1, 1, 2, 3]                  # GCN is A whatever N is
    assert seen["table 4"] == [0, 0, 1, 2, 3, 3]                  # TGA reads W there
    assert seen["Z"] == seen["default"]


# ---- 4. order ----------------------------------------------------------------------------------------------------------------------------
def test_numbering_follows_first_appearance_in_the_array_passed(ctx):
    case = planted()
    batch = upload(ctx, case)
    n = len(case.records)
    orders = {"reversed": list(range(n))[::-1], "shuffled": np.random.default_rng(11).permutation(n).tolist(),
              "subset": list(range(1, n, 3)), "twice": list(range(n)) + list(range(n))}
    for name, order in orders.items():
        for unit in ("protein", "gene"):
            got, want, dg, r = run(ctx, batch, case, records=[case.records[g] for g in order], unit=unit)
            assert same(got, want), (name, unit)
            reps = got[1][1:1 + dg.n_groups]
            assert np.all(np.diff(reps) > 0)
    got, want, dg, r = run(ctx, batch, case, records=[case.records[g] for g in orders["twice"]])
    assert np.all(got[2][1:1 + dg.n_groups] % 2 == 0)             # every record twice: every group's size is even


# ---- 5. shapes ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def windows_case():
    """300 windows of 30 codons at 300 offsets of one random contig: 300 distinct strings (checked), in both units."""
    seq = tables_ref.quiet_codons(400, 31).encode("ascii")
    recs = [(0, 1 + 3 * g, 90 + 3 * g, 1 if g % 2 else -1, 1, 1) for g in range(300)]
    return Case([seq], [False], [11], recs)


def test_shapes(ctx):
    case = windows_case()
    batch = upload(ctx, case)
    for unit in ("protein", "gene"):
        got, want, dg, r = run(ctx, batch, case, records=[], unit=unit)                     # G = 0
        assert same(got, want) and dg.n_groups == 0 and dg.gene_begin.tolist() == [0, 0]
        got, want, dg, r = run(ctx, batch, case, records=case.records[:1], unit=unit)        # G = 1
        assert same(got, want) and dg.n_groups == 1
        got, want, dg, r = run(ctx, batch, case, records=[case.records[7]] * 300, unit=unit)   # one group, one long run
        assert same(got, want) and dg.n_groups == 1 and got[2][1] == 300
        got, want, dg, r = run(ctx, batch, case, unit=unit)                                   # 300 distinct strings
        assert same(got, want) and dg.n_groups == 300 and len(set(r[4])) == 300
        assert ctx.protein_groups_stats() == {"rounds": 1, "differing_pairs": 0}
    mixed = [case.records[g % 37] for g in range(300)]
    for which in itertools.product((True, False), repeat=3):                                  # optional outputs NULL in every combination
        got, want, dg, r = run(ctx, batch, case, records=mixed, which=which)
        assert same(got, want) and dg.n_groups == 37, which
        assert [x is None for x in (dg.representatives, dg.sizes, dg.digests)] == [not w for w in which]


# ---- 6. the collision path ---------------------------------------------------------------------------------------------------------------
def collide(strings, bits):
    """Distinct strings that share the low `bits` bits of digest word 0 (the reference's): the most in one bucket."""
    buckets = {}
    for s in set(strings):
        buckets.setdefault(ref.digest(s)[0] & ((1 << bits) - 1), set()).add(s)
    return max(len(b) for b in buckets.values())


@pytest.mark.parametrize("bits", [1, 2, 5])
@pytest.mark.parametrize("which", ["planted", "edges"])
@pytest.mark.parametrize("unit", ["protein", "gene"])
def test_collisions_are_settled_by_the_strings(ctx, monkeypatch, unit, which, bits):
    case = planted() if which == "planted" else length_edges(unit)[0]
    batch = upload(ctx, case)
    plain, want, dg, r = run(ctx, batch, case, unit=unit)
    assert same(plain, want) and ctx.protein_groups_stats()["rounds"] == 1
    deepest = collide(r[4], bits)
    assert deepest >= 2                                           # the inputs do collide in the low bits (on the CPU, by the reference)
    monkeypatch.setenv(KNOB, str(bits))
    got, want, dg, r = run(ctx, batch, case, unit=unit)
    assert same(got, want) and same(got, plain)                   # every output, digests included
    stats = ctx.protein_groups_stats()
    assert stats["rounds"] >= deepest > 1 and stats["differing_pairs"] >= 1, stats
    monkeypatch.setenv(KNOB, "62")
    with pytest.raises(ValueError, match=KNOB):
        run(ctx, batch, case, unit=unit)
    monkeypatch.delenv(KNOB)
    got, want, dg, r = run(ctx, batch, case, unit=unit)
    assert same(got, plain) and ctx.protein_groups_stats()["rounds"] == 1


# ---- 7. memory history -------------------------------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_what_memory_held(ctx):
    case = planted()
    first = None
    for poison, fill in ((None, CANARY), (0xFF, 0x00), (0x00, 0xFF), (None, CANARY)):
        ctx.debug_poison(poison)
        try:
            batch = upload(ctx, case)
            for unit in ("protein", "gene"):
                got, want, dg, r = run(ctx, batch, case, unit=unit, fill=fill)
                assert same(got, want), (poison, unit)
        finally:
            ctx.debug_poison(None)
        named = [g[1:1 + len(case.records)] for g in got[:1]] + [got[1][1:1 + dg.n_groups], got[2][1:1 + dg.n_groups]]
        first = named if first is None else first
        assert same(named, first)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_host_and_leave_the_context_usable(ctx):
    from pyrodigal_amd import ProteinGroups, _cabi
    case = planted()
    batch = upload(ctx, case)
    genes = gene_array(case.records)
    G = len(genes)
    t = Target(G)
    ptrs = [m.ptr + 8 for m in t.mem]
    host = np.zeros(2 * G + 8, np.int64)
    n_groups = ctypes.c_int64(-7)

    def raw(group=ptrs[0], reps=ptrs[1], sizes=ptrs[2], digests=ptrs[3], capacity=G, recs=genes, tables=case.tables, **change):
        o = ProteinGroups().opts()
        for name, v in change.items():
            setattr(o, name, v)
        tables = np.ascontiguousarray(tables, np.int32)
        rc = ctx.L.pga_group_proteins(ctx.h, batch.h, len(recs), ctypes.c_void_p(recs.ctypes.data), ctypes.c_void_p(tables.ctypes.data), ctypes.byref(o),
                                      ctypes.c_void_p(group), ctypes.c_void_p(reps), ctypes.c_void_p(sizes), ctypes.c_void_p(digests), capacity, None,
                                      ctypes.byref(n_groups))
        return rc, ctx.L.pga_last_error(ctx.h).decode()

    def changed(g, **fields):
        out = genes.copy()
        for name, v in fields.items():
            out[name][g] = v
        return out

    bad_table = case.tables.copy()
    bad_table[3] = 7
    for what, kw, word in (("a host pointer for the groups", dict(group=host.ctypes.data), "d_group is not device memory"),
                           ("a host pointer for the digests", dict(digests=host.ctypes.data), "d_digest is not device memory"),
                           ("a misaligned pointer", dict(sizes=ptrs[2] + 4), "d_size is not aligned"),
                           ("no d_group", dict(group=None), "d_group is NULL"),
                           ("capacity below G", dict(capacity=G - 1), "capacity = %d" % (G - 1)),
                           ("capacity below G for the sizes alone", dict(capacity=G - 1, reps=None), "capacity"),
                           ("a record outside its contig", dict(recs=changed(5, end=len(case.seqs[0]) + 1)), "gene 5 lies outside"),
                           ("a record of another contig", dict(recs=changed(4, contig=5)), "gene 4 lies outside"),
                           ("a record across the origin of a linear contig", dict(recs=changed(0, begin=len(case.seqs[0]) - 5, end=len(case.seqs[0]) + 6)), "gene 0"),
                           ("a unit that is none", dict(unit=2), "unit must be"),
                           ("an unknown residue that is no character", dict(unknown_residue=200), "unknown_residue"),
                           ("a table that is none", dict(tables=bad_table), "contig 3: 7 is not a valid translation table")):
        rc, msg = raw(**kw)
        assert rc == _cabi.PGA_EINVAL and word in msg and msg.startswith("pga_group_proteins: "), (what, rc, msg)
    with pytest.raises(ValueError, match="not device memory"):
        ctx.protein_groups(batch, genes, ProteinGroups(), tables=case.tables, out=(View(host.ctypes.data, (G,)),) + t.out[1:])
    with pytest.raises(ValueError, match="representatives needs shape"):
        ctx.protein_groups(batch, genes, ProteinGroups(), tables=case.tables, out=(t.out[0], View(ptrs[1], (G - 1,)), None, None))
    with pytest.raises(ValueError, match="digests needs shape"):
        ctx.protein_groups(batch, genes, ProteinGroups(), tables=case.tables, out=t.out[:3] + (View(ptrs[3], (G, 3)),))
    with pytest.raises(TypeError, match="int64"):
        ctx.protein_groups(batch, genes, ProteinGroups(), tables=case.tables, out=(View(ptrs[0], (G,), "<i4"),) + t.out[1:])
    with pytest.raises(TypeError, match="group is required"):
        ctx.protein_groups(batch, genes, ProteinGroups(), tables=case.tables, out=(None,) + t.out[1:])
    with pytest.raises(ValueError, match="tables="):
        ctx.protein_groups(batch, genes, ProteinGroups())
    with pytest.raises(TypeError, match="ProteinGroups"):
        ctx.protein_groups(batch, genes, "protein", tables=case.tables)
    assert n_groups.value == -7 and np.all(host == 0)
    assert all(np.all(m.to_numpy(np.uint8) == CANARY) for m in t.mem)           # nothing was written anywhere
    rc, msg = raw()                                                              # the context runs a good call afterwards
    assert rc == 0, msg
    want = ref.protein_groups_ref(case.seqs, case.circular, case.records, "protein", case.tables)
    assert n_groups.value == len(want[1]) and same(t.read(), t.expect(*want[:4]))
    rc, msg = raw(unit=_cabi.GROUP_GENE, tables=bad_table)                       # (the tables are not read for bases)
    assert rc == 0, msg


# ---- 9. composition ----------------------------------------------------------------------------------------------------------------------
def test_the_representatives_proteins_indexed_by_group_are_everybodys(ctx):
    from pyrodigal_amd import ProteinGroups, ProteinTokens
    case = planted()
    batch = upload(ctx, case)
    genes = gene_array(case.records)
    G = len(genes)
    got, want, dg, r = run(ctx, batch, case)
    assert same(got, want)
    group, reps = got[0][1:1 + G], got[1][1:1 + dg.n_groups]
    spec = ProteinTokens({chr(k): k for k in range(1, 128)}, dtype="uint8", layout="padded")
    W = int(spec.lengths(genes).max())

    def tokens(records):
        mem = keep(hip_mem.DeviceArray.from_numpy(np.full((len(records), W), CANARY, np.uint8)))
        ctx.translate_tokens(batch, records, spec, tables=case.tables, out=View(mem.ptr, (len(records), W), "|u1"))
        return mem.to_numpy(np.uint8).reshape(len(records), W)

    everybody, unique = tokens(genes), tokens(genes[reps])
    assert np.array_equal(unique[group], everybody)                               # row for row
    assert [bytes(row[row != 0]) for row in everybody] == r[4]                    # ... and they are the strings that were grouped


# ---- 10. through the finder ----------------------------------------------------------------------------------------------------------------
FINDER_SCRIPT = r'''
import sys
import torch                                   # first: the library then binds to the HIP runtime of torch's wheel
if not torch.cuda.is_available():
    print("torch sees no GPU")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
import numpy as np
from pyrodigal_amd import DeviceGroups, DeviceSequences, ProteinGroups, benchdata, lib
from tests.util import read_fasta

bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])
s = read_fasta("GCF_001457455.1_NCTC11397_genomic_100kb.fna.gz")[0][1].encode("ascii")
rc = s.translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1]
seqs = [s, rc, s[1000:50000]]


def check(given, spec, **options):
    finder = lib.GeneFinder(meta=True, metagenomic_bins=bins)
    want_genes = finder.find_genes_batch(given, **options)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        genes, dg = finder.find_groups_batch(given, spec, **options)
        biggest = dg.sizes.max() if dg.n_groups else None          # a consumer on the same stream
    assert isinstance(dg, DeviceGroups)
    key = lambda x: [[(g.begin, g.end, g.strand) for g in c] for c in x]
    assert key(genes) == key(want_genes)
    flat = [g for c in genes for g in c]
    G = len(flat)
    strings = [g.translate(include_stop=spec.include_stop) if spec.of == "protein" else g.sequence() for g in flat]
    number, group, reps, sizes = {}, [], [], []
    for g, p in enumerate(strings):
        u = number.setdefault(p, len(number))
        if u == len(reps):
            reps.append(g); sizes.append(0)
        sizes[u] += 1
        group.append(u)
    for t in (dg.group, dg.representatives, dg.sizes, dg.digests):
        assert t.is_cuda and t.dtype == torch.int64 and t.device.index == 0
    assert dg.n_groups == len(reps) and tuple(dg.group.shape) == (G,) and tuple(dg.digests.shape) == (G, 2)
    assert tuple(dg.representatives.shape) == tuple(dg.sizes.shape) == (dg.n_groups,)
    assert dg.group.cpu().tolist() == group and dg.representatives.cpu().tolist() == reps and dg.sizes.cpu().tolist() == sizes
    assert dg.digests.cpu().tolist() == [list(ProteinGroups.digest_of(p)) for p in strings]
    assert int(biggest) == max(sizes)
    assert dg.gene_begin.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in genes])]).tolist()
    return G, dg.n_groups


G, U = check(seqs, ProteinGroups())
assert G > 150 and U < G, (G, U)                # the reverse complement and the piece carry the genome's proteins again
G1, U1 = check(seqs, ProteinGroups("gene"))
assert G1 == G and U1 < G
assert check(seqs, ProteinGroups(include_stop=True, strict=False))[0] == G
rows = np.full((len(seqs), max(map(len, seqs))), ord("N"), np.uint8)
for i, q in enumerate(seqs):
    rows[i, :len(q)] = np.frombuffer(q, np.uint8)
given = DeviceSequences(torch.from_numpy(rows).cuda(), [len(q) for q in seqs])
assert check(given, ProteinGroups()) == (G, U)
Gc, Uc = check(seqs, ProteinGroups(), circular=True)
assert Uc < Gc
print("find_groups_batch ok: %d genes in %d groups" % (G, U))
'''


def test_find_groups_batch_in_a_fresh_process(tmp_path):
    """torch is imported by the child alone (this process holds the library's HIP runtime and gets no second one); `out=` omitted
    allocates the tensors under torch's current stream.  The child says so when torch sees no GPU, and the test is skipped."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "torch_protein_groups.py"
    script.write_text(FINDER_SCRIPT)
    done = subprocess.run([sys.executable, str(script), root], timeout=300, capture_output=True, text=True)
    assert done.returncode == 0, "child ended with %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    if "torch sees no GPU" in done.stdout:
        pytest.skip("torch sees no GPU")
    assert "find_groups_batch ok" in done.stdout
