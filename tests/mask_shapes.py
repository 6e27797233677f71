"""Batches that put the mask-union builder of DESIGN.md 4.9 -- pga_launch_mask_union: k_mask_paint_runs / find_runs,
k_mask_paint_regions / paint_words, mask_edges, k_mask_count, k_scan_counts, k_mask_place -- at its bit, word, wave, tile and contig
edges: the inputs of tests/test_mask_shapes_cpu.py and tests/test_mask_shapes_gpu.py.  A helper module, not a test.

A shape is a batch: contigs, per-contig named regions or None, and the switches mask / mask_lowercase / min_mask.  Nothing is drawn
at random: what the bitmap sees is a base's place in the batch (g = the contig's base + the position), so every design says where in
the batch its contigs begin -- a filler contig of chosen length goes first -- and fillers and backgrounds are upper-case ACGT
(tests.util.synthetic_contig), so only the designed letters qualify.  A design is built once and emitted for every source that can
express it: runs of N, the same runs in lower case, the same intervals as named regions.

The reference is tests/mask_ref.py.  `restate` is the builder's bit logic in plain Python -- paint, mask_edges, the counts per 2 048
bases, the scan in rounds, the placement, the contig offsets, the run walk -- which counts EVENTS: one expression of the kernels
deciding one way at one kind of boundary.  It is test code: it tells the CPU test what the catalogue reaches, and replaces no
reference.  An event that no batch can produce is listed in IMPOSSIBLE with its reason, not dropped."""
from bisect import bisect_right
from collections import Counter, namedtuple

import numpy as np

from tests import mask_ref
from tests.util import synthetic_contig

WORD = 32                      # bases per word of the bitmap
GROUP = 64 * WORD              # bases per wavefront of k_mask_count / k_mask_place (MK_WAVE_BITS): one count
BLOCK = 256 * WORD             # bases per workgroup of the two
SCAN_ROUND = 4096              # counts per round of k_scan_counts
TILE = 3072                    # positions of a workgroup of find_runs (an extraction tile)
PER_THREAD = 12                # ... of one of its threads
SOURCES = ("N", "lower", "named")
FILL = GROUP
# shapes whose node count masking changes at the extraction stage: at least this many (94 by the references, asserted of them in
# tests/test_mask_shapes_cpu.py and of the device in tests/test_mask_shapes_gpu.py)
MASKING_CHANGES_NODES = 90

Shape = namedtuple("Shape", "name seqs regions mask lower min_mask claims")

_UNIT = {}


def background(n, seed=0):
    """n upper-case letters; long ones by repetition of 2 048."""
    if n <= 4096:
        return synthetic_contig(n, 0.5, 7000 + seed)
    if seed not in _UNIT:
        _UNIT[seed] = synthetic_contig(GROUP, 0.5, 7000 + seed)
    return (_UNIT[seed] * (n // GROUP + 1))[:n]


def painted(seq, ivs, source):
    s = bytearray(seq)
    for b, e in ivs:
        assert 0 <= b < e <= len(s)
        s[b:e] = b"N" * (e - b) if source == "N" else bytes(s[b:e]).lower()
    return bytes(s)


def layout(bounds, ivs_g):
    """Contigs that begin at the batch positions `bounds` (the last entry is the batch's end; equal neighbours are empty contigs) and
    intervals in batch coordinates, each inside one contig -> (lengths, {contig: [(begin, end)]})."""
    lens = [bounds[k + 1] - bounds[k] for k in range(len(bounds) - 1)]
    assert all(n >= 0 for n in lens)
    ivs = {}
    for g0, g1 in ivs_g:
        c = bisect_right(bounds[:-1], g0) - 1
        assert bounds[c] <= g0 < g1 <= bounds[c + 1], (g0, g1, bounds[c], bounds[c + 1])
        ivs.setdefault(c, []).append((g0 - bounds[c], g1 - bounds[c]))
    return lens, ivs


def emit(name, lens, ivs, min_mask, sources=SOURCES, claims=None, seed=0):
    """The design -- contig lengths and {contig: intervals} -- once per source.  Without `claims` the design claims its number of
    merged intervals: every interval as a named region, the ones the rule keeps (`e - b >= min_mask or e == L`) as runs; a design
    whose intervals touch inside a contig says what it claims itself."""
    base = [background(n, 31 * seed + k) for k, n in enumerate(lens)]
    if claims is None:
        kept = sum(e - b >= min_mask or e == lens[c] for c, v in ivs.items() for b, e in v)
        claims = dict(n=dict(named=sum(len(v) for v in ivs.values()), N=kept, lower=kept))
    out = []
    for src in sources:
        if src == "named":
            out.append(Shape(name + "/named", base, [ivs.get(k) for k in range(len(lens))], False, False, min_mask, claims))
        else:
            seqs = [painted(s, ivs.get(k, ()), src) for k, s in enumerate(base)]
            out.append(Shape(name + "/" + src, seqs, None, src == "N", src == "lower", min_mask, claims))
    return out


def source_of(shape):
    return shape.name.rsplit("/", 1)[1]


def claim(shape, key):
    v = shape.claims.get(key)
    return v.get(source_of(shape)) if isinstance(v, dict) else v


def reference(shape):
    """What pga_result.masks must hold: one (n, 2) int32 array per contig."""
    reg = shape.regions or [None] * len(shape.seqs)
    return [mask_ref.mask_union(s, r, shape.mask, shape.lower, shape.min_mask) for s, r in zip(shape.seqs, reg)]


def bases_of(seqs):
    return np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)


def measure(shape, ref=None):
    """What a shape's claims are held against, from the reference alone: the number of merged intervals, their lengths, the bits
    (g0 & 31, (g1 - 1) & 31) and the words they span in the batch's bitmap, and each contig's base."""
    ref = reference(shape) if ref is None else ref
    base = bases_of(shape.seqs)
    g = [(int(base[c] + b), int(base[c] + e)) for c, r in enumerate(ref) for b, e in r.tolist()]
    return dict(n=len(g), len=[g1 - g0 for g0, g1 in g], bits=[(g0 & 31, (g1 - 1) & 31) for g0, g1 in g],
                words=[((g1 - 1) >> 5) - (g0 >> 5) + 1 for g0, g1 in g], base=[int(x) for x in base[:-1]], g=g)


# ---- bit and word ------------------------------------------------------------------------------------------------------------------

BIT_FIRST = (0, 1, 31)
BIT_LENGTHS = (1, 2, 31, 32, 33, 64, 65)


def bit_word_series():
    """One interval per contig, its first base at bit 0, 1 or 31 of a word, 1 .. 65 bases long: the last base falls on bit 0, 30 and
    31 among others, the first and the last word are the same word (1 base; 2 from bit 1), neighbours (2 from bit 31) and apart (65)."""
    out = []
    for r0 in BIT_FIRST:
        lens, ivs, bits, words = [FILL + 7], {}, [], []
        at = lens[0]
        for k, n in enumerate(BIT_LENGTHS):
            b = (r0 - at) % WORD + 2 * WORD
            ivs[k + 1] = [(b, b + n)]
            bits.append((r0, (r0 + n - 1) % WORD))
            words.append((r0 + n - 1) // WORD + 1)
            lens.append(b + n + 70 + k)
            at += lens[-1]
        n = len(BIT_LENGTHS)
        out += emit("bit/first%d" % r0, lens, ivs, 1, claims=dict(n=n, bits=bits, len=list(BIT_LENGTHS), words=words), seed=r0)
    return out


LANE_WORDS = (1, 2, 63, 64, 65, 128, 129)


def lanes_series():
    """One interval from bit 0 of a word over 1 .. 129 words (the 64 lanes of k_mask_paint_regions take the words in turn: one turn,
    exactly one, two, exactly two, three), the last word full and partial."""
    out = []
    for full in (True, False):
        lens, ivs, words, length = [FILL + 11], {}, [], []
        at = lens[0]
        for k, W in enumerate(LANE_WORDS):
            b = -at % WORD + WORD
            n = WORD * W if full else WORD * (W - 1) + 5
            ivs[k + 1] = [(b, b + n)]
            words.append(W)
            length.append(n)
            lens.append(b + n + 40 + k)
            at += lens[-1]
        out += emit("lanes/%s" % ("full" if full else "partial"), lens, ivs, 1,
                    claims=dict(n=len(LANE_WORDS), words=words, len=length, bits=[(0, 31 if full else 4)] * len(LANE_WORDS)), seed=40 + full)
    return out


# ---- the groups and blocks of the counting and placing kernels ----------------------------------------------------------------------------

def group_series():
    """A run that begins in the last bit of a group of 2 048 bases and one that ends in the first bit of one (a group with a start and
    no end next to one with an end and no start), the same at a block of 8 192, and a run that is one whole group and nothing else."""
    bounds = [0, 2000, 2100, 4000, 4200, 6100, 8300, 16300, 16500, 24500, 24700, 26000]
    ivs_g = [(GROUP - 1, GROUP + 2), (2 * GROUP - 6, 2 * GROUP + 1), (3 * GROUP, 4 * GROUP), (2 * BLOCK - 1, 2 * BLOCK + 6), (3 * BLOCK - 6, 3 * BLOCK + 1)]
    lens, ivs = layout(bounds, ivs_g)
    return emit("group/edges", lens, ivs, 1, claims=dict(n=5, g=ivs_g), seed=50)


CONTIG_WORDS = (0, 1, 62, 63)
STARTS_BEFORE = (0, 1, 3)


def contig_word_designs():
    """(word of the contig's first base in its group, run starts in the words before it, the bit of the first base, which of
    below / at / above hold a run start in the first base's own word)."""
    out = [(w, nb, 5, ("below", "at", "above")) for w in CONTIG_WORDS for nb in STARTS_BEFORE if nb == 0 or w > 0]
    out += [(1, 1, 5, own) for own in ((), ("below",), ("at",), ("above",))]
    out += [(1, 1, 0, ("at", "above")), (62, 3, 31, ("below", "at")), (0, 0, 0, ())]
    return out


def contig_word_series():
    """k_mask_place's thread per contig: the contig's first base in word 0, 1, 62 and 63 of its group, with 0, 1 and 3 run starts in the
    words before it (all in word 0 of the group, which is what a contig in word 1 leaves room for), and one-base runs in its own word
    below, at and above its first base.  Every design has two groups to itself: the previous contig P = [G - 40, first base), the
    contig C of 60 bases, fillers around them."""
    bounds, ivs_g, n = [0], [], 0
    for k, (w, nb, bit, own) in enumerate(contig_word_designs()):
        G = 2 * GROUP * k + GROUP
        first = G + WORD * w + bit
        bounds += [G - 40, first, first + 60]
        ivs_g += [(G + 3 + 4 * j, G + 4 + 4 * j) for j in range(nb)]
        if "below" in own:
            ivs_g.append((first - 3, first - 2))
        if "at" in own:
            ivs_g.append((first, first + 1))
        if "above" in own:
            ivs_g.append((first + 4, first + 5))
        n += nb + len(own)
    bounds.append(bounds[-1] + 500)
    lens, ivs = layout(bounds, sorted(ivs_g))
    return emit("group/contig_word", lens, ivs, 1, claims=dict(n=n, g=sorted(ivs_g)), seed=60)


# ---- scan rounds -----------------------------------------------------------------------------------------------------------------------

SCAN_GROUPS = (SCAN_ROUND - 1, SCAN_ROUND, SCAN_ROUND + 1)


def scan_shapes(n_groups):
    """A batch whose bitmap is exactly n_groups counts long (about 8.4 Mbases, built by repetition; three contigs), with runs in the
    first group, in the last, and across the boundaries of groups 4 094 | 4 095 and 4 095 | 4 096: at the second one the first round of
    the scan ends, and its carry holds one start more than ends.  STAGE_SEQUENCE only."""
    total = n_groups * GROUP - WORD
    bounds = [0, 5000, total - 5000, total]
    cand = [(10, 70), (GROUP - 1, GROUP + 2), ((SCAN_ROUND - 1) * GROUP - 3, (SCAN_ROUND - 1) * GROUP + 3),
            (SCAN_ROUND * GROUP - 3, SCAN_ROUND * GROUP + 60), (total - 5009, total - 5000), (total - 5000, total - 4993),
            (total - 200, total - 140), (total - 70, total)]
    ivs_g = [iv for iv in cand if iv[1] <= total - 5000 or iv[0] >= total - 5000]
    ivs_g = sorted(iv for iv in ivs_g if iv[1] <= total)
    assert all(a[1] <= b[0] for a, b in zip(ivs_g, ivs_g[1:]))
    lens, ivs = layout(bounds, ivs_g)
    return emit("scan/%d" % n_groups, lens, ivs, 1, claims=dict(n=len(ivs_g), g=ivs_g, groups=n_groups), seed=70)


def groups_of(seqs):
    """Counts of the builder for a batch (pga_mask_waves)."""
    total = sum(len(s) for s in seqs)
    return ((total + WORD) // WORD + 63) // 64


# ---- contig joints ---------------------------------------------------------------------------------------------------------------------

JOINT_MIN_MASK = 10
JOINTS = (("31|0", 2400), ("0|1", 2753), ("mid", 3117), ("group", 2 * GROUP))


def joint_series(mm=JOINT_MIN_MASK):
    """Contig i ends in a run and contig i + 1 begins with one, both min_mask - 1, min_mask or min_mask + 1 long: the first reaches the
    end of its sequence and is masked whatever its length, the second only by the rule; as named regions both are.  The joint lies
    between bit 31 and bit 0, between bit 0 and bit 1, inside a word, and on a group boundary, with 0 .. 3 empty contigs in it (then an
    empty contig is also the batch's first and last)."""
    out = []
    for m in (mm - 1, mm, mm + 1):
        for empties in (0, 1, 2, 3):
            bounds, ivs_g = [0] * (1 + (empties > 0)), []
            for _, j in JOINTS:
                bounds += [j - 150] + [j] * (empties + 1) + [j + 150]
                ivs_g += [(j - m, j), (j, j + m)]
            bounds += [4500] * (1 + (empties > 0))
            lens, ivs = layout(bounds, ivs_g)
            runs = 4 + 4 * (m >= mm)
            out += emit("joint/m%d/empty%d" % (m, empties), lens, ivs, mm, claims=dict(n=dict(named=8, N=runs, lower=runs), empties=empties), seed=80 + m)
    for m in (mm - 1, mm + 1):                      # a whole contig of five bases masked between two masked neighbours
        lens, ivs = layout([0, 2000, 2150, 2155, 2300, 2600], [(2140, 2150), (2150, 2155), (2155, 2155 + m)])
        out += emit("joint/whole/m%d" % m, lens, ivs, mm, seed=90 + m)
    return out


SHORT_TRIOS = {"a": ("N", "NC", "CN"), "b": ("NN", "A", "N"), "c": ("AC", "NN", "C")}


def _short(text):
    iv = [(k, k + 1) for k, ch in enumerate(text) if ch == "N"]
    if len(iv) == 2:
        iv = [(0, 2)]
    return len(text), iv


def short_series(mm=JOINT_MIN_MASK):
    """Contigs of one and two bases -- no extraction tile: the one-thread-per-contig tail of find_runs, in blocks of 256 contigs, and
    the contig marks of k_mask_paint_regions in blocks of 256 -- masked and not, as contig 255, 256 and 257 of a batch of 260; and
    batches of 255 and 256 contigs in all, whose last contig ends in a run (k_mask_place has n_contigs + 1 contig threads)."""
    out = []
    for name, trio in SHORT_TRIOS.items():
        lens, ivs = [300] + [30] * 254, {}
        for k, text in enumerate(trio):
            n, iv = _short(text)
            lens.append(n)
            if iv:
                ivs[255 + k] = iv
        lens += [30, 30]
        for m in (1, mm):
            out += emit("short/%s/mm%d" % (name, m), lens, ivs, m, seed=100)
    for total in (255, 256):
        lens = [300] + [30] * (total - 2) + [2]
        out += emit("short/total%d" % total, lens, {total - 1: [(1, 2)], 3: [(28, 30)]}, mm, seed=100)
    return out


# ---- the run walk ------------------------------------------------------------------------------------------------------------------------

WALK_MIN_MASK = 10


def walk_series(mm=WALK_MIN_MASK):
    """find_runs: a run that begins at L - 1 - k, k = 0 .. 17, and reaches L (none, one and two steps of eight bytes, then single
    bytes; masked whatever its length); the same run ending one base short of L; a run of 1 .. 17 followed by a non-member; runs that
    begin on position 0 and 11 of a thread's twelve and on position 0 of the next thread; runs that end at 3 071, 3 072 and 3 073 of a
    contig of two tiles, one that begins on the second tile's first position and one whose previous base, in the first tile, is a
    member; contigs one base longer than a tile and exactly a tile long."""
    out = []
    lens, ivs = [FILL + 3], {}
    for k in range(18):
        L = 200 + k % 5
        lens.append(L)
        ivs[k + 1] = [(L - 1 - k, L)]
    out += emit("walk/reach", lens, ivs, mm, seed=110)
    ivs = {k + 1: [(lens[k + 1] - 2 - k, lens[k + 1] - 1)] for k in range(18)}
    out += emit("walk/short_of_L", lens, ivs, mm, seed=110)
    out += emit("walk/followed", [FILL + 5] + [150] * 17, {n: [(60, 60 + n)] for n in range(1, 18)}, mm, seed=111)
    out += emit("walk/followed_mm1", [FILL + 5] + [150] * 17, {n: [(60, 60 + n)] for n in range(1, 18)}, 1, seed=111)
    out += emit("walk/thread", [FILL + 9, 400], {1: [(120, 130), (143, 155), (168, 180)]}, mm, seed=112)
    two = [[(TILE - 12, TILE - 1), (TILE + 28, TILE + 40)], [(TILE - 12, TILE)], [(TILE - 12, TILE + 1)], [(TILE, TILE + 13)], [(TILE - 1, TILE + 13)]]
    lens = [FILL + 13] + [TILE + 228] * len(two) + [TILE + 1] * 3 + [TILE]
    ivs = {k + 1: v for k, v in enumerate(two)}
    ivs.update({6: [(TILE, TILE + 1)], 7: [(TILE - 1, TILE + 1)], 8: [(TILE - 12, TILE + 1)], 9: [(TILE - 10, TILE)]})
    out += emit("walk/tile", lens, ivs, mm, seed=113)
    return out


# ---- byte classes ------------------------------------------------------------------------------------------------------------------------

LOWER_EDGE_BYTES = (0x40, 0x41, 0x5a, 0x5b, 0x60, 0x61, 0x7a, 0x7b, 0x7f, 0x80, 0xff)
UNKNOWN_BYTES = (ord("N"), ord("n"), ord("R"), 0x00)
BYTE_RUN = (30, 70)            # the run every byte is planted in; its eight-byte steps begin at 31, the planted byte is in the second


def byte_series():
    """RunOfLowerCase::all8 is three byte tricks without carries whose edges are 0x60 | 0x61, 0x7a | 0x7b and 0x7f | 0x80: each of
    eleven bytes in each of the eight lanes of an eight-byte step inside an otherwise lower-case run (0x61 and 0x7a continue it, the
    others split it; min_mask 10 and 1).  For the unknown source N, n, R and 0x00 likewise inside a run of N: all four continue it.
    A step of eight that accepts a byte never asks Run::is about it, so each byte also stands where Run::is decides alone: as a run's
    first byte, as the byte before it, and in the single-byte walk behind the last step."""
    out = []
    b, e = BYTE_RUN
    for name, values, lower in (("lower", LOWER_EDGE_BYTES, True), ("unknown", UNKNOWN_BYTES, False)):
        seqs = [background(FILL + 17, 120)]
        for v in values:
            for lane in range(8):
                s = bytearray(painted(background(100, 121 + lane), [(b, e)], "lower" if lower else "N"))
                s[b + 1 + 8 + lane] = v
                seqs.append(bytes(s))
            # ... and where Run::is alone decides: the run's first byte, the byte before it, and the single-byte walk behind the last
            # step of eight (a run of 15 that ends five bases before the end of its contig)
            for at, run in ((b, (b, b + 20)), (b - 1, (b, b + 20)), (92, (80, 95)), (94, (80, 95))):
                s = bytearray(painted(background(100, 130 + at), [run], "lower" if lower else "N"))
                s[at] = v
                seqs.append(bytes(s))
        for mm in (10, 1):
            out.append(Shape("byte/%s/mm%d/%s" % (name, mm, "lower" if lower else "N"), seqs, None, not lower, lower, mm, {}))
    return out


# ---- sources together --------------------------------------------------------------------------------------------------------------------

def together_series():
    out = []
    fill = background(FILL + 21, 130)
    bgd = background(600, 131)

    def put(*pieces):
        s = bytearray(bgd)
        for at, text in pieces:
            s[at:at + len(text)] = text
        return bytes(s)

    def low(b, e):
        return (b, bytes(bgd[b:e]).lower())
    # an N run of 30 touching a lower-case run of 30 under min_mask 50: neither qualifies, nothing is masked
    out.append(Shape("together/touching_short/N+lower", [fill, put((100, b"N" * 30), low(130, 160))], None, True, True, 50, dict(n=0)))
    # n runs: both sources, one interval
    out.append(Shape("together/n_runs/N+lower", [fill, put((100, b"n" * 60), (300, b"n" * 49))], None, True, True, 50, dict(n=1, len=[60])))
    # a lower-case run with n inside: the lower-case source masks it all, the unknown source nothing
    out.append(Shape("together/n_inside/N+lower", [fill, put(low(100, 170), (130, b"n" * 5))], None, True, True, 50, dict(n=1, len=[70])))
    # a named one-base region that joins two qualifying runs, and one that touches a run that does not qualify
    out.append(Shape("together/join/N+lower+named", [fill, put((100, b"N" * 50), low(151, 201), (300, b"N" * 30))], [None, [(150, 151), (330, 331)]],
                     True, True, 50, dict(n=2, len=[101, 1])))
    # 0, 1, 3, 4 and 5 named regions in the batch (k_mask_paint_regions: workgroups of four), next to a lower-case run
    for k in (0, 1, 3, 4, 5):
        regs = [(40 * j + 10, 40 * j + 20) for j in range(k)]
        out.append(Shape("together/regions%d/lower+named" % k, [fill, put(low(400, 460))], [None, regs] if k else None, False, True, 50,
                         dict(n=k + 1, len=[10] * k + [60])))
    # duplicates, and one nested in the other
    out.append(Shape("together/duplicate_nested/named", [fill, bgd], [None, [(100, 200), (100, 200), (120, 130), (300, 310), (300, 310), (199, 201)]],
                     False, False, 50, dict(n=2, len=[101, 10])))
    return out


# ---- densest lists -----------------------------------------------------------------------------------------------------------------------

def cap_of(shape):
    """FindCall's bound on the list's length (finder.hip)."""
    total, nc = sum(len(s) for s in shape.seqs), len(shape.seqs)
    per_source = total // max(1, shape.min_mask) + nc + 1
    n_regions = sum(len(r) for r in shape.regions or [] if r is not None)
    return min((per_source if shape.mask else 0) + (per_source if shape.lower else 0) + n_regions, total // 2 + nc + 1)


def densest_series():
    """The longest lists a batch can have, against `cap` = total / 2 + NC + 1: every second base of 4 097 (2 049 intervals under a
    bound of 2 050), 300 one-base contigs, 300 two-base contigs aC; alone in their batch, where the bound is tightest, and behind a
    filler of odd length."""
    out = []
    fill = background(FILL + 7, 140)
    for src, one in (("lower", b"a"), ("N", b"N")):
        alt = (one + b"C") * 2048 + one
        for name, seqs in (("alternating", [alt]), ("ones", [one] * 300), ("twos", [one + b"C"] * 300)):
            n = 2049 if name == "alternating" else 300
            out.append(Shape("densest/%s/alone/%s" % (name, src), seqs, None, src == "N", src == "lower", 1, dict(n=n)))
            out.append(Shape("densest/%s/filler/%s" % (name, src), [fill] + seqs, None, src == "N", src == "lower", 1, dict(n=n)))
    return out


def catalogue():
    """Every shape but the scan rounds (scan_shapes), which are 8.4 Mbases each and built when asked for."""
    return (bit_word_series() + lanes_series() + group_series() + contig_word_series() + joint_series() + short_series() + walk_series()
            + byte_series() + together_series() + densest_series())


def permuted(n):
    """The one fixed permutation every batch is also run in: reversed, then rotated by one."""
    idx = list(range(n))[::-1]
    return idx[1:] + idx[:1]


def pure_unknown(shape):
    """Its only source is runs of unknown bases: the oracle masks the same runs."""
    return shape.mask and not shape.lower and shape.regions is None


# ---- the builder restated --------------------------------------------------------------------------------------------------------------

def _cls(n):
    return n if n < 2 else "several"


def _word_class(w):
    return w if w in CONTIG_WORDS else "between"


EVENTS = tuple(
    [("paint", k) for k in ("same_word", "next_word", "far_word", "first_bit0", "first_bit31", "first_mid", "last_bit0", "last_bit31", "last_mid")]
    + [("region_words", k) for k in ("1", "2..63", "64", "65..127", "128", "129..")]
    + [("bit0", before, c) for before in (0, 1) for c in (0, 1)]                  # a set bit 0: `before`, and `c` of that bit
    + [("bit31", after, c) for after in (0, 1) for c in (0, 1)]                   # a set bit 31: `after`, and `c_after`
    + [("bit31_in_last_word",), ("word0_set",), ("last_word_set",), ("split_inside_word",)]
    + [("first_base", before, c) for before in (0, 1) for c in (0, 1)]            # a set bit at a contig's first base
    + [("group", s, e) for s in ("no_start", "starts") for e in ("no_end", "ends")]
    + [("group_edge", k) for k in ("start_in_last_bit", "end_in_first_bit", "whole_group")]
    + [("block_edge", k) for k in ("start_in_last_bit", "end_in_first_bit")]
    + [("contig_thread", w, n) for w in CONTIG_WORDS + ("between",) for n in (0, 1, "several")]
    + [("partial_word", bit, n) for bit in ("bit0", "above0") for n in ("none", "some")]
    + [("own_word", k) for k in ("below", "at", "above")]
    + [("end_thread", k) for k in ("none", "some")]
    + [("find_contig", k) for k in ("alone", "equal_bases")]
    + [("scan", k) for k in ("one_round", "two_rounds", "carry_differs", "full_round")]
    + [("cap", k) for k in ("half_binds", "sources_bind", "one_below", "full", "exceeded")]
    + [("walk", "steps8", k) for k in (0, 1, "several")] + [("walk", "stop8", k) for k in ("no_room", "non_member")]
    + [("rule", k) for k in ("long", "short_reaches_L", "short_dropped", "exactly_min")]
    + [("start", k) for k in ("batch_first", "contig_first_after_member", "contig_first_after_non_member", "thread_first", "thread_last",
                              "tile_first", "not_tile_first_after_member")]
    + [("tail", L, k) for L, ks in ((1, ("0", "1")), (2, ("00", "01", "10", "11"))) for k in ks] + [("tail_block", 0), ("tail_block", 1)]
    + [("all8_lower", v, lane) for v in LOWER_EDGE_BYTES for lane in range(8)]
    + [("all8_unknown", v, lane) for v in UNKNOWN_BYTES for lane in range(8)]
    # Run::is deciding alone on an edge byte: a run's first byte, the byte before it, a byte of the single-byte walk
    + [("is", "lower", "first", v) for v in (0x61, 0x7a)] + [("is", "lower", "before", v) for v in LOWER_EDGE_BYTES if v not in (0x61, 0x7a)]
    + [("is", "lower", "walk", v) for v in LOWER_EDGE_BYTES]
    + [("is", "unknown", role, v) for role in ("first", "walk") for v in UNKNOWN_BYTES])

# Events no batch can produce, each with its reason: what the CPU test accepts as missing from the whole catalogue, and nothing else.
IMPOSSIBLE = {
    ("first_base", 0, 0): "a contig's first base always carries the contig mark: c is set there, whatever the bit before it",
    ("first_base", 1, 0): "the same, with the neighbour's last base masked",
    ("bit31_in_last_word",): "the last word holds bit `total` (pga_mask_words); its bit 31 lies at or behind the end of the batch and is never painted, "
                             "so the `w + 1 < nw` guards of `after` and `c_after` never decide for a set bit",
    ("contig_thread", 0, 1): "a contig whose first base lies in word 0 of its group has no whole word before it in the group",
    ("contig_thread", 0, "several"): "the same",
    ("partial_word", "bit0", "some"): "the mask (1u << 0) - 1u is empty: no bit of the word lies below bit 0",
    ("cap", "exceeded"): "disjoint runs that do not touch number at most (total + NC) / 2 < total / 2 + NC + 1, the runs of one kind that qualify "
                         "at most total / min_mask + NC, and a union has no more intervals than its sources: the list fills `cap` exactly when "
                         "every named region stands alone (`full`) and never exceeds it, so `ks < cap` and `min(n, cap)` never cut",
}


def _all8_lower(w):
    H = 0x8080808080808080
    if w & H:
        return False
    M = (1 << 64) - 1
    return ((w + 0x1f1f1f1f1f1f1f1f) & M & H) == H and ((w + 0x0505050505050505) & M & H) == 0


def _find_runs(seqs, base, member, all8, min_mask, kind, ev, letters):
    """find_runs restated: the candidates are the members whose previous byte OF THE SAME CONTIG is none (`i > 0 &&`), the walk is the
    kernel's.  `member`: bool array over the batch; `all8(batch position)`: the kernel's test of eight bytes at once."""
    out = []
    for c, s in enumerate(seqs):
        L, g = len(s), int(base[c])
        m = member[g:g + L]
        if L in (1, 2):
            ev[("tail", L, "".join("01"[int(x)] for x in m))] += 1
            ev[("tail_block", min(c // 256, 1))] += 1
            for i in range(L):
                if not m[i] or (i > 0 and m[i - 1]):
                    continue
                e = i + 1
                while e < L and m[e]:
                    e += 1
                if e - i >= min_mask or e == L:
                    out.append((c, i, e))
            continue
        if L < 3:
            continue
        prev = np.concatenate([[False], m[:-1]])
        at_tile = np.arange(TILE, L, TILE)
        if len(at_tile) and np.any(m[at_tile] & m[at_tile - 1]):
            ev[("start", "not_tile_first_after_member")] += 1
        for i in np.flatnonzero(m & ~prev).tolist():
            if i == 0:
                ev[("start", "batch_first" if g == 0 else "contig_first_after_member" if member[g - 1] else "contig_first_after_non_member")] += 1
            elif i % TILE == 0:
                ev[("start", "tile_first")] += 1
            if i % PER_THREAD == 0:
                ev[("start", "thread_first")] += 1
            if i % PER_THREAD == PER_THREAD - 1:
                ev[("start", "thread_last")] += 1
            edge = LOWER_EDGE_BYTES if kind == "lower" else UNKNOWN_BYTES
            if letters[g + i] in edge:
                ev[("is", kind, "first", int(letters[g + i]))] += 1
            if kind == "lower" and i > 0 and letters[g + i - 1] in edge:
                ev[("is", kind, "before", int(letters[g + i - 1]))] += 1
            e, steps = i + 1, 0
            while e + 8 <= L:
                if not all8(g + e, kind, ev):
                    ev[("walk", "stop8", "non_member")] += 1
                    break
                e += 8
                steps += 1
            else:
                ev[("walk", "stop8", "no_room")] += 1
            ev[("walk", "steps8", _cls(steps))] += 1
            while e < L:
                if letters[g + e] in edge:
                    ev[("is", kind, "walk", int(letters[g + e]))] += 1
                if not m[e]:
                    break
                e += 1
            if e - i >= min_mask or e == L:
                ev[("rule", "long" if e - i >= min_mask else "short_reaches_L")] += 1
                if e - i == min_mask:
                    ev[("rule", "exactly_min")] += 1
                out.append((c, i, e))
            else:
                ev[("rule", "short_dropped")] += 1
    return out


def restate(shape):
    """The builder in plain Python -> (one (n, 2) int32 array per contig, Counter of events)."""
    ev = Counter()
    seqs, n = shape.seqs, len(shape.seqs)
    base = bases_of(seqs)
    total = int(base[-1])
    nw = (total + WORD) // WORD
    nwv = (nw + 63) // 64
    letters = np.frombuffer(b"".join(seqs), np.uint8)
    bits = np.zeros(nw, np.uint32)
    cbits = np.zeros(nw, np.uint32)

    def paint_words(g0, g1, first, step):
        w0, w1 = g0 >> 5, (g1 - 1) >> 5
        for w in range(w0 + first, w1 + 1, step):
            m = 0xffffffff
            if w == w0:
                m &= (0xffffffff << (g0 & 31)) & 0xffffffff
            if w == w1:
                m &= 0xffffffff >> (31 - ((g1 - 1) & 31))
            bits[w] |= np.uint32(m)

    def paint_events(g0, g1):
        w0, w1 = g0 >> 5, (g1 - 1) >> 5
        ev[("paint", "same_word" if w0 == w1 else "next_word" if w1 == w0 + 1 else "far_word")] += 1
        ev[("paint", {0: "first_bit0", 31: "first_bit31"}.get(g0 & 31, "first_mid"))] += 1
        ev[("paint", {0: "last_bit0", 31: "last_bit31"}.get((g1 - 1) & 31, "last_mid"))] += 1

    def all8(at, kind, ev):
        chunk = letters[at:at + 8]
        if kind == "lower":
            ok = _all8_lower(int.from_bytes(chunk.tobytes(), "little"))
            inside = (chunk >= 97) & (chunk <= 122)
            assert ok == bool(inside.all())                                      # the byte tricks against the plain rule
            if int((~inside).sum()) <= 1:
                for lane, v in enumerate(chunk.tolist()):
                    if v in LOWER_EDGE_BYTES and (not inside[lane] or ok):
                        ev[("all8_lower", v, lane)] += 1
            return ok
        ok = bool((~mask_ref.KNOWN[chunk]).all())                                # eight digits of 6
        if ok:
            for lane, v in enumerate(chunk.tolist()):
                if v in UNKNOWN_BYTES:
                    ev[("all8_unknown", v, lane)] += 1
        return ok

    for kind, on, member in (("unknown", shape.mask, ~mask_ref.KNOWN[letters]), ("lower", shape.lower, (letters >= 97) & (letters <= 122))):
        if on:
            for c, b, e in _find_runs(seqs, base, member, all8, shape.min_mask, kind, ev, letters):
                paint_events(int(base[c]) + b, int(base[c]) + e)
                paint_words(int(base[c]) + b, int(base[c]) + e, 0, 1)
    for c, regs in enumerate(shape.regions or []):
        for b, e in regs or []:
            g0, g1 = int(base[c]) + max(int(b), 0), int(base[c]) + min(int(e), len(seqs[c]))
            if g0 >= g1:
                continue
            paint_events(g0, g1)
            W = ((g1 - 1) >> 5) - (g0 >> 5) + 1
            ev[("region_words", "1" if W == 1 else "2..63" if W < 64 else "64" if W == 64 else "65..127" if W < 128 else "128" if W == 128 else "129..")] += 1
            for lane in range(64):
                paint_words(g0, g1, lane, 64)
    for c in range(n):
        cbits[int(base[c]) >> 5] |= np.uint32(1 << (int(base[c]) & 31))

    # mask_edges over every word at once
    one, z = np.uint32(1), np.zeros(1, np.uint32)
    before = np.concatenate([z, bits[:-1] >> np.uint32(31)])
    after = np.concatenate([bits[1:] & one, z])
    c_after = np.concatenate([cbits[1:] & one, z])
    S = bits & (~((bits << one) | before) | cbits)
    E = bits & (~((bits >> one) | (after << np.uint32(31))) | ((cbits >> one) | (c_after << np.uint32(31))))
    low, top = (bits & one) != 0, (bits >> np.uint32(31)) != 0
    for bf in (0, 1):
        for cc in (0, 1):
            ev[("bit0", bf, cc)] += int((low & (before == bf) & ((cbits & one) == cc)).sum())
            ev[("bit31", bf, cc)] += int((top & (after == bf) & (c_after == cc)).sum())
    ev[("bit31_in_last_word",)] += int(top[-1])
    ev[("word0_set",)] += int(bits[0] != 0)
    ev[("last_word_set",)] += int(bits[-1] != 0)
    ev[("split_inside_word",)] += int(((bits & (bits << one) & cbits & ~one) != 0).sum())

    def bit(g):
        return int(bits[g >> 5] >> np.uint32(g & 31)) & 1 if g >= 0 else 0
    for c in range(n):
        g = int(base[c])
        if len(seqs[c]) and bit(g):
            ev[("first_base", bit(g - 1), int(cbits[g >> 5] >> np.uint32(g & 31)) & 1)] += 1

    # counts per group, the scan in rounds with a carry
    def popcount(a):
        return np.unpackbits(np.ascontiguousarray(a).view(np.uint8)).reshape(-1, 32).sum(axis=1).astype(np.int64)
    ps, pe = popcount(S), popcount(E)
    pad = nwv * 64 - nw
    cnt_s = np.concatenate([ps, np.zeros(pad, np.int64)]).reshape(nwv, 64).sum(axis=1)
    cnt_e = np.concatenate([pe, np.zeros(pad, np.int64)]).reshape(nwv, 64).sum(axis=1)
    for a, b in zip(cnt_s.tolist(), cnt_e.tolist()):
        ev[("group", "starts" if a else "no_start", "ends" if b else "no_end")] += 1
    off_s, off_e = np.zeros(nwv + 1, np.int64), np.zeros(nwv + 1, np.int64)
    carry_s = carry_e = 0
    for r in range(0, nwv, SCAN_ROUND):
        if r and carry_s != carry_e:
            ev[("scan", "carry_differs")] += 1
        for cnt, off, carry in ((cnt_s, off_s, carry_s), (cnt_e, off_e, carry_e)):
            chunk = cnt[r:r + SCAN_ROUND]
            off[r:r + len(chunk)] = carry + np.cumsum(chunk) - chunk
        carry_s += int(cnt_s[r:r + SCAN_ROUND].sum())
        carry_e += int(cnt_e[r:r + SCAN_ROUND].sum())
    off_s[nwv], off_e[nwv] = carry_s, carry_e
    ev[("scan", "one_round" if nwv <= SCAN_ROUND else "two_rounds")] += 1
    ev[("scan", "full_round")] += int(nwv == SCAN_ROUND)
    assert carry_s == carry_e

    # placement: the k-th start and the k-th end, independently
    def find_contig(g):
        lo, hi = 0, n - 1
        while lo < hi:
            mid = (lo + hi + 1) >> 1
            if base[mid] <= g:
                lo = mid
            else:
                hi = mid - 1
        return lo
    cap = cap_of(shape)
    ev[("cap", "half_binds" if cap == total // 2 + n + 1 else "sources_bind")] += 1
    begin, end = np.full(carry_s, -1, np.int64), np.full(carry_s, -1, np.int64)
    cs, ce = np.cumsum(ps) - ps, np.cumsum(pe) - pe          # starts before the word: the group's offset plus the lanes below
    for w in np.flatnonzero(S | E).tolist():
        grp = w >> 6
        ks = int(off_s[grp] + cs[w] - cs[grp * 64])
        ke = int(off_e[grp] + ce[w] - ce[grp * 64])
        for i in range(32):
            g = w * 32 + i
            if int(S[w]) >> i & 1:
                k = find_contig(g)
                ev[("find_contig", "equal_bases" if k > 0 and base[k - 1] == base[k] else "alone")] += 1
                if ks < cap:
                    begin[ks] = g - base[k]
                ks += 1
                if g % GROUP == GROUP - 1:
                    ev[("group_edge", "start_in_last_bit")] += 1
                if g % BLOCK == BLOCK - 1:
                    ev[("block_edge", "start_in_last_bit")] += 1
            if int(E[w]) >> i & 1:
                if ke < cap:
                    end[ke] = g + 1 - base[find_contig(g)]
                ke += 1
                if g % GROUP == 0:
                    ev[("group_edge", "end_in_first_bit")] += 1
                if g % BLOCK == 0:
                    ev[("block_edge", "end_in_first_bit")] += 1
    ev[("cap", "one_below")] += int(carry_s == cap - 1)
    ev[("cap", "full")] += int(carry_s == cap)
    ev[("cap", "exceeded")] += int(carry_s > cap)
    # the thread per contig, and the one for the end of the batch
    moff = []
    for c in range(n + 1):
        g = int(base[c])
        wg, grp = g >> 5, g // GROUP
        whole = int(ps[grp * 64:wg].sum())
        own = int(S[wg])
        part = bin(own & ((1 << (g & 31)) - 1)).count("1")
        moff.append(min(int(off_s[grp]) + whole + part, cap))
        if c == n:
            ev[("end_thread", "some" if moff[-1] else "none")] += 1
            continue
        ev[("contig_thread", _word_class(wg & 63), _cls(whole))] += 1
        ev[("partial_word", "bit0" if g & 31 == 0 else "above0", "some" if part else "none")] += 1
        if len(seqs[c]):
            ev[("own_word", "below")] += int(part > 0)
            ev[("own_word", "at")] += own >> (g & 31) & 1
            ev[("own_word", "above")] += int(own >> (g & 31) >> 1 != 0)
    lists = [np.stack([begin[moff[c]:moff[c + 1]], end[moff[c]:moff[c + 1]]], axis=1).astype(np.int32) for c in range(n)]
    gl = [(int(base[c] + b), int(base[c] + e)) for c, r in enumerate(lists) for b, e in r.tolist()]
    ev[("group_edge", "whole_group")] += sum(g0 % GROUP == 0 and g1 - g0 == GROUP for g0, g1 in gl)
    assert set(ev) <= set(EVENTS), sorted(set(ev) - set(EVENTS), key=str)
    return lists, ev
