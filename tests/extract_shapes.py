"""Contigs that put the front end -- k_digitize, the GC prefix, k_tile_stops, k_extract_tile / extract_strand, k_scan_counts,
k_place_nodes, k_group_enable -- at its length, frame, tile and end edges: the inputs of tests/test_extract_shapes_cpu.py and
tests/test_extract_shapes_gpu.py ("The front end at its edges").  A helper module, not a test.

Everything is deterministic and designed, not drawn: the background is a GCC repeat, which holds neither a stop nor a start codon on
either strand (any string of G and C does), so the only codons a contig holds are the ones a builder puts there, and the CPU test can
state EXACT populations from the oracle alone.  Every shape is designed in strand-local coordinates: strand 1 is the contig as
written, strand -1 its reverse complement, whose reverse strand then reads the design (position i of the design is ndx L - 1 - i)."""
from collections import namedtuple

import numpy as np

from tests.orf_shapes import START_CODONS, STOP_CODONS, revcomp  # noqa: F401  (the CPU test reads the codon sets from here)

TILE = 3072                    # positions of a workgroup of k_extract_tile (EX_TILE)
PER_THREAD = 12                # ... of one of its threads
WAVE = 64 * PER_THREAD         # ... of one of its wavefronts
HALF = 32 * PER_THREAD         # positions k_tile_stops decodes per round at either end of a tile
STAGE_SLACK = 8                # PGA_STAGE_SLACK
STOPS = b"TAACTAACTAA"         # a stop codon in each of the three frames
STOPS_RC = b"TTAGTTAGTTA"      # ... of the reverse strand
GENE_LENGTHS = ((90, 60), (120, 90))      # (min_gene, min_edge_gene): the defaults and one other pair
T_STOP = 3

# name, letters, strand of the design, region intervals (or None), what the design claims (a dict, read by the CPU test)
Shape = namedtuple("Shape", "name seq strand regions meta")
# a designed node: kind "start" / "stop", strand-local position, present on an open contig, present on a closed one
Node = namedtuple("Node", "kind at open closed")


def quiet(n):
    return (b"GCC" * (n // 3 + 1))[:n]


def contig(L, pieces):
    """L bases of background with `pieces` = [(position, letters)] written over it.  The letter before a piece becomes G: C before
    TAA / TAG would read CTA, a stop of the other strand, and C before ATG would read CAT, a start of the other strand."""
    s = bytearray(quiet(L))
    for at, text in pieces:
        assert 0 <= at and at + len(text) <= L, (at, len(text), L)
        s[at:at + len(text)] = text
        if at > 0 and s[at - 1] == ord("C"):
            s[at - 1] = ord("G")
    return bytes(s)


def sites(seq, strand, codons):
    """Strand-local positions at which one of `codons` begins."""
    s = bytes(seq).upper() if strand == 1 else revcomp(bytes(seq).upper())
    out = []
    for c in codons:
        k = s.find(c)
        while k >= 0:
            out.append(k)
            k = s.find(c, k + 1)
    return sorted(out)


def to_ndx(shape, at):
    """Forward coordinate of the design's position `at`."""
    return at if shape.strand == 1 else len(shape.seq) - 1 - at


def _both(name, design, meta, regions=None):
    """The design on the forward strand and, as the reverse complement of the whole contig, on the reverse strand."""
    L = len(design)
    rc_regions = None if regions is None else sorted((L - e, L - b) for b, e in regions)
    return [Shape(name + "/+", design, 1, regions, meta), Shape(name + "/-", revcomp(design), -1, rc_regions, meta)]


def virtual_stop(L, f):
    """Where the ORF of frame f ends on an open contig that holds no stop of the frame."""
    return L - 3 - ((L - 3 - f) % 3)


# ---- gene-length thresholds ------------------------------------------------------------------------------------------------------------

def length_series(min_gene, min_edge_gene):
    """`last - i + 3 >= min_gene` (inclusive) for an ORF between two stops, `>= min_edge_gene` for one that runs off the right end,
    `last - i > min_edge_gene` (strict) for the edge start of an ORF open at the left end; for all residues of L mod 3."""
    out = []
    for r in range(3):
        L = 600 + r
        for g in (min_gene - 3, min_gene, min_gene + 3):                  # between two stops: the only start codon g bases long
            i, ok = 201, g >= min_gene
            last = i + g - 3
            d = contig(L, [(i - 33, b"TAA"), (i, b"ATG"), (last, b"TAG")])
            out += _both("length/%d/L%d/closed_orf/%d" % (min_gene, r, g), d,
                         dict(nodes=[Node("start", i, ok, ok), Node("stop", last, ok, ok)], g=g, kind="closed_orf"))
        for f in range(3):
            for g in (min_edge_gene - 3, min_edge_gene, min_edge_gene + 3):      # off the right end
                last = virtual_stop(L, f)
                i, ok = last + 3 - g, g >= min_edge_gene
                d = contig(L, [(i - 33, b"TAA"), (i, b"ATG")])
                out += _both("length/%d/L%d/right_open/f%d/%d" % (min_gene, r, f, g), d,
                             dict(nodes=[Node("start", i, ok, False), Node("stop", last, ok, False)], g=g, kind="right_open"))
            for dist in (min_edge_gene - 3, min_edge_gene, min_edge_gene + 3):   # open at the left end, no start codon inside
                last, ok = f + dist, dist > min_edge_gene
                d = contig(L, [(last, b"TAA")])
                out += _both("length/%d/L%d/left_open/f%d/%d" % (min_gene, r, f, dist), d,
                             dict(nodes=[Node("start", f, ok, False), Node("stop", last, ok, False)], g=dist, kind="left_open"))
    return out


# ---- codons across ownership boundaries --------------------------------------------------------------------------------------------------

THREAD_TARGETS = tuple(PER_THREAD * 100 + q for q in range(PER_THREAD))          # every position of a thread
WAVE_TARGETS = (WAVE - 2, WAVE - 1, WAVE, WAVE + 1)                               # 766 .. 769
TILE_TARGETS = (TILE - 3, TILE - 2, TILE - 1, TILE, TILE + 1)                     # 3069 .. 3073
PHASE_TARGETS = THREAD_TARGETS + WAVE_TARGETS + TILE_TARGETS
PHASE_TAILS = (0, 1, 2, 11, 12, 13)                                               # L - 3072 k on the reverse strand


def phase_series():
    """One ORF -- far stop, one start codon at exactly min_gene (90), near stop -- slid so that its start codon, and separately its
    stop codon, has each of PHASE_TARGETS as its ndx.  A thread owns the same FORWARD positions on both strands, so the targets are
    forward coordinates; on the reverse strand the strand-local geometry (first position and frame of a tile) depends on L."""
    out = []
    for strand, lengths in ((1, (TILE + 300,)), (-1, tuple(2 * TILE + t for t in PHASE_TAILS))):
        for L in lengths:
            for kind in ("start", "stop"):
                for T in PHASE_TARGETS:
                    at = T if strand == 1 else L - 1 - T
                    i = at if kind == "start" else at - 87
                    d = contig(L, [(i - 30, b"TAA"), (i, b"ATG"), (i + 87, b"TAG")])
                    meta = dict(nodes=[Node("start", i, True, True), Node("stop", i + 87, True, True)], target=(kind, T), L=L)
                    out.append(Shape("phase/%s/%d/L%d/%s" % (kind, T, L, "+-"[strand < 0]), d if strand == 1 else revcomp(d), strand, None, meta))
    return out


LEFT_STOP_OFFSETS = ((0, "below"), (30, "below"), (84, "below"), (86, "below"),              # x = last + 3 - min_gene < lo
                     (87, "at"), (98, "at"), (99, "at"), (187, "at"))                          # x - lo = 0, 11, 12, 100
LEFT_START_CODONS = (1, 2, 30, 400)                                                           # codons left of the tile boundary


def left_of_tile_series():
    """last_start_codon: the stop lies `off` positions past the first position `lo` of its tile, the ORF's only start codon k codons
    left of the tile (answered by the codon-by-codon walk; from S.lsc of the neighbouring thread or straight from the walk, by
    whether x = last + 3 - min_gene reaches into the tile and whether the thread before x's exists).  "none": the only start codon
    lies left of the previous stop, so the ORF holds none and its stop is no node."""
    out = []
    for strand, lengths in ((1, (TILE + 400,)), (-1, (2 * TILE, 2 * TILE + 1, 2 * TILE + 2))):
        for L in lengths:
            lo = TILE if strand == 1 else L - TILE            # strand-local first position of the tile that holds the stop
            for off, where in LEFT_STOP_OFFSETS:
                last = lo + off
                below = last - 3 * ((last - lo) // 3 + 1)     # the frame's last position left of the tile
                for k in LEFT_START_CODONS + ("none",):
                    if k == "none":
                        i = below - 60
                        d, ok = contig(L, [(i - 30, b"TAA"), (i, b"ATG"), (i + 30, b"TAA"), (last, b"TAG")]), False
                    else:
                        i = below - 3 * (k - 1)
                        d, ok = contig(L, [(i - 30, b"TAA"), (i, b"ATG"), (last, b"TAG")]), last - i + 3 >= 90
                    meta = dict(nodes=[Node("start", i, ok, ok), Node("stop", last, ok, ok)], where=where, k=k, off=off, L=L)
                    out.append(Shape("left/%s%d/k%s/L%d/%s" % (where, off, k, L, "+-"[strand < 0]), d if strand == 1 else revcomp(d), strand, None, meta))
    return out


# ---- k_tile_stops and the tile carries ---------------------------------------------------------------------------------------------------

LONE_OFFSETS = tuple(sorted({0, 1, 2, TILE - 3} | set(range(HALF - 3, HALF + 3)) | set(range(2 * HALF - 3, 2 * HALF + 3))
                            | set(range(TILE - HALF - 2, TILE - HALF + 3))))
LAST_TILE_LENGTHS = (1, 2, 3, 12, 383, 384, 385, 767, 768, 769)


def _starts_at(base):
    """(position, ATG) in each of the three frames, twelve bases apart."""
    return [(base + 4 * k, b"ATG") for k in range(3)]


def lone_stop_series():
    """Three tiles without a stop except ONE, at offset p of the middle tile; start codons of every frame in the first and the last
    tile, a stop of every frame at the contig's end.  The frame of p sees its next / previous stop in the neighbouring tile, the
    other two frames see theirs two tiles away (carry_finish walks on, in both directions).  Then last tiles shorter than one and
    two rounds of k_tile_stops, and five tiles of which the middle three hold neither a stop nor a node."""
    out = []
    L = 3 * TILE
    for p in LONE_OFFSETS:
        d = contig(L, _starts_at(300) + _starts_at(1500) + _starts_at(2900) + [(TILE + p, b"TAG")] + _starts_at(2 * TILE + 500) + [(L - 11, STOPS)])
        out += _both("lone/p%d" % p, d, dict(p=p, lone=TILE + p))
    for n in LAST_TILE_LENGTHS:
        L = 2 * TILE + n
        d = contig(L, _starts_at(300) + [(TILE + 1000, b"TAG")] + _starts_at(TILE + 2000) + [(L - 11, STOPS)])
        out += _both("lone/last%d" % n, d, dict(last_tile=n))
    L = 5 * TILE
    d = contig(L, _starts_at(300) + _starts_at(2900) + _starts_at(4 * TILE + 500) + [(L - 11, STOPS)])
    out += _both("lone/five_tiles", d, dict(empty_tiles=(1, 2, 3)))
    return out


# ---- contig ends ---------------------------------------------------------------------------------------------------------------------------

END_LENGTHS = tuple(range(3, 21)) + tuple(range(87, 97))


def ends_series():
    """Contigs of 3 .. 20 and 87 .. 96 bases: bare, with a start codon at the edge-start position of a frame, with a stop codon at the
    frame's virtual stop, and with both."""
    out = []
    for L in END_LENGTHS:
        out += _both("ends/L%d/bare" % L, quiet(L), dict(L=L))
        for f in range(3):
            vs = virtual_stop(L, f)
            if f + 3 <= L:
                out += _both("ends/L%d/start%d" % (L, f), contig(L, [(f, b"ATG")]), dict(L=L, start=f))
            if vs >= 0:
                out += _both("ends/L%d/stop%d" % (L, f), contig(L, [(vs, b"TAA")]), dict(L=L, stop=vs))
            if f + 3 <= vs:
                out += _both("ends/L%d/both%d" % (L, f), contig(L, [(f, b"ATG"), (vs, b"TAA")]), dict(L=L, start=f, stop=vs))
    return out


NEIGHBOUR_ENDS = (b"T", b"TA", b"AT", b"TT")
NEIGHBOUR_BEGINS = (b"AA", b"A", b"G", b"GA")


def neighbour_series():
    """ONE batch, in this order: a contig whose ORF runs off its right end and which ends in T, TA, AT or TT, next to one that begins
    with AA, A, G or GA and whose first ORF is open at its left end -- a stop (TAA, TAG, TGA) or a start (ATG, TTG) would form across
    the boundary, in the frame of the ORF, if a read ignored it; then the mirror image of every pair."""
    out = []
    for e in NEIGHBOUR_ENDS:
        for b in NEIGHBOUR_BEGINS:
            left = b"TAAATG" + b"CCG" * 35 + e                   # the codon that begins at 111 is cut off by the end
            right = b + b"CCG" * 35 + b"TAGG" + b"CCG" * 10
            out += [left, right, revcomp(right), revcomp(left)]
    return out


# ---- unknown bases and named regions -----------------------------------------------------------------------------------------------------

_ORF_FAR, _ORF_START, _ORF_LAST, _ORF_L = 100, 220, 430, 600


def _one_orf():
    return bytearray(contig(_ORF_L, [(_ORF_FAR, b"TAA"), (_ORF_START, b"ATG"), (_ORF_LAST, b"TAG")]))


def unknown_series(min_mask):
    """One ORF (far stop 100, start 220, stop 430) with one N at each base of its start codon and of either stop codon and one inside
    it; and with a run of min_mask - 1, min_mask, min_mask + 1 unknown bases that ends 0, 1 or 3 bases before the start codon or
    begins 0, 1 or 3 bases after it."""
    out = []

    def add(name, at, n):
        d = _one_orf()
        d[at:at + n] = b"N" * n
        out.extend(_both("unknown/%d/%s" % (min_mask, name), bytes(d), dict(run=(at, at + n))))
    for k in range(3):
        add("start%d" % k, _ORF_START + k, 1)
        add("far%d" % k, _ORF_FAR + k, 1)
        add("near%d" % k, _ORF_LAST + k, 1)
    add("inside", _ORF_START + 31, 1)
    for m in (min_mask - 1, min_mask, min_mask + 1):
        if m < 1:
            continue
        for gap in (0, 1, 3):
            add("before/m%d/gap%d" % (m, gap), _ORF_START - gap - m, m)
            add("after/m%d/gap%d" % (m, gap), _ORF_START + 3 + gap, m)
    return out


def region_series():
    """Named intervals over the REAL bases of the one ORF [i, last] = [220, 430]: one that ends at i, i + 1, last,
    last + 1; one that begins at last - 1, last, last + 1; and the boundary case -- a region over the start codon, hidden by a
    second one that begins exactly at the stop ("two"), next to the first region alone ("one").  The reverse strand's mask test is
    the forward one moved by a base (it compares forward coordinates of the codons' LAST bases), so the design is moved with it
    (shift 1); the unmoved mirror images are in the series too (shift 0)."""
    i, last = _ORF_START, _ORF_LAST
    cases = [("end_at_i", [(i - 15, i)], True), ("end_at_i+1", [(i - 15, i + 1)], False), ("end_at_last", [(last - 15, last)], False),
             ("end_at_last+1", [(last - 15, last + 1)], False), ("begin_at_last-1", [(last - 1, last + 20)], False),
             ("begin_at_last", [(last, last + 20)], True), ("begin_at_last+1", [(last + 1, last + 20)], True),
             ("one", [(i - 5, i + 10)], False), ("two", [(i - 5, i + 10), (last, last + 20)], True)]
    d = bytes(_one_orf())
    out = []
    for name, iv, present in cases:
        meta = dict(nodes=[Node("start", i, present, present), Node("stop", last, present, present)], case=name)
        out.append(Shape("region/%s/+" % name, d, 1, iv, meta))
        for shift in (1, 0):
            rc = sorted((_ORF_L - e - shift, _ORF_L - b - shift) for b, e in iv)
            out.append(Shape("region/%s/-%d" % (name, shift), revcomp(d), -1, rc, meta if shift else dict(case=name)))
    return out


def lower_cased(shape):
    """The letters of a region shape with its intervals in lower case: under mask_lowercase and min_mask 1 the same mask list."""
    s = bytearray(shape.seq)
    for b, e in shape.regions:
        s[b:e] = bytes(s[b:e]).lower()
    return bytes(s)


# ---- digitise --------------------------------------------------------------------------------------------------------------------------------

DIGITISE_PIECES = (1024, 4096, 16384)             # a wavefront's piece, a block's quarter, a block of k_digitize
ALPHABET = bytes(range(256))                      # the oracle reads every byte: ACGT in either case, anything else as unknown


def digitise_series():
    """Two orderings of one set of contigs.  The first puts a contig boundary at every residue mod 16 and one within 16 bases on
    either side of a multiple of 1024, 4096 and 16 384 (a 16-byte piece with a boundary inside goes base by base; counts are held
    back per wavefront and contig); lengths 0 .. 40 and around the three piece sizes; letters from all 256 byte values, with ACGT
    of either case and the IUPAC letters more often than the rest; 40 000 bases of G alone and of N alone."""
    rng = np.random.default_rng(20250101)
    common = np.frombuffer(b"ACGTacgtACGTacgtRYKMSWBDHVNrykmswbdhvn-*", np.uint8)

    def letters(n):
        a = common[rng.integers(0, len(common), n)].copy()
        rare = rng.random(n) < 0.05
        a[rare] = rng.integers(0, 256, int(rare.sum()), dtype=np.uint8)
        return a.tobytes()
    seqs = [letters(n) for n in range(41)]
    at = sum(range(41))
    for piece in DIGITISE_PIECES:                  # a boundary at piece - 1 and one at piece + 1
        seqs += [letters(piece - 1 - at), letters(2)]
        at = piece + 1
    for piece in DIGITISE_PIECES:
        seqs += [letters(piece + d) for d in (-17, -1, 0, 1, 17)]
    seqs += [b"G" * 40000, letters(7), b"N" * 40000, letters(23), ALPHABET, ALPHABET[::-1]]
    order = [int(k) for k in np.random.default_rng(20250102).permutation(len(seqs))]
    return seqs, [seqs[k] for k in order]


def boundaries(seqs):
    """Batch positions at which a contig begins or the batch ends."""
    return np.cumsum([0] + [len(s) for s in seqs])


# ---- many tiles, full staging ------------------------------------------------------------------------------------------------------------

TILE_COUNTS = (4095, 4096, 4097, 8193)            # k_scan_counts works in rounds of 4096 counts with a carry


def n_tiles(seqs):
    return sum((len(s) + TILE - 1) // TILE for s in seqs)


def tile_count_series():
    """{tile count: batch} of contigs of 100 .. 200 bases, one tile each, drawn in turn from 101 distinct ones that hold a node or
    more (an ORF off the left end and its stop)."""
    kinds = [contig(100 + k, [(7 + k % 3, b"ATG"), (70 + k % 3 + 3 * (k % 7), b"TAA")]) for k in range(101)]
    return {n: [kinds[(j * 37 + n) % 101] for j in range(n)] for n in TILE_COUNTS}


def tile_node_counts(nodes, L):
    """Nodes per tile of a contig of L bases, from the oracle's nodes."""
    return np.bincount(nodes["ndx"].astype(np.int64) // TILE, minlength=(L + TILE - 1) // TILE)


def room(tile_len, shift):
    """Staging slots of a tile under one slot per 2^shift positions (k_extract_tile)."""
    return (tile_len >> shift) + STAGE_SLACK


def dense_tail(n, tail):
    """A tile of background, then STOPS_RC + (GT)n + STOPS and `tail` bases: a GTG start at every second position of the run."""
    return quiet(TILE) + STOPS_RC + b"GT" * n + STOPS + quiet(tail)


STAGING_SHIFT = 2
PLACE_COUNTS = (128, 129, 256, 257)               # k_place_nodes works in rounds of 128 nodes


def staging_series(count_nodes):
    """{name: contig}.  "room-1", "room", "room+1": the contig's last tile holds exactly that many nodes, with room the tile's staging
    slots at PGA_STAGE_SHIFT = 2.  (At the default shift of 1 no sequence reaches room: a start node needs the two letters TG after
    it or the two letters CA before it to itself, so a tile of n positions holds n / 2 of them, stop nodes lie a gene length apart,
    and the six edge nodes of an open end are what the slack of 8 is for; the densest last tile found holds room - 3.)  "place128"
    .. "place257": its last tile holds that many.  "edge3": an open contig whose last tile is three bases long and holds four edge
    nodes.  `count_nodes(seq)`: nodes per tile of an open contig under table 11 (the oracle's: tile_node_counts)."""
    out = {}
    want = {"room-1": -1, "room": 0, "room+1": 1}
    for tail in range(0, 40):
        for n in range(90, 130):
            s = dense_tail(n, tail)
            d = int(count_nodes(s)[1]) - room(len(s) - TILE, STAGING_SHIFT)
            for name, delta in want.items():
                if d == delta and name not in out:
                    out[name] = s
        if len(out) == 3:
            break
    for c in PLACE_COUNTS:
        for n in range(c - 20, c + 80):
            s = dense_tail(n, 30)
            if int(count_nodes(s)[1]) == c:
                out["place%d" % c] = s
                break
    out["edge3"] = contig(TILE + 3, _starts_at(300))
    return out


# ---- the GC window of meta mode --------------------------------------------------------------------------------------------------------------

def gc_window_table():
    """[(name, contig, low, high)]: 12 kb of a genome (its genes are called whatever GC value the model carries) whose window
    (tests/sets_ref.py: window) has neither bound clamped; the same with G + C filler behind it, `low` clamped at 0.65; and with
    A + T filler, `high` clamped at 0.35.  The model to call them with is gc_window_model()."""
    from tests import sets_ref
    from tests.util import read_fasta
    real = read_fasta("GCF_001457455.1_NCTC11397_genomic_100kb.fna.gz")[0][1].upper().encode()[:12000] + STOPS
    out = []
    for name, filler in (("unclamped", b""), ("low_clamped", quiet(14500)), ("high_clamped", b"AT" * 7400)):
        seq = real + filler
        low, high = sets_ref.window(sets_ref.gc_count(seq) / len(seq))
        out.append((name, seq, low, high))
    return out


def gc_window_model():
    from oracle import oracle as orc
    from tests.util import golden_path
    return orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz"))


def gc_window_values(low, high):
    """[(model GC, is the model kept)]: each bound, the double below it and the double above it -- k_group_enable keeps a model
    iff !(gc < low || gc > high)."""
    import math
    return [(low, True), (math.nextafter(low, -1.0), False), (math.nextafter(low, 1.0), True),
            (high, True), (math.nextafter(high, -1.0), True), (math.nextafter(high, 2.0), False)]
