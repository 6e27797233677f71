"""Contigs whose ORFs have a prescribed stop-to-stop span and start nodes at prescribed codons: the inputs of
tests/test_coding_score_cpu.py and tests/test_coding_score_gpu.py.  A helper module, not a test.

Codons are counted as the coding-score kernels count them (orf_codons in pyrodigal_amd/csrc/pipeline.hip): from the ORF's stop
node outwards, x(ci) = p + step * (ci + 1), ci = 0 .. ncod - 1."""
import numpy as np

from tests.util import synthetic_contig

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
START_CODONS = (b"ATG", b"GTG", b"TTG")
STOP_CODONS = (b"TAA", b"TAG", b"TGA")
T_STOP = 3                                  # node type of a stop node (0 .. 2: ATG, GTG, TTG)

# the length classes of k_coding_score_quads are cut above these spans (the last one is the default of PGA_CS_WAVE) ...
CLASS_EDGES = (16, 32, 48, 64, 96, 128, 192, 256, 384, 512, 2048)
# ... so the designed contig holds every edge, the span one beyond it, the rounds of 16 and 64 codons and the 1000-codon switch of
# the length factor
SPANS = tuple(sorted({s for e in CLASS_EDGES for s in (e, e + 1)}
                     | {31, 63, 65, 127, 255, 257, 998, 999, 1000, 1001, 1023, 1024, 1025, 2047, 2111, 2112, 2113, 3000}))
SHORT_SPANS = (15, 16, 17, 18, 31, 32, 33)  # scored with min_gene = min_edge_gene = 45
SHORT_MIN_GENE = 45
_PLANTED = (29, 30, 31, 32, 47, 48, 63, 64, 65, 79, 80, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512,
            997, 998, 999, 1000, 1023, 1024, 2047, 2048, 2049)


def revcomp(seq):
    return bytes(seq).translate(_COMP)[::-1]


def planted_starts(ncod):
    """Start codons of an ORF of `ncod` codons: at the boundaries of the walks' rounds and masks, and at its outer end."""
    far = (ncod - 17, ncod - 16, ncod - 15, ncod - 2, ncod - 1)
    return sorted({ci for ci in _PLANTED + far if 0 <= ci < ncod})


def outer_starts(ncod):
    """The outermost three codons."""
    return [ci for ci in (ncod - 3, ncod - 2, ncod - 1) if ci >= 0]


def _bases(n, rng, gc):
    p = [(1 - gc) / 2, gc / 2, gc / 2, (1 - gc) / 2]
    return rng.choice(4, size=n, p=p)


def _sense_codons(n, rng, gc):
    """n codons that are neither a stop nor a start codon, as an (n, 3) array of indices into ACGT."""
    bad = {tuple(b"ACGT".index(c) for c in cod) for cod in START_CODONS + STOP_CODONS}
    out = _bases(3 * n, rng, gc).reshape(n, 3)
    while True:
        redo = [k for k in range(n) if tuple(out[k]) in bad]
        if not redo:
            return out
        out[redo] = _bases(3 * len(redo), rng, gc).reshape(len(redo), 3)


def orf(ncod, starts, rng, gc=0.5):
    """One forward ORF as text: the far stop, the codons ci = ncod - 1 .. 0, the near stop (the one its stop node sits on).  Codon ci
    is a start codon (ATG, GTG, TTG in turn) where ci is in `starts` and a sense codon that is no start codon everywhere else."""
    cod = _ACGT[_sense_codons(ncod, rng, gc)]
    text = [bytes(cod[ncod - 1 - k]) for k in range(ncod)]           # in reading order: the outermost codon first
    for t, ci in enumerate(sorted(starts)):
        assert 0 <= ci < ncod
        text[ncod - 1 - ci] = START_CODONS[t % 3]
    far, near = (STOP_CODONS[int(k)] for k in rng.integers(0, 3, 2))
    return far + b"".join(text) + near


def designed_contig(spans, rng, gc=0.5, layout=False):
    """ORFs of the given spans -- an entry is `ncod` (start codons where planted_starts puts them) or `(ncod, starts)` -- with 0, 1
    or 2 filler bases between them, followed by the reverse complement of the whole: every shape exists on both strands, in all
    frames and at all residues of a position mod 16.  With `layout` also [(position of the stop node, strand, ncod, starts)]."""
    parts, at, placed = [], 0, []
    for k, sp in enumerate(spans):
        ncod, starts = (int(sp), planted_starts(int(sp))) if np.isscalar(sp) else (int(sp[0]), sorted(sp[1]))
        parts.append(bytes(_ACGT[_bases(k % 3, rng, gc)]))
        parts.append(orf(ncod, starts, rng, gc))
        at += len(parts[-2]) + len(parts[-1])
        placed.append((at - 3, ncod, starts))
    half = b"".join(parts)
    seq = half + revcomp(half)
    if not layout:
        return seq
    return seq, [(p, 1, n, st) for p, n, st in placed] + [(len(seq) - 1 - p, -1, n, st) for p, n, st in placed]


def designed(gc=0.5, spans=SPANS, seed=20240611, layout=False):
    return designed_contig(spans, np.random.default_rng(seed), gc, layout)


def designed_short_edges(gc=0.5, seed=20240612, layout=False):
    """Spans around 16 and 32 codons with start codons at their outermost three codons."""
    return designed_contig([(n, outer_starts(n)) for n in SHORT_SPANS], np.random.default_rng(seed), gc, layout)


def end_contig(ncod, inside, strand, seed, gc=0.5, tail=240):
    """A contig whose first ORF runs off its left end (strand 1): no far stop, its outermost codon `inside` bases after the
    contig's first base (what precedes it continues the ORF); then its near stop and `tail` random bases.  strand -1: the mirror
    image, a reverse ORF that runs off the right end."""
    rng = np.random.default_rng(seed)
    text = orf(ncod + 6, planted_starts(ncod), rng, gc)[3:]          # without the far stop
    s = text[18 - inside:] + synthetic_contig(tail, gc, seed + 1)
    return s if strand == 1 else revcomp(s)


def orf_codons(p, q, strand, L):
    """The span rule of the kernels (orf_codons) for one stop node at p with far end q."""
    if strand == 1:
        lowb = max(q + 1, 0)
        xmin = lowb + (p - lowb) % 3
        return (p - 3 - xmin) // 3 + 1 if xmin <= p - 3 else 0
    highb = min(q - 1, L - 1)
    xmax = highb - (highb - p) % 3
    return (xmax - (p + 3)) // 3 + 1 if xmax >= p + 3 else 0


def orf_spans(nodes, L):
    """(indices of the stop nodes, their stop-to-stop spans in codons, their strands) of oracle node arrays of a contig of L bases."""
    idx = np.flatnonzero(nodes["type"] == T_STOP)
    spans = np.asarray([orf_codons(int(nodes["ndx"][i]), int(nodes["stop_val"][i]), int(nodes["strand"][i]), L) for i in idx], np.int64)
    return idx, spans, nodes["strand"][idx].astype(np.int64)


def start_codons_of(nodes, L, i):
    """{ci: node index} of the start nodes of the ORF of stop node i."""
    p, strand = int(nodes["ndx"][i]), int(nodes["strand"][i])
    mine = np.flatnonzero((nodes["type"] != T_STOP) & (nodes["strand"] == strand) & (nodes["stop_val"] == p))
    return {abs(int(nodes["ndx"][k]) - p) // 3 - 1: int(k) for k in mine}


# ---- several models: the table columns of k_coding_score_quads --------------------------------------------------------------------------

GC_SPANS = (65, 257, 513, 1001, 2049)
MODEL_SET_SIZES = (1, 2, 3, 4, 5, 7, 9, (4, 2))      # (4, 2): four models of table 11 and two of table 4
# the model meant to win on the GC 0.5 contig, by its place among the window's models: columns 0 .. 3 of the quads m0 = 0, 4 and 8
_WINNER_SLOT = {1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 7: 5, 9: 8, (4, 2): 2}


def model_contigs():
    """The designed contig at GC 0.5 and two smaller ones at GC 0.35 and 0.65: their GC windows are disjoint, so they use
    different table columns in one launch."""
    return [designed(), designed(0.35, GC_SPANS, 20240613), designed(0.65, GC_SPANS, 20240614)]


def model_set(size):
    """One model for the GC 0.35 contig, two for the GC 0.65 contig, then `size` models that all lie in the window of the GC 0.5
    contig: with the window's models last in the table, that contig's quads are the columns 3 .. 3 + size - 1 and its last quad
    is partly empty, for sizes 1, 5 and 9 past the end of the table (whose stride is the number of models rounded up to even).
    Copies of the fixture models with other GC values; the strongest source sits where _WINNER_SLOT says."""
    from tests.circular_ref import meta_bins
    pool = [b for b in meta_bins() if b.trans_table == 11]

    def made(src, gc, tt=11):
        t = pool[src].copy(); t.set_gc(gc); t.set_trans_table(tt)
        return t
    n11, n4 = size if isinstance(size, tuple) else (size, 0)
    out = [made(2, 0.36), made(9, 0.60), made(10, 0.66)]
    w = _WINNER_SLOT[size]
    out += [made(0 if j == w else 7 + (j * 3) % 5, 0.45 + 0.0125 * ((j - w) % n11)) for j in range(n11)]
    out += [made(6 + j, 0.47 + 0.04 * j, 4) for j in range(n4)]
    return out
