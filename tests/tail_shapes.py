"""Deterministic inputs that put the traceback tail (pyrodigal_amd/csrc/tail.inl over the rules of tail_rules.h) at its
edges: the inputs of tests/test_tail_cpu.py, which proves with tests/tail_ref.py what they contain, and of
tests/test_tail_shapes_gpu.py, which compares the device on them.  A helper module, not a test.

Sources: the genome fixture and its reverse complement, sliced; planted_genome of tests/golden/make_models.py; synthetic contigs;
the fixture models, the meta model set, and the NCTC11397 model with other start-type weights, under which five times as many
starts move.  The slice coordinates below were found with the search tools of this module (cut_before_gene, place_gene,
find_cut) and are kept as constants, so that a test run only has to check them."""
import functools
import importlib.util
import os

from oracle import oracle as orc
from tests import dp_inject
from tests import tail_ref
from tests.orf_shapes import revcomp
from tests.util import golden_path, read_fasta, synthetic_contig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENOME = "GCF_001457455.1_NCTC11397_genomic.fna.gz"
MODEL = "GCF_001457455.1_NCTC11397_genomic.tinf_closed.bin.gz"
MAX_OVERLAPS = (30, 60, 200)
MIN_GENE = {30: 90, 60: 90, 200: 200}          # the shortest gene that goes with an overlap: the finder refuses max_overlap > min_gene (ref: lib.pyx:5169-5181)
ONE_GENE = b"ATG" + b"GCA" * 60 + b"TAA"
DEGENERATE = (b"", b"ACGT", b"N" * 500, ONE_GENE)          # empty, without nodes, edge nodes but no gene, one gene


@functools.lru_cache(maxsize=None)
def genome(strand=1):
    g = read_fasta(GENOME)[0][1].encode()
    return g if strand == 1 else revcomp(g)


@functools.lru_cache(maxsize=None)
def planted(length, gc, seed):
    spec = importlib.util.spec_from_file_location("make_models", os.path.join(ROOT, "tests", "golden", "make_models.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return bytes(mod.planted_genome(length, gc, seed))


def nctc():
    return orc.Training.load(golden_path(MODEL))


def altered(type_wt, st_wt):
    """The NCTC11397 model with other start-type weights and another start weight."""
    t = nctc()
    t.type_wt[:] = type_wt
    t._f64(16)[0] = st_wt
    return t


ALTERED = tuple((tw, st) for tw in ((-3.0, 1.0, 2.0), (-6.0, 3.0, 3.0)) for st in (1.0, 0.5))
TWEAK_MODEL = ((-6.0, 3.0, 3.0), 1.0)


def meta_models():
    from pyrodigal_amd import benchdata
    return [orc.Training(b) for _, b in benchdata.load_model_set()]


# ---- tools ------------------------------------------------------------------------------------------------------------------------------

def cut_before_gene(genes, k, step=7):
    """Candidate left cuts that make gene k of a contig its first gene: the bases in front of its begin, then those inside the gene
    before it (a cut there leaves that gene too short to be called or turns it into an edge gene; the caller checks)."""
    prev_end = int(genes["end"][k - 1]) if k > 0 else 0
    b = int(genes["begin"][k])
    return list(range(b - 3, max(prev_end, b - 400), -step)) + list(range(prev_end, max(0, prev_end - 300), -(step + 4)))


def place_gene(seq, tinf, want, max_overlap=60, closed=False):
    """`seq` trimmed from the left by whole genes so that the last gene whose in-order tweak differs from the parallel one has index
    `want`: (offset of the cut, result of tail_ref.run on the trimmed contig), or None.  Trimming shifts a gene's index and with
    it its place in the fix-up's 64-gene windows."""
    big = tail_ref.run(seq, tinf, closed=closed, max_overlap=max_overlap)
    if not big["differs"] or big["differs"][-1] < want:
        return None
    for cut in cut_before_gene(big["final"], big["differs"][-1] - want):
        r = tail_ref.run(seq[cut:], tinf, closed=closed, max_overlap=max_overlap)
        if r["differs"] and r["differs"][-1] == want:
            return cut, r
    return None


# ---- splices: five slices of the genome of some 3 000 nodes, each around a triple overlap -------------------------------------------------
# Together (open ends, the NCTC11397 model): 7 triple overlaps, 7 reverse start -> forward stop, 26 forward stop -> forward stop,
# 17 reverse stop -> reverse stop, splices on adjacent path edges in every slice, one on the first edge from the best gene end
# (slice 0) and one on the edge into the head of the path (slice 2).
SPLICE_SLICES = ((69105, 119105), (350563, 400563), (375067, 425067), (1462014, 1512014), (1738999, 1788999))


def splice_series():
    return [genome()[a:b] for a, b in SPLICE_SLICES]


# ---- elimination: thirty-one 20 kbp contigs of random sequence in meta mode --------------------------------------------------------------------
# The last one also serves mark_reset_series below.
def elimination_series():
    return [synthetic_contig(20000, 0.5, 4000 + k) for k in range(30)] + [synthetic_contig(20000, 0.3 + 0.4 * 16 / 40, 4057)]


# ---- a triple overlap whose spliced-in reverse stop has an ov_mark to reset ----------------------------------------------------------------
# Two of 300 random contigs (GC 0.30 .. 0.70) under model 7 of the meta set hold one; under the NCTC11397 model none of 1 200 does, and
# none of the 934 triple overlaps of the genome and its reverse complement.  Single mode: in meta mode the nodes a call returns are
# extracted and scored again after the tail, so the tail's ov_mark cannot be seen there.
MARK_RESET_MODEL = 7


def mark_reset_series():
    return [synthetic_contig(20000, 0.3 + 0.4 * 16 / 40, 4057), synthetic_contig(20000, 0.3 + 0.4 * 37 / 40, 4283)]


# ---- gene list: paths longer than a wave, a round and a chunk -------------------------------------------------------------------------------
# name: (contig, nodes with open ends, the unit its path is longer than, the form of the gene list that meets it)
GENE_LIST = {
    "wave": (lambda: planted(60000, 0.30, 11), 1567, 64, "k_tp_small, 64 threads"),
    "round": (lambda: planted(400000, 0.22, 21)[:204409], 4096, 256, "k_tp_small, 256 threads"),
    "steps": (lambda: genome()[:200000], 13419, 256, "k_tp_extract, 256 threads"),
    "chunk": (lambda: genome()[840000:1440000], 33954, 1024, "k_tp_extract_sum / _chunk; k_tp_extract with 1024 threads"),
}


def minus_one_gene(seq, tinf, closed=False):
    """`seq` without its first gene (cut three bases in front of its second gene's begin)."""
    o = orc.Oracle(seq)
    o.find_genes_single(tinf, orc.Params(closed=closed))
    return seq[int(o.genes()["begin"][1]) - 4:]


# ---- start tweaks: the gene whose in-order result differs from the parallel one, at every place of a 64-gene window -----------------------
# Reverse complement of the genome, model TWEAK_MODEL.  The gene's start lies near TWEAK_AT; every slice ends TWEAK_AT + 4000.
TWEAK_AT = 526534
TWEAK_LEFT = {                      # name: (left end of the slice, index of the differing gene)
    "short": (TWEAK_AT - 4000, 5),
    "mid": (TWEAK_AT - 30000, 31),
    "last_of_first_window": (462027, 64),      # index = 0 (mod 64): the last gene of its window, redone behind gene 63
    "first_of_window": (460417, 65),           # index = 1 (mod 64): its predecessor is the window before's last gene
    "interior": (452578, 70),
    "last_of_window": (401546, 128),
}


def tweak_contig(name):
    return genome(-1)[TWEAK_LEFT[name][0]:TWEAK_AT + 4000]


def tweak_series():
    return [tweak_contig(k) for k in TWEAK_LEFT]


# ---- launch edges: contigs of an exact node count (open ends, translation table 11) ---------------------------------------------------------
NODE_CUTS = {                       # nodes: (strand, first base, length)
    2048: (1, 100000, 28273), 2049: (1, 0, 30545), 4096: (1, 0, 61735), 4097: (1, 0, 61749),
    32767: (1, 0, 497217), 32768: (1, 0, 497252),
}
# a slice of 32 768 nodes of the reverse complement that holds the differing gene of the tweak series
LONG_TWEAK = (-1, TWEAK_AT - 250000, 509898)
# the same for genes of at least 200 bases (max_overlap = 200): 33 022 nodes, the differing gene is gene 432
LONG_TWEAK_200 = (-1, TWEAK_AT - 500000, 1040000)


def cut(strand, first, length):
    return genome(strand)[first:first + length]


def with_nodes(n):
    return cut(*NODE_CUTS[n])


def find_cut(strand, first, n, span):
    """The length at which the genome from `first` holds exactly n nodes (how NODE_CUTS was made)."""
    s = dp_inject.trimmed_to_nodes(genome(strand)[first:first + span], n)
    return None if s is None else len(s)


def companions(k, seed=5000):
    """k short contigs (1.5 .. 4 kbp, mixed GC) with the degenerate ones spread among them."""
    out = [synthetic_contig(1500 + 83 * (j % 31), 0.35 + 0.3 * (j % 17) / 16, seed + j) for j in range(k)]
    for j, d in enumerate(DEGENERATE):
        if k > len(DEGENERATE):
            out[(j * k) // len(DEGENERATE)] = d
    return out


def repeated(k, distinct=12, seed=5100):
    """k contigs made of repeats of `distinct` short ones and the degenerate ones: the oracle runs once per distinct contig."""
    base = [synthetic_contig(1200 + 211 * j, 0.4 + 0.02 * j, seed + j) for j in range(distinct)] + list(DEGENERATE)
    return [base[(7 * j) % len(base)] for j in range(k)]
