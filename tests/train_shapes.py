"""Genomes that reach the training's kernels (pyrodigal_amd/csrc/train.inl) at their sequence, ORF and batch edges: the inputs of
tests/test_train_cpu.py and tests/test_train_shapes_gpu.py.  A helper module, not a test.  Everything is deterministic; every
series exists on the forward strand (side 1) and, as the reverse complement of the whole genome, on the reverse strand (side -1).
Genomes are as small as their rule allows: the oracle trains each in milliseconds and the device takes a batch of them per call."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

from oracle import oracle as orc
from tests import start_shapes
from tests.orf_shapes import _ACGT, _sense_codons, revcomp
from tests.util import synthetic_contig

# opts: the keyword arguments of Context.train that differ from its defaults (translation_table, start_weight, force_nonsd are per
# genome in a batch; closed, min_gene and mask belong to the call)
Genome = namedtuple("Genome", "tag side seq opts")
SIDES = (1, -1)


def _planted(length, gc, seed):
    from pyrodigal_amd import benchdata
    return benchdata.planted_contig(length, gc, seed)


def _both(tag, seq, **opts):
    return [Genome(tag, 1, seq, opts), Genome(tag, -1, revcomp(seq), opts)]


def _codons(n, seed, gc=0.5):
    return bytes(_ACGT[_sense_codons(n, np.random.default_rng(seed), gc)].reshape(-1))


# Seven sense codons that put a stop codon into each of the five other frames (TAA twice on this strand, TAG and twice TAA on the
# other): repeated, they make an ORF with no other ORF inside it on either strand, and no start codon but the one before it.
CLEAN_UNIT = b"CTAACTAAGGTTACCGCTTAC"


def _clean_orf(units):
    return b"ATG" + CLEAN_UNIT * units + b"TAA"


def n_nodes(seq, tt=11, closed=False, min_gene=90):
    o = orc.Oracle(seq)
    return o.extract(tt, orc.Params(closed=closed, min_gene=min_gene))


# ---- length_series ----------------------------------------------------------------------------------------------------------------
LENGTHS_SHORT = tuple(range(90, 131)) + tuple(range(197, 204))          # the 120-base window cut at both ends, every L mod 3
LENGTHS_3K = (2999, 3000, 3001)
BEYOND_LAST_STOP = (6, 7, 8)                                              # L minus the position of the last stop codon


def short_genome(L):
    """Ten bases, ATG, 34 sense codons, TAA, random bases, cut to L: an ORF open at the end below 118 bases, whole from 118."""
    return (synthetic_contig(10, 0.5, 8100) + b"ATG" + _codons(34, 8101, 0.6) + b"TAA" + synthetic_contig(100, 0.55, 8102))[:L]


def length_series():
    out = []
    for L in LENGTHS_SHORT:
        out += _both(("length", L), short_genome(L))
    for L in LENGTHS_3K:
        out += _both(("length", L), _planted(L, 0.5, 8110))
    for k in BEYOND_LAST_STOP:                                             # ... ATG <ORF> TAA and k - 3 bases: hexamers up to L - 6
        body = _planted(600, 0.5, 8120) + b"ATG" + _codons(60, 8121) + b"TAA"
        out += _both(("beyond", k), body + b"CGC"[:k - 3])
    return out


# ---- end_series -------------------------------------------------------------------------------------------------------------------
END_KINDS = ("sd", "mot")
DOWNSTREAM = tuple(range(0, 6))                                            # bases between the stop codon and the end of the genome


def end_genome(kind, u):
    """u upstream bases, an ORF of 301 sense codons with one start and nothing else inside it, a short tail: the start that the
    training counts upstream of is the planted one."""
    return start_shapes.end_upstream(kind, u) + _clean_orf(43) + synthetic_contig(60, 0.5, 8270 + u)


def end_series():
    """A long ORF (300 sense codons) whose start lies u bases from the upstream end of the genome (start_shapes.END_U: every cut of
    the two upstream windows and of the motif search), under an SD and a motif seed; the same ORF with its stop 0 .. 5 bases from the
    downstream end; and open at the downstream end."""
    out = []
    for kind in END_KINDS:
        for u in start_shapes.END_U:
            out += _both(("end_up", kind, u), end_genome(kind, u))
    head = _planted(500, 0.5, 8200) + b"TAA" + start_shapes._SD_UPSTREAM[-20:]
    orf = _clean_orf(43)[:-3]
    for k in DOWNSTREAM:
        out += _both(("end_down", k), head + orf + b"TAA" + b"CGCGC"[:k])
    out += _both(("end_open",), head + orf)
    out += _both(("end_open",), head + orf + b"C")
    out += _both(("end_open",), head + orf + b"CG")
    return out


# ---- threshold_series -------------------------------------------------------------------------------------------------------------
NODE_TARGETS = (1998, 1999, 2000, 2001, 2002)


def many_starts(reps):
    """One forward ORF with a start codon every six bases and no other ORF on either strand (with closed ends): ATGCTA repeated reads
    TGCTAA in the next frame and TAGCAT on the other strand.  One confident ORF, about `reps` nodes."""
    return b"TAA" + b"ATGCTA" * reps + b"TAAC"


@lru_cache(maxsize=None)
def many_starts_with_nodes(target):
    for reps in range(target - 10, target + 40):
        if n_nodes(many_starts(reps), closed=True) == target:
            return many_starts(reps)
    raise AssertionError("no repeat count gives %d nodes" % target)


# the halving at equality with a consequence: next to the one confident ORF a second one (GCA repeated; what the path takes is its
# shadow on the other strand) whose hexamer occurs in forty stop-ridden copies elsewhere, which puts its coding score between 17.5
# and 35: it becomes confident only once the threshold has been halved at sum * 2000 == n, and then changes the counts
_HALVING_JUNK = b"GCAGCAGCATAGTTAACTAA"


def _halving(reps):
    return b"TAA" + b"ATGCTA" * reps + b"TAAC" + _HALVING_JUNK * 40 + b"TAAC" + b"ATG" + b"GCA" * 32 + b"TAAC"


@lru_cache(maxsize=None)
def halving_genome():
    for reps in range(1980, 2040):
        if n_nodes(_halving(reps), closed=True) == 2000:
            return _halving(reps)
    raise AssertionError("no repeat count gives 2000 nodes")


GC_EDGES = (0.04, 0.085, 0.115, 0.885, 0.915, 0.96)
OPTION_SETS = (dict(), dict(force_nonsd=True), dict(start_weight=0.0), dict(start_weight=3.0), dict(min_gene=120), dict(closed=True),
               dict(translation_table=4), dict(translation_table=4, closed=True, force_nonsd=True, start_weight=3.0, min_gene=120))


# found by search: genomes whose SD decision turns on the -0.5 term alone (rbs_wt[0] in [-0.5, 0) with a strong 5 - 6 base bin, and
# below -0.5 with one), on either strand; the other three terms decide alone in many genomes of the series
SD_TERM_C = ((2000, 0.5, 8947), (2000, 0.65, 8953), (3000, 0.5, 8949), (3000, 0.65, 8953))


def threshold_series():
    out = []
    for L, gc, seed in SD_TERM_C:
        out += _both(("sd_term_c", L, gc, seed), _planted(L, gc, seed))
    for n in NODE_TARGETS:
        out += _both(("nodes", n), many_starts_with_nodes(n), closed=True)
    out += _both(("halving",), halving_genome(), closed=True)
    for gc in GC_EDGES:
        out += _both(("gc", gc), _planted(3000, gc, 8300 + int(1000 * gc)))
    for k, (L, gc) in enumerate(((3000, 0.45), (6000, 0.62))):
        body = _planted(L, gc, 8350 + k)
        for opts in OPTION_SETS:
            out += _both(("options", k) + tuple(sorted(opts.items())), body, **opts)
    return out


# ---- tie_series -------------------------------------------------------------------------------------------------------------------
# An exact tie between two starts of one ORF cannot be planted through the trained hexamer table in a genome this small; these
# genomes hold ORFs with many starts (every second, third and fifth codon), where the search walks longest, and the counters of
# tests/train_ref.py say whether a tie was met.

def tie_series():
    out = []
    for k, period in enumerate((2, 3, 5)):
        unit = b"ATG" + _codons(period - 1, 8400 + k)
        body = _planted(1500, 0.5, 8410 + k) + b"TAA" + unit * (240 // period) + _codons(40, 8420 + k) + b"TAA" + synthetic_contig(50, 0.5, 8430 + k)
        out += _both(("many_starts", period), body)
    for pad in range(3):
        out += _both(("abutting_triple", pad), triple_genome(pad))
    return out


def triple_genome(pad, rest=36):
    """Read along one strand: gene R2, whose stop codon is followed at once by the start codon of R0 in its frame; R1, in the next
    frame, which starts 23 bases before that stop codon, runs through all of R0 and on; and on the other strand gene A, whose stop
    codon overlaps R1's by four bases.  A, R1, R2 are three consecutive overlapping genes, the one connection (A's stop to R2's stop
    through R1's start) that looks through all three slots of a stop's starts: R0's start stands in none of them, and must not.
    Where R0's start is taken all the same (k_ovl_starts0 with `me - 2` one base further out), the connection scorer, which carries
    the overlap of the last slot it looked at into the score, overrates that connection by some 200.  R1 ends `rest` codons after
    R0: between 30 and 39 the right path prefers R0 to R1 by a little and the overrated one takes A, R1, R2, another set of genes,
    on the reverse strand; on the forward strand the same shift changes nothing.  `pad` bases in front shift the frames."""
    open_two = b"GCAGCA" + b"GATGGC" + b"GCA" * 6                        # GCA.. in R2's frame; CAG CAG ATG GCG CAG.. in the next
    r2 = b"ATG" + CLEAN_UNIT * 20 + open_two + b"TAA"
    r0 = b"ATG" + b"GCA" * 32 + b"TAA"                                     # open in the next frame as well: CAG.. CAT AAG CAG..
    r1_rest = b"GCA" * rest + b"G" + b"GCT" + b"TAA"                         # ..CAG GCT TAA in R1's frame
    a = revcomp(b"ATG" + CLEAN_UNIT * 43 + b"GCT" + b"TAA")
    assert r1_rest[-4:] == a[:4] == b"TTAA"
    return b"C" * pad + _planted(600, 0.5, 8450) + b"TAAC" + r2 + r0 + r1_rest + a[4:] + synthetic_contig(50, 0.5, 8451)


# ---- gc_frame_ties ----------------------------------------------------------------------------------------------------------------

def gc_frame_ties():
    """Runs of all-AT and all-GC, 60 bases and longer: the three totals of a window are equal (0 or full), and at the borders of the
    runs every pair ties; ORFs run through them (the runs hold no stop codon in the frames ATA / TAT and GCG / CGC)."""
    seq = (_planted(1500, 0.5, 8500) + b"AT" * 45 + _planted(900, 0.45, 8501) + b"GC" * 45 + _planted(600, 0.55, 8502) + b"A" * 70 + b"G" * 70
           + b"ATG" + b"GCA" * 40 + b"AT" * 33 + b"GCA" * 10 + b"TAA" + synthetic_contig(40, 0.5, 8503))
    return _both(("gc_ties",), seq)


# ---- degenerate -------------------------------------------------------------------------------------------------------------------

def degenerate():
    out = []
    out += _both(("edge_nodes_only",), b"N" * 300)                                     # open ends: twelve edge nodes
    out += _both(("no_node_closed",), b"N" * 300, closed=True)                         # status only
    out += _both(("no_node",), b"TAATTAAC" * 12)                                       # stop codons in all six frames
    out += _both(("too_short",), b"ACG")
    for k in range(12):                                                                 # 2 .. 19 nodes, most without a confident ORF
        out += _both(("tiny", k), synthetic_contig(200, 0.3 + 0.055 * k, 8600 + k))
    out += _both(("n_runs",), _planted(1200, 0.5, 8620) + b"N" * 80 + _planted(1500, 0.5, 8621) + b"N" * 49 + _planted(600, 0.5, 8622), mask=True)
    out += _both(("n_runs",), _planted(1200, 0.5, 8620) + b"N" * 80 + _planted(1500, 0.5, 8621) + b"N" * 49 + _planted(600, 0.5, 8622))
    return out


SERIES = {"length": length_series, "end": end_series, "threshold": threshold_series, "tie": tie_series, "gc_ties": gc_frame_ties,
          "degenerate": degenerate}


@lru_cache(maxsize=None)
def series(name):
    return tuple(SERIES[name]())


def fixture_slices():
    """A slice of each real fixture: the restatement against the oracle on sequence no generator made."""
    from tests.util import read_fasta
    out = []
    for name, lo, hi, opts in (("SRR492066", 30000, 60000, {}), ("KK037166", 0, 40000, {}), ("MIIJ01000039", 10000, 35000, dict(translation_table=4)),
                               ("GCF_001457455.1_NCTC11397_genomic_100kb", 50000, 70000, dict(closed=True))):
        out.append(Genome(("fixture", name), 1, read_fasta(name + ".fna.gz")[0][1][lo:hi].encode(), opts))
    return out


# ---- batch_series -----------------------------------------------------------------------------------------------------------------
BATCH_SIZES = (1, 2, 63, 64, 65, 128, 129, 257)
_BATCH_TABLES = (11, 4, 25, 15)                          # at most four distinct tables per call
FIVE_TABLES = (11, 4, 25, 15, 1)
# where the longest genome stands; the empty genome (no node) takes the first place where the longest does not
_LONGEST_AT = {1: "first", 2: "first", 63: "last", 64: "middle", 65: "first", 128: "last", 129: "middle", 257: "first"}
Member = namedtuple("Member", "seq translation_table start_weight force_nonsd")


def _pool():
    """Members with the call's defaults (open ends, min_gene 90, no masking): the tiny genomes (2 .. 19 nodes) first."""
    tiny = [g.seq for g in series("degenerate") if g.tag[0] == "tiny"] + [g.seq for g in series("length") if g.tag[0] == "length" and g.tag[1] < 300][::7]
    ends = [g.seq for g in series("end") if g.tag[0] == "end_up" and g.tag[2] in (0, 1, 14, 21, 44)] + [g.seq for g in series("end") if g.tag[0] != "end_up"][::3]
    mid = [g.seq for g in series("threshold") if g.tag[0] == "gc"][::2] + [g.seq for g in series("gc_ties")]
    return tiny, ends, mid


def batch(G):
    """(members, the index of the empty genome or None): unequal lengths, SD and motif genomes alternating (force_nonsd on every
    second member), the tiny genomes next to each other, two neighbours with the same sequence, tables, start weights."""
    tiny, ends, mid = _pool()
    longest = _planted(8000, 0.5, 8700)
    empty = b"TAATTAAC" * 12
    seqs = []
    k = 0
    while len(seqs) < G:
        run = tiny[(3 * k) % len(tiny):][:6] if k % 2 == 0 else [ends[k % len(ends)], mid[k % len(mid)], ends[(k + 5) % len(ends)]]
        seqs += run
        if k % 4 == 1:
            seqs.append(seqs[-1])                        # two neighbours with the same sequence
        k += 1
    seqs = seqs[:G]
    at = {"first": 0, "middle": G // 2, "last": G - 1}[_LONGEST_AT[G]]
    seqs[at] = longest
    empty_at = None
    if G >= 2:
        # first place, last place, or next to the boundary of a block of 64 genomes
        empty_at = {2: 1, 63: 0, 64: 63, 65: 64, 128: 0, 129: 128, 257: 63}[G]
        assert empty_at != at
        seqs[empty_at] = empty
    members = [Member(s, _BATCH_TABLES[(g // 3) % 4] if g % 5 == 4 else 11, (4.35, 3.0, 0.0)[(g // 2) % 3] if g % 7 == 3 else 4.35, g % 2 == 1)
               for g, s in enumerate(seqs)]
    return members, empty_at


def permutation(G, seed=8800):
    return np.random.default_rng(seed + G).permutation(G).tolist()
