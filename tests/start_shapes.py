"""Contigs whose start nodes sit at the thresholds of the start scorer (k_score_starts, k_start_prologue, k_score_starts_mm in
pyrodigal_amd/csrc/pipeline.hip): the inputs of tests/test_start_score_cpu.py and tests/test_start_score_gpu.py.  A helper module,
not a test.  Everything is deterministic; every shape exists on the forward strand and, as the reverse complement of the whole
contig, on the reverse strand."""
import numpy as np

from tests.orf_shapes import START_CODONS, STOP_CODONS, T_STOP, _ACGT, _sense_codons, revcomp
from tests.util import synthetic_contig

# ---- end_series: a start u bases from the upstream end of its contig ---------------------------------------------------------------------
# every length of the upstream composition window (0, 1, 2 .. 14, 15 .. 44 bases from the end, full from 44), every start the motif
# search cuts short (up to 21 bases) and the RBS search (up to 20), then starts past min(start, 63) of the prologue's record
END_U = tuple(range(0, 48)) + tuple(range(60, 67))
END_CODONS = 300                    # sense codons behind the start: no ORF-length scaling (orf >= 250)
# what lies upstream of the start, cut to its last u bases.  "sd": AGGAGG and parts of it at every spacer class, so that SD bins other
# than 0 occur with the motif whole, cut short and hanging off the end; "random": i.i.d. bases
_SD_UPSTREAM = b"CATTAGGAGGTCAACCGTGGAGGATCTTAACGGAGGTGATCCAAGGAGGTTACATCAGGAGGACTTCA"
# "mot": AGAAGA seven bases before the start and nothing else a motif table knows (no other G)
_MOT_UPSTREAM = b"CTTCATTACCTATTCATACTCACTTCTTCATTCACCATTCACTTTTCATCATCAAGAAGATCATTCA"
# "far": the same motif fifteen bases before the start, the widest spacer the search knows: its first base is the contig's first
# base at u = 21, the last distance at which the search drops a candidate
_FAR_UPSTREAM = b"CTTCATTACCTATTCATACTCACTTCTTCATTCACCATTCACTTTCAGAAGATCATTCACTTCATCA"
END_SEEDS = ("sd", "mot", "far", "random")


def _stopless(n, seed):
    """n i.i.d. bases without a stop codon of table 11 in any forward frame (as tests/test_stages_gpu.py builds its ORF body)."""
    s = synthetic_contig(n, 0.5, seed).replace(b"TAA", b"TCA").replace(b"TAG", b"TCG").replace(b"TGA", b"TCA")
    assert not any(stop in s for stop in STOP_CODONS)
    return s


def end_upstream(kind, u):
    full = {"sd": _SD_UPSTREAM, "mot": _MOT_UPSTREAM, "far": _FAR_UPSTREAM}.get(kind) or synthetic_contig(len(_SD_UPSTREAM), 0.5, 7100)
    assert len(full) >= max(END_U)
    return full[len(full) - u:]


def end_contig(kind, u, strand):
    """u upstream bases, ATG, END_CODONS codons without a stop in any frame, TAA, a short random tail."""
    s = end_upstream(kind, u) + b"ATG" + _stopless(3 * END_CODONS, 7200 + u) + b"TAA" + synthetic_contig(60, 0.5, 7300 + u)
    return s if strand == 1 else revcomp(s)


def end_series():
    """[(kind, u, strand, contig)], one contig per entry: a batch of 220 short contigs per strand, so every workgroup of the scorers
    holds more than four contigs."""
    return [(kind, u, strand, end_contig(kind, u, strand)) for strand in (1, -1) for kind in END_SEEDS for u in END_U]


# ---- orf_series: ORF lengths around 120 and 250, contig lengths around 1500 and 3000, edge genes around 5 sqrt(L) ------------------------
ORF_LENGTHS = (117, 120, 123, 246, 249, 252, 255)            # |ndx - stop_val| of a start node
ORF_MIN_GENE, ORF_MIN_EDGE_GENE = 120, 90                    # the shortest listed ORF is exactly the minimum: orf + 3 >= min_gene
CONTIG_LENGTHS = (1499, 1500, 1501, 2999, 3000, 3001)
# an edge node with a negative coding score loses its start score in meta mode when orf >= 5 sqrt(L): 150 at 900, 250 at 2500 bases
EDGE_CASES = ((900, (147, 150, 153)), (2500, (249, 252)))
EDGE_GCS = (0.35, 0.65)


def _planted_orf(orf, rng, gc, k):
    """A start codon, orf / 3 - 1 codons that are neither start nor stop codons, a stop codon: one start node, `orf` bases before its stop."""
    assert orf % 3 == 0
    body = bytes(_ACGT[_sense_codons(orf // 3 - 1, rng, gc)].reshape(-1))
    return STOP_CODONS[k % 3] + START_CODONS[k % 3] + body + STOP_CODONS[(k + 1) % 3]


def _open_orf(ncod, rng, gc):
    """ATG and ncod codons that run off the end of the contig: its starts have no stop codon (edge genes that are no edge nodes)."""
    return b"ATG" + bytes(_ACGT[_sense_codons(ncod, rng, gc)].reshape(-1))


def length_contig(L, strand, seed=7400):
    """A contig of exactly L bases: the listed ORFs (those that fit) between random spacers, and at its right end an ORF of low GC
    that runs off the contig (coding scores below zero: the penalties that depend on L > 1500)."""
    rng = np.random.default_rng(seed + L)
    orfs = ORF_LENGTHS if L > 2000 else (117, 120, 123, 249, 252)
    parts = [synthetic_contig(150, 0.5, seed + L + 1)]
    for k, orf in enumerate(orfs):
        parts.append(_planted_orf(orf, rng, 0.5, k))
        parts.append(synthetic_contig(7 + k % 3, 0.5, seed + L + 10 + k))
    tail = b"TAA" + _open_orf(40, rng, 0.3)
    used = sum(len(p) for p in parts) + len(tail)
    assert used <= L
    parts.append(synthetic_contig(L - used, 0.5, seed + L + 2))
    s = b"".join(parts) + tail
    assert len(s) == L
    return s if strand == 1 else revcomp(s)


def edge_contig(L, orf, gc, strand, seed=7500):
    """A contig of L bases that opens with orf / 3 codons without a start or stop codon and a stop codon: with open ends an edge node at
    ndx 0 whose ORF is `orf` bases long."""
    rng = np.random.default_rng(seed + 7 * L + orf + int(100 * gc))
    head = bytes(_ACGT[_sense_codons(orf // 3, rng, gc)].reshape(-1)) + b"TAA"
    s = head + synthetic_contig(L - len(head), 0.5, seed + L + orf + 1)
    return s if strand == 1 else revcomp(s)


def orf_series():
    """[(tag, strand, contig)]: tag is ("length", L) or ("edge", L, orf, gc)."""
    out = [(("length", L), strand, length_contig(L, strand)) for L in CONTIG_LENGTHS for strand in (1, -1)]
    out += [(("edge", L, orf, gc), strand, edge_contig(L, orf, gc, strand))
            for L, orfs in EDGE_CASES for orf in orfs for gc in EDGE_GCS for strand in (1, -1)]
    return out


# ---- scan_series: the 500 nodes the scan for an edge node of the same ORF covers ----------------------------------------------------------
# prefix "": the first start is an ordinary ATG at ndx 0, which scoring converts to an edge node (conv); "CC": the same at ndx 2;
# "GCC": position 0 holds no start codon, so extraction itself puts an edge node there
SCAN_PREFIXES = {"conv0": b"", "conv2": b"CC", "edge": b"GCC"}


def scan_contig(variant, strand):
    """A 3600-base ORF open at the contig's upstream end with a start every six bases (and as many on the other strand): some of its
    starts lie within 500 nodes of the edge node at its end, the others beyond."""
    s = SCAN_PREFIXES[variant] + b"ATGGCC" * 600 + b"TAA" + synthetic_contig(300, 0.5, 7600)
    return s if strand == 1 else revcomp(s)


def scan_series():
    """[(variant, strand, contig)]"""
    return [(v, strand, scan_contig(v, strand)) for v in SCAN_PREFIXES for strand in (1, -1)]


# ---- tile_series: the cuts of the model-major order ---------------------------------------------------------------------------------------
TILE_SIZES = (256, 512, 1024)


def tile_series():
    """A batch of 607 contigs: 600 of 120 .. 400 bases (a few starts each, some none), among them a scan contig of either strand
    (more than 1024 starts each: chains longer than any tile, with short chains before and behind them in their model's order), a
    planted contig of 20 kbp, and contigs without any node."""
    from pyrodigal_amd import benchdata
    rng = np.random.default_rng(7700)
    small = [synthetic_contig(int(rng.integers(120, 401)), 0.40 + 0.18 * float(rng.random()), 7701 + k) for k in range(600)]
    extra = {37: b"", 150: scan_contig("edge", 1), 151: b"ATG", 310: b"N" * 500, 311: scan_contig("conv0", -1),
             470: benchdata.planted_contig(20000, 0.58, 7790), 599: b""}
    out = []
    for k, s in enumerate(small):
        out.append(s)
        if k in extra:
            out.append(extra[k])
    return out


# ---- the models ----------------------------------------------------------------------------------------------------------------------------
# The SD and the non-SD model of tests/test_coding_score_gpu.py, and "motif": the motif table of "nonsd" holds two entries above -4 (a
# 4-mer and a 5-mer at one spacer class), so no input makes its motif search return 3 or 6 bases; a model trained without SD motifs on
# the 100 kb fixture has weights for all four lengths.  No trained table of the fixtures has a 6-base motif in the widest spacer class
# (13 .. 15 bases), the only candidates 21 bases upstream of a start: that one weight of "motif" is set by hand.
MOT_WT = 80 + 28 * 8 + 32 * 4 * 8           # offset of mot_wt[4][4][4096] in struct _training
FAR_MOTIF, FAR_MOTIF_INDEX, FAR_MOTIF_WEIGHT = b"AGAAGA", 260, 2.5
MODEL_NAMES = ("sd", "nonsd", "motif")
# the models of the listed launches: (source, GC label, translation table).  Entry LISTED_UNUSED lies outside every contig's GC window
# and no contig is given to it: a model without a chain between models with chains.
LISTED_MODELS = (("sd", 0.45, 11), ("motif", 0.52, 11), ("nonsd", 0.75, 11), ("nonsd", 0.585, 11), ("motif", 0.50, 4), ("sd", 0.62, 11))
LISTED_UNUSED = 2


def base_models():
    from oracle import oracle as orc
    from tests.util import golden_path, read_fasta
    sd = orc.Training.load(golden_path("SRR492066.training.bin.gz"))
    nonsd = orc.Oracle(read_fasta("KK037166.fna.gz")[0][1]).train()
    motif = orc.Oracle(read_fasta("GCF_001457455.1_NCTC11397_genomic_100kb.fna.gz")[0][1]).train(force_nonsd=True)
    assert sd.uses_sd == 1 and nonsd.uses_sd == 0 and motif.uses_sd == 0
    assert orc.mer_text(6, FAR_MOTIF_INDEX) == FAR_MOTIF.decode() and FAR_MOTIF in _FAR_UPSTREAM
    motif._f64(MOT_WT + 8 * ((3 * 4 + 3) * 4096 + FAR_MOTIF_INDEX))[0] = FAR_MOTIF_WEIGHT        # mot_wt[3][3][AGAAGA]
    return {"sd": sd, "nonsd": nonsd, "motif": motif}


def listed_models(base):
    out = []
    for src, gc, tt in LISTED_MODELS:
        t = base[src].copy(); t.set_gc(gc); t.set_trans_table(tt)
        out.append(t)
    return out


def model_of_contig(n):
    """Contig i under the i-th of the used models in turn."""
    used = [m for m in range(len(LISTED_MODELS)) if m != LISTED_UNUSED]
    return [used[i % len(used)] for i in range(n)]


# ---- what the oracle's node arrays say about an input --------------------------------------------------------------------------------------

def start_distance(nodes, L):
    """Per node: the strand-local position of a start node (bases between it and the upstream end of its contig), -1 for a stop node."""
    d = np.where(nodes["strand"] == 1, nodes["ndx"], L - 1 - nodes["ndx"]).astype(np.int64)
    return np.where(nodes["type"] == T_STOP, -1, d)


def orf_lengths(nodes):
    return np.abs(nodes["ndx"].astype(np.int64) - nodes["stop_val"].astype(np.int64))


def open_orf_starts(nodes):
    """The start nodes whose ORF has no stop codon (its stop node is an edge node) and that are no edge nodes themselves."""
    open_stops = {(int(nodes["ndx"][i]), int(nodes["strand"][i])) for i in np.flatnonzero((nodes["type"] == T_STOP) & (nodes["edge"] == 1))}
    return [int(i) for i in np.flatnonzero((nodes["type"] != T_STOP) & (nodes["edge"] == 0))
            if (int(nodes["stop_val"][i]), int(nodes["strand"][i])) in open_stops]


def tile_layout(starts, contigs_of_model, tile):
    """The model-major order of k_mm_place with every model's chains in batch order: {model: (chains [(contig, first item, starts)],
    chains per tile)}.  `starts[m][c]`: the start nodes of contig c under model m's translation table; `contigs_of_model`: the contigs
    a model scores.  Only chains with start nodes take part, and every model begins a tile of its own.  (The device orders a model's
    chains by atomics; a chain with more starts than a tile has items is cut in any order.)"""
    out = {}
    for m, contigs in contigs_of_model.items():
        at, chains = 0, []
        for c in contigs:
            if starts[m][c] > 0:
                chains.append((c, at, starts[m][c]))
                at += starts[m][c]
        tiles = [sum(1 for _, a, n in chains if a < (t + 1) * tile and a + n > t * tile) for t in range(-(-at // tile))]
        out[m] = (chains, tiles)
    return out
