"""The rule for circular contigs, restated over the CPU oracle: the unchanged linear finder twice, and a choice of
where to cut.  Reference for tests/test_circular_cpu.py and tests/test_circular_gpu.py."""
import glob
import os

import numpy as np

from oracle import oracle as orc
from tests.util import GOLDEN, golden_path, read_fasta, synthetic_contig


def cut_of(genes, L):
    """Step 2: genes as (begin, end, ...) 1-based inclusive; the middle of the widest uncovered stretch, the middle half first."""
    cov = np.zeros(L + 2, np.int64)
    for g in genes:
        b, e = int(g[0]), int(g[1])
        cov[b] += 1
        cov[e + 1] -= 1
    free = (np.cumsum(cov)[1:L + 1] == 0).astype(np.int8)
    d = np.diff(np.concatenate([[0], free, [0]]))
    gb, ge = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    if not len(gb):
        return L // 2
    mid, w = (gb + ge) // 2, ge - gb
    inner = (mid >= L // 4) & (mid < L - L // 4)
    if inner.any():
        mid, w = mid[inner], w[inner]
    best = np.flatnonzero(w == w.max())
    return int(mid[best[np.argmin(np.abs(mid[best] - L // 2))]])   # argmin: first = lowest mid


def meta_bins():
    """The 13 bins of tests/golden/models, in sorted file order."""
    return [orc.Training.load(p) for p in sorted(glob.glob(os.path.join(GOLDEN, "models", "*.tinf.bin.gz")))]


def oracle_call(seq, models, meta, closed, **oracle_kw):
    """The linear call on the CPU oracle; returns the Oracle (genes(), nodes()) and the winning model (0 in single mode)."""
    o = orc.Oracle(seq, **oracle_kw)
    if meta:
        phase = o.find_genes_meta(models, orc.Params(closed=closed))
    else:
        o.find_genes_single(models[0], orc.Params(closed=closed))
        phase = 0
    return o, phase


def coords(o):
    g = o.genes()
    n = o.nodes()
    return [(int(b), int(e), int(n["strand"][s])) for b, e, s in zip(g["begin"], g["end"], g["start_ndx"])]


class Circular:
    """The circular call of `seq`: `cut`, `rotated` (R), `oracle` (the Oracle of pass 2, on R), `model`, `genes` (begin, end, strand
    in the record's coordinates, in the order the device reports them) and `order` (their indices into the oracle's genes)."""

    def __init__(self, seq, models, meta, closed=False, **oracle_kw):
        seq = seq.encode("ascii") if isinstance(seq, str) else bytes(seq)
        L = len(seq)
        p1, _ = oracle_call(seq, models, meta, closed, **oracle_kw)
        self.linear = coords(p1)
        self.cut = cut_of(self.linear, L)
        self.rotated = seq[self.cut:] + seq[:self.cut]
        self.oracle, self.model = oracle_call(self.rotated, models, meta, True, **oracle_kw)
        g = coords(self.oracle)
        # pass 2's order, rotated: the genes that begin in S[:cut] (begin_R > L - cut) come first
        self.order = [k for k, x in enumerate(g) if x[0] > L - self.cut] + [k for k, x in enumerate(g) if x[0] <= L - self.cut]
        self.genes = [((g[k][0] - 1 + self.cut) % L + 1, (g[k][0] - 1 + self.cut) % L + 1 + g[k][1] - g[k][0], g[k][2]) for k in self.order]


def planted_orf():
    """The synthetic input of the issue: a 1 206-bp ORF cut at its base 600, the halves at the two ends of 30 kbp of noise.
    Returns (S, the ORF)."""
    rng = np.random.default_rng(3)
    g = "ATG" + "".join(rng.choice(["GCT", "GAA", "AAA", "CTG", "GGT", "GAT", "ACC", "ATC", "CGT", "CAG"], 400)) + "TAA"
    s = g[600:] + synthetic_contig(30000, 0.5, 77).decode("ascii") + "TTAGTTAGTTAGAGGAGGTAAACC" + g[:600]
    return s.encode("ascii"), g


def fixture(name):
    return read_fasta(name + ".fna.gz")[0][1].encode("ascii")


def single_model(name):
    return [orc.Training.load(golden_path(name))]
