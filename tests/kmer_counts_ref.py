"""The rule of pga_count_kmers (include/pyrodigal_amd.h) restated in plain Python and numpy, from the header's text: the class of a
letter, the code of a window, the axis of a contig row and of a gene row, the bins.  Nothing here imports the package."""
import numpy as np

LETTERS = "ACGT"                                   # the public order: A, C, G, T = 0 .. 3
_CLASS = np.full(256, 4, np.int64)                 # anything else reads N = 4
for _k, _ch in enumerate(LETTERS):
    _CLASS[ord(_ch)] = _CLASS[ord(_ch.lower())] = _k


def classes(seq):
    """The class of every letter of `seq` (bytes): 0 .. 3, or 4 for N."""
    return _CLASS[np.frombuffer(bytes(seq), np.uint8)]


def rc(code, k):
    """The code of the reverse complement of the k-mer with `code`."""
    digits = [(code >> (2 * j)) & 3 for j in range(k)]                # last base first
    out = 0
    for d in digits:
        out = out * 4 + (3 - d)
    return out


def kmer(code, k):
    return "".join(LETTERS[(code >> (2 * (k - 1 - j))) & 3] for j in range(k))


def identity_table(k):
    return list(range(4 ** k))


def canonical_table(k):
    """bin = the rank of min(code, rc(code)) among the canonical codes in ascending order."""
    canon = sorted({min(x, rc(x, k)) for x in range(4 ** k)})
    rank = {c: r for r, c in enumerate(canon)}
    return [rank[min(x, rc(x, k))] for x in range(4 ** k)]


def count_axis(axis, k, step, table, n_bins):
    """The counts of the windows that start at t = 0, step, 2 step, .. while t + k <= len(axis), of an axis of classes, and the number
    of those window positions.  A window that holds an N is not counted, nor one whose bin is -1."""
    n = len(axis)
    out = np.zeros(n_bins, np.int64)
    if n < k:
        return out, 0
    starts = np.arange(0, n - k + 1, step)
    code = np.zeros(len(starts), np.int64)
    ok = np.ones(len(starts), bool)
    for j in range(k):
        c = axis[starts + j]
        ok &= c < 4
        code = code * 4 + (c & 3)
    bins = np.asarray(table, np.int64)[code[ok]]
    np.add.at(out, bins[bins >= 0], 1)
    return out, len(starts)


def contig_axis(seq, k, circular):
    """Forward strand as stored; on a circle base j of window p is read at (p + j) mod L, p = 0 .. L - 1; none if L < k."""
    c = classes(seq)
    if len(c) < k:
        return c[:0]
    return np.concatenate([c, c[:k - 1]]) if circular else c


def gene_axis(seq, begin, end, strand, circular):
    """The gene [begin, end] (1-based, inclusive) in its own direction: q(t) = begin + t forward, end - t reverse, taken modulo L on a
    circle; a reverse gene's letters are complemented, N stays N."""
    c = classes(seq)
    L, n = len(c), end - begin + 1
    assert 1 <= begin <= L and 3 <= n <= L and n % 3 == 0 and (end <= L or circular)
    t = np.arange(n)
    q = begin + t if strand == 1 else end - t
    x = c[(q - 1) % L]
    return x if strand == 1 else np.where(x < 4, 3 - x, 4)


def kmer_counts_ref(seqs, circular, records, k, rows, step, table, n_bins):
    """(counts [R, n_bins] int32, windows [R] int64) of `rows` = "contig", "gene" or "contig_genes"; `records`: (contig, begin, end,
    strand, ...) tuples; `circular`: a flag per contig."""
    assert 1 <= k <= 6 and len(table) == 4 ** k and all(-1 <= b < n_bins for b in table) and n_bins <= 4096
    assert step in ((1,) if rows == "contig" else (1, 3))
    if rows == "contig":
        got = [count_axis(contig_axis(s, k, circ), k, 1, table, n_bins) for s, circ in zip(seqs, circular)]
    else:
        got = [count_axis(gene_axis(seqs[r[0]], r[1], r[2], r[3], circular[r[0]]), k, step, table, n_bins) for r in records]
    counts = np.array([g[0] for g in got], np.int64).reshape(len(got), n_bins)
    windows = np.array([g[1] for g in got], np.int64)
    if rows == "contig_genes":
        c2, w2 = np.zeros((len(seqs), n_bins), np.int64), np.zeros(len(seqs), np.int64)
        for g, r in enumerate(records):
            c2[r[0]] += counts[g]
            w2[r[0]] += windows[g]
        counts, windows = c2, w2
    assert counts.max(initial=0) <= np.iinfo(np.int32).max
    return counts.astype(np.int32), windows
