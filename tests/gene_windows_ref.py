"""The rule of pga_gene_windows (include/pyrodigal_amd.h) restated in plain Python and numpy, from the header's text: the class of
every base a window names, the tokens of a row, and the padded and ragged tensors.  A record is (contig, begin, end, strand, ...) with
1-based inclusive begin and end, as in pga_gene; end > length names a gene across the origin of a circular contig.  A window bound is
(anchor, delta) with the anchor "start" or "end"."""
import numpy as np

A, C, G, T, N, OUTSIDE = range(6)
LETTER_CLASS = {"A": A, "C": C, "G": G, "T": T}
COMPLEMENT = {A: T, T: A, C: G, G: C, N: N}
DEFAULT_BASE_IDS = (0, 1, 2, 3, 4, 4)                          # A, C, G, T, N, outside (= N)
DEFAULT_CODON_IDS = tuple(range(64)) + (64, 64)                # the 64 codons in ACGT order, unknown, outside (= unknown)


def offsets_of(record, begin, end):
    """(t_lo, t_hi) of a window on a record: anchors start = 0 and end = n."""
    n = record[2] - record[1] + 1
    anchor = {"start": 0, "end": n}
    return anchor[begin[0]] + begin[1], anchor[end[0]] + end[1]


def base_class(seq, circular, record, t):
    """The class of offset t on the record's reading axis: 0 .. 3 = A, C, G, T in the gene's strand, 4 = N, 5 = outside."""
    _, b, e, strand = record[:4]
    L = len(seq)
    q = b + t if strand == 1 else e - t
    if circular:
        q = (q - 1) % L + 1                                    # Python's % is the floor modulo
    elif q < 1 or q > L:
        return OUTSIDE
    c = LETTER_CLASS.get(chr(seq[q - 1]).upper(), N)
    return c if strand == 1 else COMPLEMENT[c]


def row_tokens(seq, circular, record, begin, end, unit="base", ids=None, bos=None, eos=None, max_length=None):
    """The tokens of one row: [bos], the ids of the first R units, [eos]."""
    t_lo, t_hi = offsets_of(record, begin, end)
    m = max(0, t_hi - t_lo)
    classes = [base_class(seq, circular, record, t_lo + x) for x in range(m)]
    if unit == "base":
        ids = DEFAULT_BASE_IDS if ids is None else ids
        units = [ids[c] for c in classes]
    else:
        ids = DEFAULT_CODON_IDS if ids is None else ids
        assert begin[1] % 3 == 0 and end[1] % 3 == 0 and m % 3 == 0
        units = []
        for j in range(m // 3):
            c0, c1, c2 = classes[3 * j:3 * j + 3]
            if OUTSIDE in (c0, c1, c2):
                units.append(ids[65])
            elif N in (c0, c1, c2):
                units.append(ids[64])
            else:
                units.append(ids[16 * c0 + 4 * c1 + c2])
    s = (bos is not None) + (eos is not None)
    if max_length is not None:
        assert max_length >= s + 1
        units = units[:max_length - s]                         # cut on the far side: eos survives
    return ([bos] if bos is not None else []) + units + ([eos] if eos is not None else [])


def gene_windows_ref(seqs, circular, records, begin, end, unit="base", ids=None, bos=None, eos=None, max_length=None, layout="padded",
                     pad=0, width=None, dtype=np.int64):
    """The tensor of the rule ([G, W] padded, W = `width` or the longest row; 1-D ragged), the offsets of the rows and their lengths."""
    rows = [row_tokens(seqs[r[0]], bool(circular[r[0]]) if circular is not None else False, r, begin, end, unit, ids, bos, eos, max_length)
            for r in records]
    lens = np.array([len(r) for r in rows], np.int64)
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    if layout == "ragged":
        flat = [v for row in rows for v in row]
        return np.array(flat, np.int64).astype(dtype), off, lens
    w = int(lens.max()) if width is None and len(rows) else (0 if width is None else width)
    out = np.full((len(rows), w), pad, np.int64)
    for g, row in enumerate(rows):
        out[g, :len(row)] = row
    return out.astype(dtype), off, lens
