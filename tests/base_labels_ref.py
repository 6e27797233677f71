"""The rule of pga_label_bases (include/pyrodigal_amd.h) restated in numpy: the raw byte of every base of a contig under gene records,
the four preset class maps, and the padded and ragged tensors.  A record is (contig, begin, end, strand, partial_begin, partial_end)
with 1-based inclusive begin and end, as in pga_gene; end > length names a gene across the origin of a circular contig."""
import numpy as np

FWD, REV, START, STOP = (0x01, 0x02, 0x04), (0x08, 0x10, 0x20), 0x40, 0x80
PRESETS = ("raw", "coding", "strand", "frame")


def raw_labels(length, records):
    """uint8[length]: the OR over the records that cover each position; `records` are those of this one contig, in any order."""
    raw = np.zeros(length, np.uint8)
    p = np.arange(length, dtype=np.int64)
    for _, b, e, strand, partial_begin, partial_end in records:
        assert 1 <= b <= length and 3 <= e - b + 1 <= length and (e - b + 1) % 3 == 0, (b, e, length)
        for q in (p + 1, p + 1 + length):                   # at most one of the two lies in [b, e]
            covered = (b <= q) & (q <= e)
            if strand == 1:
                phase = (q - b) % 3
                bits = np.choose(phase, FWD)
                bits = bits | np.where((q <= b + 2) & (partial_begin == 0), START, 0)
                bits = bits | np.where((q >= e - 2) & (partial_end == 0), STOP, 0)
            else:
                phase = (e - q) % 3                         # counted in the gene's own reading direction
                bits = np.choose(phase, REV)
                bits = bits | np.where((q >= e - 2) & (partial_end == 0), START, 0)
                bits = bits | np.where((q <= b + 2) & (partial_begin == 0), STOP, 0)
            raw |= np.where(covered, bits, 0).astype(np.uint8)
    return raw


def preset_map(name):
    """int64[256]: the id of every raw byte under a preset."""
    ids = np.zeros(256, np.int64)
    for raw in range(256):
        position_bits = [k for k in range(6) if raw >> k & 1]
        if name == "raw":
            ids[raw] = raw
        elif name == "coding":
            ids[raw] = 1 if position_bits else 0
        elif name == "strand":
            ids[raw] = (1 if any(k < 3 for k in position_bits) else 0) + (2 if any(k >= 3 for k in position_bits) else 0)
        elif name == "frame":
            ids[raw] = 0 if not position_bits else 7 if len(position_bits) > 1 else position_bits[0] + 1
        else:
            raise KeyError(name)
    return ids


def base_labels_ref(lengths, records, class_map, layout="padded", pad=-100, width=None, dtype=np.int64):
    """The tensor of the rule: ([B, W] padded, W = `width` or the longest contig) or (1-D ragged), and the offsets of the contigs."""
    lengths = [int(x) for x in lengths]
    class_map = np.asarray(class_map, np.int64)
    rows = [class_map[raw_labels(n, [r for r in records if r[0] == i])] for i, n in enumerate(lengths)]
    off = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    if layout == "ragged":
        return (np.concatenate(rows) if rows else np.zeros(0, np.int64)).astype(dtype), off
    w = max(lengths, default=0) if width is None else width
    out = np.full((len(lengths), w), pad, np.int64)
    for i, row in enumerate(rows):
        out[i, :len(row)] = row
    return out.astype(dtype), off
