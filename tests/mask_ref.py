"""The plain reference for every reported mask list: the union of intervals and the runs of a flag array (numpy, vectorised for the
scale test).  A helper module, not a test: tests/test_region_masks_gpu.py and the catalogue of tests/mask_shapes.py share it."""
import numpy as np

KNOWN = np.zeros(256, bool)
KNOWN[list(b"ACGTacgt")] = True


def union(intervals):
    """Sorted, disjoint, touching intervals joined: the reference for every reported list (numpy, vectorised for the scale test)."""
    a = np.asarray(intervals, dtype=np.int64).reshape(-1, 2)
    if not len(a):
        return np.zeros((0, 2), np.int32)
    a = a[np.argsort(a[:, 0], kind="stable")]
    reach = np.maximum.accumulate(a[:, 1])
    first = np.concatenate([[True], a[1:, 0] > reach[:-1]])
    idx = np.flatnonzero(first)
    return np.stack([a[idx, 0], np.maximum.reduceat(a[:, 1], idx)], axis=1).astype(np.int32)


def runs_of(flags, min_len):
    """[begin, end) of the runs of set flags that are at least min_len long or reach the end (the rule of ref lib.pyx:699-713)."""
    f = np.concatenate([[0], np.asarray(flags, np.int8), [0]])
    d = np.diff(f)
    b, e = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    keep = (e - b >= min_len) | (e == len(flags))
    return np.stack([b[keep], e[keep]], axis=1).astype(np.int32)


def is_unknown(seq):
    """Anything outside ACGTacgt."""
    return ~KNOWN[np.frombuffer(bytes(seq), np.uint8)]


def is_lower(seq):
    """The bytes a .. z."""
    a = np.frombuffer(bytes(seq), np.uint8)
    return (a >= 97) & (a <= 122)


def mask_union(seq, regions=None, mask=False, mask_lowercase=False, min_mask=50):
    """What pga_result.masks must report for one contig: named intervals as given, runs by the rule, joined."""
    iv = [tuple(int(x) for x in r) for r in (regions if regions is not None else [])]
    if mask:
        iv += runs_of(is_unknown(seq), min_mask).tolist()
    if mask_lowercase:
        iv += runs_of(is_lower(seq), min_mask).tolist()
    return union(iv)
