"""The rule of pga_sketch_proteins and pga_sketch_pairs (include/pyrodigal_amd.h) restated in plain Python, from the header's text, with
Python integers.  The string of a gene record comes from tests/protein_groups_ref.string_of -- never from the code under test."""
import numpy as np

from tests import protein_groups_ref

MASK = (1 << 64) - 1
INT64_MAX = (1 << 63) - 1
SKIP = 255
GOLDEN, MUL1, MUL2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def mix(x, seed=0):
    """z of the header: the key plus (seed + 1) times the golden ratio, through the finaliser of splitmix64."""
    z = (x + (seed + 1) * GOLDEN) & MASK
    z = ((z ^ (z >> 30)) * MUL1) & MASK
    z = ((z ^ (z >> 27)) * MUL2) & MASK
    return z ^ (z >> 31)


def hash_of(x, seed=0):
    return mix(x, seed) >> 1


def default_classes(unknown_residue="X"):
    table = list(range(128))
    table[ord(unknown_residue)] = SKIP
    return table


def classes_of(groups):
    """A reduced alphabet: every string of `groups` is one class, letters not named are skipped."""
    table = [SKIP] * 128
    for n, letters in enumerate(groups):
        for ch in letters:
            assert table[ord(ch)] == SKIP
            table[ord(ch)] = n
    return table


def codes_of(string, unit, classes=None):
    if unit == "gene":
        return [{65: 0, 67: 1, 71: 2, 84: 3}.get(b, SKIP) for b in bytes(string)]
    return [classes[b] if b < 128 else SKIP for b in bytes(string)]


def keys_of(string, k, unit, classes=None):
    """The keys of the valid windows, in order."""
    bits = 2 if unit == "gene" else 8
    codes = codes_of(string, unit, classes)
    keys = []
    for j in range(len(codes) - k + 1):
        w = codes[j:j + k]
        if SKIP in w:
            continue
        keys.append(sum(c << (bits * (k - 1 - i)) for i, c in enumerate(w)))
    return keys


def sketch(string, k, s, unit="protein", seed=0, classes=None):
    """(the count smallest distinct hashes ascending, valid windows)"""
    keys = keys_of(string, k, unit, classes)
    return sorted({hash_of(x, seed) for x in keys})[:s], len(keys)


def pair(row_a, row_b, s):
    """(shared, m) of two lists of real entries"""
    a, b = set(row_a), set(row_b)
    low = sorted(a | b)[:s]
    return sum(1 for v in low if v in a and v in b), len(low)


def sketches_ref(strings, k, s, unit="protein", seed=0, classes=None):
    """(sketch [G, s], count [G], windows [G]) as int64 arrays, and the rows as lists."""
    G = len(strings)
    out, count, windows, rows = np.full((G, s), INT64_MAX, np.int64), np.zeros(G, np.int64), np.zeros(G, np.int64), []
    for g, string in enumerate(strings):
        row, w = sketch(string, k, s, unit, seed, classes)
        out[g, :len(row)] = row
        count[g], windows[g] = len(row), w
        rows.append(row)
    return out, count, windows, rows


def protein_sketches_ref(seqs, circular, records, k, s, unit="protein", seed=0, classes=None, tables=None, include_stop=False, strict=True,
                         unknown_residue="X"):
    strings = [protein_groups_ref.string_of(seqs, circular, r, unit, tables, include_stop, strict, unknown_residue) for r in records]
    if classes is None:
        classes = default_classes(unknown_residue)
    return sketches_ref(strings, k, s, unit, seed, classes) + (strings,)


def pairs_ref(rows, pairs, s):
    """(shared [P], union [P]); -1 for a pair with an index outside 0 .. G - 1"""
    G = len(rows)
    shared, union = [], []
    for a, b in pairs:
        if 0 <= a < G and 0 <= b < G:
            x, m = pair(rows[a], rows[b], s)
        else:
            x, m = -1, -1
        shared.append(x)
        union.append(m)
    return np.array(shared, np.int64).reshape(-1), np.array(union, np.int64).reshape(-1)
