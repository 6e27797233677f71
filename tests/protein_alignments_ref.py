"""The rules of pga_align_pairs and pga_cluster_edges (include/pyrodigal_amd.h) in plain Python: what the device must give, number
for number.

Rows are sequences of Python integers, the elements of a token row.  The edit distance is the full-matrix DP: it has no band, so it
cannot share a bug with the kernel.  Nothing here is fast, and nothing here knows how the device does it."""


def edit_distance(a, b):
    """The unit-cost Levenshtein distance of two rows: substitutions, insertions and deletions cost 1 each."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (0 if a[i - 1] == b[j - 1] else 1), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[len(b)]


def edit_distance_rows(a, b):
    """`edit_distance`, a matrix row at a time in numpy, for the long and the many pairs of the device tests (test_protein_alignments_cpu
    holds it against `edit_distance`).  Still the full matrix: row i from row i - 1, and the insertions along the row as a running
    minimum of cur[k] - k."""
    import numpy as np
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    idx = np.arange(len(b) + 1, dtype=np.int64)
    prev = idx.copy()
    for i in range(1, len(a) + 1):
        cur = np.empty_like(prev)
        cur[0] = i
        cur[1:] = np.minimum(prev[:-1] + (b != a[i - 1]), prev[1:] + 1)
        prev = np.minimum.accumulate(cur - idx) + idx
    return int(prev[len(b)])


def align_pairs(rows, pairs, max_distance, num, den, distance_of=edit_distance):
    """(distance, passed) of every pair, clauses 1 to 4: -1 and 0 for an index outside 0 .. G - 1; else the distance capped at
    max_distance + 1, and 1 where it is within max_distance and distance * den <= (den - num) * the longer row."""
    G = len(rows)
    distance, passed = [], []
    for a, b in pairs:
        if not (0 <= a < G and 0 <= b < G):
            distance.append(-1); passed.append(0)
            continue
        d = min(distance_of(rows[a], rows[b]), max_distance + 1)
        distance.append(d)
        passed.append(1 if d <= max_distance and d * den <= (den - num) * max(len(rows[a]), len(rows[b])) else 0)
    return distance, passed


def cluster_edges(edges, keep, n, weights):
    """The components of 0 .. n - 1 under the kept edges.  Returns a dict: cluster [n], representatives [U], sizes [U], n_clusters,
    n_used -- the kept edges with both indices inside 0 .. n - 1, an edge of a record with itself among them."""
    label = list(range(n))

    def find(x):
        while label[x] != x:
            x = label[x]
        return x

    used = 0
    for e, (a, b) in enumerate(edges):
        if keep is not None and not keep[e]:
            continue
        if not (0 <= a < n and 0 <= b < n):
            continue
        used += 1
        ra, rb = find(a), find(b)
        if ra != rb:
            label[max(ra, rb)] = min(ra, rb)        # (the smaller root stays a root: a root is its component's smallest member)
    label = [find(g) for g in range(n)]
    roots = sorted(set(label))
    number = {r: u for u, r in enumerate(roots)}
    members = {r: [] for r in roots}
    for g in range(n):
        members[label[g]].append(g)
    heaviest = lambda ms: min(ms, key=lambda g: (-(weights[g] if weights is not None else 0), g))      # noqa: E731
    return {
        "cluster": [number[label[g]] for g in range(n)],
        "representatives": [heaviest(members[r]) for r in roots],
        "sizes": [len(members[r]) for r in roots],
        "n_clusters": len(roots), "n_used": used,
    }
