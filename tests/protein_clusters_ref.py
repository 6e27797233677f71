"""The rule of pga_cluster_sketches (include/pyrodigal_amd.h) in plain Python: what the device must give, number for number.

Rows are lists of Python integers -- the real entries of a sketch row, ascending and distinct, `len(row)` being the device's count.
Nothing here is fast, and nothing here knows how the device does it."""


def shared_of(row_a, row_b, size):
    """(shared, m) of two rows as pga_sketch_pairs defines them: of the m = min(size, |union|) smallest hashes of the union, those
    that lie in both."""
    a, b = set(row_a), set(row_b)
    low = sorted(a | b)[:size]
    return sum(1 for v in low if v in a and v in b), len(low)


def heaviest(members, weights):
    """The member of greatest weight; on a tie, the smallest index (weights None: all equal)."""
    return min(members, key=lambda g: (-(weights[g] if weights is not None else 0), g))


def candidates(rows, weights, probes):
    """Clauses 1 to 3: (the sorted distinct candidate pairs, the number of proposals that made them)."""
    buckets = {}
    for g, row in enumerate(rows):
        for h in row[:probes]:                      # (padding behind the count is not in `row` at all)
            buckets.setdefault(h, []).append(g)
    proposed = []
    for members in buckets.values():
        c = heaviest(members, weights)
        proposed += [(min(c, g), max(c, g)) for g in members if g != c]
    return sorted(set(proposed)), len(proposed)


def cluster(rows, weights, size, probes, num, den, min_union):
    """The whole rule.  Returns a dict: cluster [G], representatives [U], sizes [U], edges [(a, b)], edge_shared, edge_union,
    n_clusters, n_edges -- and, for the tests' own assertions, candidates (the distinct pairs) and proposals (with duplicates)."""
    G = len(rows)
    for row in rows:
        assert len(row) <= size and all(x < y for x, y in zip(row, row[1:])), row
    cand, proposals = candidates(rows, weights, probes)
    edges, edge_shared, edge_union = [], [], []
    for a, b in cand:
        shared, m = shared_of(rows[a], rows[b], size)
        if m >= max(min_union, 1) and shared * den >= num * m:
            edges.append((a, b)); edge_shared.append(shared); edge_union.append(m)
    # components by repeated relabelling: slow, and plainly right
    label = list(range(G))
    changed = True
    while changed:
        changed = False
        for a, b in edges:
            low = min(label[a], label[b])
            if label[a] != low or label[b] != low:
                label[a] = label[b] = low
                changed = True
    # (a label is now the smallest member of its component: every relabelling lowers a label to that of a neighbour, and the loop
    #  ends only when both ends of every edge agree)
    roots = sorted(set(label))
    number = {r: u for u, r in enumerate(roots)}
    members = {r: [] for r in roots}
    for g in range(G):
        members[label[g]].append(g)
    return {
        "cluster": [number[label[g]] for g in range(G)],
        "representatives": [heaviest(members[r], weights) for r in roots],
        "sizes": [len(members[r]) for r in roots],
        "edges": edges, "edge_shared": edge_shared, "edge_union": edge_union,
        "n_clusters": len(roots), "n_edges": len(edges),
        "candidates": cand, "proposals": proposals,
    }
