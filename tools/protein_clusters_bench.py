"""Near-identical proteins clustered on the device from their sketches: what `DeviceSketches.cluster` saves over the torch route a
caller had before.

One context, meta mode under `benchdata.load_model_set()`.  The batch is that of tools/protein_sketches_bench.py: the 6 250 x 20 kbp
batch of tools/device_input_bench.py with every contig present a second time, reverse-complemented (12 500 contigs).  `find_genes` and
`protein_sketches` run once, outside the clock; only the step behind them is timed, on the host clock:
  route (a): torch -- a stable sort of the first `probes` sketch columns with their record indices, run heads and a `cumsum` for the
             buckets, the centre of every bucket by `scatter_reduce(amax)` over (weight, -index) packed into one int64, one packed
             pair per member and `torch.unique`, `DeviceSketches.compare` (`pga_sketch_pairs`) over the distinct pairs, the
             threshold, and the components by repeated `scatter_reduce(amin)` over the edges until no label changes (one
             host round trip per round); numbering, representatives and sizes by `cumsum`, `scatter_reduce` and `bincount`;
  route (b): `DeviceSketches.cluster` -- and once more with the six tensors given, which leaves the library's own host work and the
             device.
Warm-up rounds, then rounds that alternate between the routes; min / median / max.  The two routes must give the same clusters,
representatives, sizes and edges in every round (asserted).  The JSON line also says how many probes, distinct candidates, edges and
clusters the batch gives (`Context.cluster_stats`), and how many rounds the torch loop took.

`--trace clusters` makes three calls of `DeviceSketches.cluster`, for a kernel trace of its own.

    python tools/protein_clusters_bench.py [--contigs 6250] [--rounds 7] [--warmup 1] [--k 5] [--size 32] [--probes 8]
                                           [--num 9] [--den 10] [--min-union 8] [--trace clusters]"""
import argparse
import json
import os
import sys
import time

import torch                     # first: the library then binds to the HIP runtime of torch's wheel
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrodigal_amd import ProteinClusters, ProteinSketches, _cabi, benchdata

COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=6250)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--probes", type=int, default=8)
    ap.add_argument("--num", type=int, default=9)
    ap.add_argument("--den", type=int, default=10)
    ap.add_argument("--min-union", type=int, default=8)
    ap.add_argument("--trace", choices=["clusters"])
    args = ap.parse_args()
    n = args.contigs
    lengths, gcs, seeds = benchdata.config4_spec(n * 16)            # every 16th contig of the 100 000 x 20 kbp job: one rank's share
    seqs = [benchdata.synthetic_contig(int(a), float(b), int(c)) for a, b, c in zip(lengths[::16], gcs[::16], seeds[::16])]
    seqs += [s.translate(COMPLEMENT)[::-1] for s in seqs]
    ctx = _cabi.Context(0)
    ctx.set_models([b for _, b in benchdata.load_model_set()])
    dev = torch.device("cuda", 0)
    batch = ctx.upload(seqs)
    res = ctx.find_genes(batch, meta=True)
    spec = ProteinClusters(ProteinSketches(args.k, args.size), args.probes, (args.num, args.den), args.min_union)
    ds = ctx.protein_sketches(batch, res, spec.sketches)
    G, s, P = ds.n, args.size, args.probes
    num, den = spec.min_resemblance

    if args.trace == "clusters":
        for _ in range(3):
            dc = ds.cluster(spec)
        print(json.dumps({"trace": "clusters", "contigs": len(seqs), "genes": G, "size": s, "probes": P, **ctx.cluster_stats()}))
        return

    ids = torch.arange(G, dtype=torch.int64, device=dev)
    # (weight, -index) in one int64: the windows of a record are far below 2^31
    packed = ds.windows * G + (G - 1 - ids)

    def route_a():
        t0 = time.perf_counter()
        valid = torch.arange(P, device=dev)[None, :] < ds.counts.clamp(0, s).clamp(max=P)[:, None]
        h = ds.sketches[:, :P][valid]                                # row-major: ascending record index
        g = ids[:, None].expand(G, P)[valid]
        h, order = torch.sort(h, stable=True)
        g = g[order]
        head = torch.ones_like(h, dtype=torch.bool)
        head[1:] = h[1:] != h[:-1]
        bucket = torch.cumsum(head, 0) - 1
        best = torch.full((int(bucket[-1]) + 1,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, bucket, packed[g], "amax")
        c = (G - 1 - best % G)[bucket]
        member = c != g
        lo, hi = torch.minimum(c, g)[member], torch.maximum(c, g)[member]
        key = torch.unique(lo * G + hi)                              # sorted: ascending (a, b)
        pairs = torch.stack([key // G, key % G], dim=1).contiguous()
        t1 = time.perf_counter()
        shared, m = ds.compare(pairs)
        ok = (m >= max(spec.min_union, 1)) & (shared * den >= num * m)
        edges, eshared, eunion = pairs[ok], shared[ok], m[ok]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        label, rounds = ids.clone(), 0
        a, b = edges[:, 0], edges[:, 1]
        while True:
            low = torch.minimum(label[a], label[b])
            new = label.scatter_reduce(0, a, low, "amin").scatter_reduce(0, b, low, "amin")
            rounds += 1
            if bool(torch.equal(new, label)):
                break
            label = new
        root = label == ids
        number = torch.cumsum(root, 0) - 1
        cluster = number[label]
        U = int(number[-1]) + 1
        rep = G - 1 - torch.full((U,), -1, dtype=torch.int64, device=dev).scatter_reduce(0, cluster, packed, "amax") % G
        sizes = torch.bincount(cluster, minlength=U)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return ((cluster, rep, sizes, edges, eshared, eunion), int(pairs.shape[0]), rounds,
                {"candidates": t1 - t0, "compare and threshold": t2 - t1, "components and numbering": t3 - t2, "total": t3 - t0})

    C = G * P
    outs = tuple(torch.empty(shape, dtype=torch.int64, device=dev) for shape in ((G,), (G,), (G,), (C, 2), (C,), (C,)))

    def route_b(given=False):
        """`given`: with the six tensors in hand, as a caller in a loop has them"""
        t0 = time.perf_counter()
        dc = ds.cluster(spec, out=outs) if given else ds.cluster(spec)
        t1 = time.perf_counter()
        return dc, {"total": t1 - t0}

    times = {}

    def note(key, t):
        for part, v in t.items():
            times.setdefault(key, {}).setdefault(part, []).append(1e3 * v)

    names = ("cluster", "representatives", "sizes", "edges", "edge_shared", "edge_union")
    for rnd in range(args.warmup + args.rounds):
        keep = rnd >= args.warmup
        dc, tb = route_b()
        got, candidates, rounds, ta = route_a()
        for name, x in zip(names, got):
            assert bool(torch.equal(getattr(dc, name), x)), "the routes differ on %s" % name
        found = ctx.cluster_stats()
        assert found["candidates"] == candidates and found["edges"] == dc.n_edges == int(got[3].shape[0]) and found["clusters"] == dc.n_clusters
        again, tg = route_b(given=True)
        for name in names:
            assert bool(torch.equal(getattr(again, name), getattr(dc, name))), name
        if keep:
            note("a/torch", ta)
            note("b/cluster", tb)
            note("b/cluster, tensors given", tg)
        largest = int(dc.sizes.max())
        del dc, got
        print("round %d of %d" % (rnd + 1, args.warmup + args.rounds), file=sys.stderr, flush=True)
    result = {"contigs": len(seqs), "genes": G, "k": args.k, "size": s, "probes": P, "min_resemblance": [num, den], "min_union": spec.min_union,
              **found, "largest_cluster": largest, "torch_rounds": rounds, "rounds": args.rounds, "routes_agree": True,
              "device": ctx.device_info()["name"],
              "ms": {key: {part: stats(v) for part, v in parts.items()} for key, parts in times.items()}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
