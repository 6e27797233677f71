"""Cluster edges verified by banded edit distance on the device: what `DeviceProteins.align` and `DeviceClusters.relink` cost on the
edges of a large batch, and what `find_verified_clusters_batch` costs over `find_clusters_batch`.

One context, meta mode under `benchdata.load_model_set()`.  The batch is that of tools/protein_clusters_bench.py: the 6 250 x 20 kbp
batch of tools/device_input_bench.py with every contig present a second time, reverse-complemented (12 500 contigs).  `find_genes`,
`translate_tokens`, `protein_sketches` and `DeviceSketches.cluster` run once, outside the clock; then, on the host clock:
  align:   `DeviceProteins.align(edges, ProteinAlignments())` over the edges of the default `ProteinClusters`;
  relink:  `DeviceClusters.relink(keep=passed)`;
  finder:  `GeneFinder.find_verified_clusters_batch` against `GeneFinder.find_clusters_batch` on the same sequences, in turn.
Warm-up rounds, then the timed rounds; min / median / max.  The JSON line also gives `Context.align_stats`, the edges that passed
and the clusters before and after.

`--trace align` makes three calls of `align` and of `relink`, for a kernel trace of its own.

    python tools/protein_alignments_bench.py [--contigs 6250] [--rounds 7] [--warmup 1] [--max-distance 32] [--num 9] [--den 10]
                                             [--no-finder] [--trace align]"""
import argparse
import json
import os
import sys
import time

import torch                     # first: the library then binds to the HIP runtime of torch's wheel

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrodigal_amd import ProteinAlignments, ProteinClusters, VerifiedClusters, _cabi, benchdata

COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=6250)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-distance", type=int, default=32)
    ap.add_argument("--num", type=int, default=9)
    ap.add_argument("--den", type=int, default=10)
    ap.add_argument("--no-finder", action="store_true")
    ap.add_argument("--trace", choices=["align"])
    args = ap.parse_args()
    n = args.contigs
    lengths, gcs, seeds = benchdata.config4_spec(n * 16)            # every 16th contig of the 100 000 x 20 kbp job: one rank's share
    seqs = [benchdata.synthetic_contig(int(a), float(b), int(c)) for a, b, c in zip(lengths[::16], gcs[::16], seeds[::16])]
    seqs += [s.translate(COMPLEMENT)[::-1] for s in seqs]
    spec = VerifiedClusters(ProteinClusters(), ProteinAlignments(args.max_distance, (args.num, args.den)))
    ctx = _cabi.Context(0)
    ctx.set_models([b for _, b in benchdata.load_model_set()])
    batch = ctx.upload(seqs)
    res = ctx.find_genes(batch, meta=True)
    proteins = ctx.translate_tokens(batch, res, spec.tokens)
    ds = ctx.protein_sketches(batch, res, spec.clusters.sketches)
    dc = ds.cluster(spec.clusters)
    E = dc.n_edges

    if args.trace == "align":
        for _ in range(3):
            distance, passed = proteins.align(dc.edges, spec.alignments)
            dc.relink(passed)
        print(json.dumps({"trace": "align", "contigs": len(seqs), "genes": ds.n, "edges": E, **ctx.align_stats()}))
        return

    times = {"align": [], "relink": []}
    out_a = tuple(torch.empty(E, dtype=torch.int64, device="cuda") for _ in range(2))
    out_r = tuple(torch.empty(ds.n, dtype=torch.int64, device="cuda") for _ in range(3))
    for rnd in range(args.warmup + args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        distance, passed = proteins.align(dc.edges, spec.alignments, out=out_a)
        t1 = time.perf_counter()
        cluster, reps, sizes, U, used = dc.relink(passed, out=out_r)
        t2 = time.perf_counter()
        if rnd >= args.warmup:
            times["align"].append(1e3 * (t1 - t0))
            times["relink"].append(1e3 * (t2 - t1))
    found = ctx.align_stats()
    assert found["pairs"] == E and used == found["passed"] == int(passed.sum())
    result = {"contigs": len(seqs), "genes": ds.n, "edges": E, "max_distance": args.max_distance, "min_identity": [args.num, args.den], **found,
              "clusters_before": dc.n_clusters, "clusters_after": U, "mean_tokens": round(float(proteins.lengths.mean()), 1),
              "distance_histogram": torch.bincount(distance.clamp(min=0), minlength=args.max_distance + 2).tolist(),
              "rounds": args.rounds, "device": ctx.device_info()["name"]}
    del batch
    ctx.close()

    if not args.no_finder:
        from pyrodigal_amd import lib
        bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), name) for name, b in benchdata.load_model_set()])
        finder = lib.GeneFinder(meta=True, metagenomic_bins=bins)
        times["find_clusters_batch"], times["find_verified_clusters_batch"] = [], []
        for rnd in range(args.warmup + args.rounds):
            for key, call, rule in (("find_clusters_batch", finder.find_clusters_batch, spec.clusters),
                                    ("find_verified_clusters_batch", finder.find_verified_clusters_batch, spec)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                genes, got = call(seqs, rule)
                t1 = time.perf_counter()
                if rnd >= args.warmup:
                    times[key].append(1e3 * (t1 - t0))
                if key == "find_verified_clusters_batch":
                    assert (got.n_clusters, got.n_passed, got.candidates.n_edges) == (U, used, E)
                del genes, got
            print("round %d of %d" % (rnd + 1, args.warmup + args.rounds), file=sys.stderr, flush=True)
    result["ms"] = {key: stats(v) for key, v in times.items()}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
