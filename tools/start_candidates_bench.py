"""Every gene's candidate start sites left on the device: what `Context.start_candidates` saves over the detour through the host
(DESIGN.md 4.17).

One context, meta mode under `benchdata.load_model_set()`, the 6 250 x 20 kbp batch of tools/device_input_bench.py.  `find_genes`
runs outside the clock, once with `want_nodes=True`: its node arrays are on the host for route (a) and on the device for route (b).
Only the step behind it is timed, for a consumer that wants positions, types and all seven score columns of every candidate of every
gene as torch tensors (int64 / float32, ragged):
  route (a), the detour, vectorised: the per-contig node arrays joined, the start nodes sorted by (contig, stop_val, strand) with a
             stable numpy sort, every gene's group by two searches, the rows expanded at once and gathered -- no Python loop over
             genes or candidates -- and the upload of the three tensors;
  route (b): `start_candidates` -- plan, write and `torch.empty`.
3 warm-up rounds, then 15 rounds that alternate between the routes; min / median / max per part.  Both routes must give the same
tensors in every round (asserted).  What a find costs with the arena kept on the device (`want_nodes="device"`) and with the nodes
brought home (`want_nodes=True`) over a plain one is timed in alternating rounds as well.

`--trace starts` makes three calls of four instances of the write kernel and of `k_gene_windows` (int64 and uint8, ragged) on the
same genes, for a kernel trace; `--trace plain` makes three plain `find_genes` + `translate_genes` calls, for a kernel list that can be
compared by name and count with the one before this feature.  `--profile DIR` runs `--trace starts` in a child process under
`rocprofv3 --kernel-trace --stats` (no counters) and prints the rows of the two kernels, the sort and `k_gene_windows` with the bytes
each call wrote.

    python tools/start_candidates_bench.py [--contigs 6250] [--rounds 15] [--trace starts|plain] [--profile DIR]"""
import argparse
import glob
import json
import os
import sqlite3
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("total", "cscore", "sscore", "rscore", "uscore", "tscore", "gc_cont")
TRACE_CASES = (("int64", "float32", "ragged"), ("int64", "float32", "padded"), ("int32", "float64", "ragged"), ("int32", "float64", "padded"))


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3)}


def profile(args):
    """A child under rocprofv3 (this process has not touched the GPU), then the rows that matter of its kernel statistics."""
    os.makedirs(args.profile, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", args.profile, "-o", "start_candidates", "--", sys.executable, os.path.abspath(__file__),
           "--trace", "starts", "--contigs", str(args.contigs)]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=300)     # (a run takes under a minute)
    if done.returncode != 0:
        sys.exit("rocprofv3 ended with %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:]))
    info = json.loads([line for line in done.stdout.splitlines() if line.startswith("{")][-1])
    rows = []
    for path in glob.glob(os.path.join(args.profile, "**", "*_results.db"), recursive=True):       # rocprofv3's database: its `kernels` view
        db = sqlite3.connect(path)
        for name, calls, total, avg, lo, hi in db.execute("select name, count(*), sum(duration), avg(duration), min(duration), max(duration) "
                                                          "from kernels group by name"):
            if any(k in name for k in ("k_start_candidates", "k_start_lookup", "k_start_nodes", "k_sco_keys", "k_sco_bounds", "radix_sort",
                                       "k_gene_windows")):
                rows.append({"name": name, "calls": calls, "total_ns": total, "average_ns": avg, "min_ns": lo, "max_ns": hi})
        db.close()
    print(json.dumps({"profile": info, "kernels": sorted(rows, key=lambda r: r["name"])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=6250)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", choices=["starts", "plain"])
    ap.add_argument("--profile", metavar="DIR")
    args = ap.parse_args()
    if args.profile:
        return profile(args)

    import torch                 # first: the library then binds to the HIP runtime of torch's wheel
    import numpy as np
    sys.path.insert(0, ROOT)
    from pyrodigal_amd import _cabi, benchdata

    n = args.contigs
    lengths, gcs, seeds = benchdata.config4_spec(n * 16)            # every 16th contig of the 100 000 x 20 kbp job: one rank's share
    seqs = [benchdata.synthetic_contig(int(a), float(b), int(c)) for a, b, c in zip(lengths[::16], gcs[::16], seeds[::16])]
    ctx = _cabi.Context(0)
    ctx.set_models([b for _, b in benchdata.load_model_set()])
    dev = torch.device("cuda", 0)
    batch = ctx.upload(seqs)

    if args.trace == "plain":
        res = ctx.find_genes(batch, meta=True)
        for _ in range(3):
            ctx.translate_genes(batch, ctx.find_genes(batch, meta=True))
        print(json.dumps({"trace": "plain", "contigs": n, "genes": int(len(res.genes))}))
        return

    if args.trace == "starts":
        res = ctx.find_genes(batch, meta=True, want_nodes="device")
        written = {}
        for _ in range(3):
            for index_dtype, dtype, layout in TRACE_CASES:
                pad = dict(pad=-1, score_pad=0.0) if layout == "padded" else {}
                ds = ctx.start_candidates(batch, res, _cabi.StartCandidates(FIELDS, dtype=dtype, index_dtype=index_dtype, layout=layout, **pad))
                written["k_start_candidates/%s/%s/%s" % (index_dtype, dtype, layout)] = \
                    2 * ds.positions.numel() * ds.positions.element_size() + ds.scores.numel() * ds.scores.element_size()
                candidates = int(ds.lengths.sum())
                del ds
            for dtype in ("int64", "uint8"):
                w = ctx.gene_windows(batch, res, _cabi.GeneWindows(dtype=dtype, layout="ragged"))
                written["k_gene_windows/%s/ragged" % dtype] = w.tokens.numel() * w.tokens.element_size()
                del w
        nodes = int(sum(c["n_nodes"] for c in res.contigs))
        print(json.dumps({"trace": "starts", "contigs": n, "genes": int(len(res.genes)), "candidates": candidates, "nodes": nodes,
                          "bytes_written_per_call": written}))
        return

    # ---- what a find costs with the nodes kept or brought home ----
    find_ms = {"plain": [], "device": [], "host": []}
    for rnd in range(2 + 5):
        for name, wn in (("plain", False), ("device", "device"), ("host", True)):
            t0 = time.perf_counter()
            r = ctx.find_genes(batch, meta=True, want_nodes=wn)
            if rnd >= 2:
                find_ms[name].append(1e3 * (time.perf_counter() - t0))
            del r
    res = ctx.find_genes(batch, meta=True, want_nodes=True)          # outside the clock: nodes on the host and on the device
    genes = np.ascontiguousarray(res.genes)
    spec = _cabi.StartCandidates(FIELDS, dtype="float32", index_dtype="int64", layout="ragged")
    NC = len(res.nodes)

    def route_host():
        """(a): the grouping of tests/start_candidates_ref.py with numpy over the host's node arrays, and the upload."""
        t0 = time.perf_counter()
        counts = np.array([nd["n"] for nd in res.nodes], np.int64)
        first = np.concatenate([[0], np.cumsum(counts)])
        col = {k: np.concatenate([nd[k] for nd in res.nodes]) for k in ("ndx", "stop_val", "type", "strand", "edge", "cscore", "sscore", "rscore",
                                                                       "uscore", "tscore", "gc_cont")}
        t1 = time.perf_counter()
        contig = np.repeat(np.arange(NC, dtype=np.int64), counts)
        key = (contig << 34) | ((col["stop_val"].astype(np.int64) + 16) << 1) | (col["strand"] != 1)
        starts = np.nonzero(col["type"] != 3)[0]
        order = starts[np.argsort(key[starts], kind="stable")]          # stable: ndx order within a key
        skey = key[order]
        x = first[genes["contig"]] + genes["start_ndx"]
        lo, hi = np.searchsorted(skey, key[x], "left"), np.searchsorted(skey, key[x], "right")
        cnt = hi - lo
        ends = np.cumsum(cnt)
        k = np.arange(int(ends[-1]), dtype=np.int64) - np.repeat(ends - cnt, cnt)
        fwd = np.repeat(genes["strand"] == 1, cnt)
        y = order[np.where(fwd, np.repeat(lo, cnt) + k, np.repeat(hi, cnt) - 1 - k)]
        t2 = time.perf_counter()
        pos = col["ndx"][y].astype(np.int64) + 1
        typ = np.where(col["edge"][y] != 0, 3, col["type"][y] & 3).astype(np.int64)
        sco = np.stack([col["cscore"][y] + col["sscore"][y], col["cscore"][y], col["sscore"][y], col["rscore"][y], col["uscore"][y],
                        col["tscore"][y], col["gc_cont"][y].astype(np.float64)], axis=1).astype(np.float32)
        t3 = time.perf_counter()
        out = tuple(torch.from_numpy(a).to(dev) for a in (pos, typ, sco))
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        return out, {"join": t1 - t0, "group": t2 - t1, "gather": t3 - t2, "upload": t4 - t3, "total": t4 - t0}

    def route_device():
        """(b): the tensors are written where they are wanted."""
        t0 = time.perf_counter()
        ds = ctx.start_candidates(batch, genes, spec)
        t1 = time.perf_counter()
        return (ds.positions, ds.types, ds.scores), {"start_candidates": t1 - t0, "total": t1 - t0}

    times = {"a": {}, "b": {}}
    candidates = 0
    for rnd in range(args.warmup + args.rounds):
        a, ta = route_host()
        b, tb = route_device()
        for u, v in zip(a, b):
            assert u.shape == v.shape and u.dtype == v.dtype and bool(torch.equal(u, v)), "the two routes differ"
        candidates = int(b[0].numel())
        del a, b
        if rnd >= args.warmup:
            for route, t in (("a", ta), ("b", tb)):
                for part, v in t.items():
                    times[route].setdefault(part, []).append(1e3 * v)
        print("round %d of %d" % (rnd + 1, args.warmup + args.rounds), file=sys.stderr, flush=True)
    # where the time of (b) goes: the two library calls through ctypes alone, on tensors made beforehand
    import ctypes
    count, chosen = np.zeros(len(genes), np.int32), np.zeros(len(genes), np.int32)
    out = (torch.empty(candidates, dtype=torch.int64, device=dev), torch.empty(candidates, dtype=torch.int64, device=dev),
           torch.empty((candidates, 7), dtype=torch.float32, device=dev))
    o = spec.opts()
    plan_ms, write_ms = [], []
    for _ in range(args.rounds):
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        rc = ctx.L.pga_start_plan_create(ctx.h, batch.h, len(genes), genes.ctypes.data, ctypes.byref(h), count.ctypes.data, chosen.ctypes.data)
        t1 = time.perf_counter()
        assert rc == 0
        rc = ctx.L.pga_start_plan_write(ctx.h, h, ctypes.byref(o), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), candidates, candidates,
                                        7 * candidates, None)
        t2 = time.perf_counter()
        assert rc == 0
        ctx.L.pga_start_plan_free(ctx.h, h)
        plan_ms.append(1e3 * (t1 - t0)); write_ms.append(1e3 * (t2 - t1))
    print(json.dumps({"contigs": n, "genes": int(len(genes)), "candidates": candidates, "nodes": int(sum(nd["n"] for nd in res.nodes)),
                      "rounds": args.rounds, "tensors_identical": True, "device": ctx.device_info()["name"],
                      "ms": {r: {part: stats(v) for part, v in parts.items()} for r, parts in times.items()},
                      "library_plan_create_ms": stats(plan_ms), "library_plan_write_ms": stats(write_ms),
                      "find_genes_ms": {k: stats(v) for k, v in find_ms.items()}}))


if __name__ == "__main__":
    main()
