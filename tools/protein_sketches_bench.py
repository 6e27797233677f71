"""MinHash sketches of the predicted proteins on the device: what `Context.protein_sketches` saves over the routes a caller had before
(DESIGN.md 4.20).

One context, meta mode under `benchdata.load_model_set()`.  The batch is that of tools/protein_groups_bench.py: the 6 250 x 20 kbp batch
of tools/device_input_bench.py with every contig present a second time, reverse-complemented (12 500 contigs).  `find_genes` runs once,
outside the clock (its gene records are on the host for every route); only the step behind it is timed, on the host clock:
  route (a): `translate_tokens` into a padded uint8 `[G, W]` tensor (the letters as ids, pad 0), then in torch `unfold` into windows,
             the keys and hashes of all `G x (W - k + 1)` windows (int64 arithmetic wraps as the rule's does), a sort of every row, the
             duplicates of a row pushed behind by a second sort, and the first `size` columns;
  route (b): `translate_genes` -- every letter to the host --, the hashes of all windows in one numpy pass and `np.unique` per protein
             (`ProteinSketches.sketch_of` vectorised; checked against it on the first proteins);
  route (c): `protein_sketches` -- and once more with the contigs' tables and the three tensors given, which leaves the library's own
             host work and the device.
Warm-up rounds, then rounds that alternate between the routes; min / median / max.  The three routes must give the same sketches,
counts and windows in every round (asserted).

`--trace sketches` makes three calls of `protein_sketches` and of `protein_groups` in both units (`k_string_digest` reads the same
letters) and three of `DeviceSketches.compare` over 1 000 000 random pairs, for a kernel trace of its own; with a library built with
`-DPGA_SKETCH_COUNT_PASSES` it also prints the hashes behind a record's first 64 windows that passed the record's threshold, next to
what `s ln(n / 64)` expects (and `s + s ln(n / s)`, what inserting every window from the first on would try).

    python tools/protein_sketches_bench.py [--contigs 6250] [--rounds 7] [--warmup 1] [--k 5] [--size 32] [--gene-k 21]
                                           [--skip-torch] [--skip-host] [--trace sketches]"""
import argparse
import json
import os
import sys
import time

import torch                     # first: the library then binds to the HIP runtime of torch's wheel
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrodigal_amd import ProteinGroups, ProteinSketches, ProteinTokens, _cabi, benchdata

COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
INT64_MAX = (1 << 63) - 1


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3)}


def signed(c):
    return c - (1 << 64) if c >= 1 << 63 else c


def torch_hash(x, seed):
    """the rule's hash over an int64 tensor of keys: two's-complement arithmetic wraps, and >> is made logical by a mask"""
    shr = lambda z, n: (z >> n) & ((1 << (64 - n)) - 1)       # noqa: E731
    z = x + signed(((seed + 1) * 0x9E3779B97F4A7C15) & ((1 << 64) - 1))
    z = (z ^ shr(z, 30)) * signed(0xBF58476D1CE4E5B9)
    z = (z ^ shr(z, 27)) * signed(0x94D049BB133111EB)
    z = z ^ shr(z, 31)
    return shr(z, 1)


def numpy_hash(x, seed):
    with np.errstate(over="ignore"):
        z = x + np.uint64(((seed + 1) * 0x9E3779B97F4A7C15) & ((1 << 64) - 1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(1)).astype(np.int64)


def expected_passes(windows, s, ranked=64):
    """the insertions a record of n distinct uniformly hashed windows is expected to try: window j is among the s smallest of the first j
    with probability min(1, s / j) -- s + s ln(n / s) in all; the first `ranked` windows are ranked, not inserted, which leaves
    s ln(n / ranked) for s <= ranked"""
    n = np.asarray(windows, np.float64)
    plain = np.where(n > s, s + s * np.log(np.maximum(n, 1) / s), n)
    first = np.minimum(n, ranked)
    return float((plain - np.where(first > s, s + s * np.log(np.maximum(first, 1) / s), first)).sum()), float(plain.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=6250)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--size", type=int, default=32)
    ap.add_argument("--gene-k", type=int, default=21)
    ap.add_argument("--skip-torch", action="store_true", help="leave route (a) out (it holds G x W x k int64 keys)")
    ap.add_argument("--skip-host", action="store_true", help="leave route (b) out")
    ap.add_argument("--trace", choices=["sketches"])
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
    genes = np.ascontiguousarray(res.genes)
    G = len(genes)
    residues = int(_cabi._residue_counts(genes, False).sum())
    gene_bases = int((genes["end"].astype(np.int64) - genes["begin"] + 1).sum())
    k, s = args.k, args.size
    spec = ProteinSketches(k, s)
    gene_spec = ProteinSketches(args.gene_k, s, "gene")
    letters = ProteinTokens({chr(c): c for c in range(1, 128)}, dtype="uint8", layout="padded")

    if args.trace == "sketches":
        pairs = torch.from_numpy(np.random.default_rng(1).integers(0, G, size=(1_000_000, 2))).to(dev)
        out = {"trace": "sketches", "contigs": len(seqs), "genes": G, "residues": residues, "gene_bases": gene_bases, "k": k, "size": s,
               "gene_k": args.gene_k, "pairs": int(pairs.shape[0])}
        for _ in range(3):
            ds = ctx.protein_sketches(batch, res, spec)
            passes = ctx.protein_sketch_passes()
            dg = ctx.protein_sketches(batch, res, gene_spec)
            gene_passes = ctx.protein_sketch_passes()
            ctx.protein_groups(batch, res, ProteinGroups())
            ctx.protein_groups(batch, res, ProteinGroups("gene"))
            shared, union = ds.compare(pairs)
        for name, d, p in (("protein", ds, passes), ("gene", dg, gene_passes)):
            w = d.windows.cpu().numpy()
            behind, plain = expected_passes(w, s)
            out[name] = {"windows": int(w.sum()), "passes": p, "expected_passes": round(behind), "expected_passes_without_ranking": round(plain),
                         "share_of_windows": None if p < 0 else round(p / max(int(w.sum()), 1), 5)}
        out["pairs_with_a_shared_hash"] = int((shared > 0).sum())
        print(json.dumps(out))
        return

    shifts = torch.tensor([8 * (k - 1 - i) for i in range(k)], dtype=torch.int64, device=dev)

    def route_a():
        t0 = time.perf_counter()
        dp = ctx.translate_tokens(batch, res, letters)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        win = dp.tokens.unfold(1, k, 1)                                                        # [G, W - k + 1, k], a view
        valid = ((win != 0) & (win != ord(spec.unknown_residue))).all(dim=2)
        keys = (win.to(torch.int64) << shifts).sum(dim=2)
        h = torch.where(valid, torch_hash(keys, spec.seed), torch.full_like(keys, INT64_MAX))
        del keys, win
        windows = valid.sum(dim=1)
        h, _ = torch.sort(h, dim=1)
        dup = torch.zeros_like(h, dtype=torch.bool)
        dup[:, 1:] = h[:, 1:] == h[:, :-1]
        h = torch.where(dup, torch.full_like(h, INT64_MAX), h)
        h, _ = torch.sort(h, dim=1)
        sketch = h[:, :s].contiguous()
        count = (sketch != INT64_MAX).sum(dim=1)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (sketch, count, windows, tuple(dp.tokens.shape)), {"translate_tokens": t1 - t0, "torch": t2 - t1, "total": t2 - t0}

    skip = np.zeros(256, bool)
    skip[ord(spec.unknown_residue)] = True
    skip[128:] = True

    def route_b():
        t0 = time.perf_counter()
        prot, off = ctx.translate_genes(batch, res, include_stop=False)
        t1 = time.perf_counter()
        off = np.asarray(off, np.int64)
        total = int(off[G])
        data = np.asarray(prot[:total], np.uint8)
        nw = max(total - k + 1, 0)
        keys = np.zeros(nw, np.uint64)
        bad = np.zeros(nw, bool)
        for i in range(k):
            part = data[i:i + nw]
            keys = (keys << np.uint64(8)) | part.astype(np.uint64)
            bad |= skip[part]
        # (a window that begins within k - 1 letters of its protein's end runs into the next one: no protein's range below holds it)
        h = numpy_hash(keys, spec.seed)
        h[bad] = INT64_MAX
        good = np.concatenate([[0], np.cumsum(~bad)])
        sketch = np.full((G, s), INT64_MAX, np.int64)
        count, windows = np.zeros(G, np.int64), np.zeros(G, np.int64)
        for g in range(G):
            lo, hi = int(off[g]), max(int(off[g + 1]) - k + 1, int(off[g]))
            hi = min(hi, nw)
            if hi <= lo:
                continue
            windows[g] = good[hi] - good[lo]
            u = np.unique(h[lo:hi])[:s]
            if windows[g] < hi - lo:
                u = u[u != INT64_MAX]
            sketch[g, :len(u)] = u
            count[g] = len(u)
        t2 = time.perf_counter()
        return (sketch, count, windows, data, off), {"translate_genes": t1 - t0, "numpy": t2 - t1, "total": t2 - t0}

    tables = np.array(_cabi._default_tables(ctx, res.contigs), np.int32)
    outs = (torch.empty((G, s), dtype=torch.int64, device=dev), torch.empty(G, dtype=torch.int64, device=dev), torch.empty(G, dtype=torch.int64, device=dev))

    def route_c(given=False):
        """`given`: with the tables of the contigs and the three tensors in hand, as a caller in a loop has them"""
        t0 = time.perf_counter()
        ds = ctx.protein_sketches(batch, genes, spec, tables=tables, out=outs) if given else ctx.protein_sketches(batch, res, spec)
        t1 = time.perf_counter()
        return ds, {"total": t1 - t0}

    times = {}

    def note(key, t):
        for part, v in t.items():
            times.setdefault(key, {}).setdefault(part, []).append(1e3 * v)

    shape = None
    for rnd in range(args.warmup + args.rounds):
        keep = rnd >= args.warmup
        ds, tc = route_c()
        if not args.skip_host:
            (sk_b, cnt_b, win_b, data, off), tb = route_b()
            if rnd == 0:                                            # the vectorised host route is sketch_of
                for g in range(min(G, 200)):
                    row, w = spec.sketch_of(data[off[g]:off[g + 1]].tobytes())
                    assert (sk_b[g, :cnt_b[g]].tolist(), int(win_b[g])) == (row, w), "route (b) is not sketch_of at gene %d" % g
            assert bool(torch.equal(ds.sketches, torch.from_numpy(sk_b).to(dev))), "routes (b) and (c) differ on the sketches"
            assert bool(torch.equal(ds.counts, torch.from_numpy(cnt_b).to(dev))) and bool(torch.equal(ds.windows, torch.from_numpy(win_b).to(dev)))
            if keep:
                note("b/numpy", tb)
        if not args.skip_torch:
            (sk_a, cnt_a, win_a, shape), ta = route_a()
            assert bool(torch.equal(ds.sketches, sk_a)), "routes (a) and (c) differ on the sketches"
            assert bool(torch.equal(ds.counts, cnt_a)) and bool(torch.equal(ds.windows, win_a)), "routes (a) and (c) differ on the counts"
            del sk_a, cnt_a, win_a
            if keep:
                note("a/torch", ta)
        again, tg = route_c(given=True)
        assert bool(torch.equal(again.sketches, ds.sketches)) and bool(torch.equal(again.counts, ds.counts))
        if keep:
            note("c/protein_sketches", tc)
            note("c/protein_sketches, tables and tensors given", tg)
        full = int((ds.counts == s).sum())
        del ds
        print("round %d of %d" % (rnd + 1, args.warmup + args.rounds), file=sys.stderr, flush=True)
    result = {"contigs": len(seqs), "genes": G, "residues": residues, "k": k, "size": s, "full_sketches": full, "padded_shape": shape,
              "rounds": args.rounds, "routes_agree": True, "device": ctx.device_info()["name"],
              "ms": {key: {part: stats(v) for part, v in parts.items()} for key, parts in times.items()}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
