"""Proteins left on the device as token tensors: what `Context.translate_tokens` saves over the detour through the host
(DESIGN.md 4.14).

One context, meta mode under `benchdata.load_model_set()`, the 6 250 x 20 kbp batch of tools/device_input_bench.py.  `find_genes`
runs once, outside the clock; only the step behind it is timed, for a consumer that wants the proteins as token ids in a torch tensor:
  route (a), what the library offered before: `translate_genes` (letters come home), the numpy vocabulary map, BOS / EOS and the
             padding or the ragged concatenation, and the upload of the tensor;
  route (b): `translate_tokens` into a torch tensor it allocates.
Three cases: int64 padded, int64 ragged, uint8 ragged.  3 warm-up rounds, then 15 rounds that alternate between the routes; min /
median / max per part.  Both routes must give the same tensor in every round (asserted).

`--trace tokens` makes three calls of every `k_translate_tokens` case and of `translate_genes` (k_translate) on the same genes, for a
kernel trace of its own; `--trace plain` makes three plain `find_genes` + `translate_genes` calls, for a kernel list that can be
compared by name and count with the one before this feature.

    python tools/protein_tokens_bench.py [--contigs 6250] [--rounds 15] [--trace tokens|plain]"""
import argparse
import json
import os
import sys
import time

import torch                     # first: the library then binds to the HIP runtime of torch's wheel
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrodigal_amd import ProteinTokens, _cabi, benchdata

VOCAB = "-ACDEFGHIKLMNPQRSTVWYX*"        # id = position; '-' (0) is the pad
BOS, EOS, PAD = 30, 31, 0
CASES = (("int64", "padded"), ("int64", "ragged"), ("uint8", "ragged"))


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=6250)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", choices=["tokens", "plain"])
    args = ap.parse_args()
    n = args.contigs
    lengths, gcs, seeds = benchdata.config4_spec(n * 16)            # every 16th contig of the 100 000 x 20 kbp job: one rank's share
    seqs = [benchdata.synthetic_contig(int(a), float(b), int(c)) for a, b, c in zip(lengths[::16], gcs[::16], seeds[::16])]
    ctx = _cabi.Context(0)
    ctx.set_models([b for _, b in benchdata.load_model_set()])
    dev = torch.device("cuda", 0)
    batch = ctx.upload(seqs)
    res = ctx.find_genes(batch, meta=True)
    index = np.zeros(128, np.int64)
    index[np.frombuffer(VOCAB.encode(), np.uint8)] = np.arange(len(VOCAB))

    if args.trace == "plain":
        for _ in range(3):
            ctx.translate_genes(batch, ctx.find_genes(batch, meta=True))
        print(json.dumps({"trace": "plain", "contigs": n, "genes": int(len(res.genes))}))
        return

    def route_host(dtype, layout):
        """(a): letters home, numpy map and layout, upload."""
        t0 = time.perf_counter()
        letters, off = ctx.translate_genes(batch, res, include_stop=False)
        t1 = time.perf_counter()
        ids = index[letters]                                           # int64, as the consumer's embedding wants them
        g = len(off) - 1
        lens = np.diff(off) + 2
        if layout == "padded":
            host = np.full((g, int(lens.max())), PAD, np.int64)
            row = np.repeat(np.arange(g), lens - 2)
            col = np.arange(len(ids)) - np.repeat(off[:-1], lens - 2) + 1
            host[row, col] = ids
            host[:, 0] = BOS
            host[np.arange(g), lens - 1] = EOS
        else:
            start = off[:-1] + 2 * np.arange(g)                        # gene g begins 2 g elements later than its letters
            host = np.empty(len(ids) + 2 * g, np.int64)
            host[np.arange(len(ids)) + np.repeat(2 * np.arange(g) + 1, lens - 2)] = ids
            host[start] = BOS
            host[start + lens - 1] = EOS
        host = host.astype(getattr(np, dtype), copy=False)
        t2 = time.perf_counter()
        out = torch.from_numpy(host).to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return out, {"translate_genes": t1 - t0, "numpy": t2 - t1, "upload": t3 - t2, "total": t3 - t0}

    specs = {c: ProteinTokens(VOCAB, bos=BOS, eos=EOS, pad=PAD, dtype=c[0], layout=c[1]) for c in CASES}

    def route_device(dtype, layout):
        """(b): the tokens are written where they are wanted."""
        t0 = time.perf_counter()
        dp = ctx.translate_tokens(batch, res, specs[(dtype, layout)])
        t1 = time.perf_counter()
        return dp.tokens, {"translate_tokens": t1 - t0, "total": t1 - t0}

    if args.trace == "tokens":
        for _ in range(3):
            ctx.translate_genes(batch, res, include_stop=False)
            for case in CASES:
                route_device(*case)
        print(json.dumps({"trace": "tokens", "contigs": n, "genes": int(len(res.genes))}))
        return

    times = {(r, c): {} for r in ("a", "b") for c in CASES}
    elems = {}
    for rnd in range(args.warmup + args.rounds):
        for case in CASES:
            a, ta = route_host(*case)
            b, tb = route_device(*case)
            assert a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b)), "the two routes differ: %s %s" % case
            elems[case] = int(b.numel())
            if rnd >= args.warmup:
                for route, t in (("a", ta), ("b", tb)):
                    for k, v in t.items():
                        times[(route, case)].setdefault(k, []).append(1e3 * v)
    out = {"contigs": n, "genes": int(len(res.genes)), "rounds": args.rounds, "tensors_identical": True, "device": ctx.device_info()["name"],
           "elements": {"%s/%s" % c: v for c, v in elems.items()},
           "ms": {"%s/%s/%s" % ((r,) + c): {part: stats(v) for part, v in parts.items()} for (r, c), parts in times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
