"""Gene and flanking nucleotide windows left on the device: what `Context.gene_windows` saves over the detour through the host
(DESIGN.md 4.16).

One context, meta mode under `benchdata.load_model_set()`, the 6 250 x 20 kbp batch of tools/device_input_bench.py.  `find_genes`
runs once, outside the clock (its gene records are on the host for both routes); only the step behind it is timed, for a consumer that
wants the nucleotides of every gene, or of the region around its start, as a torch tensor of token ids, one row per gene:
  route (a), what the library offered before: the rule of tests/gene_windows_ref.py with numpy over the host's copy of the letters --
             the positions of all rows expanded at once, one gather, the complement of the reverse rows, the ids, the padded rows or
             the ragged concatenation, no Python loop over genes -- and the upload of the tensor;
  route (b): `gene_windows` into a torch tensor it allocates.
Three cases: the gene itself as int64 padded and as uint8 ragged, and the 90-base start context (start - 60 .. start + 30) as int64
padded.  3 warm-up rounds, then 15 rounds that alternate between the routes; min / median / max per part.  Both routes must give the
same tensor in every round (asserted).

`--trace windows` makes three calls of every `k_gene_windows` instance (the gene itself) and of the `k_translate_tokens` and
`k_label_bases` instances of the same element width and layout, for a kernel trace of its own; `--trace plain` makes three plain
`find_genes` + `translate_genes` calls, for a kernel list that can be compared by name and count with the one before this feature.

    python tools/gene_windows_bench.py [--contigs 6250] [--rounds 15] [--trace windows|plain]"""
import argparse
import ctypes
import json
import os
import sys
import time

import torch                     # first: the library then binds to the HIP runtime of torch's wheel
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrodigal_amd import _cabi, benchdata

BODY, START = (("start", 0), ("end", 0)), (("start", -60), ("start", 30))
CASES = (("body", BODY, "int64", "padded"), ("body", BODY, "uint8", "ragged"), ("start", START, "int64", "padded"))
PAD = 7
CLASS_OF = np.full(256, 4, np.uint8)                           # A, C, G, T = 0 .. 3 in either case, anything else N = 4
for k, pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
    CLASS_OF[list(pair)] = k
COMPLEMENT = np.array([3, 2, 1, 0, 4, 5], np.uint8)            # and 5, outside, stays


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3)}


def gather(genes, letters, off, lens, circular, begin, end):
    """(uint8 classes of all rows, one after the other; the bases of every row): the rule of tests/gene_windows_ref.py for base tokens."""
    c = genes["contig"].astype(np.int64)
    b, e = genes["begin"].astype(np.int64), genes["end"].astype(np.int64)
    n, L = e - b + 1, lens[c]
    fwd = genes["strand"] == 1
    t_lo = np.where(begin[0] == "end", n, 0) + begin[1]
    t_hi = np.where(end[0] == "end", n, 0) + end[1]
    m = np.maximum(t_hi - t_lo, 0)
    ends = np.cumsum(m)
    x = np.arange(int(ends[-1]) if len(ends) else 0, dtype=np.int64) - np.repeat(ends - m, m)       # the base within its row
    step = np.where(fwd, 1, -1)
    q = np.repeat(np.where(fwd, b - 1 + t_lo, e - 1 - t_lo), m) + np.repeat(step, m) * x            # 0-based, before wrap and edges
    Lr = np.repeat(L, m)
    circ = np.repeat(circular[c], m)
    inside = circ | ((q >= 0) & (q < Lr))
    q = np.where(circ, q % Lr, np.clip(q, 0, Lr - 1))
    cls = CLASS_OF[letters[np.repeat(off[c], m) + q]]
    cls[~inside] = 5
    rev = np.repeat(~fwd, m)
    cls[rev] = COMPLEMENT[cls[rev]]
    return cls, m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=6250)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", choices=["windows", "plain"])
    args = ap.parse_args()
    n = args.contigs
    lengths, gcs, seeds = benchdata.config4_spec(n * 16)            # every 16th contig of the 100 000 x 20 kbp job: one rank's share
    seqs = [benchdata.synthetic_contig(int(a), float(b), int(c)) for a, b, c in zip(lengths[::16], gcs[::16], seeds[::16])]
    ctx = _cabi.Context(0)
    ctx.set_models([b for _, b in benchdata.load_model_set()])
    dev = torch.device("cuda", 0)
    batch = ctx.upload(seqs)
    res = ctx.find_genes(batch, meta=True)

    if args.trace == "plain":
        for _ in range(3):
            ctx.translate_genes(batch, ctx.find_genes(batch, meta=True))
        print(json.dumps({"trace": "plain", "contigs": n, "genes": int(len(res.genes))}))
        return

    if args.trace == "windows":
        from pyrodigal_amd import ProteinTokens
        elems = {}
        for _ in range(3):
            for dtype in ("uint8", "int32", "int64"):
                for layout in ("padded", "ragged"):
                    w = ctx.gene_windows(batch, res, _cabi.GeneWindows(bos=30, eos=31, pad=100, dtype=dtype, layout=layout))
                    p = ctx.translate_tokens(batch, res, ProteinTokens("-ACDEFGHIKLMNPQRSTVWYX*", bos=30, eos=31, dtype=dtype, layout=layout))
                    l = ctx.label_bases(batch, res, _cabi.BaseLabels("frame", pad=100, dtype=dtype, layout=layout))
                    elems[layout] = {"k_gene_windows": int(w.tokens.numel()), "k_translate_tokens": int(p.tokens.numel()),
                                     "k_label_bases": int(l.labels.numel())}
                    del w, p, l
        print(json.dumps({"trace": "windows", "contigs": n, "genes": int(len(res.genes)), "bases": int(batch.lengths.sum()), "elements": elems}))
        return

    lens = np.asarray(batch.lengths, np.int64)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    letters = np.frombuffer(b"".join(seqs), np.uint8)              # the host's copy of the input: the detour has it at hand
    circular = np.zeros(len(lens), bool)
    genes = np.ascontiguousarray(res.genes)
    specs = {c[0] + "/" + c[2] + "/" + c[3]: _cabi.GeneWindows(*c[1], outside=5, pad=PAD, dtype=c[2], layout=c[3]) for c in CASES}

    def route_host(window, dtype, layout):
        """(a): the letters gathered and complemented with numpy, the ids and the layout, upload."""
        t0 = time.perf_counter()
        cls, m = gather(genes, letters, off, lens, circular, *window)
        t1 = time.perf_counter()
        ids = cls.astype(getattr(np, dtype))                       # (the ids are the classes: A, C, G, T = 0 .. 3, N = 4, outside = 5)
        if layout == "padded":
            host = np.full((len(m), int(m.max())), PAD, ids.dtype)
            host[np.arange(host.shape[1])[None, :] < m[:, None]] = ids
        else:
            host = ids
        t2 = time.perf_counter()
        out = torch.from_numpy(host).to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return out, {"gather": t1 - t0, "ids_and_layout": t2 - t1, "upload": t3 - t2, "total": t3 - t0}

    def route_device(name):
        """(b): the tokens are written where they are wanted."""
        t0 = time.perf_counter()
        dw = ctx.gene_windows(batch, res, specs[name])
        t1 = time.perf_counter()
        return dw.tokens, {"gene_windows": t1 - t0, "total": t1 - t0}

    times = {(r, name): {} for r in ("a", "b") for name in specs}
    elems = {}
    for rnd in range(args.warmup + args.rounds):
        for what, window, dtype, layout in CASES:
            name = what + "/" + dtype + "/" + layout
            a, ta = route_host(window, dtype, layout)
            b, tb = route_device(name)
            assert a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b)), "the two routes differ: %s" % name
            elems[name] = int(b.numel())
            del a, b
            if rnd >= args.warmup:
                for route, t in (("a", ta), ("b", tb)):
                    for k, v in t.items():
                        times[(route, name)].setdefault(k, []).append(1e3 * v)
        print("round %d of %d" % (rnd + 1, args.warmup + args.rounds), file=sys.stderr, flush=True)
    # where the time of (b) goes: the marshalling in Python, and in the library the host checks with the row descriptors, the copy and
    # the kernel together -- the library's share is the call through ctypes alone, on a tensor made beforehand
    spec = specs["body/uint8/ragged"]
    total = int(spec.lengths(genes).sum())
    out = torch.empty(total, dtype=torch.uint8, device=dev)
    o, len_out = spec.opts(), np.zeros(len(genes), np.int64)
    lib_ms = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        rc = ctx.L.pga_gene_windows(ctx.h, batch.h, len(genes), genes.ctypes.data, ctypes.byref(o), out.data_ptr(), out.numel(), None, len_out.ctypes.data)
        lib_ms.append(1e3 * (time.perf_counter() - t0))
        assert rc == 0
    result = {"contigs": n, "genes": int(len(genes)), "bases": int(off[-1]), "rounds": args.rounds, "tensors_identical": True,
              "device": ctx.device_info()["name"], "elements": elems,
              "ms": {"%s/%s" % (r, name): {part: stats(v) for part, v in parts.items()} for (r, name), parts in times.items()},
              "library_call_body_uint8_ragged_ms": stats(lib_ms)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
