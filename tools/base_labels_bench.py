"""Per-base gene labels left on the device: what `Context.label_bases` saves over the detour through the host.

One context, meta mode under `benchdata.load_model_set()`, the 6 250 x 20 kbp batch of tools/device_input_bench.py.  `find_genes`
runs once, outside the clock (its gene records are on the host for both routes); only the step behind it is timed, for a consumer that
wants the class of every base as a torch tensor in the shape of its input:
  route (a), what the library offered before: the rule of tests/base_labels_ref.py painted with numpy -- every stretch of every gene
             expanded to flat positions at once, four passes so that no two genes of a pass overlap, no Python loop over genes -- the
             class map, the padded rows or the ragged concatenation, and the upload of the tensor;
  route (b): `label_bases` into a torch tensor it allocates.
Three cases: int64 padded, int64 ragged, uint8 ragged, under the `frame` preset.  3 warm-up rounds, then 15 rounds that alternate
between the routes; min / median / max per part.  Both routes must give the same tensor in every round (asserted).

`--trace labels` makes three calls of every `k_label_bases` instance and of the `k_translate_tokens` instance of the same element width
and layout, for a kernel trace of its own; `--trace plain` makes three plain `find_genes` + `translate_genes` calls, for a kernel list
that can be compared by name and count with the one before this feature.

    python tools/base_labels_bench.py [--contigs 6250] [--rounds 15] [--trace labels|plain]"""
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

CASES = (("int64", "padded"), ("int64", "ragged"), ("uint8", "ragged"))
PAD = -100
POSITION_BITS = np.array([0x01, 0x02, 0x04, 0x20, 0x10, 0x08], np.uint8)      # by (q - b) % 3, forward then reverse ((e - q) % 3 = 2 - it)


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3)}


def paint(genes, lengths, off):
    """uint8[off[-1]]: the raw byte of every base of the batch under the gene records (the rule of tests/base_labels_ref.py)."""
    raw = np.zeros(int(off[-1]), np.uint8)
    c = genes["contig"].astype(np.int64)
    b, e, n_of = genes["begin"].astype(np.int64), genes["end"].astype(np.int64), lengths[c]
    fwd = genes["strand"] == 1
    # the codon positions: every stretch of every gene expanded to flat positions (a gene across the origin makes a second stretch,
    # from position 0), in four passes by rank, so that the stretches of one pass do not overlap and a plain fancy |= serves
    wrap = np.flatnonzero(e > n_of)
    rec = np.concatenate([np.arange(len(genes)), wrap])
    lo = np.concatenate([b - 1, np.zeros(len(wrap), np.int64)])
    hi = np.concatenate([np.minimum(e, n_of), (e - n_of)[wrap]])
    d0 = np.concatenate([np.zeros(len(genes), np.int64), (n_of - b + 1)[wrap]]) % 3       # (q - b) % 3 of the stretch's first position
    start = off[c[rec]] + lo
    rank = np.empty(len(rec), np.int64)
    rank[np.argsort(start, kind="stable")] = np.arange(len(rec))
    first_bit = (np.where(fwd[rec], 0, 3) + d0).astype(np.int32)     # an index into POSITION_BITS[0:3] or [3:6], before + within % 3
    for k in range(4):
        s = np.flatnonzero(rank % 4 == k)
        n = (hi - lo)[s]
        ends = np.cumsum(n)
        within = np.arange(int(ends[-1]) if len(ends) else 0, dtype=np.int32) - np.repeat((ends - n).astype(np.int32), n)
        pos = np.repeat(start[s], n)
        pos += within
        within %= 3
        within += np.repeat(first_bit[s] % 3, n)
        within %= 3
        within += np.repeat(first_bit[s] // 3 * 3, n)
        raw[pos] |= POSITION_BITS[within]
    # the start and stop codons: three bases at either end of every gene (a few positions: an unbuffered |= takes the overlaps)
    for at, flag, bit in ((b, genes["partial_begin"], np.where(fwd, 0x40, 0x80)), (e - 2, genes["partial_end"], np.where(fwd, 0x80, 0x40))):
        keep = flag == 0
        q = (at[keep][:, None] + np.arange(3)[None, :]).ravel()
        where = np.repeat(off[c[keep]], 3) + (q - 1) % np.repeat(n_of[keep], 3)
        np.bitwise_or.at(raw, where, np.repeat(bit[keep], 3).astype(np.uint8))
    return raw


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=6250)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", choices=["labels", "plain"])
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

    if args.trace == "labels":
        from pyrodigal_amd import ProteinTokens
        for _ in range(3):
            for dtype in ("uint8", "int32", "int64"):
                for layout in ("padded", "ragged"):
                    ctx.label_bases(batch, res, _cabi.BaseLabels("frame", pad=100, dtype=dtype, layout=layout))
                    ctx.translate_tokens(batch, res, ProteinTokens("-ACDEFGHIKLMNPQRSTVWYX*", bos=30, eos=31, dtype=dtype, layout=layout))
        print(json.dumps({"trace": "labels", "contigs": n, "genes": int(len(res.genes)), "bases": int(batch.lengths.sum())}))
        return

    lens = np.asarray(batch.lengths, np.int64)
    off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    frame = np.array(_cabi.label_class_map("frame"), np.int64)
    genes = np.ascontiguousarray(res.genes)

    def route_host(dtype, layout):
        """(a): the records painted with numpy, the class map and the layout, upload."""
        t0 = time.perf_counter()
        raw = paint(genes, lens, off)
        t1 = time.perf_counter()
        ids = frame.astype(getattr(np, dtype))[raw]
        if layout == "padded":
            host = np.full((len(lens), int(lens.max())), PAD, ids.dtype)
            host[np.arange(host.shape[1])[None, :] < lens[:, None]] = ids
        else:
            host = ids
        t2 = time.perf_counter()
        out = torch.from_numpy(host).to(dev)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        return out, {"paint": t1 - t0, "map_and_layout": t2 - t1, "upload": t3 - t2, "total": t3 - t0}

    specs = {c: _cabi.BaseLabels("frame", pad=PAD if c[0] != "uint8" else None, dtype=c[0], layout=c[1]) for c in CASES}

    def route_device(dtype, layout):
        """(b): the labels are written where they are wanted."""
        t0 = time.perf_counter()
        dl = ctx.label_bases(batch, res, specs[(dtype, layout)])
        t1 = time.perf_counter()
        return dl.labels, {"label_bases": t1 - t0, "total": t1 - t0}

    times = {(r, c): {} for r in ("a", "b") for c in CASES}
    elems = {}
    for rnd in range(args.warmup + args.rounds):
        for case in CASES:
            a, ta = route_host(*case)
            b, tb = route_device(*case)
            assert a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b)), "the two routes differ: %s %s" % case
            elems[case] = int(b.numel())
            del a, b
            if rnd >= args.warmup:
                for route, t in (("a", ta), ("b", tb)):
                    for k, v in t.items():
                        times[(route, case)].setdefault(k, []).append(1e3 * v)
        print("round %d of %d" % (rnd + 1, args.warmup + args.rounds), file=sys.stderr, flush=True)
    # where the time of (b) goes: the marshalling in Python, and in the library the host checks with the interval build, the copy and
    # the kernel together -- the library's share is the call through ctypes alone, on a tensor made beforehand
    spec = specs[("uint8", "ragged")]
    out = torch.empty(int(off[-1]), dtype=torch.uint8, device=dev)
    o, len_out = spec.opts(), np.zeros(len(lens), np.int64)
    lib_ms = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        rc = ctx.L.pga_label_bases(ctx.h, batch.h, len(genes), genes.ctypes.data, ctypes.byref(o), out.data_ptr(), out.numel(), None, len_out.ctypes.data)
        lib_ms.append(1e3 * (time.perf_counter() - t0))
        assert rc == 0
    result = {"contigs": n, "genes": int(len(genes)), "bases": int(off[-1]), "rounds": args.rounds, "tensors_identical": True,
              "device": ctx.device_info()["name"], "elements": {"%s/%s" % c: v for c, v in elems.items()},
              "ms": {"%s/%s/%s" % ((r,) + c): {part: stats(v) for part, v in parts.items()} for (r, c), parts in times.items()},
              "library_call_uint8_ragged_ms": stats(lib_ms)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
