"""Gene calls on sequences that already lie in device memory: what `Context.upload_device` saves over the detour through the host
(DESIGN.md 4.13).

One context, meta mode under `benchdata.load_model_set()`, 6 250 x 20 kbp.  Two sources on the device, as a torch program would hold
them: a uint8 tensor of letters (back to back) and an int64 tensor of token ids `[B, Lmax]`.
  series (a), today's route: device-to-host copy of the source, numpy decode to `bytes`, `Context.upload`, `find_genes`;
  series (b): `Context.upload_device`, `find_genes`.
3 warm-up rounds, then 15 rounds that alternate between the series; min / median / max per part.  The gene records of (a) and (b)
must be byte-identical (asserted).  `upload_device` returns when the pack has run (it synchronises the upload stream), so its wall
time is the time of `pga_batch_create_device`; the time of `k_pack_device` alone, and of `k_circ_rotate` on the same batch, come from
a kernel trace of `--trace kernels` (a run of its own).  `--trace host` / `--trace device` make three calls of one route each, for
kernel lists that can be compared by name and count.

    python tools/device_input_bench.py [--contigs 6250] [--rounds 15] [--trace host|device|kernels]"""
import argparse
import json
import os
import sys
import time

import torch                     # first: the library then binds to the HIP runtime of torch's wheel
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrodigal_amd import DeviceSequences, _cabi, benchdata

ALPHABET = "ACGT"


def records(res):
    """The gene and contig records field by field (the structs have padding bytes nobody writes)."""
    return b"".join(np.ascontiguousarray(a[k]).tobytes() for a in (res.genes, res.contigs) for k in a.dtype.names)


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=6250)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace", choices=["host", "device", "kernels"])
    args = ap.parse_args()
    n = args.contigs
    lengths, gcs, seeds = benchdata.config4_spec(n * 16)            # every 16th contig of the 100 000 x 20 kbp job: one rank's share
    seqs = [benchdata.synthetic_contig(int(a), float(b), int(c)) for a, b, c in zip(lengths[::16], gcs[::16], seeds[::16])]
    lens = [len(s) for s in seqs]
    total, lmax = sum(lens), max(lens)
    ctx = _cabi.Context(0)
    ctx.set_models([b for _, b in benchdata.load_model_set()])
    dev = torch.device("cuda", 0)
    letters = torch.from_numpy(np.frombuffer(b"".join(seqs), np.uint8).copy()).to(dev)
    index = np.zeros(256, np.int64)
    index[np.frombuffer(ALPHABET.encode(), np.uint8)] = np.arange(len(ALPHABET))
    rows = np.full((n, lmax), len(ALPHABET), np.int64)                 # the padding: an id outside the alphabet
    for i, s in enumerate(seqs):
        rows[i, :len(s)] = index[np.frombuffer(s, np.uint8)]
    tokens = torch.from_numpy(rows).to(dev)
    table = np.frombuffer((ALPHABET + "N").encode(), np.uint8)
    torch.cuda.synchronize()
    sources = {"uint8": (letters, None), "int64": (tokens, ALPHABET)}

    def route_host(name):
        """(a): copy home, decode, upload, find."""
        t0 = time.perf_counter()
        if name == "uint8":
            host = letters.cpu().numpy()
            t1 = time.perf_counter()
            flat = host.tobytes()
            offs = np.concatenate([[0], np.cumsum(lens)])
            decoded = [flat[offs[i]:offs[i + 1]] for i in range(n)]
        else:
            host = tokens.cpu().numpy()
            t1 = time.perf_counter()
            text = table[host]                                         # [B, Lmax] of ASCII codes
            decoded = [text[i, :lens[i]].tobytes() for i in range(n)]
        t2 = time.perf_counter()
        batch = ctx.upload(decoded)
        t3 = time.perf_counter()
        res = ctx.find_genes(batch, meta=True)
        t4 = time.perf_counter()
        batch.close()
        return res, {"d2h": t1 - t0, "decode": t2 - t1, "upload": t3 - t2, "find": t4 - t3, "total": t4 - t0}

    def route_device(name, circular=False):
        """(b): pack on the device, find."""
        data, alphabet = sources[name]
        t0 = time.perf_counter()
        batch = ctx.upload_device(DeviceSequences(data, lens, alphabet=alphabet))
        t1 = time.perf_counter()
        if circular:
            batch.set_circular(True)
        res = ctx.find_genes(batch, meta=True)
        t2 = time.perf_counter()
        batch.close()
        return res, {"create_device": t1 - t0, "find": t2 - t1, "total": t2 - t0}

    if args.trace:
        for _ in range(3):
            if args.trace == "host":
                route_host("uint8")
            elif args.trace == "device":
                route_device("uint8")
            else:
                route_device("uint8", circular=True)                  # k_pack_device<1> and k_circ_rotate on the same batch
                ctx.upload_device(DeviceSequences(tokens, lens, alphabet=ALPHABET)).close()
                ctx.upload_device(DeviceSequences(letters, lens, alphabet={65: "A", 67: "C", 71: "G", 84: "T"})).close()
        print(json.dumps({"trace": args.trace, "contigs": n, "bases": total}))
        return

    times = {(r, s): {} for r in ("a", "b") for s in sources}
    want = None
    for rnd in range(args.warmup + args.rounds):
        for name in sources:
            for route, fn in (("a", route_host), ("b", route_device)):
                res, t = fn(name)
                got = records(res)
                if want is None:
                    want = got
                assert got == want, "the gene records of route (%s) on the %s source differ" % (route, name)
                if rnd >= args.warmup:
                    for k, v in t.items():
                        times[(route, name)].setdefault(k, []).append(1e3 * v)
    out = {"contigs": n, "bases": total, "rounds": args.rounds, "genes": int(len(res.genes)), "records_identical": True,
           "device": ctx.device_info()["name"], "ms": {"%s/%s" % k: {part: stats(v) for part, v in parts.items()} for k, parts in times.items()}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
