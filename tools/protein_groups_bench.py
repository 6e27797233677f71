"""Identical predicted proteins grouped on the device: what `Context.protein_groups` saves over the routes a caller had before
(DESIGN.md 4.19).

One context, meta mode under `benchdata.load_model_set()`.  The synthetic batches carry no copies, so the batch is the 6 250 x 20 kbp
batch of tools/device_input_bench.py with every contig present a second time, reverse-complemented: 12 500 contigs, and every protein
at least twice.  `find_genes` runs once, outside the clock (its gene records are on the host for every route); only the step behind it
is timed, on the host clock:
  route (a): `translate_tokens` into a padded uint8 `[G, W]` tensor (the letters as ids, pad 0), then
             `torch.unique(dim=0, return_inverse=True)` -- a lexicographic sort of G rows of W tokens;
  route (b): `translate_genes` -- every letter to the host -- and a `dict` over the proteins;
  route (c): `protein_groups` -- and once more with the contigs' tables and the four tensors given, which leaves the library's own
             host work and the device.
Warm-up rounds, then rounds that alternate between the routes; min / median / max.  The three routes must agree on the partition in
every round (asserted): each is reduced to the first member of every gene's group.

`--trace groups` makes three calls of `protein_groups` in both units, and of `k_translate_tokens<1, false>` and
`k_gene_windows<1, false>` (uint8, ragged: they read the same letters) for a kernel trace of its own.

    python tools/protein_groups_bench.py [--contigs 6250] [--rounds 9] [--warmup 2] [--skip-unique] [--trace groups]"""
import argparse
import json
import os
import sys
import time

import torch                     # first: the library then binds to the HIP runtime of torch's wheel
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrodigal_amd import ProteinGroups, ProteinTokens, _cabi, benchdata

COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=6250)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-unique", action="store_true", help="leave route (a) out (its sort needs G x W bytes several times over)")
    ap.add_argument("--trace", choices=["groups"])
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
    spec = ProteinGroups()
    letters = ProteinTokens({chr(k): k for k in range(1, 128)}, dtype="uint8", layout="padded")

    if args.trace == "groups":
        for _ in range(3):
            ctx.protein_groups(batch, res, spec)
            ctx.protein_groups(batch, res, ProteinGroups("gene"))
            ctx.translate_tokens(batch, res, ProteinTokens({chr(k): k for k in range(1, 128)}, dtype="uint8", layout="ragged"))
            ctx.gene_windows(batch, res, _cabi.GeneWindows(dtype="uint8", layout="ragged"))
        print(json.dumps({"trace": "groups", "contigs": len(seqs), "genes": G, "residues": residues, "gene_bases": gene_bases,
                          "rounds_and_differing_pairs": ctx.protein_groups_stats()}))
        return

    def first_of(labels):
        """the first member of every gene's group, from any labelling of the groups (a device tensor)"""
        first = torch.full((int(labels.max()) + 1,), G, dtype=torch.int64, device=dev)
        first.scatter_reduce_(0, labels, torch.arange(G, device=dev), reduce="amin")
        return first[labels]

    def route_a():
        t0 = time.perf_counter()
        dp = ctx.translate_tokens(batch, res, letters)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        uniq, inverse = torch.unique(dp.tokens, dim=0, return_inverse=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        shape = tuple(dp.tokens.shape)
        return (inverse, int(uniq.shape[0]), shape), {"translate_tokens": t1 - t0, "unique": t2 - t1, "total": t2 - t0}

    def route_b():
        t0 = time.perf_counter()
        prot, off = ctx.translate_genes(batch, res, include_stop=False)
        t1 = time.perf_counter()
        data = prot.tobytes()
        number, group = {}, np.empty(G, np.int64)
        for g in range(G):
            group[g] = number.setdefault(data[off[g]:off[g + 1]], len(number))
        t2 = time.perf_counter()
        return (group, len(number)), {"translate_genes": t1 - t0, "dict": t2 - t1, "total": t2 - t0}

    tables = np.array(_cabi._default_tables(ctx, res.contigs), np.int32)
    outs = (torch.empty(G, dtype=torch.int64, device=dev), torch.empty(G, dtype=torch.int64, device=dev),
            torch.empty(G, dtype=torch.int64, device=dev), torch.empty((G, 2), dtype=torch.int64, device=dev))

    def route_c(given=False):
        """`given`: with the tables of the contigs and the four tensors in hand, as a caller in a loop has them"""
        t0 = time.perf_counter()
        dg = ctx.protein_groups(batch, genes, spec, tables=tables, out=outs) if given else ctx.protein_groups(batch, res, spec)
        t1 = time.perf_counter()
        return dg, {"total": t1 - t0}

    times = {}

    def note(key, t):
        for part, v in t.items():
            times.setdefault(key, {}).setdefault(part, []).append(1e3 * v)

    shape = None
    for rnd in range(args.warmup + args.rounds):
        keep = rnd >= args.warmup
        dg, tc = route_c()
        mine = dg.representatives[dg.group]
        (group_b, n_b), tb = route_b()
        assert n_b == dg.n_groups, "route (b) finds %d groups, route (c) %d" % (n_b, dg.n_groups)
        assert bool(torch.equal(first_of(torch.from_numpy(group_b).to(dev)), mine)), "routes (b) and (c) differ on the partition"
        assert bool(torch.equal(dg.group, torch.from_numpy(group_b).to(dev))), "routes (b) and (c) number the groups differently"
        if not args.skip_unique:
            (inverse, n_a, shape), ta = route_a()
            assert n_a == dg.n_groups, "route (a) finds %d groups, route (c) %d" % (n_a, dg.n_groups)
            assert bool(torch.equal(first_of(inverse), mine)), "routes (a) and (c) differ on the partition"
            del inverse
            if keep:
                note("a/unique", ta)
        again, tg = route_c(given=True)
        assert bool(torch.equal(again.group, dg.group)) and again.n_groups == dg.n_groups
        if keep:
            note("b/dict", tb)
            note("c/protein_groups", tc)
            note("c/protein_groups, tables and tensors given", tg)
        n_groups, run = dg.n_groups, ctx.protein_groups_stats()
        del dg, mine
        print("round %d of %d" % (rnd + 1, args.warmup + args.rounds), file=sys.stderr, flush=True)
    result = {"contigs": len(seqs), "genes": G, "groups": n_groups, "residues": residues, "padded_shape": shape, "rounds": args.rounds,
              "routes_agree": True, "verification": run, "device": ctx.device_info()["name"],
              "ms": {key: {part: stats(v) for part, v in parts.items()} for key, parts in times.items()}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
