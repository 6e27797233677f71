"""K-mer and codon counts of contigs and genes on the device: what `Context.kmer_counts` saves over the routes a caller had before
(DESIGN.md 4.18).

One context, meta mode under `benchdata.load_model_set()`, the 6 250 x 20 kbp batch of tools/device_input_bench.py.  `find_genes`
runs once, outside the clock (its gene records are on the host for every route); only the step behind it is timed:
  route (a), codon usage per gene through the windows: `gene_windows(unit="codon")` as int64 ragged tokens, then
             `torch.zeros(...).index_put_(..., accumulate=True)` on the device -- 8 bytes written per codon to be read once;
  route (b), canonical 4-mers per contig through torch on the device: the letters as a `[B, L]` tensor, a look-up into classes,
             `unfold(1, 4, 1)`, the codes, the folded bins, one `bincount`;
  route (c): `kmer_counts` -- codon rows per gene, codon rows per contig over its genes, canonical 4-mer rows per contig, in-frame
             dicodon rows per gene and per contig over its genes.
3 warm-up rounds, then 15 rounds that alternate between the routes; min / median / max.  The routes must agree in every round
(asserted): (a) with the codon rows, (b) with the 4-mer rows, the rows per contig with the sums of the gene rows, the dicodon rows
with the pairs of neighbouring codon tokens of (a).  `--forms` times every form of the kernel (PGA_KMER_COUNTS_FORM) on every case.

`--trace counts` makes three calls of every case in every form, and of `k_gene_windows<1, false>` and `k_label_bases<1, false>`
(uint8, ragged: both read every letter of the genes or contigs) for a kernel trace of its own; `--trace plain` makes three plain
`find_genes` + `translate_genes` calls, for a kernel list that can be compared by name and count with the one before this feature.

    python tools/kmer_counts_bench.py [--contigs 6250] [--rounds 15] [--forms] [--trace counts|plain]"""
import argparse
import json
import os
import sys
import time

import torch                     # first: the library then binds to the HIP runtime of torch's wheel
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrodigal_amd import KmerCounts, _cabi, benchdata

CASES = {
    "codons/gene": KmerCounts(3, rows="gene", step=3),
    "codons/contig_genes": KmerCounts(3, rows="contig_genes", step=3),
    "4-mers canonical/contig": KmerCounts(4, canonical=True),
    "dicodons/gene": KmerCounts(6, rows="gene", step=3),
    "dicodons/contig_genes": KmerCounts(6, rows="contig_genes", step=3),
}


FORMS = ("lds-group", "lds-wave", "direct-group", "direct-wave")      # PGA_KMER_COUNTS_FORM: histogram or none, a piece per workgroup or per wave


def stats(xs):
    xs = sorted(xs)
    return {"min": round(xs[0], 3), "median": round(xs[len(xs) // 2], 3), "max": round(xs[-1], 3)}


def forced(form):
    if form is None:
        os.environ.pop("PGA_KMER_COUNTS_FORM", None)
    else:
        os.environ["PGA_KMER_COUNTS_FORM"] = form


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=6250)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forms", action="store_true")
    ap.add_argument("--trace", choices=["counts", "plain"])
    args = ap.parse_args()
    n = args.contigs
    lengths, gcs, seeds = benchdata.config4_spec(n * 16)            # every 16th contig of the 100 000 x 20 kbp job: one rank's share
    seqs = [benchdata.synthetic_contig(int(a), float(b), int(c)) for a, b, c in zip(lengths[::16], gcs[::16], seeds[::16])]
    ctx = _cabi.Context(0)
    ctx.set_models([b for _, b in benchdata.load_model_set()])
    dev = torch.device("cuda", 0)
    batch = ctx.upload(seqs)
    res = ctx.find_genes(batch, meta=True)
    genes = np.ascontiguousarray(res.genes)
    G, B = len(genes), len(seqs)
    gene_bases = int((genes["end"].astype(np.int64) - genes["begin"] + 1).sum())
    contig_bases = int(batch.lengths.sum())

    if args.trace == "plain":
        for _ in range(3):
            ctx.translate_genes(batch, ctx.find_genes(batch, meta=True))
        print(json.dumps({"trace": "plain", "contigs": n, "genes": G}))
        return

    if args.trace == "counts":
        for _ in range(3):
            for form in FORMS:
                forced(form)
                for spec in CASES.values():
                    ctx.kmer_counts(batch, res, spec)
            forced(None)
            ctx.gene_windows(batch, res, _cabi.GeneWindows(dtype="uint8", layout="ragged"))
            ctx.label_bases(batch, res, _cabi.BaseLabels("frame", dtype="uint8", layout="ragged"))
        print(json.dumps({"trace": "counts", "contigs": n, "genes": G, "gene_bases": gene_bases, "contig_bases": contig_bases,
                          "order_per_round": [f + ": " + c for f in FORMS for c in CASES] + ["k_gene_windows<1,false>", "k_label_bases<1,false>"]}))
        return

    codon_tokens = _cabi.GeneWindows(unit="codon", dtype="int64", layout="ragged")
    gene_of_contig = torch.from_numpy(genes["contig"].astype(np.int64)).to(dev)
    Lmax = int(batch.lengths.max())
    rows = np.full((B, Lmax), ord("N"), np.uint8)
    for i, s in enumerate(seqs):
        rows[i, :len(s)] = np.frombuffer(s, np.uint8)
    letters = torch.from_numpy(rows).to(dev)                        # the input where a DeviceSequences caller has it
    lens_dev = torch.from_numpy(np.asarray(batch.lengths, np.int64)).to(dev)
    lut = torch.full((256,), 4, dtype=torch.int64, device=dev)
    for v, pair in enumerate((b"Aa", b"Cc", b"Gg", b"Tt")):
        lut[list(pair)] = v
    fold = torch.tensor(CASES["4-mers canonical/contig"].table, dtype=torch.int64, device=dev)
    weights = torch.tensor([64, 16, 4, 1], dtype=torch.int64, device=dev)

    def route_a():
        """codon usage per gene: int64 ragged codon tokens, then a scatter-add on the device."""
        t0 = time.perf_counter()
        dw = ctx.gene_windows(batch, res, codon_tokens)
        t1 = time.perf_counter()
        row = torch.repeat_interleave(torch.arange(G, device=dev), torch.from_numpy(dw.lengths).to(dev))
        counts = torch.zeros((G, 65), dtype=torch.int32, device=dev)
        counts.index_put_((row, dw.tokens), torch.ones((), dtype=torch.int32, device=dev).expand(row.shape), accumulate=True)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (counts[:, :64], dw, row), {"gene_windows": t1 - t0, "index_put": t2 - t1, "total": t2 - t0}

    def route_b():
        """canonical 4-mers per contig: classes, unfold, codes, folded bins, bincount."""
        t0 = time.perf_counter()
        cls = lut[letters.long()]
        w = cls.unfold(1, 4, 1)                                     # [B, Lmax - 3, 4]
        ok = (w < 4).all(dim=2) & (torch.arange(Lmax - 3, device=dev)[None, :] + 4 <= lens_dev[:, None])
        code = (w * weights).sum(dim=2)
        flat = (torch.arange(B, device=dev)[:, None] * 136 + fold[code.clamp(max=255)])[ok]
        counts = torch.bincount(flat, minlength=B * 136).reshape(B, 136).to(torch.int32)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return counts, {"total": t1 - t0}

    def route_c(name):
        t0 = time.perf_counter()
        dc = ctx.kmer_counts(batch, res, CASES[name])
        t1 = time.perf_counter()
        return dc, {"total": t1 - t0}

    times = {}

    def note(key, t):
        for part, v in t.items():
            times.setdefault(key, {}).setdefault(part, []).append(1e3 * v)

    for rnd in range(args.warmup + args.rounds):
        keep = rnd >= args.warmup
        (a, dw, row), ta = route_a()
        got = {}
        for name in CASES:
            got[name], tc = route_c(name)
            if keep:
                note("c/" + name, tc)
            if args.forms:
                for form in FORMS:
                    forced(form)
                    other, tf = route_c(name)
                    forced(None)
                    assert bool(torch.equal(other.counts, got[name].counts)), "the forms differ: %s" % name
                    del other
                    if keep:
                        note("c/%s [%s]" % (name, form), tf)
        b, tb = route_b()
        if keep:
            note("a/codons/gene", ta)
            note("b/4-mers canonical/contig", tb)
        assert bool(torch.equal(a, got["codons/gene"].counts)), "route (a) and the codon rows differ"
        assert bool(torch.equal(b, got["4-mers canonical/contig"].counts)), "route (b) and the 4-mer rows differ"
        for kind in ("codons", "dicodons"):
            per = got[kind + "/gene"].counts
            sums = torch.zeros_like(got[kind + "/contig_genes"].counts).index_add_(0, gene_of_contig, per)
            assert bool(torch.equal(sums, got[kind + "/contig_genes"].counts)), "the %s rows per contig are not the sums of the gene rows" % kind
            del sums
        # the dicodon rows against the pairs of neighbouring codon tokens of route (a)
        tok = dw.tokens
        pair = (row[:-1] == row[1:]) & (tok[:-1] < 64) & (tok[1:] < 64)
        di = torch.zeros((G, 4096), dtype=torch.int32, device=dev)
        di.index_put_((row[:-1][pair], (tok[:-1] * 64 + tok[1:])[pair]), torch.ones((), dtype=torch.int32, device=dev).expand(int(pair.sum())), accumulate=True)
        assert bool(torch.equal(di, got["dicodons/gene"].counts)), "the dicodon rows differ from the codon pairs"
        windows = {name: int(dc.windows.sum()) for name, dc in got.items()}
        del a, b, dw, row, got, di, tok, pair
        print("round %d of %d" % (rnd + 1, args.warmup + args.rounds), file=sys.stderr, flush=True)
    result = {"contigs": n, "genes": G, "gene_bases": gene_bases, "contig_bases": contig_bases, "rounds": args.rounds, "routes_agree": True,
              "device": ctx.device_info()["name"], "windows": windows,
              "ms": {key: {part: stats(v) for part, v in parts.items()} for key, parts in times.items()}}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
