"""GeneFinder.select_translation_table against the host loop it replaces, on one device.

The genomes are mutated copies of the GCF_001457455.1 fixture (tests/golden): G genomes of 1 to 5 Mbp, each made of random slices
of the fixture (reverse-complemented at random) with 1 % point substitutions, one to four contigs each.  Nothing is downloaded.

  new:        select_translation_table(genomes)  -- one upload per device call, K trainings and K finds on the device, the coding
              bases counted where the gene records are
  host loop:  train_batch(genomes under 11 and under 4), find_genes_batch(contigs, training_infos=...), numpy densities

Prints the wall time of each, the share of training in the new call (train_batch of the same G x K trainings alone, over the new
call), and the bytes copied device to host per genome by each (models + what the find returns).

    python tools/table_select_bench.py --genomes 64
"""
import argparse
import gzip
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "GCF_001457455.1_NCTC11397_genomic.fna.gz")
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
GENE_RECORD = 88        # sizeof(pga_gene)
CONTIG_RECORD = 8 + 4 + 8


def fixture():
    with gzip.open(FIXTURE, "rt") as f:
        return "".join(l.strip() for l in f if not l.startswith(">")).upper().encode()


def make_genomes(n, seed=1):
    base = fixture()
    rng = np.random.default_rng(seed)
    out = []
    for g in range(n):
        length = int(rng.integers(1_000_000, 5_000_001))
        parts, have = [], 0
        while have < length:
            k = min(int(rng.integers(200_000, 800_000)), length - have)
            a = int(rng.integers(0, len(base) - k))
            s = base[a:a + k]
            parts.append(s.translate(_COMP)[::-1] if rng.random() < 0.5 else s)
            have += k
        seq = np.frombuffer(b"".join(parts), np.uint8).copy()
        hit = rng.random(seq.size) < 0.01
        seq[hit] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(hit.sum()))]
        seq = seq.tobytes()
        cuts = sorted(set([0, len(seq)] + [int(x) for x in rng.integers(100_000, len(seq) - 100_000, int(rng.integers(0, 4)))]))
        out.append([seq[a:b] for a, b in zip(cuts, cuts[1:])])
    return out


def host_loop(lib, genomes, tables):
    G, K = len(genomes), len(tables)
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tinfs = lib.GeneFinder().train_batch(genomes * K, translation_table=[t for t in tables for _ in range(G)])
    t_train = time.perf_counter() - t0
    contigs, models, owner = [], [], []
    for k in range(K):
        for g, gen in enumerate(genomes):
            contigs += gen
            models += [tinfs[k * G + g]] * len(gen)
            owner += [(k, g)] * len(gen)
    found = lib.GeneFinder(keep_nodes=False).find_genes_batch(contigs, training_infos=models)
    coding = np.zeros((K, G), np.int64)
    n_genes = 0
    for c, genes, (k, g) in zip(contigs, found, owner):
        cov = np.zeros(len(c), bool)
        for gene in genes:
            cov[max(gene.begin, 1) - 1:min(gene.end, len(c))] = True
        coding[k, g] += int(cov.sum())
        n_genes += len(genes)
    wall = time.perf_counter() - t0
    d2h = K * G * 558392 + n_genes * GENE_RECORD + len(contigs) * CONTIG_RECORD
    return wall, t_train, coding, d2h / G


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--genomes", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--json", help="also write the result here")
    args = ap.parse_args()
    from pyrodigal_amd import lib
    tables = (11, 4)
    genomes = make_genomes(args.genomes)
    bases = sum(len(c) for g in genomes for c in g)
    n_contigs = sum(len(g) for g in genomes)
    # warm-up: contexts, kernels, caches
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lib.GeneFinder().select_translation_table(genomes[:2])
        host_loop(lib, genomes[:2], tables)
    res = {"genomes": args.genomes, "contigs": n_contigs, "mbp": bases / 1e6, "new_s": [], "host_s": [], "train_only_s": []}
    for _ in range(args.repeat):
        f = lib.GeneFinder()
        t0 = time.perf_counter()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sel = f.select_translation_table(genomes)
        res["new_s"].append(time.perf_counter() - t0)
        wall, t_train, coding, host_d2h = host_loop(lib, genomes, tables)
        res["host_s"].append(wall)
        res["train_only_s"].append(t_train)
        same = all(sel[g].coding_bases[t] == int(coding[k, g]) for k, t in enumerate(tables) for g in range(len(genomes)))
        res["identical"] = bool(same)
    new_s, host_s, train_s = min(res["new_s"]), min(res["host_s"]), min(res["train_only_s"])
    K = len(tables)
    new_d2h = K * 558392 + K * n_contigs / len(genomes) * CONTIG_RECORD
    res.update({"new_wall_s": new_s, "host_wall_s": host_s, "speedup": host_s / new_s, "training_share_of_new": train_s / new_s,
                "d2h_bytes_per_genome_new": new_d2h, "d2h_bytes_per_genome_host": host_d2h,
                "picked": {str(t): sum(1 for s in sel if s.translation_table == t) for t in tables}})
    print(json.dumps(res))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
