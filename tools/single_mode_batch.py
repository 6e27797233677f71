"""Single mode over many genomes: the reference's per-genome loop against the per-genome models in one call.
  (a) per genome: GeneFinder(closed=True).train(g), then find_genes(g)             (benches/run_single/bench.py:37-42)
  (b) GeneFinder(closed=True).train_batch(genomes), then find_genes_batch(genomes, training_infos=...)
Medians of `--runs` runs after a warm-up, host to host; (a) and (b) must give identical models and gene records.
usage: python tools/single_mode_batch.py [--genomes 64] [--length 2000000] [--runs 3]"""
import argparse, gzip, json, os, statistics, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pyrodigal_amd import benchdata, lib                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genomes", type=int, default=64)
    ap.add_argument("--length", type=int, default=2_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--only-b", action="store_true", help="one run of (b), no comparison (for a kernel trace)")
    a = ap.parse_args()
    genomes = [benchdata.planted_contig(a.length, 0.30 + 0.40 * k / max(1, a.genomes - 1), 5000 + k) for k in range(a.genomes)]
    gz = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "GCF_001457455.1_NCTC11397_genomic.fna.gz")
    genomes.append(b"".join(l.strip().encode() for l in gzip.open(gz, "rt") if not l.startswith(">")))
    mbp = sum(len(g) for g in genomes) / 1e6

    def loop():
        out = []
        for g in genomes:
            f = lib.GeneFinder(closed=True)
            t = f.train(g)
            out.append((t, f.find_genes(g)))
        return out

    def batched():
        ts = lib.GeneFinder(closed=True).train_batch(genomes)
        return list(zip(ts, lib.GeneFinder(closed=True).find_genes_batch(genomes, training_infos=ts)))

    def key(res):
        return [(t.raw.tobytes(), [(x.begin, x.end, x.strand, x.start_type, x.score) for x in g]) for t, g in res]

    if a.only_b:
        batched()
        return
    loop(); batched()                                           # warm-up: contexts, caches
    times = {"a_loop": [], "b_batched": []}
    for _ in range(a.runs):
        for name, fn in (("a_loop", loop), ("b_batched", batched)):
            t0 = time.perf_counter(); r = fn(); times[name].append(time.perf_counter() - t0)
            if name == "a_loop":
                ref = key(r)
            else:
                assert key(r) == ref, "(a) and (b) differ"
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"genomes": len(genomes), "mbp": round(mbp, 2), "runs": a.runs, "identical": True,
                      "a_loop_s": round(med["a_loop"], 3), "b_batched_s": round(med["b_batched"], 3),
                      "a_mbp_per_s": round(mbp / med["a_loop"], 2), "b_mbp_per_s": round(mbp / med["b_batched"], 2),
                      "speedup": round(med["a_loop"] / med["b_batched"], 3)}))


if __name__ == "__main__":
    main()
