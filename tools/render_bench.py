"""Text output on one MI355X: the device renderer (Context.render_genes) against the host writers (Genes.write_*), and the
command line from a FASTA file to GFF + protein FASTA, and to GenBank + the start-score file.

  (a) render kernels (length pass + scan + write pass; scores: and the row sort) of GFF, protein FASTA, gene FASTA, GenBank and
      the start scores of one 6 250 x 20 kbp meta call, next to that call's find_genes device time, with the node arrays kept on
      the device (want_nodes="device") and without (want_nodes=0: the lean gather)
  (b) the host writers' loop (write_gff / write_translations / write_genes / write_genbank / write_scores) over the same results
  (c) python -m pyrodigal_amd -p meta from a FASTA file to GFF + .faa and to -f gbk + -s, wall time and Gbp/s, next to the
      Python loop over GeneFinder.find_genes_batch + the writers on the same file

Prints one JSON line.  Synthetic inputs go to a temporary directory."""
import argparse
import io
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contigs", type=int, default=6250)
    ap.add_argument("--length", type=int, default=20_000)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from pyrodigal_amd import _cabi, benchdata, lib
    models = benchdata.load_model_set()
    n, L = args.contigs, args.length
    lens, gcs, seeds = benchdata.config4_spec(n, L)
    seqs = benchdata.generate(lens, gcs, seeds, procs=16)
    ids = ["contig_%d" % i for i in range(n)]
    out = {"contigs": n, "length": L}

    # (a) device: find_genes + render_genes on the resident batch
    ctx = _cabi.Context(0)
    ctx.set_models([b for _, b in models])
    descs = [name.replace(".gz", "") for name, _ in models]      # what the command line reports: the bin files' names
    b = ctx.upload(seqs)
    r = ctx.find_genes(b, meta=True)                   # warm-up
    fmts = _cabi.RENDER_FORMATS
    fg, fg_lean, rk, rw = [], [], {k: [] for k in fmts}, []
    for _ in range(args.repeats):
        fg_lean.append(ctx.find_genes(b, meta=True).t_total_ms)
        r = ctx.find_genes(b, meta=True, want_nodes="device")
        fg.append(r.t_total_ms)
        t0 = time.perf_counter()
        txt = ctx.render_genes(b, r, ids, fmts, meta=True, descriptions=descs, unbinned_model=min(5, len(models) - 1))
        rw.append((time.perf_counter() - t0) * 1e3)
        for k, v in txt.items():
            rk[k].append(v.kernel_ms)
    b.close()
    med = lambda xs: sorted(xs)[len(xs) // 2]
    out["genes"] = int(len(r.genes))
    out["find_genes_device_ms"] = med(fg)
    out["find_genes_device_ms_lean"] = med(fg_lean)        # want_nodes=0, what bench.py runs
    out["render_kernel_ms"] = {k: med(v) for k, v in rk.items()}
    out["render_kernel_ms_total"] = sum(out["render_kernel_ms"].values())
    out["render_over_find"] = out["render_kernel_ms_total"] / out["find_genes_device_ms"]
    out["render_call_wall_ms"] = med(rw)
    out["text_bytes"] = {k: len(v.data) for k, v in txt.items()}
    out["fallback_lines"] = sum(v.fallback for v in txt.values())
    ctx.close()

    # (b) the host writers over the same calls
    bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=bl), d) for d, (_, bl) in zip(descs, models)])
    finder = lib.GeneFinder(meta=True, metagenomic_bins=bins)
    t0 = time.perf_counter()
    genes = finder.find_genes_batch(seqs)
    t_find = time.perf_counter() - t0
    host = {}
    for fmt, meth in (("gff", "write_gff"), ("faa", "write_translations"), ("fna", "write_genes"), ("gbk", "write_genbank"),
                      ("scores", "write_scores")):
        s = io.StringIO()
        t0 = time.perf_counter()
        for g, sid in zip(genes, ids):
            getattr(g, meth)(s, sid)              # (the finder keeps the nodes: write_scores needs them)
        host[fmt] = (time.perf_counter() - t0) * 1e3
        assert s.getvalue().encode() == txt[fmt].data, fmt          # the device text is the writers' text
    out["host_writer_ms"] = host
    out["host_writer_over_render_kernels"] = sum(host.values()) / out["render_kernel_ms_total"]
    out["host_find_genes_batch_ms"] = t_find * 1e3
    print(json.dumps(out), file=sys.stderr, flush=True)        # (a) and (b), should (c) not finish

    # (c) the command line, file to GFF + .faa
    with tempfile.TemporaryDirectory() as tmp:
        fa = os.path.join(tmp, "in.fna")
        with open(fa, "wb") as f:
            for sid, s in zip(ids, seqs):
                f.write(b">" + sid.encode() + b"\n")
                for k in range(0, len(s), 80):
                    f.write(s[k:k + 80] + b"\n")
        paths = []
        for name, bl in models:
            p = os.path.join(tmp, name.replace(".gz", ""))
            with open(p, "wb") as f:
                f.write(bl)
            paths.append(p)
        cmd = [sys.executable, "-m", "pyrodigal_amd", "-p", "meta", "-i", fa, "-o", os.path.join(tmp, "o.gff"), "-a",
               os.path.join(tmp, "o.faa"), "--meta-bins", *paths]
        cmd_gbk = [sys.executable, "-m", "pyrodigal_amd", "-p", "meta", "-i", fa, "-o", os.path.join(tmp, "o.gbk"), "-f", "gbk",
                   "-s", os.path.join(tmp, "o.scores"), "--meta-bins", *paths]
        walls, walls_gbk = [], []
        for _ in range(3):
            t0 = time.perf_counter()
            subprocess.run(cmd, cwd=ROOT, check=True, timeout=600)
            walls.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            subprocess.run(cmd_gbk, cwd=ROOT, check=True, timeout=600)
            walls_gbk.append(time.perf_counter() - t0)
        with open(os.path.join(tmp, "o.gff"), "rb") as f:
            assert f.read() == txt["gff"].data
        with open(os.path.join(tmp, "o.scores"), "rb") as f:
            assert f.read() == txt["scores"].data
        bases = n * L
        out["cli_wall_s"] = med(walls)
        out["cli_gbps"] = bases / med(walls) / 1e9
        out["cli_gbk_scores_wall_s"] = med(walls_gbk)
        out["cli_gbk_scores_gbps"] = bases / med(walls_gbk) / 1e9
        # the Python loop the command line replaces: read, find_genes_batch, write_gff + write_translations
        t0 = time.perf_counter()
        recs = []
        with _cabi.FastaReader(fa) as rd:
            for batch in rd.batches():
                recs.extend(batch)
        gl = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_genes_batch([s for _, _, s in recs])
        with open(os.path.join(tmp, "h.gff"), "w") as g1, open(os.path.join(tmp, "h.faa"), "w") as g2:
            for g, (sid, _, _) in zip(gl, recs):
                g.write_gff(g1, sid)
                g.write_translations(g2, sid)
        out["host_loop_wall_s"] = time.perf_counter() - t0
        out["host_loop_gbps"] = bases / out["host_loop_wall_s"] / 1e9
        out["cli_over_host_loop"] = out["host_loop_wall_s"] / out["cli_wall_s"]
        # ... and the loop -f gbk -s replaced: find_genes_batch with the nodes, write_genbank + write_scores
        t0 = time.perf_counter()
        gl = lib.GeneFinder(meta=True, metagenomic_bins=bins, keep_nodes=True).find_genes_batch([s for _, _, s in recs])
        with open(os.path.join(tmp, "h.gbk"), "w") as g1, open(os.path.join(tmp, "h.scores"), "w") as g2:
            for g, (sid, _, _) in zip(gl, recs):
                g.write_genbank(g1, sid)
                g.write_scores(g2, sid)
        out["host_loop_gbk_scores_wall_s"] = time.perf_counter() - t0
        out["cli_gbk_scores_over_host_loop"] = out["host_loop_gbk_scores_wall_s"] / out["cli_gbk_scores_wall_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
