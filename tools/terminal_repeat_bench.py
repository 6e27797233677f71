"""Direct terminal repeats: what the detection and the trimmed copy cost in front of the circular call, on one device.

Three shapes, every batch resident, meta mode with the 16 models of `benchdata.load_model_set()`, one context:

  meta_none   6 250 x 20 kbp, every contig searched, none has a repeat            (a) the plain call
  meta_all    the same contigs with their first 127 bases appended to each        (a) the circular call on the contigs as they were
  one_5m      one 5 Mbp contig with its first 10 kbp appended                     (a) the circular call on the 5 Mbp

(b) is always detection + trimmed copy + call on the batch with the repeats.  Rounds of (a) and (b) alternate; host clock around the
calls, min / median / max.  The detection alone and the copy alone are timed in rounds of their own.

    python tools/terminal_repeat_bench.py --json profiles/terminal_repeat_timings.json
    rocprofv3 --kernel-trace --stats ... -- python tools/terminal_repeat_bench.py --shapes meta_all --calls 6 --only b

`--only plain` runs the plain call and the circular call of a shape without the option, through nothing but the parent commit's
interface: the same script under the parent's tree gives the kernel list to compare with.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.environ.get("PGA_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(which, procs):
    from pyrodigal_amd import benchdata
    out = {}
    if "meta_none" in which or "meta_all" in which:
        n = 6250
        lengths, gcs, seeds = benchdata.config4_spec()
        t = benchdata.generate(lengths[:n * 16:16], gcs[:n * 16:16], seeds[:n * 16:16], procs=procs)
        if "meta_none" in which:
            out["meta_none"] = (t, t, None)
        if "meta_all" in which:
            out["meta_all"] = ([s + s[:127] for s in t], t, True)
    if "one_5m" in which:
        t = benchdata.config2()
        out["one_5m"] = ([t[0] + t[0][:10_000]], t, True)
    return out


def summary(xs):
    return {"min_ms": min(xs) * 1e3, "median_ms": statistics.median(xs) * 1e3, "max_ms": max(xs) * 1e3}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--shapes", default="meta_none,meta_all,one_5m")
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=0, help="no timing: this many calls of what --only names (for a kernel trace)")
    ap.add_argument("--only", choices=("a", "b", "plain"), default=None)
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--json", help="also write the result here")
    args = ap.parse_args()
    from pyrodigal_amd import _cabi, benchdata
    ctx = _cabi.Context(0)
    ctx.set_models([m[1] for m in benchdata.load_model_set()])
    result = {"device": ctx.device_info()["name"], "rounds": args.rounds, "shapes": {}}
    for name, (S, T, flags) in shapes(args.shapes.split(","), args.procs).items():
        bS = ctx.upload(S)
        bT = bS if T is S else ctx.upload(T)
        if flags:
            bT.set_circular(flags)

        def call_a():
            return ctx.find_genes(bT, meta=True)

        def call_b():
            _, trim = bS.terminal_repeats()
            t = bS.trim_terminal_repeats(trim)
            try:
                return ctx.find_genes(t, meta=True), trim
            finally:
                if t is not bS:
                    t.close()

        if args.calls:
            for _ in range(args.calls):
                if args.only == "plain":          # the parent's interface only
                    lin = ctx.upload(T)
                    ctx.find_genes(lin, meta=True)
                    lin.close()
                    call_a()
                elif args.only == "a":
                    call_a()
                else:
                    call_b()
            bS.close()
            if bT is not bS:
                bT.close()
            continue
        ra = call_a()
        rb, trim = call_b()
        same = ra.genes.tobytes() == rb.genes.tobytes() and (ra.cuts is None) == (rb.cuts is None) and (ra.cuts is None or ra.cuts.tolist() == rb.cuts.tolist())
        for _ in range(args.warmup):
            call_a(); call_b()
        ta, tb, td, tc = [], [], [], []
        for _ in range(args.rounds):
            t0 = time.perf_counter(); call_a(); t1 = time.perf_counter(); call_b(); t2 = time.perf_counter()
            ta.append(t1 - t0); tb.append(t2 - t1)
        for _ in range(args.rounds):
            t0 = time.perf_counter(); _, tr = bS.terminal_repeats(); t1 = time.perf_counter()
            t = bS.trim_terminal_repeats(tr); t2 = time.perf_counter()
            if t is not bS:
                t.close()
            td.append(t1 - t0); tc.append(t2 - t1)
        result["shapes"][name] = {
            "contigs": len(S), "mbp": sum(len(s) for s in S) / 1e6, "genes": int(len(rb.genes)), "trimmed": int((trim > 0).sum()),
            "identical_to_a": bool(same), "a_call": summary(ta), "b_detect_trim_call": summary(tb),
            "b_over_a": {"min": min(tb) / min(ta), "median": statistics.median(tb) / statistics.median(ta)},
            "detect_alone": summary(td), "trim_alone": summary(tc)}
        bS.close()
        if bT is not bS:
            bT.close()
    ctx.close()
    if not args.calls:
        print(json.dumps(result))
        if args.json:
            with open(args.json, "w") as f:
                json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
