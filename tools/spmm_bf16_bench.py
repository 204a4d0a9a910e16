#!/usr/bin/env python3
"""fp32 against bf16 storage of the SpMM's gathered operand (GALA_SPMM_X_BF16), interleaved in
one process on bench.py's Products-shaped graphs (uniform, R-MAT, banded) at F = 32, 128, 256;
the R-MAT graph with and without its REF-order hub plan.

Both calls are gala_spmm_f32 with the dst norm on the same graph and the same (bf16-exact)
feature values, fp32 out; the outputs are compared bit for bit before anything is timed.  Times
are HIP events over `--reps` calls, the two storages alternating `--rounds` times (median and
spread reported).  The gather rate is edges * F * bytes-per-element of X over the time: the
bytes the algorithm asks for, not HBM traffic.  One JSON line per (graph, plan, F); needs a GPU.

    python3 tools/spmm_bf16_bench.py [--scale 1.0] [--out profiles/spmm_bf16.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "gala-gnn-acceleration-language_amd"), ROOT]
from gala import ops  # noqa: E402
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--graphs", default="uniform,rmat,banded")
    ap.add_argument("--features", default="32,128,256")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spmm_bf16_bench: needs a GPU (a CPU run gives no time)")
    timer = bench.Timer(True)
    out = open(args.out, "a") if args.out else None
    for kind in args.graphs.split(","):
        hg = bench.products_graph(kind, args.scale)
        plans = [("auto", ops.DeviceGraph.from_host(hg))]
        if plans[0][1].split_rows > 0:   # the same rows summed by the row kernel alone
            plans.append(("none", ops.DeviceGraph.from_host(hg, split=False)))
        for plan, dg in plans:
            norm = ops.degree(dg, power=-0.5)
            for F in (int(f) for f in args.features.split(",")):
                Xb = (torch.rand((hg.n_cols, F), device="cuda") * 2 - 1).to(torch.bfloat16)
                Xf = Xb.float()
                Yf, Yb = torch.empty_like(Xf[: hg.n_rows]), torch.empty_like(Xf[: hg.n_rows])
                run = {"fp32": lambda: ops.spmm(dg, Xf, out=Yf, dst_scale=norm),
                       "bf16": lambda: ops.spmm(dg, Xb, out=Yb, dst_scale=norm)}
                for fn in run.values():   # warm-up: code objects, the plan's workspace
                    fn()
                torch.cuda.synchronize()
                same = bool(torch.equal(Yf, Yb))
                ms = {k: [] for k in run}
                for _ in range(args.rounds):
                    for k, fn in run.items():
                        ms[k].append(timer(fn, args.reps) * 1e3)
                med = {k: statistics.median(v) for k, v in ms.items()}
                rec = {"graph": kind, "N": hg.n_rows, "E": hg.nnz, "plan": plan, "hub_rows": dg.split_rows, "F": F,
                       "bit_identical": same,
                       "fp32_ms": round(med["fp32"], 4), "bf16_ms": round(med["bf16"], 4),
                       "fp32_ms_range": [round(min(ms["fp32"]), 4), round(max(ms["fp32"]), 4)],
                       "bf16_ms_range": [round(min(ms["bf16"]), 4), round(max(ms["bf16"]), 4)],
                       "fp32_gather_GBps": round(hg.nnz * F * 4 / med["fp32"] / 1e6, 1),
                       "bf16_gather_GBps": round(hg.nnz * F * 2 / med["bf16"] / 1e6, 1),
                       "ratio_fp32_over_bf16": round(med["fp32"] / med["bf16"], 3),
                       "reps": args.reps, "rounds": args.rounds}
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                del Xb, Xf, Yf, Yb
    if out:
        out.close()


if __name__ == "__main__":
    main()
