"""The REF row-statistics pair (gat_fwd_stats + gat_bwd_stats, aR given) of one GAT layer of 3 heads
x 40 floats at the Products shape, alternated in one process with the only way to run that layer
without csrc/gat_headw.hip: every head zero-padded to 64 floats (F = 192) on the narrow kernels.

    headw    3 x 40 (F = 120), gat_headw.hip
    padded   3 x 64 (F = 192, columns 40..63 of every head zero), gat.hip / gat_fused.hip

HIP events, --rounds rounds of --calls calls per leg after one warm-up round; prints one JSON line
per leg (median and range of the forward, the backward and their sum) and the largest difference
of the two legs' Y and dX on the real columns.

    python tools/gat_head_widths_bench.py [--scale 1.0] [--rounds 3] [--calls 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "gala-gnn-acceleration-language_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    from gala import ops
    g = bench.products_graph("uniform", a.scale)
    dg = ops.DeviceGraph.from_host(g, split=False)
    gen = torch.Generator(device="cuda").manual_seed(5)
    H, D, DP, n = 3, 40, 64, g.n_rows
    aL, aR = (torch.rand(n, H, device="cuda", generator=gen) * 2 - 1 for _ in range(2))
    x, dY = (torch.rand(n, H, D, device="cuda", generator=gen) * 2 - 1 for _ in range(2))
    pad = lambda t: torch.nn.functional.pad(t, (0, DP - D)).reshape(n, H * DP).contiguous()
    legs = {"headw": (x.reshape(n, H * D), dY.reshape(n, H * D)), "padded": (pad(x), pad(dY))}
    res = {k: {"fwd": [], "bwd": []} for k in legs}
    out = {}
    for rnd in range(a.rounds + 1):                    # the first round warms up
        for name, (X, G) in legs.items():
            for _ in range(a.calls):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                Y, q, Ym, sma = ops.gat_fwd_stats(dg, aL, X, aR=aR, heads=H, slope=0.2)
                e[1].record()
                dX, daL = ops.gat_bwd_stats(dg, aL, aR, G, q, Y, Ym, sma, heads=H, slope=0.2)
                e[2].record()
                torch.cuda.synchronize()
                if rnd > 0:
                    res[name]["fwd"].append(e[0].elapsed_time(e[1]))
                    res[name]["bwd"].append(e[1].elapsed_time(e[2]))
            out[name] = (Y.view(n, H, -1)[:, :, :D], dX.view(n, H, -1)[:, :, :D], daL)
            del Y, q, Ym, sma, dX, daL
    diff = [float((u - v).abs().max()) for u, v in zip(out["headw"], out["padded"])]
    for name, r in res.items():
        pair = [f + b for f, b in zip(r["fwd"], r["bwd"])]
        stat = lambda v: [round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3)]
        line = {"leg": name, "n": n, "nnz": g.nnz, "heads": H, "D": D, "F": legs[name][0].shape[1],
                "fwd_ms_med_min_max": stat(r["fwd"]), "bwd_ms_med_min_max": stat(r["bwd"]),
                "pair_ms_med_min_max": stat(pair), "max_abs_diff_Y_dX_daL": diff}
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")


if __name__ == "__main__":
    main()
