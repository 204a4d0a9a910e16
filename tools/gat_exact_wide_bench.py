"""One GAT layer of 8 heads x 64 (F = 512) at the Products shape through the mirror's
gat_aggregate_apply, forward and backward with autograd, alternated in one process, medians over
--reps runs:

    exact_wide  FIXED, the exact statistics pair's wide kernels (gat_exact_wide.hip)
    ref_stats   REF, the row-statistics pair's wide kernels (gat_wide.hip)

the only two complete layers at this width.  Prints one JSON line per variant with the times, the
ratio to the REF pair and the peak allocation above the layer's inputs and outputs.

    python tools/gat_exact_wide_bench.py [--scale 1.0] [--reps 5] [--out FILE]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    import gala
    E = gala.torch_ext()
    g = bench.products_graph("uniform", a.scale)
    E.slots_clear()
    off, cols = torch.from_numpy(g.rowptr).cuda(), torch.from_numpy(g.col).cuda()
    vals = torch.ones(g.nnz, device="cuda")
    for _ in range(2):                       # one pattern in both slots: symmetric (tested by the mirror)
        E.slots_push(off, cols, vals, None, 1, False)
    gen = torch.Generator(device="cuda").manual_seed(5)
    H, F, n = 8, 512, g.n_rows
    aL, aR = ((torch.rand(n, H, device="cuda", generator=gen) * 2 - 1).requires_grad_() for _ in range(2))
    x = (torch.rand(n, F, device="cuda", generator=gen) * 2 - 1).requires_grad_()
    dY = torch.rand(n, F, device="cuda", generator=gen) * 2 - 1
    ins = (aL, aR, x)
    variants = {"exact_wide": 1, "ref_stats": 0}       # softmax mode
    res = {k: {"fwd": [], "bwd": [], "peak": 0} for k in variants}
    for rep in range(a.reps + 1):                      # the first round warms up
        for name, mode in variants.items():
            for p in ins:
                p.grad = None
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            e[0].record()
            Y = E.gat_aggregate_apply(aL, aR, x, 0, 0.2, mode)
            e[1].record()
            Y.backward(dY)
            e[2].record()
            torch.cuda.synchronize()
            made = Y.numel() * 4 + sum(p.grad.numel() * 4 for p in ins)
            res[name]["peak"] = max(res[name]["peak"], torch.cuda.max_memory_allocated() - base - made)
            if rep > 0:
                res[name]["fwd"].append(e[0].elapsed_time(e[1]))
                res[name]["bwd"].append(e[1].elapsed_time(e[2]))
            del Y
    layer = {k: [f + b for f, b in zip(r["fwd"], r["bwd"])] for k, r in res.items()}
    ref = float(np.median(layer["ref_stats"]))
    for name, r in res.items():
        line = {"variant": name, "n": n, "nnz": g.nnz, "heads": H, "F": F, "fwd_ms": round(float(np.median(r["fwd"])), 3),
                "bwd_ms": round(float(np.median(r["bwd"])), 3), "layer_ms": round(float(np.median(layer[name])), 3),
                "layer_vs_ref_stats": round(float(np.median(layer[name])) / ref, 4),
                "layer_vs_ref_stats_range": [round(min(layer[name]) / ref, 4), round(max(layer[name]) / ref, 4)],
                "peak_above_io_bytes": int(r["peak"]), "alpha_bytes": g.nnz * H * 4, "fwd_all": r["fwd"], "bwd_all": r["bwd"]}
        s = json.dumps(line)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")


if __name__ == "__main__":
    main()
