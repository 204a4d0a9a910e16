"""One GAT layer at the Products shape through the mirror's gat_aggregate_apply, forward and
backward with autograd, alternated in one process, medians over --reps runs:

    exact       FIXED, the exact statistics pair (gala_gat_{fwd,bwd}_stats_exact_f32)
    fixed_old   FIXED with GALA_GAT_EXACT_STATS=0: the alpha-storing path (what ran before)
    ref_stats   REF, the row-statistics pair (gala_gat_{fwd,bwd}_stats_f32)

for 8 heads x 32 (F = 256) and 1 head, F = 47.  Prints one JSON line per variant and shape with
the times and the peak allocation above the layer's inputs and outputs.

    python tools/gat_exact_bench.py [--graph uniform|rmat] [--scale 1.0] [--reps 5] [--out FILE]

Exits 1 if the exact pair is not faster than the alpha-storing path on some shape.
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
ENV = "GALA_GAT_EXACT_STATS"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=("uniform", "rmat"), default="uniform")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import bench
    import gala
    from gala import layout
    E = gala.torch_ext()
    g = bench.products_graph(a.graph, a.scale)
    t, perm = layout.transpose(g)
    assert np.array_equal(t.rowptr, g.rowptr) and np.array_equal(t.col, g.col), "a symmetric graph"
    E.slots_clear()
    off, cols = torch.from_numpy(g.rowptr).cuda(), torch.from_numpy(g.col).cuda()
    vals = torch.ones(g.nnz, device="cuda")
    # layer 0: a FIXED program's slots (the transpose uploaded apart, with its edge permutation);
    # layer 1: an undirected REF program's (slot 3 is slot 2)
    E.slots_push(off, cols, vals, None, 1, False)
    E.slots_push(torch.from_numpy(t.rowptr).cuda(), torch.from_numpy(t.col).cuda(), vals, None, 1, False)
    E.slots_set_transpose_perm(1, torch.from_numpy(perm).cuda())
    E.slots_push(off, cols, vals, None, 1, False)
    E.slots_push(off, cols, vals, None, 1, False)
    del t, perm
    gen = torch.Generator(device="cuda").manual_seed(5)
    ok = True
    for H, F in ((8, 256), (1, 47)):
        n = g.n_rows
        aL, aR = ((torch.rand(n, H, device="cuda", generator=gen) * 2 - 1).requires_grad_() for _ in range(2))
        x = (torch.rand(n, F, device="cuda", generator=gen) * 2 - 1).requires_grad_()
        dY = torch.rand(n, F, device="cuda", generator=gen) * 2 - 1
        ins = (aL, aR, x)
        variants = {"exact": ("1", 0, 1), "fixed_old": ("0", 0, 1), "ref_stats": ("1", 1, 0)}   # env, layer, mode
        res = {k: {"fwd": [], "bwd": [], "peak": 0} for k in variants}
        outs = {}
        for rep in range(a.reps + 1):
            for name, (env, li, mode) in variants.items():
                os.environ[ENV] = env
                for p in ins:
                    p.grad = None
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                e[0].record()
                Y = E.gat_aggregate_apply(aL, aR, x, li, 0.2, mode)
                e[1].record()
                Y.backward(dY)
                e[2].record()
                torch.cuda.synchronize()
                made = Y.numel() * 4 + sum(p.grad.numel() * 4 for p in ins)
                res[name]["peak"] = max(res[name]["peak"], torch.cuda.max_memory_allocated() - base - made)
                if rep > 0:
                    res[name]["fwd"].append(e[0].elapsed_time(e[1]))
                    res[name]["bwd"].append(e[1].elapsed_time(e[2]))
                else:
                    outs[name] = [Y.detach().clone()] + [p.grad.clone() for p in ins]
                del Y
        os.environ.pop(ENV, None)
        # the two FIXED paths compute the same layer
        err = {nm: float((u - v).abs().max() / max(v.abs().max().item(), 1e-30))
               for nm, u, v in zip(("Y", "d_aL", "d_aR", "dX"), outs["exact"], outs["fixed_old"])}
        med = {k: (float(np.median(r["fwd"])), float(np.median(r["bwd"]))) for k, r in res.items()}
        for name in variants:
            f, b = med[name]
            line = {"variant": name, "graph": a.graph, "n": n, "nnz": g.nnz, "heads": H, "F": F, "fwd_ms": round(f, 3),
                    "bwd_ms": round(b, 3), "layer_ms": round(f + b, 3), "peak_above_io_bytes": int(res[name]["peak"]),
                    "alpha_bytes": g.nnz * H * 4, "layer_vs_fixed_old": round((f + b) / sum(med["fixed_old"]), 4),
                    "fwd_vs_ref_stats": round(f / med["ref_stats"][0], 4), "bwd_vs_ref_stats": round(b / med["ref_stats"][1], 4),
                    "fwd_all": res[name]["fwd"], "bwd_all": res[name]["bwd"]}
            if name == "exact":
                line["max_rel_diff_vs_fixed_old"] = err
            s = json.dumps(line)
            print(s, flush=True)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(s + "\n")
        # the alpha-storing path holds alpha, its transpose and dz: at least three E * H arrays more
        assert res["fixed_old"]["peak"] - res["exact"]["peak"] >= 2 * g.nnz * H * 4, "the switch did not switch paths"
        ok = ok and sum(med["exact"]) < sum(med["fixed_old"])
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
