#!/usr/bin/env python3
"""In-process A/B of a directed FIXED GAT layer through the operator mirror: the directed exact
pair (GALA_GAT_EXACT_DIRECTED=1: gala_gat_fwd_stats_exact_f32 + gala_gat_bwd_stats_exact_t_f32)
against the alpha-storing path of the same build, the switch toggled per call, alternately for
`rounds` rounds after tools/ab_gat_exact.py.  The graph is the Products-shaped R-MAT graph of
bench.py made directed (its distinct edges, each stored direction kept with probability 1/2), at
8 heads x 32 and 1 head x 47.  Also timed: gala_csr_is_transpose_i32; also recorded: each path's
peak allocation above the layer's inputs (its output and gradients included).  Prints one JSON line per round and path
and a summary per shape.  Measurement only.

    python tools/ab_gat_exact_directed.py [--scale 1.0] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gala-gnn-acceleration-language_amd"))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import gala  # noqa: E402
from gala import layout, ops  # noqa: E402

SLOPE = 0.2
ENV = "GALA_GAT_EXACT_DIRECTED"


def directed(hg, seed=1):
    n = hg.n_rows
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(hg.rowptr.astype(np.int64)))
    key = np.unique(rows * n + hg.col.astype(np.int64))
    key = key[np.random.default_rng(seed).random(key.shape[0]) < 0.5]
    return layout.csr_build(n, n, (key // n).astype(np.int32), (key % n).astype(np.int32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")

    T = gala.torch_ext()
    g = directed(bench.products_graph("rmat", a.scale))
    gT, perm = layout.transpose(g)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    T.slots_clear()
    T.slots_push(dev(g.rowptr), dev(g.col), torch.ones(g.nnz, device="cuda"), None, 1, False)
    T.slots_push(dev(gT.rowptr), dev(gT.col), torch.ones(gT.nnz, device="cuda"), None, 1, False)
    T.slots_set_transpose_perm(1, dev(perm))
    N = g.n_rows
    timer = bench.Timer(True)
    dg, dgT = ops.DeviceGraph.from_host(g, split=False), ops.DeviceGraph.from_host(gT, split=False)
    assert ops.is_transpose(dg, dgT)
    t_check = timer(lambda: ops.is_transpose(dg, dgT), 10)
    emit({"n": N, "nnz": g.nnz, "max_out_degree": int(np.diff(g.rowptr).max()),
          "max_in_degree": int(np.diff(gT.rowptr).max()), "is_transpose_ms": round(t_check * 1e3, 4)})
    del dg, dgT
    gen = torch.Generator(device="cuda").manual_seed(4321)
    for H, F in ((8, 256), (1, 47)):
        X = (torch.rand((N, F), device="cuda", generator=gen) * 2 - 1).requires_grad_()
        dY = torch.rand((N, F), device="cuda", generator=gen) * 2 - 1
        aL = (torch.rand((N, H), device="cuda", generator=gen) - 0.5).requires_grad_()
        aR = (torch.rand((N, H), device="cuda", generator=gen) - 0.5).requires_grad_()

        def layer():
            for t in (X, aL, aR):
                t.grad = None
            T.gat_aggregate_apply(aL, aR, X, 0, SLOPE, 1).backward(dY)

        samples, peaks = {"directed": [], "alpha": []}, {}
        for r in range(a.rounds + 1):              # round 0: warm-up, not recorded
            for path in ("directed", "alpha"):
                os.environ[ENV] = "1" if path == "directed" else "0"
                layer()
                for t in (X, aL, aR):              # the warm call's gradients are not part of the base
                    t.grad = None
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                layer()
                torch.cuda.synchronize()
                peaks[path] = torch.cuda.max_memory_allocated() - base
                ms = timer(layer, 5) * 1e3
                if r > 0:
                    samples[path].append(ms)
                    emit({"heads": H, "F": F, "round": r, "path": path, "fwd_bwd_ms": round(ms, 4)})
        os.environ.pop(ENV, None)
        med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
        emit({"heads": H, "F": F, "rounds": a.rounds,
              "summary": {k: {"fwd_bwd_ms_median": round(med(v), 4), "min_max": [round(min(v), 4), round(max(v), 4)],
                              "peak_bytes_above_inputs": int(peaks[k])} for k, v in samples.items()},
              "directed_over_alpha_median": round(med(samples["directed"]) / med(samples["alpha"]), 4),
              "alpha_array_bytes": g.nnz * H * 4})
        del X, dY, aL, aR


if __name__ == "__main__":
    main()
