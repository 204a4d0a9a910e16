#!/usr/bin/env python3
"""In-process A/B of builds of libgala_hip.so on the exact GAT pair (gala_gat_{fwd,bwd}_stats_exact_f32)
at the Products shape, 8 heads x 32 (source logits recomputed) and 1 head, F = 47 (given), as
tools/ab_gat.py does it for the REF statistics pair: the builds tools/ab/libgala_hip_<label>.so
(other commits: git worktree + make; the SAME build under two labels gives that build's own
run-to-run range inside this process) and "tree", this tree's library, run alternately on the
same inputs.  For "tree" the backward is also timed as its two table calls at self_col NULL
(gala_gat_bwd_exact_pre_ex_f32 + gala_gat_bwd_exact_gather_ex_f32: two launches, what
gala.dist.HaloGatExact runs with the side-line exchange between them).  Prints one JSON line per
round and build, then per shape the medians, tree / build ratios, the per-round spread between
builds and whether every build's outputs are bit-identical to the tree's.  Measurement only.

    python tools/ab_gat_exact.py [--graph uniform|rmat] [--rounds 5] [--out FILE]
"""
import argparse
import ctypes
import glob
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gala-gnn-acceleration-language_amd"))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from ab_gat import load  # noqa: E402
from gala import _abi, ops  # noqa: E402

SLOPE = 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", choices=("uniform", "rmat"), default="uniform")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    libs = {os.path.basename(f)[len("libgala_hip_"):-3]: load(f)
            for f in sorted(glob.glob(os.path.join(ROOT, "tools", "ab", "libgala_hip_*.so")))}
    libs["tree"] = _abi.lib()
    fns = {k: ctypes.cast(L.gala_gat_fwd_stats_exact_f32, ctypes.c_void_p).value for k, L in libs.items()}
    assert len(set(fns.values())) == len(fns), fns   # every build loaded as its own copy

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(s + "\n")

    hg = bench.products_graph(a.graph, 1.0)
    dg = ops.DeviceGraph.from_host(hg)
    N = hg.n_rows
    timer = bench.Timer(True)
    gen = torch.Generator(device="cuda").manual_seed(4321)
    for H, F, rc in ((8, 256, True), (1, 47, False)):
        X = torch.rand((N, F), device="cuda", generator=gen) * 2 - 1
        dY = torch.rand((N, F), device="cuda", generator=gen) * 2 - 1
        aL = torch.rand((N, H), device="cuda", generator=gen) - 0.5
        aR = torch.rand((N, H), device="cuda", generator=gen) - 0.5
        wR = (torch.rand(F, device="cuda", generator=gen) - 0.5) * 0.2
        bR = torch.zeros(H, device="cuda")
        side = torch.empty((N, 4 * H), device="cuda")
        outs, samples = {}, {k: [] for k in list(libs) + ["tree_pre+gather"]}
        for r in range(a.rounds + 1):          # round 0: warm-up, not recorded
            for k in libs:
                _abi._lib = libs[k]
                st = {}

                def fwd():
                    st["f"] = ops.gat_fwd_stats_exact(dg, aL, X, aR=None if rc else aR, wR=wR if rc else None,
                                                      bR=bR if rc else None, heads=H, slope=SLOPE)

                def bwd():
                    Y, lse, Ym, sma, ar = st["f"]
                    st["b"] = ops.gat_bwd_stats_exact(dg, aL, ar, X, dY, lse, Y, Ym, sma, heads=H, slope=SLOPE,
                                                      symmetric=True)

                def split():   # the same backward as two launches (tree only)
                    Y, lse, Ym, sma, ar = st["f"]
                    d_aL = ops.gat_bwd_exact_pre_table(dg, aL, dY, lse, Y, Ym, sma, None, side, heads=H)
                    dX, d_aR = ops.gat_bwd_exact_gather_table(dg, ar, X, dY, side, None, heads=H, slope=SLOPE)
                    st["s"] = (dX, d_aL, d_aR)
                fwd()
                bwd()
                torch.cuda.synchronize()
                if k not in outs:
                    outs[k] = [t.clone() for t in st["f"]] + [t.clone() for t in st["b"]]
                tf, tb = timer(fwd, 10), timer(bwd, 10)
                rec = {"graph": a.graph, "heads": H, "F": F, "round": r, "lib": k, "fwd_ms": round(tf * 1e3, 4),
                       "bwd_ms": round(tb * 1e3, 4)}
                if k == "tree":
                    split()
                    torch.cuda.synchronize()
                    if "tree_pre+gather" not in outs:
                        outs["tree_pre+gather"] = [t.clone() for t in st["s"]]
                    ts = timer(split, 10)
                    rec["bwd_pre_gather_ms"] = round(ts * 1e3, 4)
                    if r > 0:
                        samples["tree_pre+gather"].append((tf * 1e3, ts * 1e3))
                if r > 0:
                    samples[k].append((tf * 1e3, tb * 1e3))
                    emit(rec)
                del st
        _abi._lib = libs["tree"]
        same = {k: all(torch.equal(u, v) for u, v in zip(outs[k], outs["tree"])) for k in libs}
        same["tree_pre+gather"] = all(torch.equal(u, v) for u, v in zip(outs["tree_pre+gather"], outs["tree"][5:]))
        med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
        summ = {k: {"fwd_ms_median": round(med([f for f, _ in v]), 4), "bwd_ms_median": round(med([b for _, b in v]), 4),
                    "fwd_ms_min_max": [round(min(f for f, _ in v), 4), round(max(f for f, _ in v), 4)],
                    "bwd_ms_min_max": [round(min(b for _, b in v), 4), round(max(b for _, b in v), 4)]}
                for k, v in samples.items()}
        ratio = {k: {"fwd": round(summ["tree"]["fwd_ms_median"] / summ[k]["fwd_ms_median"], 4),
                     "bwd": round(summ["tree"]["bwd_ms_median"] / summ[k]["bwd_ms_median"], 4)} for k in libs if k != "tree"}
        emit({"graph": a.graph, "n": N, "nnz": hg.nnz, "heads": H, "F": F, "recomputed_aR": rc, "rounds": a.rounds,
              "summary": summ, "tree_over_build_median": ratio, "bit_identical_to_tree": same})
        del X, dY, side, outs


if __name__ == "__main__":
    main()
