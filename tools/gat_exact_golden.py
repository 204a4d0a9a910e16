#!/usr/bin/env python3
"""Writes tests/golden/gat_exact/gat_exact_square_<graph>.npz: the square exact pair's host-twin outputs
(gala_cpu_gat_{fwd,bwd}_stats_exact_f32 through gala.backend.CpuBackend) for one case per graph
of tests/_gat_exact_ref.py, under the plan X.PLAN.  It calls only the square entry points, so it
runs unchanged on the commit before the rectangular calls existed (42af8ce), which is where the
committed files come from:

    python tools/gat_exact_golden.py

Each file holds, per output, the sha256 of the whole array and a copy of a row subset (every hub
row and every STRIDE-th row), which keeps a file far below the size limit for committed files.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "gala-gnn-acceleration-language_amd"), os.path.join(ROOT, "oracle"),
          os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import _gat_exact_ref as X  # noqa: E402
from gala import backend  # noqa: E402

# (graph, heads, F, aR recomputed, logits past 30)
GOLDEN_CASES = (("cora", 1, 47, True, False), ("hub", 3, 24, False, True), ("long", 8, 256, True, False))
STRIDE = 32
NAMES = ("Y", "lse", "Ym", "sma", "aR", "dX", "daL", "daR")


def square_outputs(case):
    """The eight arrays of NAMES, each [n, -1] float32, from the square host twins."""
    name, H, F, rc, big = case
    g = X.graph(name)
    i = X.inputs(g, H, F, rc, big)
    be = backend.CpuBackend()
    cg = be.graph(g)
    cg.set_split_plan(*X.PLAN)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    aL, Xt, dY = t(i.aL), t(i.X), t(i.dY)
    if rc:
        f = be.gat_stats_exact(cg, aL, None, Xt, H, X.SLOPE, wR=t(i.wR), bR=t(i.bR))
    else:
        f = be.gat_stats_exact(cg, aL, t(i.aR), Xt, H, X.SLOPE)
    b = be.gat_bwd_stats_exact(cg, aL, f[4], Xt, dY, f[1], f[0], f[2], f[3], H, X.SLOPE)
    return {k: np.ascontiguousarray(v.numpy().reshape(g.n_rows, -1)) for k, v in zip(NAMES, tuple(f) + tuple(b))}


def subset_rows(name):
    g = X.graph(name)
    hub = np.flatnonzero(np.diff(g.rowptr) > X.PLAN[0])
    return np.unique(np.concatenate([hub, np.arange(0, g.n_rows, STRIDE)])).astype(np.int64)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    out = os.path.join(ROOT, "tests", "golden", "gat_exact")   # apart from the oracle fixtures tests/golden/*.npz
    os.makedirs(out, exist_ok=True)
    for case in GOLDEN_CASES:
        o = square_outputs(case)
        rows = subset_rows(case[0])
        rec = {"rows": rows, "case": np.array(X.case_id(case))}
        for k, v in o.items():
            rec[k] = v[rows]
            rec[k + "_sha256"] = np.array(digest(v))
        path = os.path.join(out, f"gat_exact_square_{case[0]}.npz")
        np.savez(path, **rec)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
