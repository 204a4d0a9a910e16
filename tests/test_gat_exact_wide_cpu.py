"""The exact GAT pair's host twins on rows of 257 .. 1024 floats (the head dots in the wide
kernels' grouping, 4 or 8 edges per rescale) against the float64 layer, with the constants of
tests/_gat_exact_ref.py unchanged.  GALA_GAT_EXACT_RECORD (a JSON-lines file) takes the worst
ratios: profiles/gat_exact_wide_bounds_cpu.jsonl holds them."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import _edge_ref as E
import _gat_exact_ref as X
from gala import backend

SHAPES = ((512, 8), (320, 5), (768, 2), (1024, 32), (260, 1))     # (F, heads)


@pytest.mark.parametrize("rc,big", [(False, False), (True, True)], ids=["aR-plain", "rc-big"])
@pytest.mark.parametrize("F,H", SHAPES, ids=lambda v: str(v))
def test_wide_twins_against_float64(F, H, rc, big):
    g = X.graph("cora")
    i = X.inputs(g, H, F, rc, big)
    be = backend.CpuBackend()
    cg = be.graph(g)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    aL, Xt = t(i.aL), t(i.X)
    if rc:
        Y, lse, Ym, sma, aR = be.gat_stats_exact(cg, aL, None, Xt, H, X.SLOPE, wR=t(i.wR), bR=t(i.bR))
        ar64, arm = X.source_logits(i.X, i.wR, i.bR, H)
        E.assert_bounded("aR_out", aR.numpy(), ar64, arm, X.C_AR, g=g, per="row", record=False)
    else:
        Y, lse, Ym, sma, aR = be.gat_stats_exact(cg, aL, t(i.aR), Xt, H, X.SLOPE)
    dX, daL, daR = be.gat_bwd_stats_exact(cg, aL, aR, Xt, t(i.dY), lse, Y, Ym, sma, H, X.SLOPE)
    ref = X.exact_layer(g, i.aL, aR.numpy(), i.X, i.dY, H)
    got = dict(Y=Y, Ym=Ym, sma=sma, lse=lse, dX=dX, daL=daL, daR=daR)
    case = X.case_id(("cora", H, F, rc, big))
    worst = X.check(case, {k: v.numpy().reshape(g.n_rows, -1) for k, v in got.items()}, ref, g)
    path = os.environ.get("GALA_GAT_EXACT_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "backend": "cpu", **worst}) + "\n")
