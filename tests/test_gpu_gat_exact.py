"""The exact GAT pair on the GPU (gala_gat_{fwd,bwd}_stats_exact_f32): every output against the
float64 layer per element (the constants of tests/_gat_exact_ref.py, measured on the host
twins) and against the twins, run-to-run bit identity, the hub-row plan, the argument checks."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import _edge_ref as E
import _gat_exact_ref as X
from gala import _abi, backend, ops

pytestmark = pytest.mark.gpu
NAMES = ("Y", "lse", "Ym", "sma", "dX", "daL", "daR")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(dg, i, H, pad=False):
    """(outputs in NAMES order as device tensors, aR used)."""
    aL, Xd, dY = _dev(i.aL), _dev(i.X), _dev(i.dY)
    if pad:
        Xd, dY = ops.pad_rows(Xd), ops.pad_rows(dY)
    if i.rc:
        Y, lse, Ym, sma, aR = ops.gat_fwd_stats_exact(dg, aL, Xd, wR=_dev(i.wR), bR=_dev(i.bR), heads=H, slope=X.SLOPE)
    else:
        Y, lse, Ym, sma, aR = ops.gat_fwd_stats_exact(dg, aL, Xd, aR=_dev(i.aR), heads=H, slope=X.SLOPE)
    dX, daL, daR = ops.gat_bwd_stats_exact(dg, aL, aR, Xd, dY, lse, Y, Ym, sma, heads=H, slope=X.SLOPE)
    return (Y, lse, Ym, sma, dX, daL, daR), aR


def _host(outs, n):
    return {k: v.cpu().numpy().reshape(n, -1) for k, v in zip(NAMES, outs)}


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_kernels_against_float64_and_twins(case):
    name, H, F, rc, big = case
    g = X.graph(name)
    i = X.inputs(g, H, F, rc, big)
    dg = ops.DeviceGraph.from_host(g)
    assert (dg.split_rows > 0) == (name != "cora")
    outs, aR = _run(dg, i, H)
    again, _ = _run(dg, i, H)
    torch.cuda.synchronize()
    for k, a, b in zip(NAMES, outs, again):
        assert torch.equal(a, b), f"{k}: not bit-identical run to run"
    got = _host(outs, g.n_rows)
    aRh = aR.cpu().numpy()
    if rc:
        ar64, arm = X.source_logits(i.X, i.wR, i.bR, H)
        E.assert_bounded("aR_out", aRh, ar64, arm, X.C_AR, g=g, per="row", record=False)
    ref = X.exact_layer(g, i.aL, aRh, i.X, i.dY, H)
    worst = X.check("gpu " + X.case_id(case), got, ref, g)
    path = os.environ.get("GALA_GAT_EXACT_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": X.case_id(case), "backend": "hip", **worst}) + "\n")
    # the twins from the same source logits: two fp32 evaluations of one element, each within c
    be = backend.CpuBackend()
    cg = be.graph(g)
    cg.set_split_plan(*X.PLAN)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    Y, lse, Ym, sma, _ = be.gat_stats_exact(cg, t(i.aL), t(aRh), t(i.X), H, X.SLOPE)
    dX, daL, daR = be.gat_bwd_stats_exact(cg, t(i.aL), t(aRh), t(i.X), t(i.dY), lse, Y, Ym, sma, H, X.SLOPE)
    twin = dict(Y=Y, lse=lse, Ym=Ym, sma=sma, dX=dX, daL=daL, daR=daR)
    for k in NAMES:
        E.assert_bounded(f"gpu vs twin {k}", got[k], twin[k].numpy().reshape(g.n_rows, -1), getattr(ref, k + "_mass"),
                         2 * X.C[k], g=g, per="row", chunk=X.PLAN[1], record=False)


def test_padded_rows_take_the_vector_path():
    """F = 47 in rows padded to 48 floats (float4 loads, 12 lanes) against the float64 layer."""
    g = X.graph("hub")
    i = X.inputs(g, 1, 47, False, True)
    dg = ops.DeviceGraph.from_host(g)
    outs, aR = _run(dg, i, 1, pad=True)
    ref = X.exact_layer(g, i.aL, aR.cpu().numpy(), i.X, i.dY, 1)
    X.check("gpu padded F47", _host(outs, g.n_rows), ref, g)


def test_rows_below_the_threshold_do_not_depend_on_the_plan():
    """With and without the hub-row plan: the forward's rows and d_aL of every row at or below
    the threshold are bit-identical; dX and d_aR of such a row read its neighbours' side lines
    (lse, g), so they are bit-identical where no neighbour is a hub row."""
    g = X.graph("long")
    i = X.inputs(g, 8, 64, False, False)
    a, _ = _run(ops.DeviceGraph.from_host(g), i, 8)
    b, _ = _run(ops.DeviceGraph.from_host(g, split=False), i, 8)
    a, b = _host(a, g.n_rows), _host(b, g.n_rows)
    hub = np.diff(g.rowptr) > X.PLAN[0]
    assert hub.sum() >= 4
    for k in ("Y", "lse", "Ym", "sma", "daL"):
        assert np.array_equal(a[k][~hub], b[k][~hub]), k
    assert any(not np.array_equal(a[k][hub], b[k][hub]) for k in NAMES)
    # the gather itself does not depend on the plan: dX and d_aR of every ordinary row with no
    # hub neighbour (its side lines are ordinary rows' too) are bit-identical as well
    far = ~hub & ~X.has_neighbour_in(g, hub)
    assert far.sum() > 50
    for k in ("dX", "daR"):
        assert np.array_equal(a[k][far], b[k][far]), k
    ref = X.exact_layer(g, i.aL, i.aR, i.X, i.dY, 8)
    X.check("gpu no plan", b, ref, g)


def test_argument_checks():
    g = X.graph("hub")
    H, F = 8, 64
    i = X.inputs(g, H, F, False, False)
    dg = ops.DeviceGraph.from_host(g)
    aL, aR, Xd, dY = _dev(i.aL), _dev(i.aR), _dev(i.X), _dev(i.dY)
    Y, lse, Ym, sma, _ = ops.gat_fwd_stats_exact(dg, aL, Xd, aR=aR, heads=H, slope=X.SLOPE)
    n = g.n_rows
    out = [torch.full((n, F), 7.0, device="cuda"), torch.full((n * H,), 7.0, device="cuda"),
           torch.full((n * H,), 7.0, device="cuda")]
    side = torch.empty(n * H * 4, device="cuda")

    def bwd(csr):
        return _abi.lib().gala_gat_bwd_stats_exact_f32(
            csr, aL.data_ptr(), aR.data_ptr(), Xd.data_ptr(), F, dY.data_ptr(), F, F, H, X.SLOPE, lse.data_ptr(),
            Y.data_ptr(), F, Ym.data_ptr(), F, sma.data_ptr(), side.data_ptr(), out[0].data_ptr(), F,
            out[1].data_ptr(), out[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
    # a plan with hub rows whose workspace is too small: refused, nothing launched
    plan = dg._split["plan"]
    need = 2 * F + H
    assert plan.ws_cols >= need
    keep = plan.ws_cols
    plan.ws_cols = need - 1
    try:
        assert bwd(dg.csr()) == _abi.GALA_ERR_INVALID_ARG
    finally:
        plan.ws_cols = keep
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in out)
    assert bwd(dg.csr()) == _abi.GALA_OK
    # a shape the statistics pair refuses
    j = X.inputs(g, 2, 12, False, False)
    with pytest.raises(_abi.GalaError) as e:
        ops.gat_fwd_stats_exact(dg, _dev(j.aL), _dev(j.X), aR=_dev(j.aR), heads=2)
    assert e.value.status == _abi.GALA_ERR_UNSUPPORTED
    # a directed pattern: the helper refuses before any launch
    d = ops.DeviceGraph.from_host(X.G.with_empty_rows())
    z, v = torch.zeros(d.n_rows, 4, device="cuda"), torch.zeros(d.n_rows, device="cuda")
    with pytest.raises(ValueError):
        ops.gat_bwd_stats_exact(d, v, v, z, z, v, z, z, v)
