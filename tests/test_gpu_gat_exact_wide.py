"""The exact GAT pair on rows of 257 .. 1024 floats (gat_exact_wide.hip, through the entry points
and operators of the narrow pair): every output per element against the float64 layer with the
constants of tests/_gat_exact_ref.py, the host twins, run-to-run bit identity, the directed form,
a FIXED 8 x 64 layer through the mirror, and the shapes that stay refused.
GALA_GAT_EXACT_RECORD (a JSON-lines file) takes the worst ratios of the pair:
profiles/gat_exact_wide_bounds_gpu.jsonl holds them."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import _edge_ref as E
import _gat_exact_directed_ref as D
import _gat_exact_ref as X
from gala import _abi, backend, ops

pytestmark = pytest.mark.gpu
NAMES = ("Y", "lse", "Ym", "sma", "dX", "daL", "daR")
SHAPES = ((512, 8), (320, 5), (768, 2), (1024, 32), (260, 1))     # (F, heads): 8 or 4 edges per batch
FIXED = _abi.GALA_SOFTMAX_FIXED


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _pair(dg, i, H):
    aL, Xd = _dev(i.aL), _dev(i.X)
    kw = dict(wR=_dev(i.wR), bR=_dev(i.bR)) if i.rc else dict(aR=_dev(i.aR))
    Y, lse, Ym, sma, aR = ops.gat_fwd_stats_exact(dg, aL, Xd, heads=H, slope=X.SLOPE, **kw)
    dX, daL, daR = ops.gat_bwd_stats_exact(dg, aL, aR, Xd, _dev(i.dY), lse, Y, Ym, sma, heads=H, slope=X.SLOPE)
    return (Y, lse, Ym, sma, dX, daL, daR), aR


def _host(outs, n):
    return {k: v.cpu().numpy().reshape(n, -1) for k, v in zip(NAMES, outs)}


def test_graphs_hold_every_batch_class():
    """Rows of degree 0, below U, exactly U, and above U without being a multiple, for U = 4 and 8."""
    deg = np.concatenate([np.diff(X.graph(k).rowptr) for k in ("cora", "hub")])
    assert deg.max() >= 1128
    for U in (4, 8):
        for cls in (deg == 0, (deg > 0) & (deg < U), deg == U, (deg > U) & (deg % U != 0)):
            assert cls.any(), U


@pytest.mark.parametrize("rc", [False, True], ids=["aR", "rc"])
@pytest.mark.parametrize("big", [False, True], ids=["plain", "big"])
@pytest.mark.parametrize("name", ["cora", "hub"])
@pytest.mark.parametrize("F,H", SHAPES, ids=lambda v: str(v))
def test_pair_against_float64_and_twins(F, H, name, big, rc):
    g = X.graph(name)
    i = X.inputs(g, H, F, rc, big)
    dg = ops.DeviceGraph.from_host(g, split=False)
    outs, aR = _pair(dg, i, H)
    again, _ = _pair(dg, i, H)
    torch.cuda.synchronize()
    for k, a, b in zip(NAMES, outs, again):
        assert torch.equal(a, b), f"{k}: not bit-identical run to run"
    got, aRh = _host(outs, g.n_rows), aR.cpu().numpy()
    if rc:
        ar64, arm = X.source_logits(i.X, i.wR, i.bR, H)
        E.assert_bounded("aR_out", aRh, ar64, arm, X.C_AR, g=g, per="row", record=False)
    ref = X.exact_layer(g, i.aL, aRh, i.X, i.dY, H)
    case = X.case_id((name, H, F, rc, big))
    worst = X.check("gpu " + case, got, ref, g)
    path = os.environ.get("GALA_GAT_EXACT_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": case, "backend": "hip", **worst}) + "\n")
    # the twins from the same source logits: two fp32 evaluations of one element, each within c
    be = backend.CpuBackend()
    cg = be.graph(g)
    Y, lse, Ym, sma, _ = be.gat_stats_exact(cg, _t(i.aL), _t(aRh), _t(i.X), H, X.SLOPE)
    dX, daL, daR = be.gat_bwd_stats_exact(cg, _t(i.aL), _t(aRh), _t(i.X), _t(i.dY), lse, Y, Ym, sma, H, X.SLOPE)
    twin = dict(Y=Y, lse=lse, Ym=Ym, sma=sma, dX=dX, daL=daL, daR=daR)
    for k in NAMES:
        E.assert_bounded(f"gpu vs twin {k}", got[k], twin[k].numpy().reshape(g.n_rows, -1), getattr(ref, k + "_mass"),
                         2 * X.C[k], g=g, per="row", record=False)


@pytest.mark.parametrize("F,H", [(512, 8), (260, 1)], ids=lambda v: str(v))
@pytest.mark.parametrize("flip", [False, True], ids=["uni", "uniT"])
def test_directed(F, H, flip):
    """gat_exact_directed on a directed graph and on its transpose, no plans; with AT == A on a
    symmetric graph the directed backward equals the symmetric one bit for bit."""
    g, gT = D.graph("uni"), D.transposed(D.graph("uni"))
    if flip:
        g, gT = gT, g
    i = X.inputs(g, H, F, flip, True)
    dg, dgT = ops.DeviceGraph.from_host(g, split=False), ops.DeviceGraph.from_host(gT, split=False)
    kw = dict(wR=_dev(i.wR), bR=_dev(i.bR)) if i.rc else dict(aR=_dev(i.aR))
    fwd, bwd = ops.gat_exact_directed(dg, dgT, _dev(i.aL), _dev(i.X), _dev(i.dY), heads=H, slope=X.SLOPE, **kw)
    ref = D.directed_layer(g, i.aL, fwd[4].cpu().numpy(), i.X, i.dY, H)
    D.check(f"directed F{F} {flip}", _host(fwd[:4] + bwd, g.n_rows), ref, c=X.C)
    s = X.graph("cora")
    j = X.inputs(s, H, F, False, False)
    ds = ops.DeviceGraph.from_host(s, split=False)
    (Y, lse, Ym, sma, dX, daL, daR), aR = _pair(ds, j, H)
    tb = ops.gat_bwd_stats_exact_t(ds, ds, _dev(j.aL), aR, _dev(j.X), _dev(j.dY), lse, Y, Ym, sma, heads=H, slope=X.SLOPE)
    assert all(torch.equal(a, b) for a, b in zip(tb, (dX, daL, daR)))


@pytest.mark.parametrize("ffn", [False, True], ids=["aR", "ffn"])
def test_fixed_layer_through_the_mirror(ffn, monkeypatch):
    """A FIXED layer of 8 x 64 on a symmetric pattern through gat_aggregate_apply / gat_aggregate_ffn_apply
    against the float64 layer.  ffn: dX is two terms (the layer's dX and d_aR wR), bounded by the larger
    of their constants times their masses; dW sums n products in fp32: (n + 1) * 2^-24 + C["daR"] times
    its mass.  GALA_GAT_EXACT_STATS=0 leaves no backward at this width: refused."""
    import gala
    F, H, g, M = 512, 8, X.graph("cora"), gala.torch_ext()
    i = X.inputs(g, H, F, ffn, False)
    off, cols = _dev(g.rowptr), _dev(g.col)
    M.slots_clear()
    for _ in range(2):
        M.slots_push(off, cols, torch.ones(g.nnz, device="cuda"), None, 1, False)
    src = (i.aL, i.X, i.wR.reshape(1, -1), i.bR) if ffn else (i.aL, i.aR, i.X)
    ins = [_dev(a).requires_grad_() for a in src]
    apply = M.gat_aggregate_ffn_apply if ffn else M.gat_aggregate_apply
    Y = apply(*ins, 0, X.SLOPE, FIXED)
    Y.backward(_dev(i.dY))
    gr = [t.grad.cpu().numpy() for t in ins]
    aR = X.source_logits(i.X, i.wR, i.bR, H)[0].astype(np.float32) if ffn else i.aR
    ref = X.exact_layer(g, i.aL, aR, i.X, i.dY, H)
    X.check("mirror", dict(Y=Y.detach().cpu().numpy(), daL=gr[0].reshape(g.n_rows, -1)), ref, g)
    if ffn:
        w, x = i.wR.astype(np.float64), i.X.astype(np.float64)
        da, dam = np.repeat(ref.daR, F // H, 1), np.repeat(ref.daR_mass, F // H, 1)
        E.assert_bounded("mirror ffn dX", gr[1], ref.dX + da * w, ref.dX_mass + dam * np.abs(w),
                         max(X.C["dX"], X.C["daR"]), g=g, per="row", record=False)
        E.assert_bounded("mirror ffn dW", gr[2].ravel(), (da * x).sum(0), (dam * np.abs(x)).sum(0),
                         (g.n_rows + 1) * 2.0 ** -24 + X.C["daR"], record=False)
    else:
        X.check("mirror", dict(daR=gr[1].reshape(g.n_rows, -1), dX=gr[2]), ref, g)
    monkeypatch.setenv("GALA_GAT_EXACT_STATS", "0")
    with pytest.raises(RuntimeError, match="GALA_ERR_UNSUPPORTED"):
        apply(*ins, 0, X.SLOPE, FIXED)


@pytest.mark.parametrize("F,H,plan", [(1028, 1, False), (258, 1, False), (512, 64, False), (512, 8, True)])
def test_refusals(F, H, plan):
    """Past 1024 floats, rows that are no float4 vectors, more than 32 heads, a hub-row plan (of A,
    and of AT alone): refused by the three entry points with nothing written."""
    g = X.graph("long")
    dg, flat = ops.DeviceGraph.from_host(g, split=plan), ops.DeviceGraph.from_host(g, split=False)
    assert (dg.split_rows > 0) == plan
    n = g.n_rows
    aL, Xd, v = torch.zeros(n, H, device="cuda"), torch.zeros(n, F, device="cuda"), torch.zeros(n * H, device="cuda")
    out = {k: torch.full((n, F), 7.0, device="cuda") for k in ("Y", "Ym", "dX")}
    out.update({k: torch.full((n * H,), 7.0, device="cuda") for k in ("lse", "sma", "daL", "daR")})
    side, st = torch.empty(n * H * 4, device="cuda"), torch.cuda.current_stream().cuda_stream
    p, lib = (lambda t: t.data_ptr()), _abi.lib()
    bwd_args = (p(aL), p(aL), p(Xd), F, p(Xd), F, F, H, X.SLOPE, p(v), p(Xd), F, p(Xd), F, p(v), p(side),
                p(out["dX"]), F, p(out["daL"]), p(out["daR"]), st)
    ws = 2 * F + 3 * H
    assert lib.gala_gat_fwd_stats_exact_f32(dg.csr(ws), p(aL), p(aL), None, None, p(Xd), F, F, H, X.SLOPE, p(out["Y"]), F,
                                            p(out["lse"]), p(out["Ym"]), F, p(out["sma"]), None, st) == _abi.GALA_ERR_UNSUPPORTED
    assert lib.gala_gat_bwd_stats_exact_f32(dg.csr(ws), *bwd_args) == _abi.GALA_ERR_UNSUPPORTED
    assert lib.gala_gat_bwd_stats_exact_t_f32(dg.csr(ws), flat.csr(), *bwd_args) == _abi.GALA_ERR_UNSUPPORTED
    assert lib.gala_gat_bwd_stats_exact_t_f32(flat.csr(), dg.csr(ws), *bwd_args) == _abi.GALA_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in out.values())
