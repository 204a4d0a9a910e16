"""GPU: the narrow-row fused GAT kernels for head widths that are no power of two of float4
vectors (csrc/gat_headw.hip: F <= 256, D / 4 = 3, 5, 6, 7, 10 ...) behind gat_fwd_ex, gat_fwd_stats
and gat_bwd_stats.  (1) Every output bounded per element against float64 (tests/_edge_ref.py, the
constants of tests/test_gpu_edge_bounds.py), source logits given and recomputed (RC: the reference
runs on the forward's aR_out, itself bounded against the float64 Linear).  (2) The Linear-folding
backward equals the unfolded one plus d_aL * wR bit for bit, and two runs give the same bits.
(3) One 3 x 40 layer through the operator mirror.  (4) What stays refused at these widths.
Graphs without a hub-row plan; a batch is 8 edges and 64 / G rows of different lengths share a
wave (degrees asserted)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _edge_ref as er
from _edge_ref import C, FIXED, REF, SLOPE, assert_bounded, c_alpha, edge_inputs
from _graphs import edge_bound_graph as graph
import gala
from gala import _abi, ops

pytestmark = pytest.mark.gpu
# D/4 = 3 in a group of 8 (two idle lanes); 7, a prime; 25 of 32 lanes, heads not dividing G; the
# Arxiv shape (D/4 = 10, dot groups of 2); G = 64 with D/4 = 6; 63 lanes, 168 pairs per batch
SHAPES = [(24, 2), (56, 2), (100, 5), (120, 3), (192, 8), (252, 21)]
GRAPHS, CA, U = ["long", "empty"], c_alpha(None), 8


@functools.lru_cache(maxsize=None)
def setup(gname, F, heads):
    """(host inputs, device inputs, device graph without a plan); the degrees a batch of U needs."""
    g = graph(gname)
    deg = np.diff(g.rowptr.astype(np.int64))
    assert (deg == 0).any() and ((deg > 0) & (deg < U)).any() and (deg == U).any()
    assert ((deg > U) & (deg % U != 0)).any(), gname
    assert (np.ptp(deg[:deg.size // 8 * 8].reshape(-1, 8), axis=1) > 0).any()   # unequal rows in one wave
    i = edge_inputs(g, heads, F)
    d = SimpleNamespace(**{k: torch.from_numpy(getattr(i, k)).cuda() for k in ("aL", "aR", "X", "dY", "wR", "bR")})
    return i, d, ops.DeviceGraph.from_host(g, split=False)


@functools.lru_cache(maxsize=None)
def source_logits(gname, F, heads, rc):
    """(aR on the host, on the device, the forward's keywords); RC: aR_out, bounded against the float64 Linear."""
    i, d, dg = setup(gname, F, heads)
    if not rc:
        return i.aR, d.aR, dict(aR=d.aR)
    aR_dev = ops.gat_fwd_stats(dg, d.aL, d.X, wR=d.wR, bR=d.bR, heads=heads, slope=SLOPE, want_aR=True)[4]
    aR = aR_dev.cpu().numpy().reshape(-1, heads)
    t = i.X.astype(np.float64).reshape(-1, heads, F // heads) * i.wR.astype(np.float64).reshape(1, heads, -1)
    assert_bounded(f"headw_aR_{gname}_F{F}", aR, t.sum(2) + i.bR, np.abs(t).sum(2) + np.abs(i.bR), C["sddmm"],
                   per="row", g=i.R)
    return aR, aR_dev, dict(wR=d.wR, bR=d.bR)


@functools.lru_cache(maxsize=None)
def reference(gname, F, heads, rc, mode):
    i, _, _ = setup(gname, F, heads)
    return er.gat_fwd(i.R, i.aL, source_logits(gname, F, heads, rc)[0], i.X, heads, SLOPE, mode, stats=mode == REF)


@pytest.mark.parametrize("mode", [REF, FIXED])
@pytest.mark.parametrize("F,heads", SHAPES)
@pytest.mark.parametrize("gname", GRAPHS)
def test_headw_fwd_ex_recomputed(gname, F, heads, mode):
    """gat_fwd_ex with the source logits recomputed: Y alone, Y with alpha, and (REF) the factored (p, q)."""
    i, d, dg = setup(gname, F, heads)
    kw = dict(source_logits(gname, F, heads, True)[2], heads=heads, slope=SLOPE, mode=mode)
    fw = reference(gname, F, heads, True, mode)
    tag = f"{gname}_F{F}_h{heads}_m{mode}"
    Y0 = ops.gat_fwd_ex(dg, d.aL, d.X, **kw)
    assert_bounded(f"headw_Y_alone_{tag}", Y0.cpu().numpy(), fw.Y, fw.Y_mass, C["Y"], per="row", g=i.R)
    Y, al = ops.gat_fwd_ex(dg, d.aL, d.X, want_alpha=True, **kw)
    assert_bounded(f"headw_alpha_{tag}", al.cpu().numpy(), fw.alpha, fw.alpha, CA, per="edge", g=i.R)
    assert_bounded(f"headw_Y_{tag}", Y.cpu().numpy(), fw.Y, fw.Y_mass, C["Y"], per="row", g=i.R)
    if mode == REF:
        Y2, p, q = ops.gat_fwd_ex(dg, d.aL, d.X, factored=True, **kw)
        pq = p.cpu().double().view(-1, heads).numpy() * q.cpu().double().view(-1, heads).numpy()[i.R.row]
        assert_bounded(f"headw_pq_{tag}", pq, fw.alpha, fw.alpha, CA, per="edge", g=i.R)
        assert_bounded(f"headw_q_{tag}", q.cpu().numpy(), fw.q, fw.q, CA, per="row", g=i.R)
        assert_bounded(f"headw_exY_{tag}", Y2.cpu().numpy(), fw.Y, fw.Y_mass, C["Y"], per="row", g=i.R)


@pytest.mark.parametrize("rc", [False, True], ids=["aR", "rc"])
@pytest.mark.parametrize("F,heads", SHAPES)
@pytest.mark.parametrize("gname", GRAPHS)
def test_headw_stats_pair(gname, F, heads, rc):
    """gat_fwd_stats (Y, q, Ym, sma, p) and gat_bwd_stats (dX, d_aL) from aR and from p."""
    i, d, dg = setup(gname, F, heads)
    aR, aR_dev, fkw = source_logits(gname, F, heads, rc)
    fw = reference(gname, F, heads, rc, REF)
    bx = er.gat_bwd(i.R, i.aL, aR, i.X, i.dY, fw.alpha, heads, SLOPE, REF, dX=True)
    tag = f"{gname}_F{F}_h{heads}_rc{int(rc)}"
    out = ops.gat_fwd_stats(dg, d.aL, d.X, heads=heads, slope=SLOPE, want_p=True, **fkw)
    again = ops.gat_fwd_stats(dg, d.aL, d.X, heads=heads, slope=SLOPE, want_p=True, **fkw)
    assert all(torch.equal(a, b) for a, b in zip(out, again)), tag
    Y, q, Ym, sma, p = out
    assert_bounded(f"headw_stats_Y_{tag}", Y.cpu().numpy(), fw.Y, fw.Y_mass, C["Y"], per="row", g=i.R)
    assert_bounded(f"headw_stats_q_{tag}", q.cpu().numpy(), fw.q, fw.q, CA, per="row", g=i.R)
    assert_bounded(f"headw_stats_Ym_{tag}", Ym.cpu().numpy(), fw.Ym, fw.Ym_mass, C["Y"], per="row", g=i.R)
    assert_bounded(f"headw_stats_sma_{tag}", sma.cpu().numpy(), fw.sma, fw.sma, C["Y"], per="row", g=i.R)
    assert_bounded(f"headw_stats_p_{tag}", p.cpu().numpy(), fw.p, fw.p, CA, per="edge", g=i.R)
    for how, pe in (("aR", None), ("p", p)):
        bkw = dict(heads=heads, slope=SLOPE, p=pe)
        dX, daL = ops.gat_bwd_stats(dg, d.aL, aR_dev, d.dY, q, Y, Ym, sma, **bkw)
        assert_bounded(f"headw_dX_{how}_{tag}", dX.cpu().numpy(), bx.dX, bx.dX_mass, C["Y"], per="row", g=i.R)
        assert_bounded(f"headw_daL_{how}_{tag}", daL.cpu().numpy(), bx.daL, bx.daL_mass, C["daL"], per="row", g=i.R)
        dX2, daL2 = ops.gat_bwd_stats(dg, d.aL, aR_dev, d.dY, q, Y, Ym, sma, **bkw)
        assert torch.equal(dX, dX2) and torch.equal(daL, daL2), (how, tag)
        # the Linear-folding form adds fl(d_aL * wR) to that dX at the store
        dXl, _ = ops.gat_bwd_stats(dg, d.aL, aR_dev, d.dY, q, Y, Ym, sma, wR=d.wR, **bkw)
        assert torch.equal(dXl, dX + daL.view(-1, heads).repeat_interleave(F // heads, 1) * d.wR), (how, tag)


@pytest.mark.parametrize("ffn", [False, True], ids=["aR", "ffn"])
def test_headw_layer_through_the_mirror(ffn):
    """A REF layer of 3 x 40 on one pattern through gat_aggregate_apply / gat_aggregate_ffn_apply (the
    DSL's layer: its backward folds the Linear's dX term) against float64.  The ffn layer's dX is two
    terms bounded by C["Y"] >= C["daL"] times their masses; dW sums n products in fp32: (n + 1) * 2^-24
    + C["daL"] times its mass.  A FIXED layer with gradients has no HIP backward here: refused."""
    F, heads, g, E = 120, 3, graph("empty"), gala.torch_ext()
    i, d, _ = setup("empty", F, heads)
    fw = reference("empty", F, heads, ffn, REF)
    bx = er.gat_bwd(i.R, i.aL, source_logits("empty", F, heads, ffn)[0], i.X, i.dY, fw.alpha, heads, SLOPE, REF, dX=True)
    off, cols = torch.from_numpy(g.rowptr).cuda(), torch.from_numpy(g.col).cuda()
    E.slots_clear()
    for _ in range(2):
        E.slots_push(off, cols, torch.ones(g.nnz, device="cuda"), None, 1, False)
    ins = [t.clone().requires_grad_() for t in ((d.aL, d.X, d.wR, d.bR) if ffn else (d.aL, d.aR, d.X))]
    apply = E.gat_aggregate_ffn_apply if ffn else E.gat_aggregate_apply
    Y = apply(*ins, 0, SLOPE, REF)
    Y.backward(d.dY)
    assert_bounded(f"headw_mirror_Y_{ffn}", Y.detach().cpu().numpy(), fw.Y, fw.Y_mass, C["Y"], per="row", g=i.R)
    assert_bounded(f"headw_mirror_daL_{ffn}", ins[0].grad.cpu().numpy(), bx.daL, bx.daL_mass, C["daL"], per="row", g=i.R)
    if ffn:
        w, da, dam = i.wR.astype(np.float64), np.repeat(bx.daL, F // heads, 1), np.repeat(bx.daL_mass, F // heads, 1)
        assert_bounded("headw_mirror_ffn_dX", ins[1].grad.cpu().numpy(), bx.dX + da * w, bx.dX_mass + dam * np.abs(w),
                       C["Y"], per="row", g=i.R)
        x = i.X.astype(np.float64)
        assert_bounded("headw_mirror_ffn_dW", ins[2].grad.cpu().numpy(), (da * x).sum(0), (dam * np.abs(x)).sum(0),
                       (g.n_rows + 1) * 2.0 ** -24 + C["daL"])
    else:
        assert_bounded("headw_mirror_daR", ins[1].grad.cpu().numpy(), bx.daL, bx.daL_mass, C["daL"], per="row", g=i.R)
        assert_bounded("headw_mirror_dX", ins[2].grad.cpu().numpy(), bx.dX, bx.dX_mass, C["Y"], per="row", g=i.R)
    with pytest.raises(RuntimeError, match="GALA_ERR_UNSUPPORTED"):
        apply(*ins, 0, SLOPE, FIXED)


@pytest.mark.parametrize("F,heads,plan,exact", [(12, 2, False, False), (120, 3, True, False), (24, 2, False, True)])
def test_headw_refusals_remain(F, heads, plan, exact):
    """Heads of 6 floats (no float4 vectors), a hub-row plan, the exact pair."""
    g = graph("long")
    dg = ops.DeviceGraph.from_host(g) if plan else ops.DeviceGraph.from_host(g, split=False)
    assert (dg.split_rows > 0) == plan
    n = g.n_rows
    aL, X = torch.zeros(n, heads, device="cuda"), torch.zeros(n, F, device="cuda")
    v, w = torch.zeros(n * heads, device="cuda"), torch.zeros(F, device="cuda")
    calls = [lambda: ops.gat_fwd_stats_exact(dg, aL, X, aR=aL, heads=heads)] if exact else [
        lambda: ops.gat_fwd_ex(dg, aL, X, wR=w, heads=heads),
        lambda: ops.gat_fwd_stats(dg, aL, X, aR=aL, heads=heads),
        lambda: ops.gat_bwd_stats(dg, aL, aL, X, v, X, X, v, heads=heads)]
    for call in calls:
        with pytest.raises(_abi.GalaError) as e:
            call()
        assert e.value.status == _abi.GALA_ERR_UNSUPPORTED
