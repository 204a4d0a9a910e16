"""GPU: the wide-row fused GAT kernels (csrc/gat_wide.hip: 256 < F <= 1024) behind gat_fwd_ex,
gat_fwd_stats and gat_bwd_stats.  (1) Every output bounded per element against float64
(tests/_edge_ref.py, the constants of tests/test_gpu_edge_bounds.py), source logits given and
recomputed (RC: the reference runs on the forward's aR_out, itself bounded against the float64
Linear).  (2) REF with given logits: bit for bit the narrow kernels on every 256-float column block
of whole heads.  (3) Shapes outside the served range still raise GALA_ERR_UNSUPPORTED.
Graphs without a hub-row plan; a batch is 8 edges at two slices and 4 beyond (degrees asserted)."""
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
SHAPES = [(512, 8), (320, 5), (768, 2), (1024, 32), (260, 1)]
GRAPHS, CA = ["long", "empty"], c_alpha(None)


@functools.lru_cache(maxsize=None)
def setup(gname, F, heads):
    """(host inputs, device inputs, device graph without a plan); the degrees the batches need."""
    g = graph(gname)
    deg = np.diff(g.rowptr.astype(np.int64))
    assert (deg == 0).any()
    for U in (4, 8):
        assert ((deg > 0) & (deg < U)).any() and (deg == U).any() and ((deg > U) & (deg % U != 0)).any(), (gname, U)
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
    assert_bounded(f"wide_aR_{gname}_F{F}", aR, t.sum(2) + i.bR, np.abs(t).sum(2) + np.abs(i.bR), C["sddmm"],
                   per="row", g=i.R)
    return aR, aR_dev, dict(wR=d.wR, bR=d.bR)


@functools.lru_cache(maxsize=None)
def reference(gname, F, heads, rc, mode):
    i, _, _ = setup(gname, F, heads)
    return er.gat_fwd(i.R, i.aL, source_logits(gname, F, heads, rc)[0], i.X, heads, SLOPE, mode, stats=mode == REF)


@pytest.mark.parametrize("mode", [REF, FIXED])
@pytest.mark.parametrize("rc", [False, True], ids=["aR", "rc"])
@pytest.mark.parametrize("F,heads", SHAPES)
@pytest.mark.parametrize("gname", GRAPHS)
def test_wide_fwd_ex(gname, F, heads, rc, mode):
    """gat_fwd_ex: Y alone, Y with alpha, and (REF) the factored (p, q)."""
    i, d, dg = setup(gname, F, heads)
    kw = dict(source_logits(gname, F, heads, rc)[2], heads=heads, slope=SLOPE, mode=mode)
    fw = reference(gname, F, heads, rc, mode)
    tag = f"{gname}_F{F}_h{heads}_rc{int(rc)}_m{mode}"
    Y0 = ops.gat_fwd_ex(dg, d.aL, d.X, **kw)
    assert_bounded(f"wide_Y_alone_{tag}", Y0.cpu().numpy(), fw.Y, fw.Y_mass, C["Y"], per="row", g=i.R)
    Y, al = ops.gat_fwd_ex(dg, d.aL, d.X, want_alpha=True, **kw)
    assert_bounded(f"wide_alpha_{tag}", al.cpu().numpy(), fw.alpha, fw.alpha, CA, per="edge", g=i.R)
    assert_bounded(f"wide_Y_{tag}", Y.cpu().numpy(), fw.Y, fw.Y_mass, C["Y"], per="row", g=i.R)
    if mode == REF:
        Y2, p, q = ops.gat_fwd_ex(dg, d.aL, d.X, factored=True, **kw)
        pq = p.cpu().double().view(-1, heads).numpy() * q.cpu().double().view(-1, heads).numpy()[i.R.row]
        assert_bounded(f"wide_pq_{tag}", pq, fw.alpha, fw.alpha, CA, per="edge", g=i.R)
        assert_bounded(f"wide_q_{tag}", q.cpu().numpy(), fw.q, fw.q, CA, per="row", g=i.R)
        assert_bounded(f"wide_exY_{tag}", Y2.cpu().numpy(), fw.Y, fw.Y_mass, C["Y"], per="row", g=i.R)


@pytest.mark.parametrize("rc", [False, True], ids=["aR", "rc"])
@pytest.mark.parametrize("F,heads", SHAPES)
@pytest.mark.parametrize("gname", GRAPHS)
def test_wide_stats_pair(gname, F, heads, rc):
    """gat_fwd_stats (Y, q, Ym, sma, p) and gat_bwd_stats (dX, d_aL) from aR and from p."""
    i, d, dg = setup(gname, F, heads)
    aR, aR_dev, fkw = source_logits(gname, F, heads, rc)
    fw = reference(gname, F, heads, rc, REF)
    bx = er.gat_bwd(i.R, i.aL, aR, i.X, i.dY, fw.alpha, heads, SLOPE, REF, dX=True)
    tag = f"{gname}_F{F}_h{heads}_rc{int(rc)}"
    Y, q, Ym, sma, p = ops.gat_fwd_stats(dg, d.aL, d.X, heads=heads, slope=SLOPE, want_p=True, **fkw)
    assert_bounded(f"wide_stats_Y_{tag}", Y.cpu().numpy(), fw.Y, fw.Y_mass, C["Y"], per="row", g=i.R)
    assert_bounded(f"wide_stats_q_{tag}", q.cpu().numpy(), fw.q, fw.q, CA, per="row", g=i.R)
    assert_bounded(f"wide_stats_Ym_{tag}", Ym.cpu().numpy(), fw.Ym, fw.Ym_mass, C["Y"], per="row", g=i.R)
    assert_bounded(f"wide_stats_sma_{tag}", sma.cpu().numpy(), fw.sma, fw.sma, C["Y"], per="row", g=i.R)
    assert_bounded(f"wide_stats_p_{tag}", p.cpu().numpy(), fw.p, fw.p, CA, per="edge", g=i.R)
    for how, pe in (("aR", None), ("p", p)):
        dX, daL = ops.gat_bwd_stats(dg, d.aL, aR_dev, d.dY, q, Y, Ym, sma, heads=heads, slope=SLOPE, p=pe)
        assert_bounded(f"wide_dX_{how}_{tag}", dX.cpu().numpy(), bx.dX, bx.dX_mass, C["Y"], per="row", g=i.R)
        assert_bounded(f"wide_daL_{how}_{tag}", daL.cpu().numpy(), bx.daL, bx.daL_mass, C["daL"], per="row", g=i.R)
        # the Linear-folding form adds fl(d_aL * wR) to that dX at the store
        dXl, _ = ops.gat_bwd_stats(dg, d.aL, aR_dev, d.dY, q, Y, Ym, sma, heads=heads, slope=SLOPE, p=pe, wR=d.wR)
        assert torch.equal(dXl, dX + daL.view(-1, heads).repeat_interleave(F // heads, 1) * d.wR), (how, tag)


@pytest.mark.parametrize("F,heads", [(512, 8), (1024, 32)])
def test_wide_equals_narrow_on_column_blocks(F, heads):
    """REF, aR given: per head the wide kernels form the narrow kernels' CSR-order fmaf chains,
    so each 256-float block equals the narrow kernels run on that block's strided view."""
    _, d, dg = setup("long", F, heads)
    n, hb = dg.n_rows, 256 * heads // F
    Y, q, Ym, sma = ops.gat_fwd_stats(dg, d.aL, d.X, aR=d.aR, heads=heads, slope=SLOPE)
    dX, _ = ops.gat_bwd_stats(dg, d.aL, d.aR, d.dY, q, Y, Ym, sma, heads=heads, slope=SLOPE)
    assert torch.equal(ops.gat_fwd_ex(dg, d.aL, d.X, aR=d.aR, heads=heads, slope=SLOPE), Y)
    for b in range(F // 256):
        cols, hs = slice(256 * b, 256 * (b + 1)), slice(hb * b, hb * (b + 1))
        aLb, aRb = d.aL[:, hs].contiguous(), d.aR[:, hs].contiguous()
        Yn, qn, Ymn, sman = ops.gat_fwd_stats(dg, aLb, d.X[:, cols], aR=aRb, heads=hb, slope=SLOPE)
        dXn, _ = ops.gat_bwd_stats(dg, aLb, aRb, d.dY[:, cols], qn, Yn, Ymn, sman, heads=hb, slope=SLOPE)
        assert torch.equal(Y[:, cols], Yn) and torch.equal(Ym[:, cols], Ymn), b
        assert torch.equal(q.view(n, heads)[:, hs], qn.view(n, hb)), b
        assert torch.equal(sma.view(n, heads)[:, hs], sman.view(n, hb)), b
        assert torch.equal(dX[:, cols], dXn), b


@pytest.mark.parametrize("ffn", [False, True], ids=["aR", "ffn"])
def test_wide_layer_through_the_mirror(ffn):
    """A REF layer of 8 x 64 on one pattern through gat_aggregate_apply / gat_aggregate_ffn_apply (the
    DSL's layer: its backward folds the Linear's dX term) against float64.  The ffn layer's dX is two
    terms bounded by C["Y"] >= C["daL"] times their masses; dW sums n products in fp32: (n + 1) * 2^-24
    + C["daL"] times its mass.  A FIXED layer with gradients has no HIP backward here: refused."""
    F, heads, g, E = 512, 8, graph("empty"), gala.torch_ext()
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
    assert_bounded(f"mirror_Y_{ffn}", Y.detach().cpu().numpy(), fw.Y, fw.Y_mass, C["Y"], per="row", g=i.R)
    assert_bounded(f"mirror_daL_{ffn}", ins[0].grad.cpu().numpy(), bx.daL, bx.daL_mass, C["daL"], per="row", g=i.R)
    if ffn:
        w, da, dam = i.wR.astype(np.float64), np.repeat(bx.daL, F // heads, 1), np.repeat(bx.daL_mass, F // heads, 1)
        assert_bounded("mirror_ffn_dX", ins[1].grad.cpu().numpy(), bx.dX + da * w, bx.dX_mass + dam * np.abs(w), C["Y"],
                       per="row", g=i.R)
        x = i.X.astype(np.float64)
        assert_bounded("mirror_ffn_dW", ins[2].grad.cpu().numpy(), (da * x).sum(0), (dam * np.abs(x)).sum(0),
                       (g.n_rows + 1) * 2.0 ** -24 + C["daL"])
    else:
        assert_bounded("mirror_daR", ins[1].grad.cpu().numpy(), bx.daL, bx.daL_mass, C["daL"], per="row", g=i.R)
        assert_bounded("mirror_dX", ins[2].grad.cpu().numpy(), bx.dX, bx.dX_mass, C["Y"], per="row", g=i.R)
    with pytest.raises(RuntimeError, match="GALA_ERR_UNSUPPORTED"):
        apply(*ins, 0, SLOPE, FIXED)


@pytest.mark.parametrize("F,heads,plan", [(1028, 1, False), (258, 1, False), (512, 64, False), (512, 8, True)])
def test_refusals_unchanged(F, heads, plan):
    """Past 1024 floats, rows that are no float4 vectors, more than 32 heads, a hub-row plan."""
    g = graph("long")
    dg = ops.DeviceGraph.from_host(g) if plan else ops.DeviceGraph.from_host(g, split=False)
    assert (dg.split_rows > 0) == plan
    n = g.n_rows
    aL, X = torch.zeros(n, heads, device="cuda"), torch.zeros(n, F, device="cuda")
    v = torch.zeros(n * heads, device="cuda")
    calls = [lambda: ops.gat_fwd_ex(dg, aL, X, aR=aL, heads=heads),
             lambda: ops.gat_fwd_stats(dg, aL, X, aR=aL, heads=heads),
             lambda: ops.gat_bwd_stats(dg, aL, aL, X, v, X, X, v, heads=heads)]
    for call in calls:
        with pytest.raises(_abi.GalaError) as e:
            call()
        assert e.value.status == _abi.GALA_ERR_UNSUPPORTED
