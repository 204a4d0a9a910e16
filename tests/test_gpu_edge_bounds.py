"""GPU: the edge-softmax, row-sum, SDDMM and GAT kernels bounded per element against float64.

Every kernel that regroups a reduction (the chunked K7 row sum, the SDDMM dot, the edge
softmax forward / backward, the fused GAT forward / backward and its factored, recomputed,
statistics and attention-recompute variants) against tests/_edge_ref.py through
assert_bounded: |got - ref| <= c * mass + floor on every element, mass the float64 sum of the
absolute terms of that element, c per quantity from the oracle's own error
(_edge_ref.C; measured by tests/test_edge_bounds_cpu.py).  Nothing is masked out.

Graphs: _graphs.long_rows_graph() (rows of exactly 1023 ... 2600 and 63 ... 129 edges: either
side of the hub threshold and of every chunk boundary of the plans below, empty and one-edge
rows, a self loop on every other row), column-tiled by 1000 where the op takes segments, and
with_empty_rows().  Hub-row plans: none, (threshold 64, 32-edge chunks, degree row order),
(64, 16) and the default (DeviceGraph.from_host: 1024, 512).  Inputs: test_edge_bounds_cpu's
edge_inputs, plain and spotlight (the logit of the edges at both ends of every chunk boundary
lifted, so that one edge missing from or doubled in a sum moves the row by 80 x the bound
with 512-edge chunks, 7 x with 32 and 3.8 x with 16; _edge_ref.spot_check asserts the minimum
spotlit weight on the float64 reference).  alpha's c is the input set's (_edge_ref.c_alpha).
GALA_TEST_RECORD=<path> appends every check's worst ratios (profiles/edge_bounds_gpu.jsonl).
"""
import functools

import numpy as np
import pytest
import torch

import _edge_ref as er
from _edge_ref import C, FIXED, REF, SLOPE, assert_bounded, c_alpha, edge_inputs, spot_check
from _graphs import edge_bound_graph as graph
from gala import _abi, ops

pytestmark = pytest.mark.gpu

assert (REF, FIXED) == (_abi.GALA_SOFTMAX_REF, _abi.GALA_SOFTMAX_FIXED)
PLANS = {"none": None, "t64c32": (64, 32, True), "t64c16": (64, 16, False), "default": "default"}
CHUNK = {"none": None, "t64c32": 32, "t64c16": 16, "default": 512}
# (graph, plan, spotlight chunk): plain inputs under every plan; the spotlight set of a plan's
# own chunk boundaries (512 for the rows no plan splits); tiled graphs take no plan
LAYOUTS = ([("long", p, None) for p in PLANS]
           + [("long", "none", 512), ("long", "default", 512), ("long", "t64c32", 32), ("long", "t64c16", 16),
              ("long_tiled", "none", None), ("long_tiled", "none", 512), ("empty", "none", None),
              ("empty", "t64c32", None)])
SQUARE = [lay for lay in LAYOUTS if lay[0] != "empty"]
ids = lambda lay: f"{lay[0]}-{lay[1]}-spot{lay[2]}"  # noqa: E731
MODES = [REF, FIXED]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def device_graph(gname, plan):
    g = graph(gname)
    if PLANS[plan] == "default":
        dg = ops.DeviceGraph.from_host(g)
        assert dg.split_rows == 7
        return dg
    dg = ops.DeviceGraph.from_host(g, split=False)
    if PLANS[plan]:
        thr, chunk, order = PLANS[plan]
        dg.set_split_plan(g.rowptr, thr, chunk=chunk, row_order=order)
        assert dg.split_rows == (15 if gname == "long" else 1)
    return dg


@functools.lru_cache(maxsize=None)
def inputs(gname, heads, F, spot):
    return edge_inputs(graph(gname), heads, F, spot)


@functools.lru_cache(maxsize=None)
def dev_inputs(gname, heads, F, spot):
    i = inputs(gname, heads, F, spot)
    return er.SimpleNamespace(**{k: dev(getattr(i, k)) for k in ("s", "d", "v_pos", "v_signed", "aL", "aR", "X", "dY",
                                                                 "wR", "bR")})


@functools.lru_cache(maxsize=None)
def ref_gat(gname, heads, F, spot, mode):
    """The float64 forward (with the statistics) and, from its alpha rounded to fp32 -- the
    array the alpha-reading backward kernels are handed -- the backward; computed once."""
    i = inputs(gname, heads, F, spot)
    fw = er.gat_fwd(i.R, i.aL, i.aR, i.X, heads, SLOPE, mode, stats=True)
    if spot:
        spot_check(i, fw.alpha, gat=True)
    fw.alpha32 = fw.alpha.astype(np.float32)
    fw.bw = er.gat_bwd(i.R, i.aL, i.aR, i.X, i.dY, fw.alpha32, heads, SLOPE, mode)
    return fw


def cases(layouts, shapes):
    """(layout, heads, F); the spotlight set runs on D = 32 per head (the float64 reference is
    the cost of a case)."""
    return [pytest.param(lay, h, F, id=f"{ids(lay)}-h{h}-F{F}") for lay in layouts for (h, F) in shapes
            if not lay[2] or (h, F) in ((1, 32), (8, 256), (3, 96))]


def case(lay, heads, F):
    gname, plan, spot = lay
    i = inputs(gname, heads, F, spot)
    kw = dict(g=i.R, chunk=CHUNK[plan])
    return i, dev_inputs(gname, heads, F, spot), device_graph(gname, plan), kw


@pytest.mark.parametrize("heads", [1, 3, 8])
@pytest.mark.parametrize("lay", [lay for lay in LAYOUTS if lay[2] is None], ids=ids)
def test_row_sum_chunked(lay, heads):
    """K7 with the plan's hub rows as chunk partials, positive and signed terms."""
    i, d, dg, kw = case(lay, heads, 32 * heads)
    for name in ("v_pos", "v_signed"):
        got = host(ops.row_sum(dg, getattr(d, name).reshape(-1), heads=heads, eps=1e-12, hub="chunked"))
        assert_bounded(f"row_sum_{name}_{ids(lay)}_h{heads}", got, *er.row_sum(i.R, getattr(i, name), heads),
                       C["row_sum"], per="row", **kw)


@pytest.mark.parametrize("heads,F", [(1, 32), (8, 256), (3, 96), (1, 47)])
@pytest.mark.parametrize("lay", [lay for lay in LAYOUTS if lay[2] is None], ids=ids)
def test_sddmm(lay, heads, F):
    i, d, dg, kw = case(lay, heads, F)
    got = host(ops.sddmm(dg, d.dY, d.X, heads=heads))
    assert_bounded(f"sddmm_{ids(lay)}_h{heads}_F{F}", got, *er.sddmm(i.R, i.dY, i.X, heads), C["sddmm"], per="edge", **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("lay,heads,F", cases(LAYOUTS, [(1, 32), (3, 96), (8, 256)]))
def test_edge_softmax(lay, heads, F, mode):
    """Forward from the logits; backward from the float64 alpha rounded to fp32.  (A head count
    that is no power of two, heads = 3, takes edge.hip's generic kernel under every plan.)"""
    i, d, dg, kw = case(lay, heads, 32 * heads)
    tag = f"{ids(lay)}_h{heads}_m{mode}"
    a_ref, a_mass = er.softmax_fwd(i.R, i.s, heads, mode)
    if lay[2]:
        spot_check(i, a_ref, gat=False)
    got = host(ops.edge_softmax(dg, d.s.reshape(-1), heads=heads, mode=mode))
    assert_bounded(f"softmax_fwd_{tag}", got, a_ref, a_mass, c_alpha(lay[2]), per="edge", **kw)
    a32 = a_ref.astype(np.float32)
    got = host(ops.edge_softmax_bwd(dg, dev(a32), d.d.reshape(-1), heads=heads, mode=mode))
    assert_bounded(f"softmax_bwd_{tag}", got, *er.softmax_bwd(i.R, a32, i.d, heads, mode), C["ds"], per="edge", **kw)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("lay,heads,F", cases(LAYOUTS, [(1, 32), (8, 256), (3, 96), (1, 47)]))
def test_gat_fwd_bwd(lay, heads, F, mode):
    """gat_fwd: alpha and Y, and Y alone.  With heads = 3 (a row group of 32 lanes: three 8-lane
    heads, 8 idle) a forward that writes alpha runs the plan's hub rows unsplit (gat.hip: the
    per-head alpha pass needs heads | row group), so only the call without alpha takes the chunk
    combine at that head count.  gat_bwd: d_aL, and dz in FIXED mode; it refuses heads that do
    not divide the row group (GALA_ERR_UNSUPPORTED), so not at heads = 3.  gat_fwd_ex factored
    (REF): p * q and q."""
    i, d, dg, kw = case(lay, heads, F)
    fw = ref_gat(lay[0], heads, F, lay[2], mode)
    tag = f"{ids(lay)}_h{heads}_F{F}_m{mode}"
    Y, al = ops.gat_fwd(dg, d.aL, d.aR, d.X, heads=heads, slope=SLOPE, mode=mode, want_alpha=True)
    assert_bounded(f"gat_alpha_{tag}", host(al), fw.alpha, fw.alpha, c_alpha(lay[2]), per="edge", **kw)
    assert_bounded(f"gat_Y_{tag}", host(Y), fw.Y, fw.Y_mass, C["Y"], per="row", **kw)
    Y0 = ops.gat_fwd(dg, d.aL, d.aR, d.X, heads=heads, slope=SLOPE, mode=mode)
    assert_bounded(f"gat_Y_alone_{tag}", host(Y0), fw.Y, fw.Y_mass, C["Y"], per="row", **kw)
    if mode == REF:
        Y2, p, q = ops.gat_fwd_ex(dg, d.aL, d.X, aR=d.aR, heads=heads, factored=True)
        pq = host(p).reshape(-1, heads).astype(np.float64) * host(q).reshape(-1, heads).astype(np.float64)[i.R.row]
        assert_bounded(f"gat_pq_{tag}", pq, fw.alpha, fw.alpha, c_alpha(lay[2]), per="edge", **kw)
        assert_bounded(f"gat_q_{tag}", host(q), fw.q, fw.q, c_alpha(lay[2]), per="row", **kw)
        assert_bounded(f"gat_exY_{tag}", host(Y2), fw.Y, fw.Y_mass, C["Y"], per="row", **kw)
    if heads == 3:
        with pytest.raises(_abi.GalaError):
            ops.gat_bwd(dg, d.aL, d.aR, d.X, d.dY, dev(fw.alpha32.ravel()), heads=heads, slope=SLOPE, mode=mode)
        return
    daL, dz = ops.gat_bwd(dg, d.aL, d.aR, d.X, d.dY, dev(fw.alpha32.ravel()), heads=heads, slope=SLOPE, mode=mode)
    assert_bounded(f"gat_daL_{tag}", host(daL), fw.bw.daL, fw.bw.daL_mass, C["daL"], per="row", **kw)
    if mode == FIXED:
        assert_bounded(f"gat_dz_{tag}", host(dz), fw.bw.dz, fw.bw.dz_mass, C["ds"], per="edge", **kw)


def check_stats_pair(tag, i, d, dg, kw, fw, aR, aR_dev, fwd_kw, heads, ca):
    """The statistics forward's Y, q, Ym, sma; the statistics backward's and the recomputing
    fused backward's dX and d_aL (from the kernels' own forward outputs)."""
    bx = er.gat_bwd(i.R, i.aL, aR, i.X, i.dY, fw.alpha, heads, SLOPE, REF, dX=True)
    Y, q, Ym, sma = ops.gat_fwd_stats(dg, d.aL, d.X, heads=heads, slope=SLOPE, **fwd_kw)[:4]
    assert_bounded(f"stats_Y_{tag}", host(Y), fw.Y, fw.Y_mass, C["Y"], per="row", **kw)
    assert_bounded(f"stats_q_{tag}", host(q), fw.q, fw.q, ca, per="row", **kw)
    assert_bounded(f"stats_Ym_{tag}", host(Ym), fw.Ym, fw.Ym_mass, C["Y"], per="row", **kw)
    assert_bounded(f"stats_sma_{tag}", host(sma), fw.sma, fw.sma, C["Y"], per="row", **kw)
    dX, daL = ops.gat_bwd_stats(dg, d.aL, aR_dev, d.dY, q, Y, Ym, sma, heads=heads, slope=SLOPE)
    assert_bounded(f"stats_dX_{tag}", host(dX), bx.dX, bx.dX_mass, C["Y"], per="row", **kw)
    assert_bounded(f"stats_daL_{tag}", host(daL), bx.daL, bx.daL_mass, C["daL"], per="row", **kw)
    kw2 = {k: v for k, v in fwd_kw.items() if k in ("aR", "wR", "bR")}
    dX, daL = ops.gat_bwd_fused(dg, d.aL, d.X, d.dY, q, heads=heads, slope=SLOPE, **kw2)
    assert_bounded(f"fused_dX_{tag}", host(dX), bx.dX, bx.dX_mass, C["Y"], per="row", **kw)
    assert_bounded(f"fused_daL_{tag}", host(daL), bx.daL, bx.daL_mass, C["daL"], per="row", **kw)


@pytest.mark.parametrize("lay,heads,F", cases(SQUARE, [(1, 32), (8, 256), (3, 96), (1, 47)]))
def test_gat_stats_pair_and_fused_backward(lay, heads, F):
    """REF, square pattern, the source logits given."""
    i, d, dg, kw = case(lay, heads, F)
    fw = ref_gat(lay[0], heads, F, lay[2], REF)
    check_stats_pair(f"{ids(lay)}_h{heads}_F{F}", i, d, dg, kw, fw, i.aR, d.aR, dict(aR=d.aR), heads,
                     c_alpha(lay[2]))


@pytest.mark.parametrize("heads,F", [(1, 32), (8, 256), (3, 96), (1, 47)])
@pytest.mark.parametrize("lay", [lay for lay in SQUARE if lay[2] is None], ids=ids)
def test_gat_stats_pair_recomputed_source_logits(lay, heads, F):
    """The same with aR recomputed from (wR, bR) inside the kernels: the reference runs on the
    forward's aR_out ("Source logits"), which is itself checked against the
    float64 per-head Linear at c * (sum |x||w| + |b|)."""
    i, d, dg, kw = case(lay, heads, F)
    aR_out = ops.gat_fwd_stats(dg, d.aL, d.X, wR=d.wR, bR=d.bR, heads=heads, slope=SLOPE, want_aR=True)[4]
    aR = host(aR_out).reshape(-1, heads)
    D = F // heads
    t = i.X.astype(np.float64).reshape(-1, heads, D) * i.wR.astype(np.float64).reshape(1, heads, D)
    assert_bounded(f"stats_aR_{ids(lay)}_h{heads}_F{F}", aR, t.sum(2) + i.bR, np.abs(t).sum(2) + np.abs(i.bR),
                   C["sddmm"], per="row", **kw)
    fw = er.gat_fwd(i.R, i.aL, aR, i.X, heads, SLOPE, REF, stats=True)
    check_stats_pair(f"rc_{ids(lay)}_h{heads}_F{F}", i, d, dg, kw, fw, aR, aR_out, dict(wR=d.wR, bR=d.bR), heads,
                     c_alpha(lay[2]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("F", [32, 47])
@pytest.mark.parametrize("lay", [lay for lay in LAYOUTS if lay[2] is None], ids=ids)
def test_gat_attention_recompute(lay, F, mode):
    """gat_fwd_attn / gat_bwd_attn (one head, aR = X wR + bR inside the kernel, no aR output):
    the reference runs on ops.head_attn's logits."""
    i, d, dg, kw = case(lay, 1, F)
    aR = host(ops.head_attn(d.X, d.wR, d.bR, heads=1))
    fw = er.gat_fwd(i.R, i.aL, aR, i.X, 1, SLOPE, mode)
    tag = f"{ids(lay)}_F{F}_m{mode}"
    Y, al = ops.gat_fwd_attn(dg, d.aL, d.wR, d.bR, d.X, slope=SLOPE, mode=mode, want_alpha=True)
    assert_bounded(f"attn_alpha_{tag}", host(al), fw.alpha, fw.alpha, c_alpha(lay[2]), per="edge", **kw)
    assert_bounded(f"attn_Y_{tag}", host(Y), fw.Y, fw.Y_mass, C["Y"], per="row", **kw)
    if mode == REF:
        a32 = fw.alpha.astype(np.float32)
        bw = er.gat_bwd(i.R, i.aL, aR, i.X, i.dY, a32, 1, SLOPE, REF)
        daL = ops.gat_bwd_attn(dg, d.aL, d.wR, d.bR, d.X, d.dY, dev(a32.ravel()), slope=SLOPE)
        assert_bounded(f"attn_daL_{tag}", host(daL), bw.daL, bw.daL_mass, C["daL"], per="row", **kw)
