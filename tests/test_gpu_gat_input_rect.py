"""GPU: the input-space GAT kernels (csrc/gat_input.hip) over a row partition with a halo.

The ranks of tests/_gat_rect.py's partitions run one after another on one GPU through the
rectangular entry points (gala_gat_in_{fwd,fwd_t,q,bwd}_rect_f32), q of the halo rows copied
between the ranks' tables with gala_gat_in_q_{gather,scatter}_f32.  The walk's row outputs are
bit-identical to the square kernels on the whole graph and within tests/test_gpu_gat_input_hub.py's
tolerances of the rectangular host twins; T mode (q pass, q copy, the T-mode forward,
gala_gat_in_bwd_t_f32) is bit-identical to the rectangular walk on every output, M included; one
rank at row_base 0 is the square entry points bit for bit; hub rows keep the whole graph's
chunks; gala.dist.HaloGatInput on one rank equals ops.gat_input_layer(tmode=True).
"""
import numpy as np
import pytest
import torch

from gala import dist as gdist
from gala import ops
from gala.backend import HipBackend
from _gat_rect import (PARTITION_IDS, PARTITIONS, check_grads_against_ref, check_partitions, compose_grads,
                       cpu_rect_layer, halo_lists, make_parts, sum_parts)
from _graphs import check_phase_graph, phase_graph
from _hub_graphs import HUB_SYM_PLAN_SIZES, PLANS, check_hub_sym_graph, hub_sym_graph
from test_gat_input_cpu import grad_close, layer_inputs, ref_on_own_logits
from test_gpu_gat_input import dev
from test_gpu_gat_input_hub import planned

pytestmark = pytest.mark.gpu
SHAPES = [(100, 8, 32), (37, 4, 16)]
ROW_KEYS = ("Y", "Ym", "q", "sma", "daL")
_CACHE = {}


def graphs():
    if not _CACHE:
        g = phase_graph(True)
        check_phase_graph(g, True)
        h = hub_sym_graph()
        check_hub_sym_graph(h)
        check_partitions(g)
        check_partitions(h)
        _CACHE.update(phase=g, hub=h)
    return _CACHE


def inputs(name, shape):
    fin, heads, D = shape
    return layer_inputs(graphs()[name].n_rows, fin, heads, D, seed=fin + heads)


def square(name, plan, shape, relu, tmode=False):
    """The square kernels on the whole graph (identity order), once per case."""
    key = ("sq", name, plan, shape, relu, tmode)
    if key not in _CACHE:
        g = graphs()[name]
        X, W, b, wL, bL, wR, bR, dY = inputs(name, shape)
        out = ops.gat_input_layer(planned(g, plan), dev(X), dev(W), dev(b), dev(wL), dev(bL), dev(wR), dev(bR),
                                  shape[1], dY=dev(dY), relu=relu, tmode=tmode)
        torch.cuda.synchronize()
        _CACHE[key] = {k: v.cpu().numpy() for k, v in out.items() if v is not None and k != "T"}
    return _CACHE[key]


def gpu_copy_q(parts, xexts, heads):
    for dst, src, drows, srows in halo_lists(parts):
        buf = ops.gat_in_q_gather(xexts[src], dev(srows), heads)
        ops.gat_in_q_scatter(xexts[dst], buf, heads, rows=dev(drows))


def gpu_rect_layer(g, bounds, plan, X, W, b, wL, bL, wR, bR, dY, heads, relu=False, tmode=False, slope=0.2):
    """_gat_rect.cpu_rect_layer on the kernels: walk (forward, q copy, backward) or T mode (q
    pass, q copy, T-mode forward, gala_gat_in_bwd_t_f32)."""
    parts = make_parts(g, bounds)
    fin = X.shape[1]
    Wd, bd = dev(W), dev(b)
    u, c = ops.gat_in_compose(Wd, bd, dev(wL), dev(bL), dev(wR), dev(bR), heads)
    dgs = [planned(p.graph, plan) for p in parts]
    xexts = [ops.gat_in_prep(dev(X[p.xs_to_global()]), u, c, heads) if p.n_cols else
             torch.empty(0, 128, device="cuda") for p in parts]
    Ts = [torch.empty(p.n, 896, device="cuda") if tmode else None for p in parts]
    if tmode:
        for p, dg, xe in zip(parts, dgs, xexts):
            ops.gat_in_q(dg, xe, heads, slope, row_base=p.lo)
        gpu_copy_q(parts, xexts, heads)
    fw = [ops.gat_in_fwd(dg, xe, Wd, bd, heads, fin, slope, relu=relu, T=T, row_base=p.lo)
          for p, dg, xe, T in zip(parts, dgs, xexts, Ts)]
    if not tmode:
        gpu_copy_q(parts, xexts, heads)
    outs, Ms, Gws, Gbs = [], [], [], []
    for p, dg, xe, T, (Y, Ym, q, sma) in zip(parts, dgs, xexts, Ts, fw):
        dy = dev(dY[p.r0:p.r0 + p.n])
        daL, M = ops.gat_in_bwd(dg, xe, dy, Y, Ym, sma, heads, fin, slope, relu=relu, T=T,
                                row_base=None if tmode else p.lo)
        if p.n:
            Gw, Gb = ops.dense_grad(dev(X[p.r0:p.r0 + p.n]), daL)
        else:
            Gw, Gb = torch.zeros(heads, fin, device="cuda"), torch.zeros(heads, device="cuda")
        torch.cuda.synchronize()
        outs.append({k: v.cpu().numpy() for k, v in dict(Y=Y, Ym=Ym, q=q, sma=sma, daL=daL).items()})
        Ms.append(M.cpu().numpy())
        Gws.append(Gw.cpu().numpy())
        Gbs.append(Gb.cpu().numpy())
    res = {k: np.concatenate([o[k] for o in outs]) for k in ROW_KEYS}
    res.update(compose_grads(sum_parts(Ms), sum_parts(Gws), sum_parts(Gbs), W, b, wL, wR, heads))
    res["M_parts"], res["parts"] = Ms, parts
    res["hubs"] = sum(dg.split_rows for dg in dgs)
    return res


@pytest.mark.parametrize("world,bounds", PARTITIONS[1:], ids=PARTITION_IDS[1:])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_partitioned_walk_and_t_mode(shape, relu, world, bounds):
    g = graphs()["phase"]
    inp = inputs("phase", shape)
    heads = shape[1]
    walk = gpu_rect_layer(g, bounds, None, *inp, heads, relu=relu)
    sq = square("phase", None, shape, relu)
    for k in ROW_KEYS:
        assert np.array_equal(walk[k], sq[k]), k
    host = cpu_rect_layer(g, bounds, None, *inp, heads, relu=relu)
    np.testing.assert_allclose(walk["Y"], host["Y"], atol=2e-6, rtol=2e-6)
    np.testing.assert_allclose(walk["daL"], host["daL"], atol=2e-6, rtol=2e-6)
    np.testing.assert_allclose(walk["dW"], host["dW"], atol=1e-5 * np.abs(host["dW"]).max())
    ref = ref_on_own_logits(g, dict(sq, Y=walk["Y"]), *inp, heads, relu=relu)
    check_grads_against_ref(walk, ref, inp[0], heads)
    tm = gpu_rect_layer(g, bounds, None, *inp, heads, relu=relu, tmode=True)
    for k in ROW_KEYS + ("M", "Gw", "Gb", "dW", "db", "dwL", "dbL"):
        assert np.array_equal(tm[k], walk[k]), k
    for a, c in zip(tm["M_parts"], walk["M_parts"]):
        assert np.array_equal(a, c)


@pytest.mark.parametrize("tmode", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_rank_at_row_base_zero_is_the_square_entry_points(shape, tmode):
    g = graphs()["phase"]
    world, bounds = PARTITIONS[0]
    got = gpu_rect_layer(g, bounds, None, *inputs("phase", shape), shape[1], relu=True, tmode=tmode)
    assert world == 1 and got["parts"][0].lo == 0
    sq = square("phase", None, shape, True, tmode)
    for k in ROW_KEYS + ("M",):
        assert np.array_equal(got[k], sq[k]), k


@pytest.mark.parametrize("world,bounds", PARTITIONS[1:3], ids=PARTITION_IDS[1:3])
@pytest.mark.parametrize("tmode", [False, True])
@pytest.mark.parametrize("plan", PLANS)
def test_partitioned_hub_rows(plan, tmode, world, bounds):
    """hub_sym_graph under (64, 64) and the default plan: the ranks' hub rows are the whole
    graph's, their sums the square kernels' under the same plan; rows at or below the threshold
    are bit-identical to a run without a plan."""
    g = graphs()["hub"]
    shape = SHAPES[0]
    inp = inputs("hub", shape)
    got = gpu_rect_layer(g, bounds, plan, *inp, shape[1], relu=True, tmode=tmode)
    assert got["hubs"] == HUB_SYM_PLAN_SIZES[plan][0]
    sq = square("hub", plan, shape, True, tmode)
    for k in ROW_KEYS:
        assert np.array_equal(got[k], sq[k]), k
    base = gpu_rect_layer(g, bounds, None, *inp, shape[1], relu=True, tmode=tmode)
    rows = np.diff(g.rowptr) <= plan[0]
    for k in ("Y", "Ym", "q", "sma"):
        assert np.array_equal(got[k][rows], base[k][rows]), k
    ref = ref_on_own_logits(g, dict(sq, Y=got["Y"]), *inp, shape[1], relu=True)
    for k in ("dW", "db", "dwL", "dbL"):
        grad_close(got[k], ref[k], k)


def test_q_gather_and_scatter_round_trip():
    gen = torch.Generator(device="cuda").manual_seed(5)
    H = 5
    xe = torch.rand((1000, 128), device="cuda", generator=gen)
    keep = xe.clone()
    rows = torch.arange(997, 0, -7, dtype=torch.int32, device="cuda")      # a strided list, descending
    slots = torch.tensor([116 + 4 * (h // 3) + h % 3 for h in range(H)], device="cuda")
    q = ops.gat_in_q_gather(xe, rows, H)
    assert torch.equal(q, keep[rows.long()][:, slots])
    other = torch.zeros_like(xe)
    ops.gat_in_q_scatter(other, q, H, rows=rows)
    want = torch.zeros_like(xe)
    want[rows.long().unsqueeze(1), slots.unsqueeze(0)] = q
    assert torch.equal(other, want) and torch.equal(ops.gat_in_q_gather(other, rows, H), q)
    ops.gat_in_q_scatter(other, q, H, row0=3)                                # a contiguous block
    want[torch.arange(3, 3 + len(rows), device="cuda").unsqueeze(1), slots.unsqueeze(0)] = q
    assert torch.equal(other, want) and torch.equal(xe, keep)


@pytest.mark.parametrize("name", ["phase", "hub"])
def test_halo_gat_input_on_one_rank_equals_the_layer(name):
    """gala.dist.HaloGatInput on HipBackend with comm None (world 1) against
    ops.gat_input_layer(tmode=True) on the same graph: every output bit for bit."""
    g = graphs()[name]
    shape = SHAPES[0]
    heads = shape[1]
    X, W, b, wL, bL, wR, bR, dY = (dev(a) for a in inputs(name, shape))
    want = ops.gat_input_layer(ops.DeviceGraph.from_host(g), X, W, b, wL, bL, wR, bR, heads, dY=dY, relu=True,
                               tmode=True)
    part = gdist.partition_graph(g, 0, 1, halo_mode="p2p")
    layer = gdist.HaloGatInput(part, X, heads, HipBackend("cuda"))
    assert layer.tmode and layer.halo_bytes() == 0
    Y = layer.forward_train(None, W, b, wL, bL, wR, bR, relu=True)
    daL, M, (Gw, Gb) = layer.backward(dY)
    grads = ops.gat_in_param_grads(M, Gw, Gb, W, b, wL, wR, heads)
    torch.cuda.synchronize()
    assert torch.equal(Y, want["Y"]) and torch.equal(daL, want["daL"]) and torch.equal(M, want["M"])
    for k in ("Ym", "q", "sma"):
        assert torch.equal(layer.saved[("Y", "Ym", "q", "sma").index(k)], want[k]), k
    for k in ("dW", "db", "dwL", "dbL", "dwR", "dbR"):
        assert torch.equal(grads[k], want[k]), k
    assert torch.equal(layer.forward(None, W, b, wL, bL, wR, bR, relu=True), want["Y"])
