"""GPU: the input-space GAT layer (csrc/gat_input.hip) on graphs whose split plan has hub rows.

Hub rows are summed by the pre-pass k_gat_in_chunks (one wave per chunk) and combined in chunk
order by the persistent kernels; T mode's q of a hub row is the sum of per-chunk sums.  Against
the oracle's pass-by-pass REF layer at tests/test_gpu_gat_input.py's tolerances and against the
host twins (tests/test_gat_input_hub_cpu.py), on _graphs.long_rows_graph (directed; forward
and, transposed, backward), on _hub_graphs.hub_sym_graph (symmetric, 8205 rows: every kind of
hand-off between hub, ordinary and empty rows, walk and T mode, two row orders) and on
test_gpu_hub_rows.hub_graph (one 20 000-edge row), under the plans (threshold 64, chunk 64)
and the default (1024, 512); and the mirror's op, whose own plan has hub rows on these graphs.
"""
import numpy as np
import pytest
import torch

from gala import _abi, layout, ops
from _hub_graphs import HUB_SYM_PLAN_SIZES, PLANS, check_hub_sym_graph, hub_sym_graph
from test_gat_input_cpu import grad_close, layer_inputs, ref_on_own_logits
from test_gat_input_hub_cpu import cpu_layer_plan, long_graphs
from test_gpu_gat_input import check_against_ref, dev, mirror_op_against_the_chain

pytestmark = pytest.mark.gpu
_SYM = {}


def sym_graph():
    if not _SYM:
        g = hub_sym_graph()
        check_hub_sym_graph(g)
        _SYM["g"] = g
    return _SYM["g"]


def planned(g, plan):
    """g on the device with the hub-row plan (threshold, chunk), or none."""
    dg = ops.DeviceGraph.from_host(g, split=False)
    if plan is not None:
        dg.set_split_plan(g.rowptr, plan[0], chunk=plan[1])
    return dg


def gpu_layer(g, X, W, b, wL, bL, wR, bR, dY, heads, gT=None, relu=False, order=None, tmode=False, plan=None):
    """test_gpu_gat_input.gpu_layer with a plan on g and on gT; also returns T and the plans' hub rows."""
    dg = planned(g, plan)
    dgT = None if gT is None else planned(gT, plan)
    od = None if order is None else dev(order)
    out = ops.gat_input_layer(dg, dev(X), dev(W), dev(b), dev(wL), dev(bL), dev(wR), dev(bR), heads,
                              dY=dev(dY), gT=dgT, relu=relu, order=od, order_t=od, tmode=tmode)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
    res["hubs"] = (dg.split_rows, 0 if dgT is None else dgT.split_rows)
    return res


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("fin,heads,D", [(100, 8, 32), (37, 4, 16), (100, 3, 4)])
@pytest.mark.parametrize("plan", PLANS)
def test_walk_over_hub_rows(plan, fin, heads, D, relu, transposed):
    """Forward over long_rows_graph's hub rows; transposed: the layer on the transposed graph,
    whose backward walks them (gT = long_rows_graph carrying the plan)."""
    g, gT = long_graphs()
    if transposed:
        g, gT = gT, g
    inp = layer_inputs(g.n_rows, fin, heads, D, seed=fin + heads)
    got = gpu_layer(g, *inp, heads, gT=gT, relu=relu, plan=plan)
    assert got["hubs"][1 if transposed else 0] == (15 if plan[0] == 64 else 7)
    ref = ref_on_own_logits(g, got, *inp, heads, relu=relu)
    check_against_ref(got, ref)
    host = cpu_layer_plan(g, gT, plan, *inp, heads, relu=relu)
    np.testing.assert_allclose(got["Y"], host["Y"], atol=2e-6, rtol=2e-6)
    np.testing.assert_allclose(got["daL"], host["daL"], atol=2e-6, rtol=2e-6)
    np.testing.assert_allclose(got["dW"], host["dW"], atol=1e-5 * np.abs(host["dW"]).max())
    base = gpu_layer(g, *inp, heads, gT=gT, relu=relu)
    rows = np.diff(g.rowptr) <= plan[0]
    for k in ("Y", "Ym", "q", "sma"):
        assert np.array_equal(got[k][rows], base[k][rows]), k


@pytest.mark.parametrize("plan", PLANS)
def test_symmetric_graph_walk_and_t_mode(plan):
    """Every hand-off kind (hub_sym_graph), walk and T mode, identity and degree order: each
    against the oracle; Y, q, sma bit-identical between the orders, and T mode bit-identical
    to the walk on every output."""
    g = sym_graph()
    fin, heads, D = 100, 8, 32
    inp = layer_inputs(g.n_rows, fin, heads, D, seed=41)
    runs = {}
    for tm in (False, True):
        for name, order in (("id", None), ("deg", ops.degree_order(g.rowptr))):
            got = gpu_layer(g, *inp, heads, relu=True, order=order, tmode=tm, plan=plan)
            assert got["hubs"][0] == HUB_SYM_PLAN_SIZES[plan][0]
            check_against_ref(got, ref_on_own_logits(g, got, *inp, heads, relu=True))
            runs[tm, name] = got
    for tm in (False, True):
        for k in ("Y", "q", "sma"):
            assert np.array_equal(runs[tm, "id"][k], runs[tm, "deg"][k]), (tm, k)
    for name in ("id", "deg"):
        for k in ("Y", "Ym", "q", "sma", "daL", "M", "dW", "db", "dwL", "dbL"):
            assert np.array_equal(runs[False, name][k], runs[True, name][k]), (name, k)


@pytest.mark.parametrize("tmode", [False, True])
@pytest.mark.parametrize("plan", PLANS)
def test_spotlight_gradient_on_hub_columns(plan, tmode):
    """dY zero except on the hub rows: M and dW are the hub columns' aggregates alone, so a lost
    chunk cannot hide under 1e-4 of another column's entries."""
    g = sym_graph()
    fin, heads, D = 100, 8, 32
    X, W, b, wL, bL, wR, bR, dY = layer_inputs(g.n_rows, fin, heads, D, seed=43)
    dY[np.diff(g.rowptr) <= plan[0]] = 0
    got = gpu_layer(g, X, W, b, wL, bL, wR, bR, dY, heads, tmode=tmode, plan=plan)
    ref = ref_on_own_logits(g, got, X, W, b, wL, bL, wR, bR, dY, heads)
    check_against_ref(got, ref)
    for k in ("dW", "db"):
        grad_close(got[k], ref[k], k)


def test_one_long_row():
    """A 20 000-edge row (40 chunks of 512) under the default plan: forward, and the backward
    over it on the transposed graph."""
    from test_gpu_hub_rows import hub_graph
    g = hub_graph()
    gT, _ = layout.transpose(g)
    assert np.diff(g.rowptr).max() >= 20000
    for a, aT in ((g, gT), (gT, g)):
        inp = layer_inputs(a.n_rows, 100, 8, 32, seed=47)
        got = gpu_layer(a, *inp, 8, gT=aT, relu=True, plan=(1024, 512))
        assert max(got["hubs"]) >= 2
        check_against_ref(got, ref_on_own_logits(a, got, *inp, 8, relu=True))


@pytest.mark.parametrize("tmode", [False, True])
def test_two_calls_are_bit_identical(tmode):
    g = sym_graph()
    inp = layer_inputs(g.n_rows, 100, 8, 32, seed=53)
    a = gpu_layer(g, *inp, 8, relu=True, tmode=tmode, plan=(64, 64))
    b = gpu_layer(g, *inp, 8, relu=True, tmode=tmode, plan=(64, 64))
    for k in ("Y", "Ym", "q", "sma", "daL", "M") + (("T",) if tmode else ()):
        assert np.array_equal(a[k], b[k]), k


@pytest.fixture(scope="module")
def E():
    import gala
    return gala.torch_ext()


@pytest.mark.parametrize("symmetric", [True, False])
def test_mirror_op_on_graphs_with_hub_rows(E, symmetric):
    """gat_input_layer_apply where the mirror's own plan (threshold 1024, 512-edge chunks) has
    hub rows: the symmetric graph (T mode) and long_rows_graph (directed: the backward walks
    the transposed pattern with a plan of its own)."""
    g = sym_graph() if symmetric else long_graphs()[0]
    assert np.diff(g.rowptr).max() > layout.split_threshold(g.n_rows, g.nnz) == 1024
    mirror_op_against_the_chain(E, g, pin_relu_mask=True)
    E.slots_clear()


def test_chunk_not_a_multiple_of_64_is_refused():
    g, _ = long_graphs()
    X, W, b, wL, bL, wR, bR, dY = layer_inputs(g.n_rows, 100, 8, 32, seed=1)
    dg = planned(g, (64, 32))
    assert dg.split_rows == 15
    xext = torch.zeros(g.n_rows, 128, device="cuda")
    with pytest.raises(_abi.GalaError):
        ops.gat_in_fwd(dg, xext, dev(W), dev(b), 8, 100)
