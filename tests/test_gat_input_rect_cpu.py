"""CPU: the input-space GAT layer over a row partition with a halo, on the host twins.

The rectangular forms (gala_cpu_gat_in_{fwd,bwd}_rect_f32: a rank's rows over its table [lower
halo | own rows | higher halo], row r's own extended row at row_base + r) run rank after rank in
one process (tests/_gat_rect.py), q of the halo rows copied between the tables with the q pack /
unpack twins.  Every row keeps the whole graph's CSR order and hub chunks, so the concatenated
row outputs are BIT-identical to the square twin on the whole graph; the ranks' partials of M
and G, summed and composed into the six parameter gradients, meet the criteria of
tests/test_gat_input_cpu.py and tests/test_gat_input_phases_cpu.py against the oracle's
pass-by-pass REF layer.  tests/test_gpu_gat_input_rect.py runs the gfx950 kernels the same way.
"""
import numpy as np
import pytest

import oracle as orc  # noqa: F401  (the oracle's path, as the helpers below need it)
from gala import _abi
from _gat_rect import PARTITION_IDS, PARTITIONS, check_partitions, cpu_rect_layer, check_grads_against_ref, make_parts
from _graphs import check_phase_graph, phase_graph
from _hub_graphs import HUB_SYM_PLAN_SIZES, PLANS, PlannedCsr, check_hub_sym_graph, hub_sym_graph
from test_cpu_backend import P, HostCsr
from test_gat_input_cpu import TOL, layer_inputs, ref_on_own_logits
from test_gat_input_hub_cpu import cpu_layer_plan
from test_gat_input_phases_cpu import PHASE_SHAPES_CPU

ROW_KEYS = ("Y", "Ym", "q", "sma", "daL")
_CACHE = {}


def graphs():
    if not _CACHE:
        g = phase_graph(True)
        check_phase_graph(g, True)
        h = hub_sym_graph()
        check_hub_sym_graph(h)
        _CACHE.update(phase=g, hub=h)
    return _CACHE


def whole(name, plan, shape, relu):
    """The square twin on the whole graph and the oracle's layer on its logits, once per case."""
    key = (name, plan, shape, relu)
    if key not in _CACHE:
        g = graphs()[name]
        fin, heads, D = shape
        inp = layer_inputs(g.n_rows, fin, heads, D, seed=fin + heads)
        sq = cpu_layer_plan(g, g, plan, *inp, heads, relu=relu)
        ref = ref_on_own_logits(g, sq, *inp, heads, relu=relu)
        _CACHE[key] = (inp, sq, ref)
    return _CACHE[key]


def test_partitions_have_the_shapes_under_test():
    for g in (graphs()["phase"], graphs()["hub"]):
        check_partitions(g)


def check_partitioned(name, plan, shape, relu, bounds):
    g = graphs()[name]
    fin, heads, D = shape
    inp, sq, ref = whole(name, plan, shape, relu)
    got = cpu_rect_layer(g, bounds, plan, *inp, heads, relu=relu)
    for k in ROW_KEYS:
        assert np.array_equal(got[k], sq[k]), k
    np.testing.assert_allclose(got["daL"], ref["daL"], **TOL)
    check_grads_against_ref(got, ref, inp[0], heads)
    return got, sq


@pytest.mark.parametrize("world,bounds", PARTITIONS, ids=PARTITION_IDS)
@pytest.mark.parametrize("shape", PHASE_SHAPES_CPU)
def test_partitioned_twins_equal_the_square_twin_on_the_phase_graph(shape, world, bounds):
    got, sq = check_partitioned("phase", None, shape, True, bounds)
    if world == 1:    # one rank, row_base 0: the square entry points bit for bit, M included
        assert got["parts"][0].lo == 0
        assert np.array_equal(got["M"], sq["M"])
        for k in ("dW", "db", "dwL", "dbL"):
            assert np.array_equal(got[k], sq[k]), k


@pytest.mark.parametrize("world,bounds", PARTITIONS[1:], ids=PARTITION_IDS[1:])
@pytest.mark.parametrize("plan", PLANS)
def test_partitioned_twins_keep_the_hub_chunks(plan, world, bounds):
    """hub_sym_graph under both plans: a rank's hub rows are the whole graph's (the same
    threshold), cut into the same chunks."""
    got, sq = check_partitioned("hub", plan, (37, 4, 16), False, bounds)
    assert sq["hubs"][0] == HUB_SYM_PLAN_SIZES[plan][0]
    hubs = sum(PlannedCsr(p.graph, *plan).n_rows_split for p in got["parts"])
    assert hubs == HUB_SYM_PLAN_SIZES[plan][0]
    base = whole("hub", None, (37, 4, 16), False)[1]
    rows = np.diff(graphs()["hub"].rowptr) <= plan[0]
    assert np.array_equal(got["Y"][rows], base["Y"][rows]) and not np.array_equal(got["Y"][~rows], base["Y"][~rows])


def test_q_pack_and_unpack_twins():
    rng = np.random.default_rng(2)
    H = 5
    xe = rng.uniform(-1, 1, (40, 128)).astype(np.float32)
    keep = xe.copy()
    rows = np.arange(37, 0, -3, dtype=np.int32)
    slots = [116 + 4 * (h // 3) + h % 3 for h in range(H)]
    out = np.empty((len(rows), H), np.float32)
    _abi.call_cpu("gala_gat_in_q_gather_f32", len(rows), P(rows), 40, H, P(xe), P(out), None)
    assert np.array_equal(out, keep[rows][:, slots])
    src = rng.uniform(-1, 1, (len(rows), H)).astype(np.float32)
    _abi.call_cpu("gala_gat_in_q_scatter_f32", len(rows), P(rows), 0, 40, H, P(src), P(xe), None)
    keep[np.ix_(rows, slots)] = src
    assert np.array_equal(xe, keep)
    _abi.call_cpu("gala_gat_in_q_scatter_f32", len(rows), None, 7, 40, H, P(src), P(xe), None)   # a block
    keep[np.ix_(np.arange(7, 7 + len(rows)), slots)] = src
    assert np.array_equal(xe, keep)
    C = _abi.cpu_lib()
    assert C.gala_cpu_gat_in_q_scatter_f32(len(rows), None, 40 - len(rows) + 1, 40, H, P(src), P(xe), None) == \
        _abi.GALA_ERR_INVALID_ARG
    assert C.gala_cpu_gat_in_q_gather_f32(3, P(rows), 40, 9, P(xe), P(out), None) == _abi.GALA_ERR_UNSUPPORTED


def test_rectangular_status_codes():
    """row_base < 0 and row_base + n_rows > n_cols: invalid; n_rows > n_cols: unsupported; the
    square entry points still refuse a pattern that is not square -- on both libraries, before
    any launch (host pointers throughout)."""
    part = make_parts(graphs()["phase"], PARTITIONS[2][1])[1]
    hg = part.graph
    assert 0 < part.lo and hg.n_rows < hg.n_cols
    fin, heads, D = 37, 4, 16
    F = heads * D
    xext, W = np.zeros((hg.n_cols, 128), np.float32), np.zeros((F, fin), np.float32)
    Y, q = np.zeros((hg.n_rows, F), np.float32), np.zeros((hg.n_rows, heads), np.float32)
    M, ws = np.zeros((heads, D, fin + 1), np.float32), np.zeros(8, np.float32)
    A = HostCsr(hg)
    tall = HostCsr(hg)
    tall.c.n_cols = hg.n_rows - 1
    C, G = _abi.cpu_lib(), _abi.lib()

    def fwd(fn, a, *base):
        return fn(a.ref, *base, None, fin, heads, D, 0.2, P(xext), P(W), fin, None, P(Y), P(Y), F, P(q), P(q), 0, None)

    def fwd_t(fn, a, *base):
        return fn(a.ref, *base, None, fin, heads, D, 0.2, P(xext), P(W), fin, None, P(Y), P(Y), F, P(q), P(q), 0,
                  P(xext), None)

    def bwd(fn, a, *base):
        return fn(a.ref, *base, None, fin, heads, D, 0.2, P(xext), P(Y), P(Y), P(Y), F, P(q), P(q), P(M), P(ws),
                  1 << 30, 0, None)

    def qpass(a, base):
        return G.gala_gat_in_q_rect_f32(a.ref, base, heads, 0.2, P(xext), P(xext), None)

    past = hg.n_cols - hg.n_rows + 1
    calls = [(fwd, C.gala_cpu_gat_in_fwd_rect_f32), (bwd, C.gala_cpu_gat_in_bwd_rect_f32),
             (fwd, G.gala_gat_in_fwd_rect_f32), (fwd_t, G.gala_gat_in_fwd_t_rect_f32),
             (bwd, G.gala_gat_in_bwd_rect_f32)]
    for call, fn in calls:
        assert call(fn, A, -1) == _abi.GALA_ERR_INVALID_ARG, fn
        assert call(fn, A, past) == _abi.GALA_ERR_INVALID_ARG, fn
        assert call(fn, tall, 0) == _abi.GALA_ERR_UNSUPPORTED, fn
    assert qpass(A, -1) == qpass(A, past) == _abi.GALA_ERR_INVALID_ARG and qpass(tall, 0) == _abi.GALA_ERR_UNSUPPORTED
    for call, fn in ((fwd, C.gala_cpu_gat_in_fwd_f32), (bwd, C.gala_cpu_gat_in_bwd_f32), (fwd, G.gala_gat_in_fwd_f32),
                     (fwd_t, G.gala_gat_in_fwd_t_f32), (bwd, G.gala_gat_in_bwd_f32)):
        assert call(fn, A) == _abi.GALA_ERR_UNSUPPORTED, fn
