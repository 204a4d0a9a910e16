"""The exact GAT layer on a directed pattern on the GPU (gala_gat_bwd_stats_exact_t_f32 after the
exact forward, gala_csr_is_transpose_i32): every output against the float64 layer per element
(the constants of tests/_gat_exact_directed_ref.py, measured on the host twins) and against the
twins, the symmetric pair as the special case, the transpose test past one round of its
grid-stride loop, the plan of A^T, the operator mirror and a compiled program with
GALA_GAT_EXACT_DIRECTED=1, the argument checks."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import _edge_ref as E
import _gat_exact_directed_ref as D
import _gat_exact_ref as X
from gala import _abi, backend, layout, ops

pytestmark = pytest.mark.gpu
NAMES = ("Y", "lse", "Ym", "sma", "dX", "daL", "daR")
ENV = "GALA_GAT_EXACT_DIRECTED"
CHECK_ROUND = D.CHECK_ROUND      # k_csr_is_transpose's items per round (csrc/csr_check.hip:23, 106-107)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(dg, dgT, i, H):
    """(outputs in NAMES order as device tensors, aR used) through gala.ops' directed helper."""
    aL, Xd, dY = _dev(i.aL), _dev(i.X), _dev(i.dY)
    kw = dict(wR=_dev(i.wR), bR=_dev(i.bR)) if i.rc else dict(aR=_dev(i.aR))
    (Y, lse, Ym, sma, aR), (dX, daL, daR) = ops.gat_exact_directed(dg, dgT, aL, Xd, dY, heads=H, slope=D.SLOPE, **kw)
    return (Y, lse, Ym, sma, dX, daL, daR), aR


def _host(outs, n):
    return {k: v.cpu().numpy().reshape(n, -1) for k, v in zip(NAMES, outs)}


@pytest.mark.parametrize("case", D.CASES, ids=D.case_id)
def test_kernels_against_float64_and_twins(case):
    name, H, F, rc, big = case
    g, i, ref, twin, aRt = D.twin_case(case)
    gT = D.transposed(g)
    dg, dgT = ops.DeviceGraph.from_host(g), ops.DeviceGraph.from_host(gT)
    assert (dg.split_rows > 0) == (name != "uni") == (dgT.split_rows > 0)
    outs, aR = _run(dg, dgT, i, H)
    again, _ = _run(dg, dgT, i, H)
    torch.cuda.synchronize()
    for k, a, b in zip(NAMES, outs, again):
        assert torch.equal(a, b), f"{k}: not bit-identical run to run"
    got = _host(outs, g.n_rows)
    aRh = aR.cpu().numpy().reshape(g.n_rows, H)
    if not np.array_equal(aRh, aRt):
        # the kernel's recomputed source logits differ from the twin's in some last bit: the float64
        # layer and the twins from the logits the kernels used
        ar64, arm = X.source_logits(i.X, i.wR, i.bR, H)
        E.assert_bounded("aR_out", aRh, ar64, arm, X.C_AR, g=g, per="row", record=False)
        ref = D.directed_layer(g, i.aL, aRh, i.X, i.dY, H)
        be = backend.CpuBackend()
        cg, cgT = be.graph(g), be.graph(gT)
        cg.set_split_plan(*D.PLAN)
        cgT.set_split_plan(*D.PLAN)
        j = D.inputs(g, H, F, False, big)
        j.aR = aRh
        twin, _ = D.twin_layer(be, cg, cgT, j, H)
    worst = D.check("gpu " + D.case_id(case), got, ref)
    print("gpu", D.case_id(case), {k: f"{v:.3g}" for k, v in worst.items()})
    # two fp32 evaluations of one element, each within c of the float64 layer
    for k in NAMES:
        E.assert_bounded(f"gpu vs twin {k}", got[k], twin[k].reshape(g.n_rows, -1), getattr(ref, k + "_mass"),
                         2 * D.C[k], g=ref.R if k in D.FWD else ref.RT, per="row", chunk=D.PLAN[1], record=False)


@pytest.mark.parametrize("name,H,F", [("cora", 1, 47), ("long", 8, 64)])
def test_symmetric_pair_is_the_special_case(name, H, F):
    """On a symmetric (g, g) the directed backward is bit-identical to gala_gat_bwd_stats_exact_f32
    (hub rows of the plan included)."""
    g = X.graph(name)
    i = X.inputs(g, H, F, False, True)
    dg = ops.DeviceGraph.from_host(g)
    aL, Xd, dY = _dev(i.aL), _dev(i.X), _dev(i.dY)
    Y, lse, Ym, sma, aR = ops.gat_fwd_stats_exact(dg, aL, Xd, aR=_dev(i.aR), heads=H, slope=X.SLOPE)
    a = ops.gat_bwd_stats_exact(dg, aL, aR, Xd, dY, lse, Y, Ym, sma, heads=H, slope=X.SLOPE)
    b = ops.gat_bwd_stats_exact_t(dg, dg, aL, aR, Xd, dY, lse, Y, Ym, sma, heads=H, slope=X.SLOPE)
    assert ops.is_transpose(dg, dg)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def test_rows_of_the_transpose_below_the_threshold_do_not_depend_on_its_plan():
    """With and without a hub-row plan on A^T (A's plan fixed, so the forward and the side lines are
    the same): every output of a row of A^T at or below the threshold is bit-identical; its hub
    row is summed as chunk partials."""
    g = D.graph("split")
    gT = D.transposed(g)
    i = D.inputs(g, 8, 256, False, False)
    dg = ops.DeviceGraph.from_host(g)
    a, _ = _run(dg, ops.DeviceGraph.from_host(gT), i, 8)
    b, _ = _run(dg, ops.DeviceGraph.from_host(gT, split=False), i, 8)
    a, b = _host(a, g.n_rows), _host(b, g.n_rows)
    hub = np.diff(gT.rowptr) > D.PLAN[0]
    assert hub.sum() == 1
    for k in NAMES:
        assert np.array_equal(a[k][~hub], b[k][~hub]), k
    assert any(not np.array_equal(a[k][hub], b[k][hub]) for k in ("dX", "daR"))


# ---- the transpose test -----------------------------------------------------------------------

def _count(a, at):
    da, dat = ops.DeviceGraph.from_host(a, split=False), ops.DeviceGraph.from_host(at, split=False)
    count = torch.full((1,), -1, device="cuda", dtype=torch.int32)
    _abi.call("gala_csr_is_transpose_i32", da.csr(), dat.csr(), count.data_ptr(), torch.cuda.current_stream().cuda_stream)
    return int(count.item())


@pytest.mark.parametrize("name", ["uni", "rmat", "split"])
def test_is_transpose_on_the_device(name):
    g = D.graph(name)
    gT = D.transposed(g)
    assert _count(g, gT) == 0 and _count(gT, g) == 0
    dg, dgT = ops.DeviceGraph.from_host(g), ops.DeviceGraph.from_host(gT)
    assert ops.is_transpose(dg, dgT) and not ops.is_transpose(dg, dg)
    for k, (a, at) in D.negatives(g, gT).items():
        assert _count(a, at) > 0, k
    s = X.graph("cora")
    assert _count(s, s) == 0


def test_is_transpose_past_one_round():
    """n + 2 E items past the grid cap: the last round holds only edges of a; the one planted
    mismatch is an edge of a in that round (at stays well-formed, so no other item sees it)."""
    rng = np.random.default_rng(4)
    n, E_ = 4000, 130_000
    key = np.unique(rng.integers(0, n * n, 140_000))
    key = np.sort(rng.choice(key, E_, replace=False))
    g = D.simple(n, key // n, key % n)
    gT = layout.transpose(g)[0]
    total = n + 2 * g.nnz
    assert CHECK_ROUND == D.check_round_from_source()    # the launch code's cap, not only this file's copy
    assert g.nnz == E_ and CHECK_ROUND < total < 2 * CHECK_ROUND
    first = CHECK_ROUND - n - g.nnz                      # a's first edge of the second round
    assert 0 < first < g.nnz - 100
    assert _count(g, gT) == 0
    # a's edge e = (r, c): in row c of at the entry r becomes a row that row c does not hold
    rows = np.repeat(np.arange(n), np.diff(g.rowptr))
    for e in (first, g.nnz - 1):
        r, c = int(rows[e]), int(g.col[e])
        lo, hi = int(gT.rowptr[c]), int(gT.rowptr[c + 1])
        k = lo + int(np.searchsorted(gT.col[lo:hi], r))
        assert gT.col[k] == r
        below = int(gT.col[k - 1]) if k > lo else -1
        above = int(gT.col[k + 1]) if k + 1 < hi else n
        free = [v for v in range(below + 1, above) if v != r]
        assert free, "no free row id between the neighbours"
        col = gT.col.copy()
        col[k] = free[0]
        # the edge of a that at now holds instead, (free[0], c), is not in a: every other edge of a is found
        assert _count(g, layout.HostGraph(n, n, gT.rowptr, col)) == 1, e


# ---- the operator mirror ----------------------------------------------------------------------

@pytest.fixture(scope="module")
def T():
    import gala
    return gala.torch_ext()


def _push(T, g, bw=None, perm=None):
    """Slot 0 = g, slot 1 = its transpose with the edge permutation (a FIXED program's slots)."""
    T.slots_clear()
    T.slots_push(_dev(g.rowptr), _dev(g.col), torch.ones(g.nnz, device="cuda"), None, 1, False)
    if bw is None:
        bw, perm = layout.transpose(g)
    T.slots_push(_dev(bw.rowptr), _dev(bw.col), torch.ones(bw.nnz, device="cuda"), None, 1, False)
    T.slots_set_transpose_perm(1, _dev(perm))


def _layer(T, i, ffn=False):
    """One forward + backward of the FIXED layer: [Y, grads...] on the host."""
    aL, Xd = _dev(i.aL).requires_grad_(), _dev(i.X).requires_grad_()
    if ffn:
        wR, bR = _dev(i.wR.reshape(1, -1)).requires_grad_(), _dev(i.bR).requires_grad_()
        ins = [aL, Xd, wR, bR]
        Y = T.gat_aggregate_ffn_apply(aL, Xd, wR, bR, 0, D.SLOPE, 1)
    else:
        aR = _dev(i.aR).requires_grad_()
        ins = [aL, aR, Xd]
        Y = T.gat_aggregate_apply(aL, aR, Xd, 0, D.SLOPE, 1)
    Y.backward(_dev(i.dY))
    torch.cuda.synchronize()
    return [Y.detach().cpu().numpy()] + [t.grad.cpu().numpy() for t in ins]


@pytest.mark.parametrize("case", [("rmat", 8, 256, False, True), ("split", 1, 47, False, False), ("uni", 2, 8, False, True)],
                         ids=D.case_id)
def test_mirror_with_the_switch(T, monkeypatch, case):
    """The directed FIXED layer through gat_aggregate_apply: with GALA_GAT_EXACT_DIRECTED=1 Y, dX,
    d_aL and d_aR lie within the float64 bounds, and within those bounds of the alpha-storing
    path's (other summation orders: no bit identity, and some bit does differ); a slot 1 that is
    not the transpose (one edge moved) falls back to the alpha-storing path's bits."""
    name, H, F, rc, big = case
    g, i, ref, _, _ = D.twin_case(case)
    n = g.n_rows
    _push(T, g)
    monkeypatch.delenv(ENV, raising=False)
    off = _layer(T, i)
    monkeypatch.setenv(ENV, "1")
    on = _layer(T, i)
    monkeypatch.setenv(ENV, "0")
    assert all(np.array_equal(a, b) for a, b in zip(_layer(T, i), off))
    for tag, o in (("on", on), ("off", off)):
        got = dict(Y=o[0], daL=o[1], daR=o[2], dX=o[3])
        D.check(f"mirror {tag}", {k: v.reshape(n, -1) for k, v in got.items()}, ref, chunk=None)
    for k, a, b in zip(("Y", "daL", "daR", "dX"), on, off):
        E.assert_bounded(f"mirror on vs off {k}", a.reshape(n, -1), b.reshape(n, -1), getattr(ref, k + "_mass"),
                         2 * D.C[k], g=ref.R if k in D.FWD else ref.RT, per="row", record=False)
    assert not all(np.array_equal(a, b) for a, b in zip(on, off))     # the switch does switch
    # slot 1 with one edge moved to the next row (no transpose; the permutation goes with it)
    bw, perm = layout.transpose(g)
    _push(T, g, D.negatives(g, bw)["moved"][1], perm)
    monkeypatch.setenv(ENV, "1")
    moved_on = _layer(T, i)
    monkeypatch.delenv(ENV)
    moved_off = _layer(T, i)
    assert all(np.array_equal(a, b) for a, b in zip(moved_on, moved_off))


def test_mirror_ffn_layer_with_the_switch(T, monkeypatch):
    """The DSL's layer (aR = Linear(X) recomputed in the kernels), 8 heads x 32 on the R-MAT graph:
    Y and every gradient of the two paths within the float64 bounds."""
    case = ("rmat", 8, 256, True, False)
    g, i, _, _, _ = D.twin_case(case)
    H, F = case[1], case[2]
    _push(T, g)
    monkeypatch.setenv(ENV, "1")
    on = _layer(T, i, ffn=True)
    monkeypatch.delenv(ENV)
    off = _layer(T, i, ffn=True)
    assert not all(np.array_equal(a, b) for a, b in zip(on, off))
    ar64, _ = X.source_logits(i.X, i.wR, i.bR, H)
    ref = D.directed_layer(g, i.aL, ar64.astype(np.float32), i.X, i.dY, H)
    Dh = F // H
    wR = i.wR.astype(np.float64)
    dX64 = ref.dX + np.repeat(ref.daR, Dh, axis=1) * wR[None, :]
    dXm = ref.dX_mass + np.repeat(ref.daR_mass, Dh, axis=1) * np.abs(wR)[None, :]
    x64 = i.X.astype(np.float64)
    dW64 = (np.repeat(ref.daR, Dh, axis=1) * x64).sum(0)
    dWm = (np.repeat(ref.daR_mass, Dh, axis=1) * np.abs(x64)).sum(0)
    for tag, o in (("on", on), ("off", off)):
        D.check(f"ffn {tag}", dict(Y=o[0], daL=o[1].reshape(g.n_rows, -1)), ref)
        E.assert_bounded(f"ffn {tag} dX", o[2], dX64, dXm, D.C["dX"], g=ref.RT, per="row", record=False)
        E.assert_bounded(f"ffn {tag} dW", o[3].ravel(), dW64, dWm, D.C["daR"], record=False)
        E.assert_bounded(f"ffn {tag} db", o[4].ravel(), ref.daR.sum(0), ref.daR_mass.sum(0), D.C["daR"], record=False)


def test_compiled_directed_fixed_program(tmp_path):
    """tests/dsl/gat_directed_fixed.txt (gat_directed.txt with gat_fixed_gradients(true)) compiled by
    galac, one epoch on the GPU on a directed graph with distinct edges, through the runtime's own
    slot upload (both layers run gat_aggregate_ffn_apply on slots 0 and 1: FIXED keeps the first
    layer out of input space): with the switch set it meets the float64 executor of its IR,
    gradients included, and its gradients are not the alpha-storing path's bits
    (D.check_directed_fixed_program)."""
    D.check_directed_fixed_program(tmp_path)


def test_compiled_directed_fixed_program_falls_back_on_duplicate_edges(tmp_path, monkeypatch):
    """The same program on the synthetic Cora graph, which stores two edges twice: its transpose
    has no strictly ascending rows, gala_csr_is_transpose_i32 says no, and both layers keep the
    alpha-storing path bit for bit (and meet the IR's executor)."""
    from _dsl_check import PROGS, check_against_ir, run_prog
    assert "gat_directed_fixed" in PROGS, "run tools/build_dsl_progs.py (build()) first"
    monkeypatch.setenv(ENV, "1")
    _, on = run_prog("gat_directed_fixed", tmp_path, "--iters", "1")
    check_against_ir("gat_directed_fixed", on)
    rows = np.repeat(np.arange(len(on["rowptr"]) - 1), np.diff(on["rowptr"]))
    key = rows.astype(np.int64) * len(on["rowptr"]) + on["col"]
    assert np.unique(key).shape[0] < key.shape[0]       # (the duplicates that make it fall back)
    monkeypatch.delenv(ENV)
    _, off = run_prog("gat_directed_fixed", tmp_path, "--iters", "1")
    assert all(np.array_equal(on[k], off[k]) for k in on if k.startswith("grad:"))


def test_argument_checks():
    g = D.graph("split")
    gT = D.transposed(g)
    H, F = 8, 64
    i = D.inputs(g, H, F, False, False)
    dg, dgT = ops.DeviceGraph.from_host(g), ops.DeviceGraph.from_host(gT)
    aL, aR, Xd, dY = _dev(i.aL), _dev(i.aR), _dev(i.X), _dev(i.dY)
    Y, lse, Ym, sma, _ = ops.gat_fwd_stats_exact(dg, aL, Xd, aR=aR, heads=H, slope=D.SLOPE)
    n = g.n_rows
    out = [torch.full((n, F), 7.0, device="cuda"), torch.full((n * H,), 7.0, device="cuda"),
           torch.full((n * H,), 7.0, device="cuda")]
    side = torch.full((n * H * 4,), 7.0, device="cuda")
    need = 2 * F + H

    def bwd(a, at):
        return _abi.lib().gala_gat_bwd_stats_exact_t_f32(
            a, at, aL.data_ptr(), aR.data_ptr(), Xd.data_ptr(), F, dY.data_ptr(), F, F, H, D.SLOPE, lse.data_ptr(),
            Y.data_ptr(), F, Ym.data_ptr(), F, sma.data_ptr(), side.data_ptr(), out[0].data_ptr(), F,
            out[1].data_ptr(), out[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
    # the plan of A^T has a hub row: a workspace too small for it is refused, nothing launched
    # (the pre-pass over A's rows neither: the side table stays as it was)
    dgT.csr(need)
    plan = dgT._split["plan"]
    assert plan.n_rows_split == 1 and plan.ws_cols >= need
    keep = plan.ws_cols
    plan.ws_cols = need - 1
    try:
        assert bwd(dg.csr(), dgT.csr()) == _abi.GALA_ERR_INVALID_ARG
    finally:
        plan.ws_cols = keep
    # mismatched n, a tiled pattern
    small = ops.DeviceGraph.from_host(D.simple(n - 1, [0, 1], [1, 0]))
    tiled = ops.DeviceGraph.from_host(layout.col_tile(g, 1000))
    count = torch.full((1,), -1, device="cuda", dtype=torch.int32)
    for a, at in ((dg, small), (small, dgT), (dg, tiled), (tiled, dgT)):
        assert bwd(a.csr(), at.csr()) == _abi.GALA_ERR_INVALID_ARG
        st = _abi.lib().gala_csr_is_transpose_i32(a.csr(), at.csr(), count.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert st == _abi.GALA_ERR_INVALID_ARG
        assert not ops.is_transpose(a, at)
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in out + [side]) and int(count.item()) == -1
    assert bwd(dg.csr(), dgT.csr()) == _abi.GALA_OK
    # a shape the pair refuses
    z, v = torch.zeros(n, 12, device="cuda"), torch.zeros(n * 2, device="cuda")
    with pytest.raises(_abi.GalaError) as e:
        ops.gat_bwd_stats_exact_t(dg, dgT, v, v, z, z, v, z, z, v, heads=2)
    assert e.value.status == _abi.GALA_ERR_UNSUPPORTED
    # the helper tests the pair once, and refuses a second pattern that is not the transpose
    calls = []
    orig = ops.is_transpose
    try:
        ops.is_transpose = lambda a, b: (calls.append(1), orig(a, b))[1]
        other = ops.DeviceGraph.from_host(g)
        for _ in range(2):
            with pytest.raises(ValueError):
                ops.gat_exact_directed(dg, other, aL, Xd, dY, aR=aR, heads=H)
        fresh = ops.DeviceGraph.from_host(gT)
        for _ in range(2):
            ops.gat_exact_directed(dg, fresh, aL, Xd, dY, aR=aR, heads=H)
    finally:
        ops.is_transpose = orig
    assert len(calls) == 2
