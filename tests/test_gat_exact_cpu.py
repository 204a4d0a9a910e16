"""The exact GAT pair on the host (gala_cpu_gat_{fwd,bwd}_stats_exact_f32, the twins of the HIP
kernels): the float64 reference against torch.autograd, the twins against the float64
reference per element, and the constants of the bounds (tests/_gat_exact_ref.py)."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest
import torch

import _edge_ref as E
import _gat_exact_ref as X
from gala import _abi, backend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_has_the_exact_pair():
    for lib in (_abi.lib(), _abi.cpu_lib()):
        pre = "gala_cpu_" if lib is _abi.cpu_lib() else "gala_"
        assert hasattr(lib, pre + "gat_fwd_stats_exact_f32") and hasattr(lib, pre + "gat_bwd_stats_exact_f32")
    assert _abi.lib().gala_abi_version() == 6


def test_reference_is_the_derivative():
    """exact_layer's gradients are torch.autograd's of the dense float64 layer: 211 rows, 3
    heads, logits on a grid of 1/64 (their fp32 sum is exact, so both see the same branch)."""
    rng = np.random.default_rng(1)
    src, dst = rng.integers(0, 190, 900).astype(np.int32), rng.integers(0, 190, 900).astype(np.int32)
    g = X.symmetrise(X.layout.csr_build(211, 211, src, dst), loops=False)       # vertices 190.. isolated
    n, H, D = g.n_rows, 3, 5
    aL = (rng.integers(-192, 193, (n, H)) / 64.0).astype(np.float32)
    aR = (rng.integers(-192, 193, (n, H)) / 64.0 + 1.0 / 128).astype(np.float32)     # no logit is 0
    Xf, dY = E._u(rng, -1, 1, n, H * D), E._u(rng, -1, 1, n, H * D)
    ref = X.exact_layer(g, aL, aR, Xf, dY, H)
    mask = torch.zeros((n, n), dtype=torch.bool)
    R = ref.R
    mask[torch.from_numpy(R.row), torch.from_numpy(R.col)] = True
    taL, taR, tX = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (aL, aR, Xf))
    z = torch.nn.functional.leaky_relu(taL[:, None, :] + taR[None, :, :], float(np.float32(X.SLOPE)))   # [r, c, h]; the fp32 slope
    z = z.masked_fill(~mask[:, :, None], -float("inf"))
    nonempty = torch.from_numpy(R.deg > 0)
    a = torch.zeros_like(z)
    a[nonempty] = torch.softmax(z[nonempty], dim=1)
    Y = torch.einsum("rch,chd->rhd", a, tX.view(n, H, D)).reshape(n, H * D)
    Y.backward(torch.tensor(dY, dtype=torch.float64))
    assert (R.deg == 0).sum() > 10
    for name, got, want in (("Y", ref.Y, Y.detach()), ("dX", ref.dX, tX.grad), ("daL", ref.daL, taL.grad),
                            ("daR", ref.daR, taR.grad)):
        err = np.abs(got - want.numpy()).max()
        assert err < 1e-12, (name, err)
    # what the REF backward would give instead is far from it
    assert np.abs(ref.daL - ref.daR).max() > 1e-2 and np.abs(ref.dX_on_A - ref.dX).max() > 1e-2


_WORST = {}


def _twin_case(case):
    name, H, F, rc, big = case
    g = X.graph(name)
    i = X.inputs(g, H, F, rc, big)
    be = backend.CpuBackend()
    cg = be.graph(g)
    cg.set_split_plan(*X.PLAN)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    aL, Xt, dY = t(i.aL), t(i.X), t(i.dY)
    if rc:
        Y, lse, Ym, sma, aR = be.gat_stats_exact(cg, aL, None, Xt, H, X.SLOPE, wR=t(i.wR), bR=t(i.bR))
        ar64, arm = X.source_logits(i.X, i.wR, i.bR, H)
        E.assert_bounded("aR_out", aR.numpy(), ar64, arm, X.C_AR, g=g, per="row", record=False)
    else:
        Y, lse, Ym, sma, aR = be.gat_stats_exact(cg, aL, t(i.aR), Xt, H, X.SLOPE)
    dX, daL, daR = be.gat_bwd_stats_exact(cg, aL, aR, Xt, dY, lse, Y, Ym, sma, H, X.SLOPE)
    ref = X.exact_layer(g, i.aL, aR.numpy(), i.X, i.dY, H)
    got = dict(Y=Y.numpy(), Ym=Ym.numpy(), sma=sma.numpy(), lse=lse.numpy(), dX=dX.numpy(), daL=daL.numpy(),
               daR=daR.numpy())
    return g, i, ref, got, aR.numpy().reshape(g.n_rows, H)


@pytest.mark.parametrize("case", X.CASES, ids=X.case_id)
def test_twins_against_float64(case):
    """Every output of the twins within c * mass of the float64 layer; the worst ratios go to
    GALA_GAT_EXACT_RECORD (a JSON-lines file) when set -- profiles/gat_exact_bounds_cpu.jsonl
    holds them, and _gat_exact_ref.MEASURED their maxima."""
    g, i, ref, got, aR = _twin_case(case)
    if case[4]:
        z = i.aL.reshape(-1, case[1])[ref.R.row] + aR[ref.R.col]
        assert (z > 30).sum() > 100, "logits where the REF softmax's clamp would matter"
    worst = X.check(X.case_id(case), got, ref, g)
    _WORST[X.case_id(case)] = worst
    path = os.environ.get("GALA_GAT_EXACT_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(json.dumps({"case": X.case_id(case), "backend": "cpu", **worst}) + "\n")
    # REF's gradients cannot pass: d_aR is not d_aL, and dX over A is not dX over A^T
    far = lambda a, b, mass, c: float(np.max(np.abs(a - b) / (c * mass + 1e-12)))
    assert far(ref.daL, ref.daR, ref.daR_mass, X.C["daR"]) > 100
    assert far(ref.dX_on_A, ref.dX, ref.dX_mass, X.C["dX"]) > 100


def test_constants_are_the_measured_ones():
    """MEASURED holds the committed profile's maxima, and C is 8 x that."""
    rows = [json.loads(l) for l in open(os.path.join(ROOT, "profiles", "gat_exact_bounds_cpu.jsonl"))]
    assert {r["case"] for r in rows} == {X.case_id(c) for c in X.CASES}
    for q in X.QUANTITIES:
        worst = max(r[q] for r in rows)
        assert worst <= X.MEASURED[q] <= 1.05 * worst + 1e-12, (q, worst, X.MEASURED[q])
        assert X.C[q] == E.c_from(X.MEASURED[q])


def test_plan_changes_only_hub_rows():
    """Rows at or below the threshold are bit-identical with and without a plan; hub rows are
    summed as chunk partials (a different association: some differ)."""
    name, H, F = "long", 8, 64
    g = X.graph(name)
    i = X.inputs(g, H, F, False, False)
    be = backend.CpuBackend()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out = []
    for plan in (None, X.PLAN):
        cg = be.graph(g)
        if plan:
            cg.set_split_plan(*plan)
        f = be.gat_stats_exact(cg, t(i.aL), t(i.aR), t(i.X), H, X.SLOPE)
        b = be.gat_bwd_stats_exact(cg, t(i.aL), f[4], t(i.X), t(i.dY), f[1], f[0], f[2], f[3], H, X.SLOPE)
        out.append([a.numpy().reshape(g.n_rows, -1) for a in f[:4] + b])
    hub = np.diff(g.rowptr) > X.PLAN[0]
    # d_aL (index 5) of an ordinary row reads only its own forward rows; dX / d_aR of an ordinary
    # row read hub rows' lse and g through the side lines, whose last bits the plan may change
    for k, (a, b) in enumerate(zip(*out)):
        if k in (0, 1, 2, 3, 5):
            assert np.array_equal(a[~hub], b[~hub]), k
    assert any(not np.array_equal(a[hub], b[hub]) for a, b in zip(*out))
    far = ~hub & ~X.has_neighbour_in(g, hub)     # no hub row's side line is read: dX (4), d_aR (6) too
    assert far.sum() > 50
    for k in (4, 6):
        assert np.array_equal(out[0][k][far], out[1][k][far]), k


def test_argument_checks():
    g = X.graph("cora")
    be = backend.CpuBackend()
    cg = be.graph(g)
    i = X.inputs(g, 2, 12, False, False)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    # D / VEC = 3 lanes per head: not a power of two
    with pytest.raises(_abi.GalaError) as e:
        be.gat_stats_exact(cg, t(i.aL), t(i.aR), t(i.X), 2, X.SLOPE)
    assert e.value.status == _abi.GALA_ERR_UNSUPPORTED
    # a directed pattern is refused before any call
    d = be.graph(X.G.with_empty_rows())
    assert not d.symmetric and cg.symmetric
    z = torch.zeros(d.n_rows, 4)
    v = torch.zeros(d.n_rows)
    with pytest.raises(ValueError):
        be.gat_bwd_stats_exact(d, v, v, z, z, v, z, z, v, 1, X.SLOPE)
