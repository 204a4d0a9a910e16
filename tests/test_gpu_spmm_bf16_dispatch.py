"""GPU: every branch of the bf16 SpMM's dispatch (GALA_SPMM_X_BF16 / GALA_SPMM_Y2_BF16: spmm_bf16() in
csrc/spmm.hip, the kernels of csrc/spmm_bf16.hip) against the oracle, bit for bit.

Widening bf16 to fp32 is exact and the sums stay fp32 chains in CSR order, so ops.spmm on a bf16 X
must equal oracle.spmm on X.float() bit for bit -- no tolerance anywhere.  Every case of CASES runs
on tests/_bf16_graphs.py's graph under its plan (the hub rows in k_spmm_bf16_hub on the plan's side
stream: tiles of 64 .. 512 edges, rows of 1 .. 41 tiles, every remainder of the chain's rotation)
and again without a plan (every row in k_spmm_bf16_rows).  A case first asserts the branch it is
there for -- the vector width, the column ranges, the row kernel's (G, CH), the hub kernel's
(FSP, T) and the edge-weight heads per hub slice -- from _bf16_graphs' mirror of the dispatch.

The epilogue fields the oracle lacks: dst_deg is the oracle's dst_scale with the device's own
deg^-0.5 (ops.degree: the same expression), out2 is the fp32 product s2 * Y of the oracle's Y, and
a bf16 out2 is that product rounded to nearest even; both are also compared with the fp32 call on
X.float().

Made in the library, f_base read as 0 in k_spmm_bf16_rows' head index (the weight's head of a
column past the first range) turns both runs of w264h4_xv1, w264h4_xv1_rs and f32x_y2b_264_h4 red
and leaves tests/test_gpu_spmm_bf16.py green.
"""
import functools
from dataclasses import dataclass

import numpy as np
import pytest
import torch

import _bf16_graphs as B
import oracle as orc
from gala import ops
from _graphs import to_oracle

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
SENTINEL = -7.0


@dataclass(frozen=True)
class Case:
    id: str
    F: int
    expect: tuple           # (xv, ((range F, (G, CH), (FSP, T, heads per slice) | None), ...)) under the plan
    x: str = "bf16"         # X's storage
    xoff: int = 0           # X is columns xoff .. xoff + F of a buffer of ldx columns
    ldx: int = 0            # (0: xoff + F)
    ldy: int = 0            # out (and out2) are the first F columns of a buffer of ldy columns (0: F)
    heads: int = 0          # edge-weight heads; 0: no edge weights
    rs: bool = False        # val_row_scale
    src: bool = False
    dst: bool = False
    accum: bool = False
    deg: bool = False       # dst_deg
    y2: str = ""            # out2's storage: "", "f32", "bf16"


def R(F, G, CH, fsp=None, T=None, hps=()):
    return (F, (G, CH), None if fsp is None else (fsp, T, tuple(hps)))


W1 = dict(heads=1)
CASES = [
    # ---- column ranges: F > 256 * xv --------------------------------------------------------------
    Case("r264_xv1_base2", 264, (1, (R(256, 64, 4, 64, 64), R(8, 8, 1, 32, 128))), xoff=1, ldx=266, src=True, dst=True),
    Case("r513_xv1_oddld", 513, (1, (R(256, 64, 4, 64, 64), R(256, 64, 4, 64, 64), R(1, 1, 1, 32, 128)))),
    Case("r514_xv2", 514, (2, (R(512, 64, 4, 64, 128), R(2, 1, 1, 32, 256)))),
    Case("r2056_xv8", 2056, (8, (R(2048, 64, 4, 64, 256), R(8, 1, 1, 32, 512)))),
    # head_dim 66: column 256, the second range's first, is head 3's
    Case("w264h4_xv1", 264, (1, (R(256, 64, 4, 64, 64, (1, 2, 2, 2)), R(8, 8, 1, 32, 128, (1,)))), xoff=1, ldx=266, heads=4),
    Case("w264h4_xv1_rs", 264, (1, (R(256, 64, 4, 64, 64, (1, 2, 2, 2)), R(8, 8, 1, 32, 128, (1,)))), xoff=1, ldx=266,
         heads=4, rs=True, src=True),
    # fp32 X, bf16 out2: k_spmm_hub_exact on an offset X and Y, then k_spmm_bf16_hub_y2; with 4 heads no hub kernel
    Case("f32x_y2b_264", 264, (1, (R(256, 64, 4, 64, None), R(8, 8, 1, 32, None))), x="f32", ldx=265, deg=True, y2="bf16"),
    Case("f32x_y2b_264_h4", 264, (1, (R(256, 64, 4), R(8, 8, 1))), x="f32", ldx=265, heads=4, dst=True, y2="bf16"),
    # ---- the nine row-kernel shapes in 16-byte vectors; ACCUM with dst_deg and out2 ----------------
    Case("f8", 8, (8, (R(8, 1, 1, 32, 512),))),
    Case("f16_accum_deg_y2f", 16, (8, (R(16, 2, 1, 32, 512),)), accum=True, deg=True, y2="f32"),
    Case("f32", 32, (8, (R(32, 4, 1, 32, 512),))),
    Case("f64", 64, (8, (R(64, 8, 1, 64, 256),))),
    Case("f128_accum_deg_y2b", 128, (8, (R(128, 16, 1, 64, 256),)), accum=True, deg=True, y2="bf16"),
    Case("f256", 256, (8, (R(256, 32, 1, 64, 256),))),
    Case("f512", 512, (8, (R(512, 32, 2, 64, 256),))),
    Case("f1024", 1024, (8, (R(1024, 64, 2, 64, 256),))),
    Case("f1032", 1032, (8, (R(1032, 64, 4, 64, 256),))),                     # the first L past 128
    Case("f2042_padded", 2042, (8, (R(2042, 64, 4, 64, 256),)), ldx=2048, ldy=2048),   # a masked last vector of 2
    # ---- the three shapes past 32 lanes in 8-, 4- and 2-byte vectors; <W, SRCS> = <1, 1> in each ----
    Case("f132_xv4_w_src", 132, (4, (R(132, 32, 2, 64, 256, (1, 1, 1)),)), src=True, **W1),
    Case("f260_xv4", 260, (4, (R(260, 64, 2, 64, 256),))),
    Case("f1022_xv4_padded", 1022, (4, (R(1022, 64, 4, 64, 256),)), ldx=1028, ldy=1024),
    Case("f126_xv2_w_src", 126, (2, (R(126, 32, 2, 64, 128, (1, 1)),)), src=True, **W1),
    Case("f254_xv2", 254, (2, (R(254, 64, 2, 64, 128),))),
    Case("f511_xv2_padded", 511, (2, (R(511, 64, 4, 64, 128),)), ldx=514, ldy=512),
    Case("f47_xv1_w_src", 47, (1, (R(47, 32, 2, 64, 64, (1,)),)), src=True, **W1),
    Case("f100_xv1", 100, (1, (R(100, 64, 2, 64, 64),)), ldx=101),
    Case("f255_xv1", 255, (1, (R(255, 64, 4, 64, 64),)), ldx=257),
    # ---- the hub kernel's <W, SRCS> at both slice widths (<0, 0>: f32 and f64 above) ----------------
    Case("f32_w", 32, (8, (R(32, 4, 1, 32, 512, (1,)),)), **W1),
    Case("f32_src", 32, (8, (R(32, 4, 1, 32, 512),)), src=True),
    Case("f32_w_src", 32, (8, (R(32, 4, 1, 32, 512, (1,)),)), src=True, **W1),
    Case("f64_w", 64, (8, (R(64, 8, 1, 64, 256, (1,)),)), **W1),
    Case("f64_src", 64, (8, (R(64, 8, 1, 64, 256),)), src=True),
    Case("f64_w_src", 64, (8, (R(64, 8, 1, 64, 256, (1,)),)), src=True, **W1),
    # a short last slice of 8 features; ACCUM from Y (no dst factor)
    Case("f72_accum", 72, (8, (R(72, 16, 1, 64, 256),)), accum=True),
    # ---- edge-weight heads per hub slice ----------------------------------------------------------
    Case("f64_h2", 64, (8, (R(64, 8, 1, 64, 256, (2,)),)), heads=2),
    # head_dim 24: boundaries inside both slices; ACCUM behind a dst factor
    Case("f96_h4_rs_accum_dst", 96, (8, (R(96, 16, 1, 64, 256, (3, 2)),)), heads=4, rs=True, accum=True, dst=True),
    Case("f64_h4", 64, (8, (R(64, 8, 1, 64, 256, (4,)),)), heads=4, rs=True),
    # more than kHubHeads heads in a slice: the hub rows stay in the row kernel (split_threshold 0)
    Case("f32_h8", 32, (4, (R(32, 8, 1),)), heads=8),
    Case("f128_h32", 128, (4, (R(128, 32, 1),)), heads=32, rs=True),
]
BY_ID = {c.id: c for c in CASES}


def geometry(c: Case):
    """(ldx, ldy, head_dim, one_head, the out2 view for pick_vec)."""
    ldx, ldy = c.ldx or c.xoff + c.F, c.ldy or c.F
    return ldx, ldy, c.F // c.heads if c.heads else c.F, c.heads <= 1, (0, ldy, c.y2 == "bf16") if c.y2 else None


def branches(c: Case, plan: bool):
    """The case's branch from the mirrored dispatch: (xv, ((range F, (G, CH), hub), ...))."""
    ldx, ldy, head_dim, one_head, y2 = geometry(c)
    xv = B.pick_vec(c.x == "bf16", c.xoff, ldx, 0, ldy, y2, c.F, head_dim, one_head)
    return xv, tuple((r["F"], r["rows"], r["hub"]) for r in B.dispatch(c.x == "bf16", xv, c.F, c.heads, plan))


@functools.lru_cache(None)
def graphs():
    hg = B.bf16_hub_graph()
    B.check_bf16_hub_graph(hg)
    noplan = ops.DeviceGraph.from_host(hg, split=False)
    planned = ops.DeviceGraph.from_host(hg, split=False)
    planned.set_split_plan(hg.rowptr, **B.PLAN)
    assert planned.split_rows == len(B.HUB_DEGREES) and noplan.split_rows == 0
    norm = ops.degree(noplan, power=-0.5).cpu().numpy()       # deg_rsqrt, the dst_deg factor's expression
    assert np.isinf(norm[B.EMPTY_BLOCKS[0][0]]) and norm[B.hub_rows()[0]] == np.float32(1) / np.sqrt(np.float32(65))
    return hg, {True: planned, False: noplan}, norm


@functools.lru_cache(None)
def reference(cid):
    """Host operands and the oracle's Y (and out2), once per case for both of its runs."""
    c = BY_ID[cid]
    hg, _, norm = graphs()
    ldx = geometry(c)[0]
    gen = torch.Generator().manual_seed(CASES.index(c))
    h = dict(X=torch.randn(hg.n_cols, ldx, generator=gen).to(bf16))       # bf16-representable in either storage
    if c.x == "f32":
        h["X"] = h["X"].float()
    h["src"] = torch.rand(hg.n_cols, generator=gen) + 0.5 if c.src else None
    h["dst"] = torch.rand(hg.n_rows, generator=gen) + 0.5 if c.dst else None
    h["val"] = torch.randn(hg.nnz, c.heads, generator=gen) if c.heads else None
    h["rs"] = torch.rand(hg.n_rows, c.heads, generator=gen) + 0.5 if c.rs else None
    h["Y0"] = torch.randn(hg.n_rows, c.F, generator=gen) if c.accum else None
    eff = h["val"]
    if c.rs:    # the factored weight is the rounded fp32 product val * row_scale
        eff = eff * h["rs"][np.repeat(np.arange(hg.n_rows), np.diff(hg.rowptr))]
    og = to_oracle(hg, None if eff is None else eff.numpy().ravel(), max(c.heads, 1))
    ds = norm if c.deg else None if h["dst"] is None else h["dst"].numpy()
    Xw = h["X"][:, c.xoff:c.xoff + c.F].float().contiguous().numpy()
    want = orc.spmm(og, Xw, src_scale=None if h["src"] is None else h["src"].numpy(), dst_scale=ds,
                    Y=None if h["Y0"] is None else h["Y0"].numpy().copy(), accum=c.accum)
    with np.errstate(invalid="ignore"):
        want2 = ds[:, None] * want if c.y2 else None                      # fl(s2 * Y): s2 is the dst factor
    return h, want, want2


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in other places"
    bad = (got.view(np.int32) != want.view(np.int32)) & ~nan
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements differ, in rows "
                           f"{np.unique(np.nonzero(bad)[0])[:8]} and columns {np.unique(np.nonzero(bad)[1])[:8]}")


def same_bf16(got, want32, what):
    """got (bf16) is want32 (fp32) rounded to nearest even; NaN in the same places."""
    want = want32.to(bf16)
    num = ~want32.isnan()
    assert torch.equal(got.isnan(), want32.isnan()), f"{what}: NaN in other places"
    bad = (got.view(torch.int16) != want.view(torch.int16)) & num
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ"


def device_run(c, dg, h, X, y2):
    """ops.spmm of the case on X (its storage or widened), out and out2 inside sentinel buffers."""
    n, (_, ldy, *_) = dg.n_rows, geometry(c)
    cu = lambda t: None if t is None else t.cuda()
    g = dg if not c.heads else dg.with_values(cu(h["val"]), val_heads=c.heads, row_scale=cu(h["rs"]))
    buf = torch.full((n, ldy), SENTINEL, device="cuda")
    if c.accum:
        buf[:, :c.F] = cu(h["Y0"])
    buf2 = torch.full((n, ldy), SENTINEL, device="cuda", dtype=bf16 if y2 == "bf16" else torch.float32) if y2 else None
    out = ops.spmm(g, X, src_scale=cu(h["src"]), dst_scale=cu(h["dst"]), out=buf[:, :c.F], accum=c.accum, dst_deg=c.deg,
                   out2=None if buf2 is None else buf2[:, :c.F])
    torch.cuda.synchronize()
    for b in (buf, buf2):
        assert b is None or bool((b[:, c.F:] == SENTINEL).all()), "the row padding was written"
    assert out.data_ptr() == buf.data_ptr() and buf.data_ptr() % 16 == 0 and (buf2 is None or buf2.data_ptr() % 16 == 0)
    return out, None if buf2 is None else buf2[:, :c.F]


@pytest.mark.parametrize("plan", [True, False], ids=["plan", "noplan"])
@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_bf16_dispatch_equals_the_oracle(cid, plan):
    c = BY_ID[cid]
    hg, dgs, _ = graphs()
    xv, ranges = branches(c, plan)
    assert xv == c.expect[0], (xv, c.expect[0])
    assert ranges == (c.expect[1] if plan else tuple((F, s, None) for F, s, _ in c.expect[1])), ranges
    h, want, want2 = reference(cid)
    Xfull = h["X"].cuda()
    X = Xfull[:, c.xoff:c.xoff + c.F]
    esize = 2 if c.x == "bf16" else 4
    assert Xfull.data_ptr() % 16 == 0 and X.data_ptr() - Xfull.data_ptr() == c.xoff * esize and X.stride(0) == geometry(c)[0]
    assert (c.x == "bf16") == (X.dtype == bf16) and (c.x == "bf16" or c.y2 == "bf16"), "a bf16 operand takes spmm_bf16()"
    got, got2 = device_run(c, dgs[plan], h, X, c.y2)
    same_bits(got.cpu().numpy(), want, f"{cid}: Y against the oracle")
    hubs = B.hub_rows()
    assert np.isfinite(want[hubs]).all() and np.abs(want[hubs]).max() > 1.0, "the hub rows hold sums"
    if not c.y2:
        return
    (same_bf16(got2.cpu(), torch.from_numpy(want2), f"{cid}: out2 against the oracle") if c.y2 == "bf16"
     else same_bits(got2.cpu().numpy(), want2, f"{cid}: out2 against the oracle"))
    # and the fp32 call on the widened input
    Y32, o32 = device_run(c, dgs[plan], h, X.float().contiguous(), "f32")
    same_bits(got.cpu().numpy(), Y32.cpu().numpy(), f"{cid}: Y against the fp32 call")
    (same_bf16(got2, o32, f"{cid}: out2 against the fp32 call") if c.y2 == "bf16"
     else same_bits(got2.cpu().numpy(), o32.cpu().numpy(), f"{cid}: out2 against the fp32 call"))


def test_the_table_covers_the_dispatch():
    """Over CASES' asserted branches: all nine row-kernel shapes in 16-byte vectors, the three past 32
    lanes in every narrower vector, both slice widths, all four tile sizes, all four <W, SRCS> at both
    slice widths in 16-byte vectors and <1, 1> in every vector, two and three column ranges, 1 .. 4
    heads in a slice and the fallback past that, ACCUM on hub rows behind and without a dst factor."""
    assert len(CASES) <= 40 and len(BY_ID) == len(CASES)
    shapes, hubs, flags, n_ranges, hps, fallback = set(), set(), set(), set(), set(), set()
    for c in CASES:
        xv, ranges = branches(c, True)
        assert (xv, ranges) == c.expect, c.id
        n_ranges.add(len(ranges))
        for F, shape, hub in ranges:
            shapes.add((xv, shape))
            if c.x != "bf16":
                continue
            if hub is None:
                fallback.add(c.id)
                continue
            hubs.add((hub[0], hub[1]))
            flags.add((xv, hub[0], c.heads > 0, c.src))
            hps |= set(hub[2])
    nine = {(1, 1), (2, 1), (4, 1), (8, 1), (16, 1), (32, 1), (32, 2), (64, 2), (64, 4)}
    assert {s for xv, s in shapes if xv == 8} == nine
    for xv in (4, 2, 1):
        assert {(32, 2), (64, 2), (64, 4)} <= {s for v, s in shapes if v == xv}, xv
    assert {f for f, _ in hubs} == {32, 64} and {t for _, t in hubs} == set(B.TILES)
    assert {(8, fsp, w, s) for fsp in (32, 64) for w in (False, True) for s in (False, True)} <= flags
    assert all(any(f[0] == xv and f[2] and f[3] for f in flags) for xv in (4, 2, 1))
    assert {1, 2, 3} <= n_ranges and hps == {1, 2, 3, 4} and fallback == {"f32_h8", "f128_h32"}
    on_hubs = [c for c in CASES if c.accum and c.x == "bf16"]
    assert any(c.dst for c in on_hubs) and any(not c.dst and not c.deg for c in on_hubs)
    assert {c.y2 for c in on_hubs if c.deg} == {"f32", "bf16"}
    # fp32 X with a bf16 out2 past one range: with the fp32 hub kernel, and with it switched off
    f32x = {c.id: branches(c, True)[1] for c in CASES if c.x == "f32"}
    assert len(f32x["f32x_y2b_264"]) == 2 and all(h == (fsp, None, ()) for (_, _, h), fsp in zip(f32x["f32x_y2b_264"], (64, 32)))
    assert all(h is None for _, _, h in f32x["f32x_y2b_264_h4"])
    # weighted heads across a range boundary: the second range starts inside the last head
    w = BY_ID["w264h4_xv1"]
    assert (B.MAX_VECS * 1) // (w.F // w.heads) == w.heads - 1 and BY_ID["w264h4_xv1_rs"].rs
