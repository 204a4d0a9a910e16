"""CPU (host backend, gloo): gala.dist.HaloGatExact over a communicator, world 1, 2 and 3.

Each rank runs the layer on its rows of gala.dist.partition_graph (p2p or the dense table); the
gathered outputs equal the one-process helper of tests/_gat_exact_rect.py on the same bounds bit
for bit (which tests/test_gat_exact_rect_cpu.py shows equal to the square pair), hub rows of the
whole graph's plan included.  With the source logit's Linear (aR recomputed) dX also carries
d_aR wR, and (dwR, dbR), summed over the ranks, match the one-process gradients of d_aR.
halo_bytes() is the formula part.halo_bytes(2F + H + 4H): derived, not measured."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import _gat_exact_rect as R
import _gat_exact_ref as X
from gala import dist as gdist
from gala.backend import CpuBackend
from gala.comm import Comm
from test_dist_partition_cpu import _free_port

# (world, graph, shape of R.SHAPES, halo mode)
CASES = ((1, "cora", 0, "p2p"), (2, "hub", 3, "p2p"), (3, "hub", 0, "dense"), (3, "cora", 3, "p2p"),
         (2, "long", 1, "dense"))


def _inputs(name, shape):
    H, F, rc, big = R.SHAPES[shape]
    return X.inputs(X.graph(name), H, F, rc, big)


def _worker(rank, world, port, name, shape, halo_mode, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        g = X.graph(name)
        i = _inputs(name, shape)
        pt = gdist.partition_graph(g, rank, world, halo_mode=halo_mode)
        own = slice(pt.r0, pt.r0 + pt.n)
        gat = gdist.HaloGatExact(pt, i.F, i.heads, CpuBackend(), Comm(), slope=X.SLOPE, symmetric=True)
        t = lambda a: torch.from_numpy(a[own].copy())  # noqa: E731
        grads = []
        if i.rc:
            Y = gat.forward_train(t(i.aL), None, t(i.X), torch.from_numpy(i.wR), torch.from_numpy(i.bR))
            dX, daL, daR, dW, db = gat.backward(t(i.dY))
            for G in (dW, db):
                dist.all_reduce(G)
                grads.append(G.numpy().copy())
        else:
            Y = gat.forward_train(t(i.aL), t(i.aR), t(i.X))
            dX, daL, daR = gat.backward(t(i.dY))
        sizes = [int(pt.bounds[r + 1] - pt.bounds[r]) for r in range(world)]
        out = []
        for T in (Y, dX, daL, daR):
            pad = torch.full((max(sizes), T.shape[1]), float("nan"))
            pad[:pt.n] = T
            ts = [torch.empty_like(pad) for _ in sizes]
            dist.all_gather(ts, pad)
            out.append(torch.cat([x[:s] for x, s in zip(ts, sizes)]).numpy())
        hb = torch.tensor([float(gat.halo_bytes()), float(pt.halo_bytes(2 * i.F + 5 * i.heads))], dtype=torch.float64)
        hbs = [torch.empty_like(hb) for _ in sizes]
        dist.all_gather(hbs, hb)
        if rank == 0:
            q.put(out + [torch.stack(hbs).numpy(), pt.bounds.copy()] + grads)
        dist.barrier()      # every rank tears down together (gloo)
    finally:
        dist.destroy_process_group()
    q.close()
    q.join_thread()
    os._exit(0)   # skip library destructors: a gloo rank can abort in one at interpreter exit


@pytest.mark.parametrize("world,name,shape,halo_mode", CASES)
def test_halo_gat_exact_bit_identical_to_one_process(world, name, shape, halo_mode):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, name, shape, halo_mode, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    Y, dX, daL, daR, hb, bounds = got[:6]
    g = X.graph(name)
    i = _inputs(name, shape)
    be = CpuBackend()
    thr = gdist.partition_graph(g, 0, world, halo_mode="p2p").split_threshold
    want, _ = R.rect_layer(be, name, tuple(int(b) for b in bounds), i, plan=(thr, 512))
    if name != "cora":
        assert (thr, 512) == X.PLAN and (np.diff(g.rowptr) > thr).sum() >= 4
    np.testing.assert_array_equal(Y, want["Y"])
    np.testing.assert_array_equal(daL, want["daL"])
    np.testing.assert_array_equal(daR, want["daR"])
    if i.rc:     # the Linear's share of dX, by the same call on the whole graph's rows
        full = torch.from_numpy(want["dX"].copy())
        be.head_attn_bwd(torch.from_numpy(want["daR"].copy()), torch.from_numpy(i.wR), i.heads, full)
        np.testing.assert_array_equal(dX, full.numpy())
        dW, db = be.head_linear_grads(torch.from_numpy(i.X), torch.from_numpy(want["daR"].copy()), i.heads)
        # sums over the ranks in another order than over all rows: fp32 rounding of n-term sums
        np.testing.assert_allclose(got[6], dW.numpy(), rtol=1e-4, atol=1e-4 * np.abs(dW.numpy()).max())
        np.testing.assert_allclose(got[7], db.numpy(), rtol=1e-4, atol=1e-4 * np.abs(db.numpy()).max())
    else:
        np.testing.assert_array_equal(dX, want["dX"])
    # halo_bytes(): the formula on every rank, nothing at world 1
    np.testing.assert_array_equal(hb[:, 0], hb[:, 1] if world > 1 else np.zeros(world))
    assert world == 1 or hb[:, 0].sum() > 0
