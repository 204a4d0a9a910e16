"""CPU: the mirror on host tensors has no row-width limit (the HIP backend's is not applied to them): a FIXED
layer of 8 x 64 on two patterns trains; float64 autograd reference, tolerances of test_gpu_torch_ext."""
import numpy as np
import torch

from gala import layout
from _graphs import features, with_empty_rows


def test_fixed_layer_of_512_floats_trains_on_host_tensors():
    import gala
    E, g, H, D = gala.torch_ext(), with_empty_rows(), 8, 64
    t, perm = layout.transpose(g)
    E.slots_clear()
    for s in (g, t):
        E.slots_push(torch.from_numpy(s.rowptr), torch.from_numpy(s.col), torch.ones(s.nnz), None, 1, False)
    E.slots_set_transpose_perm(1, torch.from_numpy(perm))
    N, w = g.n_rows, torch.linspace(-1, 1, H * D)
    ins = [torch.from_numpy(features(N, f, seed=s)) for f, s in ((H, 1), (H, 2), (H * D, 3))]
    got = [a.clone().requires_grad_() for a in ins]
    Y = E.gat_aggregate_apply(*got, 0, 0.2, 1)
    (Y * w).sum().backward()
    E.slots_clear()
    r = torch.from_numpy(np.repeat(np.arange(N), np.diff(g.rowptr))).long()
    c = torch.from_numpy(g.col.astype(np.int64))
    l64, r64, x64 = ref = [a.double().requires_grad_() for a in ins]
    z = torch.nn.functional.leaky_relu(l64[r] + r64[c], 0.2)
    p = torch.exp(z - torch.full((N, H), -torch.inf).double().scatter_reduce(0, r[:, None].expand(-1, H), z, "amax")[r])
    alpha = p / torch.zeros(N, H).double().index_add(0, r, p)[r]
    Y64 = torch.zeros(N, H, D).double().index_add(0, r, alpha[:, :, None] * x64[c].view(-1, H, D)).view(N, H * D)
    (Y64 * w.double()).sum().backward()
    np.testing.assert_allclose(Y.detach().numpy(), Y64.detach().numpy(), atol=1e-4, rtol=1e-4)
    for a, b, rtol in zip(got, ref, (1e-3, 1e-3, 1e-4)):
        np.testing.assert_allclose(a.grad.numpy(), b.grad.numpy(), atol=1e-4, rtol=rtol)
