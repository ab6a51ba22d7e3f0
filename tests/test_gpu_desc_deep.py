"""htf.DescriptorMLP(conservative=True, dense="mfma", H3=...) on the MI355X (csrc/cfwide3.hip, include/htf_cfwide3.h): the first
sweep of the conservative forces for three hidden layers on the fp32 matrix instruction, against fp64 torch autograd of

    E_i = W4^T act(W3^T act(W2^T act(W1^T G_i + b1) + b2) + b3) + b4,   F = -grad(sum_i E_i, pos)

with test_gpu_desc_total.py's descriptor, systems and bias trick (b4 included).

Bound: test_gpu_desc_wide.py's rule, TOL sqrt(max(H1, H2, H3, 64) / 64) with TOL = 2e-5 of the largest reference value.

Largest error / largest reference value measured per case of test_deep_values, in CASES' order (forces, energy), units of 1e-6:
(1.7, 0.7) (1.9, 1.3) (3.0, 0.7) (0.8, 0.8) (2.4, 7.2) (1.0, 0.5) (2.8, 1.8) (1.3, 1.0) (0.5, 0.2) (14.7, 0.2) (1.9, 1.1) (1.7, 1.0)
(1.5, 0.8); species (1.4, 2.0); virial test (1.9 forces, 1.1 virial).  The tenth is the 1 x 1 x 1 tanh network, whose largest force
is 0.008: the error there is 1.2e-7 absolute."""
import math

import numpy as np
import pytest
import torch

from test_gpu_desc_total import TOL, _close, _descriptor, _neighbor_types, _pair_vectors, _system

pytestmark = pytest.mark.gpu


def _deep(htf, H1, H2, H3, K=16, n_types=1, activation="tanh", high=1.8, r_cut=None, n_species=1, seed=3, bias=0.1):
    """test_gpu_desc_wide._wide with the third width: mlp_params' zero biases replaced, b4 too."""
    lay = htf.DescriptorMLP(K=K, H1=H1, H2=H2, H3=H3, low=0.5, high=high, n_types=n_types, activation=activation, seed=seed,
                            r_cut=r_cut, n_species=n_species, conservative=True, dense="mfma")
    rng = np.random.default_rng(seed + 100)
    ws = lay.get_weights()
    for i in (1, 3, 5, 7):
        ws[i] = (bias * rng.standard_normal(ws[i].shape)).astype(np.float32)
    lay.set_weights(ws)
    return lay


def _network(lay, G, sp):
    W = [torch.as_tensor(np.asarray(w, dtype=np.float64), device=G.device) for w in lay.get_weights()]
    W = W if lay.n_species > 1 else [w[None] for w in W]
    act = torch.tanh if lay.activation == "tanh" else (lambda v: v)
    h = G
    for i in (0, 2, 4):
        h = act(torch.einsum("bd,bdh->bh", h, W[i][sp]) + W[i + 1][sp])
    return torch.einsum("bd,bdh->bh", h, W[6][sp])[:, 0] + W[7][sp][:, 0]


def _oracle(lay, pos, L, x, idx, sp=None):
    """Autograd of the definition: (F [N, 3] = -grad(sum E, pos), E [N])."""
    occ = (x[:, :, :3] != 0).any(dim=2)
    sp = torch.zeros(len(pos), dtype=torch.long, device=pos.device) if sp is None else sp
    q = pos[:, :3].detach().clone().requires_grad_(True)
    E = _network(lay, _descriptor(lay, _pair_vectors(q, idx, occ, L), _neighbor_types(lay, x))[0], sp)
    (g,) = torch.autograd.grad(E.sum(), q)
    return -g, E.detach()


def _bound(*widths):
    return TOL * math.sqrt(max(widths + (64,)) / 64.0)


# (H1, H2, H3, config, K, n_types, cut, activation, dtype).  The tile: 32 rows at 256^3, 240^3 and 256 x 224 x 160 (640 image
# lines), 64 rows at all others; 256 x 256 x 96 (608 lines) is the widest the 64-row tile takes.  D = 16, 21 and 64.
CASES = [
    (256, 256, 256, "b256", 16, 4, True, "tanh", torch.float32),
    (256, 256, 256, "a", 7, 3, False, "linear", torch.float64),
    (240, 240, 240, "a", 16, 1, True, "tanh", torch.float64),
    (65, 33, 97, "a", 7, 3, False, "tanh", torch.float32),
    (65, 33, 97, "b256", 16, 1, True, "linear", torch.float64),
    (160, 128, 96, "b256", 16, 4, False, "tanh", torch.float32),
    (32, 24, 16, "a", 16, 1, True, "tanh", torch.float64),
    (32, 24, 16, "b256", 7, 3, False, "linear", torch.float32),
    (1, 1, 1, "a", 7, 3, True, "linear", torch.float32),
    (1, 1, 1, "a", 16, 1, False, "tanh", torch.float64),
    (8, 256, 8, "a", 16, 4, True, "tanh", torch.float32),
    (256, 256, 96, "a", 16, 4, False, "tanh", torch.float32),
    (256, 224, 160, "a", 7, 3, True, "tanh", torch.float32),
]


@pytest.mark.parametrize("H1,H2,H3,config,K,n_types,cut,activation,dtype", CASES)
def test_deep_values(htf, cuda, H1, H2, H3, config, K, n_types, cut, activation, dtype):
    p, L, rc_list, x, idx = _system(config)
    assert len(p) % 32 and len(p) % 64   # the last tile is ragged
    lay = _deep(htf, H1, H2, H3, K=K, n_types=n_types, activation=activation, high=rc_list, r_cut=0.9 * rc_list if cut else None,
                seed=5 + n_types)
    nl = htf.Nlist(x.to(dtype), index=idx)
    f = htf.compute_nlist_forces(nl, lay(nl, p.to(dtype)))
    assert f.dtype == dtype and f.shape == (len(p), 4)
    F, E = _oracle(lay, p, L, x, idx)
    assert F.abs().max().item() > 0
    _close(f[:, :3], F, "forces", tol=_bound(H1, H2, H3))
    _close(f[:, 3], E, "energy", tol=_bound(H1, H2, H3))


def test_deep_one_network_per_species(htf, cuda):
    """S = 3 with species 1 absent: one launch per species present, species 0 and 2 interleaved through the row lists."""
    p, L, rc_list, x, idx = _system("a")
    lay = _deep(htf, 96, 160, 40, K=20, n_types=2, high=rc_list, r_cut=0.9 * rc_list, n_species=3, seed=11)
    sp = (p[:, 3].long() % 2) * 2
    assert lay.species_counts(sp.to(torch.float32), x)[1] == 0
    f = lay.total_forces(x, idx, types=p[:, 3].contiguous(), species=sp.to(torch.float32))
    F, E = _oracle(lay, p, L, x, idx, sp=sp)
    _close(f[:, :3], F, "forces", tol=_bound(96, 160, 40))
    _close(f[:, 3], E, "energy", tol=_bound(96, 160, 40))


def test_deep_virial(htf, cuda):
    """Pass 2's second consumer of the g table: W_i = -1/2 sum_s x (outer) phi, phi by include/htf_cforce.h's formula in fp64 with
    g from autograd of the three-layer network with respect to G (every type and index of system "a" is in range)."""
    p, L, rc_list, x, idx = _system("a")
    lay = _deep(htf, 96, 160, 40, K=16, n_types=3, high=rc_list, r_cut=0.9 * rc_list, seed=31)
    nl = htf.Nlist(x, index=idx)
    f, w = htf.compute_nlist_forces(nl, lay(nl, p.to(x.dtype)), virial=True)
    B, x3, tn, ti = len(p), x[:, :, :3].double(), _neighbor_types(lay, x).long(), p[:, 3].long()
    G, r, live, fc, dfc = _descriptor(lay, x3, tn)
    G = G.detach().requires_grad_(True)
    (g,) = torch.autograd.grad(_network(lay, G, torch.zeros(B, dtype=torch.long, device=x.device)).sum(), G)
    g = g.view(B, lay.n_types, lay.K)
    s = g[torch.arange(B, device=x.device)[:, None], tn] + g[idx.long().clamp(0, B - 1), ti[:, None]]
    d = r[..., None] - torch.as_tensor(lay.centers.astype(np.float64), device=x.device)
    ek = torch.exp(-d * d / float(lay.gap))
    dEdr = fc * (-2.0 / float(lay.gap)) * (s * d * ek).sum(dim=-1) + dfc * (s * ek).sum(dim=-1)
    phi = (dEdr / r * live.to(r.dtype))[..., None] * (x3 + 1e-7)
    _close(f[:, :3], phi.sum(dim=1), "forces", tol=_bound(96, 160, 40))
    _close(w, -0.5 * torch.einsum("bsi,bsj->bij", x3, phi), "virial", tol=_bound(96, 160, 40))


def test_deep_zero_rows(htf, cuda):
    lay = _deep(htf, 128, 128, 128, K=8, n_types=2)
    x = torch.zeros((0, 32, 4), device=cuda)
    f = lay.total_forces(x, torch.zeros((0, 32), dtype=torch.int32, device=cuda), types=torch.zeros((0,), device=cuda))
    assert f.shape == (0, 4)
