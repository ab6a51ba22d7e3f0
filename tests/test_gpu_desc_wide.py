"""htf.DescriptorMLP(conservative=True, dense="mfma") on the MI355X (csrc/cfwide.hip, include/htf_cfwide.h): the first sweep of
the conservative forces with the dense stack on the fp32 matrix instruction, hidden layers up to 256 wide, against the
references of test_gpu_desc_total.py -- the fp64 autograd oracle of the definition and the fp64 formula of include/htf_cforce.h.
Systems, shapes and the bias trick are that file's.

Bound: TOL = 2e-5 of the largest reference value while max(H1, H2) <= 64; above, TOL sqrt(max(H1, H2) / 64): the rounding
error of an fp32 chain grows with the square root of its length, and 64 is the length TOL was set for.

Largest error / largest reference value measured per case of test_wide_values, in CASES' order (forces, energy), units of 1e-6:
(1.1, 0.9) (2.6, 0.8) (1.7, 1.4) (0.6, 0.4) (2.6, 0.3) (2.0, 1.3) (0.6, 0.4) (3.0, 2.0) (1.7, 0.7) (0.6, 0.3) (14.7, 0.2) (2.9, 1.5).
The eleventh is the 1 x 1 tanh network on the small system, whose largest force is 0.015: the error there is 2.3e-7 absolute."""
import math

import numpy as np
import pytest
import torch

from test_gpu_desc_total import TOL, _close, _system, formula, oracle

pytestmark = pytest.mark.gpu


def _wide(htf, H1, H2, K=16, n_types=1, activation="tanh", high=1.8, r_cut=None, n_species=1, seed=3, dense="mfma", bias=0.1):
    """test_gpu_desc_total._layer with the widths and ``dense``: mlp_params' zero biases replaced."""
    lay = htf.DescriptorMLP(K=K, H1=H1, H2=H2, low=0.5, high=high, n_types=n_types, activation=activation, seed=seed,
                            r_cut=r_cut, n_species=n_species, conservative=True, dense=dense)
    rng = np.random.default_rng(seed + 100)
    ws = lay.get_weights()
    for i in (1, 3, 5):
        ws[i] = (bias * rng.standard_normal(ws[i].shape)).astype(np.float32)
    lay.set_weights(ws)
    return lay


def _bound(H1, H2):
    return TOL * math.sqrt(max(H1, H2, 64) / 64.0)


# (H1, H2, config, K, n_types, cut, activation, dtype): every width pair on both systems' slot counts between them; D = 16,
# 21 (odd) and 64; both activations, cutoffs and dtypes at the top width
CASES = [
    (256, 256, "b256", 16, 4, True, "tanh", torch.float32),
    (256, 256, "a", 16, 1, False, "linear", torch.float64),
    (256, 256, "a", 7, 3, True, "tanh", torch.float64),
    (65, 33, "a", 7, 3, False, "tanh", torch.float32),
    (65, 33, "b256", 16, 1, True, "linear", torch.float64),
    (96, 160, "a", 16, 4, True, "tanh", torch.float32),
    (96, 160, "b256", 7, 3, False, "linear", torch.float32),
    (32, 24, "a", 16, 1, True, "tanh", torch.float64),
    (32, 24, "b256", 16, 4, False, "tanh", torch.float32),
    (1, 1, "a", 7, 3, True, "linear", torch.float32),
    (1, 1, "a", 16, 1, False, "tanh", torch.float64),
    (160, 96, "a", 16, 1, True, "tanh", torch.float32),
]


@pytest.mark.parametrize("H1,H2,config,K,n_types,cut,activation,dtype", CASES)
def test_wide_values(htf, cuda, H1, H2, config, K, n_types, cut, activation, dtype):
    p, L, rc_list, x, idx = _system(config)
    assert len(p) % 32 and len(p) % 64   # the last tile is ragged
    lay = _wide(htf, H1, H2, K=K, n_types=n_types, activation=activation, high=rc_list, r_cut=0.9 * rc_list if cut else None,
                seed=5 + n_types)
    nl = htf.Nlist(x.to(dtype), index=idx)
    f = htf.compute_nlist_forces(nl, lay(nl, p.to(dtype)))
    assert f.dtype == dtype and f.shape == (len(p), 4)
    F, E = oracle(lay, p, L, x, idx)
    assert F.abs().max().item() > 0
    _close(f[:, :3], F, "forces", tol=_bound(H1, H2))
    _close(f[:, 3], E, "energy", tol=_bound(H1, H2))


@pytest.mark.parametrize("config,n_types", [("a", 3), ("b256", 1)])
def test_wide_agrees_with_lanes(htf, cuda, config, n_types):
    """The same weights on both dense stacks at a width both take: equal within TOL, and the table pass 2 reads likewise."""
    p, L, rc_list, x, idx = _system(config)
    kw = dict(K=16, n_types=n_types, high=rc_list, r_cut=0.9 * rc_list, seed=9)
    wide, lanes = _wide(htf, 32, 24, **kw), _wide(htf, 32, 24, dense="lanes", **kw)
    assert torch.equal(wide.w, lanes.w)
    types = p[:, 3].contiguous()
    a, b = wide.total_forces(x, idx, types=types), lanes.total_forces(x, idx, types=types)
    _close(a[:, :3], b[:, :3], "forces")
    _close(a[:, 3], b[:, 3], "energy")


@pytest.mark.parametrize("S", [2, 3])
def test_wide_one_network_per_species(htf, cuda, S):
    """A species absent from the batch: one launch per species present, each over its row list.  S = 2: every row is species 1;
    S = 3: species 0 and 2 interleaved, a tile's rows scattered through the list."""
    p, L, rc_list, x, idx = _system("a")
    lay = _wide(htf, 96, 160, K=20, n_types=2, high=rc_list, r_cut=0.9 * rc_list, n_species=S, seed=11)
    sp = torch.ones_like(p[:, 3].long()) if S == 2 else (p[:, 3].long() % 2) * 2
    assert 0 in lay.species_counts(sp.to(torch.float32), x)
    f = lay.total_forces(x, idx, types=p[:, 3].contiguous(), species=sp.to(torch.float32))
    F, E = oracle(lay, p, L, x, idx, sp=sp)
    _close(f[:, :3], F, "forces", tol=_bound(96, 160))
    _close(f[:, 3], E, "energy", tol=_bound(96, 160))


def test_wide_virial(htf, cuda):
    p, L, rc_list, x, idx = _system("a")
    lay = _wide(htf, 96, 160, K=16, n_types=3, high=rc_list, r_cut=0.9 * rc_list, seed=31)
    nl = htf.Nlist(x, index=idx)
    f, w = htf.compute_nlist_forces(nl, lay(nl, p.to(x.dtype)), virial=True)
    F, E, W, _, _ = formula(lay, x, idx, p[:, 3].long())
    _close(f[:, :3], F, "forces", tol=_bound(96, 160))
    _close(w, W, "virial", tol=_bound(96, 160))


def test_wide_zero_rows(htf, cuda):
    lay = _wide(htf, 128, 128, K=8, n_types=2)
    x = torch.zeros((0, 32, 4), device=cuda)
    f = lay.total_forces(x, torch.zeros((0, 32), dtype=torch.int32, device=cuda), types=torch.zeros((0,), device=cuda))
    assert f.shape == (0, 4)
