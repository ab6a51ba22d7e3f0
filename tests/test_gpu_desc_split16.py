"""htf.DescriptorMLP(conservative=True, dense="split16") on the MI355X (csrc/cfwide16.hip, include/htf_cfwide16.h): the first sweep
of the conservative forces with the dense stack on the fp16 matrix instruction, operands split as hi + lo, against the
references of test_gpu_desc_total.py.  Cases, layers and the bound -- the fp32 stack's own, TOL sqrt(max(H1, H2, 64) / 64) --
are test_gpu_desc_wide.py's: split16 is held to the tolerance of the fp32 path.

Largest error / largest reference value measured per case of test_split16_values, in CASES' order (forces, energy), units of
1e-6: (1.0, 0.9) (2.5, 0.8) (1.4, 1.2) (0.9, 0.5) (2.5, 0.2) (1.6, 1.0) (0.5, 0.5) (3.1, 1.4) (1.9, 1.0) (0.5, 0.2) (4.3, 0.2)
(2.9, 2.1).  e16 / e32 of test_split16_error_of_the_fp32_stacks_size (forces, energy): 256 x 256 (0.89, 1.07), 96 x 160 (0.83,
0.79), 32 x 24 (1.11, 1.51)."""
import numpy as np
import pytest
import torch

from test_gpu_desc_total import _close, _system, formula, oracle
from test_gpu_desc_wide import CASES, _bound, _wide

pytestmark = pytest.mark.gpu

def _case(htf, case, dense):
    """(the layer, its forces [N, 4] through compute_nlist_forces, the oracle's arguments) of a test_gpu_desc_wide case."""
    H1, H2, config, K, n_types, cut, activation, dtype = case
    p, L, rc_list, x, idx = _system(config)
    assert len(p) % 32 and len(p) % 64   # the last tile is ragged
    lay = _wide(htf, H1, H2, K=K, n_types=n_types, activation=activation, high=rc_list, r_cut=0.9 * rc_list if cut else None,
                seed=5 + n_types, dense=dense)
    nl = htf.Nlist(x.to(dtype), index=idx)
    f = htf.compute_nlist_forces(nl, lay(nl, p.to(dtype)))
    assert f.dtype == dtype and f.shape == (len(p), 4)
    return lay, f, (p, L, x, idx)


def _rel(got, ref):
    return (got.double() - ref).abs().max().item() / ref.abs().max().item()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-%s-D%d-%s" % (c[0], c[1], c[2], c[3] * c[4], c[6]))
def test_split16_values(htf, cuda, case):
    lay, f, system = _case(htf, case, "split16")
    F, E = oracle(lay, *system)
    assert F.abs().max().item() > 0
    _close(f[:, :3], F, "forces", tol=_bound(*case[:2]))
    _close(f[:, 3], E, "energy", tol=_bound(*case[:2]))


@pytest.mark.parametrize("case", [CASES[0], CASES[5], CASES[8]], ids=["256x256", "96x160", "32x24"])
def test_split16_error_of_the_fp32_stacks_size(htf, cuda, case):
    """test_pair_mlp_split_operands' gate on the same weights: e16 <= 4 e32 + 1e-7 of the largest reference value."""
    (lay, f16, system), (lay32, f32, _) = _case(htf, case, "split16"), _case(htf, case, "mfma")
    assert torch.equal(lay.w, lay32.w)
    F, E = oracle(lay, *system)
    for what, c, ref in (("forces", slice(0, 3), F), ("energy", 3, E)):
        e16, e32 = _rel(f16[:, c], ref), _rel(f32[:, c], ref)
        assert e16 <= 4.0 * e32 + 1e-7, (what, e16, e32)


@pytest.mark.parametrize("S", [2, 3])
def test_split16_one_network_per_species(htf, cuda, S):
    """test_gpu_desc_wide's: a species absent from the batch, S = 3 with a tile's rows scattered through the list."""
    p, L, rc_list, x, idx = _system("a")
    lay = _wide(htf, 96, 160, K=20, n_types=2, high=rc_list, r_cut=0.9 * rc_list, n_species=S, seed=11, dense="split16")
    sp = torch.ones_like(p[:, 3].long()) if S == 2 else (p[:, 3].long() % 2) * 2
    assert 0 in lay.species_counts(sp.to(torch.float32), x)
    f = lay.total_forces(x, idx, types=p[:, 3].contiguous(), species=sp.to(torch.float32))
    F, E = oracle(lay, p, L, x, idx, sp=sp)
    _close(f[:, :3], F, "forces", tol=_bound(96, 160))
    _close(f[:, 3], E, "energy", tol=_bound(96, 160))


def test_split16_virial_zero_rows_and_equal_bits(htf, cuda):
    p, L, rc_list, x, idx = _system("a")
    lay = _wide(htf, 96, 160, K=16, n_types=3, high=rc_list, r_cut=0.9 * rc_list, seed=31, dense="split16")
    nl = htf.Nlist(x, index=idx)
    f, w = htf.compute_nlist_forces(nl, lay(nl, p.to(x.dtype)), virial=True)
    F, E, W, _, _ = formula(lay, x, idx, p[:, 3].long())
    _close(f[:, :3], F, "forces", tol=_bound(96, 160))
    _close(w, W, "virial", tol=_bound(96, 160))
    x0 = torch.zeros((0, 32, 4), device=cuda)
    f0 = lay.total_forces(x0, torch.zeros((0, 32), dtype=torch.int32, device=cuda), types=torch.zeros((0,), device=cuda))
    assert f0.shape == (0, 4)
    big = _wide(htf, 256, 256, K=16, n_types=3, high=rc_list, seed=7, dense="split16")
    types = p[:, 3].contiguous()
    assert torch.equal(big.total_forces(x, idx, types=types), big.total_forces(x, idx, types=types))


def test_split16_out_of_range_is_not_finite(htf, cuda):
    """activation="linear" with W1 scaled until about half the rows have a hidden value beyond fp16's largest number, 65504:
    those rows' energies are NaN or infinite, and every finite energy is the oracle's within the bound.  (g does not depend on
    h1 when the activation is linear, so the forces stay finite and right.)"""
    p, L, rc_list, x, idx = _system("a")
    lay = _wide(htf, 96, 160, K=16, n_types=3, activation="linear", high=rc_list, r_cut=0.9 * rc_list, seed=13, dense="split16")
    ws = lay.get_weights()
    G = lay.descriptor(htf.Nlist(x)).double().cpu().numpy()
    ws[0] = (ws[0] * np.float32(65504.0 / np.median(np.abs(G @ ws[0].astype(np.float64)).max(axis=1)))).astype(np.float32)
    lay.set_weights(ws)
    z1 = np.abs(G @ ws[0].astype(np.float64) + ws[1]).max(axis=1)
    over, safe = torch.as_tensor(z1 > 65600.0, device=cuda), torch.as_tensor(z1 < 65400.0, device=cuda)
    assert over.sum() >= 8 and safe.sum() >= 8 and np.abs(ws[0]).max() < 65504.0
    f = lay.total_forces(x, idx, types=p[:, 3].contiguous())
    F, E = oracle(lay, p, L, x, idx)
    fin = torch.isfinite(f[:, 3])
    assert not fin[over].any() and fin[safe].all()
    _close(f[fin, 3], E[fin], "finite energies", tol=_bound(96, 160), scale=E.abs().max().item())
    _close(f[:, :3], F, "forces", tol=_bound(96, 160))


@pytest.mark.parametrize("which,value", [(0, 1.0e5), (2, float("nan"))], ids=["W1-above-fp16", "W2-nan"])
def test_split16_bad_weight_is_not_finite_with_tanh(htf, cuda, which, value):
    """One weight beyond fp16's range, or NaN, under tanh: its products are NaN in every row of its hidden unit, and the
    activation must hand that on -- every energy is non-finite, none saturates to a finite value."""
    p, L, rc_list, x, idx = _system("a")
    lay = _wide(htf, 96, 160, K=16, n_types=3, high=rc_list, r_cut=0.9 * rc_list, seed=13, dense="split16")
    ws = lay.get_weights()
    ws[which][3, 5] = value
    lay.set_weights(ws)
    f = lay.total_forces(x, idx, types=p[:, 3].contiguous())
    assert not torch.isfinite(f[:, 3]).any()
