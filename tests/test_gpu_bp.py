"""htf.DescriptorMLP(r_cut=..., n_species=...) on the MI355X (csrc/bp.hip over desc_row.h and dtrain_row.h).

The cutoff is checked against fp64 torch autograd of the definition, the reference() of tests/test_gpu_desc.py and the
double backward of tests/test_gpu_desc_train.py with fc multiplied in:

    fc(r) = 0.5 (cos(pi r / rc) + 1) for r < rc, 0 beyond;   G_i[t*K + k] = sum_j live_ij [t_ij = t] fc(r_ij) exp(-(r_ij - mu_k)^2 / gap)

at those files' bounds (2e-5 of the largest reference value; 2e-4 of the largest gradient entry).  The row list and the
species are checked bit for bit against a layer of one network on the same rows (include/htf_bp.h, contracts (b) and (c))."""
import math

import numpy as np
import pytest
import torch

from helpers import random_nlist
from test_gpu_desc import TOL, _close
from test_gpu_desc_train import TOL as GTOL, _blocks

pytestmark = pytest.mark.gpu


def _layer(htf, K=16, n_types=1, H1=32, H2=32, activation="tanh", low=0.0, high=3.0, seed=3, bias=0.1, **kw):
    lay = htf.DescriptorMLP(K=K, H1=H1, H2=H2, low=low, high=high, n_types=n_types, activation=activation, seed=seed, **kw)
    if bias:   # (mlp_params' zero biases would leave the bias paths untested)
        rng = np.random.default_rng(seed + 100)
        ws = lay.get_weights()
        for i in (1, 3, 5):
            ws[i] = (bias * rng.standard_normal(ws[i].shape)).astype(np.float32)
        lay.set_weights(ws)
    return lay


def _single(htf, lay, s):
    """A layer of one network holding network ``s`` of ``lay``, everything else alike."""
    cfg = lay.get_config()
    cfg.pop("n_species", None)
    one = htf.DescriptorMLP(**cfg)
    with torch.no_grad():
        one.w.copy_(lay.w[s * lay.P:(s + 1) * lay.P])
    return one


def _fc(r, rc):
    return torch.where(r < rc, 0.5 * (torch.cos(math.pi * r / rc) + 1.0), torch.zeros_like(r))


def net(lay, W, x, create_graph=False):
    """The layer's definition in plain torch, in the dtype of ``x`` and ``W`` (the six Keras arrays of ONE network),
    differentiable in ``W``: (pred [B, 4] = (2 sum_j dE_i/dx_ij, E_i), G [B, D], the pair gradient 2 dE/dx [B, NN, 3])."""
    mu = torch.as_tensor(lay.centers, dtype=x.dtype, device=x.device)
    act = torch.tanh if lay.activation == "tanh" else (lambda v: v)
    xx = x.detach().clone().requires_grad_(True)
    t = xx[:, :, :3] + 1e-7
    r = torch.sqrt((t * t).sum(dim=2))
    live = r > 3e-6
    typ = torch.zeros_like(r) if lay.n_types == 1 else torch.round(xx[:, :, 3].detach())
    e = torch.exp(-(r[..., None] - mu) ** 2 / float(lay.gap))
    if lay.r_cut is not None:
        e = e * _fc(r, float(lay.r_cut))[..., None]
    G = torch.cat([(e * (live & (typ == tt)).to(x.dtype)[..., None]).sum(dim=1) for tt in range(lay.n_types)], dim=1)
    h1 = act(G @ W[0] + W[1])
    h2 = act(h1 @ W[2] + W[3])
    E = (h2 @ W[4] + W[5])[:, 0]
    (g,) = torch.autograd.grad(E.sum(), xx, create_graph=create_graph)
    nf = 2.0 * g[:, :, :3]
    return torch.cat([nf.sum(dim=1), E[:, None]], dim=1), G, nf


def reference(lay, x):
    """fp64 autograd of the definition with the cutoff: (F [B, 3], E [B], G [B, D], V [B, 3, 3]), the virial by the generic
    route's formula as tests/test_gpu_desc.py states it."""
    W = [torch.as_tensor(np.asarray(w, dtype=np.float64), device=x.device) for w in lay.get_weights()]
    x64 = x.detach().to(torch.float64)
    pred, G, nf = net(lay, W, x64)
    n3 = x64[:, :, :3]
    rmag = torch.sqrt((n3 * n3).sum(dim=2))
    fmag = torch.sqrt((nf * nf).sum(dim=2))
    den = 2.0 * rmag
    frs = torch.where(den == 0, torch.zeros_like(den), fmag / den)
    V = -1.0 * torch.einsum("ij,ijk,ijl->ikl", frs, n3, n3)
    return pred[:, :3].detach(), pred[:, 3].detach(), G.detach(), V.detach()


def _err(got, ref):
    return (got.double() - ref.double()).abs().max().item() / ref.double().abs().max().item()


def _rows_around(rng, B, NN, rc, n_types):
    """Random rows with live distances in [0.3 rc, 1.15 rc]; slots 0 and 1 of every row are moved to 0.6 rc and 1.1 rc, so
    that every row has neighbors on both sides of rc whatever was drawn."""
    nl, cnt = random_nlist(rng, B, NN, fill=0.75, rmin=0.3 * rc, rmax=1.15 * rc, ntypes=n_types, dtype=np.float64)
    assert cnt.min() >= 2
    for slot, r in ((0, 0.6 * rc), (1, 1.1 * rc)):
        nl[:, slot, :3] *= r / np.linalg.norm(nl[:, slot, :3], axis=1, keepdims=True)
    return nl


# ------------------------------------------------------------------------------------------------ 1. the cutoff against its definition
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("NN", [37, 128, 256])
@pytest.mark.parametrize("activation", ["tanh", "linear"])
@pytest.mark.parametrize("n_types", [1, 3])
def test_cutoff_forces_energy_virial_descriptor(htf, cuda, n_types, activation, NN, dtype):
    rc = 2.75
    rng = np.random.default_rng(7 + NN + 3 * n_types)
    # live distances on both sides of rc in every row
    x = torch.from_numpy(_rows_around(rng, 300, NN, rc, n_types)).to(dtype).to(cuda)
    r = torch.linalg.norm(x[:, :, :3].double(), dim=2)
    assert ((r > 0) & (r < rc)).any(dim=1).all() and (r > rc).any(dim=1).all()
    lay = _layer(htf, K=32 if n_types == 1 else 16, n_types=n_types, H1=64, H2=48, activation=activation, high=3.0,
                 seed=5 + n_types, r_cut=rc)
    nlist = htf.Nlist(x)
    f, v = htf.compute_nlist_forces(nlist, lay(nlist), virial=True)
    G = lay.descriptor(x)
    assert f.dtype == dtype and v.dtype == dtype and G.dtype == dtype and f.shape == (300, 4) and v.shape == (300, 3, 3)
    F, E, Gref, V = reference(lay, x)
    print("cutoff T=%d %s NN=%d %s: forces %.3g energy %.3g virial %.3g descriptor %.3g of the scale (bound %.0e)" % (
        n_types, activation, NN, dtype, _err(f[:, :3], F), _err(f[:, 3], E), _err(v, V), _err(G, Gref), TOL))
    _close(f[:, :3], F, "forces")
    _close(f[:, 3], E, "energy")
    _close(v, V, "virial")
    _close(G, Gref, "descriptor")
    # without the virial: the same forces, bit for bit
    assert torch.equal(lay.forces(x), f)


# ------------------------------------------------------------------------------------------------ 2. beyond the cutoff is nothing
@pytest.mark.parametrize("n_types", [1, 2])
def test_beyond_the_cutoff_is_nothing(htf, cuda, n_types):
    rc, B, NN = 2.5, 200, 100
    rng = np.random.default_rng(3 + n_types)
    inner, cnt = random_nlist(rng, B, 60, fill=0.7, rmin=0.3 * rc, rmax=0.99 * rc, ntypes=n_types, dtype=np.float64)
    outer, _ = random_nlist(rng, B, 40, fill=0.6, rmin=1.0001 * rc, rmax=1.5 * rc, ntypes=n_types, dtype=np.float64)
    # interleave so that the far neighbors sit between near ones, in every lane's slots
    full = np.ascontiguousarray(np.concatenate([inner, outer], axis=1)[:, rng.permutation(NN)])
    x = torch.from_numpy(full).float().to(cuda)
    r = torch.linalg.norm(x[:, :, :3], dim=2)
    far = r >= 1.0001 * rc * (1 - 1e-6)
    assert far.any(dim=1).sum().item() > B // 2 and not ((r > 0.995 * rc) & ~far).any()
    x0 = x.clone()
    x0[far] = 0.0
    labels = torch.from_numpy(0.05 * rng.standard_normal((B, 4))).float().to(cuda)
    lay = _layer(htf, K=16, n_types=n_types, H1=24, H2=20, r_cut=rc, trainable=True)
    f, v = lay.forces(x, virial=True)
    f0, v0 = lay.forces(x0, virial=True)
    assert torch.equal(f, f0) and torch.equal(v, v0)
    assert torch.equal(lay.descriptor(x), lay.descriptor(x0))
    assert torch.equal(lay.loss_gradient(x, labels), lay.loss_gradient(x0, labels))


# ------------------------------------------------------------------------------------------------ 3. continuity
def _continuity_rows(n_rows, rc):
    """Row j (row seed j): four neighbors at 0.9 <= r <= 2.5 in random directions; ``with`` adds one at (rc (1 - 1e-5), 0, 0)."""
    without = np.zeros((n_rows, 8, 4))
    for j in range(n_rows):
        rng = np.random.default_rng(j)
        v = rng.standard_normal((4, 3))
        without[j, :4, :3] = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.9, 2.5, (4, 1))
    with_ = without.copy()
    with_[:, 4, 0] = rc * (1 - 1e-5)
    return without, with_


@pytest.mark.parametrize("seed", [3, 4, 5])
def test_energy_is_continuous_at_the_cutoff(htf, cuda, seed):
    """A neighbor entering at rc: without a cutoff function E_i jumps (the fp64 reference of the layer as it was says by how
    much); with r_cut = rc the kernel's E_i moves by at most 1e-3 of that jump.  fc(rc (1 - 1e-5)) = 2.5e-10."""
    rc = 3.0
    kw = dict(K=16, H1=32, H2=32, low=0.0, high=rc, activation="tanh", seed=seed, bias=0.0)   # mlp_params' own weights
    plain, smooth = _layer(htf, **kw), _layer(htf, r_cut=rc, **kw)
    assert torch.equal(plain.w, smooth.w)
    a, b = (torch.from_numpy(t).float().to(cuda) for t in _continuity_rows(4, rc))
    assert (torch.linalg.norm(b[:, 4, :3], dim=1) < rc).all()
    jump = (reference(plain, b)[1] - reference(plain, a)[1]).abs()
    rows = torch.nonzero(jump >= 1e-2)[:, 0]
    print("seed %d: reference jumps %s, rows used %s" % (seed, jump.tolist(), rows.tolist()))
    assert len(rows) > 0
    got_smooth = (smooth.forces(b)[:, 3].double() - smooth.forces(a)[:, 3].double()).abs()
    got_plain = (plain.forces(b)[:, 3].double() - plain.forces(a)[:, 3].double()).abs()
    print("   with r_cut %s, without %s" % (got_smooth.tolist(), got_plain.tolist()))
    assert (got_smooth[rows] <= 1e-3 * jump[rows]).all()
    assert (got_plain[rows] > 0.5 * jump[rows]).all()


# ------------------------------------------------------------------------------------------------ 4. the row list (contract b)
def _pairs(rng, B, NN, dtype):
    """random_nlist without its loop over the rows: live neighbors of two types at 0.3 <= r <= 3.2 (both sides of 2.6), padding."""
    v = rng.standard_normal((B, NN, 3))
    v *= rng.uniform(0.3, 3.2, (B, NN, 1)) / np.linalg.norm(v, axis=2, keepdims=True)
    nl = np.concatenate([v, rng.integers(0, 2, (B, NN, 1)).astype(np.float64)], axis=2)
    nl[np.arange(NN)[None, :] >= rng.binomial(NN, 0.75, B)[:, None]] = 0.0
    return torch.from_numpy(nl).to(dtype)


# the sizes follow the launch geometry (csrc/desc_row.h desc_grid, csrc/dtrain_row.h dtrain_grid): fewer rows than a block
# has waves, partial slots (NN = 37) and all four (256), several blocks, one row past the forces grid's single pass
# (2048 blocks x 4 waves) and one block's worth past the sweep grid's (512 blocks x 64 rows)
FORCES_GRID_ROWS, SWEEP_BLOCKS, SWEEP_BLOCK_ROWS = 2048 * 4, 512, 64
LIST_CASES = ([(B, NN, torch.float32, "small") for B in (1, 3, 5) for NN in (37, 256)]
              + [(300, NN, dt, "wide") for NN in (37, 256) for dt in (torch.float32, torch.float64)]
              + [(FORCES_GRID_ROWS + 3, 16, torch.float32, "small"), (SWEEP_BLOCKS * SWEEP_BLOCK_ROWS + 3, 16, torch.float32, "small")])
NETWORKS = {"small": dict(K=8, n_types=2, H1=8, H2=8), "wide": dict(K=16, n_types=2, H1=24, H2=20)}


def test_a_row_list_changes_which_rows_are_evaluated_never_a_bit(htf, cuda):
    """Every comparison is torch.equal.  Forces and virial into NaN-filled outputs: the identity list and the reversed list
    give the call without a list; every third row gives it on the listed rows and leaves the others NaN.  The sweep: the
    identity list gives the call without a list (a reordered one need not: the partial sums follow q).  The descriptor entry
    at r_cut = 0 is the layer without a cutoff.  The scratch size is dtrain_grid(n) partials of 1 + P."""
    from hoomd_tf_amd import _lib, ops
    lib, check = _lib.lib, _lib.check
    assert [c[0] for c in LIST_CASES[-2:]] == [8195, 32771]
    nan = float("nan")
    for B, NN, dtype, size in LIST_CASES:
        rng = np.random.default_rng(B + NN)
        x = _pairs(rng, B, NN, dtype).to(cuda)
        labels = torch.from_numpy(0.05 * rng.standard_normal((B, 4))).float().to(cuda)
        lists = {"identity": torch.arange(B, dtype=torch.int32, device=cuda),
                 "reversed": torch.arange(B - 1, -1, -1, dtype=torch.int32, device=cuda),
                 "third": torch.arange(1, B, 3, dtype=torch.int32, device=cuda)}
        assert len(lists["third"]) < B
        listed = torch.zeros(B, dtype=torch.bool, device=cuda)
        listed[lists["third"].long()] = True
        for r_cut in (None, 2.6):
            for activation in ("tanh", "linear"):
                kw = {} if r_cut is None else {"r_cut": r_cut}
                lay = _layer(htf, activation=activation, trainable=True, **NETWORKS[size], **kw)
                rc = float(lay.r_cut or 0.0)
                act = _lib.ACT_TANH if activation == "tanh" else _lib.ACT_LINEAR
                net_args = (x.data_ptr(), ops._dt(x), B, NN, lay.K, lay.n_types, lay.H1, lay.H2, act, lay.w.data_ptr(),
                            lay.mu.data_ptr(), float(lay.gap))
                what = "B=%d NN=%d %s r_cut=%s %s" % (B, NN, dtype, r_cut, activation)
                f, v = lay.forces(x, virial=True)
                assert torch.isfinite(f).all() and torch.isfinite(v).all(), what
                for name, rows in lists.items():
                    f2, v2 = torch.full_like(f, nan), torch.full_like(v, nan)
                    check(lib.htf_bp_forces(*net_args, f2.data_ptr(), ops._dt(f2), v2.data_ptr(), rows.data_ptr() if len(rows) else None,
                                            len(rows), rc, ops._stream(x)))
                    f3 = torch.full_like(f, nan)
                    check(lib.htf_bp_forces(*net_args, f3.data_ptr(), ops._dt(f3), None, rows.data_ptr() if len(rows) else None,
                                            len(rows), rc, ops._stream(x)))
                    if name == "third":
                        assert torch.equal(f2[listed], f[listed]) and torch.equal(v2[listed], v[listed]), (what, name)
                        assert torch.isnan(f2[~listed]).all() and torch.isnan(v2[~listed]).all() and torch.isnan(f3[~listed]).all()
                        assert torch.equal(f3[listed], f[listed]), (what, name)
                    else:
                        assert torch.equal(f2, f) and torch.equal(v2, v) and torch.equal(f3, f), (what, name)
                # the sweep
                pred = f.to(torch.float32).contiguous()
                accum = lay.loss_gradient(x, labels, pred=pred)
                assert torch.isfinite(accum).all() and accum[1:].abs().max().item() > 0, what
                n = int(lib.htf_bp_scratch_floats(B, lay.K, lay.n_types, lay.H1, lay.H2))
                assert n == min(-(-B // SWEEP_BLOCK_ROWS), SWEEP_BLOCKS) * (1 + lay.P), what
                scratch = torch.empty(n, dtype=torch.float32, device=cuda)
                accum2 = torch.full_like(accum, nan)
                check(lib.htf_bp_loss_grad(*net_args, labels.data_ptr(), ops._dt(labels), pred.data_ptr(), accum2.data_ptr(),
                                           scratch.data_ptr(), lists["identity"].data_ptr(), B, rc, ops._stream(x)))
                assert torch.equal(accum2, accum), what
            # the descriptor does not see the network: once per cutoff
            if r_cut is None:
                G = lay.descriptor(x)
                G2 = torch.full_like(G, nan)
                check(lib.htf_bp_descriptor(x.data_ptr(), ops._dt(x), B, NN, lay.K, lay.n_types, lay.mu.data_ptr(), float(lay.gap),
                                            G2.data_ptr(), ops._dt(G2), 0.0, ops._stream(x)))
                assert torch.equal(G2, G) and torch.isfinite(G).all(), what


# ------------------------------------------------------------------------------------------------ 5. species, forces (contract b)
def _species(case, B, rng):
    sp = rng.integers(0, 3, size=B)
    if case == "one-row":     # species 1 has exactly one row
        sp[sp == 1] = 0
        sp[B // 3] = 1
    elif case == "empty":     # species 2 has none
        sp[sp == 2] = 1
    return sp


@pytest.mark.parametrize("r_cut", [None, 2.6])
@pytest.mark.parametrize("case", ["one-row", "empty"])
def test_species_forces_are_the_single_networks(htf, cuda, case, r_cut):
    B, NN, S = 300, 70, 3
    rng = np.random.default_rng(11)
    nl, _ = random_nlist(rng, B, NN, fill=0.75, rmin=0.3, rmax=3.2, ntypes=2, dtype=np.float32)
    x = torch.from_numpy(nl).to(cuda)
    sp = _species(case, B, rng)
    counts = np.bincount(sp, minlength=S)
    assert counts[1] == 1 if case == "one-row" else counts[2] == 0
    kw = {} if r_cut is None else {"r_cut": r_cut}
    lay = _layer(htf, K=16, n_types=2, H1=24, H2=20, n_species=S, seed=8, **kw)
    assert not torch.equal(lay.w[:lay.P], lay.w[lay.P:2 * lay.P])
    species = torch.from_numpy(sp + rng.uniform(-0.4, 0.4, B)).float().to(cuda)      # rint(species) picks the network
    f, v = lay.forces(x, virial=True, species=species)
    assert torch.isfinite(f).all() and torch.isfinite(v).all()
    for s in range(S):
        rows = torch.from_numpy(np.nonzero(sp == s)[0]).to(cuda)
        one = _single(htf, lay, s)
        assert one.n_species == 1 and one.r_cut == lay.r_cut
        f1, v1 = one.forces(x, virial=True)
        assert torch.equal(f[rows], f1[rows]) and torch.equal(v[rows], v1[rows])
        # ... and they do not depend on the batch either: the species' rows alone
        assert torch.equal(f[rows], one.forces(x[rows].contiguous()))
    assert torch.equal(lay.forces(x, species=species), f)
    # a [B, 4] positions tensor: column 3; through the symbolic energy as well
    pos = torch.zeros((B, 4), device=cuda)
    pos[:, 3] = torch.from_numpy(sp).float().to(cuda)
    assert torch.equal(lay.forces(x, species=pos), f)
    nlist = htf.Nlist(x)
    assert torch.equal(htf.compute_nlist_forces(nlist, lay(nlist, pos)), f)
    assert torch.equal(lay(nlist, pos).tensor(), f[:, 3])
    # the cached partition follows an in-place write to the species tensor
    pos[:, 3] = 0.0
    assert torch.equal(lay.forces(x, species=pos), _single(htf, lay, 0).forces(x))


def test_species_small_batches_and_errors(htf, cuda):
    lay = _layer(htf, K=8, n_types=1, H1=8, H2=8, n_species=3, r_cut=2.5, trainable=True)
    for B in (5, 0):
        x = torch.from_numpy(random_nlist(np.random.default_rng(B), B, 20, dtype=np.float32)[0]).to(cuda)
        species = torch.tensor([2, 0, 2, 1, 0][:B], dtype=torch.float32, device=cuda)
        f, v = lay.forces(x, virial=True, species=species)
        assert f.shape == (B, 4) and v.shape == (B, 3, 3) and torch.isfinite(f).all()
        for i in range(B):
            assert torch.equal(f[i:i + 1], _single(htf, lay, int(species[i])).forces(x[i:i + 1].contiguous()))
        acc = lay.loss_gradient(x, torch.zeros((B, 4), device=cuda), species=species)
        assert acc.shape == (3, 1 + lay.P) and torch.isfinite(acc).all()
        if B == 0:
            assert (acc == 0).all()
    x = torch.from_numpy(random_nlist(np.random.default_rng(1), 6, 20, dtype=np.float32)[0]).to(cuda)
    with pytest.raises(ValueError, match="species"):
        lay.forces(x)
    with pytest.raises(ValueError, match="species"):
        lay.loss_gradient(x, torch.zeros((6, 4), device=cuda))
    for bad in (3.0, -1.0, 2.6, float("nan")):
        species = torch.tensor([0, 1, 2, bad, 0, 1], dtype=torch.float32, device=cuda)
        with pytest.raises(ValueError, match="outside"):
            lay.forces(x, species=species)
    with pytest.raises(ValueError, match="species must be"):
        lay.forces(x, species=torch.zeros(5, device=cuda))
    # one network: species are accepted and ignored
    one = _layer(htf, K=8, H1=8, H2=8, r_cut=2.5)
    assert torch.equal(one.forces(x, species=torch.full((6,), 7.0, device=cuda)), one.forces(x))


# ------------------------------------------------------------------------------------------------ 6. species, sweep (contract c)
@pytest.mark.parametrize("r_cut", [None, 2.6])
@pytest.mark.parametrize("case", ["one-row", "empty"])
def test_species_sweep_is_the_single_networks_on_the_gathered_rows(htf, cuda, case, r_cut):
    B, NN, S = 300, 70, 3
    rng = np.random.default_rng(13)
    nl, _ = random_nlist(rng, B, NN, fill=0.75, rmin=0.3, rmax=3.2, ntypes=2, dtype=np.float32)
    x = torch.from_numpy(nl).to(cuda)
    labels = torch.from_numpy(0.05 * rng.standard_normal((B, 4))).float().to(cuda)
    sp = _species(case, B, rng)
    species = torch.from_numpy(sp).float().to(cuda)
    kw = {} if r_cut is None else {"r_cut": r_cut}
    lay = _layer(htf, K=16, n_types=2, H1=24, H2=20, n_species=S, seed=8, trainable=True, **kw)
    pred = lay.forces(x, species=species)
    accum = lay.loss_gradient(x, labels, species=species)
    assert accum.shape == (S, 1 + lay.P) and accum.dtype == torch.float32 and torch.isfinite(accum).all()
    for s in range(S):
        rows = torch.from_numpy(np.nonzero(sp == s)[0]).to(cuda)
        if len(rows) == 0:
            assert (accum[s] == 0).all()
            continue
        one = _single(htf, lay, s)
        want = one.loss_gradient(x[rows].contiguous(), labels[rows].contiguous(), pred=pred[rows].contiguous())
        assert torch.equal(accum[s], want), s
        assert accum[s, 1:].abs().max().item() > 0
    assert torch.equal(lay.loss_gradient(x, labels, species=species), accum)
    out = torch.full_like(accum, float("nan"))
    assert lay.loss_gradient(x, labels, pred=pred, accum=out, species=species) is out and torch.equal(out, accum)


# ------------------------------------------------------------------------------------------------ 7. the sweep with the cutoff
def _reference_gradient(lay, x, resid32):
    """d SSR / d theta in fp64 by double backward through the definition with fc, the residual being the sweep's own."""
    W = [torch.as_tensor(w.astype(np.float64), device=x.device).requires_grad_(True) for w in lay.get_weights()]
    pred, _, _ = net(lay, W, x.to(torch.float64), create_graph=True)
    labels_eff = pred.detach() - resid32.to(torch.float64)
    ssr = ((pred - labels_eff) ** 2).sum()
    return torch.cat([g.reshape(-1) for g in torch.autograd.grad(ssr, W)])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("NN", [37, 256])
@pytest.mark.parametrize("n_types", [1, 2])
@pytest.mark.parametrize("activation", ["tanh", "linear"])
def test_cutoff_gradient_against_fp64_double_backward(htf, cuda, activation, n_types, NN, dtype):
    rc, B = 2.75, 300
    rng = np.random.default_rng(7 + NN + 3 * n_types)
    nl = _rows_around(rng, B, NN, rc, n_types)
    nl[0] = 0.0             # row 0: no live neighbor (padding with a nonzero column 3)
    nl[0, :, 3] = 1.0
    x = torch.from_numpy(nl).to(dtype).to(cuda)
    labels = torch.from_numpy(0.05 * rng.standard_normal((B, 4))).float().to(cuda)
    lay = _layer(htf, K=16, n_types=n_types, H1=24, H2=20, activation=activation, seed=5 + n_types, r_cut=rc, trainable=True)
    accum = lay.loss_gradient(x, labels)
    assert accum.dtype == torch.float32 and accum.shape == (1 + lay.P,) and torch.isfinite(accum).all()
    pred = lay.forces(x).to(torch.float32)
    resid = pred - labels
    g = _reference_gradient(lay, x, resid)
    got = accum[1:].double()
    scale, err = g.abs().max().item(), (got - g).abs().max().item()
    ssr = (resid.double() ** 2).sum().item()
    print("cutoff sweep %s T=%d NN=%d %s: max|got - g| = %.3g, max|g| = %.3g, ratio %.3g (bound %.0e); SSR %.9g vs %.9g" % (
        activation, n_types, NN, dtype, err, scale, err / scale, GTOL, accum[0].item(), ssr))
    assert np.isfinite(err) and scale > 0 and err < GTOL * scale
    assert abs(accum[0].item() - ssr) <= 1e-5 * ssr
    for k, sl in _blocks(lay):
        assert g[sl].abs().max().item() > 0 and got[sl].abs().max().item() > 0, "%s carries no signal" % k
    assert torch.equal(lay.loss_gradient(x, labels, pred=pred), accum)


# ------------------------------------------------------------------------------------------------ 8. through tfcompute
NN_BOX, RC_BOX = 128, 2.4


def _fcc_sim2(htf, cuda, seed, third_type=False):
    """The 500-particle fcc box of tests/test_gpu_desc.py::_fcc_sim with two particle types (and one particle of a third)."""
    from hoomd_tf_amd import standin
    pos, L, a = standin.fcc_positions(5, 0.8442)
    rng = np.random.default_rng(seed)
    pos = pos + 0.03 * a * rng.standard_normal(pos.shape)
    pos -= np.round(pos / L) * L
    types = (rng.uniform(size=len(pos)) < 0.3).astype(np.int32)
    if third_type:
        types[7] = 2
    sysm = standin.System(pos, L, types=types, dtype=torch.float32, device=cuda)
    sysm.randomize_velocities(kT=0.3, seed=seed)
    sim = standin.Simulation(sysm)
    sim.integrate_nve(0.001)
    return sim, sysm


def _kernel_model(htf, lay):
    class M(htf.SimModel):
        def setup(self):
            self.desc = lay

        def compute(self, nlist, positions, box):
            return htf.compute_nlist_forces(nlist, self.desc(nlist, positions))
    return M


def _layers_model(htf, lay):
    """The same network from RBFExpansion, fc, a masked sum and one Dense stack per species (torch ops and autograd)."""
    ws = lay.get_weights()

    class L(htf.SimModel):
        def setup(self):
            self.rbf = htf.RBFExpansion(lay.low, lay.high, lay.K)
            self.ds = []
            for s in range(lay.n_species):
                ds = [htf.Dense(lay.H1, activation="tanh"), htf.Dense(lay.H2, activation="tanh"), htf.Dense(1)]
                for d, (k, b) in zip(ds, ((ws[0][s], ws[1][s]), (ws[2][s], ws[3][s]), (ws[4][s], ws[5][s]))):
                    d.build(k.shape[0])
                    d.set_weights([k, b])
                self.ds.append(ds)

        def compute(self, nlist, positions, box):
            r = htf.safe_norm(nlist[:, :, :3], axis=2)
            live = (htf.nlist_rinv(nlist).tensor() > 0).to(torch.float32)
            t = nlist.ad[:, :, :3] + 1e-7       # the same distances on the autograd leaf, for fc
            fc = _fc(torch.sqrt((t * t).sum(dim=2)), float(lay.r_cut))
            g = (self.rbf(r) * (live * fc)[..., None]).sum(dim=1)
            sp = torch.round(positions[:, 3])
            e = sum((sp == s).to(torch.float32) * ds[2](ds[1](ds[0](g)))[:, 0] for s, ds in enumerate(self.ds))
            return htf.compute_nlist_forces(nlist, e)
    return L


def test_tfcompute_species_and_cutoff(htf, cuda):
    """Three steps of the two-type box: batches give the bits of the whole step, and the forces are those of the same
    network written with the layers -- each side is held to 2e-5 of the fp64 scale, so the two differ by at most 4e-5, the
    bound of tests/test_gpu_desc.py::test_equals_network_written_with_the_layers."""
    lay = _layer(htf, K=16, H1=32, H2=32, low=0.8, high=2.5, seed=15, r_cut=RC_BOX, n_species=2)
    runs = []
    for Model, bs in ((_kernel_model(htf, lay), None), (_kernel_model(htf, lay), 500 // 3), (_layers_model(htf, lay), None)):
        sim, sysm = _fcc_sim2(htf, cuda, seed=19)
        tfc = htf.tfcompute(Model(NN_BOX))
        tfc.attach(sim.nlist_cell(), r_cut=2.5, batch_size=bs)
        sim.run(3)
        torch.cuda.synchronize()
        assert not tfc.graph_safe() and tfc._plan is None
        runs.append((sysm.force[:sysm.N].clone(), sysm.pos[:sysm.N].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert runs[2][0][:, :3].abs().max().item() > 1e-2
    assert (runs[0][1][:, :3] - runs[2][1][:, :3]).abs().max().item() < 1e-4
    _close(runs[0][0][:, :3], runs[2][0][:, :3], "forces", tol=2 * TOL)
    _close(runs[0][0][:, 3], runs[2][0][:, 3], "energy", tol=2 * TOL)


def _training_run(htf, cuda, lay, optimizer, steps, types_seed=23):
    """The set-up of tests/test_gpu_desc_train.py::_training_run on the two-type box: LJModel drives the run and supplies the labels."""
    import build_examples
    sim, sysm = _fcc_sim2(htf, cuda, seed=types_seed)
    nlist = sim.nlist_cell()
    lj = htf.tfcompute(build_examples.LJModel(NN_BOX))
    lj.attach(nlist, r_cut=2.5)
    model = _kernel_model(htf, lay)(NN_BOX, output_forces=False)
    model.compile(optimizer, loss='MeanSquaredError')
    tfc = htf.tfcompute(model)
    tfc.attach(nlist, train=True, r_cut=2.5)
    tfc.set_reference_forces(lj)
    sim.run(steps)
    torch.cuda.synchronize()
    return model, tfc, sysm


def test_one_sgd_step_moves_each_species_by_its_own_gradient(htf, cuda):
    """After ONE SGD step from fresh weights, w_s - w0_s = -lr g_s / (4 N) for the two species of the box, g from
    loss_gradient on the step's own tensor, positions and staged labels; N is the whole batch.  The third species has no
    particle: its weights keep their bits.  The step is sized as in tests/test_gpu_desc_train.py::
    test_one_sgd_step_is_the_sweeps_gradient (max|dw| about 0.25), with that test's bound of 1e-6 max|dw|."""
    kw = dict(K=8, H1=8, H2=8, high=2.5, r_cut=RC_BOX, n_species=3, trainable=True)

    def run(lr):
        lay = _layer(htf, **kw)
        w0 = lay.w.clone()
        model, tfc, sysm = _training_run(htf, cuda, lay, htf.optimizers.SGD(lr), 1)
        x = torch.from_numpy(tfc.get_nlist_array()).to(torch.float32).to(cuda)
        pos = torch.from_numpy(tfc.get_positions_array()).to(torch.float32).to(cuda)
        fresh = _layer(htf, **kw)
        assert torch.equal(fresh.w, w0) and x.shape[0] == sysm.N and pos.shape == (sysm.N, 4)
        counts = fresh.species_counts(pos, x)
        assert counts[0] > 0 and counts[1] > 0 and counts[2] == 0
        accum = fresh.loss_gradient(x, tfc._labels[:sysm.N].contiguous(), species=pos)
        loss = float(model.metrics[0].result())
        return (lay.w.double() - w0.double()).view(3, -1), accum.double(), sysm.N, loss, torch.equal(lay.w[2 * lay.P:], w0[2 * lay.P:])

    _, accum, N, _, _ = run(1e-3)
    lr = 0.25 * 4 * N / accum[:, 1:].abs().max().item()
    dw, accum2, _, loss, third_kept = run(lr)
    assert torch.equal(accum2, accum) and third_kept and (dw[2] == 0).all()
    want = -lr * accum[:, 1:] / (4 * N)
    scale = want.abs().max().item()
    for s in (0, 1):
        err = (dw[s] - want[s]).abs().max().item()
        print("one SGD step, species %d: lr %.4g, max|dw_s| %.3g of max|dw| %.3g, max err %.3g" % (s, lr, want[s].abs().max().item(), scale, err))
        assert want[s].abs().max().item() > 0 and err <= 1e-6 * scale
    # the reported loss: the sum of the species' sums of squared residuals / (4 N)
    assert abs(loss - accum[:, 0].sum().item() / (4 * N)) <= 1e-5 * loss


def test_tfcompute_species_out_of_range_raises(htf, cuda):
    """A layer of two species takes the box's types 0 and 1; one particle of a third type raises."""
    lay = _layer(htf, K=8, H1=8, H2=8, high=2.5, n_species=2)
    sim, sysm = _fcc_sim2(htf, cuda, seed=5, third_type=True)
    tfc = htf.tfcompute(_kernel_model(htf, lay)(NN_BOX))
    tfc.attach(sim.nlist_cell(), r_cut=2.5)
    with pytest.raises(ValueError, match="outside"):
        sim.run(1)
