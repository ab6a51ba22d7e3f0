"""Force matching on the angular conservative forces of htf.DescriptorMLP on the host: the C ABI table of
include/htf_atrain.h, the header as C99, the code objects of the sweep, the layer's ``trainable="angular"`` value, the argument
checks of the entry point, and the mathematics of the sweep in fp64 torch.  No GPU."""
import math
import os
import re

import numpy as np
import pytest
import torch

# kernel names the older census tests search by substring: no new kernel may carry one
OLDER_CENSUS = ("ang_", "bp_", "dtrain_", "desc_mlp", "cf_grad_kernel", "cf_pair_force_kernel", "cf_pair_kernel", "ct_sweep_kernel")


def _header():
    from helpers import ROOT
    return open(os.path.join(ROOT, "include", "htf_atrain.h")).read()


# ------------------------------------------------------------------------------------------------ 1. the ABI table
def test_at_abi_table(htf):
    """The symbols of include/htf_atrain.h are AT_PROTOTYPES: exported, bound under the active binding, argument for argument,
    and no name is shared with another table.  The older tables keep their sizes and the ABI version has not moved."""
    import ctypes
    import subprocess
    L = htf._lib
    names = sorted(set(re.findall(r"HTF_API[^;]*?\b(htf_\w+)\s*\(", _header())))
    assert names == sorted(L.AT_PROTOTYPES) == ["htf_at_loss_grad"]
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and hasattr(L.lib, n)
        decl = re.search(r"HTF_API\s+\w+\s+%s\s*\(([^)]*)\)" % n, _header()).group(1)
        assert len(decl.split(",")) == len(L.AT_PROTOTYPES[n][1]) == len(L.CT_PROTOTYPES["htf_ct_loss_grad"][1]) + 1 == 21, n
    for t in (L.PROTOTYPES, L.STANDIN_PROTOTYPES, L.STEP_CHECK_PROTOTYPES, L.CG_PROTOTYPES, L.GEOM_PROTOTYPES, L.NLIST_PROTOTYPES,
              L.BP_PROTOTYPES, L.CF_PROTOTYPES, L.CT_PROTOTYPES, L.ANG_PROTOTYPES):
        assert not set(names) & set(t)
    every = [n for n, _ in L.ALL_PROTOTYPES]
    assert set(names) <= set(every) and len(every) == len(set(every))
    assert (len(L.BP_PROTOTYPES), len(L.CF_PROTOTYPES), len(L.CT_PROTOTYPES), len(L.ANG_PROTOTYPES)) == (4, 3, 1, 3)
    assert raw.htf_abi_version() == 5 and L.ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {line.split()[-1] for line in nm.splitlines() if line.strip()}


def test_at_pybind_module_exports_table(htf):
    import importlib
    mod_path = os.path.join(os.path.dirname(htf._lib.LIB_PATH), "_htf_abi.so")
    if not os.path.exists(mod_path):
        pytest.skip("the pybind11 module is not built")
    mod = importlib.import_module("hoomd_tf_amd._htf_abi")
    for n in htf._lib.AT_PROTOTYPES:
        assert hasattr(mod, n)


def test_at_header_is_plain_c():
    """include/htf_atrain.h compiles as C99 beside the other descriptor headers."""
    import subprocess
    import tempfile
    from helpers import ROOT
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "htf_amd.h"\n#include "htf_bp.h"\n#include "htf_cforce.h"\n#include "htf_ctrain.h"\n'
                             '#include "htf_angular.h"\n#include "htf_atrain.h"\n'
                             'int main(void){int (*f)(const void *, int, const int *, unsigned, unsigned, unsigned, unsigned, '
                             'unsigned, unsigned, int, const float *, const float *, float, const float *, float *, float *, '
                             'const int *, unsigned, float, unsigned, htf_stream) = htf_at_loss_grad; (void)f; return HTF_OK;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


# ------------------------------------------------------------------------------------------------ 2. the code objects
def test_at_kernels_use_no_scratch(tmp_path):
    """Every instantiation of the sweep -- activation x cutoff x list x l_max x nlist dtype -- keeps to registers: no private
    segment, no vector-register spills; its name stays out of the older census tests' searches, and the library keeps one
    reduction kernel."""
    import test_codeobj as t
    if not (os.path.exists(t.LIB) and os.path.exists(t.READELF)):
        pytest.skip("library or llvm-readelf missing")
    meta = t._kernel_metadata(tmp_path)
    sweep = [n for n in meta if "at_sweep_kernel" in n]
    assert len(sweep) == 32
    assert not [(n, s) for n in sweep for s in OLDER_CENSUS if s in n]
    assert len([n for n in meta if "dtrain_reduce_kernel" in n]) == 1
    bad = {n: meta[n] for n in sweep if meta[n]["private_segment_fixed_size"] or meta[n]["vgpr_spill_count"]}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 3. the layer
def test_at_layer_trainable_angular(htf):
    for l_max in (1, 2):
        lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable="angular", l_max=l_max)
        assert lay.trainable == "angular" and lay.conservative is True and lay.l_max == l_max and lay.D == 8 * (1 + l_max)
        cfg = lay.get_config()
        assert cfg["trainable"] == "angular" and cfg["conservative"] is True and cfg["l_max"] == l_max
        again = htf.DescriptorMLP(device="cpu", **cfg)
        assert again.trainable == "angular" and again.conservative is True and again.l_max == l_max and again.get_config() == cfg
        assert torch.equal(again.w, lay.w)
    # the value alone implies the conservative forces
    assert htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable="angular", conservative=False, l_max=1).conservative is True
    full = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable="angular", l_max=2, r_cut=2.5, n_species=2, n_types=2).get_config()
    assert full["n_species"] == 2 and full["n_types"] == 2 and full["r_cut"] == 2.5
    assert htf.DescriptorMLP(device="cpu", **full).get_config() == full
    # no angular channels to fit without l_max: the message names the value that fits the radial layer
    for kw in (dict(), dict(l_max=0), dict(conservative=True)):
        with pytest.raises(ValueError, match="angular") as info:
            htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable="angular", **kw)
        assert 'trainable="total"' in str(info.value)
    # the other values are what they were
    with pytest.raises(ValueError, match="trainable"):
        htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable="forces")
    with pytest.raises(ValueError, match="trainable"):
        htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable="forces", l_max=1)
    assert htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable=True).get_config()["trainable"] is True
    assert htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable="total").get_config()["trainable"] == "total"
    assert htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True, l_max=1).trainable is False
    # what the optimizer step asks of a trainable layer
    d = htf.optimizers.SGD(0.1).desc(lay.nonneg_mask, lay.l1_reg)
    assert d.nonneg_mask == 0 and d.l1_reg[0] == 0.0


def test_at_pinned_raises_name_the_way_out(htf):
    """The two NotImplementedErrors tests/test_angular_cpu.py pins still say ``follow-up`` and now name what works."""
    for tr in (True, "total"):
        with pytest.raises(NotImplementedError, match="follow-up") as info:
            htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=(tr == "total"), l_max=1, trainable=tr)
        assert 'trainable="angular"' in str(info.value)
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True, l_max=2)
    with pytest.raises(NotImplementedError, match="follow-up") as info:
        lay.total_loss_gradient(torch.zeros((4, 16, 4)), torch.zeros((4, 4)), torch.zeros((4, 16), dtype=torch.int32))
    assert "angular_loss_gradient" in str(info.value)


def test_at_angular_loss_gradient_has_no_cpu_path(htf):
    """Callable on any layer with l_max > 0, trainable or not; no CPU path; an l_max = 0 layer is pointed to its own sweep."""
    x, labels, index = torch.zeros((4, 16, 4)), torch.zeros((4, 4)), torch.zeros((4, 16), dtype=torch.int32)
    for kw in (dict(trainable="angular", l_max=1), dict(conservative=True, l_max=2), dict(trainable="angular", l_max=2, n_types=2)):
        lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", **kw)
        with pytest.raises(ValueError, match="device tensor"):
            lay.angular_loss_gradient(x, labels, index)
    for kw in (dict(trainable="total"), dict(conservative=True), dict()):
        lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", **kw)
        with pytest.raises(ValueError, match="total_loss_gradient"):
            lay.angular_loss_gradient(x, labels, index)


# ------------------------------------------------------------------------------------------------ 4. the entry point
def test_at_loss_grad_entry_point_argument_errors(htf):
    """The C checks (no launch, no device needed): htf_ct_loss_grad's, l_max and the width of the input."""
    L = htf._lib
    mu = torch.zeros(8)
    w = torch.zeros(16 * 8 + 8 + 8 * 8 + 8 + 8 + 1)
    args = dict(nlist=0x1000, dt=L.HTF_F32, index=0x6000, B=4, NN=16, K=8, T=1, H1=8, H2=8, act=L.ACT_TANH, w=w.data_ptr(),
                mu=mu.data_ptr(), gap=0.5, rho=0x3000, accum=0x4000, scratch=0x5000, rows=None, n_rows=4, rc=0.0, l_max=1)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_at_loss_grad(a["nlist"], a["dt"], a["index"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"],
                                      a["w"], a["mu"], a["gap"], a["rho"], a["accum"], a["scratch"], a["rows"], a["n_rows"], a["rc"],
                                      a["l_max"], None)

    for bad in (dict(K=1), dict(K=33, T=2), dict(NN=257), dict(gap=0.0), dict(gap=-1.0), dict(dt=5), dict(mu=None), dict(nlist=None),
                dict(n_rows=5), dict(rc=-1.0), dict(rc=float("nan")), dict(rc=float("inf")), dict(rc=-float("inf")), dict(H1=0),
                dict(H2=65), dict(act=7), dict(w=None), dict(rho=None), dict(accum=None), dict(scratch=None), dict(index=None),
                dict(B=0, w=None), dict(B=0, n_rows=1),
                dict(l_max=0), dict(l_max=3), dict(K=13, T=5, l_max=0), dict(K=13, T=5, l_max=1 << 31), dict(K=5, T=13),
                dict(K=13, T=5), dict(K=33), dict(K=22, l_max=2)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    # 65 channels and 66 inputs are refused where 64 and 63 inputs are taken (B = 0: no launch)
    none = dict(B=0, n_rows=0, nlist=None, index=None, rho=None, accum=None, scratch=None)
    assert call(K=33, **none) == L.HTF_ERR_INVALID and call(K=13, T=5, **none) == L.HTF_ERR_INVALID and "descriptor network" in L.last_error()
    assert call(K=32, **none) == L.HTF_OK and call(K=7, T=3, l_max=2, **none) == L.HTF_OK and call(K=16, T=2, **none) == L.HTF_OK
    # B = 0: HTF_OK with no row pointer to read and, without an accum to zero-fill, no launch; the limits are still checked
    assert call(**none) == L.HTF_OK and call(l_max=2, **none) == L.HTF_OK
    assert call(K=1, **none) == L.HTF_ERR_INVALID and "descriptor network" in L.last_error()
    assert call(l_max=0, **none) == L.HTF_ERR_INVALID and "descriptor network" in L.last_error()


# ------------------------------------------------------------------------------------------------ 5. the mathematics
def _lattice(n=4, rc_list=1.5, seed=3):
    """An n^3 jittered periodic lattice of spacing 1 with two types: (pos [N, 3], types [N], L, idx [N, NN] with -1 on empty slots,
    occ [N, NN]) in fp64 on the CPU; every pair inside rc_list under minimum image, so the list is symmetric."""
    rng = np.random.default_rng(seed)
    ijk = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    pos = torch.from_numpy(ijk + rng.uniform(-0.08, 0.08, ijk.shape))
    types = torch.from_numpy(rng.integers(0, 2, len(pos)).astype(np.float64))
    L = float(n)
    d = pos[None, :, :] - pos[:, None, :]
    d = d - L * torch.round(d / L)
    near = (d.norm(dim=2) < rc_list) & ~torch.eye(len(pos), dtype=torch.bool)
    assert torch.equal(near, near.T)
    NN = int(near.sum(dim=1).max())
    idx = torch.full((len(pos), NN), -1, dtype=torch.long)
    for i in range(len(pos)):
        js = torch.nonzero(near[i])[:, 0]
        idx[i, :len(js)] = js
    return pos, types, L, idx, idx >= 0


def tangent(lay, aux, tn, d):
    """Xdot = [Gdot | Adot | Qdot] [B, D] by DESIGN.md 0.7 from the slots' d [B, NN, 3] and _inputs' aux, in aux's dtype."""
    r, live, fc, dfc, u, v, M = (aux[k] for k in ("r", "live", "fc", "dfc", "u", "v", "M"))
    dt = r.dtype
    B, NN = r.shape
    mu = torch.as_tensor(lay.centers.astype(np.float64)).to(dt)
    dk = r[..., None] - mu
    ek = torch.exp(-dk * dk / float(lay.gap)) * live.to(dt)[..., None]
    w = fc[..., None] * ek                                                              # [B, NN, K]
    wp = fc[..., None] * (-2.0 / float(lay.gap)) * dk * ek + dfc[..., None] * ek
    onehot = torch.stack([(tn == tt).to(dt) for tt in range(lay.n_types)], dim=2)       # [B, NN, T]

    def chan(z):   # [B, NN, K] -> [B, Dr, NN]
        return (z[:, :, None, :] * onehot[:, :, :, None]).reshape(B, NN, lay.n_types * lay.K).transpose(1, 2)

    a = (d * u).sum(dim=2)
    perp = (d - a[..., None] * u) / r[..., None]
    wt, wd = chan(w), chan(wp * a[..., None])
    Gdot = wd.sum(dim=2)
    vdot = wd @ u + wt @ perp
    uu = (u[..., :, None] * u[..., None, :]).reshape(B, NN, 9)
    pu = (perp[..., :, None] * u[..., None, :] + u[..., :, None] * perp[..., None, :]).reshape(B, NN, 9)
    Mdot = wd @ uu + wt @ pu
    blocks = [Gdot, 2.0 * (v * vdot).sum(dim=2), 2.0 * (M * Mdot).sum(dim=2)][:1 + lay.l_max]
    return torch.cat(blocks, dim=1)


@pytest.mark.parametrize("l_max", [1, 2])
def test_at_mathematics_on_the_host(htf, l_max):
    """2 d/dtheta sum_i (grad_X E_i . Xdot_i + rho_iE E_i), Xdot by the formulas of DESIGN.md 0.7, equals d/dtheta of
    2 sum_i rho_i . pred_i with pred = (-d(sum E)/dr, E) by autograd through the positions, to 1e-12 of the largest entry: a
    4^3 jittered periodic lattice, a symmetric list, two types, a cutoff, tanh, random weights with non-zero biases."""
    import test_gpu_desc_angular as A
    import test_gpu_desc_total_train as TT
    pos, types, L, idx, occ = _lattice()
    lay = htf.DescriptorMLP(K=6, H1=12, H2=10, low=0.5, high=1.5, n_types=2, activation="tanh", seed=7, r_cut=1.35,
                            conservative=True, l_max=l_max, device="cpu")
    rng = np.random.default_rng(11 + l_max)
    lay.set_weights([(0.3 * rng.standard_normal(w.shape)).astype(np.float32) for w in lay.get_weights()])
    W = TT._weights(lay, "cpu")
    assert all(w.abs().max().item() > 0 for w in W)
    sp = torch.zeros(len(pos), dtype=torch.long)
    tn = torch.where(occ, types[idx.clamp(min=0)], torch.full_like(types[idx.clamp(min=0)], -1.0))
    rho = torch.from_numpy(rng.standard_normal((len(pos), 4)))

    # the reference: autograd through the positions
    q = pos.clone().requires_grad_(True)
    E = TT._net(lay, W, A._inputs(lay, A._pair_vectors(q, idx, occ, L), tn)[0], sp)
    (g,) = torch.autograd.grad(E.sum(), q, create_graph=True)
    pred = torch.cat([-g, E[:, None]], dim=1)
    ref = TT._flat(torch.autograd.grad(2.0 * (rho * pred).sum(), W))[0]

    # the sweep's regrouping: every term on the row whose energy it differentiates
    x3 = A._pair_vectors(pos, idx, occ, L)
    X, aux = A._inputs(lay, x3, tn)
    assert int(aux["live"].sum()) > 0 and int((~aux["live"] & occ).sum()) > 0   # the cutoff drops listed neighbors
    d = rho[:, None, :3] - rho[idx.clamp(min=0), :3] * occ[..., None].to(torch.float64)
    Xdot = tangent(lay, aux, tn, d)
    Xl = X.detach().requires_grad_(True)
    Ei = TT._net(lay, W, Xl, sp)
    (gX,) = torch.autograd.grad(Ei.sum(), Xl, create_graph=True)
    got = TT._flat(torch.autograd.grad(2.0 * ((gX * Xdot).sum() + (rho[:, 3] * Ei).sum()), W, retain_graph=True))[0]

    scale, err = ref.abs().max().item(), (got - ref).abs().max().item()
    print("l_max = %d: max|got - ref| = %.3g of %.3g, ratio %.3g" % (l_max, err, scale, err / scale))
    for k, sl in TT._blocks(lay):
        assert ref[sl].abs().max().item() > 0 and got[sl].abs().max().item() > 0, k
    # the angular blocks of the tangent carry weight: without them the answer is another
    Xr = Xdot.clone()
    Xr[:, lay.Dr:] = 0.0
    radial = TT._flat(torch.autograd.grad(2.0 * ((gX * Xr).sum() + (rho[:, 3] * Ei).sum()), W))[0]
    assert (radial - ref).abs().max().item() > 1e-3 * scale
    assert math.isfinite(err) and err <= 1e-12 * scale
