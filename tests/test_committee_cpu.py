"""The committee of descriptor networks (htf.DescriptorMLP(n_models=M)) on the host: the C ABI table of
include/htf_committee.h, the header as C99, the code objects of the two sweeps, the layer's ``n_models`` argument, its weights
and ``member(m)``, and the argument checks of the entry points.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

# what existing host tests count the family's kernels by: no committee kernel may carry one of these
FAMILY_SUBSTRINGS = ("bp_", "dtrain_", "desc_mlp", "cf_grad_kernel", "cf_pair_force_kernel", "cf_pair_kernel", "ct_sweep_kernel",
                     "at_sweep_kernel", "ang_", "ghost")


def _header():
    from helpers import ROOT
    return open(os.path.join(ROOT, "include", "htf_committee.h")).read()


def test_cmt_abi_table(htf):
    """The symbols of include/htf_committee.h are CMT_PROTOTYPES: exported, bound under the active binding, argument for
    argument, and no name is shared with another table.  The other tables keep their sizes and the ABI version has not moved."""
    import ctypes
    import subprocess
    L = htf._lib
    names = sorted(set(re.findall(r"HTF_API[^;]*?\b(htf_\w+)\s*\(", _header())))
    assert names == sorted(L.CMT_PROTOTYPES) == ["htf_cmt_forces", "htf_cmt_grad"]
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and hasattr(L.lib, n)
        decl = re.search(r"HTF_API\s+\w+\s+%s\s*\(([^)]*)\)" % n, _header()).group(1)
        assert len(decl.split(",")) == len(L.CMT_PROTOTYPES[n][1]), n
    for t in (L.PROTOTYPES, L.STANDIN_PROTOTYPES, L.STEP_CHECK_PROTOTYPES, L.CG_PROTOTYPES, L.GEOM_PROTOTYPES, L.NLIST_PROTOTYPES,
              L.BP_PROTOTYPES, L.CF_PROTOTYPES, L.CT_PROTOTYPES, L.ANG_PROTOTYPES, L.AT_PROTOTYPES, L.CGHOST_PROTOTYPES):
        assert not set(names) & set(t)
    every = [n for n, _ in L.ALL_PROTOTYPES]
    assert set(names) <= set(every) and len(every) == len(set(every))
    assert len(L.BP_PROTOTYPES) == 4 and len(L.CF_PROTOTYPES) == 3
    assert raw.htf_abi_version() == 5 and L.ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {line.split()[-1] for line in nm.splitlines() if line.strip()}


def test_cmt_pybind_module_exports_table(htf):
    import importlib
    mod_path = os.path.join(os.path.dirname(htf._lib.LIB_PATH), "_htf_abi.so")
    if not os.path.exists(mod_path):
        pytest.skip("the pybind11 module is not built")
    mod = importlib.import_module("hoomd_tf_amd._htf_abi")
    for n in htf._lib.CMT_PROTOTYPES:
        assert hasattr(mod, n)


def test_cmt_header_is_plain_c():
    """include/htf_committee.h compiles as C99 beside htf_amd.h and htf_cforce.h."""
    import subprocess
    import tempfile
    from helpers import ROOT
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "htf_amd.h"\n#include "htf_cforce.h"\n#include "htf_committee.h"\n'
                             'int main(void){(void)htf_cmt_grad; (void)htf_cmt_forces; (void)htf_cf_grad; '
                             'return HTF_CMT_MAX_MODELS == 8 && HTF_CMT_MAX_LDS_BYTES == 163840u ? HTF_OK : 1;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_cmt_kernels_use_no_scratch(tmp_path):
    """Every instantiation of the two sweeps keeps to registers: no private segment, no vector-register spills.  The launchers'
    dispatch tables: pass 1 activation x cutoff x list x nlist dtype, pass 2 virial x cutoff x wide gather x nlist dtype; the
    number of members is a run-time argument of both.  Their names stay out of the other families' counts."""
    import test_codeobj as t
    if not (os.path.exists(t.LIB) and os.path.exists(t.READELF)):
        pytest.skip("library or llvm-readelf missing")
    meta = t._kernel_metadata(tmp_path)
    grad = [n for n in meta if "cmt_grad_kernel" in n]
    force = [n for n in meta if "cmt_force_kernel" in n]
    assert (len(grad), len(force)) == (16, 16)
    assert sorted(grad + force) == sorted(n for n in meta if "cmt_" in n)
    assert not [n for n in grad + force if any(s in n for s in FAMILY_SUBSTRINGS)]
    bad = {n: meta[n] for n in grad + force if meta[n]["private_segment_fixed_size"] or meta[n]["vgpr_spill_count"]}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the layer
def test_cmt_layer_argument_checks(htf):
    kw = dict(K=8, H1=8, H2=8, device="cpu", conservative=True)
    lay = htf.DescriptorMLP(n_models=3, **kw)
    assert lay.n_models == 3 and lay.conservative is True and lay.trainable is False and lay.deviation is None
    assert lay.w.numel() == 3 * lay.P
    assert htf.DescriptorMLP(n_models=np.int64(2), **kw).n_models == 2
    for bad in (0, 9, -1, 2.0, "2", True, None):
        with pytest.raises(ValueError, match="n_models.*total_forces"):
            htf.DescriptorMLP(n_models=bad, **kw)
    with pytest.raises(ValueError, match="conservative=True.*total_forces"):
        htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", n_models=2)
    with pytest.raises(NotImplementedError, match="l_max.*follow-up.*total_forces"):
        htf.DescriptorMLP(l_max=1, n_models=2, **kw)
    for tr in (True, "total", "angular"):
        with pytest.raises(NotImplementedError, match="trainable.*follow-up.*member"):
            htf.DescriptorMLP(trainable=tr, n_models=2, **kw)
    # the LDS budget of the first sweep: M networks, at construction, both byte counts in the message
    assert htf.DescriptorMLP.committee_lds_bytes(8, 16, 1, 32, 32) == 4 * (8 * 1684 + 16 + 1024)
    need = htf.DescriptorMLP.committee_lds_bytes(8, 64, 1, 64, 64)
    assert need == 4 * (8 * 8516 + 64 + 1024) > 160 * 1024
    with pytest.raises(ValueError, match=r"%d bytes.*%d bytes" % (need, 160 * 1024)):
        htf.DescriptorMLP(K=64, H1=64, H2=64, device="cpu", conservative=True, n_models=8)
    assert htf.DescriptorMLP(K=64, H1=64, H2=64, device="cpu", conservative=True, n_models=4).n_models == 4   # 4 x 34 KB fits
    # no CPU path, like total_forces of any layer; the single network's methods point to member(m)
    with pytest.raises(ValueError, match="device tensor"):
        lay.total_forces(torch.zeros((4, 16, 4)), torch.zeros((4, 16), dtype=torch.int32))
    x, labels = torch.zeros((4, 16, 4)), torch.zeros((4, 4))
    idx = torch.zeros((4, 16), dtype=torch.int32)
    for what, call in (("forces", lambda: lay.forces(x)), ("loss_gradient", lambda: lay.loss_gradient(x, labels)),
                       ("total_loss_gradient", lambda: lay.total_loss_gradient(x, labels, idx)),
                       ("angular_loss_gradient", lambda: lay.angular_loss_gradient(x, labels, idx)),
                       ("descriptor", lambda: lay.descriptor(htf.Nlist(x)))):
        with pytest.raises(NotImplementedError, match=r"member\(m\)\.%s" % what):
            call()
    with pytest.raises(NotImplementedError, match="follow-up.*member"):
        lay.total_forces(x, idx, n_ghost=2, halo=lambda t: None)
    with pytest.raises(ValueError, match="committee"):
        htf.DescriptorMLP(**kw).total_forces(x, idx, members=True)


def test_cmt_config(htf):
    kw = dict(K=8, H1=8, H2=8, device="cpu")
    assert "n_models" not in htf.DescriptorMLP(**kw).get_config()
    assert "n_models" not in htf.DescriptorMLP(n_models=1, conservative=True, **kw).get_config()
    cfg = htf.DescriptorMLP(n_models=4, conservative=True, r_cut=2.5, n_species=2, **kw).get_config()
    assert cfg["n_models"] == 4 and cfg["conservative"] is True and cfg["n_species"] == 2
    again = htf.DescriptorMLP(device="cpu", **cfg)
    assert again.n_models == 4 and again.get_config() == cfg


@pytest.mark.parametrize("S", [1, 2])
def test_cmt_weights_round_trip(htf, tmp_path, S):
    """w holds [M][S][P] floats, member m and species s from mlp_params(seed + m S + s); the six arrays carry a leading axis of
    length M, ahead of the species axis."""
    from hoomd_tf_amd.initializers import mlp_params
    M = 3
    lay = htf.DescriptorMLP(K=8, H1=6, H2=5, n_types=2, device="cpu", conservative=True, n_models=M, n_species=S, seed=7)
    P = lay.P
    assert lay.w.shape == (M * S * P,)
    lead = (M, S) if S > 1 else (M,)
    ws = lay.get_weights()
    assert [w.shape for w in ws] == [lead + tuple(sh) for sh in lay._shapes]
    for m in range(M):
        for s in range(S):
            ref = mlp_params(seed=7 + m * S + s, K=16, H1=6, H2=5)
            flat = np.concatenate([ref[k].ravel() for k in lay._KEYS]).astype(np.float32)
            assert np.array_equal(lay.w[(m * S + s) * P:(m * S + s + 1) * P].numpy(), flat)
            for k, w in zip(lay._KEYS, ws):
                assert np.array_equal(w[(m, s) if S > 1 else (m,)], ref[k].astype(np.float32))
    rng = np.random.default_rng(1)
    new = [rng.standard_normal(w.shape).astype(np.float32) for w in ws]
    ptr = lay.w.data_ptr()
    lay.set_weights(new)
    assert lay.w.data_ptr() == ptr and all(np.array_equal(a, b) for a, b in zip(lay.get_weights(), new))
    with pytest.raises(ValueError, match="shape mismatch"):
        lay.set_weights([w[0] for w in new])
    path = str(tmp_path / "w.npz")
    lay.save_weights(path)
    other = htf.DescriptorMLP(K=8, H1=6, H2=5, n_types=2, device="cpu", conservative=True, n_models=M, n_species=S)
    other.load_weights(path)
    assert torch.equal(other.w, lay.w)


def test_cmt_member_is_a_view(htf):
    M, S = 3, 2
    lay = htf.DescriptorMLP(K=8, H1=6, H2=5, device="cpu", conservative=True, r_cut=2.0, n_models=M, n_species=S)
    P = lay.P
    for m in range(M):
        one = lay.member(m)
        assert one.w.data_ptr() == lay.w.data_ptr() + 4 * m * S * P and one.w.numel() == S * P
        assert one.n_models == 1 and one.trainable is False and one.deviation is None
        cfg = lay.get_config()
        del cfg["n_models"]
        assert one.get_config() == cfg
        assert all(np.array_equal(a, b[m]) for a, b in zip(one.get_weights(), lay.get_weights()))
    one = lay.member(1, trainable="total")
    assert one.trainable == "total" and one.conservative is True
    with torch.no_grad():
        one.w.add_(1.0)   # in place on the view: the committee's own weights
    assert float((lay.get_weights()[1][1] - one.get_weights()[1]).max()) == 0.0
    for bad in (-1, M, 1.5, True):
        with pytest.raises(ValueError, match="member"):
            lay.member(bad)


# ------------------------------------------------------------------------------------------------ the entry points
def _args(htf):
    L = htf._lib
    mu = torch.zeros(8)
    P = 8 * 8 + 8 + 8 * 8 + 8 + 8 + 1
    w = torch.zeros(2 * P)
    return L, (mu, w), dict(nlist=0x1000, dt=L.HTF_F32, B=4, NN=16, K=8, T=1, H1=8, H2=8, act=L.ACT_TANH, w=w.data_ptr(),
                            mu=mu.data_ptr(), gap=0.5, g=0x2000, e=0x3000, rows=None, n_rows=4, rc=0.0, index=0x4000,
                            types=None, out=0x5000, odt=L.HTF_F32, vir=None, M=2, stride=P, dev=0x6000, mem=None)


COMMON_BAD = (dict(K=1), dict(K=33, T=2), dict(NN=257), dict(gap=0.0), dict(dt=5), dict(mu=None), dict(nlist=None),
              dict(rc=-1.0), dict(rc=float("nan")), dict(g=None), dict(e=None), dict(M=0), dict(M=1), dict(M=9))


def test_cmt_grad_entry_point_argument_errors(htf):
    """The C checks (no launch, no device needed): status HTF_ERR_INVALID and a message."""
    L, keep, args = _args(htf)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_cmt_grad(a["nlist"], a["dt"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"], a["w"], a["mu"],
                                  a["gap"], a["g"], a["e"], a["rows"], a["n_rows"], a["rc"], a["M"], a["stride"], None)

    for bad in COMMON_BAD + (dict(H1=0), dict(H2=65), dict(act=7), dict(w=None), dict(n_rows=5), dict(stride=args["stride"] - 1)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    # over the LDS budget: refused without a launch, both byte counts in the message
    assert call(K=64, H1=64, H2=64, M=8, stride=1 << 20) == L.HTF_ERR_INVALID
    assert "%d bytes" % htf.DescriptorMLP.committee_lds_bytes(8, 64, 1, 64, 64) in L.last_error() and "163840" in L.last_error()
    # no rows: HTF_OK, nothing launched; the limits are still checked
    assert call(B=0, n_rows=0, nlist=None, g=None, e=None) == L.HTF_OK
    assert call(n_rows=0) == L.HTF_OK
    assert call(B=0, n_rows=0, nlist=None, g=None, e=None, M=9) == L.HTF_ERR_INVALID


def test_cmt_forces_entry_point_argument_errors(htf):
    L, keep, args = _args(htf)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_cmt_forces(a["nlist"], a["dt"], a["index"], a["types"], a["B"], a["NN"], a["K"], a["T"], a["mu"], a["gap"],
                                    a["g"], a["e"], a["out"], a["odt"], a["vir"], a["rc"], a["M"], a["dev"], a["mem"], None)

    for bad in COMMON_BAD + (dict(odt=3), dict(out=None), dict(index=None), dict(T=2), dict(dev=None)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    assert call(B=0, nlist=None, index=None, g=None, e=None, out=None, dev=None) == L.HTF_OK
    assert call(B=0, nlist=None, index=None, g=None, e=None, out=None, dev=None, NN=257) == L.HTF_ERR_INVALID
