"""The descriptor network on the host: the C ABI table of include/htf_desc.h, the header as C99, the argument and shape
checks of htf.DescriptorMLP and of the entry points, and the weights API (get/set, save/load, through SimModel).  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

_KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")


def _header():
    from helpers import ROOT
    return open(os.path.join(ROOT, "include", "htf_desc.h")).read()


def test_desc_abi_table(htf):
    """A sixth table: the symbols of include/htf_desc.h, exported by the library, bound under the active binding, sharing
    no name with the other five tables."""
    import ctypes
    names = sorted(set(re.findall(r"HTF_API[^;]*?\b(htf_desc_\w+)\s*\(", _header())))
    assert names == sorted(htf._lib.DESC_PROTOTYPES) and len(names) == 2
    raw = ctypes.CDLL(htf._lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and hasattr(htf._lib.lib, n)
    L = htf._lib
    others = [L.PROTOTYPES, L.STANDIN_PROTOTYPES, L.CG_PROTOTYPES, L.GEOM_PROTOTYPES, L.NLIST_PROTOTYPES]
    for t in others:
        assert not set(names) & set(t)
    # the argument counts match the header's declarations
    for n in names:
        decl = re.search(r"HTF_API\s+int\s+%s\s*\(([^)]*)\)" % n, _header()).group(1)
        assert len(decl.split(",")) == len(L.DESC_PROTOTYPES[n][1]), n


def test_desc_pybind_module_exports_table(htf):
    import importlib
    mod_path = os.path.join(os.path.dirname(htf._lib.LIB_PATH), "_htf_abi.so")
    if not os.path.exists(mod_path):
        pytest.skip("the pybind11 module is not built")
    mod = importlib.import_module("hoomd_tf_amd._htf_abi")
    for n in htf._lib.DESC_PROTOTYPES:
        assert hasattr(mod, n)


def test_desc_header_is_plain_c():
    """include/htf_desc.h compiles as C99 beside htf_amd.h."""
    import subprocess
    import tempfile
    from helpers import ROOT
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "htf_amd.h"\n#include "htf_desc.h"\n'
                             'int main(void){int (*f)(const void *, int, unsigned, unsigned, unsigned, unsigned, const float *, float, '
                             'void *, int, htf_stream) = htf_desc_descriptor; (void)f; (void)htf_desc_forces; return HTF_OK;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


@pytest.mark.parametrize("kw", [dict(K=33, n_types=2), dict(K=16, n_types=5), dict(K=65), dict(K=1), dict(H1=65), dict(H2=0),
                                dict(H2=65), dict(low=2.0, high=2.0), dict(low=3.0, high=1.0), dict(activation="relu"),
                                dict(n_types=0)])
def test_desc_layer_limits(htf, kw):
    with pytest.raises(ValueError):
        htf.DescriptorMLP(device="cpu", **kw)


def test_desc_layer_limits_at_the_edge(htf):
    """D = 64 and H = 64 are inside: one channel and one hidden unit per lane."""
    lay = htf.DescriptorMLP(K=16, n_types=4, H1=64, H2=64, device="cpu")
    assert lay.D == 64 and lay.w.numel() == 64 * 64 + 64 + 64 * 64 + 64 + 64 + 1
    lay = htf.DescriptorMLP(K=64, H1=1, H2=1, activation=None, device="cpu")
    assert lay.activation == "linear"


def test_desc_call_checks(htf):
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu")
    with pytest.raises(ValueError):
        lay(torch.zeros((4, 257, 4)))               # more than four slots per lane
    with pytest.raises(ValueError):
        lay(torch.zeros((4, 16, 3)))
    e = lay(torch.zeros((4, 256, 4)))
    with pytest.raises(ValueError):
        lay.forces(torch.zeros((4, 16, 4)))         # no CPU path
    with pytest.raises(ValueError):
        lay.descriptor(torch.zeros((4, 16, 4)))
    assert isinstance(e, htf.simmodel.DescriptorEnergy) and e.reduced


def test_desc_energy_does_not_combine(htf):
    """The layer's energy takes no part in arithmetic, in either order, with constants or with other energies: a sum the
    kernel cannot form never reaches compute_nlist_forces as wrong forces."""
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu")
    nl = htf.Nlist(torch.zeros((4, 16, 4)))
    e = lay(nl)
    lj_pair = 4.0 * (htf.nlist_rinv(nl) ** 12 - htf.nlist_rinv(nl) ** 6)
    lj = htf.reduce_sum(lj_pair, axis=1)
    for f in (lambda: e + 1.0, lambda: 1.0 + e, lambda: 2.0 * e, lambda: e * 2.0, lambda: -e, lambda: e - 1.0, lambda: e / 2.0,
              lambda: e + e, lambda: e + lj, lambda: e + lj_pair):
        with pytest.raises(TypeError):
            f()
    for f in (lambda: lj + e, lambda: lj_pair + e, lambda: lj - e):
        with pytest.raises((TypeError, RuntimeError)):
            f()


def test_desc_entry_point_argument_errors(htf):
    """The C checks (no launch, no device needed): status HTF_ERR_INVALID and a message."""
    L = htf._lib
    lib = L.lib
    mu = torch.zeros(8)
    w = torch.zeros(8 * 8 + 8 + 8 * 8 + 8 + 8 + 1)
    args = dict(nlist=0x1000, dt=L.HTF_F32, B=4, NN=16, K=8, T=1, H1=8, H2=8, act=L.ACT_TANH, w=w.data_ptr(), mu=mu.data_ptr(),
                gap=0.5, out=0x2000, odt=L.HTF_F32)

    def call(**kw):
        a = dict(args, **kw)
        return lib.htf_desc_forces(a["nlist"], a["dt"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"], a["w"], a["mu"],
                                   a["gap"], a["out"], a["odt"], None, None)

    for bad in (dict(K=1), dict(K=33, T=2), dict(NN=257), dict(H1=0), dict(H2=65), dict(act=7), dict(gap=0.0), dict(gap=-1.0),
                dict(dt=5), dict(odt=3), dict(mu=None), dict(w=None), dict(nlist=None), dict(out=None)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    # zero rows: nothing to launch, no pointer to read
    assert call(B=0, nlist=None, out=None) == L.HTF_OK
    assert lib.htf_desc_descriptor(None, L.HTF_F32, 0, 16, 8, 1, mu.data_ptr(), 0.5, None, L.HTF_F32, None) == L.HTF_OK
    assert lib.htf_desc_descriptor(None, L.HTF_F32, 3, 16, 8, 1, mu.data_ptr(), 0.5, None, L.HTF_F32, None) == L.HTF_ERR_INVALID


def test_desc_weights_follow_mlp_params(htf):
    from hoomd_tf_amd.initializers import mlp_params
    lay = htf.DescriptorMLP(K=6, n_types=3, H1=10, H2=7, seed=11, device="cpu")
    ref = mlp_params(seed=11, K=18, H1=10, H2=7)
    got = lay.get_weights()
    assert [g.shape for g in got] == [ref[k].shape for k in _KEYS]
    for g, k in zip(got, _KEYS):
        np.testing.assert_array_equal(g, ref[k])
    # the centres and spacing are RBFExpansion's
    rbf = htf.RBFExpansion(0.0, 3.0, 6)
    np.testing.assert_array_equal(lay.centers, rbf.centers)
    assert lay.gap == rbf.gap
    np.testing.assert_array_equal(lay.mu.numpy(), rbf.centers)


def test_desc_weights_round_trip(htf, tmp_path):
    lay = htf.DescriptorMLP(K=8, H1=12, H2=9, device="cpu")
    rng = np.random.default_rng(4)
    new = [rng.standard_normal(w.shape).astype(np.float32) for w in lay.get_weights()]
    w_before = lay.w
    lay.set_weights(new)
    assert lay.w is w_before                        # in place: whoever holds w sees the new values
    for a, b in zip(lay.get_weights(), new):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(lay.w.numpy(), np.concatenate([x.ravel() for x in new]))
    p = str(tmp_path / "desc.npz")
    lay.save_weights(p)
    other = htf.DescriptorMLP(K=8, H1=12, H2=9, seed=99, device="cpu")
    other.load_weights(p)
    for a, b in zip(other.get_weights(), new):
        np.testing.assert_array_equal(a, b)
    # an in-place write to w is what get_weights reports
    with torch.no_grad():
        lay.w[0] += 1.0
    assert lay.get_weights()[0][0, 0] == new[0][0, 0] + np.float32(1.0)
    with pytest.raises(ValueError):
        lay.set_weights(new[:5])
    with pytest.raises(ValueError):
        lay.set_weights([new[0].T] + new[1:])


def test_desc_weights_through_simmodel(htf, tmp_path):
    class M(htf.SimModel):
        def setup(self):
            self.desc = htf.DescriptorMLP(K=4, H1=5, H2=3, seed=2, device="cpu")

        def compute(self, nlist):
            return htf.compute_nlist_forces(nlist, self.desc(nlist))

    m = M(16)
    ws = m.get_weights()
    assert len(ws) == 6 and ws[0].shape == (4, 5) and ws[4].shape == (3, 1)
    new = [w + np.float32(0.5) for w in ws]
    m.set_weights(new)
    for a, b in zip(m.desc.get_weights(), new):
        np.testing.assert_array_equal(a, b)
    p = str(tmp_path / "m")
    m.save_weights(p)
    m2 = M(16)
    m2.load_weights(p)
    for a, b in zip(m2.get_weights(), new):
        np.testing.assert_array_equal(a, b)


def test_desc_kernels_use_no_scratch(tmp_path):
    """Every instantiation of desc_mlp_kernel keeps to registers: no private segment, no vector-register spills."""
    import test_codeobj as t
    if not (os.path.exists(t.LIB) and os.path.exists(t.READELF)):
        pytest.skip("library or llvm-readelf missing")
    meta = t._kernel_metadata(tmp_path)
    ks = [n for n in meta if "desc_mlp_kernel" in n]
    assert len(ks) == 10           # 8 force forms (activation x virial x nlist dtype) + 2 descriptor-only
    bad = {n: meta[n] for n in ks if meta[n]["private_segment_fixed_size"] or meta[n]["vgpr_spill_count"]}
    assert not bad, bad
