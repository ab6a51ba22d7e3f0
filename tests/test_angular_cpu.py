"""The angular channels of htf.DescriptorMLP on the host: the C ABI table of include/htf_angular.h, the header as C99, the code
objects of the three kernels, the layer's ``l_max`` argument and the argument checks of the entry points.  No GPU."""
import os
import re

import pytest
import torch


def _header():
    from helpers import ROOT
    return open(os.path.join(ROOT, "include", "htf_angular.h")).read()


def test_ang_abi_table(htf):
    """The symbols of include/htf_angular.h are ANG_PROTOTYPES: exported, bound under the active binding, argument for argument,
    and no name is shared with another table.  The older tables keep their sizes and the ABI version has not moved."""
    import ctypes
    import subprocess
    L = htf._lib
    names = sorted(set(re.findall(r"HTF_API[^;]*?\b(htf_\w+)\s*\(", _header())))
    assert names == sorted(L.ANG_PROTOTYPES) == ["htf_ang_descriptor", "htf_ang_forces", "htf_ang_grad"]
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and hasattr(L.lib, n)
        decl = re.search(r"HTF_API\s+\w+\s+%s\s*\(([^)]*)\)" % n, _header()).group(1)
        assert len(decl.split(",")) == len(L.ANG_PROTOTYPES[n][1]), n
    for t in (L.PROTOTYPES, L.STANDIN_PROTOTYPES, L.STEP_CHECK_PROTOTYPES, L.CG_PROTOTYPES, L.GEOM_PROTOTYPES, L.NLIST_PROTOTYPES,
              L.BP_PROTOTYPES, L.CF_PROTOTYPES, L.CT_PROTOTYPES):
        assert not set(names) & set(t)
    every = [n for n, _ in L.ALL_PROTOTYPES]
    assert set(names) <= set(every) and len(every) == len(set(every))
    assert (len(L.BP_PROTOTYPES), len(L.CF_PROTOTYPES), len(L.CT_PROTOTYPES)) == (4, 3, 1)
    assert raw.htf_abi_version() == 5 and L.ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {line.split()[-1] for line in nm.splitlines() if line.strip()}
    mod_path = os.path.join(os.path.dirname(L.LIB_PATH), "_htf_abi.so")
    if os.path.exists(mod_path):   # the pybind11 module, where built, exports the table too
        import importlib
        mod = importlib.import_module("hoomd_tf_amd._htf_abi")
        assert all(hasattr(mod, n) for n in names)


def test_ang_header_is_plain_c():
    """include/htf_angular.h compiles as C99 beside htf_amd.h, htf_bp.h and htf_cforce.h."""
    import subprocess
    import tempfile
    from helpers import ROOT
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "htf_amd.h"\n#include "htf_bp.h"\n#include "htf_cforce.h"\n#include "htf_angular.h"\n'
                             'int main(void){int (*f)(const void *, int, unsigned, unsigned, unsigned, unsigned, const float *, float, '
                             'void *, int, float, unsigned, htf_stream) = htf_ang_descriptor; (void)f; (void)htf_ang_grad; '
                             '(void)htf_ang_forces; return HTF_OK;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_ang_kernels_use_no_scratch(tmp_path):
    """Every instantiation of the three kernels keeps to registers: no private segment, no vector-register spills.  Pass 1:
    activation x cutoff x l_max x nlist dtype; pass 2: virial x cutoff x l_max x nlist dtype; the descriptor: cutoff x l_max x
    nlist dtype.  None of their names collides with what the older tests count."""
    import test_codeobj as t
    if not (os.path.exists(t.LIB) and os.path.exists(t.READELF)):
        pytest.skip("library or llvm-readelf missing")
    meta = t._kernel_metadata(tmp_path)
    grad = [n for n in meta if "ang_grad_kernel" in n]
    force = [n for n in meta if "ang_force_kernel" in n]
    desc = [n for n in meta if "ang_desc_kernel" in n]
    assert (len(grad), len(force), len(desc)) == (16, 16, 8)
    ks = grad + force + desc
    assert sorted(ks) == sorted(n for n in meta if "ang_" in n)
    banned = ("bp_", "dtrain_", "desc_mlp", "cf_grad_kernel", "cf_pair_force_kernel", "cf_pair_kernel", "ct_sweep_kernel")
    assert not [n for n in ks if any(b in n for b in banned)]
    bad = {n: meta[n] for n in ks if meta[n]["private_segment_fixed_size"] or meta[n]["vgpr_spill_count"]}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the layer
def test_ang_layer_argument_checks(htf):
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True, l_max=2)
    assert (lay.l_max, lay.Dr, lay.D) == (2, 8, 24) and lay.conservative is True
    assert lay.get_weights()[0].shape == (24, 8) and lay.P == 24 * 8 + 8 + 8 * 8 + 8 + 8 + 1
    with pytest.raises(ValueError, match="l_max"):
        htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True, l_max=3)
    with pytest.raises(ValueError, match="l_max"):
        htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True, l_max=-1)
    with pytest.raises(ValueError, match="l_max"):   # 32 * 3 = 96 inputs, over MAX_D
        htf.DescriptorMLP(K=32, H1=8, H2=8, device="cpu", conservative=True, l_max=2)
    assert htf.DescriptorMLP(K=32, H1=8, H2=8, device="cpu", conservative=True, l_max=1).D == 64
    assert htf.DescriptorMLP(K=7, n_types=3, H1=8, H2=8, device="cpu", conservative=True, l_max=2).D == 63
    with pytest.raises(ValueError, match="conservative"):
        htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", l_max=1)
    for tr in (True, "total"):
        with pytest.raises(NotImplementedError, match="follow-up"):
            htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=(tr == "total"), l_max=1, trainable=tr)
    # the row operator has no angular form
    x = torch.zeros((4, 16, 4))
    with pytest.raises(ValueError, match="angular"):
        lay.forces(x)
    with pytest.raises(ValueError, match="angular"):
        lay.loss_gradient(x, torch.zeros((4, 4)))
    with pytest.raises(NotImplementedError, match="follow-up"):
        lay.total_loss_gradient(x, torch.zeros((4, 4)), torch.zeros((4, 16), dtype=torch.int32))
    # no CPU path, like total_forces() of the radial layer
    with pytest.raises(ValueError, match="device tensor"):
        lay.total_forces(x, torch.zeros((4, 16), dtype=torch.int32))
    with pytest.raises(ValueError, match="device tensor"):
        lay.descriptor(x)
    # weights of the right input width load, others do not
    ws = lay.get_weights()
    lay.set_weights(ws)
    with pytest.raises(ValueError, match="shape"):
        lay.set_weights([ws[0][:8]] + ws[1:])


def test_ang_config(htf):
    cfg = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", r_cut=2.5, conservative=True, l_max=2).get_config()
    assert cfg["l_max"] == 2 and cfg["conservative"] is True and cfg["r_cut"] == 2.5
    again = htf.DescriptorMLP(device="cpu", **cfg)
    assert again.l_max == 2 and again.D == 24 and again.get_config() == cfg
    # l_max = 0 is the layer as it was: the same configuration, widths and weights
    plain = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu")
    assert plain.get_config() == {'K': 8, 'H1': 8, 'H2': 8, 'low': 0.0, 'high': 3.0, 'n_types': 1, 'activation': 'tanh'}
    zero = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True, l_max=0)
    ref = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True)
    assert "l_max" not in zero.get_config() and zero.get_config() == ref.get_config()
    assert zero.D == ref.D == 8 and torch.equal(zero.w, ref.w)


# ------------------------------------------------------------------------------------------------ the entry points
def _args(htf, l_max=1):
    L = htf._lib
    D = 8 * (1 + l_max)
    mu = torch.zeros(8)
    w = torch.zeros(D * 8 + 8 + 8 * 8 + 8 + 8 + 1)
    return L, (mu, w), dict(nlist=0x1000, dt=L.HTF_F32, B=4, NN=16, K=8, T=1, H1=8, H2=8, act=L.ACT_TANH, w=w.data_ptr(),
                            mu=mu.data_ptr(), gap=0.5, h=0x2000, e=0x3000, rows=None, n_rows=4, rc=0.0, index=0x4000,
                            types=None, out=0x5000, odt=L.HTF_F32, vir=None, lm=l_max)


# K n_types (1 + l_max) over 64: 65 itself has no factor 2 or 3, so with l_max in {1, 2} the smallest product over the limit is
# 66 (33 * 2, 11 * 2 * 3); 65 = 13 * 5 radial channels (130 inputs) is refused as well
COMMON_BAD = (dict(K=1), dict(K=33, T=2), dict(NN=257), dict(gap=0.0), dict(gap=-1.0), dict(dt=5), dict(mu=None), dict(nlist=None),
              dict(rc=-1.0), dict(rc=float("nan")), dict(rc=float("inf")), dict(lm=0), dict(lm=3),
              dict(K=33, T=1, lm=1), dict(K=11, T=2, lm=2), dict(K=11, T=3, lm=1), dict(K=22, T=1, lm=2), dict(K=13, T=5, lm=1))


def test_ang_input_limit(htf):
    """64 and 63 network inputs pass the checks (no rows: nothing is launched), 66 do not, and the message names l_max."""
    L, keep, args = _args(htf)

    def call(K, T, lm):
        return L.lib.htf_ang_descriptor(None, L.HTF_F32, 0, 16, K, T, args["mu"], 0.5, None, L.HTF_F32, 0.0, lm, None)

    for K, T, lm in ((32, 1, 1), (21, 1, 2), (16, 2, 1), (7, 3, 2)):
        assert call(K, T, lm) == L.HTF_OK
    for K, T, lm in ((33, 1, 1), (11, 2, 2), (11, 3, 1), (22, 1, 2)):
        assert K * T * (1 + lm) == 66 and call(K, T, lm) == L.HTF_ERR_INVALID
        assert "descriptor network" in L.last_error() and "l_max" in L.last_error()
    assert call(13, 5, 1) == L.HTF_ERR_INVALID


def test_ang_grad_entry_point_argument_errors(htf):
    """The C checks (no launch, no device needed): status HTF_ERR_INVALID and a message."""
    L, keep, args = _args(htf)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_ang_grad(a["nlist"], a["dt"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"], a["w"], a["mu"],
                                  a["gap"], a["h"], a["e"], a["rows"], a["n_rows"], a["rc"], a["lm"], None)

    for bad in COMMON_BAD + (dict(h=None), dict(e=None), dict(h=0x2004), dict(H1=0), dict(H2=65), dict(act=7), dict(w=None),
                             dict(n_rows=5), dict(B=0, n_rows=1)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    # no rows: HTF_OK, nothing launched; the limits are still checked
    assert call(B=0, n_rows=0, nlist=None, h=None, e=None) == L.HTF_OK
    assert call(n_rows=0) == L.HTF_OK and call(n_rows=0, rc=2.5, rows=0x6000, lm=2) == L.HTF_OK
    assert call(B=0, n_rows=0, nlist=None, h=None, e=None, K=1) == L.HTF_ERR_INVALID
    assert call(B=0, n_rows=0, nlist=None, h=None, e=None, lm=0) == L.HTF_ERR_INVALID


def test_ang_forces_entry_point_argument_errors(htf):
    L, keep, args = _args(htf)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_ang_forces(a["nlist"], a["dt"], a["index"], a["types"], a["B"], a["NN"], a["K"], a["T"], a["mu"], a["gap"],
                                    a["h"], a["e"], a["out"], a["odt"], a["vir"], a["rc"], a["lm"], None)

    for bad in COMMON_BAD + (dict(h=None), dict(e=None), dict(h=0x2008), dict(odt=3), dict(out=None), dict(index=None),
                             dict(T=2)):   # (T = 2 without the rows' types)
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    assert call(B=0, nlist=None, index=None, h=None, e=None, out=None) == L.HTF_OK
    assert call(B=0, nlist=None, index=None, h=None, e=None, out=None, T=2, lm=2) == L.HTF_OK
    assert call(B=0, nlist=None, index=None, h=None, e=None, out=None, NN=257) == L.HTF_ERR_INVALID
    assert call(B=0, nlist=None, index=None, h=None, e=None, out=None, lm=3) == L.HTF_ERR_INVALID


def test_ang_descriptor_entry_point_argument_errors(htf):
    L, keep, args = _args(htf)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_ang_descriptor(a["nlist"], a["dt"], a["B"], a["NN"], a["K"], a["T"], a["mu"], a["gap"], a["out"], a["odt"],
                                        a["rc"], a["lm"], None)

    for bad in COMMON_BAD + (dict(odt=3), dict(out=None)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    assert call(B=0, nlist=None, out=None) == L.HTF_OK and call(B=0, nlist=None, out=None, lm=2, rc=2.5) == L.HTF_OK
    assert call(B=0, nlist=None, out=None, lm=0) == L.HTF_ERR_INVALID
