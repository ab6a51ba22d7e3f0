"""Force matching on the conservative forces of htf.DescriptorMLP on the host: the C ABI table of include/htf_ctrain.h, the
header as C99, the code objects of the sweep, the layer's ``trainable="total"`` value and the argument checks of the entry
point.  No GPU."""
import os
import re

import pytest
import torch


def _header():
    from helpers import ROOT
    return open(os.path.join(ROOT, "include", "htf_ctrain.h")).read()


def test_ct_abi_table(htf):
    """The symbols of include/htf_ctrain.h are CT_PROTOTYPES: exported, bound under the active binding, argument for argument,
    and no name is shared with another table.  The ABI version has not moved."""
    import ctypes
    import subprocess
    L = htf._lib
    names = sorted(set(re.findall(r"HTF_API[^;]*?\b(htf_\w+)\s*\(", _header())))
    assert names == sorted(L.CT_PROTOTYPES) == ["htf_ct_loss_grad"]
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and hasattr(L.lib, n)
        decl = re.search(r"HTF_API\s+\w+\s+%s\s*\(([^)]*)\)" % n, _header()).group(1)
        assert len(decl.split(",")) == len(L.CT_PROTOTYPES[n][1]) == 20, n
    for t in (L.PROTOTYPES, L.STANDIN_PROTOTYPES, L.STEP_CHECK_PROTOTYPES, L.CG_PROTOTYPES, L.GEOM_PROTOTYPES, L.NLIST_PROTOTYPES,
              L.BP_PROTOTYPES, L.CF_PROTOTYPES):
        assert not set(names) & set(t)
    every = [n for n, _ in L.ALL_PROTOTYPES]
    assert set(names) <= set(every) and len(every) == len(set(every))
    assert len(L.BP_PROTOTYPES) == 4 and len(L.CF_PROTOTYPES) == 3 and raw.htf_abi_version() == 5 and L.ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {line.split()[-1] for line in nm.splitlines() if line.strip()}


def test_ct_pybind_module_exports_table(htf):
    import importlib
    mod_path = os.path.join(os.path.dirname(htf._lib.LIB_PATH), "_htf_abi.so")
    if not os.path.exists(mod_path):
        pytest.skip("the pybind11 module is not built")
    mod = importlib.import_module("hoomd_tf_amd._htf_abi")
    for n in htf._lib.CT_PROTOTYPES:
        assert hasattr(mod, n)


def test_ct_header_is_plain_c():
    """include/htf_ctrain.h compiles as C99 beside htf_bp.h and htf_cforce.h."""
    import subprocess
    import tempfile
    from helpers import ROOT
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "htf_amd.h"\n#include "htf_bp.h"\n#include "htf_cforce.h"\n#include "htf_ctrain.h"\n'
                             'int main(void){int (*f)(const void *, int, const int *, unsigned, unsigned, unsigned, unsigned, '
                             'unsigned, unsigned, int, const float *, const float *, float, const float *, float *, float *, '
                             'const int *, unsigned, float, htf_stream) = htf_ct_loss_grad; (void)f; return HTF_OK;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_ct_kernels_use_no_scratch(tmp_path):
    """Every instantiation of the sweep -- activation x cutoff x list x nlist dtype -- keeps to registers: no private segment,
    no vector-register spills; its name stays out of the row sweep's census, and the library keeps one reduction kernel."""
    import test_codeobj as t
    if not (os.path.exists(t.LIB) and os.path.exists(t.READELF)):
        pytest.skip("library or llvm-readelf missing")
    meta = t._kernel_metadata(tmp_path)
    sweep = [n for n in meta if "ct_sweep_kernel" in n]
    assert len(sweep) == 16
    assert not [n for n in sweep if "bp_" in n or "dtrain_" in n or "desc_mlp" in n or "cf_" in n]
    assert len([n for n in meta if "dtrain_reduce_kernel" in n]) == 1
    bad = {n: meta[n] for n in sweep if meta[n]["private_segment_fixed_size"] or meta[n]["vgpr_spill_count"]}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the layer
def test_ct_layer_trainable_total(htf):
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable="total")
    assert lay.trainable == "total" and lay.conservative is True
    cfg = lay.get_config()
    assert cfg["trainable"] == "total" and cfg["conservative"] is True
    again = htf.DescriptorMLP(device="cpu", **cfg)
    assert again.trainable == "total" and again.conservative is True and again.get_config() == cfg
    # the value alone implies the conservative forces
    assert htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable="total", conservative=False).conservative is True
    full = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable="total", r_cut=2.5, n_species=2).get_config()
    assert htf.DescriptorMLP(device="cpu", **full).get_config() == full
    # the row operator's sweep still does not go with the conservative forces, and the message names the way out
    with pytest.raises(ValueError, match="conservative") as info:
        htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True, trainable=True)
    assert 'trainable="total"' in str(info.value)
    with pytest.raises(ValueError, match="trainable"):
        htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable="forces")
    # True and False are what they were
    assert htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable=True).get_config()["trainable"] is True
    assert htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True).trainable is False
    # what the optimizer step asks of a trainable layer
    d = htf.optimizers.SGD(0.1).desc(lay.nonneg_mask, lay.l1_reg)
    assert d.nonneg_mask == 0 and d.l1_reg[0] == 0.0


def test_ct_total_loss_gradient_has_no_cpu_path(htf):
    """Callable on any layer, like total_forces; no CPU path, like loss_gradient."""
    for kw in (dict(trainable="total"), dict(conservative=True), dict()):
        lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", **kw)
        with pytest.raises(ValueError, match="device tensor"):
            lay.total_loss_gradient(torch.zeros((4, 16, 4)), torch.zeros((4, 4)), torch.zeros((4, 16), dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ the entry point
def test_ct_loss_grad_entry_point_argument_errors(htf):
    """The C checks (no launch, no device needed): htf_bp_loss_grad's, and the index."""
    L = htf._lib
    mu = torch.zeros(8)
    w = torch.zeros(8 * 8 + 8 + 8 * 8 + 8 + 8 + 1)
    args = dict(nlist=0x1000, dt=L.HTF_F32, index=0x6000, B=4, NN=16, K=8, T=1, H1=8, H2=8, act=L.ACT_TANH, w=w.data_ptr(),
                mu=mu.data_ptr(), gap=0.5, rho=0x3000, accum=0x4000, scratch=0x5000, rows=None, n_rows=4, rc=0.0)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_ct_loss_grad(a["nlist"], a["dt"], a["index"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"],
                                      a["w"], a["mu"], a["gap"], a["rho"], a["accum"], a["scratch"], a["rows"], a["n_rows"], a["rc"],
                                      None)

    for bad in (dict(K=1), dict(K=33, T=2), dict(NN=257), dict(gap=0.0), dict(gap=-1.0), dict(dt=5), dict(mu=None), dict(nlist=None),
                dict(n_rows=5), dict(rc=-1.0), dict(rc=float("nan")), dict(rc=float("inf")), dict(rc=-float("inf")), dict(H1=0),
                dict(H2=65), dict(act=7), dict(w=None), dict(rho=None), dict(accum=None), dict(scratch=None), dict(index=None),
                dict(B=0, w=None), dict(B=0, n_rows=1)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    # B = 0: HTF_OK with no row pointer to read and, without an accum to zero-fill, no launch; the limits are still checked
    none = dict(B=0, n_rows=0, nlist=None, index=None, rho=None, accum=None, scratch=None)
    assert call(**none) == L.HTF_OK
    assert call(K=1, **none) == L.HTF_ERR_INVALID and "descriptor network" in L.last_error()
