"""Force matching for the descriptor network on the host: the C ABI table of include/htf_desc_train.h, the header as C99, the
code object of the sweep, the ``trainable`` flag of htf.DescriptorMLP and the argument checks of the entry point.  No GPU."""
import os
import re

import pytest
import torch


def _header():
    from helpers import ROOT
    return open(os.path.join(ROOT, "include", "htf_desc_train.h")).read()


def test_desc_train_abi_table(htf):
    """A seventh table: the symbols of include/htf_desc_train.h, exported by the library, bound under the active binding,
    sharing no name with the other six tables; the ABI version has not moved."""
    import ctypes
    L = htf._lib
    names = sorted(set(re.findall(r"HTF_API[^;]*?\b(htf_\w+)\s*\(", _header())))
    assert names == sorted(L.DESC_TRAIN_PROTOTYPES) and len(names) == 2
    assert all(n.startswith("htf_dtrain_") for n in names)
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and hasattr(L.lib, n)
    for t in (L.PROTOTYPES, L.STANDIN_PROTOTYPES, L.CG_PROTOTYPES, L.GEOM_PROTOTYPES, L.NLIST_PROTOTYPES, L.DESC_PROTOTYPES):
        assert not set(names) & set(t)
    for n in names:
        decl = re.search(r"HTF_API\s+\w+\s+%s\s*\(([^)]*)\)" % n, _header()).group(1)
        assert len(decl.split(",")) == len(L.DESC_TRAIN_PROTOTYPES[n][1]), n
    assert raw.htf_abi_version() == 5 and L.ABI_VERSION == 5


def test_desc_train_pybind_module_exports_table(htf):
    import importlib
    mod_path = os.path.join(os.path.dirname(htf._lib.LIB_PATH), "_htf_abi.so")
    if not os.path.exists(mod_path):
        pytest.skip("the pybind11 module is not built")
    mod = importlib.import_module("hoomd_tf_amd._htf_abi")
    for n in htf._lib.DESC_TRAIN_PROTOTYPES:
        assert hasattr(mod, n)


def test_desc_train_header_is_plain_c():
    """include/htf_desc_train.h compiles as C99 beside htf_amd.h."""
    import subprocess
    import tempfile
    from helpers import ROOT
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "htf_amd.h"\n#include "htf_desc_train.h"\n'
                             'int main(void){size_t (*f)(unsigned, unsigned, unsigned, unsigned, unsigned) = htf_dtrain_scratch_floats; '
                             '(void)f; (void)htf_dtrain_loss_grad; return HTF_OK;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_desc_train_kernels_use_no_scratch(tmp_path):
    """Every instantiation of the sweep and its reduction keeps to registers: no private segment, no vector-register spills."""
    import test_codeobj as t
    if not (os.path.exists(t.LIB) and os.path.exists(t.READELF)):
        pytest.skip("library or llvm-readelf missing")
    meta = t._kernel_metadata(tmp_path)
    sweep = [n for n in meta if "dtrain_sweep_kernel" in n]
    assert len(sweep) == 4          # activation x nlist dtype
    assert len([n for n in meta if "dtrain_reduce_kernel" in n]) == 1
    ks = [n for n in meta if "dtrain_" in n]
    assert not [n for n in ks if "desc_mlp_kernel" in n]
    bad = {n: meta[n] for n in ks if meta[n]["private_segment_fixed_size"] or meta[n]["vgpr_spill_count"]}
    assert not bad, bad


def test_desc_trainable_flag(htf):
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu")
    assert lay.trainable is False and "trainable" not in lay.get_config()
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable=True)
    cfg = lay.get_config()
    assert lay.trainable is True and cfg["trainable"] is True
    again = htf.DescriptorMLP(device="cpu", **cfg)
    assert again.trainable is True and again.get_config() == cfg
    # what the optimizer step asks of a trainable layer
    d = htf.optimizers.SGD(0.1).desc(lay.nonneg_mask, lay.l1_reg)
    assert d.nonneg_mask == 0 and d.l1_reg[0] == 0.0


def test_desc_loss_gradient_has_no_cpu_path(htf):
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", trainable=True)
    with pytest.raises(ValueError, match="device tensor"):
        lay.forces(torch.zeros((4, 16, 4)))
    with pytest.raises(ValueError, match="device tensor"):
        lay.loss_gradient(torch.zeros((4, 16, 4)), torch.zeros((4, 4)))


def test_desc_train_entry_point_argument_errors(htf):
    """The C checks (no launch, no device needed): status HTF_ERR_INVALID and a message."""
    L = htf._lib
    lib = L.lib
    mu = torch.zeros(8)
    w = torch.zeros(8 * 8 + 8 + 8 * 8 + 8 + 8 + 1)
    args = dict(nlist=0x1000, dt=L.HTF_F32, B=4, NN=16, K=8, T=1, H1=8, H2=8, act=L.ACT_TANH, w=w.data_ptr(), mu=mu.data_ptr(),
                gap=0.5, labels=0x2000, ldt=L.HTF_F32, pred=0x3000, accum=0x4000, scratch=0x5000)

    def call(**kw):
        a = dict(args, **kw)
        return lib.htf_dtrain_loss_grad(a["nlist"], a["dt"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"], a["w"],
                                        a["mu"], a["gap"], a["labels"], a["ldt"], a["pred"], a["accum"], a["scratch"], None)

    for bad in (dict(K=1), dict(K=33, T=2), dict(NN=257), dict(H1=0), dict(H2=65), dict(act=7), dict(gap=0.0), dict(gap=-1.0),
                dict(dt=5), dict(ldt=3), dict(mu=None), dict(w=None), dict(nlist=None), dict(labels=None), dict(pred=None),
                dict(accum=None), dict(scratch=None), dict(B=0, w=None)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    # the scratch size: one partial [1 + P] per block, a function of B and the widths alone; nothing for no rows
    P = w.numel()
    assert lib.htf_dtrain_scratch_floats(0, 8, 1, 8, 8) == 0
    n1 = lib.htf_dtrain_scratch_floats(1, 8, 1, 8, 8)
    assert n1 >= 1 + P and n1 % (1 + P) == 0
    assert lib.htf_dtrain_scratch_floats(1 << 20, 8, 1, 8, 8) == lib.htf_dtrain_scratch_floats(1 << 24, 8, 1, 8, 8) >= n1


def test_desc_train_zero_rows_is_ok(htf):
    """B = 0: HTF_OK with no row pointer to read and, without an accum to zero-fill, no launch; the limits are still checked."""
    L = htf._lib
    mu, w = torch.zeros(8), torch.zeros(8 * 8 + 8 + 8 * 8 + 8 + 8 + 1)

    def call(K):
        return L.lib.htf_dtrain_loss_grad(None, L.HTF_F32, 0, 16, K, 1, 8, 8, L.ACT_TANH, w.data_ptr(), mu.data_ptr(), 0.5, None,
                                          L.HTF_F32, None, None, None, None)

    assert call(8) == L.HTF_OK
    assert call(1) == L.HTF_ERR_INVALID and "descriptor network" in L.last_error()
