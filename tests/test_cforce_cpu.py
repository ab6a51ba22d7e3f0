"""The conservative forces of htf.DescriptorMLP on the host: the C ABI table of include/htf_cforce.h, the header as C99, the
code objects of the two sweeps and of the index kernel, the layer's ``conservative`` argument and the argument checks of the
entry points.  No GPU."""
import os
import re

import pytest
import torch


def _header():
    from helpers import ROOT
    return open(os.path.join(ROOT, "include", "htf_cforce.h")).read()


def test_cf_abi_table(htf):
    """The symbols of include/htf_cforce.h are CF_PROTOTYPES: exported, bound under the active binding, argument for argument,
    and no name is shared with another table.  htf_bp.h keeps its four entries and the ABI version has not moved."""
    import ctypes
    import subprocess
    L = htf._lib
    names = sorted(set(re.findall(r"HTF_API[^;]*?\b(htf_\w+)\s*\(", _header())))
    assert names == sorted(L.CF_PROTOTYPES) == ["htf_cf_forces", "htf_cf_grad", "htf_cf_pair_index"]
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and hasattr(L.lib, n)
        decl = re.search(r"HTF_API\s+\w+\s+%s\s*\(([^)]*)\)" % n, _header()).group(1)
        assert len(decl.split(",")) == len(L.CF_PROTOTYPES[n][1]), n
    for t in (L.PROTOTYPES, L.STANDIN_PROTOTYPES, L.STEP_CHECK_PROTOTYPES, L.CG_PROTOTYPES, L.GEOM_PROTOTYPES, L.NLIST_PROTOTYPES,
              L.BP_PROTOTYPES):
        assert not set(names) & set(t)
    every = [n for n, _ in L.ALL_PROTOTYPES]
    assert set(names) <= set(every) and len(every) == len(set(every))
    assert len(L.BP_PROTOTYPES) == 4 and raw.htf_abi_version() == 5 and L.ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {line.split()[-1] for line in nm.splitlines() if line.strip()}


def test_cf_pybind_module_exports_table(htf):
    import importlib
    mod_path = os.path.join(os.path.dirname(htf._lib.LIB_PATH), "_htf_abi.so")
    if not os.path.exists(mod_path):
        pytest.skip("the pybind11 module is not built")
    mod = importlib.import_module("hoomd_tf_amd._htf_abi")
    for n in htf._lib.CF_PROTOTYPES:
        assert hasattr(mod, n)


def test_cf_header_is_plain_c():
    """include/htf_cforce.h compiles as C99 beside htf_amd.h and htf_bp.h."""
    import subprocess
    import tempfile
    from helpers import ROOT
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "htf_amd.h"\n#include "htf_bp.h"\n#include "htf_cforce.h"\n'
                             'int main(void){int (*f)(int *, const void *, int, unsigned, unsigned, unsigned, unsigned, '
                             'const htf_box *, const unsigned *, const unsigned *, const unsigned *, double, htf_stream) '
                             '= htf_cf_pair_index; (void)f; (void)htf_cf_grad; (void)htf_cf_forces; return HTF_OK;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_cf_kernels_use_no_scratch(tmp_path):
    """Every instantiation of the two sweeps and the index kernel keeps to registers: no private segment, no vector-register
    spills.  Pass 1: activation x cutoff x list x nlist dtype; pass 2: virial x cutoff x wide gather x nlist dtype; the index
    kernel: position dtype."""
    import test_codeobj as t
    if not (os.path.exists(t.LIB) and os.path.exists(t.READELF)):
        pytest.skip("library or llvm-readelf missing")
    meta = t._kernel_metadata(tmp_path)
    grad = [n for n in meta if "cf_grad_kernel" in n]
    force = [n for n in meta if "cf_pair_force_kernel" in n]
    index = [n for n in meta if "cf_pair_kernel" in n]
    assert (len(grad), len(force), len(index)) == (16, 16, 2)
    ks = grad + force + index
    assert not [n for n in ks if "bp_" in n or "dtrain_" in n or "desc_mlp" in n]
    bad = {n: meta[n] for n in ks if meta[n]["private_segment_fixed_size"] or meta[n]["vgpr_spill_count"]}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the layer
def test_cf_layer_argument_checks(htf):
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True)
    assert lay.conservative is True and lay.trainable is False
    with pytest.raises(ValueError, match="conservative"):
        htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True, trainable=True)
    # no CPU path, like forces()
    with pytest.raises(ValueError, match="device tensor"):
        lay.total_forces(torch.zeros((4, 16, 4)), torch.zeros((4, 16), dtype=torch.int32))
    # through compute_nlist_forces: a list without an index raises before anything is launched
    nl = htf.Nlist(torch.zeros((4, 16, 4)))
    assert nl.index is None
    with pytest.raises(ValueError, match="index"):
        htf.compute_nlist_forces(nl, lay(nl))
    # several types: the rows' own types come from layer(nlist, positions)
    lay3 = htf.DescriptorMLP(K=8, H1=8, H2=8, n_types=3, device="cpu", conservative=True)
    nli = htf.Nlist(torch.zeros((4, 16, 4)), index=torch.zeros((4, 16), dtype=torch.int32))
    with pytest.raises(ValueError, match="types"):
        htf.compute_nlist_forces(nli, lay3(nli))
    # the index is built when it is read, once
    calls = []
    lazy = htf.Nlist(torch.zeros((4, 16, 4)), index=lambda: calls.append(1) or torch.ones((4, 16), dtype=torch.int32))
    assert not calls
    assert lazy.index is lazy.index and len(calls) == 1 and int(lazy.index.sum()) == 64


def test_cf_default_config_is_unchanged(htf):
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu")
    assert lay.conservative is False
    assert lay.get_config() == {'K': 8, 'H1': 8, 'H2': 8, 'low': 0.0, 'high': 3.0, 'n_types': 1, 'activation': 'tanh'}
    assert "conservative" not in htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", r_cut=2.5, n_species=2).get_config()
    cfg = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", r_cut=2.5, conservative=True).get_config()
    assert cfg["conservative"] is True and cfg["r_cut"] == 2.5
    again = htf.DescriptorMLP(device="cpu", **cfg)
    assert again.conservative is True and again.get_config() == cfg


# ------------------------------------------------------------------------------------------------ the entry points
def _args(htf):
    L = htf._lib
    mu = torch.zeros(8)
    w = torch.zeros(8 * 8 + 8 + 8 * 8 + 8 + 8 + 1)
    return L, (mu, w), dict(nlist=0x1000, dt=L.HTF_F32, B=4, NN=16, K=8, T=1, H1=8, H2=8, act=L.ACT_TANH, w=w.data_ptr(),
                            mu=mu.data_ptr(), gap=0.5, g=0x2000, e=0x3000, rows=None, n_rows=4, rc=0.0, index=0x4000,
                            types=None, out=0x5000, odt=L.HTF_F32, vir=None)


COMMON_BAD = (dict(K=1), dict(K=33, T=2), dict(NN=257), dict(gap=0.0), dict(gap=-1.0), dict(dt=5), dict(mu=None), dict(nlist=None),
              dict(rc=-1.0), dict(rc=float("nan")), dict(rc=float("inf")), dict(g=None), dict(e=None))


def test_cf_grad_entry_point_argument_errors(htf):
    """The C checks (no launch, no device needed): status HTF_ERR_INVALID and a message."""
    L, keep, args = _args(htf)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_cf_grad(a["nlist"], a["dt"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"], a["w"], a["mu"],
                                 a["gap"], a["g"], a["e"], a["rows"], a["n_rows"], a["rc"], None)

    for bad in COMMON_BAD + (dict(H1=0), dict(H2=65), dict(act=7), dict(w=None), dict(n_rows=5), dict(B=0, n_rows=1)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    # no rows: HTF_OK, nothing launched; the limits are still checked
    assert call(B=0, n_rows=0, nlist=None, g=None, e=None) == L.HTF_OK
    assert call(n_rows=0) == L.HTF_OK and call(n_rows=0, rc=2.5, rows=0x6000) == L.HTF_OK
    assert call(B=0, n_rows=0, nlist=None, g=None, e=None, K=1) == L.HTF_ERR_INVALID


def test_cf_forces_entry_point_argument_errors(htf):
    L, keep, args = _args(htf)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_cf_forces(a["nlist"], a["dt"], a["index"], a["types"], a["B"], a["NN"], a["K"], a["T"], a["mu"], a["gap"],
                                   a["g"], a["e"], a["out"], a["odt"], a["vir"], a["rc"], None)

    for bad in COMMON_BAD + (dict(odt=3), dict(out=None), dict(index=None), dict(T=2)):   # (T = 2 without the rows' types)
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    assert call(B=0, nlist=None, index=None, g=None, e=None, out=None) == L.HTF_OK
    assert call(B=0, nlist=None, index=None, g=None, e=None, out=None, T=2) == L.HTF_OK
    assert call(B=0, nlist=None, index=None, g=None, e=None, out=None, NN=257) == L.HTF_ERR_INVALID


def test_cf_pair_index_entry_point_argument_errors(htf):
    L = htf._lib
    box = L.make_box([[0, 0, 0], [4, 4, 4], [0, 0, 0]])
    import ctypes
    args = dict(out=0x1000, pos=0x2000, dt=L.HTF_F32, N=8, NN=16, offset=0, batch=8, box=ctypes.byref(box), nn=0x3000, nl=0x4000,
                head=0x5000, rmax=2.5)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_cf_pair_index(a["out"], a["pos"], a["dt"], a["N"], a["NN"], a["offset"], a["batch"], a["box"], a["nn"],
                                       a["nl"], a["head"], a["rmax"], None)

    for bad in (dict(out=None), dict(pos=None), dict(nn=None), dict(nl=None), dict(head=None), dict(box=None), dict(NN=0),
                dict(offset=9), dict(offset=4, batch=5), dict(rmax=0.0), dict(dt=7)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "htf_cf_pair_index" in L.last_error()
    empty = L.make_box([[0, 0, 0], [4, 0, 4], [0, 0, 0]])
    assert call(box=ctypes.byref(empty)) == L.HTF_ERR_INVALID
    assert call(batch=0) == L.HTF_OK   # nothing to launch
