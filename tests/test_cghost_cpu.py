"""The conservative DescriptorMLP on one domain's rows, on the host: the C ABI table of include/htf_cghost.h, the header as C99,
the pybind11 module, the argument checks of the four entry points (``n_table < B`` among them), the code objects of the four
translation units that define them, the layer's ``n_ghost`` / ``halo`` argument checks, ``Nlist.ghost`` and
``SlabDomain.halo_rows``' checks.  No GPU."""
import os
import re

import pytest
import torch

NAMES = ["htf_ang_forces_ghost", "htf_at_loss_grad_ghost", "htf_cf_forces_ghost", "htf_ct_loss_grad_ghost"]
TWINS = {"htf_cf_forces_ghost": ("CF_PROTOTYPES", "htf_cf_forces"), "htf_ang_forces_ghost": ("ANG_PROTOTYPES", "htf_ang_forces"),
         "htf_ct_loss_grad_ghost": ("CT_PROTOTYPES", "htf_ct_loss_grad"), "htf_at_loss_grad_ghost": ("AT_PROTOTYPES", "htf_at_loss_grad")}


def _header():
    from helpers import ROOT
    return open(os.path.join(ROOT, "include", "htf_cghost.h")).read()


# ------------------------------------------------------------------------------------------------ 1. the ABI table
def test_cghost_abi_table(htf):
    """The symbols of include/htf_cghost.h are CGHOST_PROTOTYPES: exported, bound under the active binding, argument for argument
    (each its twin's arguments and one unsigned before the stream), and no name is shared with another table.  The older tables
    keep their sizes and the ABI version has not moved."""
    import ctypes
    import subprocess
    L = htf._lib
    names = sorted(set(re.findall(r"HTF_API[^;]*?\b(htf_\w+)\s*\(", _header())))
    assert names == sorted(L.CGHOST_PROTOTYPES) == NAMES
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and hasattr(L.lib, n)
        decl = re.search(r"HTF_API\s+\w+\s+%s\s*\(([^)]*)\)" % n, _header()).group(1).split(",")
        res, args = L.CGHOST_PROTOTYPES[n]
        table, twin = TWINS[n]
        tres, targs = getattr(L, table)[twin]
        assert len(decl) == len(args) == len(targs) + 1, n
        assert res is tres and args[:-2] == targs[:-1] and args[-2] is ctypes.c_uint and args[-1] is targs[-1] is ctypes.c_void_p, n
        assert re.fullmatch(r"\s*unsigned\s+n_table", decl[-2]) and re.fullmatch(r"\s*htf_stream\s+stream", decl[-1]), n
    for t in (L.PROTOTYPES, L.STANDIN_PROTOTYPES, L.STEP_CHECK_PROTOTYPES, L.CG_PROTOTYPES, L.GEOM_PROTOTYPES, L.NLIST_PROTOTYPES,
              L.BP_PROTOTYPES, L.CF_PROTOTYPES, L.CT_PROTOTYPES, L.ANG_PROTOTYPES, L.AT_PROTOTYPES):
        assert not set(names) & set(t)
    every = [n for n, _ in L.ALL_PROTOTYPES]
    assert set(names) <= set(every) and len(every) == len(set(every))
    assert (len(L.BP_PROTOTYPES), len(L.CF_PROTOTYPES), len(L.CT_PROTOTYPES), len(L.ANG_PROTOTYPES), len(L.AT_PROTOTYPES)) == (4, 3, 1, 3, 1)
    assert raw.htf_abi_version() == 5 and L.ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {line.split()[-1] for line in nm.splitlines() if line.strip()}
    # the older headers do not declare them
    from helpers import ROOT
    for h in ("htf_amd.h", "htf_bp.h", "htf_cforce.h", "htf_ctrain.h", "htf_angular.h", "htf_atrain.h"):
        assert not re.search(r"htf_\w+_ghost\b", open(os.path.join(ROOT, "include", h)).read()), h


def test_cghost_pybind_module_exports_table(htf):
    import importlib
    mod_path = os.path.join(os.path.dirname(htf._lib.LIB_PATH), "_htf_abi.so")
    if not os.path.exists(mod_path):
        pytest.skip("the pybind11 module is not built")
    mod = importlib.import_module("hoomd_tf_amd._htf_abi")
    for n in htf._lib.CGHOST_PROTOTYPES:
        assert hasattr(mod, n)


def test_cghost_header_is_plain_c():
    """include/htf_cghost.h compiles as C99, alone and beside the headers of its twins."""
    import subprocess
    import tempfile
    from helpers import ROOT
    with tempfile.TemporaryDirectory() as d:
        for k, pre in enumerate(('', '#include "htf_amd.h"\n#include "htf_bp.h"\n#include "htf_cforce.h"\n#include "htf_ctrain.h"\n'
                                     '#include "htf_angular.h"\n#include "htf_atrain.h"\n')):
            src = os.path.join(d, "t%d.c" % k)
            open(src, "w").write(pre + '#include "htf_cghost.h"\n'
                                 'int main(void){int (*f)(const void *, int, const int *, const float *, unsigned, unsigned, unsigned, '
                                 'unsigned, const float *, float, const float *, const float *, void *, int, void *, float, unsigned, '
                                 'htf_stream) = htf_cf_forces_ghost; '
                                 'int (*g)(const void *, int, const int *, unsigned, unsigned, unsigned, unsigned, unsigned, unsigned, int, '
                                 'const float *, const float *, float, const float *, float *, float *, const int *, unsigned, float, '
                                 'unsigned, unsigned, htf_stream) = htf_at_loss_grad_ghost; '
                                 '(void)f; (void)g; (void)htf_ang_forces_ghost; (void)htf_ct_loss_grad_ghost; return HTF_OK;}\n')
            subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                                   "-o", os.path.join(d, "t%d.o" % k)])


# ------------------------------------------------------------------------------------------------ 2. the code objects
def test_cghost_kernels_use_no_scratch(tmp_path):
    """The four translation units that define the new entries -- cforce, angular, ctrain, atrain -- hold the kernels they held
    (the ghost entries launch their twins' kernels with one more argument: no new instantiation), and every one keeps to
    registers: no private segment, no vector-register spills."""
    import test_codeobj as t
    if not (os.path.exists(t.LIB) and os.path.exists(t.READELF)):
        pytest.skip("library or llvm-readelf missing")
    meta = t._kernel_metadata(tmp_path)
    census = {"cf_grad_kernel": 16, "cf_pair_force_kernel": 16, "cf_pair_kernel": 2, "ang_grad_kernel": 16, "ang_force_kernel": 16,
              "ang_desc_kernel": 8, "ct_sweep_kernel": 16, "at_sweep_kernel": 32}
    ks = []
    for sub, count in census.items():
        found = [n for n in meta if sub in n]
        assert len(found) == count, (sub, len(found))
        ks += found
    assert not [n for n in meta if "ghost" in n]
    bad = {n: meta[n] for n in ks if meta[n]["private_segment_fixed_size"] or meta[n]["vgpr_spill_count"]}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ 3. the entry points
def _base(htf, D=8):
    L = htf._lib
    mu = torch.zeros(8)
    w = torch.zeros(D * 8 + 8 + 8 * 8 + 8 + 8 + 1)
    return L, (mu, w), dict(nlist=0x1000, dt=L.HTF_F32, B=4, NN=16, K=8, T=1, H1=8, H2=8, act=L.ACT_TANH, w=w.data_ptr(),
                            mu=mu.data_ptr(), gap=0.5, g=0x2000, e=0x3000, rows=None, n_rows=4, rc=0.0, index=0x4000, types=None,
                            out=0x5000, odt=L.HTF_F32, vir=None, rho=0x3000, accum=0x6000, scratch=0x7000, l_max=1, n_table=6)


COMMON_BAD = (dict(K=1), dict(K=33, T=2), dict(NN=257), dict(gap=0.0), dict(gap=-1.0), dict(dt=5), dict(mu=None), dict(nlist=None),
              dict(rc=-1.0), dict(rc=float("nan")), dict(rc=float("inf")))
# the table has fewer rows than the pair tensor
SHORT = (dict(n_table=3), dict(n_table=0), dict(B=1, n_rows=1, n_table=0))


@pytest.mark.parametrize("angular", [False, True])
def test_cghost_forces_entry_point_argument_errors(htf, angular):
    """The C checks of pass 2 with a table (no launch, no device needed): its twin's, and n_table >= B."""
    L, keep, args = _base(htf)

    def call(**kw):
        a = dict(args, **kw)
        if angular:
            return L.lib.htf_ang_forces_ghost(a["nlist"], a["dt"], a["index"], a["types"], a["B"], a["NN"], a["K"], a["T"], a["mu"],
                                              a["gap"], a["g"], a["e"], a["out"], a["odt"], a["vir"], a["rc"], a["l_max"], a["n_table"],
                                              None)
        return L.lib.htf_cf_forces_ghost(a["nlist"], a["dt"], a["index"], a["types"], a["B"], a["NN"], a["K"], a["T"], a["mu"], a["gap"],
                                         a["g"], a["e"], a["out"], a["odt"], a["vir"], a["rc"], a["n_table"], None)

    more = (dict(l_max=0), dict(l_max=3), dict(K=22, l_max=2), dict(g=0x2004)) if angular else ()   # (a misaligned table)
    for bad in COMMON_BAD + SHORT + (dict(g=None), dict(e=None), dict(odt=3), dict(out=None), dict(index=None), dict(T=2)) + more:
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error(), bad
    assert call(n_table=3) == L.HTF_ERR_INVALID and "n_table 3 < B 4" in L.last_error()
    # B = 0 launches nothing, whatever the table holds; the limits are still checked
    none = dict(B=0, nlist=None, index=None, g=None, e=None, out=None)
    assert call(n_table=0, **none) == L.HTF_OK and call(n_table=9, **none) == L.HTF_OK and call(n_table=9, T=2, **none) == L.HTF_OK
    assert call(n_table=9, NN=257, **none) == L.HTF_ERR_INVALID and "descriptor network" in L.last_error()


@pytest.mark.parametrize("angular", [False, True])
def test_cghost_loss_grad_entry_point_argument_errors(htf, angular):
    """The C checks of the sweeps with a residual table: their twins', and n_table >= B."""
    L, keep, args = _base(htf, D=16 if angular else 8)

    def call(**kw):
        a = dict(args, **kw)
        head = (a["nlist"], a["dt"], a["index"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"], a["w"], a["mu"], a["gap"],
                a["rho"], a["accum"], a["scratch"], a["rows"], a["n_rows"], a["rc"])
        if angular:
            return L.lib.htf_at_loss_grad_ghost(*head, a["l_max"], a["n_table"], None)
        return L.lib.htf_ct_loss_grad_ghost(*head, a["n_table"], None)

    more = (dict(l_max=0), dict(l_max=3), dict(K=22, l_max=2)) if angular else ()
    for bad in COMMON_BAD + SHORT + (dict(n_rows=5), dict(H1=0), dict(H2=65), dict(act=7), dict(w=None), dict(rho=None), dict(accum=None),
                                     dict(scratch=None), dict(index=None), dict(B=0, w=None), dict(B=0, n_rows=1),
                                     dict(n_rows=6)) + more:   # (n_rows counts rows of B, not of the table)
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error(), bad
    assert call(n_table=3) == L.HTF_ERR_INVALID and "n_table 3 < B 4" in L.last_error()
    none = dict(B=0, n_rows=0, nlist=None, index=None, rho=None, accum=None, scratch=None)
    assert call(n_table=0, **none) == L.HTF_OK and call(n_table=9, **none) == L.HTF_OK
    assert call(n_table=9, K=1, **none) == L.HTF_ERR_INVALID and "descriptor network" in L.last_error()


# ------------------------------------------------------------------------------------------------ 4. the layer
def test_cghost_layer_argument_checks(htf):
    """n_ghost and halo are checked before the device is: ghost rows need a halo, a count is a non-negative integer; the defaults
    reach the checks the methods had."""
    x, labels, index = torch.zeros((4, 16, 4)), torch.zeros((4, 4)), torch.zeros((4, 16), dtype=torch.int32)
    cases = [(htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True), ("total_forces", "total_loss_gradient")),
             (htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True, l_max=2), ("total_forces", "angular_loss_gradient"))]
    for lay, methods in cases:
        for name in methods:
            fn = getattr(lay, name)
            args = (x, index) if name == "total_forces" else (x, labels, index)
            with pytest.raises(ValueError, match="halo") as info:
                fn(*args, n_ghost=3)
            assert name in str(info.value) and "n_ghost=3" in str(info.value)
            with pytest.raises(ValueError, match="callable"):
                fn(*args, n_ghost=3, halo=7)
            for bad in (-1, 1.5, True):
                with pytest.raises(ValueError, match="n_ghost"):
                    fn(*args, n_ghost=bad, halo=lambda t: t)
            # no CPU path: the defaults, a halo that is not needed, and ghost rows with their halo all get as far as the device check
            called = []
            for kw in (dict(), dict(n_ghost=0, halo=called.append), dict(n_ghost=3, halo=called.append), dict(n_ghost=2.0, halo=called.append)):
                with pytest.raises(ValueError, match="device tensor"):
                    fn(*args, **kw)
            assert not called


def test_cghost_nlist_carries_ghost_rows(htf):
    """Nlist.ghost: None by default, a pair as given, a callable read once and only when asked -- as Nlist.index."""
    x = torch.zeros((4, 16, 4))
    assert htf.Nlist(x).ghost is None and htf.Nlist(x, index=None).ghost is None
    f = lambda t: t   # noqa: E731
    assert htf.Nlist(x, ghost=(3, f)).ghost == (3, f)
    calls = []
    lazy = htf.Nlist(x, index=torch.zeros((4, 16), dtype=torch.int32), ghost=lambda: calls.append(1) or (5, f))
    assert not calls
    assert lazy.ghost is lazy.ghost and len(calls) == 1 and lazy.ghost == (5, f)
    # ghost rows reach the layer through compute_nlist_forces: here the layer's own check speaks (no halo for 2 ghost rows)
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", conservative=True)
    nl = htf.Nlist(x, index=torch.zeros((4, 16), dtype=torch.int32), ghost=(2, None))
    with pytest.raises(ValueError, match="halo"):
        htf.compute_nlist_forces(nl, lay(nl))


# ------------------------------------------------------------------------------------------------ 5. the halo's own checks
def _slab(htf, world, rank=0):
    from hoomd_tf_amd import standin
    from hoomd_tf_amd.domain import SlabDomain
    import numpy as np
    pos = np.random.default_rng(1).uniform(-4.0, 4.0, (32, 3))
    sysm = standin.System(pos, np.array([8.0, 8.0, 8.0]), dtype=torch.float32, device="cpu")
    return sysm, SlabDomain(sysm, rank, world, r_ghost=1.0)


def test_cghost_halo_rows_checks(htf):
    """One rank: a no-op that returns the table.  Several: it raises without a send plan, while a position exchange is pending,
    and on a table that is not a contiguous fp32 tensor of n_local + n_ghost rows -- all before any message is posted."""
    sysm, one = _slab(htf, 1)
    t = torch.arange(12.0).reshape(3, 4)
    assert one.halo_rows(t, 3) is t and torch.equal(t, torch.arange(12.0).reshape(3, 4))
    sysm, dom = _slab(htf, 4)
    with pytest.raises(RuntimeError, match="rebuild"):
        dom.halo_rows(torch.zeros((sysm.N, 4)), sysm.N)
    dom.send_left, dom.send_right, dom.n_from_left, dom.n_from_right = (20, 26), (24, 32), 3, 2
    dom._works = [object()]
    assert dom.pending
    with pytest.raises(RuntimeError, match="pending"):
        dom.halo_rows(torch.zeros((sysm.N + 5, 4)), sysm.N)
    dom._works = None
    for bad in (torch.zeros((sysm.N + 4, 4)), torch.zeros((sysm.N + 5, 4), dtype=torch.float64), torch.zeros((4, sysm.N + 5)).T,
                torch.zeros(()), None):
        with pytest.raises(ValueError, match="table"):
            dom.halo_rows(bad, sysm.N)
    with pytest.raises(ValueError, match="n_local"):
        dom.halo_rows(torch.zeros((sysm.N + 4, 4)), sysm.N - 1)
