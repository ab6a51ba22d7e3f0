"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every
symbol include/htf_amd.h declares, and its host-side argument validation maps to the
exception types the reference raises.  No kernel is launched here."""
import ctypes
import os
import re

import pytest

from helpers import ROOT


def _declared_symbols(header="htf_amd.h"):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    return sorted(set(re.findall(r"HTF_API[^;]*?\b(htfs?_\w+)\s*\(", hdr)))


def test_header_symbols_exported(htf):
    names = _declared_symbols()
    assert len(names) >= 20
    raw = ctypes.CDLL(htf._lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), "libhtf_amd.so does not export %s" % n
    # and the python binding covers exactly the declared surface
    assert sorted(htf._lib.PROTOTYPES) == names
    assert raw.htf_abi_version() == 5
    standin = _declared_symbols("htf_standin.h")
    assert len(standin) >= 8 and sorted(htf._lib.STANDIN_PROTOTYPES) == standin
    for n in standin:
        assert hasattr(raw, n), "libhtf_amd.so does not export %s" % n


def test_header_is_plain_c():
    """The boundary must compile as C (no torch / C++ types in the signatures)."""
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "htf_amd.h"\n#include "htf_standin.h"\nint main(void){htf_config c; (void)c; return HTF_OK;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                               "-o", os.path.join(d, "t")])


def test_potential_validation(htf):
    with pytest.raises(ValueError):
        htf.Potential.wca(-1.0)
    with pytest.raises(ValueError):
        htf.Potential.rinv_poly([1.0], [0])
    with pytest.raises(ValueError):
        htf.Potential.rinv_poly([1.0] * 9, [1] * 9)
    with pytest.raises(ValueError):
        htf.Potential(99)
    p = htf.Potential.lj()
    assert p.handle


def test_device_tensor_required(htf):
    import torch
    with pytest.raises(ValueError):
        htf.ops.eval_forces(htf.Potential.lj(), torch.zeros(4, 8, 4))


def test_missing_library_fails_loudly(htf, tmp_path, monkeypatch):
    """No silent fallback: without libhtf_amd.so the binding refuses to import."""
    import importlib.util
    src = os.path.join(os.path.dirname(htf._lib.__file__), "_lib.py")
    dst = tmp_path / "_lib_copy.py"
    dst.write_text(open(src).read())
    spec = importlib.util.spec_from_file_location("_lib_copy", str(dst))
    mod = importlib.util.module_from_spec(spec)
    with pytest.raises(ImportError):
        spec.loader.exec_module(mod)


def test_pybind11_binding_exports_the_abi_and_runs_host_calls(htf):
    """The pybind11 binding (hoomd_tf_amd/_htf_abi.so, csrc/pybind_abi.cc; the default once built): the module exports every symbol of both headers,
    and the package's own call sites -- byref(struct), c_void_p, None, ints -- run through it unchanged: potential
    creation and validation errors, the context's host-side checks.  (The GPU suite is run under this binding by
    tools/evidence_pass.sh; here: what needs no device.)"""
    import subprocess
    import sys
    so = os.path.join(os.path.dirname(htf._lib.__file__), "_htf_abi.so")
    if not os.path.exists(so):
        pytest.skip("pybind11 module not built (make -C hoomd_tf_amd/csrc pybind)")
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import hoomd_tf_amd as htf\n"
        "from hoomd_tf_amd import _lib\n"
        "assert _lib.BINDING == 'pybind11' and type(_lib.lib).__name__ == '_PybindLib'\n"
        "names = list(_lib.PROTOTYPES) + list(_lib.STANDIN_PROTOTYPES)\n"
        "assert all(hasattr(_lib.lib._mod, n) for n in names) and len(names) == 93\n"
        "assert _lib.lib.htf_abi_version() == 5 == _lib.ABI_VERSION\n"
        "p = htf.Potential.rinv_poly([1.0, -0.5], [12, 6], cut=1.1)\n"
        "assert p.handle.value and p.num_params >= 2\n"
        "try:\n"
        "    htf.Potential.wca(-1.0)\n"
        "    raise SystemExit('no error')\n"
        "except ValueError as e:\n"
        "    assert 'sigma' in str(e)\n"
        "try:\n"
        "    htf.Context(r_cut=-1.0, nneighs=8)\n"
        "    raise SystemExit('no error')\n"
        "except (ValueError, RuntimeError):\n"
        "    pass\n"
        "print('pybind ok')\n") % ROOT
    env = dict(os.environ, HTF_BINDING="pybind11")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "pybind ok" in r.stdout, r.stdout + r.stderr[-2000:]
