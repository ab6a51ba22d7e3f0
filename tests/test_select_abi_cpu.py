"""htf.DeviationSelector on the host: the C ABI table of include/htf_select.h under both bindings, the header as C99, the code
objects of the three kernels, the argument checks of the entry points (every refusal precedes the first HIP call, so none needs
a device) and the Python surface's own refusals.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch


def _header():
    from helpers import ROOT
    return open(os.path.join(ROOT, "include", "htf_select.h")).read()


def test_sel_abi_table(htf):
    """The htf_sel_* names of include/htf_select.h are SEL_PROTOTYPES: exported by the library and by the pybind11 module when
    it is built, bound under the active binding, argument for argument; no name is shared with another table, and the pinned
    tables and the ABI version have not moved."""
    import ctypes
    import importlib
    import subprocess
    L = htf._lib
    names = sorted(set(re.findall(r"HTF_API[^;]*?\b(htf_sel_\w+)\s*\(", _header())))
    assert names == sorted(L.SEL_PROTOTYPES) == ["htf_sel_reset", "htf_sel_state_words", "htf_sel_update"]
    raw = ctypes.CDLL(L.LIB_PATH)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    for n in names:
        assert hasattr(raw, n) and hasattr(L.lib, n) and n in exported
        decl = re.search(r"HTF_API\s+[\w ]+?\s+%s\s*\(([^)]*)\)" % n, _header()).group(1)
        assert len(decl.split(",")) == len(L.SEL_PROTOTYPES[n][1]), n
    assert L.SEL_PROTOTYPES["htf_sel_state_words"][0] is ctypes.c_ulonglong
    if os.path.exists(os.path.join(os.path.dirname(L.LIB_PATH), "_htf_abi.so")):
        mod = importlib.import_module("hoomd_tf_amd._htf_abi")
        for n in names:
            assert hasattr(mod, n), "_htf_abi.so does not export %s" % n
    every = [n for n, _ in L.ALL_PROTOTYPES]
    assert set(names) <= set(every) and len(every) == len(set(every))
    assert len(L.PROTOTYPES) + len(L.STANDIN_PROTOTYPES) == 93 and not [n for n in names if n in L.PROTOTYPES]
    assert raw.htf_abi_version() == 5 and L.ABI_VERSION == 5
    # the enums the binding restates
    h = _header()
    assert "HTF_SEL_FIRST = %d, HTF_SEL_LARGEST = %d" % (L.SEL_FIRST, L.SEL_LARGEST) in h
    assert "HTF_SEL_FORCE = %d, HTF_SEL_ENERGY = %d" % (L.SEL_FORCE, L.SEL_ENERGY) in h
    for name in ("SEEN", "ACCURATE", "CANDIDATE", "FAILED", "STORED", "DROPPED", "REPLACED", "SLOT", "LAST", "HEADER_WORDS"):
        assert re.search(r"HTF_SEL_%s = %d\b" % (name, getattr(L, "SEL_" + name)), h), name
    assert "#define HTF_SEL_MAX_CAPACITY %du" % L.SEL_MAX_CAPACITY in h and "#define HTF_SEL_MAX_BLOCKS %du" % L.SEL_MAX_BLOCKS in h


def test_sel_header_is_plain_c():
    import subprocess
    import tempfile
    from helpers import ROOT
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "htf_amd.h"\n#include "htf_select.h"\n'
                             'int main(void){int (*f)(const float *, unsigned, int, float, float, int, unsigned, unsigned *, '
                             'const void *, const void *, int, void *, void *, unsigned, htf_stream) = htf_sel_update; '
                             'int (*g)(unsigned *, unsigned, htf_stream) = htf_sel_reset; '
                             'unsigned long long (*w)(unsigned) = htf_sel_state_words; (void)f; (void)g; (void)w; '
                             'return HTF_SEL_HEADER_WORDS == 16 && HTF_SEL_MAX_BLOCKS == 1024u ? HTF_OK : 1;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_sel_kernels(tmp_path):
    """Four code objects -- reduce, decide, store for fp32 and fp64 -- none with a private segment or a spill, none under a name
    another family's host test counts."""
    import test_codeobj as t
    from test_committee_cpu import FAMILY_SUBSTRINGS
    if not (os.path.exists(t.LIB) and os.path.exists(t.READELF)):
        pytest.skip("library or llvm-readelf missing")
    meta = t._kernel_metadata(tmp_path)
    ks = [n for n in meta if "sel_" in n]
    assert len(ks) == 4 and len([n for n in ks if "sel_store_kernel" in n]) == 2
    assert len([n for n in ks if "sel_reduce_kernel" in n]) == 1 and len([n for n in ks if "sel_decide_kernel" in n]) == 1
    assert not [n for n in ks if any(s in n for s in FAMILY_SUBSTRINGS + ("cmt_", "committee_"))]
    bad = {n: meta[n] for n in ks if meta[n]["private_segment_fixed_size"] or meta[n]["vgpr_spill_count"] or meta[n]["sgpr_spill_count"]}
    assert not bad, bad


def test_sel_state_words(htf):
    L = htf._lib
    for cap in (1, 3, 65536):
        assert L.lib.htf_sel_state_words(cap) == L.SEL_HEADER_WORDS + 3 * cap + 2 * L.SEL_MAX_BLOCKS
    assert L.lib.htf_sel_state_words(0) == 0 and L.lib.htf_sel_state_words(65537) == 0


def test_sel_entry_point_argument_errors(htf):
    """Every refusal of include/htf_select.h returns HTF_ERR_INVALID before the first HIP call: no device is present here."""
    L = htf._lib
    inf, nan = float("inf"), float("nan")
    args = dict(dev=0x1000, N=8, col=L.SEL_FORCE, lo=0.5, hi=1.0, policy=L.SEL_FIRST, cap=3, state=0x2000, pos=0x3000, box=0x4000,
                dt=L.HTF_F32, frames=0x5000, boxes=0x6000, mb=0)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_sel_update(a["dev"], a["N"], a["col"], a["lo"], a["hi"], a["policy"], a["cap"], a["state"], a["pos"],
                                    a["box"], a["dt"], a["frames"], a["boxes"], a["mb"], None)

    for bad in (dict(dev=None), dict(state=None), dict(pos=None), dict(frames=None), dict(boxes=None), dict(cap=0), dict(cap=65537),
                dict(N=0), dict(dt=2), dict(dt=-1), dict(policy=2), dict(policy=-1), dict(col=2), dict(col=-1), dict(lo=2.0),
                dict(lo=-0.5), dict(lo=nan), dict(lo=inf, hi=inf), dict(hi=nan), dict(hi=-1.0), dict(mb=L.SEL_MAX_BLOCKS + 1),
                dict(pos=0x3004), dict(frames=0x5008)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "htf_sel_update" in L.last_error()
    for bad in (dict(state=None), dict(cap=0), dict(cap=65537)):
        a = dict(dict(state=0x2000, cap=3), **bad)
        assert L.lib.htf_sel_reset(a["state"], a["cap"], None) == L.HTF_ERR_INVALID and "htf_sel_reset" in L.last_error()
    with pytest.raises(ValueError, match="null pointer"):
        L.check(call(dev=None))


def test_selector_constructor_and_cpu_refusals(htf):
    S = htf.DeviationSelector
    for bad in (dict(n_particles=0), dict(n_particles=2.0), dict(capacity=0), dict(capacity=65537), dict(capacity=True), dict(lo=-1.0),
                dict(lo=2.0, hi=1.0), dict(lo=float("inf")), dict(lo=float("nan")), dict(hi=float("nan")), dict(quantity="virial"),
                dict(policy="reservoir"), dict(dtype=torch.float16), dict(max_blocks=0), dict(max_blocks=1025), dict(max_blocks=1.5)):
        with pytest.raises(ValueError, match="DeviationSelector"):
            S(**dict(dict(n_particles=4, capacity=2, lo=0.5, device="cpu"), **bad))
    sel = S(4, 2, 0.1, hi=0.3, quantity="energy", policy="largest", dtype=torch.float64, device="cpu", max_blocks=2)
    assert (sel.lo, sel.hi) == (float(np.float32(0.1)), float(np.float32(0.3))) and sel.capacity == 2 and sel.n_particles == 4
    assert sel.counts() == dict.fromkeys(("seen", "accurate", "candidate", "failed", "stored", "dropped", "replaced"), 0)
    f = sel.frames()
    assert f["positions"].shape == (0, 4, 4) and f["positions"].dtype == np.float64 and f["box"].shape == (0, 3, 3)
    assert f["s"].shape == (0,) and f["argmax"].shape == (0,) and f["stamp"].shape == (0,)
    assert sel.last.shape == (2,) and sel.last.dtype == torch.float32
    with pytest.raises(ValueError, match="no frame is stored"):
        sel.trajectory()
    with pytest.raises(ValueError, match="device tensor"):
        sel.update(torch.zeros((4, 2)), torch.zeros((4, 4), dtype=torch.float64))
    sel.reset()
    assert sel.counts()["seen"] == 0
