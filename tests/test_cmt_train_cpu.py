"""Force matching for every member of a committee (htf.DescriptorMLP(n_models=M, trainable="committee")) on the host: the C ABI
table of include/htf_cmt_train.h, the header as C99, the code objects of the sweep, the layer's new value of ``trainable`` with
its refusals, and the argument checks of the two entry points.  No GPU."""
import os
import re

import pytest
import torch


def _header():
    from helpers import ROOT
    return open(os.path.join(ROOT, "include", "htf_cmt_train.h")).read()


def test_cmt_train_abi_table(htf):
    """The symbols of include/htf_cmt_train.h are CMT_TRAIN_PROTOTYPES: exported, bound under the active binding, argument for
    argument, and no name is shared with another table.  The other tables keep their sizes and the ABI version has not moved."""
    import ctypes
    import subprocess
    L = htf._lib
    names = sorted(set(re.findall(r"HTF_API[^;]*?\b(htf_\w+)\s*\(", _header())))
    assert names == sorted(L.CMT_TRAIN_PROTOTYPES) == ["htf_cmt_loss_grad", "htf_cmt_scratch_floats"]
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and hasattr(L.lib, n)
        decl = re.search(r"HTF_API\s+\w+\s+%s\s*\(([^)]*)\)" % n, _header()).group(1)
        assert len(decl.split(",")) == len(L.CMT_TRAIN_PROTOTYPES[n][1]), n
    assert len(L.CMT_TRAIN_PROTOTYPES["htf_cmt_loss_grad"][1]) == 23 and len(L.CMT_TRAIN_PROTOTYPES["htf_cmt_scratch_floats"][1]) == 6
    assert L.CMT_TRAIN_PROTOTYPES["htf_cmt_scratch_floats"][0] is ctypes.c_size_t
    for t in (L.PROTOTYPES, L.STANDIN_PROTOTYPES, L.STEP_CHECK_PROTOTYPES, L.CG_PROTOTYPES, L.GEOM_PROTOTYPES, L.NLIST_PROTOTYPES,
              L.BP_PROTOTYPES, L.CF_PROTOTYPES, L.CT_PROTOTYPES, L.ANG_PROTOTYPES, L.AT_PROTOTYPES, L.CGHOST_PROTOTYPES,
              L.CMT_PROTOTYPES):
        assert not set(names) & set(t)
    every = [n for n, _ in L.ALL_PROTOTYPES]
    assert set(names) <= set(every) and len(every) == len(set(every))
    assert (len(L.BP_PROTOTYPES), len(L.CF_PROTOTYPES), len(L.CT_PROTOTYPES), len(L.CMT_PROTOTYPES)) == (4, 3, 1, 2)
    assert raw.htf_abi_version() == 5 and L.ABI_VERSION == 5
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(names) <= {line.split()[-1] for line in nm.splitlines() if line.strip()}


def test_cmt_train_pybind_module_exports_table(htf):
    import importlib
    mod_path = os.path.join(os.path.dirname(htf._lib.LIB_PATH), "_htf_abi.so")
    if not os.path.exists(mod_path):
        pytest.skip("the pybind11 module is not built")
    mod = importlib.import_module("hoomd_tf_amd._htf_abi")
    for n in htf._lib.CMT_TRAIN_PROTOTYPES:
        assert hasattr(mod, n)


def test_cmt_train_header_is_plain_c():
    """include/htf_cmt_train.h compiles as C99 beside htf_amd.h, htf_ctrain.h and htf_committee.h."""
    import subprocess
    import tempfile
    from helpers import ROOT
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "htf_amd.h"\n#include "htf_ctrain.h"\n#include "htf_committee.h"\n#include "htf_cmt_train.h"\n'
                             'int main(void){int (*f)(const void *, int, const int *, unsigned, unsigned, unsigned, unsigned, '
                             'unsigned, unsigned, int, const float *, const float *, float, const float *, float *, float *, '
                             'const int *, unsigned, float, unsigned, unsigned, unsigned, htf_stream) = htf_cmt_loss_grad; '
                             'size_t (*g)(unsigned, unsigned, unsigned, unsigned, unsigned, unsigned) = htf_cmt_scratch_floats; '
                             '(void)f; (void)g; (void)htf_ct_loss_grad; return HTF_CMT_MAX_MODELS == 8 ? HTF_OK : 1;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_cmt_train_kernels_use_no_scratch(tmp_path):
    """Every instantiation of the sweep -- activation x cutoff x list x nlist dtype; the number of members is the block's number
    of waves -- keeps to registers: no private segment, no vector-register spills.  At two waves per SIMD (a block of eight
    waves) a wave has 256 registers.  The names stay out of the other families' counts; the partials are added by one more
    reduction kernel, a second instance of dtrain_reduce_kernel, of which the library still has one."""
    import test_codeobj as t
    from test_committee_cpu import FAMILY_SUBSTRINGS
    if not (os.path.exists(t.LIB) and os.path.exists(t.READELF)):
        pytest.skip("library or llvm-readelf missing")
    meta = t._kernel_metadata(tmp_path)
    sweep = [n for n in meta if "committee_train_kernel" in n]
    reduce_ = [n for n in meta if "committee_reduce_kernel" in n]
    assert len(sweep) == 16 and len(reduce_) == 1
    assert sorted(sweep + reduce_) == sorted(n for n in meta if "committee_" in n)
    sweep = sweep + reduce_
    assert not [n for n in sweep if "cmt_" in n or any(s in n for s in FAMILY_SUBSTRINGS)]
    assert len([n for n in meta if "dtrain_reduce_kernel" in n]) == 1
    bad = {n: meta[n] for n in sweep if meta[n]["private_segment_fixed_size"] or meta[n]["vgpr_spill_count"]
           or meta[n]["vgpr_count"] > 256}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the layer
def test_cmt_train_layer_value(htf):
    kw = dict(K=8, H1=8, H2=8, device="cpu")
    lay = htf.DescriptorMLP(n_models=3, trainable="committee", **kw)
    assert lay.trainable == "committee" and lay.conservative is True and lay.n_models == 3 and lay.w.numel() == 3 * lay.P
    cfg = lay.get_config()
    assert cfg["trainable"] == "committee" and cfg["conservative"] is True and cfg["n_models"] == 3
    again = htf.DescriptorMLP(device="cpu", **cfg)
    assert again.trainable == "committee" and again.get_config() == cfg
    # the value alone implies the conservative forces
    assert htf.DescriptorMLP(n_models=2, trainable="committee", conservative=False, **kw).conservative is True
    full = htf.DescriptorMLP(n_models=2, trainable="committee", r_cut=2.5, n_species=2, n_types=2, **kw).get_config()
    assert htf.DescriptorMLP(device="cpu", **full).get_config() == full
    # by name: a committee, and no angular channels
    for bad in (dict(), dict(n_models=1)):
        with pytest.raises(ValueError, match="n_models >= 2"):
            htf.DescriptorMLP(trainable="committee", **kw, **bad)
    with pytest.raises(ValueError, match="l_max = 0"):
        htf.DescriptorMLP(trainable="committee", n_models=2, l_max=1, **kw)
    with pytest.raises(ValueError, match="trainable.*committee"):
        htf.DescriptorMLP(trainable="members", **kw)
    # member(m, trainable=...) keeps working: a plain layer on a view of member m
    for tr in (False, "total"):
        one = lay.member(1, trainable=tr)
        assert one.trainable == tr and one.n_models == 1 and one.conservative is True
        assert one.w.data_ptr() == lay.w.data_ptr() + 4 * lay.P and one.w.numel() == lay.P
        assert "n_models" not in one.get_config()
    # what the optimizer step asks of a trainable layer
    d = htf.optimizers.SGD(0.1).desc(lay.nonneg_mask, lay.l1_reg)
    assert d.nonneg_mask == 0 and d.l1_reg[0] == 0.0


def test_cmt_train_untouched_refusals(htf):
    """What a committee refused before the new value it refuses still, message for message."""
    kw = dict(K=8, H1=8, H2=8, device="cpu", conservative=True)
    for tr in (True, "total", "angular"):
        with pytest.raises(NotImplementedError, match="trainable.*follow-up.*member"):
            htf.DescriptorMLP(trainable=tr, n_models=2, **kw)
    with pytest.raises(NotImplementedError, match="l_max.*follow-up.*total_forces"):
        htf.DescriptorMLP(l_max=1, n_models=2, **kw)
    x, labels = torch.zeros((4, 16, 4)), torch.zeros((4, 4))
    idx = torch.zeros((4, 16), dtype=torch.int32)
    for lay in (htf.DescriptorMLP(n_models=2, **kw), htf.DescriptorMLP(n_models=2, trainable="committee", **kw)):
        for what, call in (("forces", lambda: lay.forces(x)), ("loss_gradient", lambda: lay.loss_gradient(x, labels)),
                           ("total_loss_gradient", lambda: lay.total_loss_gradient(x, labels, idx)),
                           ("angular_loss_gradient", lambda: lay.angular_loss_gradient(x, labels, idx)),
                           ("descriptor", lambda: lay.descriptor(htf.Nlist(x)))):
            with pytest.raises(NotImplementedError, match=r"member\(m\)\.%s" % what):
                call()
        with pytest.raises(NotImplementedError, match="follow-up.*member"):
            lay.total_forces(x, idx, n_ghost=2, halo=lambda t: None)


def test_cmt_train_method_checks(htf):
    """committee_loss_gradient is callable on any committee, trainable or not, has no CPU path, and is not a single network's."""
    kw = dict(K=8, H1=8, H2=8, device="cpu")
    x, labels = torch.zeros((4, 16, 4)), torch.zeros((4, 4))
    idx = torch.zeros((4, 16), dtype=torch.int32)
    for lay in (htf.DescriptorMLP(n_models=2, conservative=True, **kw), htf.DescriptorMLP(n_models=2, trainable="committee", **kw)):
        with pytest.raises(ValueError, match="device tensor"):
            lay.committee_loss_gradient(x, labels, idx)
    for lay in (htf.DescriptorMLP(**kw), htf.DescriptorMLP(trainable="total", **kw)):
        with pytest.raises(ValueError, match="n_models > 1.*total_loss_gradient"):
            lay.committee_loss_gradient(x, labels, idx)


def test_cmt_train_lds_refusal(htf):
    """4 (M (P4 + 640) + K4) bytes; at construction a trainable="committee" layer above one compute unit's 160 KiB raises with
    both byte counts.  A committee that is only evaluated is held to its own sweep's figure, as before."""
    f = htf.DescriptorMLP.committee_train_lds_bytes
    assert f(8, 16, 1, 32, 32) == 4 * (8 * (1684 + 640) + 16) == 74432 > 64 * 1024
    assert f(2, 16, 1, 32, 32) == 4 * (2 * (1684 + 640) + 16)
    assert f(8, 10, 3, 24, 20) == 4 * (8 * (((30 * 25 + 24 + 24 * 21 + 41 + 3) & ~3) + 640) + 12)
    # between the two figures: 8 networks of 48 x 48 x 48 need 159 552 bytes to evaluate and 175 936 to train; the limit is 163 840
    K, H1, H2, M = 48, 48, 48, 8
    member = (K * (H1 + 1) + H1 + H1 * (H2 + 1) + 2 * H2 + 1 + 3) & ~3
    assert member == 4852
    ev, tr = htf.DescriptorMLP.committee_lds_bytes(M, K, 1, H1, H2), f(M, K, 1, H1, H2)
    assert (ev, tr) == (4 * (M * member + K + 1024), 4 * (M * (member + 640) + K)) and ev <= 160 * 1024 < tr
    assert htf.DescriptorMLP(K=K, H1=H1, H2=H2, device="cpu", conservative=True, n_models=M).n_models == M
    with pytest.raises(ValueError, match=r"training sweep.*%d bytes.*%d bytes" % (tr, 160 * 1024)):
        htf.DescriptorMLP(K=K, H1=H1, H2=H2, device="cpu", trainable="committee", n_models=M)
    assert htf.DescriptorMLP(K=64, H1=64, H2=64, device="cpu", trainable="committee", n_models=4).n_models == 4


# ------------------------------------------------------------------------------------------------ the entry points
def test_cmt_loss_grad_entry_point_argument_errors(htf):
    """The C checks (no launch, no device needed): htf_ct_loss_grad's, the members and the two strides."""
    L = htf._lib
    mu = torch.zeros(8)
    P = 8 * 8 + 8 + 8 * 8 + 8 + 8 + 1
    w = torch.zeros(2 * P)
    args = dict(nlist=0x1000, dt=L.HTF_F32, index=0x6000, B=4, NN=16, K=8, T=1, H1=8, H2=8, act=L.ACT_TANH, w=w.data_ptr(),
                mu=mu.data_ptr(), gap=0.5, rho=0x3000, accum=0x4000, scratch=0x5000, rows=None, n_rows=4, rc=0.0, M=2, ws=P,
                as_=1 + P)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_cmt_loss_grad(a["nlist"], a["dt"], a["index"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"],
                                       a["w"], a["mu"], a["gap"], a["rho"], a["accum"], a["scratch"], a["rows"], a["n_rows"], a["rc"],
                                       a["M"], a["ws"], a["as_"], None)

    for bad in (dict(K=1), dict(K=33, T=2), dict(NN=257), dict(gap=0.0), dict(gap=-1.0), dict(dt=5), dict(mu=None), dict(nlist=None),
                dict(n_rows=5), dict(rc=-1.0), dict(rc=float("nan")), dict(rc=float("inf")), dict(rc=-float("inf")), dict(H1=0),
                dict(H2=65), dict(act=7), dict(w=None), dict(rho=None), dict(accum=None), dict(scratch=None), dict(index=None),
                dict(B=0, w=None), dict(B=0, n_rows=1), dict(M=0), dict(M=1), dict(M=9), dict(ws=P - 1), dict(as_=P)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    # over the LDS budget: refused without a launch, both byte counts in the message
    assert call(K=64, H1=64, H2=64, M=8, ws=1 << 20, as_=1 << 20) == L.HTF_ERR_INVALID
    assert "%d bytes" % htf.DescriptorMLP.committee_train_lds_bytes(8, 64, 1, 64, 64) in L.last_error() and "163840" in L.last_error()
    K, H1, H2, M = 48, 48, 48, 8
    assert call(K=K, H1=H1, H2=H2, M=M, ws=1 << 20, as_=1 << 20) == L.HTF_ERR_INVALID
    assert "%d bytes" % htf.DescriptorMLP.committee_train_lds_bytes(M, K, 1, H1, H2) in L.last_error() and "163840" in L.last_error()
    # B = 0 and no rows: HTF_OK with no pointer to read and, without an accum to zero-fill, no launch; the limits are still checked
    none = dict(B=0, n_rows=0, nlist=None, index=None, rho=None, accum=None, scratch=None)
    assert call(**none) == L.HTF_OK
    assert call(rows=0x7000, **none) == L.HTF_OK
    for bad in (dict(K=1), dict(M=9), dict(M=1), dict(ws=P - 1), dict(as_=P)):
        assert call(**dict(none, **bad)) == L.HTF_ERR_INVALID and "descriptor network" in L.last_error()


def test_cmt_scratch_floats(htf):
    """One partial [1 + P] per block and member: a block per 16 rows until the grid is what 256 compute units of eight waves hold
    at once, 256 (8 // M) blocks; 0 for what the sweep refuses.  The grid is a function of the row count and M alone."""
    lib = htf._lib.lib
    P = 8 * 8 + 8 + 8 * 8 + 8 + 8 + 1
    for M in (2, 3, 8):
        assert lib.htf_cmt_scratch_floats(0, 8, 1, 8, 8, M) == 0
        for n, blocks in ((1, 1), (16, 1), (17, 2), (300, 19), (1 << 20, 256 * (8 // M)), (1 << 24, 256 * (8 // M))):
            assert lib.htf_cmt_scratch_floats(n, 8, 1, 8, 8, M) == blocks * M * (1 + P), (M, n)
    for bad in (dict(K=1), dict(M=1), dict(M=9), dict(H1=65)):
        a = dict(dict(K=8, H1=8, M=2), **bad)
        assert lib.htf_cmt_scratch_floats(4, a["K"], 1, a["H1"], 8, a["M"]) == 0
