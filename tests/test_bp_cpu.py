"""htf.DescriptorMLP's native side on the host: the C ABI table of include/htf_bp.h, the header as C99, the code objects of
the row, sweep and reduction kernels, the layer's cutoff, species and trainable arguments and the argument checks of the
entry points.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch


GONE = ("htf_desc_", "htf_dtrain_")   # the prefixes of the two tables htf_bp_* replaced


def _header():
    from helpers import ROOT
    return open(os.path.join(ROOT, "include", "htf_bp.h")).read()


def test_bp_abi_table(htf):
    """The descriptor network's one table: the symbols of include/htf_bp.h, exported by the library, bound under the active
    binding, sharing no name with the other five tables; the ABI version has not moved.  The tables it replaced are gone:
    a stale caller fails to load instead of calling with the wrong arguments."""
    import ctypes
    import subprocess
    L = htf._lib
    names = sorted(set(re.findall(r"HTF_API[^;]*?\b(htf_\w+)\s*\(", _header())))
    assert names == sorted(L.BP_PROTOTYPES) and len(names) == 4
    assert all(n.startswith("htf_bp_") for n in names)
    raw = ctypes.CDLL(L.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and hasattr(L.lib, n)
    for t in (L.PROTOTYPES, L.STANDIN_PROTOTYPES, L.CG_PROTOTYPES, L.GEOM_PROTOTYPES, L.NLIST_PROTOTYPES):
        assert not set(names) & set(t)
    for n in names:
        decl = re.search(r"HTF_API\s+\w+\s+%s\s*\(([^)]*)\)" % n, _header()).group(1)
        assert len(decl.split(",")) == len(L.BP_PROTOTYPES[n][1]), n
    # the network's arguments, then (rows, n_rows, r_cut) before the stream; the descriptor entry takes r_cut alone
    assert [len(L.BP_PROTOTYPES[n][1]) for n in ("htf_bp_forces", "htf_bp_descriptor", "htf_bp_scratch_floats", "htf_bp_loss_grad")] \
        == [19, 12, 5, 21]
    assert L.BP_PROTOTYPES["htf_bp_scratch_floats"][0] is ctypes.c_size_t
    assert raw.htf_abi_version() == 5 and L.ABI_VERSION == 5
    # no symbol of the removed tables is exported or bound any more
    assert sorted(n for n, _ in L.ALL_PROTOTYPES) == sorted(set(n for n, _ in L.ALL_PROTOTYPES))
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = [line.split()[-1] for line in nm.splitlines() if line.strip()]
    assert set(names) <= set(exported)
    assert not [n for n in exported + dir(L.lib) if n.startswith(GONE)]


def test_bp_pybind_module_exports_table(htf):
    import importlib
    mod_path = os.path.join(os.path.dirname(htf._lib.LIB_PATH), "_htf_abi.so")
    if not os.path.exists(mod_path):
        pytest.skip("the pybind11 module is not built")
    mod = importlib.import_module("hoomd_tf_amd._htf_abi")
    for n in htf._lib.BP_PROTOTYPES:
        assert hasattr(mod, n)
    assert not [n for n in dir(mod) if n.startswith(GONE)]


def test_bp_header_is_plain_c():
    """include/htf_bp.h compiles as C99 beside htf_amd.h."""
    import subprocess
    import tempfile
    from helpers import ROOT
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "htf_amd.h"\n#include "htf_bp.h"\n'
                             'int main(void){size_t (*f)(unsigned, unsigned, unsigned, unsigned, unsigned) = htf_bp_scratch_floats; '
                             'int (*g)(const void *, int, unsigned, unsigned, unsigned, unsigned, const float *, float, void *, int, '
                             'float, htf_stream) = htf_bp_descriptor; '
                             '(void)f; (void)g; (void)htf_bp_forces; (void)htf_bp_loss_grad; return HTF_OK;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", src,
                               "-o", os.path.join(d, "t.o")])


def test_bp_kernels_use_no_scratch(tmp_path):
    """Every instantiation of the row, sweep and reduction kernels keeps to registers: no private segment, no vector-register
    spills; and the layer has no kernel beside them."""
    import test_codeobj as t
    if not (os.path.exists(t.LIB) and os.path.exists(t.READELF)):
        pytest.skip("library or llvm-readelf missing")
    meta = t._kernel_metadata(tmp_path)
    rows = [n for n in meta if "bp_rows_kernel" in n]
    sweep = [n for n in meta if "bp_sweep_kernel" in n]
    reduce_ = [n for n in meta if "dtrain_reduce_kernel" in n]
    # forces: activation x virial x cutoff x list x nlist dtype = 32, descriptor only (never a list): cutoff x nlist dtype = 4
    assert len(rows) == 36
    # the sweep: activation x cutoff x list x nlist dtype
    assert len(sweep) == 16
    assert len(reduce_) == 1
    assert sorted(n for n in meta if "dtrain_" in n or "desc_mlp" in n or "bp_" in n) == sorted(rows + sweep + reduce_)
    ks = rows + sweep + reduce_
    assert len(ks) == 53
    bad = {n: meta[n] for n in ks if meta[n]["private_segment_fixed_size"] or meta[n]["vgpr_spill_count"]}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the layer
def test_bp_layer_argument_checks(htf):
    for bad in (0, 0.0, -1.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="r_cut"):
            htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", r_cut=bad)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="n_species"):
            htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", n_species=bad)
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", r_cut=2.5)
    assert lay.r_cut == float(np.float32(2.5)) and lay.n_species == 1
    assert htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", r_cut=0.1).r_cut == float(np.float32(0.1))   # rounded to fp32


def test_bp_default_config_is_unchanged(htf):
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu")
    assert lay.get_config() == {'K': 8, 'H1': 8, 'H2': 8, 'low': 0.0, 'high': 3.0, 'n_types': 1, 'activation': 'tanh'}
    assert lay.r_cut is None and lay.n_species == 1
    cfg = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", r_cut=2.5, n_species=2, trainable=True).get_config()
    assert cfg["r_cut"] == 2.5 and cfg["n_species"] == 2 and cfg["trainable"] is True
    again = htf.DescriptorMLP(device="cpu", **cfg)
    assert again.get_config() == cfg
    assert "n_species" not in htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", r_cut=2.5).get_config()
    assert "r_cut" not in htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", n_species=2).get_config()


def test_bp_species_networks_are_mlp_params_of_seed_plus_s(htf):
    from hoomd_tf_amd.initializers import mlp_params
    S, seed = 3, 11
    lay = htf.DescriptorMLP(K=8, H1=12, H2=6, n_types=2, device="cpu", n_species=S, seed=seed)
    P = 16 * 12 + 12 + 12 * 6 + 6 + 6 + 1
    assert lay.P == P and lay.w.shape == (S * P,) and lay.w.dtype == torch.float32
    ws = lay.get_weights()
    for s in range(S):
        p = mlp_params(seed=seed + s, K=16, H1=12, H2=6)
        flat = np.concatenate([p[k].ravel() for k in lay._KEYS]).astype(np.float32)
        assert np.array_equal(lay.w[s * P:(s + 1) * P].numpy(), flat)
        for k, w in zip(lay._KEYS, ws):
            assert w.shape == (S,) + p[k].shape and np.array_equal(w[s], p[k].astype(np.float32))
    # one species: today's layer, bit for bit
    one = htf.DescriptorMLP(K=8, H1=12, H2=6, n_types=2, device="cpu", seed=seed)
    assert torch.equal(one.w, lay.w[:P]) and [w.shape for w in one.get_weights()] == [w.shape[1:] for w in ws]


def test_bp_weights_round_trip(htf, tmp_path):
    S = 3
    lay = htf.DescriptorMLP(K=8, H1=8, H2=4, device="cpu", n_species=S, seed=2)
    rng = np.random.default_rng(0)
    ws = [rng.standard_normal(w.shape).astype(np.float32) for w in lay.get_weights()]
    lay.set_weights(ws)
    for a, b in zip(lay.get_weights(), ws):
        assert np.array_equal(a, b)
    # network s is contiguous in w, in Keras order
    P = lay.P
    for s in range(S):
        assert np.array_equal(lay.w[s * P:(s + 1) * P].numpy(), np.concatenate([w[s].ravel() for w in ws]))
    path = str(tmp_path / "w.npz")
    lay.save_weights(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(lay._KEYS) and z["W1"].shape == (S, 8, 8)
    other = htf.DescriptorMLP(K=8, H1=8, H2=4, device="cpu", n_species=S, seed=9)
    assert not torch.equal(other.w, lay.w)
    other.load_weights(path)
    assert torch.equal(other.w, lay.w)
    with pytest.raises(ValueError, match="shape mismatch"):
        htf.DescriptorMLP(K=8, H1=8, H2=4, device="cpu").load_weights(path)   # one network: no leading axis


def test_bp_species_are_required(htf):
    lay = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu", n_species=2)
    nl = htf.Nlist(torch.zeros((4, 16, 4)))
    with pytest.raises(ValueError, match="species"):
        lay(nl)
    e = lay(nl, torch.zeros((4, 4)))
    assert e.species is not None
    # one network: the argument is accepted and ignored
    one = htf.DescriptorMLP(K=8, H1=8, H2=8, device="cpu")
    assert one(nl, torch.zeros((4, 4))).species is None and one(nl).species is None
    # no CPU path, as before
    with pytest.raises(ValueError, match="device tensor"):
        lay.forces(torch.zeros((4, 16, 4)), species=torch.zeros(4))


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


# ------------------------------------------------------------------------------------------------ the entry points
def _args(htf):
    L = htf._lib
    mu = torch.zeros(8)
    w = torch.zeros(8 * 8 + 8 + 8 * 8 + 8 + 8 + 1)
    return L, mu, w, dict(nlist=0x1000, dt=L.HTF_F32, B=4, NN=16, K=8, T=1, H1=8, H2=8, act=L.ACT_TANH, w=w.data_ptr(),
                          mu=mu.data_ptr(), gap=0.5, out=0x2000, odt=L.HTF_F32, vir=None, labels=0x2000, ldt=L.HTF_F32,
                          pred=0x3000, accum=0x4000, scratch=0x5000, rows=None, n_rows=4, rc=0.0)


COMMON_BAD = (dict(K=1), dict(K=33, T=2), dict(NN=257), dict(gap=0.0), dict(gap=-1.0), dict(dt=5), dict(mu=None), dict(nlist=None),
              dict(n_rows=5), dict(rc=-1.0), dict(rc=float("nan")), dict(rc=float("inf")), dict(rc=-float("inf")))


def test_bp_forces_entry_point_argument_errors(htf):
    """The C checks (no launch, no device needed): status HTF_ERR_INVALID and a message."""
    L, mu, w, args = _args(htf)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_bp_forces(a["nlist"], a["dt"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"], a["w"], a["mu"],
                                   a["gap"], a["out"], a["odt"], a["vir"], a["rows"], a["n_rows"], a["rc"], None)

    for bad in COMMON_BAD + (dict(H1=0), dict(H2=65), dict(act=7), dict(odt=3), dict(w=None), dict(out=None), dict(B=0, w=None),
                             dict(B=0, n_rows=1)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    # no rows: HTF_OK with no row pointer to read, nothing launched; the limits are still checked
    assert call(B=0, n_rows=0, nlist=None, out=None) == L.HTF_OK
    assert call(n_rows=0) == L.HTF_OK and call(n_rows=0, rc=2.5, rows=0x6000) == L.HTF_OK
    assert call(B=0, n_rows=0, nlist=None, out=None, K=1) == L.HTF_ERR_INVALID


def test_bp_descriptor_entry_point_argument_errors(htf):
    L, mu, w, args = _args(htf)

    def call(**kw):
        a = dict(args, **kw)
        return L.lib.htf_bp_descriptor(a["nlist"], a["dt"], a["B"], a["NN"], a["K"], a["T"], a["mu"], a["gap"], a["out"], a["odt"],
                                       a["rc"], None)

    for bad in COMMON_BAD + (dict(odt=3), dict(out=None)):
        if "n_rows" in bad:
            continue
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    # zero rows: nothing to launch, no pointer to read; with rows the pointers are required
    assert call(B=0, nlist=None, out=None) == L.HTF_OK and call(B=0, nlist=None, out=None, rc=2.5) == L.HTF_OK
    assert call(B=3, nlist=None, out=None) == L.HTF_ERR_INVALID and "descriptor network" in L.last_error()


def test_bp_loss_grad_entry_point_argument_errors(htf):
    L, mu, w, args = _args(htf)
    lib = L.lib

    def call(**kw):
        a = dict(args, **kw)
        return lib.htf_bp_loss_grad(a["nlist"], a["dt"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"], a["w"], a["mu"],
                                    a["gap"], a["labels"], a["ldt"], a["pred"], a["accum"], a["scratch"], a["rows"], a["n_rows"],
                                    a["rc"], None)

    for bad in COMMON_BAD + (dict(H1=0), dict(H2=65), dict(act=7), dict(ldt=3), dict(w=None), dict(labels=None), dict(pred=None),
                             dict(accum=None), dict(scratch=None), dict(B=0, w=None), dict(B=0, n_rows=1)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    # B = 0: HTF_OK with no row pointer to read and, without an accum to zero-fill, no launch; the limits are still checked
    none = dict(B=0, n_rows=0, nlist=None, labels=None, pred=None, accum=None, scratch=None)
    assert call(**none) == L.HTF_OK
    assert call(K=1, **none) == L.HTF_ERR_INVALID and "descriptor network" in L.last_error()
    # the scratch size: one partial [1 + P] per block, min(ceil(n_rows / 64), 512) of them -- a function of n_rows alone
    P = w.numel()
    assert lib.htf_bp_scratch_floats(0, 8, 1, 8, 8) == 0
    for n, parts in ((1, 1), (64, 1), (65, 2), (300, 5), (64 * 512, 512), (1 << 20, 512), (1 << 24, 512)):
        assert lib.htf_bp_scratch_floats(n, 8, 1, 8, 8) == parts * (1 + P)
    assert lib.htf_bp_scratch_floats(4, 1, 1, 8, 8) == 0


def test_desc_train_zero_rows_is_ok(htf):
    """B = 0: HTF_OK with no row pointer to read and, without an accum to zero-fill, no launch; the limits are still checked."""
    L = htf._lib
    mu, w = torch.zeros(8), torch.zeros(8 * 8 + 8 + 8 * 8 + 8 + 8 + 1)

    def call(K):
        return L.lib.htf_bp_loss_grad(None, L.HTF_F32, 0, 16, K, 1, 8, 8, L.ACT_TANH, w.data_ptr(), mu.data_ptr(), 0.5, None,
                                      L.HTF_F32, None, None, None, None, 0, 0.0, None)

    assert call(8) == L.HTF_OK
    assert call(1) == L.HTF_ERR_INVALID and "descriptor network" in L.last_error()


def test_desc_entry_point_argument_errors(htf):
    """The default layer's call -- no list, n_rows = B, no cutoff -- keeps every check its own entry points had."""
    L = htf._lib
    lib = L.lib
    mu = torch.zeros(8)
    w = torch.zeros(8 * 8 + 8 + 8 * 8 + 8 + 8 + 1)
    args = dict(nlist=0x1000, dt=L.HTF_F32, B=4, NN=16, K=8, T=1, H1=8, H2=8, act=L.ACT_TANH, w=w.data_ptr(), mu=mu.data_ptr(),
                gap=0.5, out=0x2000, odt=L.HTF_F32)

    def call(**kw):
        a = dict(args, **kw)
        return lib.htf_bp_forces(a["nlist"], a["dt"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"], a["w"], a["mu"],
                                 a["gap"], a["out"], a["odt"], None, None, a["B"], 0.0, None)

    for bad in (dict(K=1), dict(K=33, T=2), dict(NN=257), dict(H1=0), dict(H2=65), dict(act=7), dict(gap=0.0), dict(gap=-1.0),
                dict(dt=5), dict(odt=3), dict(mu=None), dict(w=None), dict(nlist=None), dict(out=None)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    # zero rows: nothing to launch, no pointer to read
    assert call(B=0, nlist=None, out=None) == L.HTF_OK
    assert lib.htf_bp_descriptor(None, L.HTF_F32, 0, 16, 8, 1, mu.data_ptr(), 0.5, None, L.HTF_F32, 0.0, None) == L.HTF_OK
    assert lib.htf_bp_descriptor(None, L.HTF_F32, 3, 16, 8, 1, mu.data_ptr(), 0.5, None, L.HTF_F32, 0.0, None) == L.HTF_ERR_INVALID


def test_desc_train_entry_point_argument_errors(htf):
    """The default layer's sweep -- no list, n_rows = B, no cutoff -- keeps every check its own entry point had."""
    L = htf._lib
    lib = L.lib
    mu = torch.zeros(8)
    w = torch.zeros(8 * 8 + 8 + 8 * 8 + 8 + 8 + 1)
    args = dict(nlist=0x1000, dt=L.HTF_F32, B=4, NN=16, K=8, T=1, H1=8, H2=8, act=L.ACT_TANH, w=w.data_ptr(), mu=mu.data_ptr(),
                gap=0.5, labels=0x2000, ldt=L.HTF_F32, pred=0x3000, accum=0x4000, scratch=0x5000)

    def call(**kw):
        a = dict(args, **kw)
        return lib.htf_bp_loss_grad(a["nlist"], a["dt"], a["B"], a["NN"], a["K"], a["T"], a["H1"], a["H2"], a["act"], a["w"],
                                    a["mu"], a["gap"], a["labels"], a["ldt"], a["pred"], a["accum"], a["scratch"], None, a["B"], 0.0,
                                    None)

    for bad in (dict(K=1), dict(K=33, T=2), dict(NN=257), dict(H1=0), dict(H2=65), dict(act=7), dict(gap=0.0), dict(gap=-1.0),
                dict(dt=5), dict(ldt=3), dict(mu=None), dict(w=None), dict(nlist=None), dict(labels=None), dict(pred=None),
                dict(accum=None), dict(scratch=None), dict(B=0, w=None)):
        assert call(**bad) == L.HTF_ERR_INVALID, bad
        assert "descriptor network" in L.last_error()
    # the scratch size: one partial [1 + P] per block, a function of the row count and the widths alone; nothing for no rows
    P = w.numel()
    assert lib.htf_bp_scratch_floats(0, 8, 1, 8, 8) == 0
    n1 = lib.htf_bp_scratch_floats(1, 8, 1, 8, 8)
    assert n1 >= 1 + P and n1 % (1 + P) == 0
    assert lib.htf_bp_scratch_floats(1 << 20, 8, 1, 8, 8) == lib.htf_bp_scratch_floats(1 << 24, 8, 1, 8, 8) >= n1
