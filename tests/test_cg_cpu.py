"""Coarse-grained mapping on the host: ``sparse_mapping`` (test_utils.py:87-154 of hoomd-tf) and the argument checks of
``center_of_mass`` / ``compute_nlist`` that run before any kernel.  No GPU."""
import numpy as np
import pytest
import torch

# test_utils.py:88-98: ten atoms of one molecule onto three beads (written N x B, used B x N)
MAPPING = np.array([
    [1, 0, 0],
    [1, 0, 0],
    [0, 1, 0],
    [0, 1, 0],
    [1, 0, 0],
    [0, 0, 1],
    [0, 0, 1],
    [0, 0, 1],
    [1, 0, 0],
    [0, 1, 0]]).transpose()


def _molecules(htf, n_mol=4, masses=None):
    """A stand-in system of ``n_mol`` ten-atom chains (bonds i - i+1 inside a molecule)."""
    from hoomd_tf_amd import standin
    rng = np.random.default_rng(5)
    N = 10 * n_mol
    system = standin.System(rng.uniform(-4, 4, (N, 3)), [10.0, 10.0, 10.0], device="cpu")
    system.bonds = [(m * 10 + i, m * 10 + i + 1) for m in range(n_mol) for i in range(9)]
    if masses is not None:
        system.vel[:, 3] = torch.as_tensor(masses, dtype=system.vel.dtype)
    return system


def test_bad_sparse_mapping(htf):
    system = _molecules(htf)
    mapping = htf.find_molecules(system)
    assert len(mapping) == 4
    with pytest.raises(ValueError):          # one matrix for four molecules
        htf.sparse_mapping([MAPPING], mapping, device="cpu")
    with pytest.raises(ValueError):          # nine columns for ten atoms
        htf.sparse_mapping([MAPPING[:, :-1] for _ in mapping], mapping, device="cpu")
    with pytest.raises(TypeError):
        htf.sparse_mapping([MAPPING.tolist() for _ in mapping], mapping, device="cpu")


def test_sparse_mapping(htf):
    system = _molecules(htf)
    mapping = htf.find_molecules(system)
    s = htf.sparse_mapping([MAPPING for _ in mapping], mapping, device="cpu")
    N = system.N
    assert s.layout == torch.sparse_coo and s.is_coalesced() and s.dtype == torch.float32
    assert tuple(s.shape) == (3 * len(mapping), N)
    # the "mapped forces" idiom: sparse @ dense
    m = torch.sparse.mm(s, torch.ones((N, 1)))
    assert int(m.sum()) == len(mapping) * MAPPING.shape[1]
    dense = s.to_dense().numpy()
    np.testing.assert_array_almost_equal(dense[:MAPPING.shape[0], :MAPPING.shape[1]], MAPPING)
    assert np.sum(dense[:MAPPING.shape[0], -MAPPING.shape[1]:]) < 1e-10        # off-diagonal block
    np.testing.assert_array_equal(dense.sum(axis=1), np.tile(MAPPING.sum(axis=1), len(mapping)))
    assert abs(np.abs(dense.sum(axis=1)).sum() - dense.shape[1]) < 1e-10       # (upstream's row-sum check)
    # every molecule's block sits on the diagonal
    for k in range(len(mapping)):
        np.testing.assert_array_equal(dense[3 * k:3 * k + 3, 10 * k:10 * k + 10], MAPPING)


def test_sparse_mapping_mass_weighted(htf):
    masses = np.tile([12.0, 1.0, 1.0, 16.0, 1.0, 14.0, 1.0, 2.0, 3.0, 4.0], 4)
    system = _molecules(htf, masses=masses)
    mapping = htf.find_molecules(system)
    s = htf.sparse_mapping([MAPPING for _ in mapping], mapping, system=system, device="cpu")
    dense = s.to_dense().numpy()
    np.testing.assert_allclose(dense.sum(axis=1), 1.0, rtol=1e-6)
    w = MAPPING * masses[:10]
    np.testing.assert_allclose(dense[:3, :10], w / w.sum(axis=1, keepdims=True), rtol=1e-6)
    # raw entries are kept without a system (here: not 0/1)
    s2 = htf.sparse_mapping([2.5 * MAPPING for _ in mapping], mapping, device="cpu")
    np.testing.assert_array_equal(s2.to_dense().numpy()[:3, :10], 2.5 * MAPPING)


def test_cg_ops_need_device_tensors(htf):
    s = htf.sparse_mapping([MAPPING], [list(range(10))], device="cpu")
    with pytest.raises(ValueError):
        htf.center_of_mass(torch.zeros((10, 3)), s, [10.0, 10.0, 10.0])
    with pytest.raises(ValueError):
        htf.compute_nlist(torch.zeros((10, 3)), 2.0, 4, [10.0, 10.0, 10.0])


def test_cg_abi_table(htf):
    """The coarse-grained entry points are a third table, the symbols of include/htf_cg.h, exported by the library and
    bound under whichever binding is active; the two tables of htf_amd.h / htf_standin.h are unchanged."""
    import ctypes
    import os
    import re
    from helpers import ROOT
    hdr = open(os.path.join(ROOT, "include", "htf_cg.h")).read()
    names = sorted(set(re.findall(r"HTF_API[^;]*?\b(htf_cg_\w+)\s*\(", hdr)))
    assert names == sorted(htf._lib.CG_PROTOTYPES) and len(names) == 4
    raw = ctypes.CDLL(htf._lib.LIB_PATH)
    for n in names:
        assert hasattr(raw, n) and hasattr(htf._lib.lib, n)
    assert not set(names) & (set(htf._lib.PROTOTYPES) | set(htf._lib.STANDIN_PROTOTYPES))


def test_cg_header_is_plain_c():
    """include/htf_cg.h compiles as C99 beside htf_amd.h (no C++ or torch types in the signatures)."""
    import os
    import subprocess
    import tempfile
    from helpers import ROOT
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write('#include "htf_amd.h"\n#include "htf_cg.h"\nint main(void){return HTF_CG_MAX_NN == 256 ? HTF_OK : 1;}\n')
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src,
                               "-o", os.path.join(d, "t")])
