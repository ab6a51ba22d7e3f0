"""Every kernel that takes an ``htf_box`` on the boxes that leave its fast path: per-axis ``periodic`` flags (a HOOMD run under
domain decomposition has periodic = 0 along each decomposed axis; integration/hoomd_shim copies getPeriodic() into every call)
and tilt factors that pass upstream's skew rule (sum(tilt) < 1e-4).  The switch is the same line everywhere --
``box.ortho && box.periodic[0] && box.periodic[1] && box.periodic[2]`` -- and behind it sits HOOMD's BoxDim::minImage
(csrc/box_math.h), whose pair vectors must equal the oracle's bit for bit whichever kernel forms them.

Fixtures and box cases: tests/box_cases.py (their conditions are asserted on the oracle alone in tests/test_oracle_c.py).
Every tolerance is the one the fully periodic test of the same kernel on the same fixture family uses, named where it is taken.

What each entry point launches on these cases (read off the dispatch code; PT = position, DT = destination precision):
  build_pair_vectors      build_pair_vectors_kernel<PT, DT, 4> (fp32 positions) / <PT, DT, 2> (fp64), all four (PT, DT): the
                          multi-row path's pair_vector branch, build_row's sweep<.., false> and the replay sweep<.., true>
  build_pair_index        cf_pair_kernel<PT>: index_sweep<PT, false> and, on overflow, <PT, true>
  fused_forces            fused_forces_rows2_kernel<LJ | WCA | RINV_POLY, STORE, 2, PT, 0> (STORE = with / without the tensor;
                          fused_rows_group's general branch and single-row fallback); virial: fused_forces_kernel<LJ, true, STORE, PT>;
                          fused_forces_tails_kernel<KIND, STORE, 2 | 4, PT, 0> forced on the variants build at fixture size and, in
                          the shipped library, <LJ, STORE, 2, float, 0> at 16 384 rows and <LJ, STORE, 4, float, 0> at 49 152
  build_eval_forces2      fused_forces2_kernel<RINV_POLY, STORE, true, PT> (NN <= 128: compacting) and <.., false, PT> (NN 256);
                          fused_forces2_tails_kernel<WCA | LJ, STORE, 2, PT> (sweep2_rows_group_tails' generic rows)
  train_pair_grad_list    train_list_kernel<LJ_PARAM | WCA | RINV_POLY | JIT, PT> against train_pair_kernel<KIND, float>
  Context                 fused 0: build_pair_vectors_kernel<PT, float, 4 | 2> + the LJ evaluator; fused 1 / 2:
                          fused_forces_rows2_kernel<LJ, false | true, 2, PT, 0>; whole, in batches of 7, in two row ranges
  generated kernel        the Morse unit's fused_forces_rows2_kernel<JIT, STORE, 2, PT, 0>
  stand-in                cell_ranges_kernel's px / py / pz, build_nlist_kernel<T, ..> (below 1 024 cells) and
                          build_nlist_cells_kernel<T, ..> (from 1 024 on); nve_step_kernel<T>, nve_check_kernel<T>,
                          max_disp_kernel<T>; FusedStep: fused_forces_rows2_kernel<LJ, true, 2, float, 1> (the epilogue's rare path)
  shim (test_gpu_shim.py) TensorflowComputeAMD -> htf_compute_forces, fused 2, double precision
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import box_cases as BC
from helpers import ROOT
from oracle import htf_oracle as O
from test_gpu_parity import CONTACTS, _cond_scale, _pair_forces_lj, _record, _to_dev, assert_forces_close

pytestmark = pytest.mark.gpu

NAMES = BC.BOX_IDS
HDTS = pytest.mark.parametrize("hdt", BC.DTYPES, ids=["f32", "f64"])
BOXES = pytest.mark.parametrize("name", NAMES)


def _tdt(hdt):
    return torch.float64 if hdt == np.float64 else torch.float32


@functools.lru_cache(maxsize=None)
def _ref(which, hdt, name, NN, r_cut, offset=0, batch=None):
    """The oracle's tensor of a fixture on a box case: computed once, shared, read-only."""
    (pos, types, L, nn, head, nl), box, periodic = BC.fixture(which, hdt, name)
    t = O.prepare_neighbors(pos, types, nn, head, nl, box, r_cut, NN, offset=offset, batch_size=batch, periodic=periodic)
    t.setflags(write=False)
    return t


def _case(htf, cuda, which, hdt, name):
    sysm, box, periodic = BC.fixture(which, hdt, name)
    pos, types, L, nn, head, nl = sysm
    return sysm, box, periodic, _to_dev(htf, pos, types, nn, head, nl, hdt, cuda)


def _shapes(which):
    """(NN, r_cut, offset, batch) of a fixture: F1's tables, F2's two widths over all rows."""
    if which == "F1":
        return [(NN, rc, off, bs) for NN, rc in BC.F1_TABLE for off, bs in BC.F1_BATCHES]
    return [(NN, BC.F2_RCUT, 0, 256) for NN in BC.F2_NN]


def _wca_cond(t64, sigma=1.0):
    s, t, rp, cond = O._rinv_and_grad_factor(t64)
    return _cond_scale(t64, 2 * O._grad_from_dEds(6 * sigma ** 6 * s ** 5, s, t, rp, cond))     # as test_wca_forces


def _rinv_cond(t64):
    s, t, rp, cond = O._rinv_and_grad_factor(t64)
    return _cond_scale(t64, 2 * O._grad_from_dEds(np.ones_like(s), s, t, rp, cond))


# --------------------------------------------------------------------------- 2. ops.build_pair_vectors
@pytest.mark.parametrize("which", ["F1", "F2"])
@BOXES
@HDTS
def test_build_pair_vectors(htf, cuda, which, name, hdt):
    """build_pair_vectors_kernel<PT, DT, 4 | 2>: the multi-row fast path's general branch (pair_vector), build_row's sweep for the
    rows it hands back (empty, longer than 192 entries, a batch's last rows) and the overflow replay (F1 at NN 16, F2 at NN 32), all
    four (position, destination) precisions: the oracle's tensor bit for bit, and the largest kept count."""
    sysm, box, periodic, (p4, dnn, dhead, dnl) = _case(htf, cuda, which, hdt, name)
    for NN, r_cut, off, bs in _shapes(which):
        ref = _ref(which, hdt, name, NN, r_cut, off, bs)
        want = int(BC.kept_counts(sysm, box, periodic, r_cut, off, bs).max())
        for odt in (np.float32, np.float64):
            mc = torch.zeros(1, dtype=torch.int32, device=cuda)
            out = htf.ops.build_pair_vectors(p4, dnn, dhead, dnl, box, r_cut, NN, offset=off, batch_size=bs, max_count=mc,
                                             out_dtype=_tdt(odt), periodic=periodic)
            np.testing.assert_array_equal(out.cpu().numpy(), ref.astype(odt), err_msg=str((NN, r_cut, off, bs, odt)))
            assert int(mc.item()) == want
    if which == "F2":
        assert want > 32      # NN = 32 overflows


# --------------------------------------------------------------------------- 3. ops.build_pair_index
@pytest.mark.parametrize("which", ["F1", "F2"])
@BOXES
@HDTS
def test_build_pair_index(htf, cuda, which, name, hdt):
    """cf_pair_kernel<PT> (index_sweep, its replay on overflow): the particle of every slot as the oracle's slot order implies,
    -1 in the slots that stay empty, and the same slots occupied as in the tensor."""
    sysm, box, periodic, (p4, dnn, dhead, dnl) = _case(htf, cuda, which, hdt, name)
    for NN, r_cut, off, bs in _shapes(which):
        want = BC.pair_index(sysm, box, periodic, r_cut, NN, off, bs)
        got = htf.ops.build_pair_index(p4, dnn, dhead, dnl, box, r_cut, NN, offset=off, batch_size=bs, periodic=periodic).cpu().numpy()
        np.testing.assert_array_equal(got, want, err_msg=str((NN, r_cut, off, bs)))
        pv = htf.ops.build_pair_vectors(p4, dnn, dhead, dnl, box, r_cut, NN, offset=off, batch_size=bs, periodic=periodic).cpu().numpy()
        occupied = (pv != 0).any(axis=2)
        assert not np.any(occupied & (got < 0))
        if which == "F2":   # (no self pairs: every kept entry has a non-zero vector)
            np.testing.assert_array_equal(occupied, got >= 0)
        assert (got < 0).any() or NN <= 32


# --------------------------------------------------------------------------- 4. ops.fused_forces
def _fused_body(htf, cuda, name, hdt, tag=""):
    """F1: the tensor the fused kernels write.  F2: tensor, forces, check_count, with and without the tensor, LJ (also with the
    virial: the one-row kernel), WCA and r^-1."""
    # F1: tensors only (random rows with contacts and self pairs)
    sysm, box, periodic, (p4, dnn, dhead, dnl) = _case(htf, cuda, "F1", hdt, name)
    for NN, r_cut, off, bs in _shapes("F1"):
        ref32 = _ref("F1", hdt, name, NN, r_cut, off, bs).astype(np.float32)
        for pot in (htf.Potential.lj(), htf.Potential.wca(1.0)):
            pv = torch.full((bs, NN, 4), 7.0, dtype=torch.float32, device=cuda)
            htf.ops.fused_forces(pot, p4, dnn, dhead, dnl, box, r_cut, NN, offset=off, batch_size=bs, pair_vectors=pv, periodic=periodic)
            np.testing.assert_array_equal(pv.cpu().numpy(), ref32, err_msg=str((pot.kind, NN, r_cut, off, bs)))
    # F2
    sysm, box, periodic, (p4, dnn, dhead, dnl) = _case(htf, cuda, "F2", hdt, name)
    models = (("lj", htf.Potential.lj(), O.lj_model, lambda t: _cond_scale(t, _pair_forces_lj(t))),
              ("wca", htf.Potential.wca(1.0), lambda t: O.wca_model(t, 1.0), _wca_cond),
              ("rinv", htf.Potential.rinv_poly([1.0], [1]), lambda t: O.rinv_poly_model(t, [1.0], [1]), _rinv_cond))
    for NN in BC.F2_NN:
        ref32 = _ref("F2", hdt, name, NN, BC.F2_RCUT).astype(np.float32)
        t64 = ref32.astype(np.float64)
        pv0 = htf.ops.build_pair_vectors(p4, dnn, dhead, dnl, box, BC.F2_RCUT, NN, periodic=periodic)
        np.testing.assert_array_equal(pv0.cpu().numpy(), ref32)
        for key, pot, model, cond_of in models:
            cc = torch.zeros(1, dtype=torch.int32, device=cuda)
            f = htf.ops.fused_forces(pot, p4, dnn, dhead, dnl, box, BC.F2_RCUT, NN, check_count=cc, periodic=periodic)
            assert int(cc.item()) == htf.ops.check_nlist(pv0) == O.check_nlist_count(ref32)
            pv = torch.full_like(pv0, 7.0)
            f2 = htf.ops.fused_forces(pot, p4, dnn, dhead, dnl, box, BC.F2_RCUT, NN, pair_vectors=pv, periodic=periodic)
            assert torch.equal(pv, pv0), (key, NN)
            assert torch.equal(f2, f), (key, NN)
            f3 = htf.ops.fused_forces(pot, p4, dnn, dhead, dnl, box, BC.F2_RCUT, NN, periodic=periodic)
            assert torch.equal(f3, f), (key, NN)
            assert f.dtype == p4.dtype
            # (jittered fcc with a = 1.6: contacts at r ~ 0.7-0.9, pair forces 100x the row sums -- the named condition term of
            #  test_fused_matches_two_kernel_path_and_oracle on this fixture, from each potential's own pair forces)
            assert_forces_close("gbox%s_fused_%s_%s_NN%d_%s" % (tag, key, name, NN, hdt.__name__), f.cpu().numpy(), model(t64), cond_of(t64),
                                cancelling_rows=CONTACTS)
        # the virial: fused_forces_kernel<LJ, true, STORE, PT>
        cond = _cond_scale(t64, _pair_forces_lj(t64))
        rf, rv = O.lj_model(t64, virial=True)
        fv, vv = htf.ops.fused_forces(htf.Potential.lj(), p4, dnn, dhead, dnl, box, BC.F2_RCUT, NN, virial=True, periodic=periodic)
        pv = torch.full_like(pv0, 7.0)
        fv2, vv2 = htf.ops.fused_forces(htf.Potential.lj(), p4, dnn, dhead, dnl, box, BC.F2_RCUT, NN, virial=True, pair_vectors=pv, periodic=periodic)
        assert torch.equal(pv, pv0) and torch.equal(fv2, fv) and torch.equal(vv2, vv)
        assert_forces_close("gbox%s_fused_ljv_f_%s_NN%d_%s" % (tag, name, NN, hdt.__name__), fv.cpu().numpy(), rf, cond, cancelling_rows=CONTACTS)
        assert_forces_close("gbox%s_fused_ljv_v_%s_NN%d_%s" % (tag, name, NN, hdt.__name__), vv.cpu().numpy(), rv, 3 * cond, cancelling_rows=CONTACTS)


@BOXES
@HDTS
def test_fused_forces_body(htf, cuda, name, hdt):
    """The shipped forms at this size: fused_forces_rows2_kernel<KIND, STORE, 2, PT, 0> (fused_rows_group's general branch, its
    single-row fallback) and, for the virial, the one-row fused_forces_kernel<LJ, true, STORE, PT>.  Run again on the variants
    build with the merged-tails forms forced by test_fused_forces_merged_tails_forced."""
    _fused_body(htf, cuda, name, hdt, tag=os.environ.get("HTF_GBOX_TAG", ""))


@pytest.mark.parametrize("tails", ["2", "4"])
def test_fused_forces_merged_tails_forced(htf, cuda, tails):
    """fused_forces_tails_kernel<KIND, STORE, 2 | 4, PT, 0>: the group's ``fast`` test fails for every group on these boxes, so
    every row goes through the generic single-row routine -- forced at fixture size in a child process on the variants build."""
    from helpers import variants_env
    env = variants_env(HTF_FUSED_TAILS=tails, HTF_STATS_NO_FILE="1", HTF_GBOX_TAG="_tails" + tails)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_fused_forces_body"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


def _fcc_block(cells, rho=0.8442):
    a = (4.0 / rho) ** (1.0 / 3.0)
    cells = np.asarray(cells)
    L = cells * a
    ijk = np.stack(np.meshgrid(*[np.arange(c) for c in cells], indexing="ij"), -1).reshape(-1, 3)
    base = np.array([[0.25, 0.25, 0.25], [0.75, 0.75, 0.25], [0.75, 0.25, 0.75], [0.25, 0.75, 0.75]])
    return ((ijk[:, None, :] + base[None]) * a).reshape(-1, 3) - L / 2, L, a


@pytest.mark.parametrize("cells", [(16, 16, 16), (24, 32, 16)], ids=["16384-rows", "49152-rows"])
def test_fused_forces_merged_tails_at_their_own_size(htf, cuda, cells):
    """The shipped library at the smallest batches that select fused_forces_tails_kernel<LJ, STORE, 2, float> (16 384 rows) and
    <LJ, STORE, 4, float> (49 152), open along z: the tensor of EVERY row against the C restatement, the forces of every row
    against the two-row form of the same call (the same rows in batches below 16 384) within that form's rounding, 512 sampled
    rows against the oracle."""
    from hoomd_tf_amd import standin
    from oracle import c_oracle
    periodic, NN, r_cut = (1, 1, 0), 128, 3.0
    pos, L, a = _fcc_block(cells)
    rng = np.random.default_rng(7)
    pos = pos + 0.05 * a * rng.standard_normal(pos.shape)
    pos -= np.round(pos / L) * L
    sysm = standin.System(pos, L, dtype=torch.float32, device=cuda)      # the list: the fully periodic one
    nl = standin.CellNlist(sysm, r_cut=r_cut, r_buff=0.4)
    nl.build()
    N = sysm.N
    assert N == 4 * int(np.prod(cells)) and N in (16384, 49152)
    box = O.make_box(L, dtype=np.float32)
    args = (sysm.pos, nl.n_neigh, nl.head_list, nl.nlist, box, r_cut, NN)
    ref = c_oracle.prepare_neighbors(c_oracle.load(), sysm.pos.cpu().numpy(), nl.n_neigh.cpu().numpy().view(np.uint32),
                                     nl.head_list.cpu().numpy().view(np.uint32), nl.nlist.cpu().numpy().view(np.uint32), box, r_cut, NN,
                                     periodic=periodic)
    plain = htf.ops.build_pair_vectors(*args).cpu().numpy()
    # the open axis is seen by the rows within r_cut of its faces: 2 r_cut / L_z = 0.22 of them, less those whose partners stay
    assert (plain != ref).any(axis=(1, 2)).mean() > 0.1
    pv = torch.full((N, NN, 4), 7.0, dtype=torch.float32, device=cuda)
    f_store = htf.ops.fused_forces(htf.Potential.lj(), *args, pair_vectors=pv, periodic=periodic)
    np.testing.assert_array_equal(pv.cpu().numpy(), ref)
    f_reg = htf.ops.fused_forces(htf.Potential.lj(), *args, periodic=periodic)
    assert torch.equal(f_reg, f_store)
    np.testing.assert_array_equal(htf.ops.build_pair_vectors(*args, periodic=periodic).cpu().numpy(), ref)
    # the two-row form: the same rows in batches of 8 192
    two = torch.cat([htf.ops.fused_forces(htf.Potential.lj(), *args, offset=off, batch_size=8192, periodic=periodic) for off in range(0, N, 8192)])
    scale = float(two.abs().max())
    worst = float((f_reg - two).abs().max())
    _record("gbox_tails_vs_two_row_form_%d" % N, max_abs_err=worst, max_ratio=worst / (2e-6 * scale))
    assert worst <= 2e-6 * scale          # test_fused_matches_two_kernel_path_and_oracle's bound for batches
    rows = np.random.default_rng(5).choice(N, 512, replace=False)
    sub = ref[rows].astype(np.float64)
    ref_f = O.lj_model(sub)
    cond = _cond_scale(sub, _pair_forces_lj(sub))
    s_, _, _, _ = O._rinv_and_grad_factor(sub)
    e_cond = (2.0 * (s_ ** 12 + s_ ** 6)).sum(axis=1)       # as test_full_size_pair_vectors_every_row_bit_exact
    for key, f in (("registers", f_reg), ("one_kernel", f_store)):
        got = f.cpu().numpy()[rows]
        assert_forces_close("gbox_tails_%d_lj_%s_energy" % (N, key), got[:, 3], ref_f[:, 3], e_cond, cancelling_rows=CONTACTS)
        assert_forces_close("gbox_tails_%d_lj_%s" % (N, key), got[:, :3], ref_f[:, :3], cond, cancelling_rows=CONTACTS)


# --------------------------------------------------------------------------- 5. ops.build_eval_forces2
@BOXES
@HDTS
def test_build_eval_forces2(htf, cuda, name, hdt):
    """Config C4's sweep in one kernel on a general box, against build_pair_vectors(periodic=...) -> eval_forces2: tensor and
    histogram bit for bit, both force sets and the CV sum within test_build_eval_forces2_equals_build_then_eval2's bounds.  Base
    potentials: r^-1 takes the compacting persistent kernel fused_forces2_kernel<RINV_POLY, STORE, true, PT> (NN 256: the in-place
    form <.., false, PT>); WCA and LJ the rows-per-wave form fused_forces2_tails_kernel<KA, STORE, 2, PT> (sweep2_rows_group_tails:
    ``fast`` fails for every group, the generic single-row routine and its overflow un-binning do the work)."""
    gauss = htf.Potential.gauss(1.1, 0.05, 1.0)
    for which in ("F1", "F2"):
        sysm, box, periodic, (p4, dnn, dhead, dnl) = _case(htf, cuda, which, hdt, name)
        bases = [htf.Potential.rinv_poly([1.0], [1]), htf.Potential.wca(1.0)] + ([htf.Potential.lj()] if which == "F2" else [])
        for NN, r_cut, off, bs in _shapes(which):
            ref32 = _ref(which, hdt, name, NN, r_cut, off, bs).astype(np.float32)
            pv0 = htf.ops.build_pair_vectors(p4, dnn, dhead, dnl, box, r_cut, NN, offset=off, batch_size=bs, periodic=periodic)
            np.testing.assert_array_equal(pv0.cpu().numpy(), ref32)
            for base in bases:
                what = (which, base.kind, NN, r_cut, off, bs)
                h0 = torch.zeros(102, dtype=torch.int32, device=cuda)
                part0 = torch.zeros(htf.ops.num_partials(bs, NN), device=cuda)
                fa0, fb0 = htf.ops.eval_forces2(base, gauss, pv0, partials=part0, rdf=(0.0, 3.5, h0), out_dtype=p4.dtype)
                h1 = torch.zeros(102, dtype=torch.int32, device=cuda)
                part1 = torch.zeros(htf.ops.num_partials_fused(bs), device=cuda)
                pv1 = torch.full_like(pv0, 7.0)
                fa1, fb1 = htf.ops.build_eval_forces2(base, gauss, p4, dnn, dhead, dnl, box, r_cut, NN, offset=off, batch_size=bs,
                                                      partials=part1, rdf=(0.0, 3.5, h1), pair_vectors=pv1, periodic=periodic)
                assert torch.equal(pv1, pv0), what
                assert torch.equal(h1, h0) and int(h0.sum()) == bs * NN, what
                if which == "F1":
                    continue
                for key, a, b in (("a", fa1, fa0), ("b", fb1, fb0)):
                    bound = 2e-5 * max(1.0, float(b.abs().max()))
                    worst = float((a - b).abs().max())
                    _record("gbox_eval2_%s_%s_%s_NN%d_%s" % (base.kind, key, name, NN, hdt.__name__), max_abs_err=worst, max_ratio=worst / bound)
                    assert worst <= bound, what
                assert abs(float(part1.sum()) - float(part0.sum())) <= 2e-5 * abs(float(part0.sum())), what
                fa2, fb2 = htf.ops.build_eval_forces2(base, gauss, p4, dnn, dhead, dnl, box, r_cut, NN, periodic=periodic)   # tensor-less
                assert torch.equal(fa2, fa1) and torch.equal(fb2, fb1), what


# --------------------------------------------------------------------------- 6. ops.train_pair_grad_list
@pytest.mark.parametrize("kind", ["lj_param", "wca", "rinv_poly", "traced"])
@pytest.mark.parametrize("name", ["open-z", "tilt-neg"])
@pytest.mark.parametrize("NN,hdt", [(128, np.float32), (32, np.float32), (128, np.float64)], ids=["NN128-f32", "NN32-f32", "NN128-f64"])
def test_train_pair_grad_list(htf, cuda, kind, name, NN, hdt):
    """train_pair.hip's sweep from the index list (pair_vector in registers) against htf_train_pair_grad on the tensor of
    build_pair_vectors(periodic=...): test_training_sweep_from_the_index_list_equals_the_tensor_sweep's potentials and bounds."""
    sysm, box, periodic, (p4, dnn, dhead, dnl) = _case(htf, cuda, "F2", hdt, name)
    if kind == "lj_param":
        pot = htf.Potential.lj_param(0.9, 1.05, theta=torch.tensor([0.9, 1.05], device=cuda))
    elif kind == "wca":
        pot = htf.Potential.wca(0.95, theta=torch.tensor([0.95], device=cuda))
    elif kind == "rinv_poly":
        pot = htf.Potential.rinv_poly([1.5, -2.5], [12, 6], theta=torch.tensor([1.5, -2.5], device=cuda))
    else:
        x0 = htf.Nlist(torch.zeros((2, 4, 4), device=cuda))
        w = torch.nn.Parameter(torch.tensor([0.8, 1.05], device=cuda))
        q = (w[1] * htf.nlist_rinv(x0)) ** 6
        e = htf.reduce_sum(w[0] * 2.0 * (q * q - q), axis=1)
        assert e.lowers()
        pot = e.layer.potential(cuda)
    N = len(sysm[0])
    pv = htf.ops.build_pair_vectors(p4, dnn, dhead, dnl, box, BC.F2_RCUT, NN, periodic=periodic)
    np.testing.assert_array_equal(pv.cpu().numpy(), _ref("F2", hdt, name, NN, BC.F2_RCUT).astype(np.float32))
    labels = (0.05 * torch.randn((N, 4), generator=torch.Generator().manual_seed(3))).to(cuda)
    p0, p1 = torch.empty((N, 4), device=cuda), torch.empty((N, 4), device=cuda)
    a0 = htf.ops.train_pair_grad(pot, pv, labels, pred=p0)
    a1 = htf.ops.train_pair_grad_list(pot, p4, dnn, dhead, dnl, box, BC.F2_RCUT, NN, labels, pred=p1, periodic=periodic)
    assert torch.equal(a1, htf.ops.train_pair_grad_list(pot, p4, dnn, dhead, dnl, box, BC.F2_RCUT, NN, labels, periodic=periodic))
    scale = float(p0.abs().max())
    worst = float((p0 - p1).abs().max())
    _record("gbox_train_list_%s_%s_NN%d_%s" % (kind, name, NN, hdt.__name__), max_abs_err=worst, max_ratio=worst / (2e-6 * scale + 1e-7))
    assert worst <= 2e-6 * scale + 1e-7, worst / scale
    a0, a1 = a0.double().cpu().numpy(), a1.double().cpu().numpy()
    assert abs(a0[0] - a1[0]) <= 2e-6 * abs(a0[0])
    assert np.abs(a0[1:] - a1[1:]).max() <= 2e-5 * np.abs(a0[1:]).max() + 1e-6, (a0, a1)


# --------------------------------------------------------------------------- 7. the context
@pytest.mark.parametrize("which", ["F2", "F3"])
@BOXES
@HDTS
def test_context(htf, cuda, which, name, hdt):
    """htf_compute_forces on a general box: fused = 0 (build_pair_vectors_kernel + the evaluator), 1 and 2 (the one-kernel step
    without / with the tensor), whole, in batches of 7 and in two row ranges; the side buffer bit-identical to build_pair_vectors'.

    Forces against the oracle's computeForces with the bounds test_context_fused_mode uses between modes (rtol 2e-5, atol 1e-7) on
    F3.  On F2 that bound cannot be met by ANY fp32 row sum, whatever the box: its rows add ~170 pair forces of up to 10^3 to net
    forces of O(10), and the oracle's own fp32 restatement misses the fp64 forces there by as much as the kernels do (measured on
    the MI355X, fused = 0, whole step: 13-18 of 1 024 components outside, worst err / bound 19-143, largest difference 5.4e-5 on
    forces of ~20).  A property of the fixture, so the fixture changed: F3's rows hold one pair term each (box_cases.f3; the fp32
    restatement sits at 0.11 of the bound).  F2 keeps the tensor check and this project's bound for the same kernels on the same
    fixture (test_fused_matches_two_kernel_path_and_oracle: 1e-5 + 2e-5 |ref| and the named condition term)."""
    NN, r_cut = (128, BC.F2_RCUT) if which == "F2" else (BC.F3_NN, BC.F3_RCUT)
    sysm, box, periodic, (p4, dnn, dhead, dnl) = _case(htf, cuda, which, hdt, name)
    pos, types, L, nn, head, nl = sysm
    N = len(pos)
    ref32 = _ref(which, hdt, name, NN, r_cut).astype(np.float32)
    t64 = ref32.astype(np.float64)
    ref_f, _ = O.compute_forces(pos, types, nn, head, nl, box, r_cut, NN, lambda x: O.lj_model(x.astype(np.float64)),
                                model_dtype=np.float32, periodic=periodic)
    ref_f = ref_f.astype(np.float64)
    cond = _cond_scale(t64, _pair_forces_lj(t64))
    first = N // 3 + 1
    for fused in (0, 1, 2):
        for how in ("whole", "batched", "ranges"):
            ctx = htf.Context(r_cut=r_cut, nneighs=NN, batch_size=7 if how == "batched" else 0, scalar_dtype=_tdt(hdt), max_n=N, fused=fused)
            ctx.set_potential(htf.Potential.lj())
            force = torch.zeros((N, 4), dtype=_tdt(hdt), device=cuda)
            arr = ctx.make_arrays(p4, N, dnn, dhead, dnl, box, force, periodic=periodic)
            if how == "ranges":
                ctx.compute_forces(0, arr, rows=(0, first))
                ctx.compute_forces(0, arr, rows=(first, N - first))
                last = (0, N)           # (an unbatched context keeps row i of the step in row i of its side buffer)
            else:
                ctx.compute_forces(0, arr)
                last = (0, N) if how == "whole" else (N - (N % 7 or 7), N % 7 or 7)
            torch.cuda.synchronize()
            got = force.cpu().numpy().astype(np.float64)
            tag = "gbox_ctx_%s_%s_%s_fused%d_%s" % (which, name, hdt.__name__, fused, how)
            if which == "F3":
                err = np.abs(got - ref_f)
                bound = 1e-7 + 2e-5 * np.abs(ref_f)
                _record(tag, max_abs_err=err.max(), max_ratio=(err / bound).max(), max_ref=np.abs(ref_f).max())
                np.testing.assert_allclose(got, ref_f, rtol=2e-5, atol=1e-7, err_msg=str((fused, how)))
            else:
                assert_forces_close(tag, got, ref_f, cond, cancelling_rows=CONTACTS)
            if fused != 1:
                np.testing.assert_array_equal(ctx.nlist_buffer(last[1], cuda).cpu().numpy(), ref32[last[0]: last[0] + last[1]])
    if which == "F3":
        assert np.abs(ref_f[:, :3]).max() > 50 and (np.abs(ref_f).max(axis=1) == 0).sum() == (0 if sum(periodic) == 3 else (74 if sum(periodic) == 0 else 32))


@pytest.mark.parametrize("fused", [0, 2])
def test_context_tilt_rule_is_upstreams(htf, cuda, fused):
    """simmodel.py:195, tf.Assert(reduce_sum(box[2]) < 1e-4): tilt factors that sum to zero or less are evaluated (the cases above),
    a positive sum is refused -- (0.5, 0, 0) and (0.3, -0.2, 0.0)."""
    sysm, box, periodic, (p4, dnn, dhead, dnl) = _case(htf, cuda, "F2", np.float64, "tilt-neg")
    N = len(sysm[0])
    ctx = htf.Context(r_cut=BC.F2_RCUT, nneighs=128, scalar_dtype=torch.float64, max_n=N, fused=fused)
    ctx.set_potential(htf.Potential.lj())
    force = torch.zeros((N, 4), dtype=torch.float64, device=cuda)
    for tilt in (BC.NEG_TILT, BC.ZERO_SUM_TILT):
        ctx.compute_forces(0, ctx.make_arrays(p4, N, dnn, dhead, dnl, O.make_box(sysm[2], tilt=tilt), force))
    for tilt in ((0.5, 0.0, 0.0), (0.3, -0.2, 0.0)):
        with pytest.raises(htf.SkewedBoxError):
            ctx.compute_forces(0, ctx.make_arrays(p4, N, dnn, dhead, dnl, O.make_box(sysm[2], tilt=tilt), force))


# --------------------------------------------------------------------------- 8. one generated kernel
@pytest.mark.parametrize("name", ["open-x", "tilt-neg"])
@HDTS
def test_generated_kernel_through_the_fused_route(htf, cuda, name, hdt):
    """A generated unit's instantiations of the same templates (csrc/jit.hip: fused_forces_rows2_kernel<HTF_POT_JIT, STORE, 2, PT>
    around the traced Morse body): the tensor bit for bit, forces against torch-fp64 autograd of the expression on the reference
    tensor, with test_gpu_codegen.py's bounds."""
    from test_codegen_cpu import _models
    from test_gpu_codegen import _ref as autograd_ref
    sysm, box, periodic, (p4, dnn, dhead, dnl) = _case(htf, cuda, "F2", hdt, name)
    NN = 128
    ref32 = _ref("F2", hdt, name, NN, BC.F2_RCUT).astype(np.float32)
    t64 = ref32.astype(np.float64)
    e = _models(htf, htf.Nlist(torch.from_numpy(t64)))["morse"]
    pot = e.potential()
    pv = torch.full((len(ref32), NN, 4), 7.0, dtype=torch.float32, device=cuda)
    f = htf.ops.fused_forces(pot, p4, dnn, dhead, dnl, box, BC.F2_RCUT, NN, pair_vectors=pv, periodic=periodic)
    np.testing.assert_array_equal(pv.cpu().numpy(), ref32)
    assert torch.equal(f, htf.ops.fused_forces(pot, p4, dnn, dhead, dnl, box, BC.F2_RCUT, NN, periodic=periodic))
    ref = autograd_ref(htf, e, t64)
    xx = htf.Nlist(torch.from_numpy(t64))
    (g,) = torch.autograd.grad(e.torch_value(xx.ad).sum(), xx.ad)
    cond = np.abs(2 * g.numpy()[:, :, :3]).sum(axis=(1, 2))
    assert_forces_close("gbox_jit_morse_%s_%s" % (name, hdt.__name__), f.cpu().numpy(), ref, cond, cancelling_rows=CONTACTS)


# --------------------------------------------------------------------------- 9. the stand-in
def _brute_rows(pos, L, r_list, periodic):
    """helpers.brute_nlist under the flag-aware metric (the minimum image along the periodic axes only) -> sorted rows."""
    d = pos[None, :, :] - pos[:, None, :]
    for ax in range(3):
        if periodic[ax]:
            d[..., ax] -= np.round(d[..., ax] / L[ax]) * L[ax]
    m = (d * d).sum(axis=2) <= r_list * r_list
    np.fill_diagonal(m, False)
    return [np.nonzero(m[i])[0] for i in range(len(pos))]


@pytest.mark.parametrize("periodic", [(1, 1, 0), (0, 1, 1)], ids=["open-z", "open-x"])
@pytest.mark.parametrize("L,N,by_cell", [((9.0, 10.0, 11.0), 500, False), ((16.0, 17.0, 18.0), 2000, True)], ids=["per-particle", "per-cell"])
@pytest.mark.parametrize("tdt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_cell_nlist_with_an_open_axis(htf, cuda, tdt, L, N, by_cell, periodic):
    """CellNlist.build with ``System(periodic=...)``: the range table's px / py / pz and the search's per-axis minimum image against
    a brute-force list under the flag-aware metric, on a grid below 1 024 cells (the walk per particle) and one from 1 024 on (the
    walk per cell).  Bounds of test_cell_nlist_random_boxes_match_brute_force."""
    from hoomd_tf_amd import standin
    L = np.array(L)
    rng = np.random.default_rng(int(L[0]) + sum(periodic))
    pos = (rng.random((N, 3)) - 0.5) * L * 0.999          # every coordinate inside the box
    sysm = standin.System(pos, L, dtype=tdt, device=cuda, periodic=periodic)
    nl = standin.CellNlist(sysm, r_cut=2.5, r_buff=0.4)
    nl.build()
    ncell = int(nl._grid[2])
    assert (ncell >= 1024) == by_cell, ncell
    p = sysm.pos.cpu().numpy()[:, :3].astype(np.float64)
    ref = _brute_rows(p, L, 2.9, periodic)
    full = _brute_rows(p, L, 2.9, (1, 1, 1))
    nn_, head, flat = nl.n_neigh.cpu().numpy(), nl.head_list.cpu().numpy(), nl.nlist.cpu().numpy()
    got = [np.sort(flat[int(head[i]): int(head[i]) + int(nn_[i])]) for i in range(N)]
    mism = sum(len(set(g.tolist()) ^ set(r.tolist())) for g, r in zip(got, ref))
    assert mism <= (6 if tdt == torch.float32 else 0), mism
    # rows next to an open face hold no partner from the far side -- and some row would have had one
    ax = periodic.index(0)
    far = 0
    for i in range(N):
        across = set(full[i].tolist()) - set(ref[i].tolist())
        far += len(across)
        assert not (across & set(got[i].tolist())), i
        if len(got[i]):
            assert np.abs(p[got[i], ax] - p[i, ax]).max() <= 2.9 + 1e-5
    assert far > 0
    for g in got[:: max(1, N // 50)]:
        assert len(set(g.tolist())) == len(g)


def _dyadic_state(rng, n, dtype, dev):
    """Positions inside an 8^3 box, velocities and forces on dyadic grids: with dt = 1/32 every operation of the leapfrog step is
    exact in fp32, so x + v dt is the same number however the compiler contracts it."""
    x = rng.integers(-255, 256, (n, 3)) / 64.0
    v = rng.integers(-2048, 2049, (n, 3)) / 16.0          # up to 128: dt v reaches 4, half a box
    f = rng.integers(-64, 65, (n, 3)) / 8.0
    mk = lambda a: torch.tensor(np.concatenate([a, np.zeros((n, 1))], axis=1), dtype=dtype, device=dev)  # noqa: E731
    return x, v, f, mk


@pytest.mark.parametrize("periodic", [(1, 1, 0), (0, 1, 1)], ids=["open-z", "open-x"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("check", [False, True], ids=["nve_step", "nve_step_check"])
def test_integrator_leaves_the_open_axis_unwrapped(htf, cuda, dtype, periodic, check):
    """htfs_nve_step / htfs_nve_step_check (nve_advance, wrap1): along the open axis x(t + dt) = x + v dt bit for bit, beyond the
    face too; the other axes are wrapped into [lo, lo + L).  The plain formula in the positions' precision."""
    from test_check_step_launches import FINE, _List, _stream
    Lb, dt, n = 8.0, 1.0 / 32.0, 1500
    rng = np.random.default_rng(3 + sum(periodic) + int(check))
    x, v, f, mk = _dyadic_state(rng, n, dtype, cuda)
    pos, vel, force = mk(x), mk(v), mk(f)
    l = _List(htf, cuda, dtype, n, n, FINE, 64, pos)
    l.desc.box = htf._lib.make_box(np.array([[-4.0] * 3, [4.0] * 3, [0.0] * 3]), periodic)
    if check:
        l.scratch[2 * l.ncell: 2 * l.ncell + 2] = 0
        htf._lib.check(htf._lib.lib.htfs_nve_step_check(pos.data_ptr(), vel.data_ptr(), force.data_ptr(), l.code, n, dt, C.byref(l.desc.box),
                                                        C.byref(l.desc), l.disp.data_ptr(), _stream(htf, cuda)))
    else:
        htf._lib.check(htf._lib.lib.htfs_nve_step(pos.data_ptr(), vel.data_ptr(), force.data_ptr(), l.code, n, dt, C.byref(l.desc.box),
                                                  _stream(htf, cuda)))
    torch.cuda.synchronize()
    npdt = np.float32 if dtype == torch.float32 else np.float64
    v1 = (v.astype(npdt) + npdt(dt) * f.astype(npdt)).astype(npdt)
    x1 = (x.astype(npdt) + npdt(dt) * v1).astype(npdt)
    want = x1.copy()
    ax = periodic.index(0)
    for d in range(3):
        if d != ax:
            want[:, d] = x1[:, d] - np.floor((x1[:, d] - npdt(-4.0)) * npdt(1.0 / Lb)) * npdt(Lb)
    got = pos.cpu().numpy()
    np.testing.assert_array_equal(vel.cpu().numpy()[:, :3], v1)
    np.testing.assert_array_equal(got[:, :3], want)
    assert (np.abs(got[:, ax]) > 4.0).sum() > 50                    # rows beyond the open faces, left where they are
    others = [d for d in range(3) if d != ax]
    assert (np.abs(x1[:, others]) > 4.0).sum() > 50 and np.all(got[:, others] >= -4.0) and np.all(got[:, others] < 4.0)
    if check:   # the word it leaves: htfs_max_displacement2's on the stored positions, bit for bit (test_gpu_step_check.py)
        word = np.float32(l.disp.item())
        out = torch.zeros(1, dtype=torch.float32, device=cuda)
        htf._lib.check(htf._lib.lib.htfs_max_displacement2(pos.data_ptr(), l.ref.data_ptr(), l.code, n, C.byref(l.desc.box), out.data_ptr(),
                                                           _stream(htf, cuda)))
        assert word.tobytes() == np.float32(out.item()).tobytes() and word > 0
        assert int(l.work().abs().sum()) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("check", [False, True], ids=["max_displacement2", "nve_step_check"])
def test_displacement_along_an_open_axis_is_not_folded(htf, cuda, dtype, check):
    """row_disp2 (mimg): a row displaced by L - 0.01 along the open axis has moved (L - 0.01)^2; the same displacement along a
    periodic axis is 0.01 through the face: 1e-4.  htfs_max_displacement2 on positions set by hand, and the word htfs_nve_step_check
    leaves behind its own step -- equal bit for bit to the formula in the positions' precision."""
    from test_check_step_launches import FINE, _List, _stream
    Lb, dt, n, row = 8.0, 1.0 / 32.0, 1300, 1111          # (two blocks of 1 024 rows; the row sits in the second)
    npdt = np.float32 if dtype == torch.float32 else np.float64
    rng = np.random.default_rng(8)
    x = rng.integers(-255, 256, (n, 3)) / 64.0
    x[row] = [-3.9921875, -3.9921875, -3.9921875]
    mk = lambda a: torch.tensor(np.concatenate([a, np.zeros((n, 1))], axis=1), dtype=dtype, device=cuda)  # noqa: E731
    words = {}
    for ax, periodic in ((2, (1, 1, 0)), (0, (1, 1, 0))):     # along the open axis, then along a periodic one
        ref = mk(x)
        l = _List(htf, cuda, dtype, n, n, FINE, 64, ref)
        l.desc.box = htf._lib.make_box(np.array([[-4.0] * 3, [4.0] * 3, [0.0] * 3]), periodic)
        D = npdt(Lb - 0.01)
        if check:
            v = np.zeros((n, 3))
            v[row, ax] = float(D) / dt
            pos, vel, force = mk(x), mk(v), mk(np.zeros((n, 3)))
            l.scratch[2 * l.ncell: 2 * l.ncell + 2] = 0
            htf._lib.check(htf._lib.lib.htfs_nve_step_check(pos.data_ptr(), vel.data_ptr(), force.data_ptr(), l.code, n, dt, C.byref(l.desc.box),
                                                            C.byref(l.desc), l.disp.data_ptr(), _stream(htf, cuda)))
            torch.cuda.synchronize()
            moved = npdt(x[row, ax]) + npdt(dt) * npdt(v[row, ax])
            if periodic[ax]:
                moved = moved - np.floor((moved - npdt(-4.0)) * npdt(1.0 / Lb)) * npdt(Lb)
            assert pos.cpu().numpy()[row, ax] == moved
        else:
            xm = x.copy()
            xm[row, ax] += float(D)
            pos = mk(xm)
            l.disp.zero_()
            htf._lib.check(htf._lib.lib.htfs_max_displacement2(pos.data_ptr(), l.ref.data_ptr(), l.code, n, C.byref(l.desc.box), l.disp.data_ptr(),
                                                               _stream(htf, cuda)))
            torch.cuda.synchronize()
            moved = pos.cpu().numpy()[row, ax]
        d = npdt(moved) - npdt(x[row, ax])
        if periodic[ax]:
            d = d - npdt(Lb) * np.rint(d * npdt(1.0 / Lb))
        want = np.float32(d * d)
        words[ax] = np.float32(l.disp.item())
        assert words[ax].tobytes() == want.tobytes(), (ax, words[ax], want)
    assert abs(words[2] - (Lb - 0.01) ** 2) < 1e-4 * (Lb - 0.01) ** 2 and abs(words[0] - 1e-4) < 2e-6


@pytest.mark.parametrize("period", [4, 5])
def test_fused_step_on_a_box_with_an_open_axis(htf, cuda, period):
    """FusedStep, LJ, fp32, 4 000 rows, open along z: every group of fused_forces_rows2_kernel<LJ, STORE, 2, float, 1> falls back
    because of the box, so every row's epilogue is the rare path (group_epilogue_load with ``absent`` bits) -- positions,
    velocities and forces equal to the classic force launch + htfs_nve_step, bit for bit over 20 steps, as in
    test_fused_step_equals_force_kernel_plus_integrator."""
    from hoomd_tf_amd import standin
    periodic = (1, 1, 0)
    pos, L, a = standin.fcc_positions(10, 0.8442)
    rng = np.random.default_rng(10)
    pos = pos + 0.03 * a * rng.standard_normal(pos.shape)
    pos[:, :2] -= np.round(pos[:, :2] / L[:2]) * L[:2]
    assert np.abs(pos[:, 2]).max() < L[2] / 2 - 0.1
    out = {}
    for mode in ("classic", "fused"):
        sysm = standin.System(pos, L, dtype=torch.float32, device=cuda, periodic=periodic)
        sysm.randomize_velocities(kT=0.05, seed=4)
        nl = standin.CellNlist(sysm, r_cut=2.5, r_buff=0.4, check_period=period, device_decision=True)
        nl.build()
        ctx = htf.Context(r_cut=2.5, nneighs=80, scalar_dtype=torch.float32, max_n=sysm.N, fused=2)
        ctx.set_potential(htf.Potential.lj())
        nve = standin.NVE(sysm, 0.004)
        fs = standin.FusedStep(sysm, nl, ctx, nve)
        assert fs.available and sysm.N == 4000
        swaps = 0
        for ts in range(20):
            if mode == "fused":
                before = sysm.pos.data_ptr()
                fs.step(ts)
                swaps += int(sysm.pos.data_ptr() != before)
            else:
                nl.compute(ts)
                ctx.compute_forces(ts, fs.arrays())
                nve.step()
        torch.cuda.synchronize()
        if mode == "fused":
            assert swaps == (20 if period % 2 == 0 else 20 - 20 // period)
        out[mode] = (sysm.pos.clone(), sysm.vel.clone(), sysm.force.clone(), nl.device_builds())
    assert float(out["classic"][0][:, 2].abs().max()) < L[2] / 2          # no row left the box along z
    assert out["classic"][3] == out["fused"][3]
    for k in range(3):
        assert torch.equal(out["classic"][k], out["fused"][k]), k
    assert float(out["classic"][2][:, :3].abs().max()) > 0
