"""``iter_from_trajectory`` on the GPU: frames recorded from a live tfcompute run replayed through ``SimModel`` (forces
against an fp64 LJ restatement and against the live run), an example-05 RDF model against the oracle, and upstream's
frame selection.

Force tolerance.  The replay sees the recorded fp32 coordinates, as the restatement does.  A pair vector is formed in fp32
(difference, minimum image): absolute error <= 2 eps32 L per component, a relative error of 2 eps32 L / r in r; the LJ force
of a pair goes as r^-13, so its fp32 value is off by at most (13 * 2 L / r + 32) eps32 |f_ij| (the second term: the
arithmetic of r^-2, its powers and the products, with room).  Each atom's bound is the sum of its pairs' bounds."""
import numpy as np
import pytest
import torch

import build_examples
from helpers import min_image_np, sc_lattice
from oracle import htf_oracle as O

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
R_CUT = 2.5


def _lj_f64_and_bound(pos, L, r_cut):
    """fp64 LJ (eps = sig = 1, no shift) forces on the fp32 positions, and the per-atom bound of the module docstring."""
    d = min_image_np(pos[None, :, :].astype(np.float64) - pos[:, None, :].astype(np.float64), np.asarray(L, np.float64))
    r2 = np.sum(d * d, axis=2)
    m = (r2 <= r_cut * r_cut) & (r2 > 0)
    r2s = np.where(m, r2, 1.0)
    s6 = 1.0 / r2s ** 3
    fdr = np.where(m, (48.0 * s6 * s6 - 24.0 * s6) / r2s, 0.0)
    F = -np.sum(fdr[..., None] * d, axis=1)
    fmag = np.abs(fdr) * np.sqrt(r2s)
    bound = EPS32 * np.sum(np.where(m, fmag * (26.0 * max(L) / np.sqrt(r2s) + 32.0), 0.0), axis=1)
    return F, bound


def _record(htf, cuda, frames=20):
    """A stand-in LJ run through tfcompute: per frame the fp32 positions and the forces tfcompute produced for them."""
    from hoomd_tf_amd import standin
    pos, L = sc_lattice(6, 1.5)
    system = standin.System(pos, L, dtype=torch.float32, device=cuda)
    system.randomize_velocities(1.0, 3)
    sim = standin.Simulation(system)
    sim.integrate_nve(0.002)
    tfc = htf.tfcompute(build_examples.LJModel(32))
    tfc.attach(sim.nlist_cell(check_period=1), r_cut=R_CUT)
    sim.run(5)
    P, F = [], []
    for _ in range(frames):
        sim.run(1)
        sim.compute_forces()
        P.append(system.positions_numpy().astype(np.float32).copy())
        F.append(sim.net_force[:, :3].double().cpu().numpy().copy())
    return np.stack(P), np.stack(F), [float(v) for v in L]


def test_replayed_lj_forces_match_f64_and_live_run(htf, cuda):
    P, F_live, L = _record(htf, cuda)
    traj = htf.ArrayTrajectory(P, list(L) + [90.0] * 3, forces=F_live)
    model = build_examples.LJModel(32)
    n = 0
    for (nlist, positions, box), ts in htf.iter_from_trajectory(32, traj, r_cut=R_CUT):
        assert positions.shape == (P.shape[1], 4) and positions.dtype == torch.float32 and positions.is_cuda
        np.testing.assert_array_equal(positions[:, :3].cpu().numpy(), P[ts.frame])
        np.testing.assert_array_equal(box.cpu().numpy(), [[0, 0, 0], L, [0, 0, 0]])
        got = model([nlist, positions, box])[0][:, :3].double().cpu().numpy()
        ref, bound = _lj_f64_and_bound(P[ts.frame], L, R_CUT)
        assert np.abs(ref).max() > 0.05
        err = np.abs(got - ref)
        assert np.all(err <= bound[:, None]), (ts.frame, float((err / bound[:, None]).max()))
        live = np.abs(ts.forces.astype(np.float64) - got)
        assert np.all(live <= 2 * bound[:, None] + 2 * EPS32 * np.abs(ref)), ts.frame
        n += 1
    assert n == P.shape[0]


def test_box_centred_or_not_gives_same_forces(htf, cuda):
    P, _, L = _record(htf, cuda, frames=3)
    half = np.float32(L[0] / 2)
    model = build_examples.LJModel(32)
    outs = []
    for shift in (np.float32(0.0), half):
        Q = P.copy()
        Q = Q - np.floor(Q / np.float32(L[0])) * np.float32(L[0]) - shift        # [0, L) or [-L/2, L/2)
        traj = htf.ArrayTrajectory(Q, list(L) + [90.0] * 3)
        outs.append([model(inp)[0][:, :3].double().cpu().numpy() for inp, _ in htf.iter_from_trajectory(32, traj, r_cut=R_CUT)])
    for a, b, p in zip(outs[0], outs[1], P):
        _, bound = _lj_f64_and_bound(p, L, R_CUT)
        assert np.all(np.abs(a - b) <= 2 * bound[:, None])


def _two_type_frames(n_frames=6, seed=0):
    pos, L = sc_lattice(8, 1.4)
    rng = np.random.default_rng(seed)
    P = np.stack([pos + 0.08 * rng.standard_normal(pos.shape) * (f + 1) for f in range(n_frames)]).astype(np.float32)
    types = np.where(np.arange(pos.shape[0]) % 3 == 0, "OW", "HW")      # sorted unique: HW -> 0, OW -> 1
    return P, [float(v) for v in L], types


def test_example05_rdf_model_vs_oracle(htf, cuda):
    """Example 05: an LJ model that also averages typed RDFs in MeanTensors, over a two-type trajectory."""

    class LJRDFModel(htf.SimModel):
        def setup(self):
            self.avg_rdf = htf.MeanTensor()

        def compute(self, nlist, positions, box):
            rinv = htf.nlist_rinv(nlist)
            inv_r6 = rinv ** 6
            energy = htf.reduce_sum(4.0 / 2.0 * (inv_r6 * inv_r6 - inv_r6), axis=1)
            forces = htf.compute_nlist_forces(nlist, energy)
            rdf, r = htf.compute_rdf(nlist, [0, 3.0], positions[:, 3], nbins=40, type_i=1, type_j=0)
            self.avg_rdf.update_state(rdf)
            return forces

    P, L, types = _two_type_frames()
    NN = 64
    model = LJRDFModel(NN)
    traj = htf.ArrayTrajectory(P, list(L) + [90.0] * 3, types=types)
    refs = []
    t_idx = (types == "OW").astype(np.float32)
    for inputs, ts in htf.iter_from_trajectory(NN, traj, r_cut=3.0):
        np.testing.assert_array_equal(inputs[1][:, 3].cpu().numpy(), t_idx)
        model(inputs)
        p4 = np.concatenate([P[ts.frame], t_idx[:, None]], 1)
        nl = O.compute_nlist(p4, 3.0, NN, L, sorted=True, return_types=True)
        refs.append(O.compute_rdf(nl, [0, 3.0], t_idx, nbins=40, type_i=1, type_j=0)[0])
    ref = np.mean(refs, axis=0)
    assert ref.sum() > 0
    np.testing.assert_allclose(model.avg_rdf.result().cpu().numpy(), ref, rtol=1e-4)


def _upstream_frames(n_frames, start, end, period):
    """utils.py:740-749 with end=None meaning the last frame."""
    end = n_frames - 1 if end is None else end
    return [i for i in range(n_frames) if start <= i <= end and i % period == 0]


@pytest.mark.parametrize("start,end,period", [(0, None, 1), (0, None, 3), (2, None, 2), (3, 7, 1), (1, 8, 4), (5, 5, 1),
                                              (0.5, 6.5, 2), (9, None, 1), (20, None, 1)])
def test_frame_selection_matches_upstream(htf, cuda, start, end, period):
    P, L, _ = _two_type_frames(n_frames=10, seed=1)
    traj = htf.ArrayTrajectory(P, list(L) + [90.0] * 3)
    got = [ts.frame for _, ts in htf.iter_from_trajectory(16, traj, r_cut=2.0, period=period, start=start, end=end)]
    assert got == _upstream_frames(10, start, end, period)


def test_frames_get_new_tensors_and_new_lists(htf, cuda):
    P, L, _ = _two_type_frames(n_frames=4, seed=2)
    traj = htf.ArrayTrajectory(P, np.tile(list(L) + [90.0] * 3, (4, 1)))
    kept = [[t.clone() for t in inputs] + inputs for inputs, _ in htf.iter_from_trajectory(16, traj, r_cut=2.0)]
    assert len(kept) == 4
    for k, frame in enumerate(kept):
        for copy, live in zip(frame[:3], frame[3:]):
            assert torch.equal(copy, live)                                  # not overwritten by later frames
        np.testing.assert_array_equal(frame[1][:, :3].cpu().numpy(), P[k])
    for a, b in zip(kept, kept[1:]):
        assert not torch.equal(a[0], b[0])                                  # the list follows the frame
        assert a[0].data_ptr() != b[0].data_ptr() and a[1].data_ptr() != b[1].data_ptr()
