"""The step epilogue of the four-row force kernel takes its descriptor words through the scalar cache and its row sums by a
cross-lane read, behind the rows' last stores: the places where a lane could pick up another row's word, or a row's word before
it is there.  Every case runs the one-launch step (force kernel with the integrator as its epilogue) and the separate launches
(force kernel, htfs_nve_step -- under a brick htfs_brick_nve_halo) side by side for six steps, so that both arrays of the position
ping-pong are written, and compares positions, velocities, the force array and the pair-vector tensor bit for bit.

49 152 rows is where the four-row form starts (csrc/htf_internal.h fused_tails_rows).  r_cut 1.9 with r_buff 1.5 gives list rows of
~139 entries -- two full trips and a shared tail trip, as at the headline size -- of which ~18 are kept, so NN = 32 holds a row
and the tensor is 25 MB."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

R_CUT, R_BUFF, NN, PITCH = 1.9, 1.5, 32, 216
FOUR_ROWS = 49152
STEPS = 6


def _bits(t):
    return t.contiguous().view(torch.int32)


def _lattice(n_rows):
    from hoomd_tf_amd import standin
    pos, L, a = standin.fcc_positions(24, 0.8442)        # 55 296 sites; the first n_rows of them
    rng = np.random.default_rng(24)
    pos = pos + 0.03 * a * rng.standard_normal(pos.shape)
    pos -= np.round(pos / L) * L
    return pos[:n_rows].copy(), L


def crowd_a_row(pos, L, c):
    """Pull the third neighbor shell of particle ``c`` (24 sites of the crystal, 2.06 away) inward to 1.78, between the second
    shell and r_cut: 42 particles then lie within r_cut of ``c`` -- its row OVERFLOWS NN -- and no pair comes closer than ~0.9.
    -> the moved indices"""
    d = pos - pos[c]
    d -= np.round(d / L) * L
    r = np.linalg.norm(d, axis=1)
    third = np.nonzero((r > 1.95) & (r < 2.2))[0]
    assert len(third) >= 20, len(third)
    new = pos[c] + d[third] / r[third, None] * 1.78
    pos[third] = new - np.round(new / L) * L
    return [int(j) for j in third]


def _grow_row(nl, i, n_new, N):
    """Row ``i`` of the list with ``n_new`` entries: its own, then the lowest-numbered particles it does not list (none of them
    within r_list, so none within r_cut: candidates the kernel walks and drops)."""
    n, h = int(nl.n_neigh[i]), int(nl.head_list[i])
    assert n < n_new <= nl.pitch
    have = set(nl.nlist[h:h + n].tolist()) | {i}
    extra = [j for j in range(2 * n_new) if j not in have][:n_new - n]
    nl.nlist[h + n:h + n_new] = torch.as_tensor(extra, dtype=torch.int32, device=nl.nlist.device)
    nl.n_neigh[i] = n_new


def _run_both(htf, cuda, pos, L, edit=None):
    from hoomd_tf_amd import standin
    out = {}
    for mode in ("classic", "fused"):
        sysm = standin.System(pos, L, dtype=torch.float32, device=cuda)
        sysm.randomize_velocities(kT=1.0, seed=4)
        nl = standin.CellNlist(sysm, r_cut=R_CUT, r_buff=R_BUFF, pitch=PITCH, check_period=4, device_decision=False)
        nl.build()
        assert nl.pitch == PITCH and 128 < int(nl.n_neigh.max()) <= 192
        if edit is not None:
            edit(nl, sysm.N)
        ctx = htf.Context(r_cut=R_CUT, nneighs=NN, scalar_dtype=torch.float32, max_n=sysm.N, fused=2)
        ctx.set_potential(htf.Potential.lj())
        nve = standin.NVE(sysm, 0.002)
        fs = standin.FusedStep(sysm, nl, ctx, nve)
        assert fs.available
        arrays_seen = set()
        for ts in range(STEPS):                           # (the list stays: r_buff is 1.5, six steps move a particle ~0.02)
            arrays_seen.add(sysm.pos.data_ptr())
            if mode == "fused":
                fs.forces_and_integrate(ts)
            else:
                ctx.compute_forces(ts, fs.arrays())
                nve.step()
        torch.cuda.synchronize()
        assert len(arrays_seen) == (2 if mode == "fused" else 1)
        out[mode] = (sysm.pos.clone(), sysm.vel.clone(), sysm.force.clone(), ctx.nlist_buffer(sysm.N, cuda).clone(),
                     nl.n_neigh.clone())
    for k, name in enumerate(("positions", "velocities", "forces", "tensor")):
        assert torch.equal(_bits(out["classic"][k]), _bits(out["fused"][k])), name
    assert bool(torch.isfinite(out["fused"][2]).all())
    return out["fused"]


@pytest.mark.parametrize("extra_rows", [1, 3])
def test_ragged_last_group(htf, cuda, extra_rows):
    """49 152 + 1 and + 3 rows: the last wave's group has one or three rows, and no lane of the absent rows may store."""
    pos, L = _lattice(FOUR_ROWS + extra_rows)
    _run_both(htf, cuda, pos, L)


def test_row_without_neighbors_in_a_group(htf, cuda):
    """One row of a group has an empty list: the group takes the two-rows-at-a-time fallback, which hands its sums back."""
    pos, L = _lattice(FOUR_ROWS + 1)

    def edit(nl, N):
        nl.n_neigh[4 * 5000 + 1] = 0

    pos_f, vel_f, force_f, tensor_f, _ = _run_both(htf, cuda, pos, L, edit)
    assert not bool(force_f[4 * 5000 + 1].any()) and not bool(tensor_f[4 * 5000 + 1].any())
    assert bool(force_f[4 * 5000 + 2, :3].any())


def test_row_longer_than_three_trips_in_a_group(htf, cuda):
    """One row of a group lists more than 192 entries: the whole group falls back and hands its sums back."""
    pos, L = _lattice(FOUR_ROWS + 1)

    def edit(nl, N):
        _grow_row(nl, 4 * 5000 + 2, 200, N)

    _run_both(htf, cuda, pos, L, edit)


def test_tails_of_a_group_past_one_trip(htf, cuda):
    """Four rows of 150 entries: their tails together are 88 lanes (S[R] > 64), more than the shared trip holds."""
    pos, L = _lattice(FOUR_ROWS + 1)

    def edit(nl, N):
        for r in range(4):
            _grow_row(nl, 4 * 5000 + r, 150, N)

    _run_both(htf, cuda, pos, L, edit)


def test_row_that_overflows_its_slots_in_a_group(htf, cuda):
    """One row keeps more pairs than NN: it is redone by the single-row routine behind the full wait and hands its sums back,
    while the group's other rows went the straight-line way."""
    pos, L = _lattice(FOUR_ROWS + 1)
    c = 4 * 5000 + 1
    moved = crowd_a_row(pos, L, c)
    assert not (set(moved) & {c - 1, c + 1, c + 2})
    _, _, _, tensor_f, n_neigh = _run_both(htf, cuda, pos, L)
    kept = (tensor_f[:, :, :3] != 0).any(dim=2).sum(dim=1)
    assert int(kept[c]) == NN and int(n_neigh[c]) <= 192          # every slot of the row holds a pair: the wrap ran
    assert int(kept[c - 1]) < NN and int(kept[c + 1]) < NN and int(kept[c + 2]) < NN


@pytest.mark.parametrize("grid", [(8, 1, 1), (4, 2, 1)])
def test_halo_level_under_a_replica_brick(htf, cuda, monkeypatch, grid):
    """The epilogue's halo level (integrator + the pack of the next step's halo messages, each shifted by its message's vector) in
    the four-row form: the replica-mode brick the dd-self workload runs (8 x 1 x 1: two messages; 4 x 2 x 1: eight), a rank that
    is its own neighbor, 24^3 fcc cells -- the first size whose capacity passes 49 152 rows -- against force rows +
    htfs_brick_nve_halo (HTF_NO_STEP_EPILOGUE=1).  Six one-launch steps in periods of two, so that each period starts on the home
    array, with a migration + re-plan + list rebuild before the fifth; positions WITH the ghost region the messages land in,
    velocities, forces and the tensor, bit for bit (inert rows are NaN in both)."""
    import test_gpu_brick as tb
    out = {}
    for mode, env in (("classic", "1"), ("fused", "0")):
        monkeypatch.setenv("HTF_NO_STEP_EPILOGUE", env)
        sysm, nl, run = tb._replica_md(htf, cuda, grid, "local", cells=24, period=2, fused=2)
        assert sysm.N >= FOUR_ROWS and nl.domain.n_interior < nl.domain.cap
        assert run.fstep.available == (mode == "fused")
        home = sysm.pos.data_ptr()
        swaps = 0
        for ts in range(STEPS):
            if ts == 4:
                assert sysm.pos.data_ptr() == home
                nl.build()                                        # migration, re-plan, list rebuild
            before = sysm.pos.data_ptr()
            run.step()
            swaps += int(sysm.pos.data_ptr() != before)
        torch.cuda.synchronize()
        c = nl.domain.counts_host()                               # (raises on an overflow flag)
        assert swaps == (STEPS if mode == "fused" else 0) and sysm.pos.data_ptr() == home
        assert int(c[1]) > 0 and nl.domain.n_ghosts > 0           # boundary rows, and ghosts they were packed into
        out[mode] = (sysm.pos.clone(), sysm.vel.clone(), sysm.force.clone(), run.ctx.nlist_buffer(sysm.N, cuda).clone())
    assert out["fused"][0].shape[0] > nl.domain.cap
    for k, name in enumerate(("positions and ghosts", "velocities", "forces", "tensor")):
        assert tb._same(out["classic"][k], out["fused"][k]), name
