"""BrickDomain on the GPU: csrc/brick.hip against its torch restatement, the replica mode against the replicated single-domain
system, slabs against SlabDomain bit for bit, 2 x 2 and 5 x 1 cuts against the single-domain forces (ranks share the one GPU over
gloo)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import ROOT, check_rank_count

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _brick_of_liquid(htf, cuda, cells, grid, seed=3, steps=60, dtype=torch.float32):
    """One brick (the middle one) of a small equilibrated LJ liquid whose box is grid x the brick: a configuration that is
    periodic with the brick's period would need the liquid to be, so the brick comes from a liquid in the BRICK's own periodic
    box (cells^3 fcc cells), and the logical global box is grid x that."""
    from test_gpu_parity import _liquid
    lsys, _, L = _liquid(htf, cuda, cells=cells, steps=steps, seed=seed, dtype=dtype)
    pos = lsys.pos[:lsys.N, :3].double().cpu().numpy()
    vel = lsys.vel[:lsys.N].double().cpu().numpy()
    return pos, vel, np.asarray(L, dtype=np.float64)


def _replica_system(standin, pos, vel, Lb, grid, dev, dtype=torch.float32):
    """The brick placed at coordinate grid // 2 of the logical box grid * Lb (centred on 0)."""
    grid = np.asarray(grid)
    Lg = Lb * grid
    coords = grid // 2
    lo = -Lg / 2 + coords * Lb
    p = pos + Lb / 2 + lo            # brick-local [-Lb/2, Lb/2) -> [lo, lo + Lb)
    sysm = standin.System(p, Lg, types=np.arange(len(p)), dtype=dtype, device=dev)
    sysm.vel = torch.from_numpy(vel).to(dtype).to(dev)
    return sysm, Lg, lo


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0)) and torch.equal(torch.isnan(a), torch.isnan(b))


@pytest.mark.parametrize("grid", [(8, 1, 1), (4, 2, 1), (3, 1, 1)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_brick_kernels_match_torch(htf, cuda, grid, dtype):
    """csrc/brick.hip (destination keys, stable sorts, migration messages, class order, inert rows, halo messages, counts) ==
    the torch restatement, bit for bit, over three move-and-rebuild rounds in replica mode (particles leave through every face
    and come back through the opposite one, shifted)."""
    from hoomd_tf_amd import _lib, standin
    from hoomd_tf_amd.brick import BrickDomain
    pos, vel, Lb = _brick_of_liquid(htf, cuda, 6, grid, dtype=dtype)
    out = {}
    for backend in ("kernels", "torch"):
        sysm, Lg, lo = _replica_system(standin, pos, vel, Lb, grid, cuda, dtype)
        dom = BrickDomain(sysm, 0, grid, r_ghost=2.9, r_buff=0.4, replica=True, backend=backend,
                          transport="local" if backend == "kernels" else "torch")
        assert dom.kernels == (backend == "kernels")
        snaps = []
        for rnd in range(3):
            dom.rebuild()
            torch.cuda.synchronize()
            c = dom.counts_host()
            snaps.append((sysm.pos.clone(), sysm.vel.clone(), c.copy()))
            live = dom.live_rows()
            assert len(live) == len(pos)
            # move: a big step along the velocities (some particles cross a face), wrap into the LOGICAL global box
            x = sysm.pos[live, :3] + 0.15 * sysm.vel[live, :3]
            Lt = torch.as_tensor(Lg, dtype=dtype, device=cuda)
            x = x - torch.floor((x + Lt / 2) / Lt) * Lt
            sysm.pos[live, :3] = x
            dom.exchange()
            torch.cuda.synchronize()
            snaps.append((sysm.pos.clone(), None, None))
        out[backend] = snaps
        assert dom.n_migrated > 0
    for (pk, vk, ck), (pt, vt, ct) in zip(out["kernels"], out["torch"]):
        assert _same(pk, pt)
        if vk is not None:
            assert _same(vk, vt)
            for w in (_lib.BC_N_INT, _lib.BC_N_BND, _lib.BC_N_CAND, _lib.BC_N_ARRIVED, _lib.BC_REBUILDS):
                assert ck[w] == ct[w], w
            assert np.array_equal(ck[_lib.BC_MSG:_lib.BC_MSG + 8], ct[_lib.BC_MSG:_lib.BC_MSG + 8])
            assert np.array_equal(ck[_lib.BC_CLASS:_lib.BC_CLASS + 17], ct[_lib.BC_CLASS:_lib.BC_CLASS + 17])
            assert ck[_lib.BC_FLAGS] == ct[_lib.BC_FLAGS] == 0
            slots = slice(_lib.BC_SLOT, _lib.BC_SLOT + 16 * _lib.BRICK_MAX_MSG)   # where class c starts in message m, -1: not carried
            assert np.array_equal(ck[slots], ct[slots])


@pytest.mark.parametrize("local_grid", [True, False])
@pytest.mark.parametrize("grid,transport,replan", [((8, 1, 1), "local", 1), ((4, 2, 1), "local", 1), ((8, 1, 1), "native", 1), ((4, 2, 1), "native", 1),
                                                   ((8, 1, 1), "peer", 1), ((4, 2, 1), "peer", 1), ((8, 1, 1), "local", 2), ((4, 2, 1), "local", 2),
                                                   ((4, 2, 1), "peer", 2), ((8, 1, 1), "local", 3)])
def test_replica_brick_forces_equal_the_replicated_box(htf, cuda, grid, transport, local_grid, replan):
    """Replica mode is a physical system -- the brick repeated grid times: forces of the one rank's rows (interior rows while the
    halo is in flight, boundary rows behind it) == the single-domain forces of the replicated box, through an MD run with
    migration (particles leave through a face and re-enter through the opposite one).  ``native``: the halo and the migration
    messages travel through RCCL (this rank sending to itself), csrc/halo.hip's grouped exchange.  ``peer``: the packing kernel
    stores the rows into the receiver's inbox and signals, the unpack kernel waits for the signal -- no library in the step.
    ``replan`` = k > 1: only every k-th rebuild migrates and re-plans (BrickDomain(replan_every=k): a ghost layer (k - 1) r_buff
    thicker); the forces are compared at four different points of the plan's life."""
    from hoomd_tf_amd import _lib, standin
    from hoomd_tf_amd.brick import BrickDomain
    if transport == "native" and not _lib.lib.htf_halo_available():
        pytest.skip("librccl not loadable")
    cells = 6
    pos, vel, Lb = _brick_of_liquid(htf, cuda, cells, grid)
    rcut, rbuf, NN = 2.5, 0.4, 96
    sysm, Lg, lo = _replica_system(standin, pos, vel, Lb, grid, cuda)
    nl = standin.CellNlist(sysm, r_cut=rcut, r_buff=rbuf, check_period=1)
    dom = nl.domain = BrickDomain(sysm, 0, grid, r_ghost=rcut + rbuf, r_buff=rbuf, replica=True, transport=transport, local_grid=local_grid,
                                  replan_every=replan)
    nl.build()
    if local_grid:   # the list is binned on the brick + ghost layer alone: 1 / px / py of the logical box's cells (+ the layer)
        assert nl._grid[2] < 0.6 * np.prod(np.floor(Lg / ((rcut + rbuf) / 2.0)))
    ctx = htf.Context(r_cut=rcut, nneighs=NN, scalar_dtype=torch.float32, max_n=sysm.N)
    ctx.set_potential(htf.Potential.lj())
    nve = standin.NVE(sysm, 0.005)
    arr = ctx.make_arrays(sysm.pos, sysm.N, nl.n_neigh, nl.head_list, nl.nlist, sysm.box, sysm.force)
    overlapped = 0
    n_steps = 160
    checkpoints = (n_steps - 1,) if replan == 1 else (n_steps - 11, n_steps - 8, n_steps - 4, n_steps - 1)

    def compare():
        torch.cuda.synchronize()
        live = dom.live_rows()
        assert len(live) == len(pos)
        p = sysm.pos[live, :3].double().cpu().numpy()
        # everybody is still in the brick (a migrant shifted the wrong way -- both faces of an axis with two bricks lead to the same
        # neighbor, the shift differs -- would sit a brick width outside), give or take what moves between two rebuilds
        for d in dom.axes:
            q = p[:, d] - np.floor((p[:, d] - dom.lo[d] + 1.0) / Lg[d]) * Lg[d]      # (the integrator wraps into the logical box)
            assert np.all((q >= dom.lo[d] - 0.25 * replan) & (q < dom.hi[d] + 0.25 * replan)), d      # (r_buff / 2 per period since the plan)
        kT = float((sysm.vel[live, :3].double() ** 2).sum() / (3 * len(live)))
        assert 0.7 < kT < 1.3, kT
        got = sysm.force[live].cpu().numpy()
        assert np.all(sysm.force[~torch.isin(torch.arange(sysm.N, device=cuda), live)].cpu().numpy() == 0)   # inert rows: zero force
        # the replicated box, single domain: every brick image of every particle
        reps = np.stack(np.meshgrid(*[np.arange(g) for g in grid], indexing="ij"), -1).reshape(-1, 3)
        base = p - lo                                      # brick-local [0, Lb); rows may sit a hair outside after the last step
        allp = np.concatenate([base + r * Lb - Lg / 2 for r in reps])
        allp -= np.floor((allp + Lg / 2) / Lg) * Lg
        ref_sys = standin.System(allp, Lg, dtype=torch.float32, device=cuda)
        ref_nl = standin.CellNlist(ref_sys, r_cut=rcut, r_buff=rbuf)
        ref_nl.build()
        ref_ctx = htf.Context(r_cut=rcut, nneighs=NN, scalar_dtype=torch.float32, max_n=ref_sys.N)
        ref_ctx.set_potential(htf.Potential.lj())
        ref_ctx.compute_forces(0, ref_ctx.make_arrays(ref_sys.pos, ref_sys.N, ref_nl.n_neigh, ref_nl.head_list, ref_nl.nlist, ref_sys.box, ref_sys.force))
        torch.cuda.synchronize()
        mine = int(np.nonzero((reps == np.asarray(grid) // 2).all(axis=1))[0][0])
        want = ref_sys.force.cpu().numpy()[mine * len(p):(mine + 1) * len(p)]
        scale = np.abs(want).max()
        assert np.abs(got - want).max() < 3e-5 * scale, (np.abs(got - want).max(), scale)

    for ts in range(n_steps):
        nl.compute(ts)
        overlapped += int(dom.pending)
        ctx.compute_forces_overlapped(ts, arr, dom)
        if ts in checkpoints:
            compare()
        if ts < n_steps - 1:
            nve.step()
    torch.cuda.synchronize()
    assert nl.n_builds >= 3 and overlapped >= 30 and dom.n_migrated > 5, (nl.n_builds, overlapped, dom.n_migrated)
    assert (dom.n_light >= 2) == (replan > 1), dom.n_light


def _slab_twin_worker(rank, world, port, q, per_slab):
    """The same decomposed LJ MD twice -- SlabDomain (variable-length arrays, host-planned rebuild) and BrickDomain(world, 1, 1)
    (fixed capacity, inert rows, rebuild without a read-back) -- with the host-decided distance check: rebuilt at the same steps,
    and every particle ends at bit-identical coordinates."""
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        sys.path.insert(0, ROOT)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import hoomd_tf_amd as htf
        from hoomd_tf_amd import standin
        from hoomd_tf_amd.brick import BrickDomain
        from hoomd_tf_amd.domain import SlabDomain

        dev = torch.device("cuda:0")
        rcut, rbuf, NN = 2.5, 0.4, 80
        cells = (per_slab * world, 5, 5)
        a = (4.0 / 0.8442) ** (1.0 / 3.0)
        base = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
        grid = np.stack(np.meshgrid(*[np.arange(c) for c in cells], indexing="ij"), -1).reshape(-1, 3)
        pos0 = ((grid[:, None, :] + base[None]) * a).reshape(-1, 3)
        L = np.array(cells, dtype=np.float64) * a
        pos0 = pos0 - L / 2
        rng = np.random.default_rng(11)
        pos0 += 0.04 * a * rng.standard_normal(pos0.shape)
        pos0 -= np.round(pos0 / L) * L
        Ng = len(pos0)
        vel0 = np.zeros((Ng, 4))
        vel0[:, :3] = 1.0 * rng.standard_normal((Ng, 3))
        vel0[:, 3] = 1.0
        bounds = -L[0] / 2 + np.linspace(0, 1, world + 1) * L[0]
        mine = (pos0[:, 0] >= bounds[rank]) & (pos0[:, 0] < bounds[rank + 1])
        out = {}
        for kind in ("slab", "brick"):
            sysm = standin.System(pos0[mine], L, types=np.arange(Ng)[mine], dtype=torch.float32, device=dev)
            sysm.vel = torch.from_numpy(vel0[mine]).to(torch.float32).to(dev)
            nl = standin.CellNlist(sysm, r_cut=rcut, r_buff=rbuf, check_period=2)
            if kind == "slab":
                nl.domain = SlabDomain(sysm, rank, world, r_ghost=rcut + rbuf)
            else:
                # (ghosts at their owner's coordinates, the list binned on the global box's grid: SlabDomain's conventions, hence
                #  its neighbor order; the default -- a cell grid local to the brick -- gives the same forces in another order)
                nl.domain = BrickDomain(sysm, rank, (world, 1, 1), r_ghost=rcut + rbuf, r_buff=rbuf, local_grid=False)
                assert nl.domain.kernels
            nl.build()
            ctx = htf.Context(r_cut=rcut, nneighs=NN, scalar_dtype=torch.float32, max_n=sysm.N)
            ctx.set_potential(htf.Potential.lj())
            nve = standin.NVE(sysm, 0.004)
            builds, arr, steps_built = -1, None, []
            for ts in range(90):
                nl.compute(ts)
                if nl.n_builds != builds:
                    arr = ctx.make_arrays(sysm.pos, sysm.N, nl.n_neigh, nl.head_list, nl.nlist, sysm.box, sysm.force)
                    builds = nl.n_builds
                    steps_built.append(ts)
                ctx.compute_forces_overlapped(ts, arr, nl.domain)
                nve.step()
            torch.cuda.synchronize()
            assert len(steps_built) >= 4, steps_built
            if kind == "slab":
                ids, p, v, f = sysm.types_numpy(), sysm.pos[:sysm.N], sysm.vel, sysm.force[:sysm.N]
            else:
                live = nl.domain.live_rows()
                ids = sysm.pos[live, 3].contiguous().view(torch.int32).cpu().numpy()
                p, v, f = sysm.pos[live], sysm.vel[live], sysm.force[live]
                assert nl.domain.n_migrated > 0
            out[kind] = (steps_built, ids.copy(), p.cpu().numpy().copy(), v.cpu().numpy().copy(), f.cpu().numpy().copy())
        assert out["slab"][0] == out["brick"][0], (out["slab"][0], out["brick"][0])
        for k in range(1, 5):
            np.testing.assert_array_equal(out["slab"][k], out["brick"][k])
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


def _run_ranks(target, world, args, timeout=900):
    """The ranks SHARE this GPU: up to five processes are time-sliced on it beside this one (helpers.MAX_RANKS), each with
    spinning wait kernels of the library-free transport in flight, and on a cold box their start-up is seconds apart.  Every wait
    is bounded -- ~4 s of polling on the device (HTF_PEER_SPIN), 30 s on the host for a replayed cycle (HTF_BRICK_WAIT_S) -- so a
    rehearsal gets 30 s / 120 s.  One attempt: a wait that runs out fails the test."""
    check_rank_count(world)
    saved = {k: os.environ.get(k) for k in ("HTF_PEER_SPIN", "HTF_BRICK_WAIT_S")}
    for k, v in (("HTF_PEER_SPIN", str(1 << 25)), ("HTF_BRICK_WAIT_S", "120")):
        if saved[k] is None:
            os.environ[k] = v
    try:
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        port = _free_port()
        procs = [ctx.Process(target=target, args=(r, world, port, q) + tuple(args)) for r in range(world)]
        for p in procs:
            p.start()
        results = [q.get(timeout=timeout) for _ in procs]
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
        for res in results:
            assert res[1] == "ok", "rank %d failed:\n%s" % (res[0], res[1])
        return results
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)


@pytest.mark.parametrize("world,per_slab", [(3, 4), (5, 2)])
def test_brick_slabs_equal_slab_domain_bit_for_bit(htf, cuda, world, per_slab):
    """fixed-capacity arrays with inert rows and device-resident counts change nothing a particle sees --
    trajectories bit-identical to SlabDomain's at world 3 and at world 5 (slabs thinner than 2 r_ghost, so a rank's ghosts come
    from both neighbors on each side, four distinct ranks)."""
    _run_ranks(_slab_twin_worker, world, (per_slab,))


def _brick_md_worker(rank, world, port, q, grid, cells, transport="torch", replan_every=1):
    """80 steps of LJ MD under a px x py cut (migration across both axes and the periodic edges, the halo overlapped with the
    interior rows), then every rank's forces against the single-domain forces of the gathered configuration."""
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        sys.path.insert(0, ROOT)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import hoomd_tf_amd as htf
        from hoomd_tf_amd import _lib, standin
        from hoomd_tf_amd.brick import BrickDomain

        dev = torch.device("cuda:0")
        rcut, rbuf, NN = 2.5, 0.4, 80
        a = (4.0 / 0.8442) ** (1.0 / 3.0)
        base = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
        gridc = np.stack(np.meshgrid(*[np.arange(c) for c in cells], indexing="ij"), -1).reshape(-1, 3)
        pos = ((gridc[:, None, :] + base[None]) * a).reshape(-1, 3)
        L = np.array(cells, dtype=np.float64) * a
        pos = pos - L / 2
        rng = np.random.default_rng(5)
        pos += 0.05 * a * rng.standard_normal(pos.shape)
        pos -= np.round(pos / L) * L
        Ng = len(pos)
        vel = np.zeros((Ng, 4))
        vel[:, :3] = 1.5 * rng.standard_normal((Ng, 3))
        vel[:, 3] = 1.0
        probe = BrickDomain(standin.System(pos[:1], L, dtype=torch.float32, device=dev), rank, grid, r_ghost=rcut + rbuf, n_global=Ng)
        mine = np.ones(Ng, dtype=bool)
        for d in probe.axes:
            mine &= (pos[:, d] >= probe.lo[d]) & (pos[:, d] < probe.hi[d])
        sysm = standin.System(pos[mine], L, types=np.arange(Ng)[mine], dtype=torch.float32, device=dev)
        sysm.vel = torch.from_numpy(vel[mine]).to(torch.float32).to(dev)
        nl = standin.CellNlist(sysm, r_cut=rcut, r_buff=rbuf, check_period=1)
        dom = nl.domain = BrickDomain(sysm, rank, grid, r_ghost=rcut + rbuf, r_buff=rbuf, n_global=Ng, transport=transport,
                                      replan_every=replan_every)
        nl.build()
        ctx = htf.Context(r_cut=rcut, nneighs=NN, scalar_dtype=torch.float32, max_n=sysm.N)
        pot = htf.Potential.lj()
        ctx.set_potential(pot)
        nve = standin.NVE(sysm, 0.004)
        arr = ctx.make_arrays(sysm.pos, sysm.N, nl.n_neigh, nl.head_list, nl.nlist, sysm.box, sysm.force)
        overlapped = 0
        for ts in range(80):
            nl.compute(ts)
            overlapped += int(dom.pending)
            ctx.compute_forces_overlapped(ts, arr, dom)
            if ts < 79:
                nve.step()
        torch.cuda.synchronize()
        assert nl.n_builds >= 2 and overlapped >= 20, (nl.n_builds, overlapped)
        assert (dom.n_light > 0) == (replan_every > 1), dom.n_light
        c = dom.counts_host()
        assert int(c[_lib.BC_N_INT]) > 0                         # bricks wider than 2 r_ghost keep interior rows
        live = dom.live_rows()
        my_ids = sysm.pos[live, 3].contiguous().view(torch.int32).cpu().numpy()
        loc = torch.zeros((Ng, 3), dtype=torch.float64)
        loc[my_ids] = sysm.pos[live, :3].double().cpu()
        owned = torch.zeros(Ng, dtype=torch.float64)
        owned[my_ids] = 1
        dist.all_reduce(loc)
        dist.all_reduce(owned)
        assert bool((owned == 1).all()), "particles lost or duplicated"
        ref_sys = standin.System(loc.numpy(), L, dtype=torch.float32, device=dev)
        ref_nl = standin.CellNlist(ref_sys, r_cut=rcut, r_buff=rbuf)
        ref_nl.build()
        ref_ctx = htf.Context(r_cut=rcut, nneighs=NN, scalar_dtype=torch.float32, max_n=Ng)
        ref_ctx.set_potential(pot)
        ref_ctx.compute_forces(0, ref_ctx.make_arrays(ref_sys.pos, Ng, ref_nl.n_neigh, ref_nl.head_list, ref_nl.nlist, ref_sys.box, ref_sys.force))
        torch.cuda.synchronize()
        want = ref_sys.force.cpu().numpy()[my_ids]
        got = sysm.force[live].cpu().numpy()
        scale = np.abs(want).max()
        assert np.abs(got - want).max() < 2e-5 * scale, (np.abs(got - want).max(), scale)
        moved = torch.tensor([dom.n_migrated])
        dist.all_reduce(moved)
        assert int(moved) > 0, "test must exercise migration"
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("grid,cells", [((2, 2, 1), (8, 8, 5)), ((3, 1, 1), (12, 5, 5))])
def test_bricks_with_the_peer_transport(htf, cuda, grid, cells):
    """Transport "peer" between PROCESSES (the ranks share the one GPU; each maps its neighbors' inboxes through CUDA-IPC): the
    packing kernel of rank A stores into rank B's inbox and signals, B's unpack kernel waits on the device -- 80 MD steps with
    migration, forces == single-domain.  What an xGMI peer mapping would carry between two devices."""
    _run_ranks(_brick_md_worker, grid[0] * grid[1], (grid, cells, "peer"))


@pytest.mark.parametrize("grid,cells", [((5, 1, 1), (20, 5, 5)), ((2, 2, 1), (8, 8, 5)), ((3, 1, 1), (12, 5, 5))])
def test_bricks_on_one_gpu(htf, cuda, grid, cells):
    """5 ranks as 5 x 1 and 4 as 2 x 2 (bricks 6.7 sigma wide against r_ghost 2.9: interior rows), 80 MD steps,
    forces == single-domain (test_mpi_tensorflow.py:57-79, ``comm.decomposition``).  The 4 x 2 cut of eight ranks would need more
    processes on the one GPU than it may hold (helpers.MAX_RANKS); replica mode runs it
    (test_replica_brick_forces_equal_the_replicated_box)."""
    _run_ranks(_brick_md_worker, grid[0] * grid[1], (grid, cells))


@pytest.mark.parametrize("grid,cells,transport", [((2, 2, 1), (10, 10, 5), "torch"), ((3, 1, 1), (12, 5, 5), "peer")])
def test_bricks_with_fewer_replans(htf, cuda, grid, cells, transport):
    """BrickDomain(replan_every=2) between PROCESSES sharing the GPU (kernels backend, the list on the local grid): every other
    rebuild leaves rows and messages as they are -- rows that have left their brick, ghosts of rows that have left theirs, wrapped
    through the periodic boundary or not -- and the forces after 80 MD steps still equal the single-domain ones."""
    _run_ranks(_brick_md_worker, grid[0] * grid[1], (grid, cells, transport, 2))


def _peer_replay_worker(rank, world, port, q, grid, cells, replan_every, die_at=None):
    """Real ranks (processes sharing the one GPU), transport "peer" and NOTHING else: the halo through the neighbors' inboxes, a
    re-plan's migration messages through their mailboxes, the distance check's all-reduce through the ranks' tables (round 6) --
    the eager no-read-back loop and the replay of whole check periods from hipGraphs give the same trajectory bit for bit, and the
    forces at the end equal the single-domain ones.  ``die_at``: (rank, step) -- that rank exits there; the others must come back
    with a RuntimeError that names the missing neighbor within seconds, not hang."""
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        sys.path.insert(0, ROOT)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import time
        import hoomd_tf_amd as htf
        from hoomd_tf_amd import standin
        from hoomd_tf_amd.brick import BrickDomain

        dev = torch.device("cuda:0")
        rcut, rbuf, NN, P = 2.5, 0.4, 80, 4
        a = (4.0 / 0.8442) ** (1.0 / 3.0)
        base = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
        gridc = np.stack(np.meshgrid(*[np.arange(c) for c in cells], indexing="ij"), -1).reshape(-1, 3)
        pos = ((gridc[:, None, :] + base[None]) * a).reshape(-1, 3)
        L = np.array(cells, dtype=np.float64) * a
        pos = pos - L / 2
        rng = np.random.default_rng(5)
        pos += 0.05 * a * rng.standard_normal(pos.shape)
        pos -= np.round(pos / L) * L
        Ng = len(pos)
        vel = np.zeros((Ng, 4))
        vel[:, :3] = 1.5 * rng.standard_normal((Ng, 3))
        vel[:, 3] = 1.0
        probe = BrickDomain(standin.System(pos[:1], L, dtype=torch.float32, device=dev), rank, grid, r_ghost=rcut + rbuf, n_global=Ng,
                            replan_every=replan_every)
        mine = np.ones(Ng, dtype=bool)
        for d in probe.axes:
            mine &= (pos[:, d] >= probe.lo[d]) & (pos[:, d] < probe.hi[d])
        out = {}
        for mode in (("eager",) if die_at else ("eager", "graph")):
            sysm = standin.System(pos[mine], L, types=np.arange(Ng)[mine], dtype=torch.float32, device=dev)
            sysm.vel = torch.from_numpy(vel[mine]).to(torch.float32).to(dev)
            nl = standin.CellNlist(sysm, r_cut=rcut, r_buff=rbuf, check_period=P, device_decision=True)
            dom = nl.domain = BrickDomain(sysm, rank, grid, r_ghost=rcut + rbuf, r_buff=rbuf, n_global=Ng, transport="peer",
                                          replan_every=replan_every)
            assert "fine-grained" in dom.peer_memory, dom.peer_memory
            nl.build()
            ctx = htf.Context(r_cut=rcut, nneighs=NN, scalar_dtype=torch.float32, max_n=sysm.N)
            pot = htf.Potential.lj()
            ctx.set_potential(pot)
            run = standin.BrickRun(sysm, nl, ctx, standin.NVE(sysm, 0.004))
            if die_at:
                t0 = None
                try:
                    for ts in range(400):
                        if (rank, ts) == tuple(die_at):
                            torch.cuda.synchronize()
                            q.put((rank, "died"))
                            q.close()
                            q.join_thread()         # (the report must leave this process before it does)
                            os._exit(0)
                        if ts == die_at[1]:
                            t0 = time.monotonic()
                        run.step()
                    torch.cuda.synchronize()
                    dom.counts_host()
                    q.put((rank, "no error after the neighbor died"))
                except RuntimeError as e:
                    took = time.monotonic() - t0
                    ok = "did not arrive" in str(e) and took < 10.0
                    q.put((rank, "ok" if ok else "raised %r after %.1f s" % (str(e), took)))
                return
            run.run(10 * P)                    # through a few rebuilds
            assert nl.n_builds >= 2 and sysm.timestep % P == 0
            nl.build()                         # both modes start a fresh reference here
            run._arr = run._arrays()
            b0 = nl.n_builds
            run.run(40 * P, graph=(mode == "graph"))
            torch.cuda.synchronize()
            assert nl.n_builds - b0 >= 4 and run.dangerous_builds <= 1, (nl.n_builds - b0, run.dangerous_builds)
            dom.counts_host()
            dom.exchange_end()
            dom.exchange()
            ctx.compute_forces(sysm.timestep, run._arrays())
            torch.cuda.synchronize()
            out[mode] = (sysm.pos[:dom.cap].clone(), sysm.vel.clone(), sysm.force.clone(), dom.n_migrated, dom.n_light, nl.n_builds)
            if mode == "graph":
                # forces against the single-domain forces of the gathered configuration
                live = dom.live_rows()
                my_ids = sysm.pos[live, 3].contiguous().view(torch.int32).cpu().numpy()
                loc = torch.zeros((Ng, 3), dtype=torch.float64)
                loc[my_ids] = sysm.pos[live, :3].double().cpu()
                owned = torch.zeros(Ng, dtype=torch.float64)
                owned[my_ids] = 1
                dist.all_reduce(loc)
                dist.all_reduce(owned)
                assert bool((owned == 1).all()), "particles lost or duplicated"
                ref_sys = standin.System(loc.numpy(), L, dtype=torch.float32, device=dev)
                ref_nl = standin.CellNlist(ref_sys, r_cut=rcut, r_buff=rbuf)
                ref_nl.build()
                ref_ctx = htf.Context(r_cut=rcut, nneighs=NN, scalar_dtype=torch.float32, max_n=Ng)
                ref_ctx.set_potential(pot)
                ref_ctx.compute_forces(0, ref_ctx.make_arrays(ref_sys.pos, Ng, ref_nl.n_neigh, ref_nl.head_list, ref_nl.nlist, ref_sys.box, ref_sys.force))
                torch.cuda.synchronize()
                want = ref_sys.force.cpu().numpy()[my_ids]
                got = sysm.force[live].cpu().numpy()
                scale = np.abs(want).max()
                assert np.abs(got - want).max() < 3e-5 * scale, (np.abs(got - want).max(), scale)
            del run, ctx, nl, dom, sysm
            dist.barrier()
        for k in range(3):
            assert _same(out["eager"][k], out["graph"][k]), k
        assert out["eager"][3:] == out["graph"][3:] and out["graph"][3] > 0, (out["eager"][3:], out["graph"][3:])
        assert (out["graph"][4] > 0) == (replan_every > 1)
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))


@pytest.mark.parametrize("grid,cells,replan", [((3, 1, 1), (12, 5, 5), 1), ((2, 2, 1), (10, 10, 5), 2), ((5, 1, 1), (20, 5, 5), 2)])
def test_replayed_cycles_between_processes_with_the_peer_transport(htf, cuda, grid, cells, replan):
    """a decomposed run between real ranks with NO communication library -- halo, migration messages and the
    all-reduced distance check are stores into the neighbors' fine-grained memory -- eager and replayed from hipGraphs (three per
    rank with replan_every = 2), bit-identical, forces == single-domain.  3 slabs, 2 x 2, and 5 slabs (helpers.MAX_RANKS)."""
    _run_ranks(_peer_replay_worker, grid[0] * grid[1], (grid, cells, replan))


def test_a_rank_that_dies_is_noticed_by_every_other_rank(htf, cuda):
    """a neighbor that stops stepping used to leave the others in a collective until somebody killed them.
    With transport "peer" every wait is a bounded spin on the device: the dead rank's NEIGHBORS miss its halo message, EVERY rank
    misses its word in the next distance check's all-reduce -- each sets the flag and raises at its next rebuild, seconds later."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    env_before = os.environ.get("HTF_PEER_SPIN")
    os.environ["HTF_PEER_SPIN"] = "40000"          # ~0.1 s of polling per missing message (children inherit it)
    try:
        check_rank_count(4)
        procs = [ctx.Process(target=_peer_replay_worker, args=(r, 4, port, q, (4, 1, 1), (16, 5, 5), 1, (1, 30))) for r in range(4)]
        for p in procs:
            p.start()
        results = dict(q.get(timeout=120) for _ in procs)
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    finally:
        if env_before is None:
            os.environ.pop("HTF_PEER_SPIN", None)
        else:
            os.environ["HTF_PEER_SPIN"] = env_before
    assert results[1] == "died"
    for r in (0, 2, 3):                            # rank 3 is NOT a neighbor of rank 1: it learns through the all-reduce
        assert results[r] == "ok", (r, results[r])


def _replica_md(htf, cuda, grid, transport, cells=6, period=4, replan_every=1, fused=0):
    from hoomd_tf_amd import standin
    from hoomd_tf_amd.brick import BrickDomain
    pos, vel, Lb = _brick_of_liquid(htf, cuda, cells, grid)
    rcut, rbuf, NN = 2.5, 0.4, 96
    sysm, Lg, lo = _replica_system(standin, pos, vel, Lb, grid, cuda)
    nl = standin.CellNlist(sysm, r_cut=rcut, r_buff=rbuf, check_period=period, device_decision=True)
    nl.domain = BrickDomain(sysm, 0, grid, r_ghost=rcut + rbuf, r_buff=rbuf, replica=True, transport=transport, replan_every=replan_every)
    nl.build()
    ctx = htf.Context(r_cut=rcut, nneighs=NN, scalar_dtype=torch.float32, max_n=sysm.N, fused=fused)
    ctx.set_potential(htf.Potential.lj())
    run = standin.BrickRun(sysm, nl, ctx, standin.NVE(sysm, 0.005))
    return sysm, nl, run


@pytest.mark.parametrize("grid,transport,replan", [((8, 1, 1), "local", 1), ((4, 2, 1), "native", 1), ((8, 1, 1), "native", 1), ((4, 2, 1), "local", 1),
                                                   ((8, 1, 1), "peer", 1), ((4, 2, 1), "peer", 1), ((8, 1, 1), "local", 2), ((4, 2, 1), "peer", 2),
                                                   ((4, 2, 1), "native", 2)])
def test_replayed_cycles_equal_the_eager_loop(htf, cuda, grid, transport, replan):
    """whole check periods of the decomposed step -- distance check, halo, interior rows, boundary rows,
    integrator, and in the second graph migration + re-plan + list rebuild -- replayed from hipGraphs (with ``native`` the
    grouped ncclSend / ncclRecv of csrc/halo.hip are INSIDE the capture), the next graph chosen from the pinned word of the
    cycle before: the trajectory of the eager no-read-back loop, bit for bit, rebuilt at the same steps.  ``replan`` = 2: a third
    graph -- the list rebuilt on the rows and messages as the last plan left them -- alternates with the full rebuild, as the
    eager loop alternates them.  (In a child process with a time limit: a transport that hung inside a replay would otherwise
    hold the whole session.)"""
    import subprocess
    from hoomd_tf_amd import _lib
    if transport == "native" and not _lib.lib.htf_halo_available():
        pytest.skip("librccl not loadable")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import torch, hoomd_tf_amd as htf, test_gpu_brick as t; "
            "t._replay_body(htf, torch.device('cuda:0'), %r, %r, %r); print('REPLAY OK')" % (ROOT, os.path.join(ROOT, "tests"), grid, transport, replan))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                       env=dict(os.environ, HTF_BRICK_WAIT_S="20"))
    assert r.returncode == 0 and "REPLAY OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def _replay_body(htf, cuda, grid, transport, replan=1):
    P, warm, cycles = 4, 40, 60
    out = {}
    for mode in ("eager", "graph"):
        sysm, nl, run = _replica_md(htf, cuda, grid, transport, period=P, replan_every=replan)
        run.run(warm)                      # through a few rebuilds: RCCL connected, pinned buffers made
        assert nl.n_builds >= 2 and sysm.timestep % P == 0
        nl.build()                         # both modes start a fresh reference here, with an empty decision history
        run._arr = run._arrays()
        b0 = nl.n_builds
        if mode == "eager":
            built = []
            for _ in range(cycles * P):
                b = nl.n_builds
                run.step()
                if nl.n_builds != b:
                    built.append(sysm.timestep - 1)
        else:
            run.run(cycles * P, graph=True)
            built = list(run._rebuilt_at)
            assert run.n_cycles == cycles
        torch.cuda.synchronize()
        assert nl.n_builds - b0 >= 4 and run.dangerous_builds == 0, (nl.n_builds - b0, run.dangerous_builds)
        nl.domain.counts_host()            # (raises on an overflow flag)
        out[mode] = (built, sysm.pos.clone(), sysm.vel.clone(), sysm.force.clone(), nl.domain.n_migrated, nl.domain.n_light)
    assert out["eager"][0] == out["graph"][0], (out["eager"][0], out["graph"][0])
    assert out["eager"][5] == out["graph"][5] and (out["graph"][5] >= 2) == (replan > 1), (out["eager"][5], out["graph"][5])
    for k in (1, 2, 3):
        assert _same(out["eager"][k], out["graph"][k]), k
    assert out["eager"][4] == out["graph"][4] > 0


def test_replay_counts_cycles_past_2_to_the_24(htf, cuda):
    """the replayed cycle's counter was a float32 and stopped at 16 777 216 cycles -- ten minutes of a production run --
    after which every run(graph=True) raised 'the device never reached cycle'.  It is an unsigned word now, compared modulo 2^32:
    seeded just below 2^24 and just below 2^32, the replay keeps going and keeps deciding rebuilds."""
    sysm, nl, run = _replica_md(htf, cuda, (8, 1, 1), "local", period=4)
    run.run(40)
    run.run(8 * 4, graph=True)
    torch.cuda.synchronize()
    for seed in ((1 << 24) - 3, (1 << 32) - 3):
        # what the device and the host both believe: ``seed`` cycles done
        torch.cuda.synchronize()
        word = seed if seed < (1 << 31) else seed - (1 << 32)
        run._stat.view(torch.int32)[1] = word
        run._stat_host_words[1] = word
        run._launched = run._read = seed
        run._discard.clear()
        b0 = run.n_rebuild_cycles
        run.run(30 * 4, graph=True)
        torch.cuda.synchronize()
        assert run._launched == seed + 30 and run.n_rebuild_cycles - b0 >= 2
        assert (int(run._stat_host_words[1]) & 0xFFFFFFFF) == (seed + 30) & 0xFFFFFFFF
        assert len(run._discard) <= 2
    nl.domain.counts_host()


@pytest.mark.parametrize("grid,transport,replan", [((8, 1, 1), "local", 1), ((4, 2, 1), "local", 2), ((8, 1, 1), "native", 2), ((4, 2, 1), "native", 1)])
def test_fused_step_under_a_brick_equals_the_three_pieces(htf, cuda, grid, transport, replan):
    """Round 6: under a BrickDomain the force kernel's epilogue is the integrator AND the pack of the next step's halo messages --
    straight into the other array's ghost region (a rank that is its own neighbor) or into the send buffer (a transport) -- where
    the step was force rows + htfs_brick_nve_halo.  Same trajectory bit for bit, eager and replayed, through re-plans and list-only
    rebuilds (HTF_NO_STEP_EPILOGUE=1 selects the three pieces)."""
    import subprocess
    from hoomd_tf_amd import _lib
    if transport == "native" and not _lib.lib.htf_halo_available():
        pytest.skip("librccl not loadable")
    outs = {}
    for env_v in ("0", "1"):
        code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import torch, hoomd_tf_amd as htf, test_gpu_brick as t; "
                "t._fused_brick_body(htf, torch.device('cuda:0'), %r, %r, %r)" % (ROOT, os.path.join(ROOT, "tests"), grid, transport, replan))
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                           env=dict(os.environ, HTF_BRICK_WAIT_S="20", HTF_NO_STEP_EPILOGUE=env_v))
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST ")]
        assert r.returncode == 0 and lines, r.stdout[-1500:] + r.stderr[-3000:]
        outs[env_v] = lines[-1]
    assert "fused=True" in outs["0"] and "fused=False" in outs["1"]
    assert outs["0"].split("fused=")[0] == outs["1"].split("fused=")[0], (outs["0"], outs["1"])


def _fused_brick_body(htf, cuda, grid, transport, replan):
    import hashlib
    P = 5                                  # an odd period: four fused steps and a classic one per cycle
    digest = hashlib.sha256()
    fused = None
    for mode in ("eager", "graph"):
        sysm, nl, run = _replica_md(htf, cuda, grid, transport, period=P, replan_every=replan, fused=2)
        run.run(8 * P)
        nl.build()
        b0 = nl.n_builds
        run.run(40 * P, graph=(mode == "graph"))
        torch.cuda.synchronize()
        assert nl.n_builds - b0 >= 4
        nl.domain.counts_host()
        fused = run.fstep.available
        for t in (sysm.pos[:nl.domain.cap], sysm.vel, sysm.force):
            digest.update(torch.nan_to_num(t, nan=-7.0).cpu().numpy().tobytes())
        digest.update(repr((nl.n_builds, nl.domain.n_migrated, nl.domain.n_light)).encode())
    print("DIGEST %s fused=%s" % (digest.hexdigest(), fused))


@pytest.mark.parametrize("grid", [(8, 1, 1), (4, 2, 1)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_integrate_and_pack_in_one_launch(htf, cuda, grid, dtype):
    """htfs_brick_nve_halo == htfs_nve_step followed by htfs_brick_pack_halo: positions, velocities, the packed messages and the
    directly delivered ghosts, bit for bit (every boundary row finds its slot in every message that carries it)."""
    from hoomd_tf_amd import standin
    from hoomd_tf_amd.brick import BrickDomain
    pos, vel, Lb = _brick_of_liquid(htf, cuda, 6, grid, dtype=dtype)
    res = {}
    for transport in ("local", "native", "peer"):
        for fused in (False, True):
            sysm, Lg, lo = _replica_system(standin, pos, vel, Lb, grid, cuda, dtype)
            try:
                dom = BrickDomain(sysm, 0, grid, r_ghost=2.9, r_buff=0.4, replica=True, transport=transport)
            except Exception:  # noqa: BLE001 -- no librccl
                continue
            dom.rebuild()
            sysm.force[:, :3] = torch.randn((sysm.N, 3), generator=torch.Generator(device="cuda").manual_seed(1), device=cuda, dtype=dtype)
            sysm.force[torch.isnan(sysm.pos[:sysm.N, 0])] = 0
            nve = standin.NVE(sysm, 0.005)
            for _ in range(3):
                if fused:
                    dom.nve_step(0.005)
                else:
                    nve.step()
                dom.exchange()
            torch.cuda.synchronize()
            dom.counts_host()     # (raises on a halo timeout)
            res[(transport, fused)] = (sysm.pos.clone(), sysm.vel.clone(), dom.halo_send.clone() if transport == "native" else None)
    for transport in ("local", "native", "peer"):
        if (transport, True) not in res:
            continue
        a, b = res[(transport, False)], res[(transport, True)]
        assert _same(a[0], b[0]) and _same(a[1], b[1])
        if a[2] is not None and transport == "native":
            assert _same(a[2], b[2])
    for transport in ("native", "peer"):     # every transport delivers the same ghosts
        if (transport, True) in res:
            assert _same(res[(transport, True)][0], res[("local", True)][0])


@pytest.mark.parametrize("dt", [torch.float32, torch.float64])
def test_check_displacement_in_one_launch(dt):
    """htfs_check_displacement2 (the replayed cycle's check: accumulate, publish, reset in ONE launch) against
    htfs_max_displacement2 on the same rows, inert rows included, over consecutive calls that share the two work words."""
    import ctypes as C
    from hoomd_tf_amd import _lib
    from hoomd_tf_amd.ops import raw_stream
    DEV = torch.device("cuda:0")
    torch.manual_seed(5)
    N = 40000          # 40 workgroups: the last one to finish publishes
    L = 20.0
    box = _lib.make_box(np.array([[-L / 2] * 3, [L / 2] * 3, [0.0] * 3]), (1, 1, 1))
    ref = torch.zeros((N, 4), dtype=dt, device=DEV)
    ref[:, :3] = (torch.rand((N, 3), dtype=torch.float64, device=DEV) * L - L / 2).to(dt)
    work = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.zeros(2, dtype=torch.float32, device=DEV)
    # the cycle number is an unsigned word in the second slot's BITS (a float value stopped counting at 2^24: ADVICE r5) -- seeded
    # just below 2^24 here, and in a second pass just below 2^32 (it wraps; the host compares modulo 2^32)
    seed = (1 << 24) - 2
    out.view(torch.int32)[1] = seed
    code = _lib.HTF_F32 if dt == torch.float32 else _lib.HTF_F64
    stream = C.c_void_p(raw_stream(0))
    h_out = torch.zeros(2, dtype=torch.float32).pin_memory()
    status = torch.zeros(1000, dtype=torch.int32, device=DEV)
    h_status = torch.full((302,), -1, dtype=torch.int32).pin_memory()
    mirror = _lib.Mirror()
    mirror.src[0], mirror.dst[0], mirror.words[0] = status.data_ptr(), h_status.data_ptr(), 300
    mirror.src[1], mirror.dst[1], mirror.words[1] = status.data_ptr() + 4 * 777, h_status.data_ptr() + 4 * 300, 1
    mirror.n = 2
    for cycle in range(1, 5):
        pos = ref.clone()
        pos[:, :3] += (0.05 * cycle * torch.randn((N, 3), dtype=torch.float64, device=DEV)).to(dt)
        pos[:, :3] -= L * torch.round(pos[:, :3] / L)          # wrapped: the check takes the minimum image
        pos[7::97, 0] = float("nan")                            # inert rows have not moved
        one = torch.zeros(1, dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib.htfs_max_displacement2(pos.data_ptr(), ref.data_ptr(), code, N, C.byref(box), one.data_ptr(), stream))
        status.random_(0, 1 << 30)
        _lib.check(_lib.lib.htfs_check_displacement2(pos.data_ptr(), ref.data_ptr(), code, N, C.byref(box), work.data_ptr(),
                                                     out.data_ptr(), h_out.data_ptr() if cycle % 2 else None,
                                                     C.byref(mirror) if cycle > 1 else None, stream))
        torch.cuda.synchronize()
        assert out[0].item() == one.item() and out[0].item() > 0
        assert (int(out.view(torch.int32)[1].item()) & 0xFFFFFFFF) == seed + cycle       # 2^24 - 1, 2^24, 2^24 + 1, ...: every one distinct
        assert work.tolist() == [0, 0]
        if cycle % 2:      # the pinned words, written by the kernel itself
            assert h_out.view(torch.int32).tolist() == out.view(torch.int32).tolist()
        if cycle > 1:      # and the status words it carried along
            assert torch.equal(h_status[:300], status[:300].cpu()) and torch.equal(h_status[300:301], status[777:778].cpu())
            assert int(h_status[301]) == -1


def test_replica_brick_with_a_typed_traced_energy(htf, cuda):
    """Particle types cross the decomposition: a three-species mixture whose epsilon / sigma are gathered by species pair (a
    generated kernel, hoomd_tf_amd/codegen.py) on a 4 x 2 brick in replica mode -- the row particle's type from its own position,
    a GHOST neighbor's from the halo message that delivered it -- against the replicated single-domain box, through an MD run."""
    from test_codegen_cpu import _typed_models
    from hoomd_tf_amd import standin
    from hoomd_tf_amd.brick import BrickDomain
    from hoomd_tf_amd.simmodel import PositionsInput
    grid, cells, ntypes = (4, 2, 1), 6, 3
    pos, vel, Lb = _brick_of_liquid(htf, cuda, cells, grid)
    rcut, rbuf, NN = 2.5, 0.4, 96
    Lg = Lb * np.asarray(grid)
    lo = -Lg / 2 + (np.asarray(grid) // 2) * Lb
    types = np.random.default_rng(5).integers(0, ntypes, len(pos))
    sysm = standin.System(pos + Lb / 2 + lo, Lg, types=types, dtype=torch.float32, device=cuda)
    sysm.vel = torch.from_numpy(vel).float().to(cuda)
    e = _typed_models(htf, htf.Nlist(torch.zeros((2, 4, 4))), PositionsInput.wrap(torch.zeros((2, 4))), ntypes, big=False)["lj_table"]
    pot = e.potential()
    nl = standin.CellNlist(sysm, r_cut=rcut, r_buff=rbuf, check_period=1)
    dom = nl.domain = BrickDomain(sysm, 0, grid, r_ghost=rcut + rbuf, r_buff=rbuf, replica=True, transport="local")
    nl.build()
    ctx = htf.Context(r_cut=rcut, nneighs=NN, scalar_dtype=torch.float32, max_n=sysm.N)
    ctx.set_potential(pot)
    nve = standin.NVE(sysm, 0.004)
    arr = ctx.make_arrays(sysm.pos, sysm.N, nl.n_neigh, nl.head_list, nl.nlist, sysm.box, sysm.force)
    n_steps = 80
    for ts in range(n_steps):
        nl.compute(ts)
        ctx.compute_forces_overlapped(ts, arr, dom)
        if ts < n_steps - 1:
            nve.step()
    torch.cuda.synchronize()
    assert nl.n_builds >= 2 and dom.n_migrated > 0
    live = dom.live_rows()
    assert len(live) == len(pos)
    p = sysm.pos[live, :3].double().cpu().numpy()
    t_live = sysm.pos[live, 3].contiguous().view(torch.int32).cpu().numpy()     # (w carries the type id's bits)
    assert sorted(t_live.tolist()) == sorted(types.tolist())                       # nobody changed species on the way
    got = sysm.force[live].cpu().numpy()
    reps = np.stack(np.meshgrid(*[np.arange(g) for g in grid], indexing="ij"), -1).reshape(-1, 3)
    base = p - lo
    allp = np.concatenate([base + r * Lb - Lg / 2 for r in reps])
    allp -= np.floor((allp + Lg / 2) / Lg) * Lg
    ref_sys = standin.System(allp, Lg, types=np.tile(t_live, len(reps)), dtype=torch.float32, device=cuda)
    ref_nl = standin.CellNlist(ref_sys, r_cut=rcut, r_buff=rbuf)
    ref_nl.build()
    ref_ctx = htf.Context(r_cut=rcut, nneighs=NN, scalar_dtype=torch.float32, max_n=ref_sys.N)
    ref_ctx.set_potential(pot)
    ref_ctx.compute_forces(0, ref_ctx.make_arrays(ref_sys.pos, ref_sys.N, ref_nl.n_neigh, ref_nl.head_list, ref_nl.nlist, ref_sys.box, ref_sys.force))
    torch.cuda.synchronize()
    mine = int(np.nonzero((reps == np.asarray(grid) // 2).all(axis=1))[0][0])
    want = ref_sys.force.cpu().numpy()[mine * len(p):(mine + 1) * len(p)]
    scale = np.abs(want).max()
    assert np.abs(got - want).max() < 3e-5 * scale, (np.abs(got - want).max(), scale)
    # and the species matter: the same rows with every type erased feel different forces
    ref0 = standin.System(allp, Lg, dtype=torch.float32, device=cuda)
    ref_ctx.compute_forces(0, ref_ctx.make_arrays(ref0.pos, ref0.N, ref_nl.n_neigh, ref_nl.head_list, ref_nl.nlist, ref0.box, ref0.force))
    torch.cuda.synchronize()
    assert np.abs(ref0.force.cpu().numpy()[mine * len(p):(mine + 1) * len(p)] - want).max() > 0.05 * scale
