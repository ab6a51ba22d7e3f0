"""The decomposition `bench.py --gpus N` actually builds, against the oracle of the UNDIVIDED box, at the metric's own size
(upstream's only multi-rank evidence is test_mpi_tensorflow.py:57-79 -- forces under
``comm.decomposition`` equal the serial ones, even and uneven (:65) cuts):

(a) BrickDomain(kernels backend, torch transport, replan_every=2) exactly as bench.run_md constructs it, the C3 box
    (131 072 particles, r_cut 3.0 + r_buff 0.4, NN 128) cut 5 x 1, 2 x 2, 2 x 1 and 2 x 1 uneven, the ranks sharing the one GPU
    over gloo (at most five rank processes beside the test's own, helpers.MAX_RANKS: the 8 x 1 and 4 x 2 cuts run in (b)), MD through >= 1 full re-plan AND >= 1 list-only rebuild, then 512 sampled live rows per rank against
    O.compute_forces over a brute-force list of all 131 072 particles;
(b) the same comparison in replica mode at full brick size (the 4 x 32 x 32-cell brick of 8 x 1, the 8 x 16 x 32-cell brick of
    4 x 2): what `bench.py --workload dd-self` times, transports local / peer / native, eager and replayed;
(c) BASELINE configs[4] (config 5) block for block: 131 072 particles per rank, weak scaling, on five ranks (655 360, 5 x 1 x 1;
    config 5 itself is eight such blocks, more rank processes than the one GPU may hold), the pair-MLP driving the MD, then one
    force-matching step -- sampled rows against O.pair_mlp_model on the undivided box, the all-reduced [loss, gradient] against
    a single-domain sweep over all of its rows, weights bit-identical across ranks.
"""
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

RCUT, RBUF, NN = 3.0, 0.4, 128


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _brute_rows(allpos, gid, Lv, r, dev):
    """Neighbor rows of particles ``gid`` over ALL particles within ``r`` (minimum image, fp64 on the device, 32 rows at a time):
    independent of the stand-in's cell list and of the decomposition."""
    P = torch.from_numpy(np.asarray(allpos, dtype=np.float64)).to(dev)
    Lt = torch.as_tensor(np.asarray(Lv, dtype=np.float64), device=dev)
    rows = []
    for c in range(0, len(gid), 32):
        g = torch.as_tensor(gid[c:c + 32], device=dev)
        d = P[None, :, :] - P[g][:, None, :]
        d -= torch.round(d / Lt) * Lt
        m = (d * d).sum(dim=2) <= r * r
        m[torch.arange(len(g), device=dev), g] = False
        for k in range(len(g)):
            rows.append(torch.nonzero(m[k]).flatten().cpu().numpy())
        del d, m
    return rows


def _oracle_rows(O, allpos32, gid, Lv, model, dev):
    """O.compute_forces (TensorflowCompute.cc:129-216 restated) for the particles ``gid`` of the undivided box -> (forces [n, 4],
    the fp64 pair vectors the model saw)."""
    Ng = len(allpos32)
    rows = _brute_rows(allpos32, gid, Lv, RCUT + 0.05, dev)
    n_neigh = np.array([len(r) for r in rows], dtype=np.uint32)
    head = np.concatenate([[0], np.cumsum(n_neigh)[:-1]]).astype(np.uint32)
    flat = np.concatenate(rows)
    # O.compute_forces evaluates rows [0, n_local): the sampled particles first
    rest = np.ones(Ng, dtype=bool)
    rest[gid] = False
    order = np.concatenate([gid, np.nonzero(rest)[0]])
    new_of_old = np.empty(Ng, dtype=np.int64)
    new_of_old[order] = np.arange(Ng)
    captured = {}

    def wrapped(x):
        captured["pv"] = x.astype(np.float64)
        return model(captured["pv"])

    ref, _ = O.compute_forces(allpos32[order], np.zeros(Ng, np.int32), n_neigh, head, new_of_old[flat].astype(np.uint32),
                              O.make_box(Lv, dtype=np.float32), RCUT, NN, wrapped, model_dtype=np.float32, n_local=len(gid))
    pv64 = captured["pv"]
    assert int((np.abs(pv64[:, :, :3]).sum(axis=2) > 0).sum(axis=1).max()) < NN
    return ref, pv64


def _gather_live(dom, sysm, Ng):
    """(ids of my live rows, the live row indices, every particle's position gathered over the ranks) -- with conservation."""
    live = dom.live_rows()
    my_ids = sysm.pos[live, 3].contiguous().view(torch.int32).cpu().numpy()
    loc = torch.zeros((Ng, 3), dtype=torch.float64)
    loc[my_ids] = sysm.pos[live, :3].double().cpu()
    owned = torch.zeros(Ng, dtype=torch.float64)
    owned[my_ids] = 1
    if dist.is_initialized():
        dist.all_reduce(loc)
        dist.all_reduce(owned)
    assert bool((owned == 1).all()), "particles lost or duplicated: %d ids owned != once" % int((owned != 1).sum())
    return my_ids, live, loc.numpy().astype(np.float32)


def _nobody_outside(dom, sysm, live, Lv, slack):
    """Every live row sits in its brick, give or take what moves between two plans (nearest periodic image)."""
    p = sysm.pos[live, :3].double().cpu().numpy()
    for d in dom.axes:
        mid = 0.5 * (dom.lo[d] + dom.hi[d])
        q = p[:, d] - np.round((p[:, d] - mid) / Lv[d]) * Lv[d]
        assert np.all((q >= dom.lo[d] - slack) & (q < dom.hi[d] + slack)), \
            "axis %d: a row at %.3f outside [%.3f, %.3f)" % (d, q[np.argmax(np.abs(q - mid))], dom.lo[d], dom.hi[d])


IMAGES = ("ghosts that cross the periodic boundary are delivered NEXT TO the brick -- owner + box vector, rounded once in fp32, as HOOMD's "
          "Communicator wraps its ghosts -- so a pair across that boundary is formed from x_j + L (ulp 1.9e-6 at |x| < 32) where the "
          "undivided box forms (x_j - x_i) - L (ulp 3.8e-6 at |dx| ~ 53): two valid fp32 evaluations up to 5e-6 apart in |dx|, "
          "times |df/dr| ~ 500 per first-shell pair")


def _rank_arrays(sysm):
    """What this rank's kernels see: [live local rows | live ghost rows] compacted -> (xyz fp32 [M, 3], particle ids [M], compact
    index of every row of sysm.pos or -1)."""
    P = sysm.pos.float().cpu().numpy()
    alive = ~np.isnan(P[:, 0])
    idx = np.nonzero(alive)[0]
    where = -np.ones(len(P), dtype=np.int64)
    where[idx] = np.arange(len(idx))
    return np.ascontiguousarray(P[idx, :3]), np.ascontiguousarray(P[idx, 3]).view(np.int32).copy(), where


def _sorted_r(pv64):
    r = np.sqrt((pv64[:, :, :3] ** 2).sum(axis=2))
    r[r == 0] = np.inf
    return np.sort(r, axis=1)


def _image_term(pair_forces, delta):
    """-> f(pv64) = sum_j |f_ij(x_ij moved by delta along r) - f_ij(x_ij)| + 2 |f_ij| delta / r: how far a row's force can move when
    every pair vector moves by ``delta`` (radial part by a finite difference of the model's own pair forces, transverse part from
    their magnitude)."""
    def term(pv64):
        r = np.sqrt((pv64[:, :, :3] ** 2).sum(axis=2))
        ok = r > 0
        rs = np.where(ok, r, 1.0)
        moved = pv64.copy()
        moved[:, :, :3] *= (1.0 + delta / rs)[:, :, None]
        f0, f1 = pair_forces(pv64)[:, :, :3], pair_forces(moved)[:, :, :3]
        rad = np.sqrt(((f1 - f0) ** 2).sum(axis=2))
        tra = 2.0 * np.sqrt((f0 ** 2).sum(axis=2)) * delta / rs
        return np.where(ok, rad + tra, 0.0).sum(axis=1)
    return term


def _parity_both_ways(O, tag, sysm, rows, got, owner_pos, owner_of, period, Lbox, model, dev, cond_of, touches_boundary,
                      image_term=None, tol=None, undivided=None):
    """The three statements that together say "this rank computes the undivided box's forces":
    A. forces of the sampled rows == O.compute_forces of THIS RANK'S OWN arrays (live locals + ghosts as delivered, a brute-force
       list over them): the kernels, the list and the binning, at the stated tolerance (what upstream's test_mpi asserts: both of
       its runs see the same wrapped ghosts, test_mpi_tensorflow.py:57-79);
    B. the rank's arrays HOLD the undivided box: every live ghost is a periodic image of its owner's current position (to the one
       fp32 rounding of the shift), and every sampled row's sorted neighbor distances below 2.999 equal the undivided box's;
    C. forces == O.compute_forces of the undivided box directly -- as stated for a brick that does not touch the periodic
       boundary, + the named image-rounding term where it does (IMAGES).
    ``rows``: sampled row indices into sysm.pos; ``owner_pos`` [n, 3] fp32 / ``owner_of(ids)`` -> row of owner_pos: the undivided
    box; ``period``: the lattice the images live on (box lengths; brick widths in replica mode); ``undivided``: (positions, gid of
    the sampled rows) of the box the direct oracle runs on."""
    from test_gpu_parity import LIQUID, assert_forces_close
    tol = tol or {}
    compact, ids, where = _rank_arrays(sysm)
    ref_r, pv_r = _oracle_rows(O, compact, where[rows], Lbox, model, dev)
    assert_forces_close(tag + "_own_arrays_energy", got[:, 3], ref_r[:, 3], **tol)
    assert_forces_close(tag + "_own_arrays", got[:, :3], ref_r[:, :3], cond_of(pv_r), cancelling_rows=LIQUID, **tol)
    # B: ghosts are images of their owners
    n_loc = int((where[:sysm.N] >= 0).sum())
    g_xyz, g_ids = compact[n_loc:].astype(np.float64), ids[n_loc:]
    d = g_xyz - owner_pos[owner_of(g_ids)].astype(np.float64)
    per = np.asarray(period, dtype=np.float64)
    off = np.abs(d - np.round(d / per) * per)
    # (one rounding of the shift, one of the sum, at the coordinates' own magnitude: ulp 3.8e-6 at 53.7, 3e-5 at the 430 of config 5)
    ulps = 2.0 ** -23 * (per.max() + np.abs(g_xyz).max())
    assert len(g_ids) > 0 and off.max() <= ulps, "a ghost is not a periodic image of its owner: off by %.3g (allowed %.3g)" % (off.max(), ulps)
    all_u, gid_u = undivided
    ref_u, pv_u = _oracle_rows(O, all_u, gid_u, Lbox, model, dev)
    ru, rr = _sorted_r(pv_u), _sorted_r(pv_r)
    n_in = (ru < 2.999).sum(axis=1)
    assert n_in.min() > 40
    for k in range(len(rows)):
        assert np.abs(rr[k, :n_in[k]] - ru[k, :n_in[k]]).max() <= 2e-5, "row %d: the rank's arrays do not hold the undivided box's neighbors" % k
        assert not np.isfinite(rr[k, n_in[k]:]).any() or rr[k, n_in[k]] >= 2.999 - 2e-5
    # C: the undivided box's oracle, directly
    cond_u = cond_of(pv_u)
    if touches_boundary and image_term is not None:
        extra = image_term(pv_u)
        from test_gpu_parity import _record
        err = np.abs(got[:, :3].astype(np.float64) - ref_u[:, :3])
        strict = tol.get("atol", 1e-5) + tol.get("rtol", 2e-5) * np.abs(ref_u[:, :3]) + tol.get("ctol", 2e-6) * cond_u[:, None]
        _record(tag + "_undivided_with_image_term", max_abs_err=err.max(), max_ratio_without_image_term=(err / strict).max(),
                max_ratio_with_image_term=(err / (strict + extra[:, None])).max(), image_term_used=1.0)
        assert np.all(err <= strict + extra[:, None]), (tag, (err / (strict + extra[:, None])).max())
    else:
        assert_forces_close(tag + "_undivided", got[:, :3], ref_u[:, :3], cond_u, cancelling_rows=LIQUID, **tol)
    assert_forces_close(tag + "_undivided_energy", got[:, 3], ref_u[:, 3], **{k: v for k, v in tol.items() if k != "ctol"})


def _c3_liquid(htf, dev, rank, steps=150):
    """The bench's own kind of configuration: rank 0 relaxes the jittered C3 lattice into a liquid at kT = 1 (force cap + velocity
    rescale, as bench.py's preparation) and hands every rank the same positions and velocities."""
    from hoomd_tf_amd import standin
    pos, L, a = standin.fcc_positions(32, 0.8442)
    Ng = len(pos)
    assert Ng == 131072
    state = torch.zeros((Ng, 6), dtype=torch.float64)
    if rank == 0:
        from test_gpu_parity import _liquid
        lsys, _, _ = _liquid(htf, dev, cells=32, steps=steps, seed=3)
        state[:, :3] = lsys.pos[:Ng, :3].double().cpu()
        state[:, 3:] = lsys.vel[:Ng, :3].double().cpu()
        del lsys
        torch.cuda.empty_cache()
    if dist.is_initialized():
        dist.broadcast(state, src=0)
    vel = np.zeros((Ng, 4))
    vel[:, :3] = state[:, 3:].numpy()
    vel[:, 3] = 1.0
    return state[:, :3].numpy().copy(), vel, np.asarray(L, dtype=np.float64)


def _headline_brick_worker(rank, world, port, q, grid, fractions, steps):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import hoomd_tf_amd as htf
        from hoomd_tf_amd import _lib, standin
        from hoomd_tf_amd.brick import BrickDomain
        from oracle import htf_oracle as O
        from test_gpu_parity import LIQUID, STATS, _cond_scale, _pair_forces_lj, assert_forces_close

        dev = torch.device("cuda:0")
        pos, vel, Lv = _c3_liquid(htf, dev, rank)
        Ng = len(pos)
        ids = np.arange(Ng)
        probe = BrickDomain(standin.System(pos[:1], Lv, dtype=torch.float32, device=dev), rank, grid, r_ghost=RCUT + RBUF, r_buff=RBUF,
                            n_global=Ng, fractions=fractions, replan_every=2)
        mine = np.ones(Ng, dtype=bool)
        for d in probe.axes:
            last = probe.coords[d] == grid[d] - 1
            mine &= (pos[:, d] >= probe.lo[d]) & ((pos[:, d] < probe.hi[d]) | last)
        del probe
        sysm = standin.System(pos[mine], Lv, types=ids[mine], dtype=torch.float32, device=dev)
        sysm.vel = torch.from_numpy(vel[mine]).to(torch.float32).to(dev)
        # ---- exactly what bench.run_md builds for world > 1 (bench.py: CellNlist(check_period 5, device_decision), BrickDomain(
        # transport "torch", replan_every 2), Context(fused = 2), BrickRun's force rows + fused integrate-and-pack)
        nl = standin.CellNlist(sysm, r_cut=RCUT, r_buff=RBUF, check_period=5, device_decision=True)
        dom = nl.domain = BrickDomain(sysm, rank, grid, r_ghost=RCUT + RBUF, r_buff=RBUF, n_global=Ng, transport="torch",
                                      fractions=fractions, replan_every=2)
        assert dom.kernels and dom.local_grid
        nl.build()
        ctx = htf.Context(r_cut=RCUT, nneighs=NN, scalar_dtype=torch.float32, max_n=sysm.N, fused=2)
        ctx.set_potential(htf.Potential.lj())
        nve = standin.NVE(sysm, 0.005)
        brun = standin.BrickRun(sysm, nl, ctx, nve)
        assert brun.fstep.available            # (the step bench.py times: integrator + halo pack as the force kernel's epilogue)
        for ts in range(steps - 1):
            nl.compute(ts)
            brun.advance(ts)
        nl.compute(steps - 1)
        brun._force_rows(steps - 1)                # the last step's forces alone: positions and forces of the same instant
        torch.cuda.synchronize()
        c = dom.counts_host()                                     # (raises on an overflow / lost-particle flag)
        full = dom.n_rebuilds - dom.n_light
        assert dom.n_light >= 1 and full >= 2, "the run must pass a list-only rebuild and a full re-plan (light %d, full %d)" % (dom.n_light, full)
        assert nl.dangerous_builds <= 1, nl.dangerous_builds
        n_live = int(c[_lib.BC_N_INT] + c[_lib.BC_N_BND])
        if world > 2:
            # an even share of the rows, and the interior rows the cut leaves: none where a brick is thinner than twice the plan's
            # ghost layer (3.8 at replan_every 2) along a cut axis, more than a fifth of them otherwise (5 x 1: slabs 10.7 thick,
            # ~29 %; 2 x 2: bricks 26.9 x 26.9, ~50 %)
            n_int, share = int(c[_lib.BC_N_INT]), Ng / world
            thin = any(Lv[d] / grid[d] < 2 * dom.r_ghost for d in dom.axes)
            assert 0.915 * share < n_live < 1.086 * share and (n_int == 0 if thin else n_int > 0.2 * n_live), (n_live, n_int, thin)
        my_ids, live, allpos = _gather_live(dom, sysm, Ng)
        assert len(live) == n_live
        moved = torch.tensor([dom.n_migrated])
        dist.all_reduce(moved)
        assert int(moved) > 0, "the run must exercise migration"
        _nobody_outside(dom, sysm, live, Lv, slack=2 * RBUF / 2 + 0.1)
        kT = torch.tensor([float((sysm.vel[live, :3].double() ** 2).sum())])
        dist.all_reduce(kT)
        kT = float(kT) / (3 * Ng)
        assert 0.85 < kT < 1.15, kT                                 # (the size-dependent bugs of round 5 showed here first: 0.98 -> 1.2)
        # ---- 512 of this rank's live rows: the oracle on this rank's own arrays, the arrays against the undivided box, and the
        # oracle on the undivided box directly (_parity_both_ways)
        pick = np.random.default_rng(100 + rank).choice(len(live), 512, replace=False)
        got = sysm.force[live].cpu().numpy()[pick]
        tag = "bricks%dx%dx%d%s_k2_c3_rank%d" % (grid + ("_uneven" if fractions else "", rank))
        touches = any(dom.coords[d] in (0, grid[d] - 1) for d in dom.axes)
        _parity_both_ways(O, tag, sysm, live.cpu().numpy()[pick], got, allpos, lambda i: i, Lv, Lv, O.lj_model, dev,
                          lambda pv: _cond_scale(pv, _pair_forces_lj(pv)), touches, image_term=_image_term(_pair_forces_lj, 5e-6),
                          undivided=(allpos, my_ids[pick]))
        # inert rows carry zero force
        inert = torch.ones(sysm.N, dtype=torch.bool, device=dev)
        inert[live] = False
        assert bool((sysm.force[inert] == 0).all())
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", {k: v for k, v in STATS.items() if k.startswith(tag)}))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc(), {}))


def _run(target, world, args, timeout=1500):
    from test_gpu_parity import _record
    check_rank_count(world)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + tuple(args)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        results = [q.get(timeout=timeout) for _ in procs]
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()      # our own children, by handle
    for rank, msg, stats in results:
        assert msg == "ok", "rank %d failed:\n%s" % (rank, msg)
        for k, v in stats.items():
            _record(k, **v)
    return results


@pytest.mark.parametrize("grid,fractions", [((5, 1, 1), None), ((2, 2, 1), None), ((2, 1, 1), None), ((2, 1, 1), {0: [0.33]})],
                         ids=["5x1x1-k2", "2x2x1-k2", "2x1x1-k2", "2x1x1-uneven-k2"])
def test_bricks_at_the_headline_geometry(htf, cuda, grid, fractions):
    """(a) of the module docstring."""
    _run(_headline_brick_worker, int(np.prod(grid)), (grid, fractions, 60))


# --------------------------------------------------------------------------- (b) replica mode at full brick size
def _replica_headline(htf, dev, grid, transport, replayed, tag):
    """One rank's brick of the C3 box cut ``grid`` ways, in replica mode (what bench.py --workload dd-self times): the brick is a
    liquid equilibrated in the BRICK's own periodic box, the logical box grid x that -- 131 072 particles, all images of the
    brick's 16 384.  After the run: 512 sampled rows against the oracle over ALL images."""
    from hoomd_tf_amd import _lib, standin
    from hoomd_tf_amd.brick import BrickDomain
    from oracle import htf_oracle as O
    from test_gpu_parity import LIQUID, _cond_scale, _pair_forces_lj, assert_forces_close
    cells = tuple(32 // g for g in grid)
    a = (4.0 / 0.8442) ** (1.0 / 3.0)
    base = np.array([[0.25, 0.25, 0.25], [0.75, 0.75, 0.25], [0.75, 0.25, 0.75], [0.25, 0.75, 0.75]])
    ijk = np.stack(np.meshgrid(*[np.arange(c) for c in cells], indexing="ij"), -1).reshape(-1, 3)
    Lb = np.array(cells, dtype=np.float64) * a
    pos = ((ijk[:, None, :] + base[None]) * a).reshape(-1, 3) - Lb / 2
    rng = np.random.default_rng(3)
    pos += 0.05 * a * rng.standard_normal(pos.shape)
    pos -= np.round(pos / Lb) * Lb
    nb = len(pos)
    assert nb == 16384
    # relax the brick in its own periodic box (force cap + rescale), as bench.py's preparation
    lsys = standin.System(pos, Lb, dtype=torch.float32, device=dev)
    lsys.randomize_velocities(kT=1.0, seed=3)
    lnl = standin.CellNlist(lsys, r_cut=RCUT, r_buff=RBUF, check_period=2)
    lctx = htf.Context(r_cut=RCUT, nneighs=NN, max_n=nb, fused=2)
    lctx.set_potential(htf.Potential.lj())
    lnve = standin.NVE(lsys, 0.005)
    for ts in range(150):
        lnl.compute(ts)
        lctx.compute_forces(ts, lctx.make_arrays(lsys.pos, nb, lnl.n_neigh, lnl.head_list, lnl.nlist, lsys.box, lsys.force))
        f3 = lsys.force[:, :3]
        f3.mul_(torch.clamp(200.0 / f3.norm(dim=1, keepdim=True).clamp_min(1e-12), max=1.0))
        lnve.step()
        v3 = lsys.vel[:, :3]
        v3.mul_(torch.sqrt(1.0 / ((v3 * v3).sum() / (3.0 * nb))))
    pos = lsys.pos[:nb, :3].double().cpu().numpy()
    vel = lsys.vel[:nb].double().cpu().numpy()
    del lsys, lnl, lctx
    g = np.asarray(grid)
    Lg = Lb * g
    coords = g // 2
    lo = -Lg / 2 + coords * Lb
    sysm = standin.System(pos + Lb / 2 + lo, Lg, types=np.arange(nb), dtype=torch.float32, device=dev)
    sysm.vel = torch.from_numpy(vel).to(torch.float32).to(dev)
    nl = standin.CellNlist(sysm, r_cut=RCUT, r_buff=RBUF, check_period=5, device_decision=True)
    dom = nl.domain = BrickDomain(sysm, 0, grid, r_ghost=RCUT + RBUF, r_buff=RBUF, replica=True, transport=transport, replan_every=2)
    nl.build()
    ctx = htf.Context(r_cut=RCUT, nneighs=NN, scalar_dtype=torch.float32, max_n=sysm.N, fused=2)
    ctx.set_potential(htf.Potential.lj())
    run = standin.BrickRun(sysm, nl, ctx, standin.NVE(sysm, 0.005))
    run.run(40)                                        # eager, through >= 2 rebuilds (what a capture needs behind it)
    if replayed:
        run.run(80, graph=True)
        assert run.n_cycles == 16 and run.n_rebuild_cycles >= 2
    else:
        run.run(80)
    # the forces in sysm.force are those of the LAST step's positions BEFORE its integration: evaluate once more at rest
    dom.exchange_end()
    dom.exchange()
    ctx.compute_forces(sysm.timestep, run._arrays())
    torch.cuda.synchronize()
    c = dom.counts_host()
    assert dom.n_light >= 1 and dom.n_rebuilds - dom.n_light >= 2, (dom.n_light, dom.n_rebuilds)
    assert int(c[_lib.BC_N_INT] + c[_lib.BC_N_BND]) == nb and dom.n_migrated > 0
    live = dom.live_rows()
    assert len(live) == nb
    _nobody_outside(dom, sysm, live, Lg, slack=2 * RBUF / 2 + 0.1)
    kT = float((sysm.vel[live, :3].double() ** 2).sum() / (3 * nb))
    assert 0.85 < kT < 1.15, kT
    # all images: image r of particle k at index r * nb + k; mine is image ``coords``
    p = sysm.pos[live, :3].double().cpu().numpy() - lo
    reps = np.stack(np.meshgrid(*[np.arange(x) for x in grid], indexing="ij"), -1).reshape(-1, 3)
    allp = np.concatenate([p + r * Lb - Lg / 2 for r in reps])
    allp -= np.floor((allp + Lg / 2) / Lg) * Lg
    mine = int(np.nonzero((reps == coords).all(axis=1))[0][0])
    pick = np.random.default_rng(17).choice(nb, 512, replace=False)
    got = sysm.force[live].cpu().numpy()[pick]
    own = sysm.pos[live, :3].float().cpu().numpy()
    own_ids = sysm.pos[live, 3].contiguous().view(torch.int32).cpu().numpy()
    row_of_id = np.empty(nb, dtype=np.int64)
    row_of_id[own_ids] = np.arange(nb)
    # (the images are built from positions wrapped into the logical box; the rank's own rows may sit a hair outside after the last
    #  steps -- the periodic lattice of images is the same)
    _parity_both_ways(O, tag, sysm, live.cpu().numpy()[pick], got, own, lambda i: row_of_id[i], Lb, Lg, O.lj_model, dev,
                      lambda pv: _cond_scale(pv, _pair_forces_lj(pv)), True, image_term=_image_term(_pair_forces_lj, 5e-6),
                      undivided=(allp.astype(np.float32), mine * nb + pick))


@pytest.mark.parametrize("replayed", [False, True], ids=["eager", "replayed"])
@pytest.mark.parametrize("transport", ["local", "peer", "native"])
@pytest.mark.parametrize("grid", [(8, 1, 1), (4, 2, 1)], ids=["8x1x1", "4x2x1"])
def test_replica_bricks_at_full_brick_size(htf, cuda, grid, transport, replayed):
    """(b) of the module docstring.  In a child process with a time limit (a transport that hung inside a replay would otherwise
    hold the session)."""
    import json
    import subprocess
    from hoomd_tf_amd import _lib
    from test_gpu_parity import _record
    if transport == "native" and not _lib.lib.htf_halo_available():
        pytest.skip("librccl not loadable")
    tag = "replica%dx%dx%d_%s_%s_k2" % (grid + (transport, "replayed" if replayed else "eager"))
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r); import torch, hoomd_tf_amd as htf\n"
            "import test_gpu_headline_bricks as t, test_gpu_parity as p\n"
            "t._replica_headline(htf, torch.device('cuda:0'), %r, %r, %r, %r)\n"
            "print('STATS ' + json.dumps({k: v for k, v in p.STATS.items() if k.startswith(%r)}))\n"
            % (ROOT, os.path.join(ROOT, "tests"), grid, transport, replayed, tag, tag))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, HTF_BRICK_WAIT_S="20", HTF_STATS_NO_FILE="1"))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("STATS ")]
    assert r.returncode == 0 and lines, r.stdout[-1500:] + r.stderr[-3000:]
    for k, v in json.loads(lines[-1][6:]).items():
        _record(k, **v)


# --------------------------------------------------------------------------- (c) config 5 at its own size
def _config5_worker(rank, world, port, q, md_steps):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import hoomd_tf_amd as htf
        from hoomd_tf_amd import _lib, standin
        from hoomd_tf_amd.brick import BrickDomain
        from oracle import htf_oracle as O
        from test_gpu_parity import STATS, assert_forces_close

        dev = torch.device("cuda:0")
        # bench.run_md, --scaling weak: every rank owns one 131 072-particle block, the global periodic box is `world` blocks side
        # by side along x (1 048 576 particles at config 5's 8 ranks, 655 360 at the five here)
        pos, L, a = standin.fcc_positions(32, 0.8442)
        rng = np.random.default_rng(5 + rank)
        pos = pos + 0.03 * a * rng.standard_normal(pos.shape)     # (thermal-size jitter: no overlapping pairs, no relaxation needed)
        pos -= np.round(pos / L) * L
        nb = len(pos)
        Lg = np.asarray(L, dtype=np.float64).copy()
        Lg[0] = L[0] * world
        pos[:, 0] += (rank - (world - 1) / 2.0) * L[0]
        Ng = nb * world
        assert Ng == 131072 * world
        sysm = standin.System(pos, Lg, types=rank * nb + np.arange(nb), dtype=torch.float32, device=dev)
        sysm.randomize_velocities(kT=1.0, seed=5 + rank)
        nl = standin.CellNlist(sysm, r_cut=RCUT, r_buff=RBUF, check_period=5, device_decision=True)
        grid = (world, 1, 1)
        dom = nl.domain = BrickDomain(sysm, rank, grid, r_ghost=RCUT + RBUF, r_buff=RBUF, n_global=Ng, transport="torch", replan_every=2)
        nl.build()
        layer = htf.PairMLP(32, 64, 64, 0.0, 3.0, activation="tanh", seed=3)      # bench.make_potential's C5b layer
        pot = layer.potential()
        w0 = layer.w.clone()
        ctx = htf.Context(r_cut=RCUT, nneighs=NN, scalar_dtype=torch.float32, max_n=sysm.N, fused=0)
        ctx.set_potential(pot)
        brun = standin.BrickRun(sysm, nl, ctx, standin.NVE(sysm, 0.005))
        # ---- 5a: the pair-MLP drives the MD
        for ts in range(md_steps - 1):
            nl.compute(ts)
            brun.advance(ts)
        nl.compute(md_steps - 1)
        brun._force_rows(md_steps - 1)
        torch.cuda.synchronize()
        c = dom.counts_host()
        assert dom.n_rebuilds >= 2, dom.n_rebuilds
        n_live = int(c[_lib.BC_N_INT] + c[_lib.BC_N_BND])
        assert 125000 < n_live < 137000 and int(c[_lib.BC_N_INT]) > 0.6 * n_live      # slabs 53.7 thick: most rows see no ghost
        my_ids, live, allpos = _gather_live(dom, sysm, Ng)
        _nobody_outside(dom, sysm, live, Lg, slack=2 * RBUF / 2 + 0.1)
        total = torch.tensor([n_live])
        dist.all_reduce(total)
        assert int(total) == Ng                                                       # the global batch of 5b
        params = {k: v.copy() for k, v in layer.params.items()}
        pick = np.random.default_rng(200 + rank).choice(len(live), 256, replace=False)
        captured = {}

        def model(x):
            out, gg = O.pair_mlp_model(x, params, 0.0, 3.0, "tanh", return_grad=True)
            captured["gg"] = gg
            return out

        got = sysm.force[live].cpu().numpy()[pick]
        tag = "config5_%dx131072_rank%d" % (world, rank)

        def cond_of(pv):
            model(pv)
            return np.abs(2 * captured["gg"]).sum(axis=(1, 2))

        def mlp_pair_forces(pv):
            model(pv)
            return 2.0 * captured["gg"]

        # (the box is 269 long: coordinates carry ulps of up to 1.5e-5 there, eight times the C3 box's)
        _parity_both_ways(O, tag, sysm, live.cpu().numpy()[pick], got, allpos, lambda i: i, Lg, Lg, model, dev, cond_of,
                          rank in (0, world - 1), image_term=_image_term(mlp_pair_forces, 4e-5), tol=dict(atol=2e-5, rtol=5e-5, ctol=5e-6),
                          undivided=(allpos, my_ids[pick]))
        # ---- 5b: one force-matching step (tensorflowcompute.py:347-370 train_on_batch; labels = the LJ forces of this configuration,
        # example 06): sweep over this rank's rows -> all-reduce of [loss, 6 337 gradients] -> Adam on the device
        pv = ctx.nlist_buffer(sysm.N, dev)
        lj = htf.Potential.lj()
        labels = htf.ops.eval_forces(lj, pv)
        accum = htf.ops.train_pair_grad(pot, pv, labels)
        mine_accum = accum.clone()
        dist.all_reduce(accum)
        acc_all = accum.double().cpu().numpy()
        opt_desc = htf.optimizers.Adam(1e-3).desc(0, (0.0,))
        opt_state = torch.zeros(htf.ops.optimizer_state_floats(layer.w.numel()), dtype=torch.float32, device=dev)
        htf.ops.optimizer_step(layer.w, accum, 1.0 / (4.0 * Ng), opt_state, opt_desc)
        layer.after_update()
        torch.cuda.synchronize()
        w1 = layer.w.double().cpu()
        assert torch.isfinite(w1).all() and float((w1 - w0.double().cpu()).abs().max()) > 1e-4      # Adam's first step moves every weight by ~lr
        everybody = [torch.zeros_like(w1) for _ in range(world)]
        dist.all_gather(everybody, w1)
        for o in everybody[1:]:
            assert torch.equal(o, everybody[0]), "ranks hold different weights after the training step"
        # inert rows contribute nothing: the sweep over the live rows alone gives the same partial
        lp = pv[live].contiguous()
        acc_live = htf.ops.train_pair_grad(pot_before(htf, params), lp, labels[live].contiguous()).double().cpu().numpy()
        ma = mine_accum.double().cpu().numpy()
        assert abs(acc_live[0] - ma[0]) <= 1e-4 * abs(ma[0]) and np.abs(acc_live[1:] - ma[1:]).max() <= 2e-4 * np.abs(ma[1:]).max()
        # the undivided box, single domain (every rank builds it: 655 360 rows, a 1.25 GiB pair-vector tensor): this rank's partial ==
        # the sweep over the undivided box's rows of this rank's particles, and on rank 0 the all-reduced [loss, gradient] == ONE sweep
        # over all of its rows
        stats = {k: v for k, v in STATS.items() if k.startswith(tag)}
        whole = standin.System(allpos.astype(np.float64), Lg, dtype=torch.float32, device=dev)
        wnl = standin.CellNlist(whole, r_cut=RCUT, r_buff=RBUF)
        wnl.build()
        wpv = htf.ops.build_pair_vectors(whole.pos, wnl.n_neigh, wnl.head_list, wnl.nlist, whole.box, RCUT, NN)
        wl = htf.ops.eval_forces(lj, wpv)
        idx = torch.from_numpy(my_ids.astype(np.int64)).to(dev)
        lab_err = float((labels[live] - wl[idx]).abs().max() / wl.abs().max())
        part = htf.ops.train_pair_grad(pot_before(htf, params), wpv[idx].contiguous(), wl[idx].contiguous()).double().cpu().numpy()
        pg = np.abs(part[1:]).max()
        p_loss, p_grad = abs(part[0] - ma[0]) / part[0], np.abs(part[1:] - ma[1:]).max() / pg
        stats["config5_train_rank%d_partial_vs_undivided_rows" % rank] = dict(loss_rel_err=p_loss, grad_err_over_max=p_grad, bound=2e-4,
                                                                              label_err_over_max=lab_err)
        assert p_loss <= 1e-4 and p_grad <= 2e-4, (rank, p_loss, p_grad, lab_err)
        # the per-sweep tolerance carried through the sum over ranks: each partial is within 2e-4 max|g_r| of its rows' gradient, so the
        # all-reduced gradient is within 2e-4 sum_r max|g_r| -- the partials largely CANCEL in the sum (|sum| << sum of |parts|)
        scale = torch.tensor([pg], dtype=torch.float64)
        dist.all_reduce(scale)
        parts_sum = torch.from_numpy(part.copy())
        dist.all_reduce(parts_sum)
        if rank == 0:
            wacc = htf.ops.train_pair_grad(pot_before(htf, params), wpv, wl).double().cpu().numpy()
            gmax = np.abs(wacc[1:]).max()
            assert wacc[0] > 0 and gmax > 0
            loss_err, grad_err = abs(acc_all[0] - wacc[0]) / wacc[0], np.abs(acc_all[1:] - wacc[1:]).max() / gmax
            stats["config5_train_allreduce_vs_single_domain"] = dict(loss_rel_err=loss_err, grad_err_over_max=grad_err, bound=2e-4,
                                                                     loss=wacc[0] / (4.0 * Ng))
            cancel = float(scale) / gmax
            same_rows = np.abs(parts_sum.numpy()[1:] - wacc[1:]).max() / gmax      # (the undivided box's own rows, swept rank by rank)
            stats["config5_train_allreduce_vs_single_domain"].update(sum_of_rank_maxima_over_max=cancel, grad_err_over_sum_of_rank_maxima=grad_err / cancel,
                                                                     undivided_rows_by_rank_vs_one_sweep=same_rows)
            assert loss_err <= 1e-4 and grad_err <= 2e-4 * cancel, (loss_err, grad_err, cancel, same_rows, p_grad)
        del wpv, wl, whole, wnl
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, "ok", stats))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc(), {}))


def pot_before(htf, params):
    """The pair-MLP at the weights the sweep under test saw (the layer's own potential has been updated since)."""
    import torch as _t
    flat = np.concatenate([np.asarray(params[k], dtype=np.float32).ravel() for k in ("W1", "b1", "W2", "b2", "W3", "b3")])
    theta = _t.tensor(flat, dtype=_t.float32, device="cuda")
    pot = htf.Potential.pair_mlp(params, 0.0, 3.0, activation="tanh", precision="split16", theta=theta)
    pot._theta_keepalive = theta
    return pot


def test_config5_blocks_on_five_ranks(htf, cuda):
    """(c) of the module docstring: BASELINE configs[4]'s 131 072-particle blocks, 5 ranks sharing the GPU."""
    _run(_config5_worker, 5, (25,), timeout=2400)
