"""A conservative htf.DescriptorMLP under slab domain decomposition, end to end: standin.Simulation + tfcompute with a
SlabDomain on two ranks that share the one GPU of the test box (gloo, host-staged halo: the rig of tests/test_gpu_domain.py).

fcc 8 x 5 x 5 cells at density 0.8442: 800 particles, slabs 6.72 wide (>= 2 r_ghost = 5.8), list r_cut 2.5 + r_buff 0.4,
NN = 128; layer K = 16, high = r_cut = 2.0, so fc vanishes inside the list and the list is symmetric within the descriptor.

Forces: after NVE steps that rebuild the list and migrate particles, the last forces of both ranks, gathered by particle id,
against the fp64 all-pairs gradient at the gathered positions (the oracle of test_nve_through_tfcompute), to TOL = 2e-5 of the
largest reference value, for l_max = 0 and 2; the momentum summed over the ranks within that test's bound.  Training: a few
trainable="total" steps against LJ labels in the same processes; the ranks' weights bit-identical, and within 2e-4 max|w| of
the single-domain run of the same worker (the bound of test_training_under_slabs_matches_single_domain)."""
import os
import queue
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from helpers import ROOT
from test_gpu_domain import _free_port

pytestmark = pytest.mark.gpu
TOL = 2e-5
STEPS, DT = 24, 0.005
TRAIN_STEPS = 6
WAIT = 420   # seconds a rank may take to answer


def _fcc_800(seed):
    cells = (8, 5, 5)
    a = (4.0 / 0.8442) ** (1.0 / 3.0)
    base = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
    grid = np.stack(np.meshgrid(*[np.arange(c) for c in cells], indexing="ij"), -1).reshape(-1, 3)
    pos = ((grid[:, None, :] + base[None]) * a).reshape(-1, 3)
    L = np.array(cells, dtype=np.float64) * a
    pos = pos - L / 2
    rng = np.random.default_rng(seed)
    pos += 0.04 * a * rng.standard_normal(pos.shape)
    pos -= np.round(pos / L) * L
    vel = np.zeros((len(pos), 4))
    vel[:, :3] = 1.5 * rng.standard_normal((len(pos), 3))
    vel[:, :3] -= vel[:, :3].mean(axis=0)
    vel[:, 3] = 1.0
    return pos, vel, L


def _setup(htf, rank, world, seed):
    """(sim, system, nlist, Ng) of this rank's slab of the 800-particle box; the particle id travels as the type."""
    from hoomd_tf_amd import standin
    from hoomd_tf_amd.domain import SlabDomain
    pos, vel, L = _fcc_800(seed)
    Ng = len(pos)
    assert Ng == 800
    bounds = -L[0] / 2 + np.linspace(0, 1, world + 1) * L[0]
    mine = (pos[:, 0] >= bounds[rank]) & (pos[:, 0] < bounds[rank + 1])
    system = standin.System(pos[mine], L, types=np.arange(Ng)[mine], dtype=torch.float32, device=torch.device("cuda:0"))
    system.vel = torch.from_numpy(vel[mine]).to(torch.float32).to(system.pos.device)
    sim = standin.Simulation(system)
    sim.integrate_nve(DT)
    nlist = sim.nlist_cell(r_buff=0.4, check_period=1)
    if world > 1:
        assert L[0] / world >= 2 * (2.5 + 0.4)
        nlist.domain = SlabDomain(system, rank, world, r_ghost=2.5 + nlist.r_buff)
    return sim, system, nlist, Ng, L


def _sum_over_ranks(t, world):
    if world > 1:
        dist.all_reduce(t)
    return t


def _forces_phase(htf, rank, world, l_max):
    """NVE driven by the conservative layer; -> the figures the parent asserts on (every rank returns the same reference)."""
    import test_gpu_desc_angular as A
    import test_gpu_desc_total as T
    lay = A._layer(htf, K=16, high=2.0, r_cut=2.0, seed=71, l_max=l_max) if l_max else T._layer(htf, K=16, high=2.0, r_cut=2.0, seed=71)
    sim, system, nlist, Ng, L = _setup(htf, rank, world, seed=6)
    model = T._model(htf, lay)(128)
    tfc = htf.tfcompute(model)
    tfc.attach(nlist, r_cut=2.5)
    dev = system.pos.device
    p0 = _sum_over_ranks(system.vel[:system.N, :3].double().sum(dim=0).cpu(), world)
    sim.run(STEPS)
    torch.cuda.synchronize()
    assert tfc._plan is None and not tfc.graph_safe()
    N = system.N
    ids = torch.from_numpy(np.asarray(system.types_numpy()[:N]).astype(np.int64))
    assert model.seen.shape[0] == N and system.force.shape[0] == N
    # gather by particle id: the positions the last forces were evaluated at, the forces, who owns what
    seen = torch.zeros((Ng, 3), dtype=torch.float64)
    got = torch.zeros((Ng, 4), dtype=torch.float64)
    owned = torch.zeros(Ng, dtype=torch.float64)
    seen[ids] = model.seen[:, :3].double().cpu()
    got[ids] = system.force[:N].double().cpu()
    owned[ids] = 1
    for t in (seen, got, owned):
        _sum_over_ranks(t, world)
    assert bool((owned == 1).all()), "particles lost or duplicated"
    p1 = _sum_over_ranks(system.vel[:N, :3].double().sum(dim=0).cpu(), world)
    vmax = torch.tensor([system.vel[:N, :3].abs().max().item()], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(vmax, op=dist.ReduceOp.MAX)
    moved = _sum_over_ranks(torch.tensor([float(nlist.domain.n_migrated if world > 1 else 0)], dtype=torch.float64), world)
    F, E = A._all_pairs(lay, seen.to(dev), torch.as_tensor(L, dtype=torch.float64, device=dev), torch.float64)
    out = {"l_max": l_max, "n_builds": int(nlist.n_builds), "migrated": int(moved.item()), "n_ghost": int(getattr(system, "n_ghost", 0)),
           "f_err": (got[:, :3] - F.cpu()).abs().max().item(), "f_scale": F.abs().max().item(),
           "e_err": (got[:, 3] - E.cpu()).abs().max().item(), "e_scale": E.abs().max().item(),
           "dp": (p1 - p0).abs().max().item(), "vmax": vmax.item(), "N": Ng}
    # this rank's own rows, not only the gathered table: nothing was filled in by the other rank
    out["f_err_own"] = (system.force[:N, :3].double().cpu() - F.cpu()[ids]).abs().max().item()
    return out


def _training_phase(htf, rank, world):
    """LJ drives the run and labels it; a trainable="total" layer learns every step.  -> (weights, last loss)."""
    import build_examples
    import test_gpu_desc_total_train as TT
    lay = htf.DescriptorMLP(K=16, H1=16, H2=16, low=0.5, high=2.0, r_cut=2.0, trainable="total", seed=5)
    sim, system, nlist, Ng, L = _setup(htf, rank, world, seed=8)
    lj = htf.tfcompute(build_examples.LJModel(128))
    lj.attach(nlist, r_cut=2.5)
    model = TT._model(htf, lay)(128, output_forces=False)
    model.compile(htf.optimizers.Adam(0.003), loss='MeanSquaredError')
    tfc = htf.tfcompute(model)
    tfc.attach(nlist, train=True, r_cut=2.5)
    tfc.set_reference_forces(lj)
    w0 = lay.w.clone()
    sim.run(TRAIN_STEPS)
    torch.cuda.synchronize()
    assert model.ops.count("descriptor_mlp") == TRAIN_STEPS and "generic" not in model.ops
    w = lay.w.detach().cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(w)) and np.abs(w - w0.cpu().numpy()).max() > 1e-3
    if world > 1:
        both = [torch.zeros(len(w), dtype=torch.float64) for _ in range(world)]
        dist.all_gather(both, torch.from_numpy(w))
        for o in both[1:]:
            assert torch.equal(o, both[0]), "ranks hold different weights after training"
        n_all = _sum_over_ranks(torch.tensor([system.N]), world)
        assert int(n_all) == Ng and system.n_ghost > 0
    return w, float(tfc._opt_state[20])


def _slab_worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        for p in (ROOT, os.path.join(ROOT, "tests")):
            if p not in sys.path:
                sys.path.insert(0, p)
        if world > 1:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        import hoomd_tf_amd as htf
        forces = [_forces_phase(htf, rank, world, l_max) for l_max in ((0, 2) if world > 1 else ())]
        w, loss = _training_phase(htf, rank, world)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        q.put((rank, world, {"forces": forces, "w": w, "loss": loss}, None))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, world, None, traceback.format_exc()))


def test_conservative_descriptor_under_two_slabs(htf, cuda):
    """Both worlds start together (three processes on the GPU) so that start-up is paid once; every wait has a timeout, and a
    rank that does not answer is terminated: no retry."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = []
    for world in (2, 1):
        port = _free_port()
        procs += [ctx.Process(target=_slab_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in procs:
            res.append(q.get(timeout=WAIT))
    except queue.Empty:
        pass
    finally:
        for p in procs:
            p.join(timeout=30 if len(res) == len(procs) else 1)
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    assert len(res) == len(procs), "only %d of %d ranks answered within %d s: %s" % (len(res), len(procs), WAIT, [r[:2] for r in res])
    for rank, world, out, err in res:
        assert out is not None, "rank %d of %d failed:\n%s" % (rank, world, err)
    by = {(rank, world): out for rank, world, out, _ in res}

    # forces and momentum, from either rank of the two-slab run
    for rank in (0, 1):
        for fr in by[(rank, 2)]["forces"]:
            print("rank %d %s" % (rank, fr))
            assert fr["n_builds"] >= 2 and fr["migrated"] > 0 and fr["n_ghost"] > 0, fr
            assert fr["f_scale"] > 1e-2
            assert np.isfinite(fr["f_err"]) and fr["f_err"] <= TOL * fr["f_scale"], fr
            assert fr["f_err_own"] <= fr["f_err"]
            assert np.isfinite(fr["e_err"]) and fr["e_err"] <= TOL * fr["e_scale"], fr
            bound = STEPS * fr["N"] * (2.0 ** -24 * fr["vmax"] + DT * TOL * fr["f_scale"])
            print("   momentum drift %.3g, bound %.3g" % (fr["dp"], bound))
            assert fr["dp"] <= bound, fr

    # training: two slabs against one domain
    w1, w2 = by[(0, 1)]["w"], by[(0, 2)]["w"]
    assert np.array_equal(by[(1, 2)]["w"], w2)
    err, scale = np.abs(w2 - w1).max(), np.abs(w1).max()
    print("training: max|w(2 slabs) - w(1 domain)| = %.3g of %.3g (ratio %.3g); loss %.6g vs %.6g"
          % (err, scale, err / scale, by[(0, 2)]["loss"], by[(0, 1)]["loss"]))
    assert scale > 0 and err < 2e-4 * scale
    assert np.isfinite(by[(0, 2)]["loss"]) and by[(0, 2)]["loss"] > 0
