"""Installed plans against the model the user has NOW.  After the first traced step tfcompute replays a plan (the inference
plan, the training plan) and Simulation.run may replay a whole check period from a hipGraph without calling compute() at all.
Between two runs the user may write a weight, recompile the optimizer or flip ``train``; every later step must compute the
model as it then stands.  Each case: run until the plan is installed, change one piece of state, run again on every route
(graph=False, graph=True, graph=None), and hold the last step's forces to an fp64 restatement of the model with the present
weights on that step's own pair vectors -- and to the change the write predicts -- and the routes to each other bit for bit."""
import numpy as np
import pytest
import torch

import build_examples
from oracle import graph_torch as G

pytestmark = pytest.mark.gpu

STEPS = 256                     # graph=None replays only runs of at least 256 steps
ROUTES = (False, True, None)


def _sim(cuda, check_period, dt=0.002, kT=0.3):
    from hoomd_tf_amd import standin
    pos, L, a = standin.fcc_positions(6, 0.8442)
    rng = np.random.default_rng(2)
    pos = pos + 0.03 * a * rng.standard_normal(pos.shape)
    pos -= np.round(pos / L) * L
    sysm = standin.System(pos, L, dtype=torch.float32, device=cuda)
    sysm.randomize_velocities(kT=kT, seed=2)
    sim = standin.Simulation(sysm)
    sim.integrate_nve(dt)
    return sysm, sim, sim.nlist_cell(r_buff=0.4, check_period=check_period)


def _reference(nl64, energy_fn):
    """fp64 compute_nlist_forces (simmodel.py:526-555) of ``energy_fn(pair vectors) -> [B, NN] pair or [B] row energies`` on
    the step's own pair vectors -> (forces [B, 4], sum_j |f_ij| per row: the condition scale of the row sum)."""
    x = torch.from_numpy(nl64).requires_grad_(True)
    e = energy_fn(x)
    (g,) = torch.autograd.grad(e.sum(), x)
    rows = e.sum(dim=1) if e.dim() == 2 else e
    f = torch.cat([2.0 * g[:, :, :3].sum(dim=1), rows.detach()[:, None]], dim=1)
    return f.numpy(), np.abs(2.0 * g[:, :, :3].numpy()).sum(axis=(1, 2))


def _check_last_step(tag, tfc, energy_now, energy_before=None, **tol):
    """The forces the last step left against the fp64 model with the weights as they are now, on that step's pair vectors; and,
    after a write, the energy moved from the old weights' value to the new one's (a plan that ignored the write fails here)."""
    from test_gpu_parity import CONTACTS, assert_forces_close
    N = tfc.system.N
    nl64 = tfc.get_nlist_array().reshape(N, tfc.nneighbor_cutoff, 4)
    got = tfc.get_forces_array()
    ref, cond = _reference(nl64, energy_now)
    assert_forces_close(tag, got, ref, cond, cancelling_rows=CONTACTS, **tol)
    if energy_before is not None:
        old, _ = _reference(nl64, energy_before)
        e_got, e_new, e_old = got[:, 3].sum(), ref[:, 3].sum(), old[:, 3].sum()
        assert abs(e_new - e_old) > 1e-2 * abs(e_new), (tag, e_new, e_old)       # (the write matters)
        assert abs(e_got - e_new) < 1e-3 * abs(e_new - e_old), (tag, e_got, e_new, e_old)
    return nl64


def _routes_agree(runs):
    """graph=True and graph=None give graph=False's positions, velocities and forces after every run, bit for bit."""
    ref = runs[False]
    for route in (True, None):
        assert len(runs[route]) == len(ref)
        for k, (a, b) in enumerate(zip(ref, runs[route])):
            for name, x, y in zip(("positions", "velocities", "forces"), a, b):
                assert torch.equal(x, y), "graph=%s: %s differ from the stepwise run after run %d (max |d| %.3g)" % (
                    route, name, k, float((x - y).abs().max()))


def _snapshot(sysm, tfc):
    torch.cuda.synchronize()
    return sysm.pos.clone(), sysm.vel.clone(), tfc.force.clone()


def _count_computes(tfc):
    calls = [0]
    compute = tfc.compute

    def counted(ts):
        calls[0] += 1
        return compute(ts)
    tfc.compute = counted
    return calls


def _assert_still_replays(sim, tfc, write):
    """graph=None: a weight write does not switch the simulation off the replay -- the step still captures, and where the
    measurement picked the replay (a host-bound step; a kernel-bound one may measure faster stepwise) the next long run replays."""
    write()
    calls = _count_computes(tfc)
    sim.run(STEPS)
    torch.cuda.synchronize()
    assert not getattr(sim, "_no_graph", False), "a weight write turned the replay off"
    assert sim._graph is not None and "graph_us" in sim.graph_choice, sim.graph_choice
    if sim.graph_choice["use_graph"]:
        assert calls[0] < STEPS // 2, "the run after the write stepped %d of %d steps eagerly" % (calls[0], STEPS)


def _run_schedule(cuda, check_period, make_model, writes, energy_of, tag, dt=0.002, tol=None, after=None):
    """Every route: warm-up (plan installed), then for each ``write`` in the schedule: write (None: nothing), run STEPS steps,
    fp64 check of the last step.  -> {route: [(pos, vel, force) after each run]}."""
    runs = {}
    for route in ROUTES:
        sysm, sim, nl = _sim(cuda, check_period, dt=dt)
        model = make_model()
        from hoomd_tf_amd import tfcompute
        tfc = tfcompute(model)
        tfc.attach(nl, r_cut=2.5)
        sim.run(7, graph=False)
        assert tfc._plan is not None and tfc.model._plan is tfc._plan
        out = []
        for k, write in enumerate(writes):
            before = energy_of(model)
            if write is not None:
                write(model)
            sim.run(STEPS, graph=route)
            out.append(_snapshot(sysm, tfc))
            _check_last_step("%s_cp%d_graph%s_run%d" % (tag, check_period, route, k), tfc, energy_of(model),
                             before if write is not None else None, **(tol or {}))
            assert tfc._plan is not None and tfc.model._plan is tfc._plan
        if route is None and after is not None:
            _assert_still_replays(sim, tfc, lambda: after(model))
        runs[route] = out
    _routes_agree(runs)
    return runs


def tfc_of(model):
    """The force compute of the simulation being run (each route builds its own)."""
    from hoomd_tf_amd import standin
    f = standin.current_simulation().forces[0]
    assert f.model is model
    return f


# --------------------------------------------------------------------------- traced energies with torch Parameters
def _morse_energy(depth, width):
    def e(x):
        live = (G.nlist_rinv(x) > 0.0).to(x.dtype)
        r = G.safe_norm(x[:, :, :3], dim=2)
        y = 1.0 - torch.exp(-1.0 * width * (r - 1.122))
        return 0.5 * depth * live * (y * y - 1.0)
    return e


def _morse_model(htf, device):
    class Morse(htf.SimModel):
        def setup(self):
            self.depth = torch.nn.Parameter(torch.tensor(0.8, device=device))
            self.width = torch.nn.Parameter(torch.tensor(4.0, device=device))

        def compute(self, nlist, positions, box):
            r = htf.safe_norm(nlist[:, :, :3], axis=2)
            live = htf.cast(htf.nlist_rinv(nlist) > 0.0, torch.float32)
            x = 1.0 - htf.exp(-1.0 * self.width * (r - 1.122))
            return htf.compute_nlist_forces(nlist, htf.reduce_sum(0.5 * self.depth * live * (x * x - 1.0), axis=1))
    return Morse(96)


def _user_sgd_step(model):
    """One step of an optimizer of the user's own on the model's parameters."""
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    for p in model.parameters():
        p.grad = torch.full_like(p, -2.0)      # (+0.2 on every weight)
    opt.step()
    opt.zero_grad(set_to_none=True)


@pytest.mark.parametrize("check_period", [1, 3])
@pytest.mark.parametrize("placement", ["before_capture", "between_replays"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_traced_weights_follow_writes_on_every_route(htf, cuda, monkeypatch, tmp_path, check_period, placement, where):
    """A traced energy whose weights are kernel arguments (TracedWeights.theta): fill_, set_weights, a user's torch SGD step and
    load_weights between runs all reach the next step -- the replayed one too, and a write just before the run that captures is
    copied in before the capture, not recorded inside it."""
    from hoomd_tf_amd import _lib
    monkeypatch.setenv("HTF_NO_JIT", "0")
    device = "cpu" if where == "host" else cuda
    np.savez(str(tmp_path / "w.npz"), np.float32(0.9), np.float32(4.2))   # (SimModel.save_weights' layout: depth, width)

    def fill_depth(m):
        with torch.no_grad():
            m.depth.fill_(1.6)

    def fill_width(m):
        with torch.no_grad():
            m.width.fill_(3.0)

    writes = [fill_depth, fill_width, lambda m: m.set_weights([np.float32(1.2), np.float32(3.5)]), _user_sgd_step,
              lambda m: m.load_weights(str(tmp_path / "w.npz"))]
    if placement == "between_replays":
        writes = [None] + writes        # (the first run captures with nothing to copy; every write then meets a reused capture)
    models = []

    def make():
        models.append(_morse_model(htf, device))
        return models[-1]

    def energy_of(m):
        return _morse_energy(float(m.depth.detach()), float(m.width.detach()))

    def after(m):
        with torch.no_grad():
            m.depth.fill_(1.1)
    _run_schedule(cuda, check_period, make, writes, energy_of, "traced_%s_%s" % (where, placement), after=after)
    assert len(models) == 3 and all(m._plan.kind == _lib.POT_JIT for m in models)


def test_weights_of_several_row_terms_follow_a_write_on_every_route(htf, cuda, monkeypatch):
    """An energy of two row terms (_TracedWeightsOfTerms: the step's kernel, then a streaming evaluation) with a weight in the
    second: written between runs, it reaches the replayed step."""
    from hoomd_tf_amd.simmodel import _TracedWeightsOfTerms
    monkeypatch.setenv("HTF_NO_JIT", "0")

    class FS(htf.SimModel):
        def setup(self):
            self.amp = torch.nn.Parameter(torch.tensor(1.3, device="cuda"))

        def compute(self, nlist, positions, box):
            s = htf.nlist_rinv(nlist)
            r = htf.safe_norm(nlist[:, :, :3], axis=2)
            rho = htf.reduce_sum(htf.exp(-1.7 * r) * s * s, axis=1)
            phi = htf.reduce_sum(2.0 * s ** 12, axis=1)
            return htf.compute_nlist_forces(nlist, phi - self.amp * htf.sqrt(rho + 0.01))

    def energy_of(m):
        amp = float(m.amp.detach())

        def e(x):
            s = G.nlist_rinv(x)
            r = G.safe_norm(x[:, :, :3], dim=2)
            rho = (torch.exp(-1.7 * r) * s * s).sum(dim=1)
            return (2.0 * s ** 12).sum(dim=1) - amp * torch.sqrt(rho + 0.01)
        return e

    def fill(m):
        assert isinstance(tfc_of(m)._plan_weights, _TracedWeightsOfTerms)     # (the case: the weights of several terms)
        with torch.no_grad():
            m.amp.fill_(2.6)
    _run_schedule(cuda, 1, lambda: FS(96), [None, fill], energy_of, "row_terms")


def test_a_folded_weight_retraces_on_every_route(htf, cuda, monkeypatch):
    """A weight whose value is folded into the generated kernel's text (an Add with a constant: _plan_folded): a write makes the
    plan stale, and the next step re-traces under every route -- the replay must not run the old kernel."""
    monkeypatch.setenv("HTF_NO_JIT", "0")

    class Folded(htf.SimModel):
        def setup(self):
            self.depth = torch.nn.Parameter(torch.tensor(0.8, device="cuda"))

        def compute(self, nlist, positions, box):
            r = htf.safe_norm(nlist[:, :, :3], axis=2)
            live = htf.cast(htf.nlist_rinv(nlist) > 0.0, torch.float32)
            x = 1.0 - htf.exp(-4.0 * (r - 1.122))
            return htf.compute_nlist_forces(nlist, htf.reduce_sum(0.5 * (self.depth + 1.0) * live * (x * x - 1.0), axis=1))

    def fill(m):
        assert tfc_of(m)._plan_folded != ()       # (the case: the plan holds the weight as a constant)
        with torch.no_grad():
            m.depth.fill_(2.0)

    def energy_of(m):
        return _morse_energy(float(m.depth.detach()) + 1.0, 4.0)
    _run_schedule(cuda, 1, lambda: Folded(96), [None, fill], energy_of, "folded")


# --------------------------------------------------------------------------- built-in layers
def _lj_energy(w):
    w0, w1 = float(w[0]), float(w[1])

    def e(x):
        r = G.safe_norm(x[:, :, :3], dim=2)
        mask = r > G.RINV_DELTA
        rs = torch.where(mask, r, torch.ones_like(r))
        r6 = torch.where(mask, w1 ** 6 / rs ** 6, torch.zeros_like(r))
        return w0 * 4.0 * (r6 ** 2 - r6) / 2.0
    return e


def test_lj_layer_inference_follows_writes_on_every_route(htf, cuda):
    """LJLayer inference (TrainableGraph, train=False: the one-kernel plan reads the layer's device weights): set_weights and an
    in-place write to trainable_weights[0] reach the next step on every route."""
    def make():
        return build_examples.TrainableGraph(96, sig=1.0, eps=1.0)

    def energy_of(m):
        return _lj_energy(m.lj.w.detach().cpu().numpy())

    def copy_in_place(m):
        with torch.no_grad():
            m.lj.trainable_weights[0].copy_(torch.tensor([0.8, 0.98]))

    def scale_in_place(m):
        with torch.no_grad():
            m.lj.trainable_weights[0][0:1].mul_(1.5)
    writes = [None, lambda m: m.set_weights([np.array([1.3, 1.0], dtype=np.float32)]), copy_in_place, scale_in_place]
    _run_schedule(cuda, 1, make, writes, energy_of, "lj_layer", after=lambda m: m.lj.w.mul_(1.01))
    # the fp64 restatement is graph_torch's LJLayer (example 06)
    x = torch.from_numpy(np.random.default_rng(0).uniform(0.6, 1.6, (8, 5, 4)))
    ref, _ = _reference(x.numpy(), _lj_energy([1.3, 0.98]))
    np.testing.assert_allclose(ref, G.lj_param_forces(x, torch.tensor([1.3, 0.98], dtype=torch.float64)).detach().numpy(),
                               rtol=1e-12, atol=1e-12)


def _mlp_energy(w, dims=(32, 64, 64), low=0.0, high=3.0):
    K, H1, H2 = dims
    w = torch.from_numpy(np.asarray(w, dtype=np.float64))
    o = 0
    W1 = w[o:o + K * H1].reshape(K, H1); o += K * H1
    b1 = w[o:o + H1]; o += H1
    W2 = w[o:o + H1 * H2].reshape(H1, H2); o += H1 * H2
    b2 = w[o:o + H2]; o += H2
    W3 = w[o:o + H2]; o += H2
    b3 = w[o]

    def e(x):
        r = G.safe_norm(x[:, :, :3], dim=2)
        u = torch.tanh(torch.tanh(G.rbf_expansion(r, low, high, K) @ W1 + b1) @ W2 + b2) @ W3 + b3
        return 0.5 * u * (r > G.RINV_DELTA).to(x.dtype)
    return e


@pytest.mark.parametrize("precision", ["split16", "fp32"])
def test_pair_mlp_inference_follows_writes_on_every_route(htf, cuda, precision):
    """PairMLP inference: the kernels read operand images built from ``layer.w``.  set_weights rebuilds them; so must an in-place
    write to ``layer.w`` (trainable_weights[0]) -- on every route, the eager one included."""
    H2 = 64

    def make():
        return build_examples.PairMLPModel(96, activation="tanh", precision=precision)

    def energy_of(m):
        return _mlp_energy(m.mlp.w.detach().cpu().numpy())

    def set_weights(m):
        ws = m.get_weights()
        ws[4], ws[5] = ws[4] * 1.5, ws[5] * 1.5       # (W3, b3: the energy scales by 1.5)
        m.set_weights(ws)

    def halve_in_place(m):
        with torch.no_grad():
            m.mlp.trainable_weights[0][-(H2 + 1):].mul_(0.5)
    _run_schedule(cuda, 1, make, [None, set_weights, halve_in_place], energy_of, "pair_mlp_%s" % precision,
                  tol=dict(atol=2e-5, rtol=5e-5, ctol=5e-6),
                  after=lambda m: m.mlp.trainable_weights[0][-(H2 + 1):].mul_(1.25))
    x = torch.from_numpy(np.random.default_rng(0).uniform(0.6, 1.6, (8, 5, 4)))
    w = make().mlp.make_trainable().detach().cpu().numpy().astype(np.float64)
    ref, _ = _reference(x.numpy(), _mlp_energy(w))
    np.testing.assert_allclose(ref, G.pair_mlp_param_forces(x, torch.from_numpy(w), (32, 64, 64)).detach().numpy(),
                               rtol=1e-12, atol=1e-12)


# --------------------------------------------------------------------------- training
def _trainer(htf, cuda, optimizer):
    """examples/06: LJLayer trained by force matching against a plain LJ reference compute at every step."""
    sysm, sim, nl = _sim(cuda, 1, kT=0.5)
    lj = htf.tfcompute(build_examples.LJModel(96))
    lj.attach(nl, r_cut=2.5)
    model = build_examples.TrainableGraph(96, output_forces=False, sig=0.8, eps=1.05)
    model.compile(optimizer, loss='MeanSquaredError')
    tfc = htf.tfcompute(model)
    tfc.attach(nl, train=True, r_cut=2.5)
    tfc.set_reference_forces(lj)
    return sysm, sim, lj, model, tfc


@pytest.mark.parametrize("route", ROUTES)
def test_training_plan_follows_the_train_flag(htf, cuda, route):
    """The replayed training step (_tplan): ``tfc.train = False`` freezes the weights bit for bit; ``True`` again trains."""
    sysm, sim, lj, model, tfc = _trainer(htf, cuda, htf.optimizers.Adam(0.01))
    sim.run(10, graph=False)
    assert tfc._tplan is not None
    w0, n0 = model.lj.w.clone(), float(tfc._opt_state[19])
    tfc.train = False
    sim.run(STEPS, graph=route)
    torch.cuda.synchronize()
    assert torch.equal(model.lj.w, w0) and float(tfc._opt_state[19]) == n0, "train = False: the training plan kept training"
    tfc.train = True
    sim.run(5, graph=route)
    torch.cuda.synchronize()
    assert not torch.equal(model.lj.w, w0) and float(tfc._opt_state[19]) == n0 + 5
    assert tfc._tplan is not None


@pytest.mark.parametrize("route", ROUTES)
def test_inference_plan_trains_once_train_is_set(htf, cuda, route):
    """``tfc.train = True`` on a compute whose inference plan is installed: the next steps train (as upstream's _finish_update
    does), they do not silently run inference."""
    sysm, sim, nl = _sim(cuda, 1)
    model = build_examples.TrainableGraph(96, sig=1.0, eps=1.0)
    model.compile(htf.optimizers.Adam(0.01), loss='MeanSquaredError')
    tfc = htf.tfcompute(model)
    tfc.attach(nl, r_cut=2.5)
    sim.run(STEPS, graph=route)
    assert tfc._plan is not None and tfc.model._plan is tfc._plan
    w0 = model.lj.w.clone()
    tfc.train = True
    sim.run(3, graph=route)
    torch.cuda.synchronize()
    assert not torch.equal(model.lj.w, w0), "train = True on an inference plan: the weights did not train"
    assert tfc._opt_state is not None and float(tfc._opt_state[19]) == 3.0


class _TorchLJParam:
    """LJLayer's energy (example 06) in plain torch ops on torch Parameters: the generic training route (torch autograd, the
    compiled optimizer's torch twin)."""

    @staticmethod
    def make(htf, sig, eps):
        class M(htf.SimModel):
            def setup(self):
                self.w = torch.nn.Parameter(torch.tensor([sig, eps], device="cuda"))

            def compute(self, nlist, positions, box):
                r = torch.sqrt(torch.sum((nlist[:, :, :3] + 1e-7) ** 2, dim=2))
                mask = r > 3e-6
                rs = torch.where(mask, r, torch.ones_like(r))
                r6 = torch.where(mask, self.w[1] ** 6 / rs ** 6, torch.zeros_like(r))
                return htf.compute_nlist_forces(nlist, torch.sum(self.w[0] * 4.0 * (r6 ** 2 - r6) / 2.0, dim=1))
        return M(96, output_forces=False)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("twin", ["device", "torch"])
def test_recompiling_changes_the_optimizer(htf, cuda, monkeypatch, route, twin):
    """model.compile() after training has started: the next step uses the NEW optimizer -- SGD(learning_rate=0) freezes the
    weights bit for bit, SGD(lr) makes one step theta - lr * g with g = d MSE / d theta of that step (fp64 double backward on
    its pair vectors and labels) -- on the device-optimizer route and on the torch-twin route alike."""
    if twin == "torch":
        monkeypatch.setenv("HTF_NO_JIT", "1")
    sysm, sim, nl = _sim(cuda, 1, dt=0.0)       # (dt = 0: the pair vectors and labels after a run are the next step's)
    lj = htf.tfcompute(build_examples.LJModel(96))
    lj.attach(nl, r_cut=2.5)
    if twin == "torch":
        model = _TorchLJParam.make(htf, 0.8, 1.05)
        weights = lambda: model.w
    else:
        model = build_examples.TrainableGraph(96, output_forces=False, sig=0.8, eps=1.05)
        weights = lambda: model.lj.w
    model.compile(htf.optimizers.Adam(0.01), loss='MeanSquaredError')
    tfc = htf.tfcompute(model)
    tfc.attach(nl, train=True, r_cut=2.5)
    tfc.set_reference_forces(lj)
    sim.run(10, graph=route)
    if twin == "torch":
        assert tfc._tplan is None and tfc._torch_opt is not None
    else:
        assert tfc._tplan is not None
    model.compile(htf.optimizers.SGD(learning_rate=0.0), loss='MeanSquaredError')
    w0 = weights().detach().clone()
    sim.run(STEPS if route is None else 20, graph=route)
    torch.cuda.synchronize()
    assert torch.equal(weights().detach(), w0), "compile(SGD(0)): the first optimizer kept training"
    # one SGD step against the fp64 gradient of this very step
    N = sysm.N
    nl64 = tfc.get_nlist_array().reshape(N, 96, 4)
    labels = lj.force.double().cpu()
    theta = [float(v) for v in w0.cpu().numpy()]
    _, g = G.mse_grad_wrt_params(lambda n, ww: G.lj_param_forces(n, ww, create_graph=True), torch.from_numpy(nl64), labels, theta)
    lr = 1e-2 / float(np.abs(g).max())
    model.compile(htf.optimizers.SGD(learning_rate=lr), loss='MeanSquaredError')
    sim.run(1, graph=route)
    torch.cuda.synchronize()
    w1 = weights().detach().cpu().numpy().astype(np.float64)
    step = (np.asarray(theta) - w1) / lr
    # test_lj_param_forward_and_loss_gradient's rtol; the atol is the fp32 rounding of the stored weights (~1e-7 / lr)
    np.testing.assert_allclose(step, g, rtol=1e-3, atol=1e-4 * float(np.abs(g).max()))
