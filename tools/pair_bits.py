#!/usr/bin/env python3
"""The output bits of the pair path's entries -- the streaming evaluators (htf_eval_forces, htf_eval_forces2), the one-kernel
steps (htf_fused_forces / htf_build_eval_forces, htf_build_eval_forces2, and htf_compute_forces with a step epilogue at levels 1
and 2), the pair-MLP (evaluation and both training sweeps), the top-k network, htf_train_pair_grad and its list form,
htf_build_pair_vectors / htf_cf_pair_index, and one traced (generated) energy through the fused step, the evaluator and both
training sweeps -- on small seeded inputs, as SHA-256 of every output buffer's bytes: what a change to the host side of these
launches must leave unchanged.  A call the library refuses is recorded by its error text.  Public functions only.

    python tools/pair_bits.py OUT.json                   (the library the package loads; HTF_AMD_LIB selects another build)
    python tools/pair_bits.py --compare A.json B.json    (exit 1 and the differing outputs if any hash differs)

Run once per library, each in a fresh process.  The cases reach every branch a launch chooses at the smallest shapes that do:
B = 37 rows (more than one block, no multiple of a block's rows) at NN = 8 / 64 / 128 (4, 8, 16 lanes per row); every closed form;
both scalar types of the tensor and of the positions; virial on and off; the tensor stored or not; N = 300 at NN = 16 from an
all-pairs list, and a jittered 32 x 32 x 48 cubic lattice (six neighbors in rows of NN = 8) at batches of 16 383, 16 384, 49 151 and
49 152 rows, the edges of the plain two-row, the merged two-row and the merged four-row form; NN = 16 and 160 for the two-potential
step (compacting / in place); pair-MLP rows of NN = 32, 64, 128 (1, 2, 4 fused tiles) and 96 (not fused).  No output depends on the
order of atomics: the histogram's are integer counts."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import brute_nlist, random_nlist  # noqa: E402

B = 37
F32, F64 = torch.float32, torch.float64
DT = {F32: "f32", F64: "f64"}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def record(cases, name, fn):
    """cases[name] = {output: sha} of the tensors fn returns, or the text of the error the library answered with."""
    try:
        out = fn()
        torch.cuda.synchronize()
        cases[name] = {k: sha(v) for k, v in out.items()}
    except (RuntimeError, ValueError) as e:
        cases[name] = {"error": str(e)}


def record_eval(cases, name, ops, pot, x):
    """The streaming evaluator without and with the virial, each recorded on its own (SimplePotential has no virial)."""
    record(cases, name, lambda: {"f": ops.eval_forces(pot, x)})
    record(cases, name + "_virial", lambda: dict(zip(("f", "v"), ops.eval_forces(pot, x, virial=True))))


def closed_forms(htf, dev):
    return {"lj": htf.Potential.lj(), "wca": htf.Potential.wca(1.1), "poly": htf.Potential.rinv_poly([4.0, -4.0, 0.3], [12, 6, 2], cut=2.4),
            "simple": htf.Potential.simple(), "gauss": htf.Potential.gauss(1.4, 0.3, 0.8), "lj_param": htf.Potential.lj_param(0.9, 1.05)}


def trainable(htf, dev):
    th = lambda *v: torch.tensor(v, dtype=F32, device=dev)   # noqa: E731
    return {"lj_param": htf.Potential.lj_param(0.9, 1.05, theta=th(0.9, 1.05)), "wca": htf.Potential.wca(1.1, theta=th(1.1)),
            "poly": htf.Potential.rinv_poly([4.0, -4.0, 0.3], [12, 6, 2], theta=th(4.0, -4.0, 0.3))}


def tensor(seed, rows, NN, dtype, dev, **kw):
    nl, _ = random_nlist(np.random.default_rng(seed), rows, NN, dtype=np.float64, **kw)
    return torch.from_numpy(nl).to(dtype).to(dev)


def liquid(seed, N, L, r_cut, dev):
    """N seeded points in a periodic cube and their all-pairs list (shuffled rows), as device arrays."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-L / 2, L / 2, (N, 3))
    n_neigh, head, flat = brute_nlist(pos, [L] * 3, r_cut, shuffle_seed=seed)
    pos4 = np.concatenate([pos, rng.integers(0, 2, (N, 1)).astype(np.float64)], axis=1)
    as_i32 = lambda a: torch.from_numpy(a.astype(np.int64)).to(torch.int32).to(dev)   # noqa: E731
    return torch.from_numpy(pos4).to(dev), as_i32(n_neigh), as_i32(head), as_i32(np.concatenate([flat, [0]])), [[-L / 2] * 3, [L / 2] * 3, [0.0] * 3]


def lattice(dev, n=(32, 32, 48), a=1.0, jitter=0.03):
    """A jittered cubic lattice and the list of each site's six lattice neighbors, pitch 6."""
    rng = np.random.default_rng(11)
    ijk = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), -1).reshape(-1, 3)
    L = np.asarray(n, dtype=np.float64) * a
    pos = (ijk + 0.5) * a - L / 2 + jitter * a * rng.standard_normal(ijk.shape)
    idx = lambda q: (q[:, 0] % n[0]) * n[1] * n[2] + (q[:, 1] % n[1]) * n[2] + q[:, 2] % n[2]   # noqa: E731
    steps = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    flat = np.stack([idx(ijk + np.asarray(s)) for s in steps], axis=1).reshape(-1)
    N = len(ijk)
    pos4 = np.concatenate([pos, np.zeros((N, 1))], axis=1)
    as_i32 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int64)).to(torch.int32).to(dev)   # noqa: E731
    return torch.from_numpy(pos4).to(F32).to(dev), as_i32(np.full(N, 6)), as_i32(np.arange(N) * 6), as_i32(flat), [list(-L / 2), list(L / 2), [0.0] * 3]


def eval_cases(htf, dev, cases):
    ops = htf.ops
    pots = closed_forms(htf, dev)
    for NN in (8, 64, 128):
        for dtype in (F32, F64):
            x = tensor(100 + NN, B, NN, dtype, dev)
            for kind, pot in pots.items():
                record_eval(cases, "eval_%s_NN%d_%s" % (kind, NN, DT[dtype]), ops, pot, x)
    record(cases, "eval2_second_not_gauss", lambda: {"f": ops.eval_forces2(pots["lj"], pots["lj"], tensor(1, B, 8, F32, dev))[0]})
    record(cases, "nlist_rinv_check_nlist", lambda: {"rinv32": ops.nlist_rinv(tensor(3, B, 24, F32, dev)), "rinv64": ops.nlist_rinv(tensor(3, B, 24, F64, dev)),
                                                    "check32": torch.tensor(ops.check_nlist(tensor(3, B, 24, F32, dev))), "check64": torch.tensor(ops.check_nlist(tensor(3, B, 24, F64, dev)))})
    for kind in ("lj", "wca", "poly", "lj_param"):
        for dtype in (F32, F64):
            for NN in (16, 64):
                x = tensor(200 + NN, B, NN, dtype, dev)
                for with_rdf in (False, True):
                    def two(kind=kind, x=x, NN=NN, with_rdf=with_rdf):
                        hist = torch.zeros(34, dtype=torch.int32, device=dev)
                        part = torch.zeros(ops.num_partials(B, NN), dtype=F32, device=dev)
                        fa, fb = ops.eval_forces2(pots[kind], pots["gauss"], x, partials=part, rdf=(0.5, 3.0, hist) if with_rdf else None)
                        return {"fa": fa, "fb": fb, "partials": part, "hist": hist}
                    record(cases, "eval2_%s_NN%d_%s%s" % (kind, NN, DT[dtype], "_rdf" if with_rdf else ""), two)


def fused_cases(htf, dev, cases):
    ops = htf.ops
    pots = closed_forms(htf, dev)
    N, NN, rc = 300, 16, 1.2
    pos64, n_neigh, head, flat, box = liquid(7, N, 7.0, rc, dev)
    for kind, pot in pots.items():
        for dtype in (F32, F64):
            pos = pos64.to(dtype)
            for store in (False, True):
                for virial in (False, True):
                    if kind not in ("lj", "gauss") and (dtype == F64 or store):
                        continue   # (the other kinds: once per virial switch)
                    def one(pot=pot, pos=pos, store=store, virial=virial):
                        pv = torch.full((N, NN, 4), -1.0, dtype=F32, device=dev) if store else None
                        r = ops.fused_forces(pot, pos, n_neigh, head, flat, box, rc, NN, virial=virial, pair_vectors=pv)
                        out = {"f": r[0], "v": r[1]} if virial else {"f": r}
                        if store:
                            out["pair_vectors"] = pv
                        return out
                    record(cases, "fused_%s_%s%s%s" % (kind, DT[dtype], "_store" if store else "", "_virial" if virial else ""), one)
    from hoomd_tf_amd.initializers import mlp_params
    mlp = htf.Potential.pair_mlp(mlp_params(seed=3), 0.0, 3.0)
    record(cases, "fused_no_fused_form", lambda: {"f": ops.fused_forces(mlp, pos64.to(F32), n_neigh, head, flat, box, rc, NN)})
    # an offset batch, and the two-potential step
    record(cases, "fused_lj_offset", lambda: {"f": ops.fused_forces(pots["lj"], pos64.to(F32), n_neigh, head, flat, box, rc, NN, offset=101, batch_size=150)})
    for kind in ("lj", "wca", "poly", "lj_param", "gauss"):
        for dtype in (F32, F64):
            for nn2 in (16, 160):
                for store in (False, True):
                    def two(kind=kind, dtype=dtype, nn2=nn2, store=store):
                        hist = torch.zeros(34, dtype=torch.int32, device=dev)
                        part = torch.zeros(ops.num_partials_fused(N), dtype=F32, device=dev)
                        pv = torch.full((N, nn2, 4), -1.0, dtype=F32, device=dev) if store else None
                        fa, fb = ops.build_eval_forces2(pots[kind], pots["gauss"], pos64.to(dtype), n_neigh, head, flat, box, rc, nn2, partials=part,
                                                        rdf=(0.2, 1.3, hist), pair_vectors=pv)
                        out = {"fa": fa, "fb": fb, "partials": part, "hist": hist}
                        if store:
                            out["pair_vectors"] = pv
                        return out
                    record(cases, "fused2_%s_NN%d_%s%s" % (kind, nn2, DT[dtype], "_store" if store else ""), two)
    # the three forms of the step and both edges of each, on the lattice
    lpos, ln, lh, lf, lbox = lattice(dev)
    for batch in (16383, 16384, 49151, 49152):
        for kind in ("lj", "wca", "gauss"):
            for store in (False, True):
                def form(batch=batch, kind=kind, store=store):
                    pv = torch.full((batch, 8, 4), -1.0, dtype=F32, device=dev) if store else None
                    out = {"f": ops.fused_forces(pots[kind], lpos, ln, lh, lf, lbox, 1.3, 8, batch_size=batch, pair_vectors=pv)}
                    if store:
                        out["pair_vectors"] = pv
                    return out
                record(cases, "fused_%s_batch%d%s" % (kind, batch, "_store" if store else ""), form)
    record(cases, "fused_lj_f64_batch49152", lambda: {"f": ops.fused_forces(pots["lj"], lpos.to(F64), ln, lh, lf, lbox, 1.3, 8)})
    # build_pair_vectors / cf_pair_index: every pair of scalar types
    for pd in (F32, F64):
        for dd in (F32, F64):
            record(cases, "build_pair_vectors_%s_to_%s" % (DT[pd], DT[dd]),
                   lambda pd=pd, dd=dd: {"pair_vectors": ops.build_pair_vectors(pos64.to(pd), n_neigh, head, flat, box, rc, NN, out_dtype=dd)})
        record(cases, "pair_index_%s" % DT[pd], lambda pd=pd: {"index": ops.build_pair_index(pos64.to(pd), n_neigh, head, flat, box, rc, NN)})


def epilogue_cases(htf, dev, cases):
    """htf_compute_forces with a registered step epilogue: the integrator alone (level 1, FusedStep on one domain) and with a brick's
    halo messages (level 2, the same step under a replica BrickDomain), six steps each, no rebuild between them."""
    from hoomd_tf_amd import standin
    from hoomd_tf_amd.brick import BrickDomain
    pos, L, a = standin.fcc_positions(6, 0.8442)
    pos = pos + 0.03 * a * np.random.default_rng(21).standard_normal(pos.shape)
    pos -= np.round(pos / L) * L

    def run(brick):
        if brick:
            grid = np.asarray((2, 1, 1))
            Lg = np.asarray(L) * grid
            lo = -Lg / 2 + (grid // 2) * np.asarray(L)
            sysm = standin.System(pos + np.asarray(L) / 2 + lo, Lg, types=np.arange(len(pos)), dtype=F32, device=dev)
        else:
            sysm = standin.System(pos, L, dtype=F32, device=dev)
        sysm.randomize_velocities(kT=1.2, seed=5)
        nl = standin.CellNlist(sysm, r_cut=2.5, r_buff=0.4, check_period=50, device_decision=True)
        if brick:
            nl.domain = BrickDomain(sysm, 0, tuple(grid), r_ghost=2.9, r_buff=0.4, replica=True, transport="local")
        nl.build()
        ctx = htf.Context(r_cut=2.5, nneighs=96, scalar_dtype=F32, max_n=sysm.N, fused=2)
        ctx.set_potential(htf.Potential.lj())
        fs = standin.FusedStep(sysm, nl, ctx, standin.NVE(sysm, 0.004))
        if not fs.available:
            raise RuntimeError("the step epilogue was declined")
        for ts in range(6):
            fs.step(ts)
        torch.cuda.synchronize()
        rows = nl.domain.live_rows() if brick else slice(0, sysm.N)
        return {"pos": sysm.pos[rows], "vel": sysm.vel[rows], "force": sysm.force[rows]}
    record(cases, "step_epilogue_level1", lambda: run(False))
    record(cases, "step_epilogue_level2", lambda: run(True))


def mlp_cases(htf, dev, cases):
    from hoomd_tf_amd.initializers import mlp_params
    ops = htf.ops
    params = mlp_params(seed=3, bias_scale=0.1)
    flat = np.concatenate([np.asarray(params[k], dtype=np.float32).ravel() for k in ("W1", "b1", "W2", "b2", "W3", "b3")])
    for prec in ("fp32", "bf16", "split", "split16"):
        for act in ("tanh", "linear"):
            pot = htf.Potential.pair_mlp(params, 0.0, 3.0, activation=act, precision=prec)
            for dtype in (F32, F64):
                x = tensor(300, B, 32, dtype, dev)
                record_eval(cases, "mlp_%s_%s_%s" % (prec, act, DT[dtype]), ops, pot, x)
    for prec in ("split16", "fp32"):
        for act in ("tanh", "linear"):
            for NN in (32, 64, 96, 128):
                for dtype in (F32, F64):
                    if dtype == F64 and NN not in (32, 96):
                        continue
                    def sweep(prec=prec, act=act, NN=NN, dtype=dtype):
                        theta = torch.tensor(flat, device=dev)
                        pot = htf.Potential.pair_mlp(params, 0.0, 3.0, activation=act, precision=prec, theta=theta)
                        x = tensor(400 + NN, B, NN, dtype, dev)
                        labels = 0.05 * ops.eval_forces(htf.Potential.lj(), x, out_dtype=F32)
                        pred = torch.zeros((B, 4), dtype=F32, device=dev)
                        return {"accum": ops.train_pair_grad(pot, x, labels, pred=pred), "pred": pred, "accum_nopred": ops.train_pair_grad(pot, x, labels)}
                    record(cases, "mlp_train_%s_%s_NN%d_%s" % (prec, act, NN, DT[dtype]), sweep)
    rng = np.random.default_rng(9)
    K, H = 8, 16
    tk = {"W1": rng.normal(0, 0.4, (K, H)), "b1": rng.normal(0, 0.1, H), "W2": rng.normal(0, 0.3, (H, H)), "b2": rng.normal(0, 0.1, H),
          "W3": rng.normal(0, 0.3, (H, 1)), "b3": rng.normal(0, 0.1, 1)}
    tk = {k: v.astype(np.float32) for k, v in tk.items()}
    for act in ("tanh", None):
        pot = htf.Potential.topk_mlp(tk, activation=act)
        for dtype in (F32, F64):
            x = tensor(500, B, 64, dtype, dev)
            record_eval(cases, "topk_%s_%s" % (act or "linear", DT[dtype]), ops, pot, x)


def train_cases(htf, dev, cases):
    ops = htf.ops
    N, NN, rc = 300, 16, 1.2
    pos64, n_neigh, head, flat, box = liquid(7, N, 7.0, rc, dev)
    pots = dict(trainable(htf, dev), gauss=htf.Potential.gauss(1.4, 0.3, 0.8))
    for kind, pot in pots.items():
        for dtype in (F32, F64):
            def sweep(pot=pot, dtype=dtype):
                x = tensor(600, B, 24, dtype, dev, rmin=0.9)
                labels = 0.05 * ops.eval_forces(htf.Potential.lj(), x)
                pred = torch.zeros((B, 4), dtype=F32, device=dev)
                return {"accum": ops.train_pair_grad(pot, x, labels, pred=pred), "pred": pred}
            record(cases, "train_%s_%s" % (kind, DT[dtype]), sweep)

            def sweep_list(pot=pot, dtype=dtype):
                pos = pos64.to(dtype)
                labels = 0.05 * ops.fused_forces(htf.Potential.lj(), pos, n_neigh, head, flat, box, rc, NN)
                pred = torch.zeros((N, 4), dtype=F32, device=dev)
                return {"accum": ops.train_pair_grad_list(pot, pos, n_neigh, head, flat, box, rc, NN, labels, pred=pred), "pred": pred}
            record(cases, "train_list_%s_%s" % (kind, DT[dtype]), sweep_list)


def traced_cases(htf, dev, cases):
    """One traced energy with weights (a Morse form) as generated kernels: the fused step at the sizes of its two forms and with a
    virial, the evaluator, and both training sweeps."""
    from test_codegen_cpu import _weighted_models
    ops = htf.ops
    x = tensor(700, B, 24, F32, dev, rmin=0.9)
    w = torch.nn.Parameter(torch.tensor([1.1, 0.95], device=dev))
    a = torch.nn.Parameter(torch.tensor(0.7, device=dev))
    b = torch.nn.Parameter(torch.tensor(2.3, device=dev))
    pot = _weighted_models(htf, htf.Nlist(x), w, a, b)["morse"].layer.potential(dev)
    N, NN, rc = 300, 16, 1.2
    pos64, n_neigh, head, flat, box = liquid(7, N, 7.0, rc, dev)
    for dtype in (F32, F64):
        xd = x.to(dtype)
        labels = 0.05 * ops.eval_forces(htf.Potential.lj(), xd)
        record_eval(cases, "traced_eval_%s" % DT[dtype], ops, pot, xd)
        record(cases, "traced_train_%s" % DT[dtype], lambda xd=xd, labels=labels: {"accum": ops.train_pair_grad(pot, xd, labels)})
        pos = pos64.to(dtype)

        def fused(pos=pos):
            f, v = ops.fused_forces(pot, pos, n_neigh, head, flat, box, rc, NN, virial=True)
            pv = torch.full((N, NN, 4), -1.0, dtype=F32, device=dev)
            return {"f": ops.fused_forces(pot, pos, n_neigh, head, flat, box, rc, NN), "virial.f": f, "virial.v": v,
                    "store.f": ops.fused_forces(pot, pos, n_neigh, head, flat, box, rc, NN, pair_vectors=pv), "pair_vectors": pv}
        record(cases, "traced_fused_%s" % DT[dtype], fused)
        llabels = 0.05 * ops.fused_forces(htf.Potential.lj(), pos, n_neigh, head, flat, box, rc, NN)
        record(cases, "traced_train_list_%s" % DT[dtype],
               lambda pos=pos, llabels=llabels: {"accum": ops.train_pair_grad_list(pot, pos, n_neigh, head, flat, box, rc, NN, llabels)})
    lpos, ln, lh, lf, lbox = lattice(dev)
    for batch in (49151, 49152):
        record(cases, "traced_fused_batch%d" % batch, lambda batch=batch: {"f": ops.fused_forces(pot, lpos, ln, lh, lf, lbox, 1.3, 8, batch_size=batch)})


def compare(a, b):
    A, Bb = (json.load(open(p))["cases"] for p in (a, b))
    bad = [(c, o) for c in sorted(set(A) | set(Bb)) for o in sorted(set(A.get(c, {})) | set(Bb.get(c, {})))
           if A.get(c, {}).get(o) != Bb.get(c, {}).get(o)]
    n = sum(len(v) for v in A.values())
    for c, o in bad:
        print("differs: %s  %s" % (c, o))
    print("%d outputs of %d cases: %s" % (n, len(A), "%d differ" % len(bad) if bad else "every hash equal"))
    return 1 if bad else 0


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        return compare(sys.argv[2], sys.argv[3])
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    import hoomd_tf_amd as htf
    from hoomd_tf_amd import _lib
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    cases = {}
    for family in (eval_cases, fused_cases, epilogue_cases, mlp_cases, train_cases, traced_cases):
        family(htf, dev, cases)
    errors = sorted(c for c, v in cases.items() if "error" in v)
    with open(sys.argv[1], "w") as f:
        json.dump({"lib": _lib.LIB_PATH, "binding": _lib.BINDING, "cases": cases}, f, indent=1, sort_keys=True)
    print("%d outputs of %d cases (%d answered with an error: %s) -> %s (%s)" % (
        sum(len(v) for v in cases.values()), len(cases), len(errors), ", ".join(errors) or "-", sys.argv[1], _lib.LIB_PATH))
    return 0


if __name__ == "__main__":
    sys.exit(main())
