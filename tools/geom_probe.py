"""Times the molecular geometry ops (csrc/mol_geom.hip) against the same computation written as plain torch ops + autograd.

CG mode: a polymer melt of --chains chains of --length beads (131 072 beads, ~130 k bonds, angles and dihedrals by default)
in a periodic box at one bead per unit volume, index arrays as device tensors.  Molecule mode: --molecules molecules of
MN = 8 rows (MolSimModel's [M, MN, 4]), slots (1, 2, 3, 4).  Forward and backward (autograd.grad with a random upstream
gradient) per op; device events around --iters calls per window, the median of --windows windows; one JSON line.

    python tools/geom_probe.py [--chains 1024] [--length 128] [--molecules 16384] [--iters 20] [--windows 7]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hoomd_tf_amd as htf  # noqa: E402

OPS = {2: ("bond", htf.mol_bond_distance), 3: ("angle", htf.mol_angle), 4: ("dihedral", htf.mol_dihedral)}


def timed(fn, iters, windows):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return float(np.median(out))


def torch_geom(P, L):
    """The op's definitions in torch ops on [T, K, 3] points (the route a user writes without these ops)."""
    K = P.shape[1]

    def mi(d):
        return d - torch.round(d / L) * L

    if K == 2:
        return torch.linalg.norm(mi(P[:, 1] - P[:, 0]), dim=-1)
    if K == 3:
        a, b = mi(P[:, 0] - P[:, 1]), mi(P[:, 2] - P[:, 1])
        return torch.atan2(torch.linalg.norm(torch.cross(a, b, dim=-1), dim=-1), (a * b).sum(-1))
    b1, b2, b3 = mi(P[:, 1] - P[:, 0]), mi(P[:, 2] - P[:, 1]), mi(P[:, 3] - P[:, 2])
    n1, n2 = torch.cross(b1, b2, dim=-1), torch.cross(b2, b3, dim=-1)
    return torch.atan2(torch.linalg.norm(b2, dim=-1) * (b1 * n2).sum(-1), (n1 * n2).sum(-1)).abs()


def melt(n_chain, n_per, L, rng):
    p = np.zeros((n_chain, n_per, 3))
    p[:, 0] = rng.uniform(-L / 2, L / 2, (n_chain, 3))
    for i in range(1, n_per):
        u = rng.normal(size=(n_chain, 3))
        p[:, i] = p[:, i - 1] + u / np.linalg.norm(u, axis=1, keepdims=True)
    return (p - np.round(p / L) * L).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1024)
    ap.add_argument("--length", type=int, default=128)
    ap.add_argument("--molecules", type=int, default=16384)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("geom_probe: needs a GPU")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(1)
    B = a.chains * a.length
    L = float(B) ** (1.0 / 3.0)
    box = torch.tensor([[-L / 2] * 3, [L / 2] * 3, [0.0] * 3], device=dev)
    Lt = torch.tensor([L] * 3, device=dev)
    flat = melt(a.chains, a.length, L, rng).reshape(-1, 3)
    x = torch.from_numpy(np.concatenate([flat, np.zeros((B, 1), np.float32)], 1)).to(dev).requires_grad_(True)
    res = {"beads": B, "chains": a.chains, "length": a.length, "box": round(L, 4), "molecules": a.molecules, "MN": 8}
    for K, (name, op) in OPS.items():
        base = (np.arange(a.chains)[:, None] * a.length + np.arange(a.length - K + 1)[None, :]).reshape(-1)
        idx = [torch.from_numpy(base + s).to(dev) for s in range(K)]
        kw = {"b%d" % (s + 1): idx[s] for s in range(K)}
        T = len(base)
        res["cg_%s_terms" % name] = T
        fused = op(CG=True, cg_positions=x, box=box, **kw)
        ref = torch_geom(torch.stack([x[i, :3] for i in idx], 1), Lt)
        res["cg_%s_max_abs_diff" % name] = float((fused - ref).detach().abs().max())
        g = torch.randn_like(fused)
        with torch.no_grad():
            res["cg_%s_fwd_ms" % name] = round(timed(lambda: op(CG=True, cg_positions=x, box=box, **kw), a.iters, a.windows), 4)
            res["cg_%s_torch_fwd_ms" % name] = round(
                timed(lambda: torch_geom(torch.stack([x[i, :3] for i in idx], 1), Lt), a.iters, a.windows), 4)
        res["cg_%s_bwd_ms" % name] = round(
            timed(lambda: torch.autograd.grad(fused, x, g, retain_graph=True), a.iters, a.windows), 4)
        res["cg_%s_torch_bwd_ms" % name] = round(
            timed(lambda: torch.autograd.grad(ref, x, g, retain_graph=True), a.iters, a.windows), 4)

    # molecule mode: MolSimModel's [M, MN, 4], slots 1..4 (build_examples.MolFeatureModel)
    M, MN = a.molecules, 8
    Lm = float(M * MN) ** (1.0 / 3.0)
    boxm = torch.tensor([[-Lm / 2] * 3, [Lm / 2] * 3, [0.0] * 3], device=dev)
    Lmt = torch.tensor([Lm] * 3, device=dev)
    mp = melt(M, MN, Lm, rng)
    mol = torch.from_numpy(np.concatenate([mp, np.zeros((M, MN, 1), np.float32)], 2)).to(dev).requires_grad_(True)
    for K, (name, op) in OPS.items():
        slots = list(range(1, K + 1))
        fused = op(mol, *slots, box=boxm)
        ref = torch_geom(mol[:, slots, :3], Lmt)
        res["mol_%s_max_abs_diff" % name] = float((fused - ref).detach().abs().max())
        g = torch.randn_like(fused)
        with torch.no_grad():
            res["mol_%s_fwd_ms" % name] = round(timed(lambda: op(mol, *slots, box=boxm), a.iters, a.windows), 4)
            res["mol_%s_torch_fwd_ms" % name] = round(timed(lambda: torch_geom(mol[:, slots, :3], Lmt), a.iters, a.windows), 4)
        res["mol_%s_bwd_ms" % name] = round(
            timed(lambda: torch.autograd.grad(fused, mol, g, retain_graph=True), a.iters, a.windows), 4)
        res["mol_%s_torch_bwd_ms" % name] = round(
            timed(lambda: torch.autograd.grad(ref, mol, g, retain_graph=True), a.iters, a.windows), 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
