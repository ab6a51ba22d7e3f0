#!/usr/bin/env python3
"""The output bits of the descriptor network's eight entries -- forces (with and without virial), descriptor, loss_gradient,
total_forces (with and without virial), total_loss_gradient, angular_loss_gradient, the angular descriptor -- on small seeded
inputs, as SHA-256 of every output tensor's bytes: what a refactor of the family's kernels must leave unchanged.  Likewise the
ghost-row forms of total_forces and the two sweeps on the forces of the total energy, and the committee's total_forces (mean,
virial, deviation, members) and committee_loss_gradient.  Public methods only: the script runs on any commit that has them.

    python tools/desc_bits.py OUT.json                   (the library the package loads; HTF_AMD_LIB selects another build)
    python tools/desc_bits.py --compare A.json B.json    (exit 1 and the differing outputs if any hash differs)

Run once per library, each in a fresh process.  B = 67 rows (more than one block, not a multiple of the four waves); every
value of NN in {1, 64, 65, 256}, (K, n_types, l_max), (H1, H2) in {(1, 1), (32, 24), (64, 33)}, tanh / linear, r_cut None / 1.5,
fp32 / fp64 pair vectors and n_species 1 / 2 (once with a species absent) meets every kernel at least once, and one setting per
family carries slots with index -1 and B, NaN types and a row whose own type is out of range.  The ghost settings (l_max 0 and 2,
NN 1 and 65) add 9 ghost rows that ``halo`` fills from a seeded tensor, with slots that name ghosts, -1 and B + 9.  The
committees: D, H <= 32 with M = 8 and M = 3 (two members per wave), and K n_types = 48, H = 33 x 64 (one member per wave) with
M = 3 and with M = 5, whose sweeps take more than 64 KiB of dynamic LDS and so have the kernels' limit raised; with and without
r_cut, fp32 and fp64 pair vectors, and one committee of two species with one absent."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import random_nlist  # noqa: E402

B = 67
F32, F64 = torch.float32, torch.float64
#            NN   K  T  l  H1  H2  activation r_cut dtype S  absent dirty
SETTINGS = [(1,   4, 1, 0, 1,  1,  "tanh",    None, F32, 1, False, False),
            (64,  5, 3, 0, 32, 24, "linear",  1.5,  F64, 2, False, False),
            (65,  64, 1, 0, 64, 33, "tanh",   1.5,  F32, 1, False, False),
            (256, 5, 3, 0, 64, 33, "linear",  None, F64, 1, False, False),
            (65,  4, 1, 0, 32, 24, "tanh",    None, F64, 2, True,  False),
            (256, 64, 1, 0, 1, 1,  "linear",  1.5,  F32, 2, False, False),
            (65,  5, 3, 0, 32, 24, "tanh",    1.5,  F32, 1, False, True),
            (1,   8, 2, 1, 1,  1,  "tanh",    None, F32, 1, False, False),
            (64,  32, 1, 1, 32, 24, "linear", 1.5,  F64, 2, False, False),
            (65,  7, 3, 2, 64, 33, "tanh",    1.5,  F32, 1, False, False),
            (256, 21, 1, 2, 32, 24, "linear", None, F64, 2, True,  False),
            (256, 8, 2, 1, 64, 33, "tanh",    None, F32, 1, False, False),
            (1,   7, 3, 2, 1,  1,  "linear",  None, F32, 1, False, False),
            (65,  8, 2, 1, 64, 33, "tanh",    1.5,  F32, 1, False, True),
            (64,  7, 3, 2, 32, 24, "linear",  1.5,  F64, 1, False, True)]

GHOST = 9
#                  NN  K  T  l  H1  H2  activation r_cut dtype S
GHOST_SETTINGS = [(1,  4, 1, 0, 32, 24, "tanh",    None, F32, 1),
                  (65, 5, 3, 0, 64, 33, "linear",  1.5,  F64, 2),
                  (1,  7, 3, 2, 1,  1,  "linear",  1.5,  F64, 1),
                  (65, 7, 3, 2, 32, 24, "tanh",    None, F32, 2)]
#                      M  NN  K   T  H1  H2  activation r_cut dtype S  absent
COMMITTEE_SETTINGS = [(8, 64, 8,  1, 16, 16, "tanh",    None, F32, 1, False),
                      (3, 65, 8,  1, 16, 16, "linear",  1.5,  F64, 1, False),
                      (3, 1,  8,  1, 16, 16, "tanh",    None, F32, 2, True),
                      (3, 65, 16, 3, 33, 64, "tanh",    1.5,  F32, 1, False),
                      (5, 64, 16, 3, 33, 64, "tanh",    None, F64, 2, False)]


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_setting(htf, dev, n, s):
    NN, K, T, l_max, H1, H2, act, r_cut, dtype, S, absent, dirty = s
    torch.manual_seed(1000 + n)
    rng = np.random.default_rng(1000 + n)
    lay = htf.DescriptorMLP(K=K, H1=H1, H2=H2, low=0.5, high=1.8, n_types=T, activation=act, seed=3 + n, r_cut=r_cut,
                            n_species=S, conservative=bool(l_max), l_max=l_max, device=dev)
    w = (lay.w.cpu() + 0.1 * torch.randn(lay.w.numel())).view(S, lay.P)   # (nonzero biases)
    w[:, :lay.D * H1] *= 1.0 / 16.0        # W1: keeps tanh off saturation at 190 neighbors
    if l_max == 2:
        w[:, 2 * lay.Dr * H1:lay.D * H1] *= 1.0 / 64.0   # (the rows of Q = ||M||_F^2, about G^2 / 3)
    lay.w.copy_(w.reshape(-1))
    nl, _ = random_nlist(rng, B, NN, fill=0.75, rmin=0.3, rmax=2.0, ntypes=T, dtype=np.float64)
    index = torch.randint(0, B, (B, NN), dtype=torch.int32)
    own = torch.randint(0, T, (B,)).to(torch.float32)
    species = torch.ones(B) if absent else torch.randint(0, S, (B,)).to(torch.float32)
    labels = 0.05 * torch.randn(B, 4, dtype=torch.float64)
    if dirty:
        m = min(NN, 6)
        index[2, :m] = torch.tensor([-1, B, -7, B + 5, 0, B - 1], dtype=torch.int32)[:m]
        nl[3, :m, 3] = [np.nan, 0, np.nan, T, -1, np.nan][:m]
        own[5] = float(T)
        own[6] = -1.0
    x = torch.from_numpy(nl).to(dtype).to(dev)
    index, own, species, labels = index.to(dev), own.to(dev), species.to(dev), labels.to(dtype).to(dev)
    sp = species if S > 1 else None
    ty = own if T > 1 else None
    out = {}
    if not l_max:
        f, v = lay.forces(x, virial=True, species=sp)
        out["forces+virial.f"], out["forces+virial.v"] = sha(f), sha(v)
        out["forces"] = sha(lay.forces(x, species=sp))
        out["loss_gradient"] = sha(lay.loss_gradient(x, labels, species=sp))
    out["descriptor"] = sha(lay.descriptor(x))
    f, v = lay.total_forces(x, index, virial=True, types=ty, species=sp)
    out["total_forces+virial.f"], out["total_forces+virial.v"] = sha(f), sha(v)
    out["total_forces"] = sha(lay.total_forces(x, index, types=ty, species=sp))
    sweep = lay.angular_loss_gradient if l_max else lay.total_loss_gradient
    out["angular_loss_gradient" if l_max else "total_loss_gradient"] = sha(sweep(x, labels, index, types=ty, species=sp))
    torch.cuda.synchronize()
    return out


def seeded(n, lay, NN, T, S, absent, dtype, dev, n_table=B):
    """The seeded weights and inputs of a setting: ``lay.w`` in place; (x, index in [0, n_table), types, species, labels)."""
    torch.manual_seed(1000 + n)
    rng = np.random.default_rng(1000 + n)
    w = (lay.w.cpu() + 0.1 * torch.randn(lay.w.numel())).view(-1, lay.P)   # (nonzero biases)
    w[:, :lay.D * lay.H1] *= 1.0 / 16.0        # W1: keeps tanh off saturation at 190 neighbors
    if lay.l_max == 2:
        w[:, 2 * lay.Dr * lay.H1:lay.D * lay.H1] *= 1.0 / 64.0   # (the rows of Q = ||M||_F^2, about G^2 / 3)
    lay.w.copy_(w.reshape(-1))
    nl, _ = random_nlist(rng, B, NN, fill=0.75, rmin=0.3, rmax=2.0, ntypes=T, dtype=np.float64)
    index = torch.randint(0, n_table, (B, NN), dtype=torch.int32)
    own = torch.randint(0, T, (B,)).to(torch.float32)
    species = torch.ones(B) if absent else torch.randint(0, S, (B,)).to(torch.float32)
    labels = 0.05 * torch.randn(B, 4, dtype=torch.float64)
    return torch.from_numpy(nl).to(dtype).to(dev), index, own if T > 1 else None, species.to(dev) if S > 1 else None, labels.to(dtype).to(dev)


def run_ghost(htf, dev, n, s):
    NN, K, T, l_max, H1, H2, act, r_cut, dtype, S = s
    lay = htf.DescriptorMLP(K=K, H1=H1, H2=H2, low=0.5, high=1.8, n_types=T, activation=act, seed=3 + n, r_cut=r_cut,
                            n_species=S, conservative=True, l_max=l_max, device=dev)
    x, index, ty, sp, labels = seeded(n, lay, NN, T, S, False, dtype, dev, n_table=B + GHOST)
    index[2::7, 0] = torch.tensor([-1, B + GHOST, B, B + GHOST - 1, -7, B + GHOST + 5, B + 3, 0, B - 1, B + 1], dtype=torch.int32)
    index, ty = index.to(dev), ty.to(dev) if ty is not None else None

    def halo(table):   # (the same rows for a table of the same shape, whichever call passes it)
        g = torch.Generator().manual_seed(2000 + n)
        table[B:].copy_(0.05 * torch.randn(table[B:].shape, generator=g))

    out = {}
    f, v = lay.total_forces(x, index, virial=True, types=ty, species=sp, n_ghost=GHOST, halo=halo)
    out["total_forces+virial.f"], out["total_forces+virial.v"] = sha(f), sha(v)
    out["total_forces"] = sha(lay.total_forces(x, index, types=ty, species=sp, n_ghost=GHOST, halo=halo))
    sweep = lay.angular_loss_gradient if l_max else lay.total_loss_gradient
    out["angular_loss_gradient" if l_max else "total_loss_gradient"] = sha(
        sweep(x, labels, index, types=ty, species=sp, n_ghost=GHOST, halo=halo))
    torch.cuda.synchronize()
    return out


def run_committee(htf, dev, n, s):
    M, NN, K, T, H1, H2, act, r_cut, dtype, S, absent = s
    lay = htf.DescriptorMLP(K=K, H1=H1, H2=H2, low=0.5, high=1.8, n_types=T, activation=act, seed=3 + n, r_cut=r_cut,
                            n_species=S, conservative=True, n_models=M, device=dev)
    x, index, ty, sp, labels = seeded(n, lay, NN, T, S, absent, dtype, dev)
    index[2, 0], index[3, 0] = -1, B
    index, ty = index.to(dev), ty.to(dev) if ty is not None else None
    out = {}
    f, v, mem = lay.total_forces(x, index, virial=True, types=ty, species=sp, members=True)
    out["total_forces+virial.f"], out["total_forces+virial.v"], out["members"] = sha(f), sha(v), sha(mem)
    out["deviation"] = sha(lay.deviation)
    out["total_forces"] = sha(lay.total_forces(x, index, types=ty, species=sp))
    out["total_forces.deviation"] = sha(lay.deviation)
    out["committee_loss_gradient"] = sha(lay.committee_loss_gradient(x, labels, index, types=ty, species=sp))
    torch.cuda.synchronize()
    return out


def compare(a, b):
    A, Bb = (json.load(open(p))["cases"] for p in (a, b))
    bad = [(c, o) for c in sorted(set(A) | set(Bb)) for o in sorted(set(A.get(c, {})) | set(Bb.get(c, {})))
           if A.get(c, {}).get(o) != Bb.get(c, {}).get(o)]
    n = sum(len(v) for v in A.values())
    for c, o in bad:
        print("differs: %s  %s" % (c, o))
    print("%d outputs of %d settings: %s" % (n, len(A), "%d differ" % len(bad) if bad else "every hash equal"))
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
    cases = {}
    for n, s in enumerate(SETTINGS):
        name = "NN%d_K%d_T%d_l%d_H%dx%d_%s_rc%s_%s_S%d%s%s" % (s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7],
                                                              "f32" if s[8] == F32 else "f64", s[9], "_absent" if s[10] else "",
                                                              "_dirty" if s[11] else "")
        cases[name] = run_setting(htf, dev, n, s)
    dt = {F32: "f32", F64: "f64"}
    for n, s in enumerate(GHOST_SETTINGS, len(cases)):
        cases["ghost%d_NN%d_K%d_T%d_l%d_H%dx%d_%s_rc%s_%s_S%d" % ((GHOST,) + s[:8] + (dt[s[8]], s[9]))] = run_ghost(htf, dev, n, s)
    for n, s in enumerate(COMMITTEE_SETTINGS, len(cases)):
        cases["committee_M%d_NN%d_K%d_T%d_H%dx%d_%s_rc%s_%s_S%d%s" % (s[:8] + (dt[s[8]], s[9], "_absent" if s[10] else ""))] = \
            run_committee(htf, dev, n, s)
    with open(sys.argv[1], "w") as f:
        json.dump({"lib": _lib.LIB_PATH, "binding": _lib.BINDING, "cases": cases}, f, indent=1, sort_keys=True)
    print("%d outputs of %d settings -> %s (%s)" % (sum(len(v) for v in cases.values()), len(cases), sys.argv[1], _lib.LIB_PATH))
    return 0


if __name__ == "__main__":
    sys.exit(main())
