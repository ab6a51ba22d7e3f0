#!/usr/bin/env python3
"""NVE drift of KE + sum_i E_i under a conservative DescriptorMLP, by the procedure of DESIGN 0.4.

Usage:  python tools/desc_nve_drift.py [--l-max 0 1 2] [--steps 2000] [--every 100] [--json PATH]

The 500-particle fcc system of the tests (density 0.8442, jitter 0.03 a, kT = 0.3), r_cut = 2.0 in a list of 2.5, K = 16 on
[0.5, 2], 32 x 24 tanh, dt = 0.001, through tfcompute.  Every --every steps the total is sampled at the time of the force:
the integrator is leapfrog (v += f dt, then x += v dt), so the velocities before and after that step are averaged.  One JSON
line per l_max: first and last total, drift, largest excursion from the first sample.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hoomd_tf_amd as htf  # noqa: E402
from hoomd_tf_amd import standin  # noqa: E402


def run(l_max, steps, every, seed=73):
    dev = torch.device("cuda:0")
    lay = htf.DescriptorMLP(K=16, H1=32, H2=24, low=0.5, high=2.0, r_cut=2.0, seed=71, conservative=True, l_max=l_max)
    rng = np.random.default_rng(171)
    ws = lay.get_weights()
    for i in (1, 3, 5):
        ws[i] = (0.1 * rng.standard_normal(ws[i].shape)).astype(np.float32)
    ws[0][2 * lay.K:] *= np.float32(1.0 / 64.0)   # (the Q rows: ||M||_F^2 is in the hundreds, tanh would saturate)
    lay.set_weights(ws)

    class M(htf.SimModel):
        def compute(self, nlist, positions, box):
            return htf.compute_nlist_forces(nlist, lay(nlist, positions))

    pos, L, a = standin.fcc_positions(5, 0.8442)
    pos = pos + 0.03 * a * np.random.default_rng(seed).standard_normal(pos.shape)
    pos -= np.round(pos / L) * L
    sysm = standin.System(pos, L, dtype=torch.float32, device=dev)
    sysm.randomize_velocities(kT=0.3, seed=seed)
    sim = standin.Simulation(sysm)
    sim.integrate_nve(0.001)
    tfc = htf.tfcompute(M(128))
    tfc.attach(sim.nlist_cell(), r_cut=2.5)
    totals = []
    for _ in range(steps // every):
        sim.run(every - 1)
        before = sysm.vel[:sysm.N, :3].double().clone()
        sim.run(1)
        v = 0.5 * (before + sysm.vel[:sysm.N, :3].double())
        totals.append(0.5 * (v * v).sum().item() + sysm.force[:sysm.N, 3].double().sum().item())
    t = np.asarray(totals)
    return {"l_max": l_max, "steps": steps, "every": every, "first": t[0], "last": t[-1], "drift": t[-1] - t[0],
            "relative": (t[-1] - t[0]) / abs(t[0]), "largest_excursion": float(np.abs(t - t[0]).max()),
            "device": torch.cuda.get_device_name(0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--l-max", type=int, nargs="+", default=[0, 2], choices=(0, 1, 2))
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--every", type=int, default=100)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    lines = [json.dumps(run(lm, a.steps, a.every)) for lm in a.l_max]
    print("\n".join(lines))
    if a.json:
        with open(a.json, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
