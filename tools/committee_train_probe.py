#!/usr/bin/env python3
"""Times the committee's force-matching sweep beside M separate calls of the single-network sweep, at the C3 shape.

Usage:  python tools/committee_train_probe.py [--n 131072] [--nn 128] [--models 4 8] [--samples 15] [--reps 5] [--warmup 3]
                                              [--r-cut RC] [--window W] [--json PATH]

The rows, slots and index of tools/committee_probe.py (N rows x NN slots of a liquid-like list, 60 to NN live slots per row, the
slots' particles within --window rows of their own), the layer's default widths: K = 16 channels, 32 x 32 tanh, one type.  For
every M of --models, in one process on one device:
  (a) committee    DescriptorMLP(n_models=M).committee_loss_gradient(x, labels, index, pred=members): htf_cmt_loss_grad
  (b) separate     member(m, trainable="total").total_loss_gradient(x, labels, index, pred=members[m]) for m = 0 .. M - 1:
                   M x htf_ct_loss_grad, the single-network sweep of ctrain.o, the route a user had before
The members' predictions are evaluated once and handed to both, so that neither route times a forward call; each route forms
its own residual table from them (one [B, M, 4] table, or M tables [B, 4]) and runs its own reductions.  A sample is --reps
calls between two device events, divided by --reps; (a) and (b) alternate sample by sample, after --warmup samples of each; the
medians of --samples samples are reported with the smallest and largest, and the spread (max - min) / median of each route.
The two C entries are also timed alone, on residual tables formed beforehand, the same way.  Prints one JSON line;
separate_over_committee is the factor the committee saves.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hoomd_tf_amd as htf  # noqa: E402
from hoomd_tf_amd import _lib, ops  # noqa: E402


def sample(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, samples, reps, warmup):
    """{name: (median, min, max)} in ms per call, the functions taking turns sample by sample."""
    for _ in range(warmup):
        for fn in fns.values():
            sample(fn, reps)
    ms = {k: [] for k in fns}
    for _ in range(samples):
        for k, fn in fns.items():
            ms[k].append(sample(fn, reps))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--nn", type=int, default=128)
    ap.add_argument("--models", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--r-cut", type=float, default=None)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, NN = a.n, a.nn
    g = torch.Generator(device=dev).manual_seed(31)
    cnt = torch.randint(60, NN + 1, (N, 1), device=dev, generator=g)
    d = torch.randn((N, NN, 3), device=dev, generator=g)
    d = d / d.norm(dim=2, keepdim=True)
    r = 0.8 + 2.4 * torch.rand((N, NN, 1), device=dev, generator=g)
    mask = (torch.arange(NN, device=dev)[None, :] < cnt).to(torch.float32)[..., None]
    x = torch.cat([d * r * mask, torch.zeros((N, NN, 1), device=dev)], dim=2).contiguous()
    rows = torch.arange(N, device=dev)[:, None]
    near = ((rows + torch.randint(-a.window, a.window + 1, (N, NN), device=dev, generator=g)) % N).to(torch.int32).contiguous()
    labels = 0.05 * torch.randn((N, 4), device=dev, generator=g)
    stream = ops._stream(x)

    out = {"shape": {"N": N, "NN": NN}, "samples": a.samples, "reps": a.reps, "warmup": a.warmup, "r_cut": a.r_cut,
           "window": a.window, "device": torch.cuda.get_device_name(0), "models": {}}
    for M in a.models:
        lay = htf.DescriptorMLP(seed=9, n_models=M, trainable="committee", **({"r_cut": a.r_cut} if a.r_cut is not None else {}))
        out["shape"].update(K=lay.K, H1=lay.H1, H2=lay.H2, activation=lay.activation)
        ones = [lay.member(m, trainable="total") for m in range(M)]
        K, P, rc = lay.K, lay.P, float(lay.r_cut or 0.0)
        pred = lay.total_forces(x, near, members=True)[-1]
        preds = [pred[m].contiguous() for m in range(M)]
        acc = torch.empty((M, 1 + P), dtype=torch.float32, device=dev)
        acc1 = torch.empty((M, 1 + P), dtype=torch.float32, device=dev)

        def committee():
            lay.committee_loss_gradient(x, labels, near, pred=pred, accum=acc)

        def separate():
            for m, one in enumerate(ones):
                one.total_loss_gradient(x, labels, near, pred=preds[m], accum=acc1[m])

        # the C entries alone, on residual tables formed beforehand
        rho_c = (pred - labels[None]).permute(1, 0, 2).contiguous()
        rho_s = [(p - labels).contiguous() for p in preds]
        scr_c = torch.empty(int(_lib.lib.htf_cmt_scratch_floats(N, K, 1, lay.H1, lay.H2, M)), dtype=torch.float32, device=dev)
        scr_s = torch.empty(int(_lib.lib.htf_bp_scratch_floats(N, K, 1, lay.H1, lay.H2)), dtype=torch.float32, device=dev)
        acc2 = torch.empty((M, 1 + P), dtype=torch.float32, device=dev)

        def entry_committee():
            _lib.check(_lib.lib.htf_cmt_loss_grad(x.data_ptr(), _lib.HTF_F32, near.data_ptr(), N, NN, K, 1, lay.H1, lay.H2,
                                                  _lib.ACT_TANH, lay.w.data_ptr(), lay.mu.data_ptr(), float(lay.gap), rho_c.data_ptr(),
                                                  acc2.data_ptr(), scr_c.data_ptr(), None, N, rc, M, P, 1 + P, stream))

        def entry_separate():
            for m in range(M):
                _lib.check(_lib.lib.htf_ct_loss_grad(x.data_ptr(), _lib.HTF_F32, near.data_ptr(), N, NN, K, 1, lay.H1, lay.H2,
                                                     _lib.ACT_TANH, lay.w.data_ptr() + 4 * m * P, lay.mu.data_ptr(), float(lay.gap),
                                                     rho_s[m].data_ptr(), acc2.data_ptr() + 4 * m * (1 + P), scr_s.data_ptr(), None, N,
                                                     rc, stream))

        # the same answer first
        committee()
        separate()
        err = ((acc[:, 1:] - acc1[:, 1:]).abs().amax(dim=1) / acc1[:, 1:].abs().amax(dim=1)).max().item()
        if not err <= 4e-4:
            raise SystemExit("committee_train_probe: the committee's gradient differs from its members' sweeps by %.3g" % err)
        res = alternate({"committee_ms": committee, "separate_ms": separate}, a.samples, a.reps, a.warmup)
        res.update(alternate({"committee_entry_ms": entry_committee, "separate_entry_ms": entry_separate}, a.samples, a.reps, a.warmup))
        for k in ("committee_ms", "separate_ms", "committee_entry_ms", "separate_entry_ms"):
            res[k.replace("_ms", "_spread")] = (res[k][2] - res[k][1]) / res[k][0]
        res["grad_rel_err"] = err
        res["separate_over_committee"] = res["separate_ms"][0] / res["committee_ms"][0]
        res["separate_entry_over_committee_entry"] = res["separate_entry_ms"][0] / res["committee_entry_ms"][0]
        res["lds_bytes"] = htf.DescriptorMLP.committee_train_lds_bytes(M, K, 1, lay.H1, lay.H2)
        out["models"][str(M)] = res
    out["note"] = "(median, min, max) in ms per call; spread = (max - min) / median; one run on one device"
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
