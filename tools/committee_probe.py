#!/usr/bin/env python3
"""Times a committee of descriptor networks beside M separate calls of the single-network kernels, at the C3 shape.

Usage:  python tools/committee_probe.py [--n 131072] [--nn 128] [--models 4 8] [--samples 15] [--reps 10] [--warmup 3] [--r-cut RC]
                                        [--window W] [--json PATH]

N rows x NN slots of a liquid-like list (60 to NN live slots per row, distances 0.8 to 3.2, the slots' particles within
--window rows of their own row, as a spatially sorted system gives), the layer's default widths: K = 16 channels, 32 x 32 tanh,
one type.  For every M of --models, in one process on one device:
  (a) committee    DescriptorMLP(n_models=M).total_forces(x, index): htf_cmt_grad + htf_cmt_forces, mean forces and deviation
  (b) separate     member(m).total_forces(x, index) for m = 0 .. M - 1: M x (htf_cf_grad + htf_cf_forces), the kernels a user
                   calls today (the mean and the deviation over the M results are not formed, so (b) is flattered)
A sample is --reps calls between two device events, divided by --reps; (a) and (b) alternate sample by sample, after --warmup
samples of each; the medians of --samples samples are reported, with the smallest and largest.  The committee's two launches are
also timed alone, the same way, to say where its time goes.  Prints one JSON line; separate_over_committee is the factor the
committee saves, M being the ceiling no sharing could pass.
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
    ap.add_argument("--reps", type=int, default=10)
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
    stream = ops._stream(x)

    out = {"shape": {"N": N, "NN": NN}, "samples": a.samples, "reps": a.reps, "warmup": a.warmup, "r_cut": a.r_cut,
           "window": a.window, "device": torch.cuda.get_device_name(0), "models": {}}
    for M in a.models:
        lay = htf.DescriptorMLP(seed=9, conservative=True, n_models=M, **({"r_cut": a.r_cut} if a.r_cut is not None else {}))
        out["shape"].update(K=lay.K, H1=lay.H1, H2=lay.H2, activation=lay.activation)
        ones = [lay.member(m) for m in range(M)]
        K, rc = lay.K, float(lay.r_cut or 0.0)
        gbuf = torch.empty((N, M, lay.D), dtype=torch.float32, device=dev)
        ebuf = torch.empty((N, M), dtype=torch.float32, device=dev)
        fbuf = torch.empty((N, 4), dtype=torch.float32, device=dev)
        dbuf = torch.empty((N, 2), dtype=torch.float32, device=dev)

        def separate():
            for one in ones:
                one.total_forces(x, near)

        def pass1():
            _lib.check(_lib.lib.htf_cmt_grad(x.data_ptr(), _lib.HTF_F32, N, NN, K, 1, lay.H1, lay.H2, _lib.ACT_TANH, lay.w.data_ptr(),
                                             lay.mu.data_ptr(), float(lay.gap), gbuf.data_ptr(), ebuf.data_ptr(), None, N, rc, M,
                                             lay.P, stream))

        def pass2():
            _lib.check(_lib.lib.htf_cmt_forces(x.data_ptr(), _lib.HTF_F32, near.data_ptr(), None, N, NN, K, 1, lay.mu.data_ptr(),
                                               float(lay.gap), gbuf.data_ptr(), ebuf.data_ptr(), fbuf.data_ptr(), _lib.HTF_F32, None,
                                               rc, M, dbuf.data_ptr(), None, stream))

        # the same answer first: the committee's mean is the mean of the separate calls
        f = lay.total_forces(x, near).double()
        ref = torch.stack([one.total_forces(x, near).double() for one in ones]).mean(dim=0)
        err = (f - ref).abs().max().item() / ref.abs().max().item()
        if not err <= 2e-5:
            raise SystemExit("committee_probe: the committee's mean differs from the mean of its members' calls by %.3g" % err)
        res = alternate({"committee_ms": lambda: lay.total_forces(x, near), "separate_ms": separate}, a.samples, a.reps, a.warmup)
        res.update(alternate({"committee_pass1_ms": pass1, "committee_pass2_ms": pass2}, a.samples, a.reps, a.warmup))
        res["mean_rel_err"] = err
        res["table_bytes"] = gbuf.numel() * 4
        res["separate_over_committee"] = res["separate_ms"][0] / res["committee_ms"][0]
        out["models"][str(M)] = res
    out["note"] = "(median, min, max) in ms per call; one run on one device"
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
