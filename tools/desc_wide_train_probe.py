#!/usr/bin/env python3
"""Times the force-matching sweep of the wide dense stack, DescriptorMLP.wide_loss_gradient (htf_cfw_loss_grad), at
tools/committee_probe.py's box and protocol, beside total_loss_gradient's sweep (htf_ct_loss_grad) where that one exists.

Usage:  python tools/desc_wide_train_probe.py [--n 131072] [--nn 128] [--samples 15] [--reps 5] [--warmup 3] [--window W] [--json PATH]

N rows x NN slots of a liquid-like list (60 to NN live slots per row, distances 0.8 to 3.2, the slots' particles within
--window rows of their own row), K = 16 channels, one type, tanh, fp32, a random residual table.  For the widths 32 x 32 and
64 x 64 both sweeps on the same weights (and their largest difference first), for 128 x 128 and 256 x 256 the wide one: the C
entry alone, residual and scratch made beforehand.  A sample is --reps calls between two device events, divided by --reps;
what is compared alternates sample by sample after --warmup samples of each; medians of --samples samples are reported with
the smallest and largest.  Also: the share of --peak-tflops (the fp32 matrix peak, 157.3 on the MI355X) that the sweep's dense
FLOPs reach -- per row 8 D H1 + 12 H1 H2: forward and backward with tangent, and the two outer products -- in a call that
also forms G and Gdot and adds the tiles into the partials.  No time is a pass or fail condition.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hoomd_tf_amd as htf  # noqa: E402
from hoomd_tf_amd import _lib, ops  # noqa: E402
from committee_probe import alternate  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--nn", type=int, default=128)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--peak-tflops", type=float, default=157.3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, NN, K = a.n, a.nn, 16
    g = torch.Generator(device=dev).manual_seed(31)
    cnt = torch.randint(60, NN + 1, (N, 1), device=dev, generator=g)
    d = torch.randn((N, NN, 3), device=dev, generator=g)
    d = d / d.norm(dim=2, keepdim=True)
    r = 0.8 + 2.4 * torch.rand((N, NN, 1), device=dev, generator=g)
    mask = (torch.arange(NN, device=dev)[None, :] < cnt).to(torch.float32)[..., None]
    x = torch.cat([d * r * mask, torch.zeros((N, NN, 1), device=dev)], dim=2).contiguous()
    rows = torch.arange(N, device=dev)[:, None]
    near = ((rows + torch.randint(-a.window, a.window + 1, (N, NN), device=dev, generator=g)) % N).to(torch.int32).contiguous()
    rho = (0.05 * torch.randn((N, 4), device=dev, generator=g)).contiguous()
    stream = ops._stream(x)
    lib = _lib.lib

    out = {"shape": {"N": N, "NN": NN, "K": K, "activation": "tanh"}, "samples": a.samples, "reps": a.reps, "warmup": a.warmup,
           "window": a.window, "device": torch.cuda.get_device_name(0), "peak_tflops": a.peak_tflops, "widths": {}}
    for H in (32, 64, 128, 256):
        lay = htf.DescriptorMLP(K=K, H1=H, H2=H, seed=9, conservative=True, dense="mfma")
        sweeps = {"wide": (lib.htf_cfw_loss_grad, lib.htf_cfw_scratch_floats(N, K, 1, H, H))}
        if H <= 64:
            sweeps["lanes"] = (lib.htf_ct_loss_grad, lib.htf_bp_scratch_floats(N, K, 1, H, H))
        accum = {s: torch.empty(1 + lay.P, dtype=torch.float32, device=dev) for s in sweeps}
        scratch = {s: torch.empty(int(n), dtype=torch.float32, device=dev) for s, (_, n) in sweeps.items()}

        def sweep(s):
            entry = sweeps[s][0]
            return lambda: _lib.check(entry(x.data_ptr(), _lib.HTF_F32, near.data_ptr(), N, NN, K, 1, H, H, _lib.ACT_TANH,
                                            lay.w.data_ptr(), lay.mu.data_ptr(), float(lay.gap), rho.data_ptr(), accum[s].data_ptr(),
                                            scratch[s].data_ptr(), None, N, 0.0, stream))

        res = {"scratch_mb": 4e-6 * int(sweeps["wide"][1])}
        if "lanes" in sweeps:   # the same answer first
            sweep("wide")()
            sweep("lanes")()
            res["wide_vs_lanes_rel"] = ((accum["wide"][1:].double() - accum["lanes"][1:].double()).abs().max().item()
                                        / accum["lanes"][1:].abs().max().item())
        res.update(alternate({"sweep_%s_ms" % s: sweep(s) for s in sweeps}, a.samples, a.reps, a.warmup))
        flops = N * (8.0 * K * H + 12.0 * H * H)
        res["dense_gflop"] = flops * 1e-9
        res["wide_share_of_peak"] = flops / (res["sweep_wide_ms"][0] * 1e-3) / (a.peak_tflops * 1e12)
        out["widths"]["%dx%d" % (H, H)] = res
    out["note"] = "(median, min, max) in ms per call; one run on one device"
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
