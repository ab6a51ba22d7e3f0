#!/usr/bin/env python3
"""Times the two dense stacks of DescriptorMLP(conservative=True) -- dense="lanes" (htf_cf_grad) and dense="mfma" (htf_cfw_grad) --
at tools/committee_probe.py's box and protocol.

Usage:  python tools/desc_wide_probe.py [--n 131072] [--nn 128] [--samples 15] [--reps 10] [--warmup 3] [--window W] [--json PATH]

N rows x NN slots of a liquid-like list (60 to NN live slots per row, distances 0.8 to 3.2, the slots' particles within
--window rows of their own row), K = 16 channels, one type, tanh, fp32.  For the widths 32 x 32 and 64 x 64 both stacks, for
128 x 128 and 256 x 256 the matrix one: pass 1 alone and whole total_forces calls.  A sample is --reps calls between two device
events, divided by --reps; what is compared alternates sample by sample after --warmup samples of each; medians of --samples
samples are reported with the smallest and largest.  For the wide cases also: the share of --peak-tflops (the fp32 matrix
peak, 157.3 on the MI355X) that the dense FLOPs -- 4 (D H1 + H1 H2) + 2 H2 per row, forward and backward -- reach in pass 1
(which also forms the descriptor), and as an outside yardstick the same forward and backward on the same G as torch fp32
matmuls.  Prints one JSON line.
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
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--peak-tflops", type=float, default=157.3)
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

    out = {"shape": {"N": N, "NN": NN, "K": 16, "activation": "tanh"}, "samples": a.samples, "reps": a.reps, "warmup": a.warmup,
           "window": a.window, "device": torch.cuda.get_device_name(0), "peak_tflops": a.peak_tflops, "widths": {}}
    for H in (32, 64, 128, 256):
        stacks = ("lanes", "mfma") if H <= 64 else ("mfma",)
        lays = {s: htf.DescriptorMLP(K=16, H1=H, H2=H, seed=9, conservative=True, dense=s) for s in stacks}
        gbuf = torch.empty((N, 16), dtype=torch.float32, device=dev)
        ebuf = torch.empty((N,), dtype=torch.float32, device=dev)

        def pass1(s):
            lay = lays[s]
            entry = _lib.lib.htf_cfw_grad if s == "mfma" else _lib.lib.htf_cf_grad
            return lambda: _lib.check(entry(x.data_ptr(), _lib.HTF_F32, N, NN, 16, 1, H, H, _lib.ACT_TANH, lay.w.data_ptr(),
                                            lay.mu.data_ptr(), float(lay.gap), gbuf.data_ptr(), ebuf.data_ptr(), None, N, 0.0, stream))

        res = {}
        if len(stacks) == 2:   # the same answer first
            fa, fb = (lays[s].total_forces(x, near).double() for s in stacks)
            res["mfma_vs_lanes_rel"] = (fa - fb).abs().max().item() / fb.abs().max().item()
        res.update(alternate({"pass1_%s_ms" % s: pass1(s) for s in stacks}, a.samples, a.reps, a.warmup))
        res.update(alternate({"total_%s_ms" % s: (lambda lay=lays[s]: lay.total_forces(x, near)) for s in stacks},
                             a.samples, a.reps, a.warmup))
        flops = N * (4.0 * (16 * H + H * H) + 2.0 * H)
        res["dense_gflop"] = flops * 1e-9
        res["mfma_share_of_peak"] = flops / (res["pass1_mfma_ms"][0] * 1e-3) / (a.peak_tflops * 1e12)
        if H > 64:
            lay = lays["mfma"]
            W1, b1, W2, b2, W3, _ = (torch.as_tensor(w, device=dev) for w in lay.get_weights())
            G = lay.descriptor(htf.Nlist(x)).contiguous()

            def matmuls():
                h1 = torch.tanh(torch.addmm(b1, G, W1))
                h2 = torch.tanh(torch.addmm(b2, h1, W2))
                e = h2 @ W3
                dz2 = W3[:, 0] * (1.0 - h2 * h2)
                dz1 = (dz2 @ W2.t()) * (1.0 - h1 * h1)
                return e, dz1 @ W1.t()

            res.update(alternate({"torch_matmuls_ms": matmuls}, a.samples, a.reps, a.warmup))
        out["widths"]["%dx%d" % (H, H)] = res
    out["note"] = "(median, min, max) in ms per call; one run on one device"
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
