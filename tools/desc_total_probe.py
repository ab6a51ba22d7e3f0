#!/usr/bin/env python3
"""Times the two sweeps of the descriptor network's conservative forces beside the row operator, at the C3 shape.

Usage:  python tools/desc_total_probe.py [--n 131072] [--nn 128] [--iters 20] [--warmup 5] [--r-cut RC] [--window W] [--l-max L] [--json PATH]

N rows x NN slots, K = 16 channels, 32 x 32 tanh, one type.  HIP events around each launch, the median of --iters launches
after --warmup, all in one process on one device:
  (a) htf_bp_forces      DescriptorMLP.forces(x): the row operator, f_i = 2 sum_j dE_i/dx_ij
  (b) pass 1             htf_cf_grad: the same rows through the network's backward, g = dE/dG and E written
  (c) pass 2             htf_cf_forces: one gather of K floats of g per slot, F = -d(sum E)/dr
Pass 2 is timed twice: with the slots' particles within --window rows of their own row (what a spatially sorted system
gives; default 4096) and drawn from the whole table (the worst case for the gather: N * D * 4 bytes, 8 MB here).
Prints one JSON line; ((b) + (c)) / (a) is what the conservative forces cost over the row operator's.
--l-max 1 or 2 times the angular kernels instead (include/htf_angular.h): pass 1 htf_ang_grad, which writes the table of
4 or 10 floats per row and channel, and pass 2 htf_ang_forces, which gathers K of those records per slot; the row operator
has no angular form, so (a) is left out.  --l-max 0 (the default) is the radial path above.
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


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--nn", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--r-cut", type=float, default=None)
    ap.add_argument("--window", type=int, default=4096)
    ap.add_argument("--l-max", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, NN, K, H = a.n, a.nn, 16, 32
    g = torch.Generator(device=dev).manual_seed(31)
    cnt = torch.randint(60, NN + 1, (N, 1), device=dev, generator=g)
    d = torch.randn((N, NN, 3), device=dev, generator=g)
    d = d / d.norm(dim=2, keepdim=True)
    r = 0.8 + 2.4 * torch.rand((N, NN, 1), device=dev, generator=g)
    mask = (torch.arange(NN, device=dev)[None, :] < cnt).to(torch.float32)[..., None]
    x = torch.cat([d * r * mask, torch.zeros((N, NN, 1), device=dev)], dim=2).contiguous()
    rows = torch.arange(N, device=dev)[:, None]
    near = ((rows + torch.randint(-a.window, a.window + 1, (N, NN), device=dev, generator=g)) % N).to(torch.int32).contiguous()
    far = torch.randint(0, N, (N, NN), device=dev, generator=g).to(torch.int32).contiguous()
    lay = htf.DescriptorMLP(K=K, H1=H, H2=H, seed=9, conservative=True, **({"r_cut": a.r_cut} if a.r_cut is not None else {}),
                            **({"l_max": a.l_max} if a.l_max else {}))
    lm = a.l_max
    gbuf = torch.empty((N, lay.D) if lm == 0 else (N, K, 4 if lm == 1 else 10), dtype=torch.float32, device=dev)
    ebuf = torch.empty((N,), dtype=torch.float32, device=dev)
    out_t = torch.empty((N, 4), dtype=torch.float32, device=dev)
    rc, stream = float(lay.r_cut or 0.0), ops._stream(x)

    def pass1():
        if lm:
            _lib.check(_lib.lib.htf_ang_grad(x.data_ptr(), _lib.HTF_F32, N, NN, K, 1, H, H, _lib.ACT_TANH, lay.w.data_ptr(),
                                             lay.mu.data_ptr(), float(lay.gap), gbuf.data_ptr(), ebuf.data_ptr(), None, N, rc, lm, stream))
            return
        _lib.check(_lib.lib.htf_cf_grad(x.data_ptr(), _lib.HTF_F32, N, NN, K, 1, H, H, _lib.ACT_TANH, lay.w.data_ptr(), lay.mu.data_ptr(),
                                        float(lay.gap), gbuf.data_ptr(), ebuf.data_ptr(), None, N, rc, stream))

    def pass2(index):
        if lm:
            _lib.check(_lib.lib.htf_ang_forces(x.data_ptr(), _lib.HTF_F32, index.data_ptr(), None, N, NN, K, 1, lay.mu.data_ptr(),
                                               float(lay.gap), gbuf.data_ptr(), ebuf.data_ptr(), out_t.data_ptr(), _lib.HTF_F32, None, rc,
                                               lm, stream))
            return
        _lib.check(_lib.lib.htf_cf_forces(x.data_ptr(), _lib.HTF_F32, index.data_ptr(), None, N, NN, K, 1, lay.mu.data_ptr(),
                                          float(lay.gap), gbuf.data_ptr(), ebuf.data_ptr(), out_t.data_ptr(), _lib.HTF_F32, None, rc,
                                          stream))

    out = {"shape": {"N": N, "NN": NN, "K": K, "H1": H, "H2": H, "activation": "tanh"}, "iters": a.iters, "warmup": a.warmup,
           "r_cut": a.r_cut, "window": a.window, "l_max": lm, "table_bytes": gbuf.numel() * 4, "device": torch.cuda.get_device_name(0)}
    if lm == 0:
        out["forces_ms"] = timed(lambda: lay.forces(x), a.iters, a.warmup)
    out["pass1_ms"] = timed(pass1, a.iters, a.warmup)
    out["pass2_ms"] = timed(lambda: pass2(near), a.iters, a.warmup)
    out["pass2_whole_table_ms"] = timed(lambda: pass2(far), a.iters, a.warmup)
    out["total_forces_ms"] = timed(lambda: lay.total_forces(x, near), a.iters, a.warmup)
    if lm == 0:
        out["two_passes_over_forces"] = (out["pass1_ms"][0] + out["pass2_ms"][0]) / out["forces_ms"][0]
    out["note"] = "(median, min, max) in ms; one run on one device"
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
