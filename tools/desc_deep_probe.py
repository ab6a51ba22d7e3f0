#!/usr/bin/env python3
"""Times pass 1 of DescriptorMLP(conservative=True, dense="mfma", H3=...) -- htf_cfw3_grad, three hidden layers -- beside the
two-hidden-layer pass 1 (htf_cfw_grad) at the same H1, H2, at tools/desc_wide_probe.py's box and protocol.

Usage:  python tools/desc_deep_probe.py [--n 131072] [--nn 128] [--samples 15] [--reps 10] [--warmup 3] [--json PATH]

N rows x NN slots of a liquid-like list (60 to NN live slots per row, distances 0.8 to 3.2), K = 16 channels, one type, tanh,
fp32.  For 64^3, 128^3, 160-128-96, 240^3 and 256^3: the two entries take turns sample by sample after --warmup samples of
each; a sample is --reps calls between two device events, divided by --reps; medians of --samples samples are reported with
the smallest and largest, with the rows of the tile the launcher's LDS rule picks (include/htf_cfwide3.h), the dense FLOPs per
call -- 4 (D H1 + H1 H2 + H2 H3) + 2 H3 per row, forward and backward -- and their share of --peak-tflops (the fp32 matrix
peak, 157.3 on the MI355X) in pass 1, which also forms the descriptor.  Before the timings: E and g of the three-layer entry
against torch fp32 matmuls on the same G, and a few steps of a 256^3 layer under tfcompute on the stand-in.  Prints one JSON
line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hoomd_tf_amd as htf  # noqa: E402
from hoomd_tf_amd import _lib, ops, standin  # noqa: E402
from committee_probe import alternate  # noqa: E402

WIDTHS = ((64, 64, 64), (128, 128, 128), (160, 128, 96), (240, 240, 240), (256, 256, 256))


def tile_rows(K, T, H1, H2, H3):
    """The launcher's rule (include/htf_cfwide3.h): 64 rows while bytes(64) fit 160 KB, else 32."""
    pad = lambda v: (v + 31) & ~31   # noqa: E731
    lines = max(pad(K * T), pad(H3)) + pad(H1) + pad(H2)
    bytes_ = lambda R: 4 * ((R + 1) * lines + 2 * R * pad(H3) // 32 + ((K + 3) & ~3) + R)   # noqa: E731
    R = 64 if bytes_(64) <= 160 * 1024 else 32
    return R, bytes_(R)


def run_steps(steps=3):
    """DescriptorMLP(K=16, n_types=4, H1=H2=H3=256) under tfcompute on the stand-in: 500 particles, NVE."""
    pos, L, _ = standin.fcc_positions(5, 0.8442)
    sysm = standin.System(pos, L, dtype=torch.float32, device=torch.device("cuda:0"))
    sysm.randomize_velocities(kT=0.3, seed=7)
    sim = standin.Simulation(sysm)
    sim.integrate_nve(0.001)
    lay = htf.DescriptorMLP(K=16, n_types=4, H1=256, H2=256, H3=256, high=2.0, r_cut=2.0, conservative=True, dense="mfma")

    class M(htf.SimModel):
        def compute(self, nlist, positions, box):
            return htf.compute_nlist_forces(nlist, lay(nlist, positions))

    tfc = htf.tfcompute(M(128))
    tfc.attach(sim.nlist_cell(), r_cut=2.5)
    sim.run(steps)
    torch.cuda.synchronize()
    f = sysm.force[:sysm.N]
    assert bool(torch.isfinite(f).all()) and f[:, :3].abs().max().item() > 0
    return {"steps": steps, "max_force": f[:, :3].abs().max().item()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=131072)
    ap.add_argument("--nn", type=int, default=128)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
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
    stream = ops._stream(x)

    out = {"shape": {"N": N, "NN": NN, "K": K, "activation": "tanh"}, "samples": a.samples, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "peak_tflops": a.peak_tflops, "tfcompute_256x256x256": run_steps(), "widths": {}}
    gbuf = torch.empty((N, K), dtype=torch.float32, device=dev)
    ebuf = torch.empty((N,), dtype=torch.float32, device=dev)
    for H1, H2, H3 in WIDTHS:
        deep = htf.DescriptorMLP(K=K, H1=H1, H2=H2, H3=H3, seed=9, conservative=True, dense="mfma")
        two = htf.DescriptorMLP(K=K, H1=H1, H2=H2, seed=9, conservative=True, dense="mfma")
        head = (x.data_ptr(), _lib.HTF_F32, N, NN, K, 1, H1, H2)

        def tail(lay):
            return (_lib.ACT_TANH, lay.w.data_ptr(), lay.mu.data_ptr(), float(lay.gap), gbuf.data_ptr(), ebuf.data_ptr(), None, N, 0.0, stream)

        def pass1_deep():
            _lib.check(_lib.lib.htf_cfw3_grad(*head, H3, *tail(deep)))

        def pass1_two():
            _lib.check(_lib.lib.htf_cfw_grad(*head, *tail(two)))

        # the same answer first: fp32 matmuls on the same G
        W1, b1, W2, b2, W3, b3, W4, b4 = (torch.as_tensor(w, device=dev) for w in deep.get_weights())
        G = deep.descriptor(htf.Nlist(x)).contiguous()
        h1 = torch.tanh(torch.addmm(b1, G, W1))
        h2 = torch.tanh(torch.addmm(b2, h1, W2))
        h3 = torch.tanh(torch.addmm(b3, h2, W3))
        dz3 = W4[:, 0] * (1.0 - h3 * h3)
        dz2 = (dz3 @ W3.t()) * (1.0 - h2 * h2)
        g_ref = ((dz2 @ W2.t()) * (1.0 - h1 * h1)) @ W1.t()
        e_ref = (h3 @ W4)[:, 0] + b4
        pass1_deep()
        R, lds = tile_rows(K, 1, H1, H2, H3)
        res = {"tile_rows": R, "lds_bytes": lds,
               "g_vs_matmuls_rel": ((gbuf - g_ref).abs().max() / g_ref.abs().max()).item(),
               "e_vs_matmuls_rel": ((ebuf - e_ref).abs().max() / e_ref.abs().max()).item()}
        res.update(alternate({"pass1_H3_ms": pass1_deep, "pass1_two_layer_ms": pass1_two}, a.samples, a.reps, a.warmup))
        flops = N * (4.0 * (K * H1 + H1 * H2 + H2 * H3) + 2.0 * H3)
        res["dense_gflop"] = flops * 1e-9
        res["share_of_peak"] = flops / (res["pass1_H3_ms"][0] * 1e-3) / (a.peak_tflops * 1e12)
        res["ratio_to_two_layer"] = res["pass1_H3_ms"][0] / res["pass1_two_layer_ms"][0]
        out["widths"]["%dx%dx%d" % (H1, H2, H3)] = res
    out["note"] = "(median, min, max) in ms per call; one run on one device"
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
