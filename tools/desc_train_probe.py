#!/usr/bin/env python3
"""Times the descriptor network's force-matching sweep at the C3 shape.

Usage:  python tools/desc_train_probe.py [--n 131072] [--nn 128] [--iters 20] [--warmup 5] [--chunk 32768] [--json PATH]
                                         [--r-cut RC] [--species S]

N rows x NN slots, K = 32 channels, 64 x 64 tanh, one type.  HIP events around each launch, the median of --iters launches
after --warmup:
  (a) htf_bp_forces              DescriptorMLP.forces(x)
  (b) the training sweep         DescriptorMLP.loss_gradient(x, labels, pred=...): bp_sweep_kernel + dtrain_reduce_kernel
  (c) one training step of the same network on the generic torch route: RBF expansion, masked sum over the neighbors and
      three dense layers in plain torch (what RBFExpansion + Dense compute), forces by autograd with create_graph, the mean
      squared error over [N, 4], backward, one SGD step -- in row chunks of --chunk whose gradients add up, so that the
      [rows, NN, K] intermediates of the double backward fit whatever else shares the device.
--r-cut RC gives the layer the cosine cutoff, --species S one network per species with the rows split evenly (row i is
species i mod S); (c) is written for neither and is then left out.
Prints one JSON line; (c)/(b) is the step a user gains over the torch route, optimizer kernel aside.  To see which kernels
run: rocprofv3 --kernel-trace --stats -- python tools/desc_train_probe.py --only sweep
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hoomd_tf_amd as htf  # noqa: E402


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
    ap.add_argument("--chunk", type=int, default=32768)
    ap.add_argument("--only", choices=["all", "sweep"], default="all")
    ap.add_argument("--json", default=None)
    ap.add_argument("--r-cut", type=float, default=None)
    ap.add_argument("--species", type=int, default=1)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    N, NN, K = a.n, a.nn, 32
    g = torch.Generator(device=dev).manual_seed(31)
    cnt = torch.randint(60, NN + 1, (N, 1), device=dev, generator=g)
    d = torch.randn((N, NN, 3), device=dev, generator=g)
    d = d / d.norm(dim=2, keepdim=True)
    r = 0.8 + 2.4 * torch.rand((N, NN, 1), device=dev, generator=g)
    mask = (torch.arange(NN, device=dev)[None, :] < cnt).to(torch.float32)[..., None]
    x = torch.cat([d * r * mask, torch.zeros((N, NN, 1), device=dev)], dim=2).contiguous()
    labels = 0.05 * torch.randn((N, 4), device=dev, generator=g)
    extra, kw = {}, {}
    if a.r_cut is not None:
        extra["r_cut"] = a.r_cut
    if a.species != 1:
        extra["n_species"] = a.species
        kw["species"] = (torch.arange(N, device=dev) % a.species).to(torch.float32)
    lay = htf.DescriptorMLP(K=K, H1=64, H2=64, seed=9, trainable=True, **extra)
    pred = lay.forces(x, **kw)
    accum = torch.empty(a.species * (1 + lay.w.numel() // a.species), dtype=torch.float32, device=dev)
    out = {"shape": {"N": N, "NN": NN, "K": K, "H1": 64, "H2": 64, "activation": "tanh"}, "iters": a.iters, "warmup": a.warmup,
           "r_cut": a.r_cut, "species": a.species, "device": torch.cuda.get_device_name(0)}

    out["sweep_ms"] = timed(lambda: lay.loss_gradient(x, labels, pred=pred, accum=accum, **kw), a.iters, a.warmup)
    if a.only == "all":
        out["forces_ms"] = timed(lambda: lay.forces(x, **kw), a.iters, a.warmup)
    if a.only == "all" and not extra:

        W = [torch.nn.Parameter(torch.as_tensor(w, device=dev)) for w in lay.get_weights()]
        opt = torch.optim.SGD(W, lr=1e-4)
        mu = torch.as_tensor(lay.centers, dtype=torch.float32, device=dev)

        def torch_step():
            opt.zero_grad(set_to_none=True)
            for s in range(0, N, a.chunk):
                xx = x[s:s + a.chunk].clone().requires_grad_(True)
                t = xx[:, :, :3] + 1e-7
                rr = torch.sqrt((t * t).sum(dim=2))
                e = torch.exp(-(rr[..., None] - mu) ** 2 / float(lay.gap)) * (rr > 3e-6).to(torch.float32)[..., None]
                h = torch.tanh(torch.tanh(e.sum(dim=1) @ W[0] + W[1]) @ W[2] + W[3])
                E = (h @ W[4] + W[5])[:, 0]
                (gx,) = torch.autograd.grad(E.sum(), xx, create_graph=True)
                p = torch.cat([2.0 * gx[:, :, :3].sum(dim=1), E[:, None]], dim=1)
                (((p - labels[s:s + a.chunk]) ** 2).sum() / (4.0 * N)).backward()
            opt.step()

        out["torch_step_ms"] = timed(torch_step, max(3, a.iters // 4), 2)
        out["torch_route"] = "plain-torch equivalent of the layers model, row chunks of %d" % a.chunk
        out["torch_over_sweep"] = out["torch_step_ms"][0] / out["sweep_ms"][0]
    out["note"] = "(median, min, max) in ms; one run on one device"
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
