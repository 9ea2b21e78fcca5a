"""HyperE2VID TRAINING timings, forward + backward: the package (v2v_amd.hyper.HyperE2VID(trainable=True).train(), the dynamic layer through
v2v_amd.train.DynamicUpsampleFn) beside the stock training-mode restatement (tests/hyper_train_stock.py, the unfold + einsum + 1x1
formulation of the dynamic convolution) in float32 and under bf16 autocast; same process, same weights (golden G26's recipe), HIP events,
the variants ALTERNATING inside the timed loop in both orders (even rounds forwards, odd rounds backwards, as tools/loss_time.py does),
median of --reps rounds after warm-up, at the training shape [12,5,128,128].

    layer     decoders[0] alone, forward + backward from a fixed upstream gradient (x and skip need gradients)
    step      one network time step + l1 loss, forward + backward (states and prev_recs reset every round)

One JSON line per measurement, printed and written to --out.  --only restricts the variants (a kernel table of one variant:
rocprofv3 --kernel-trace --stats --output-format csv -- python tools/hyper_train_time.py layer --only package --reps 5).

Run on the GPU box:  python tools/hyper_train_time.py layer|step [--reps N] [--only package|fp32|bf16] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hyper_stock import KW, LAYER, g26, g26_state, sparse_voxels  # noqa: E402
from hyper_train_stock import stock_layer_train, stock_step_train, to_params  # noqa: E402
from seeded_weights import seeded_input  # noqa: E402
from v2v_amd.hyper import HyperE2VID  # noqa: E402

NAMES = {"package": "v2v_amd", "fp32": "stock fp32", "bf16": "stock bf16 autocast"}
N, H, W = 12, 128, 128


def alternate(fns, reps, warmup=3):
    """{name: callable} -> {name: (median ms, min ms)}: every round runs each callable once, on its own pair of events; odd rounds run
    them in the opposite order."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for r in range(reps):
        marks = {}
        for k in (list(fns) if r % 2 == 0 else list(fns)[::-1]):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fns[k]()
            e.record()
            marks[k] = (s, e)
        torch.cuda.synchronize()
        for k, (s, e) in marks.items():
            times[k].append(s.elapsed_time(e))
    return {k: (float(np.median(v)), float(min(v))) for k, v in times.items()}


def package_net(vals):
    net = HyperE2VID(dict(KW), trainable=True).cuda().train()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()}, strict=True)
    return net


def layer(a, kinds):
    vals = g26_state(g26())
    ev = torch.from_numpy(sparse_voxels(1, N, 5, H, W)).cuda()
    prev = torch.from_numpy(seeded_input(2, N, 1, H, W)).cuda()
    x = torch.from_numpy(seeded_input(3, N, 256, H // 8, W // 8)).cuda()
    skip = torch.from_numpy(seeded_input(4, N, 256, H // 8, W // 8)).cuda()
    gy = torch.from_numpy(seeded_input(5, N, 128, H // 4, W // 4)).cuda()
    fns = {}
    if "package" in kinds:
        dyn = package_net(vals).unetrecurrent.decoders[0]
        xb, sb = (v.to(torch.bfloat16).contiguous(memory_format=torch.channels_last).requires_grad_(True) for v in (x, skip))
        gb = gy.to(torch.bfloat16).contiguous(memory_format=torch.channels_last)

        def run_package():
            for q in dyn.parameters():
                q.grad = None
            xb.grad = sb.grad = None
            dyn(xb, ev, prev, skip=sb).backward(gb)
        fns["package"] = run_package
    for kind in ("fp32", "bf16"):
        if kind in kinds:
            p = to_params(vals, torch.float32, "cuda")
            xs, ss = x.clone().requires_grad_(True), skip.clone().requires_grad_(True)

            def run(kind=kind, p=p, xs=xs, ss=ss):
                for q in p.values():
                    q.grad = None
                xs.grad = ss.grad = None
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=kind == "bf16"):
                    y = stock_layer_train(xs + ss, ev, prev, p, LAYER, unfold=True)
                y.backward(gy.to(y.dtype))
            fns[kind] = run
    res = alternate(fns, a.reps)
    rows = [{"what": "decoders[0] forward + backward", "network": NAMES[k], "N": N, "H": H, "W": W, "ms": round(med, 4), "ms_min": round(best, 4),
             "reps": a.reps, "device": torch.cuda.get_device_name()} for k, (med, best) in res.items()]
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def step(a, kinds):
    vals = g26_state(g26())
    ev = torch.from_numpy(sparse_voxels(1, N, 5, H, W)).cuda()
    gt = torch.rand((N, 1, H, W), generator=torch.Generator().manual_seed(6)).cuda()
    fns = {}
    if "package" in kinds:
        net = package_net(vals)

        def run_package():
            net.zero_grad(set_to_none=True)
            net.reset_states()
            (net(ev, gt, 0.5)["image"].float() - gt).abs().mean().backward()
        fns["package"] = run_package
    for kind in ("fp32", "bf16"):
        if kind in kinds:
            p = to_params(vals, torch.float32, "cuda")

            def run(kind=kind, p=p):
                for q in p.values():
                    q.grad = None
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=kind == "bf16"):
                    img, _ = stock_step_train(ev, 0.5 * gt, [None] * 3, p, unfold=True)
                (img.float() - gt).abs().mean().backward()
            fns[kind] = run
    res = alternate(fns, a.reps)
    rows = [{"what": "network step forward + backward", "network": NAMES[k], "N": N, "H": H, "W": W, "ms": round(med, 4), "ms_min": round(best, 4),
             "reps": a.reps, "device": torch.cuda.get_device_name()} for k, (med, best) in res.items()]
    for r in rows:
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("layer", "step"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", choices=tuple(NAMES), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    kinds = [a.only] if a.only else list(NAMES)
    rows = layer(a, kinds) if a.what == "layer" else step(a, kinds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
