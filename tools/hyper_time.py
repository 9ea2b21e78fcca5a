"""HyperE2VID timings: the package (v2v_amd.hyper.HyperE2VID) beside the stock-PyTorch restatement of the same network (tests/hyper_stock.py,
with the stock unfold + einsum + 1x1 formulation of the dynamic convolution) in float32 and under bf16 autocast; same process, same weights
(golden G26's recipe), HIP events, the variants ALTERNATING inside the timed loop (one step of each per round), median of --reps >= 50
rounds after warm-up.  Shapes 12 x 128 x 128 (the training shape) and 1 x 192 x 240.

    step      ms per time step (states and the fed-back image carried from step to step)
    layer     decoders[0] alone on the same input [N,256,H/8,W/8] + skip: the package's dynamic layer, the package's own STATIC
              UpsampleConvLayer(256, 128, 5) (the layer it replaces: 3.4 x its matrix work), the stock dynamic layer in float32 / bf16

One JSON line per measurement, printed and written to --out.  --only restricts the variants (a kernel table of one variant:
rocprofv3 --kernel-trace --stats --output-format csv -- python tools/hyper_time.py step --only package --reps 5).

Run on the GPU box:  python tools/hyper_time.py step|layer [--reps N] [--only package|static|fp32|bf16] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hyper_stock import KW, LAYER, g26, g26_state, sparse_voxels, stock_layer, stock_step  # noqa: E402
from seeded_weights import load_seeded, seeded_input  # noqa: E402
from v2v_amd.hyper import HyperE2VID  # noqa: E402
from v2v_amd.unet import UpsampleConvLayer  # noqa: E402

NAMES = {"package": "v2v_amd", "static": "v2v_amd static UpsampleConvLayer(256,128,5)", "fp32": "stock fp32", "bf16": "stock bf16 autocast"}
SHAPES = ((12, 128, 128), (1, 192, 240))


def alternate(fns, reps, warmup=5):
    """{name: callable} -> {name: (median ms, min ms)}: every round runs each callable once, timed on its own pair of events."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        marks = {}
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            marks[k] = (s, e)
        torch.cuda.synchronize()
        for k, (s, e) in marks.items():
            times[k].append(s.elapsed_time(e))
    return {k: (float(np.median(v)), float(min(v))) for k, v in times.items()}


def stock_runner(p, ev, kind):
    st = {"states": [None] * 3, "prev": torch.zeros((ev.shape[0], 1) + tuple(ev.shape[-2:]), device="cuda")}

    def run():
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=kind == "bf16"):
            img, st["states"] = stock_step(ev, st["prev"], st["states"], p, unfold=True)
        st["prev"] = img.float()
    return run


def step(a, kinds):
    vals = g26_state(g26())
    rows = []
    for n, h, w in SHAPES:
        ev = torch.from_numpy(sparse_voxels(1, n, 5, h, w)).cuda()
        fns = {}
        if "package" in kinds:
            net = HyperE2VID(dict(KW)).cuda().eval()
            net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()}, strict=True)
            fns["package"] = lambda net=net: net(ev)
        p = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in vals.items()}
        for kind in ("fp32", "bf16"):
            if kind in kinds:
                fns[kind] = stock_runner(p, ev, kind)
        with torch.no_grad():
            res = alternate(fns, a.reps)
        for kind, (med, best) in res.items():
            rows.append({"what": "step", "network": NAMES[kind], "N": n, "H": h, "W": w, "ms_per_step": round(med, 4), "ms_min": round(best, 4), "reps": a.reps,
                         "device": torch.cuda.get_device_name()})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def layer(a, kinds):
    vals = g26_state(g26())
    rows = []
    for n, h, w in SHAPES:
        ev = torch.from_numpy(sparse_voxels(1, n, 5, h, w)).cuda()
        prev = torch.from_numpy(seeded_input(2, n, 1, h, w)).cuda()
        x = torch.from_numpy(seeded_input(3, n, 256, h // 8, w // 8)).cuda()
        skip = torch.from_numpy(seeded_input(4, n, 256, h // 8, w // 8)).cuda()
        xb, sb = (v.to(torch.bfloat16).contiguous(memory_format=torch.channels_last) for v in (x, skip))
        fns = {}
        if "package" in kinds:
            net = HyperE2VID(dict(KW)).cuda().eval()
            net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()}, strict=True)
            dyn = net.unetrecurrent.decoders[0]
            fns["package"] = lambda: dyn(xb, ev, prev, skip=sb)
        if "static" in kinds:
            static = UpsampleConvLayer(256, 128, 5, padding=2).cuda().eval()
            load_seeded(static, 5)
            fns["static"] = lambda: static(xb, sb)
        p = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in vals.items()}
        for kind in ("fp32", "bf16"):
            if kind in kinds:
                def run(kind=kind):
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=kind == "bf16"):
                        return stock_layer(x + skip, ev, prev, p, LAYER, unfold=True)[2]
                fns[kind] = run
        with torch.no_grad():
            res = alternate(fns, a.reps)
        for kind, (med, best) in res.items():
            rows.append({"what": "decoders[0]", "network": NAMES[kind], "N": n, "H": h, "W": w, "ms": round(med, 4), "ms_min": round(best, 4), "reps": a.reps,
                         "device": torch.cuda.get_device_name()})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("step", "layer"))
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--only", choices=tuple(NAMES), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    kinds = [a.only] if a.only else list(NAMES)
    rows = step(a, kinds) if a.what == "step" else layer(a, kinds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
