"""EVFlowNet timings: the package (v2v_amd.unet.EVFlowNet) beside the stock-PyTorch restatement of the same network (tests/evflow_stock.py)
in float32 and under bf16 autocast, same process, same weights (golden G25's recipe), after warm-up, HIP events.

    forward   ms per call (median of --reps >= 20), ms per image and images/s at 10 x 128^2 (one step), 400 x 128^2 (the training sequence
              B = 10, T = 40 through forward_sequence; stock: the same 400 images as one batch) and 1 x 192 x 240
    train     one training sequence B = 10, T = 40 at 128^2 as 40 forward / backward steps of the loop (L1 loss, gradients accumulated),
              one Adam step (lr 1e-4, amsgrad): ms per sequence and torch.cuda.max_memory_allocated

One JSON line per measurement, printed and written to --out.  --only restricts the networks (a kernel trace of one network's run:
rocprofv3 --kernel-trace --stats -- python tools/evflow_time.py forward --only package --reps 3).

Run on the GPU box:  python tools/evflow_time.py forward|train [--reps N] [--only package|fp32|bf16] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from evflow_stock import g25, g25_state, sparse_voxels, stock_flow  # noqa: E402
from seeded_weights import seeded_input  # noqa: E402
from v2v_amd.unet import EVFlowNet  # noqa: E402

NAMES = {"package": "v2v_amd", "fp32": "stock fp32", "bf16": "stock bf16 autocast"}


def make(kind, trainable=False):
    """-> (callable events [N,5,H,W] -> flow, parameters)."""
    vals = g25_state(g25())
    if kind == "package":
        net = EVFlowNet(dict(num_bins=5), trainable=trainable).cuda()
        net.load_state_dict({k: torch.from_numpy(v) for k, v in vals.items()}, strict=True)
        return net, list(net.parameters())
    p = {k: torch.from_numpy(v).cuda().requires_grad_(trainable) for k, v in vals.items()}
    return p, list(p.values())


def timed(fn, reps):
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    times.sort()
    return times[len(times) // 2], times[0]


def forward(a, kinds):
    rows = []
    for n, t, h, w in ((10, 1, 128, 128), (10, 40, 128, 128), (1, 1, 192, 240)):
        ev = torch.from_numpy(sparse_voxels(1, n, t, 5, h, w)).cuda()
        for kind in kinds:
            net, _ = make(kind)
            if kind == "package":
                run = (lambda: net.forward_sequence(ev)) if t > 1 else (lambda: net(ev[:, 0])["flow"])
            else:
                flat = ev.reshape(n * t, 5, h, w)

                def run():
                    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=kind == "bf16"):
                        return stock_flow(flat, net)
            with torch.no_grad():
                for _ in range(3):
                    run()
                torch.cuda.synchronize()
                med, best = timed(run, a.reps)
            rows.append({"what": "forward", "network": NAMES[kind], "images": n * t, "N": n, "T": t, "H": h, "W": w, "ms": round(med, 3), "ms_min": round(best, 3),
                         "ms_per_image": round(med / (n * t), 4), "images_per_s": round(1000.0 * n * t / med, 1), "reps": a.reps,
                         "device": torch.cuda.get_device_name()})
            print(json.dumps(rows[-1]), flush=True)
            del net
            torch.cuda.empty_cache()
    return rows


def train(a, kinds):
    n, t, size = 10, 40, 128
    ev = torch.from_numpy(sparse_voxels(1, n, t, 5, size, size)).cuda()
    target = torch.tanh(torch.from_numpy(seeded_input(2, n, t, 2, size, size))).cuda()
    rows = []
    for kind in kinds:
        net, params = make(kind, trainable=True)
        opt = torch.optim.Adam(params, lr=1e-4, amsgrad=True)

        def sequence():
            opt.zero_grad(set_to_none=True)
            for k in range(t):
                with torch.autocast("cuda", dtype=torch.bfloat16, enabled=kind == "bf16"):
                    flow = net(ev[:, k])["flow"] if kind == "package" else stock_flow(ev[:, k], net)
                (torch.nn.functional.l1_loss(flow.float(), target[:, k]) / t).backward()
            opt.step()
        sequence()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        med, best = timed(sequence, a.reps)
        rows.append({"what": "train", "network": NAMES[kind] + (" trainable=True" if kind == "package" else ""), "B": n, "T": t, "H": size, "W": size,
                     "ms_per_sequence": round(med, 2), "ms_min": round(best, 2), "reps": a.reps,
                     "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3), "device": torch.cuda.get_device_name()})
        print(json.dumps(rows[-1]), flush=True)
        del net, params, opt
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("forward", "train"))
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--only", choices=tuple(NAMES), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps is None:
        a.reps = 20 if a.what == "forward" else 5
    kinds = [a.only] if a.only else list(NAMES)
    rows = forward(a, kinds) if a.what == "forward" else train(a, kinds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
