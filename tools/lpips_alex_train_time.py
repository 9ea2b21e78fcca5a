"""LPIPS-AlexNet as a training loss, forward + backward to pred, at [12,1,128,128] (one training step) and [480,1,128,128] (all T = 40
steps of a sequence at once):

    package         v2v_amd.lpips_alex.LPIPSAlex on the device kernels (float32), dist.sum().backward(); the default grad_chunk (480: one
                    launch per layer at either batch)
    package_chunk40 the same with grad_chunk = 40, twelve launches per layer (batch 480 only; the bits do not depend on the chunk)
    stock_fp32      the stock float32 restatement (tests/lpips_alex_stock.py, plain torch.nn.functional) with autograd
    stock_bf16      the same under torch.autocast(bfloat16)

Weights are golden G34's (seeded backbone + the reference's linear layers); pred = clip(target + 0.1 N(0,1)) in [0, 1], normalize=True.
Protocol (tools/lpips_time.py's): the device idle before each call, host clock from the call to the end of a synchronise after the
backward, the variants alternating inside the timed loop, median and minimum of --reps rounds after warm-up, both orders.  The variants'
losses and gradients are compared with a float64 run of the stock module first.  --only NAME runs that variant alone --calls times at one batch and times nothing: the run to put
under a kernel trace.

Run on the GPU box:  python tools/lpips_alex_train_time.py [--reps 20] [--out profiles/lpips_alex_train/lpips_alex_train_time.jsonl]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from convgru_time import emit  # noqa: E402
from lpips_alex_time import host_alternate, layer_macs  # noqa: E402

BATCHES = (12, 480)
H = W = 128


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=("", "package", "package_chunk40", "stock_fp32", "stock_bf16"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--batch", type=int, default=480)
    a = ap.parse_args()
    import numpy as np
    import torch
    import lpips_alex_stock as STOCK
    import lpips_alex_weights as LW
    from v2v_amd.lpips_alex import LPIPSAlex
    assert torch.cuda.is_available(), "lpips_alex_train_time.py needs the GPU"
    g34 = dict(np.load(os.path.join(ROOT, "tests", "golden", "g34_lpips_alex.npz")))
    state = LW.golden_state(g34)
    model = LPIPSAlex()
    model.load_state_dict(state, strict=True)
    model.cuda()
    cuda_state = {k: v.cuda() for k, v in state.items()}
    for b in ((a.batch,) if a.only else BATCHES):
        g = torch.Generator().manual_seed(35)
        target = torch.rand((b, 1, H, W), generator=g)
        pred = (target + 0.1 * torch.randn((b, 1, H, W), generator=g)).clamp(0, 1).cuda().requires_grad_(True)
        target = target.cuda()

        def step(fn):
            pred.grad = None
            loss = fn().sum()
            loss.backward()
            return loss

        def stock_bf16():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return STOCK.lpips_alex(cuda_state, pred, target, normalize=True).float()

        fns = {"package": lambda: step(lambda: model(pred, target, normalize=True)),
               "stock_fp32": lambda: step(lambda: STOCK.lpips_alex(cuda_state, pred, target, normalize=True)),
               "stock_bf16": lambda: step(stock_bf16)}
        if b > 40:
            small = LPIPSAlex(grad_chunk=40)
            small.load_state_dict(state, strict=True)
            small.cuda()
            fns["package_chunk40"] = lambda: step(lambda: small(pred, target, normalize=True))
        if a.only:
            for _ in range(a.calls):
                fns[a.only]()
            torch.cuda.synchronize()
            return
        # agreement first, against the stock module in float64 on the device.  The inputs are random: among the 10^5 ReLU units and pool
        # windows of an image a few lie within float32 rounding of a tie, and a gate that falls the other way changes that image's gradient
        # by a visible step -- in any float32 run, the stock one included.  So the figures are per image: the median over the images is
        # the arithmetic's error, `images_above_1e-4` counts the images with a flipped gate.
        s64 = {k: v.double() for k, v in cuda_state.items()}
        p64 = pred.detach().double().requires_grad_(True)
        loss64 = STOCK.lpips_alex(s64, p64, target.double(), normalize=True).sum()
        loss64.backward()
        g64 = p64.grad.reshape(b, -1)
        out, row = {}, {"what": "agreement with the stock module in float64: loss (relative), gradient per image (max |g - g64| / max |g64|)", "batch": b, "loss": float(loss64)}
        for k, fn in fns.items():
            loss = float(fn().detach())
            out[k] = (loss, pred.grad.clone())
            e = ((pred.grad.double().reshape(b, -1) - g64).abs().max(1).values / g64.abs().max(1).values).cpu().numpy()
            row[k] = {"loss": abs(loss - float(loss64)) / float(loss64), "grad_median": float(np.median(e)), "grad_max": float(e.max()), "images_above_1e-4": int((e > 1e-4).sum())}
        emit(a, row)
        assert row["package"]["loss"] < 1e-5 and row["package"]["grad_median"] < 1e-4, "the kernels disagree with the float64 run beyond float32 rounding"
        del s64, p64, g64
        res = {}
        if "package_chunk40" in out:
            assert out["package_chunk40"][0] == out["package"][0] and torch.equal(out["package_chunk40"][1], out["package"][1]), "the chunk changed the bits"
        names = tuple(fns)
        for order in (names, names[::-1]):
            for k, (med, mn) in host_alternate({k: fns[k] for k in order}, a.reps).items():
                res.setdefault(k, []).append(med)
                emit(a, {"what": "forward + backward", "variant": k, "order": "-".join(order), "batch": b, "size": [H, W], "ms_median": round(med, 4), "ms_min": round(mn, 4),
                         "reps": a.reps})
        med = {k: sum(v) / len(v) for k, v in res.items()}
        emit(a, {"what": "summary", "batch": b, "size": [H, W], **{f"{k}_ms": round(v, 4) for k, v in med.items()},
                 "forward_gflop": round(2 * 2 * b * sum(layer_macs(H, W)) / 1e9, 2), "stock_fp32_over_package": round(med["stock_fp32"] / med["package"], 2),
                 "stock_bf16_over_package": round(med["stock_bf16"] / med["package"], 2)})


if __name__ == "__main__":
    main()
