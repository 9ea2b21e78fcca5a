"""LPIPS-VGG timing at one training time step (pred / target [12,1,128,128], normalize=True), forward + backward to pred:

    package         v2v_amd.lpips.LPIPSVGG on the device kernels (bf16 NHWC activations, fp32 accumulation)
    stock_fp32      the stock restatement (tests/lpips_stock.py, plain torch.nn.functional) in float32: what training runs today
    stock_autocast  the same under torch.autocast("cuda", dtype=torch.bfloat16)

Weights are golden G30's (seeded backbone + the reference's linear layers).  Protocol (tools/convgru_time.py's `alternate`): HIP events, the
three variants alternating inside the timed loop, median and minimum of --reps rounds after warm-up, two orders.  The variants' results
are compared first.  --only NAME runs that variant alone --reps times and times nothing: the run to put under a kernel trace.

Run on the GPU box:  python tools/lpips_time.py [--reps 20] [--out profiles/lpips/lpips_time.jsonl]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from convgru_time import alternate, emit  # noqa: E402

SHAPE = (12, 1, 128, 128)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=("", "package", "stock_fp32", "stock_autocast"))
    a = ap.parse_args()
    import numpy as np
    import torch
    import lpips_stock
    import lpips_weights as LW
    from v2v_amd.lpips import LPIPSVGG
    assert torch.cuda.is_available(), "lpips_time.py needs the GPU"
    g30 = dict(np.load(os.path.join(ROOT, "tests", "golden", "g30_lpips_vgg.npz")))
    state = LW.golden_state(g30)
    model = LPIPSVGG()
    model.load_state_dict(state, strict=True)
    model.cuda()
    cuda_state = {k: v.cuda() for k, v in state.items()}
    g = torch.Generator().manual_seed(30)
    target = torch.rand(SHAPE, generator=g).cuda()
    pred = (target.cpu() + 0.1 * torch.randn(SHAPE, generator=g)).clamp(0, 1).cuda().requires_grad_(True)
    gout = torch.arange(1, SHAPE[0] + 1, dtype=torch.float32, device="cuda")

    def package():
        pred.grad = None
        dist = model(pred, target, normalize=True)
        (dist * gout).sum().backward()
        return dist, pred.grad

    def stock(autocast):
        pred.grad = None
        if autocast:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                dist = lpips_stock.lpips_vgg(cuda_state, pred, target, True)
        else:
            dist = lpips_stock.lpips_vgg(cuda_state, pred, target, True)
        (dist.float() * gout).sum().backward()
        return dist.float(), pred.grad

    fns = {"package": package, "stock_fp32": lambda: stock(False), "stock_autocast": lambda: stock(True)}
    if a.only:
        for _ in range(a.reps):
            fns[a.only]()
        torch.cuda.synchronize()
        return
    outs = {k: [v.detach().double().clone() for v in fn()] for k, fn in fns.items()}
    ref = outs["stock_fp32"]
    agree = {k: {"dist_rel_l2": float((v[0] - ref[0]).norm() / ref[0].norm()), "dpred_rel_l2": float((v[1] - ref[1]).norm() / ref[1].norm()),
                 "dpred_cos": float((v[1] * ref[1]).sum() / v[1].norm() / ref[1].norm())} for k, v in outs.items() if k != "stock_fp32"}
    emit(a, {"what": "agreement with stock_fp32", **agree, "dist_mean": float(ref[0].mean())})
    assert agree["package"]["dist_rel_l2"] <= 2 * agree["stock_autocast"]["dist_rel_l2"] + 1e-3, "the package is further from float32 than twice stock autocast"
    res = {}
    for order in (("package", "stock_fp32", "stock_autocast"), ("stock_autocast", "stock_fp32", "package")):
        for k, (med, mn) in alternate({k: fns[k] for k in order}, a.reps).items():
            res.setdefault(k, []).append(med)
            emit(a, {"what": "fwd+bwd", "variant": k, "order": "-".join(order), "shape": list(SHAPE), "ms_median": round(med, 4), "ms_min": round(mn, 4), "reps": a.reps})
    med = {k: sum(v) / len(v) for k, v in res.items()}
    emit(a, {"what": "summary", **{f"{k}_ms": round(v, 4) for k, v in med.items()}, "stock_fp32_over_package": round(med["stock_fp32"] / med["package"], 2),
             "stock_autocast_over_package": round(med["stock_autocast"] / med["package"], 2)})


if __name__ == "__main__":
    main()
