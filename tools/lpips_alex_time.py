"""LPIPS-AlexNet timing on one test sequence (T = 40 frames, pred / frame [1,T,1,H,W] in 0..255, at 260 x 346 and 180 x 240):

    sequence        v2v_amd.lpips_alex.LPIPSAlex.sequence on the device kernels: one batched pass, result left on the device
    stock_frames    the stock float32 restatement (tests/lpips_alex_stock.py, plain torch.nn.functional) driven as the reference's
                    compute_metrics drives its own: per frame, batch 1, / 255, normalize=True, .item()
    stock_batch     the same stock module given all T frames at once, result left on the device

Weights are golden G34's (seeded backbone + the reference's linear layers).  Protocol: the device idle before each call, host clock from
the call to the end of a synchronise after it, the three variants alternating inside the timed loop, median and minimum of --reps rounds
after warm-up, both orders.  The variants' results are compared first.  --only NAME runs that variant alone --calls times at one size and
times nothing: the run to put under a kernel trace.  --tf FILE reads the kernel-trace statistics of such a run of `sequence` (--calls C at
260 x 346) and prints the achieved Tflop/s of every convolution.

Run on the GPU box:  python tools/lpips_alex_time.py [--reps 20] [--out profiles/lpips_alex/lpips_alex_time.jsonl]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from convgru_time import emit  # noqa: E402

T = 40
SIZES = ((260, 346), (180, 240))


def layer_macs(h, w):
    """multiply-adds per image of the five convolutions"""
    from v2v_amd.lpips_alex import CONVS, tap_sizes
    return [th * tw * cout * cin * ks * ks for (th, tw), (_, _, cin, cout, ks, _, _, _) in zip(tap_sizes(h, w), CONVS)]


def host_alternate(fns, reps, warmup=3):
    """{name: callable} -> {name: (median ms, min ms)}: every round runs each callable once, the device idle before it, host clock to the
    end of a synchronise after it."""
    import numpy as np
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (float(np.median(v)), float(min(v))) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", choices=("", "sequence", "stock_frames", "stock_batch"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--size", default="260x346")
    ap.add_argument("--tf", default="", help="kernel_stats.csv of a traced `--only sequence` run")
    a = ap.parse_args()
    if a.tf:
        return achieved_tf(a)
    import numpy as np
    import torch
    import lpips_alex_stock as STOCK
    import lpips_alex_weights as LW
    from v2v_amd.lpips_alex import LPIPSAlex
    assert torch.cuda.is_available(), "lpips_alex_time.py needs the GPU"
    g34 = dict(np.load(os.path.join(ROOT, "tests", "golden", "g34_lpips_alex.npz")))
    state = LW.golden_state(g34)
    model = LPIPSAlex()
    model.load_state_dict(state, strict=True)
    model.cuda()
    cuda_state = {k: v.cuda() for k, v in state.items()}
    sizes = [tuple(int(v) for v in a.size.split("x"))] if a.only else SIZES
    for h, w in sizes:
        g = torch.Generator().manual_seed(34)
        frame = (torch.rand((1, T, 1, h, w), generator=g) * 255).cuda()
        pred = (frame.cpu() + 12.0 * torch.randn((1, T, 1, h, w), generator=g)).clamp(0, 255).cuda()

        def stock_frames():
            with torch.no_grad():
                return [STOCK.lpips_alex(cuda_state, pred[0, t] / 255, frame[0, t] / 255, normalize=True).item() for t in range(T)]

        def stock_batch():
            with torch.no_grad():
                return STOCK.lpips_alex(cuda_state, pred[0] / 255, frame[0] / 255, normalize=True).reshape(-1)

        fns = {"sequence": lambda: model.sequence(pred, frame), "stock_frames": stock_frames, "stock_batch": stock_batch}
        if a.only:
            for _ in range(a.calls):
                fns[a.only]()
            torch.cuda.synchronize()
            return
        seq = fns["sequence"]().double().cpu().numpy()
        per, bat = np.array(stock_frames()), stock_batch().double().cpu().numpy()
        rel = lambda v: float((np.abs(v - seq) / seq).max())   # noqa: E731
        emit(a, {"what": "agreement with sequence (max relative difference over the frames)", "size": [h, w], "stock_frames": rel(per), "stock_batch": rel(bat),
                 "lpips_mean": float(seq.mean())})
        assert rel(per) < 1e-4 and rel(bat) < 1e-4, "the stock module and the kernels disagree beyond float32 rounding"
        res = {}
        for order in (("sequence", "stock_frames", "stock_batch"), ("stock_batch", "stock_frames", "sequence")):
            for k, (med, mn) in host_alternate({k: fns[k] for k in order}, a.reps).items():
                res.setdefault(k, []).append(med)
                emit(a, {"what": "T=40 sequence", "variant": k, "order": "-".join(order), "size": [h, w], "ms_median": round(med, 4), "ms_min": round(mn, 4), "reps": a.reps})
        med = {k: sum(v) / len(v) for k, v in res.items()}
        gflop = 2 * 2 * T * sum(layer_macs(h, w)) / 1e9
        emit(a, {"what": "summary", "size": [h, w], **{f"{k}_ms": round(v, 4) for k, v in med.items()}, "gflop": round(gflop, 1),
                 "sequence_tflops_end_to_end": round(gflop / med["sequence"], 1), "stock_frames_over_sequence": round(med["stock_frames"] / med["sequence"], 2),
                 "stock_batch_over_sequence": round(med["stock_batch"] / med["sequence"], 2)})


def achieved_tf(a):
    """the convolutions of a traced `--only sequence --calls C --size HxW` run: launches in layer order within a call (the 5x5 instance once,
    the 3x3 instance three times), so the per-layer time needs the trace itself; the statistics give the total per instance"""
    import csv
    h, w = (int(v) for v in a.size.split("x"))
    macs = layer_macs(h, w)
    flop = {"alex_stem_kernel": 2 * macs[0], "alex_conv_kernel<5>": 2 * macs[1], "alex_conv_kernel<3>": 2 * sum(macs[2:])}
    for row in csv.DictReader(open(a.tf)):
        for name, f in flop.items():
            if name in row["Name"]:
                total_ns = float(row["TotalDurationNs"])
                print(f"{name}: {total_ns / a.calls / 1e3:.1f} us per call of sequence, {f * 2 * T * a.calls / total_ns / 1e3:.1f} Tflop/s")


if __name__ == "__main__":
    main()
