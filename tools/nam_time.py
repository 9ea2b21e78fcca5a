"""NAM cell and global context block timings (protocol of tools/convgru_time.py, whose `alternate` this uses): HIP events, the variants
ALTERNATING inside the timed loop, median of --reps (60) rounds after warm-up, every round behind one untimed call.

    cell    one NAM step on NHWC state at NER-Net's three encoder shapes for batch 1 at 184 x 240 (the deepest level on its 24 x 30 canvas)
            and at 264 x 352:
              nam       the package's NAM step (v2v_nam_step_hip: three launches, instances picked by shape); nam_1 / nam_2: tile codes 1 / 2
              stock     the cell in stock PyTorch under bf16 autocast on channels-last bf16 tensors (tests/nam_stock.py)
              lstm      the package's own ConvLSTM step at the same shape (one launch of the same main loop, 4C columns)
    gcb     the global context block at its three shapes per frame size (32 / 64 / 128 channels at full, 1/2, 1/4 resolution):
              gcb       the package's three launches
              stock     the same formula in stock PyTorch, float32, channels-last

One JSON line per measurement, printed and appended to --out.

Run on the GPU box:  python tools/nam_time.py cell|gcb [--reps N] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CELL_SHAPES = ((1, 64, 92, 120), (1, 128, 46, 60), (1, 256, 24, 30), (1, 64, 132, 176), (1, 128, 66, 88), (1, 256, 33, 44))
GCB_SHAPES = ((1, 32, 184, 240), (1, 64, 92, 120), (1, 128, 46, 60), (1, 32, 264, 352), (1, 64, 132, 176), (1, 128, 66, 88))


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def cell(args):
    import torch
    from convgru_time import alternate
    from nam_stock import KEYS, nam_case, nam_ref
    from v2v_amd import nhwc_ops as N
    for shape in CELL_SHAPES:
        b, c, h, w = shape
        x, m, hp, cp, ws = nam_case(*shape, seed=1)
        nhwc = lambda t, dt=torch.bfloat16: t.permute(0, 2, 3, 1).contiguous().cuda().to(dt)        # noqa: E731
        xn, mn, hn, cn = nhwc(x), nhwc(m), nhwc(hp), nhwc(cp, torch.float32)
        packed = N.pack_nam_weights(*(ws[k].cuda() for k in KEYS))
        lstm_w = N.pack_gate_weights((torch.randn((4 * c, 2 * c, 3, 3)) * 0.02).cuda())
        bias = torch.zeros(4 * c, device="cuda")
        cl = lambda t: t.cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)  # noqa: E731
        sx, sm, sh, sc, sw = cl(x), cl(m), cl(hp), cl(cp), {k: v.cuda().to(torch.bfloat16) for k, v in ws.items()}     # every cast of nam_ref is then a no-op

        def stock():
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                return nam_ref(sx, sm, sh, sc, sw, torch.bfloat16)
        fns = {"nam": lambda: N.nam_step(xn, mn, hn, cn, packed), "nam_1": lambda: N.nam_step(xn, mn, hn, cn, packed, tile=1),
               "nam_2": lambda: N.nam_step(xn, mn, hn, cn, packed, tile=2), "stock": stock,
               "lstm": lambda: N.convlstm_step(xn, hn, cn, lstm_w, bias, nchw_dtype=None)}
        res = alternate(fns, args.reps)
        emit({"what": "cell", "shape": list(shape), "flops": 2 * b * h * w * 9 * 2 * c * 10 * c,
              **{k: {"median_ms": round(v[0], 4), "min_ms": round(v[1], 4)} for k, v in res.items()}}, args.out)


def gcb(args):
    import torch
    from convgru_time import alternate
    from gcb_stock import gcb_ref as _gcb_ref, gcb_weights as _weights
    from v2v_amd import nhwc_ops as N
    for shape in GCB_SHAPES:
        b, c, h, w = shape
        g = torch.Generator().manual_seed(1)
        x = torch.randn(shape, generator=g)
        ws = _weights(c, g)
        xn = x.permute(0, 2, 3, 1).contiguous().cuda().to(torch.bfloat16)
        packed = N.pack_gcb_weights(*(t.cuda() for t in ws))
        sx, sw = x.cuda().contiguous(memory_format=torch.channels_last), [t.cuda() for t in ws]

        def stock():
            with torch.no_grad():
                return _gcb_ref(sx, sw, torch.float32)[0]
        res = alternate({"gcb": lambda: N.gcb_nhwc(xn, packed), "stock": stock}, args.reps)
        emit({"what": "gcb", "shape": list(shape), "flops": 2 * 2 * b * h * w * c * c,
              **{k: {"median_ms": round(v[0], 4), "min_ms": round(v[1], 4)} for k, v in res.items()}}, args.out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["cell", "gcb"])
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    {"cell": cell, "gcb": gcb}[a.what](a)
