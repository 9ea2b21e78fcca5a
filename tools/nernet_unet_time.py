"""Per-step time of NER-Net's recurrent network (v2v_amd.nernet_unet.UNetNIAM_STcell_GCB), protocol of tools/convgru_time.py (whose
`alternate` this uses): HIP events, the variants ALTERNATING inside the timed loop, median of --reps (40) rounds after warm-up, every
round behind one untimed call.  B = 1 at 184 x 240 (the padded 180 x 240 frame, on its 192 x 240 canvas) and 264 x 352 (260 x 346, canvas
272 x 352):
    net       the package's network, one step on carried states
    stock     the stock restatement (tests/nernet_unet_stock.py) under bf16 autocast, channels-last, one step on carried states
    stock32   the same in float32
One JSON line per frame size, printed and appended to --out.

Run on the GPU box:  python tools/nernet_unet_time.py [--reps N] [--out FILE]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SIZES = ((184, 240), (264, 352))


def main(args):
    import torch
    from convgru_time import alternate
    from nernet_unet_stock import KWARGS, state_shapes, step
    from seeded_weights import seeded_state
    from v2v_amd.nernet_unet import UNetNIAM_STcell_GCB
    sd = {k: torch.from_numpy(v).cuda() for k, v in seeded_state(state_shapes(), 3601, 2.2).items()}
    net = UNetNIAM_STcell_GCB(dict(KWARGS)).eval().cuda()
    net.load_state_dict(sd, strict=True)
    for h, w in SIZES:
        x = torch.randn((1, 10, h, w), device="cuda") * (torch.rand((1, 10, h, w), device="cuda") > 0.6)
        xcl = x.contiguous(memory_format=torch.channels_last)
        net.reset_states()
        states = {}

        def ours():
            with torch.no_grad():
                return net(x)

        def stock(key, autocast):
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
                img, states[key] = step(sd, xcl, states.get(key))
            return img
        res = alternate({"net": ours, "stock": lambda: stock("bf16", True), "stock32": lambda: stock("f32", False)}, args.reps)
        line = json.dumps({"what": "net", "frame": [h, w], **{k: {"median_ms": round(v[0], 4), "min_ms": round(v[1], 4)} for k, v in res.items()}})
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
