"""One training sequence at the reference's training shape (B = 12, T = 40, 5 bins, 128 x 128; config/train_v2v_e2vid_10k.yaml): the
per-step loop of model/train_utils.py:339-345, an L1 loss over all steps, backward (BPTT through the ConvLSTM states), one Adam step.
Three networks from the same seeded weights: the package with trainable=True, the stock network (tools/e2vid_consumer.py) in float32,
and the stock network under bf16 autocast.  Prints and writes one JSON line per network: ms per sequence (median of HIP-event timings
after warm-up) and torch.cuda.max_memory_allocated.

Run on the GPU box:  python tools/train_step_time.py [--reps N] [--only package|fp32|bf16] [--out FILE]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from e2vid_consumer import E2VIDShapedConsumer, reference_to_stock_keys  # noqa: E402
from seeded_weights import load_seeded, seeded_input  # noqa: E402
from v2v_amd.unet import E2VIDRecurrent  # noqa: E402

KW = dict(num_bins=5, skip_type="sum", recurrent_block_type="convlstm", num_encoders=3, base_num_channels=32,
          num_residual_blocks=2, use_upsample_conv=True, final_activation="", norm=None)


def make(kind):
    pkg = E2VIDRecurrent(dict(KW), trainable=True).cuda()
    vals = load_seeded(pkg.unetrecurrent, 7)
    if kind == "package":
        return pkg
    stock = E2VIDShapedConsumer(num_bins=5).cuda()
    stock.load_state_dict(reference_to_stock_keys({k: torch.from_numpy(v) for k, v in vals.items()}), strict=True)
    return stock


def sequence(net, opt, events, target, autocast):
    opt.zero_grad(set_to_none=True)
    net.reset_states()
    loss = 0.0
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        for t in range(events.shape[1]):
            pred = net(events[:, t])
            img = pred["image"] if isinstance(pred, dict) else pred
            loss = loss + torch.nn.functional.l1_loss(img.float(), target[:, t])
    (loss / events.shape[1]).backward()
    opt.step()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", choices=("package", "fp32", "bf16"), default=None)
    ap.add_argument("--B", type=int, default=12)
    ap.add_argument("--T", type=int, default=40)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    events = torch.from_numpy(seeded_input(1, a.B, a.T, 5, a.size, a.size)).cuda()
    target = torch.sigmoid(torch.from_numpy(seeded_input(2, a.B, a.T, 1, a.size, a.size))).cuda()
    rows = []
    for kind in ([a.only] if a.only else ["package", "fp32", "bf16"]):
        net = make("package" if kind == "package" else "stock")
        opt = torch.optim.Adam(net.parameters(), lr=1e-4)
        autocast = kind == "bf16"
        sequence(net, opt, events, target, autocast)                   # warm-up: packing, allocator, kernel attributes
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        times = []
        for _ in range(a.reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            sequence(net, opt, events, target, autocast)
            e.record()
            torch.cuda.synchronize()
            times.append(s.elapsed_time(e))
        times.sort()
        row = {"network": {"package": "v2v_amd trainable=True", "fp32": "stock fp32", "bf16": "stock bf16 autocast"}[kind],
               "B": a.B, "T": a.T, "H": a.size, "W": a.size, "ms_per_sequence": round(times[len(times) // 2], 2),
               "ms_min": round(times[0], 2), "reps": a.reps, "peak_mem_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3),
               "device": torch.cuda.get_device_name()}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del net, opt
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
