#!/usr/bin/env python
"""Time NER-Net's learned voxelisation: the fused device path (v2v_amd.nernet) against the stock-torch restatement
(tests/nernet_stock.py -- the BASELINE: the reference's C passes of nn.Linear and C put_ calls, run on the same GPU).

    python tools/nernet_voxel_time.py [--out FILE.jsonl] [--events 200000 2000000] [--intervals 1 8] [--repeats N]

Shape 260 x 346, C = 5, mlp_layers [1, 50, 50, 50, 1] (config/test_nernet_original.yaml), float64 rows (x, y, t, p, b = 0) already on
the device, T intervals of `events` rows each through Voxelization.forward_sequence; the baseline runs its layer once per interval, as
the reference does.  Every shape is warmed up first; the two paths are timed ALTERNATELY, `repeats` rounds of a window that is at least
0.3 s long, host clock around a device synchronise; the median round and the spread (min .. max) are reported, plus the largest
difference of the two grids relative to the grid's largest value (one JSON line per shape).  Needs a GPU: there is no CPU fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import nernet_stock as NS  # noqa: E402
import seeded_weights as SW  # noqa: E402

H, W, C = 260, 346, 5


def rows(seed, n):
    g = np.random.Generator(np.random.PCG64(seed))
    ev = np.zeros((n, 5))
    ev[:, 0] = g.integers(0, W, n)
    ev[:, 1] = g.integers(0, H, n)
    ev[:, 2] = np.sort(1.0 + g.uniform(0, 0.04, n))
    ev[:, 3] = g.choice((-1.0, 1.0), n)
    return torch.from_numpy(ev)


def window(fn, min_seconds):
    """seconds per call over a window of at least min_seconds"""
    calls = 1
    while True:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / calls
        calls = max(calls + 1, int(calls * min_seconds / max(dt, 1e-4) * 1.2))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out")
    ap.add_argument("--events", type=int, nargs="+", default=[200_000, 2_000_000])
    ap.add_argument("--intervals", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--mlp", type=int, nargs="+", default=[1, 50, 50, 50, 1])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/nernet_voxel_time.py needs a GPU: a time taken elsewhere says nothing")
    from v2v_amd import nernet

    net = nernet.Voxelization({}, False, (C, H, W), args.mlp).cuda()
    SW.load_seeded(net.quantization_layer.value_layer, 11)
    stock = NS.StockQuantization((C, H, W), args.mlp, nn.LeakyReLU(negative_slope=0.1)).cuda()
    stock.value_layer.load_state_dict(net.quantization_layer.value_layer.state_dict())
    lines = []
    with torch.no_grad():
        for n in args.events:
            for T in args.intervals:
                seq = [rows(100 + k, n).cuda() for k in range(T)]
                fused = lambda: net.forward_sequence(seq, batch_size=1)                     # noqa: E731
                base = lambda: torch.stack([stock(e, batch_size=1) for e in seq])           # noqa: E731
                got, want = fused(), base()                                                 # warm-up of both paths at this shape ...
                fused(), base()
                diff = float((got - want).abs().max() / want.abs().max())                   # ... and the outputs compared at the size timed
                tf, tb = [], []
                for _ in range(args.repeats):
                    tf.append(window(fused, args.window))
                    tb.append(window(base, args.window))
                mf, mb = statistics.median(tf), statistics.median(tb)
                line = {"shape": [T, 1, 2 * C, H, W], "events_per_interval": n, "intervals": T, "mlp_layers": args.mlp,
                        "fused_ms": round(mf * 1e3, 4), "fused_ms_min_max": [round(min(tf) * 1e3, 4), round(max(tf) * 1e3, 4)],
                        "stock_ms": round(mb * 1e3, 4), "stock_ms_min_max": [round(min(tb) * 1e3, 4), round(max(tb) * 1e3, 4)],
                        "stock_over_fused": round(mb / mf, 2), "fused_events_per_s": round(n * T / mf), "max_rel_diff": diff,
                        "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}
                print(json.dumps(line), flush=True)
                lines.append(line)
                del seq
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
