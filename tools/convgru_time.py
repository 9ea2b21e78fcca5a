"""ConvGRU step and FlowNet timings (protocol of tools/hyper_time.py): HIP events, the variants ALTERNATING inside the timed loop (one call
of each per round), median of --reps (60) rounds after warm-up, one fresh child process per measurement, every GPU child under its own
timeout.  Every round starts with one untimed call, so that no timed call starts on an idle queue.

    cell      one recurrent step on NHWC bf16 state at the three encoder shapes of the training batch (12 x 64 x 64x64, 12 x 128 x 32x32,
              12 x 256 x 16x16) and of batch 1 at 192 x 240 (1 x 64 x 96x120, 1 x 128 x 48x60, 1 x 256 x 24x30):
                gru       the package's ConvGRU step (v2v_convgru_step_hip: gates launch + candidate launch, instances picked by shape)
                stock     stock PyTorch ConvGRU under bf16 autocast on channels-last bf16 tensors (tests/convgru_stock.py)
                lstm      the package's own ConvLSTM step at the same shape
              --tiles: also every valid (gates, candidate) instance-code pair, as gru_<g>_<c> (how the automatic choice was made)
              --big: also the encoder shapes of 8 clips at 256 x 256, where large tiles fill the chip
    net       the whole FlowNet step, the package against stock bf16 autocast, at 12 x 128 x 128 and 1 x 192 x 240, both block types
    all       runs `cell`, `cell --tiles` and `net` as child processes, then `rocprofv3 --kernel-trace --stats` of a short `cell --only gru`
              run for the kernel table; writes <out-dir>/cell.jsonl, tiles.jsonl, net.jsonl, step_kernel_stats.csv

One JSON line per measurement, printed and appended to --out.

Run on the GPU box:  python tools/convgru_time.py all [--out-dir profiles/convgru]  |  cell|net [--reps N] [--only a,b] [--tiles] [--out FILE]"""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CELL_SHAPES = ((12, 64, 64, 64), (12, 128, 32, 32), (12, 256, 16, 16), (1, 64, 96, 120), (1, 128, 48, 60), (1, 256, 24, 30))
BIG_SHAPES = ((8, 64, 128, 128), (8, 128, 64, 64), (8, 256, 32, 32))        # --big: the encoder shapes of 8 clips at 256 x 256 (every CU gets a large tile)
NET_SHAPES = ((12, 128, 128), (1, 192, 240))
GATE_COLS = {1: 128, 2: 128, 3: 256, 4: 256, 5: 256}          # columns per tile of the instance codes (include/v2v_hip.h)
CAND_COLS = {1: 64, 2: 128, 3: 256, 4: 256, 5: 128}


def alternate(fns, reps, warmup=5):
    """{name: callable} -> {name: (median ms, min ms)}: every round runs each callable once, timed on its own pair of events."""
    import numpy as np
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    lead_in = list(fns.values())[-1]
    for _ in range(reps):
        marks = {}
        lead_in()                                   # untimed: no timed call starts on an idle queue (the first of a round would pay the launch latency alone)
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


def emit(a, row):
    line = json.dumps(row)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


def cell(a, only):
    import torch
    from convgru_stock import stock_gru
    from v2v_amd import convlstm as CL
    for b, c, h, w in (CELL_SHAPES + BIG_SHAPES if a.big else CELL_SHAPES):
        g = torch.Generator().manual_seed(c + h)
        x = torch.relu(torch.randn((b, h, w, c), generator=g)).bfloat16().cuda()
        h32 = torch.tanh(torch.randn((b, h, w, c), generator=g)).cuda()
        hb = h32.bfloat16()
        ws = [(torch.randn((c, 2 * c, 3, 3), generator=g) * 0.02).cuda() for _ in range(3)]
        bs = [torch.zeros(c).cuda() for _ in range(3)]
        packed, b_gates = CL.pack_gru_weights(*ws), torch.cat(bs[:2])
        lstm_packed = CL.pack_gate_weights((torch.randn((4 * c, 2 * c, 3, 3), generator=g) * 0.02).cuda())
        lstm_bias = torch.zeros(4 * c).cuda()
        p = {f"m.{n}.weight": v.bfloat16().contiguous(memory_format=torch.channels_last) for n, v in zip(("update_gate", "reset_gate", "out_gate"), ws)}
        p.update({f"m.{n}.bias": v.bfloat16() for n, v in zip(("update_gate", "reset_gate", "out_gate"), bs)})
        xs, hs = x.permute(0, 3, 1, 2), hb.permute(0, 3, 1, 2)                  # channels-last bf16 views: what a stock network under autocast holds

        def stock():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return stock_gru(xs, hs, p, "m")
        fns = {"gru": lambda: CL.convgru_step(x, hb, h32, packed, b_gates, bs[2]), "stock": stock,
               "lstm": lambda: CL.convlstm_step(x, hb, h32, lstm_packed, lstm_bias, nchw_dtype=None)}
        fns = {k: v for k, v in fns.items() if k in only}
        if a.tiles:
            for tg, gc in GATE_COLS.items():
                for tc, cc in CAND_COLS.items():
                    if (gc == 128 or c % 128 == 0) and c % cc == 0:
                        fns[f"gru_{tg}_{tc}"] = lambda tg=tg, tc=tc: CL.convgru_step(x, hb, h32, packed, b_gates, bs[2], tile_gates=tg, tile_cand=tc)
        with torch.no_grad():
            res = alternate(fns, a.reps)
        for k, (med, mn) in res.items():
            emit(a, {"what": "cell", "variant": k, "B": b, "C": c, "H": h, "W": w, "ms_median": round(med, 5), "ms_min": round(mn, 5), "reps": a.reps})


def net(a, only):
    import numpy as np
    import torch
    from convgru_stock import BLOCKS, StockFlowNet, g27, g27_state, kwargs, sparse_voxels
    from v2v_amd.unet import FlowNet
    g = g27()
    for block in BLOCKS:
        vals = g27_state(g, block)
        for n, h, w in NET_SHAPES:
            ev = torch.from_numpy(sparse_voxels(1, n, 5, h, w)).cuda()
            fns = {}
            if "package" in only:
                m = FlowNet(kwargs(block)).cuda().eval()
                m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()}, strict=True)
                fns["package"] = lambda m=m: m(ev)
            if "stock" in only:
                s = StockFlowNet({k: torch.from_numpy(np.asarray(v)).cuda() for k, v in vals.items()}, block)

                def stock(s=s):
                    with torch.autocast("cuda", dtype=torch.bfloat16):
                        return s(ev)
                fns["stock"] = stock
            with torch.no_grad():
                res = alternate(fns, a.reps)
            for k, (med, mn) in res.items():
                emit(a, {"what": "net", "block": block, "variant": k, "N": n, "H": h, "W": w, "ms_median": round(med, 5), "ms_min": round(mn, 5), "reps": a.reps})


def child(args, seconds, log):
    """One fresh child process under its own time limit; its exit status decides whether anything else starts."""
    cmd = ["timeout", "-k", "10", str(seconds)] + args
    print("+", " ".join(cmd), flush=True)
    rc = subprocess.call(cmd, cwd=ROOT, stdout=log, stderr=subprocess.STDOUT)
    if rc != 0:
        raise SystemExit(f"child exited with {rc}: nothing more is started (see {log.name})")


def run_all(a):
    out = os.path.abspath(a.out_dir)
    os.makedirs(out, exist_ok=True)
    me, py = os.path.abspath(__file__), sys.executable
    with open(os.path.join(out, "log.txt"), "w") as log:
        for name, extra in (("cell", ["cell"]), ("tiles", ["cell", "--tiles", "--big", "--only", "gru"]), ("net", ["net"])):
            path = os.path.join(out, name + ".jsonl")
            if os.path.exists(path):
                os.remove(path)
            child([py, me] + extra + ["--reps", str(a.reps), "--out", path], 420, log)
        prof = os.path.join(out, "_rocprof")
        shutil.rmtree(prof, ignore_errors=True)
        child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "--", py, me, "cell", "--only", "gru,lstm", "--reps", "20"], 300, log)
        hits = glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True)
        if hits:
            shutil.copy(hits[0], os.path.join(out, "step_kernel_stats.csv"))
        shutil.rmtree(prof, ignore_errors=True)
    print("written:", sorted(os.listdir(out)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("cell", "net", "all"))
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--only", default="")
    ap.add_argument("--tiles", action="store_true")
    ap.add_argument("--big", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "convgru"))
    a = ap.parse_args()
    if a.what == "all":
        return run_all(a)
    default = ("gru", "stock", "lstm") if a.what == "cell" else ("package", "stock")
    only = tuple(a.only.split(",")) if a.only else default
    (cell if a.what == "cell" else net)(a, only)


if __name__ == "__main__":
    main()
