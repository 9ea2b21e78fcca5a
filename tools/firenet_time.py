"""FireNet timings (protocol of tools/convgru_time.py, whose `alternate` this imports): HIP events, the variants ALTERNATING inside the timed
loop (one call of each per round), median of --reps (60) rounds after warm-up, one fresh child process per measurement, every GPU child
under its own timeout.  Shapes: the training batch 12 x 128 x 128 and one unpadded real-data frame 1 x 180 x 240.

    net       one time step of the whole network on G28's weights:
                package      v2v_amd.unet.FireNet.forward
                graph        FireNet.forward_sequence(graph=True) over --steps (8) steps, replay time / steps
                stock_fp32   tests/firenet_stock.py StockFireNet in float32
                stock_bf16   the same under bf16 autocast
                e2vid        (12 x 128 x 128 only, context) one E2VIDRecurrent step ('convlstm') of the package
    layer     the fused launches alone against the same layer as stock ops under bf16 autocast on channels-last bf16 tensors:
                gru16 / stock_gru        one ConvGRU(16, 16, 3) step with a given state
                res16 / stock_res        one ResidualBlock(16, 16)
    all       runs `net` and `layer` as child processes, then `rocprofv3 --kernel-trace --stats` of a short `net --only package` run;
              writes <out-dir>/net.jsonl, layer.jsonl, step_kernel_stats.csv

Run on the GPU box:  python tools/firenet_time.py all [--out-dir profiles/firenet]  |  net|layer [--reps N] [--only a,b] [--out FILE]"""
import argparse
import glob
import os
import shutil
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from convgru_time import alternate, child, emit  # noqa: E402

SHAPES = ((12, 128, 128), (1, 180, 240))


def net(a, only):
    import numpy as np
    import torch
    import firenet_stock as S
    from convgru_stock import kwargs
    from v2v_amd.unet import E2VIDRecurrent, FireNet
    g = S.g28()
    vals = {k: torch.from_numpy(np.asarray(v)) for k, v in S.g28_state(g).items()}
    for n, h, w in SHAPES:
        ev = torch.from_numpy(S.sparse_voxels(1, n, a.steps, 5, h, w)).cuda()
        m = FireNet().cuda().eval()
        m.load_state_dict(vals, strict=True)
        p = {k: v.cuda() for k, v in vals.items()}
        s32, s16 = S.StockFireNet(p), S.StockFireNet(p)

        def stock_bf16():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return s16(ev[:, 0])
        fns = {"package": lambda: m(ev[:, 0]), "stock_fp32": lambda: s32(ev[:, 0]), "stock_bf16": stock_bf16}
        if (n, h, w) == SHAPES[0]:
            e2 = E2VIDRecurrent(kwargs("convlstm", num_output_channels=1)).cuda().eval()
            fns["e2vid"] = lambda: e2(ev[:, 0])
        fns = {k: v for k, v in fns.items() if k in only}
        with torch.no_grad():
            res = alternate(fns, a.reps) if fns else {}
            if "graph" in only:
                mg = FireNet().cuda().eval()
                mg.load_state_dict(vals, strict=True)
                med, mn = alternate({"graph": lambda: mg.forward_sequence(ev, graph=True)}, a.reps)["graph"]
                res["graph"] = (med / a.steps, mn / a.steps)
        for k, (med, mn) in res.items():
            emit(a, {"what": "net", "variant": k, "N": n, "H": h, "W": w, "ms_median": round(med, 5), "ms_min": round(mn, 5), "reps": a.reps,
                     **({"steps": a.steps} if k == "graph" else {})})


def layer(a, only):
    import torch
    import firenet_stock as S
    from v2v_amd import nhwc_ops as N
    g = S.g28()
    p32 = {k: torch.from_numpy(v).cuda() for k, v in S.g28_state(g).items()}
    p16 = {k: (v.bfloat16().contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.bfloat16()) for k, v in p32.items()}
    for n, h, w in SHAPES:
        gen = torch.Generator().manual_seed(h)
        x = torch.relu(torch.randn((n, h, w, 16), generator=gen)).bfloat16().cuda()
        h32 = torch.tanh(torch.randn((n, h, w, 16), generator=gen)).cuda()
        hb = h32.bfloat16()
        pg = N.pack_gru16_weights(p32["G1.update_gate.weight"], p32["G1.reset_gate.weight"], p32["G1.out_gate.weight"])
        bg, bo = torch.cat([p32["G1.update_gate.bias"], p32["G1.reset_gate.bias"]]), p32["G1.out_gate.bias"]
        pr = N.pack_resblock16_weights(p32["R1.conv1.weight"], p32["R1.conv2.weight"])
        xs, hs = x.permute(0, 3, 1, 2), hb.permute(0, 3, 1, 2)                  # channels-last bf16 views: what a stock network under autocast holds

        def stock_gru():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return S.stock_gru(xs, hs, p16, "G1")

        def stock_res():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                return S.stock_resblock(xs, p16, "R1")
        fns = {"gru16": lambda: N.convgru16_step(x, hb, h32, pg, bg, bo), "stock_gru": stock_gru,
               "res16": lambda: N.resblock16_nhwc(x, pr, p32["R1.conv1.bias"], p32["R1.conv2.bias"]), "stock_res": stock_res}
        fns = {k: v for k, v in fns.items() if k in only}
        with torch.no_grad():
            res = alternate(fns, a.reps)
        for k, (med, mn) in res.items():
            emit(a, {"what": "layer", "variant": k, "N": n, "H": h, "W": w, "ms_median": round(med, 5), "ms_min": round(mn, 5), "reps": a.reps})


def run_all(a):
    out = os.path.abspath(a.out_dir)
    os.makedirs(out, exist_ok=True)
    me, py = os.path.abspath(__file__), sys.executable
    with open(os.path.join(out, "log.txt"), "w") as log:
        for name in ("net", "layer"):
            path = os.path.join(out, name + ".jsonl")
            if os.path.exists(path):
                os.remove(path)
            child([py, me, name, "--reps", str(a.reps), "--out", path], 300, log)
        prof = os.path.join(out, "_rocprof")
        shutil.rmtree(prof, ignore_errors=True)
        child(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "--", py, me, "net", "--only", "package", "--reps", "20"], 240, log)
        hits = glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True)
        if hits:
            shutil.copy(hits[0], os.path.join(out, "step_kernel_stats.csv"))
        shutil.rmtree(prof, ignore_errors=True)
    print("written:", sorted(os.listdir(out)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("net", "layer", "all"))
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "firenet"))
    a = ap.parse_args()
    if a.what == "all":
        return run_all(a)
    default = ("package", "graph", "stock_fp32", "stock_bf16", "e2vid") if a.what == "net" else ("gru16", "stock_gru", "res16", "stock_res")
    only = tuple(a.only.split(",")) if a.only else default
    (net if a.what == "net" else layer)(a, only)


if __name__ == "__main__":
    main()
