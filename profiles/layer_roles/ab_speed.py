"""Speed of the parent's package against this tree's, same library, same Python (protocol of profiles/network_twins/README.md).

    python profiles/layer_roles/ab_speed.py child <parent|new> <process#> <out.jsonl>    one fresh process: every workload warmed up, HIP events per rep
    python profiles/layer_roles/ab_speed.py drive <processes> <out.jsonl>                alternates child processes (first half: parent first)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PARENT = os.path.abspath(os.environ.get("V2V_PARENT_DIR", os.path.join(ROOT, "parent_package")))   # git archive <parent> v2v_amd | tar -x -C $V2V_PARENT_DIR


def child(which, process, out_path):
    pkg_dir = PARENT if which == "parent" else ROOT
    sys.path.insert(0, pkg_dir)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    sys.path.insert(2, os.path.join(ROOT, "tools"))
    import numpy as np
    import torch
    import v2v_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(v2v_amd.__file__))) == pkg_dir, v2v_amd.__file__
    import evflow_time as EV              # the tools' own workloads (they import v2v_amd: already this process's package)
    import firenet_stock as FS
    import train_step_time as TR
    from seeded_weights import load_seeded, seeded_input
    from v2v_amd.unet import E2VIDRecurrent, FireNet
    rows = []

    def timed(what, fn, warm, reps):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        for r in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            rows.append({"package": which, "what": what, "process": process, "rep": r, "ms": round(s.elapsed_time(e), 4)})

    # 1. tools/train_step_time.py, package: 12 x 40 x 128 x 128, forward + BPTT + Adam
    events = torch.from_numpy(seeded_input(1, 12, 40, 5, 128, 128)).cuda()
    target = torch.sigmoid(torch.from_numpy(seeded_input(2, 12, 40, 1, 128, 128))).cuda()
    net = TR.make("package")
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    timed("train_sequence_12x40", lambda: TR.sequence(net, opt, events, target, False), 1, 5)
    del net, opt, target
    torch.cuda.empty_cache()

    # 2. E2VIDRecurrent.forward_sequence at 12 x 40 x 5 x 128 x 128: eager with overlap, and graph=True
    net = E2VIDRecurrent(dict(TR.KW)).cuda().eval()
    load_seeded(net.unetrecurrent, 7)
    with torch.no_grad():
        def eager():
            net.reset_states()
            return net.forward_sequence(events)
        timed("eager_overlap_12x40", eager, 3, 9)
        timed("graph_replay_12x40", lambda: net.forward_sequence(events, graph=True), 3, 9)
    del net, events
    torch.cuda.empty_cache()

    # 3. tools/evflow_time.py, package: the eager 400-image sequence, and training
    ev = torch.from_numpy(EV.sparse_voxels(1, 10, 40, 5, 128, 128)).cuda()
    net, _ = EV.make("package")
    with torch.no_grad():
        timed("evflow_forward_sequence_10x40", lambda: net.forward_sequence(ev), 3, 9)
    del net
    net, params = EV.make("package", trainable=True)
    opt = torch.optim.Adam(params, lr=1e-4, amsgrad=True)
    target = torch.tanh(torch.from_numpy(seeded_input(2, 10, 40, 2, 128, 128))).cuda()

    def ev_train():
        opt.zero_grad(set_to_none=True)
        for k in range(40):
            flow = net(ev[:, k])["flow"]
            (torch.nn.functional.l1_loss(flow.float(), target[:, k]) / 40).backward()
        opt.step()
    timed("evflow_train_sequence_10x40", ev_train, 1, 5)
    del net, params, opt, target, ev
    torch.cuda.empty_cache()

    # 4. FireNet (tools/firenet_time.py's network and weights): the eager sequence, 12 x 40 steps of 128 x 128
    g = FS.g28()
    fire = FireNet().cuda().eval()
    fire.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in FS.g28_state(g).items()}, strict=True)
    ev = torch.from_numpy(FS.sparse_voxels(1, 12, 40, 5, 128, 128)).cuda()
    with torch.no_grad():
        def fire_eager():
            fire.reset_states()
            return fire.forward_sequence(ev)
        timed("firenet_eager_sequence_12x40", fire_eager, 3, 9)

    with open(out_path, "a") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    med = {}
    for r in rows:
        med.setdefault(r["what"], []).append(r["ms"])
    print(which, process, {k: round(float(np.median(v)), 3) for k, v in med.items()}, flush=True)


def drive(processes, out_path):
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    open(out_path, "w").close()
    for p in range(1, processes + 1):
        order = ("parent", "new") if p <= processes // 2 else ("new", "parent")
        for which in order:
            rc = subprocess.call(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "child", which, str(p), out_path])
            if rc != 0:
                print(f"process {p} ({which}) ended with {rc}; stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "child":
        child(sys.argv[2], int(sys.argv[3]), sys.argv[4])
    else:
        sys.exit(drive(int(sys.argv[2]), sys.argv[3]))
