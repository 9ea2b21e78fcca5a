"""Old against new, bit for bit: runs every case of the layer-roles refactor on ONE package (the tree's v2v_amd, or the parent's copy under
$V2V_PARENT_DIR) and saves every output tensor and, per case, the sequence of C entry points launched.

    python profiles/layer_roles/ab_cases.py run <parent|new> <out.pt>      one package, this process
    python profiles/layer_roles/ab_cases.py compare <out.jsonl>             both packages in fresh child processes, then torch.equal on everything
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PARENT = os.path.abspath(os.environ.get("V2V_PARENT_DIR", os.path.join(ROOT, "parent_package")))   # git archive <parent> v2v_amd | tar -x -C $V2V_PARENT_DIR
N, T, H, W = 2, 3, 32, 32


def run(which, out_path):
    sys.path.insert(0, PARENT if which == "parent" else ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import v2v_amd
    from v2v_amd import nhwc_ops
    from v2v_amd import convlstm as CL
    from v2v_amd.hyper import HyperE2VID
    from v2v_amd.unet import E2VIDRecurrent, EVFlowNet, FireNet, FlowNet, UpsampleConvLayer
    from convgru_stock import kwargs
    from hyper_stock import KW as HYPER_KW, g26, g26_state, sparse_voxels
    from seeded_weights import load_seeded, seeded_input
    want_dir = PARENT if which == "parent" else ROOT
    assert os.path.dirname(os.path.dirname(os.path.abspath(v2v_amd.__file__))) == want_dir, v2v_amd.__file__

    launches, current = {}, []
    inner = nhwc_ops._launch

    def recording(name, device, *args):
        current.append(name)
        return inner(name, device, *args)
    nhwc_ops._launch = recording
    tensors = {}

    def flat(prefix, v):
        if v is None:
            return
        if isinstance(v, dict):
            for k, x in v.items():
                flat(f"{prefix}.{k}", x)
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                flat(f"{prefix}.{i}", x)
        else:
            tensors[prefix] = v.detach().float().cpu().clone()
            tensors[prefix + "#meta"] = (str(v.dtype), tuple(v.shape), tuple(v.stride()))

    def case(name, fn):
        current.clear()
        res = fn()
        torch.cuda.synchronize()
        flat(name, res)
        launches[name] = list(current)

    ev = torch.from_numpy(sparse_voxels(41, N, T, 5, H, W)).cuda()
    e2_kw = lambda block: kwargs(block, num_output_channels=1)   # noqa: E731

    def seeded(net, seed=7):
        load_seeded(net, seed)
        return net.cuda().eval()

    def hyper():
        net = HyperE2VID(dict(HYPER_KW)).cuda().eval()
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in g26_state(g26()).items()}, strict=True)
        return net

    nets = {"e2vid_convlstm": (lambda: seeded(E2VIDRecurrent(e2_kw("convlstm"))), True, True),
            "e2vid_convgru": (lambda: seeded(E2VIDRecurrent(e2_kw("convgru"))), True, True),
            "flownet_convlstm": (lambda: seeded(FlowNet(kwargs("convlstm"))), True, True),
            "flownet_convgru": (lambda: seeded(FlowNet(kwargs("convgru"))), True, True),
            "firenet": (lambda: seeded(FireNet()), False, True),
            "evflownet": (lambda: seeded(EVFlowNet(dict(num_bins=5))), False, False),
            "hyper": (hyper, False, False)}

    def states_of(net):
        st = {"states": getattr(net, "states", None)}
        if hasattr(net, "prev_recs"):
            st["prev_recs"] = net.prev_recs
        return st

    with torch.no_grad():
        for name, (make, has_overlap, has_graph) in nets.items():
            net = make()

            def loop():
                net.reset_states()
                outs = [net(ev[:, t]) for t in range(T)]
                return {"out": outs, **states_of(net)}

            def seq(**kw):
                def f():
                    net.reset_states()
                    out = net.forward_sequence(ev, **kw)
                    return {"out": out, **states_of(net)}
                return f
            case(f"infer.{name}.loop", loop)
            if has_overlap:
                case(f"infer.{name}.seq_overlap_false", seq(overlap=False))
                case(f"infer.{name}.seq_overlap_true", seq(overlap=True))
            else:
                case(f"infer.{name}.seq", seq())
            if has_graph:
                case(f"infer.{name}.seq_graph_capture", seq(graph=True))
                case(f"infer.{name}.seq_graph_replay", seq(graph=True))
            del net

    # training: loss and every parameter gradient under an L1 loss
    def train_case(make, outputs):
        def f():
            net = make()
            net.train()
            net.reset_states()
            target = torch.tanh(torch.from_numpy(seeded_input(2, N, T, outputs, H, W))).cuda()
            loss = 0.0
            for t in range(T):
                pred = net(ev[:, t])
                got = torch.cat([pred[k] for k in sorted(pred) if not (k == "image" and outputs == 2)], 1)
                loss = loss + torch.nn.functional.l1_loss(got.float(), target[:, t])
            (loss / T).backward()
            return {"loss": loss.detach(), "grads": {k: p.grad for k, p in net.named_parameters()}}
        return f
    case("train.e2vid", train_case(lambda: seeded(E2VIDRecurrent(e2_kw("convlstm"), trainable=True)), 1))
    case("train.flownet", train_case(lambda: seeded(FlowNet(kwargs("convlstm"), trainable=True)), 3))
    case("train.evflownet", train_case(lambda: seeded(EVFlowNet(dict(num_bins=5), trainable=True)), 2))

    # stand-alone layers on contiguous float32 NCHW inputs (the non-NHWC paths)
    def x32(seed, *shape):
        return torch.from_numpy(seeded_input(seed, *shape)).cuda()
    vox = torch.from_numpy(sparse_voxels(43, N, 5, H, W)).cuda()
    with torch.no_grad():
        case("layer.head", lambda: seeded(CL.ConvLayer(5, 32, 5, padding=2), 11)(vox))
        case("layer.head16", lambda: seeded(CL.ConvLayer(5, 16, 3, padding=1), 12)(vox))
        case("layer.stem", lambda: seeded(CL.ConvLayer(5, 64, 3, stride=2, padding=1), 13)(vox))
        pred = seeded(CL.ConvLayer(32, 1, 1, activation=None), 14)
        case("layer.pred", lambda: pred(x32(50, N, 32, H, W)))
        case("layer.pred_skip", lambda: pred(x32(50, N, 32, H, W), x32(51, N, 32, H, W)))
        x_cl = x32(50, N, 32, H, W).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        case("layer.pred_skip_nhwc", lambda: pred(x_cl, x32(51, N, 32, H, W).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)))
        case("layer.pred_skip_mixed", lambda: pred(x_cl, x32(51, N, 32, H, W).to(torch.bfloat16)))
        case("layer.conv", lambda: seeded(CL.ConvLayer(32, 64, 5, stride=2, padding=2), 15)(x32(52, N, 32, H, W)))
        up = seeded(UpsampleConvLayer(256, 128, 5, padding=2), 16)
        case("layer.upconv", lambda: up(x32(53, N, 256, 4, 4)))
        case("layer.upconv_sum_skip", lambda: up(x32(53, N, 256, 4, 4), x32(54, N, 256, 4, 4)))
        x4_cl = x32(53, N, 256, 4, 4).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
        case("layer.upconv_sum_skip_mixed", lambda: up(x4_cl, x32(54, N, 256, 4, 4).to(torch.bfloat16)))
        upcat = seeded(UpsampleConvLayer(256, 64, 3, padding=1), 17)
        case("layer.upconv_concat_skip", lambda: upcat(x32(55, N, 128, 4, 4), x32(56, N, 128, 4, 4), skip_type="concat"))
        case("layer.resblock", lambda: seeded(CL.ResidualBlock(64, 64), 18)(x32(57, N, 64, 8, 8)))
        lstm = seeded(CL.ConvLSTM(64, 64, 3), 19)

        def lstm_two_steps():
            s1 = lstm(x32(58, N, 64, 8, 8), None)
            s2 = lstm(x32(59, N, 64, 8, 8), s1)
            return [s1, s2]
        case("layer.convlstm", lstm_two_steps)

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    torch.save({"tensors": tensors, "launches": launches}, out_path)
    print(f"{which}: {len(launches)} cases, {sum(1 for k in tensors if not k.endswith('#meta'))} tensors, "
          f"{sum(len(v) for v in launches.values())} launches -> {out_path}", flush=True)


def compare(out_jsonl):
    import tempfile
    import torch
    os.makedirs(os.path.dirname(os.path.abspath(out_jsonl)), exist_ok=True)
    tmp = tempfile.mkdtemp()
    paths = {}
    for which in ("parent", "new"):
        paths[which] = os.path.join(tmp, f"ab_cases_{which}.pt")
        rc = subprocess.call(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "run", which, paths[which]])
        if rc != 0:
            print(f"{which}: child ended with {rc}; stopping", flush=True)
            return rc
    a, b = torch.load(paths["parent"]), torch.load(paths["new"])
    bad = 0
    with open(out_jsonl, "w") as f:
        for case_name in sorted(set(a["launches"]) | set(b["launches"])):
            la, lb = a["launches"].get(case_name), b["launches"].get(case_name)
            keys = sorted(k for k in set(a["tensors"]) | set(b["tensors"]) if k.startswith(case_name + ".") or k == case_name or k.startswith(case_name + "#"))
            n_t = n_diff = 0
            for k in keys:
                va, vb = a["tensors"].get(k), b["tensors"].get(k)
                if k.endswith("#meta"):
                    same = va == vb
                else:
                    n_t += 1
                    same = va is not None and vb is not None and va.shape == vb.shape and torch.equal(va, vb) and not bool(torch.isnan(va).any())
                if not same:
                    n_diff += 1
                    print("DIFFERENT", k, va if k.endswith("#meta") else "", vb if k.endswith("#meta") else "", flush=True)
            row = {"case": case_name, "tensors": n_t, "different": n_diff, "launches_parent": len(la or []), "launches_new": len(lb or []),
                   "launch_lists_identical": la == lb}
            bad += n_diff + (la != lb)
            f.write(json.dumps(row) + "\n")
            print(json.dumps(row), flush=True)
    for p in paths.values():
        os.remove(p)
    print("RESULT:", "all equal, all launch lists identical" if bad == 0 else f"{bad} DEFECTS", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3])
    else:
        sys.exit(compare(sys.argv[2]))
