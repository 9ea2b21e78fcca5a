"""Old against new, call by call: runs every wrapper of the package on ONE tree (this one's v2v_amd, or the parent's copy under
$V2V_PARENT_DIR) behind a proxy that records what reaches the library, and saves the call lists and every returned tensor.

    python profiles/py_call_path/ab_calls.py run <parent|new> <out.pt>      one package, this process
    python profiles/py_call_path/ab_calls.py compare <out.jsonl>             both packages in fresh child processes, then the comparison

Both trees reach the library only through _lib.lib(), so the same proxy serves both: after the first _lib.lib() it takes the place of
_lib._lib and forwards every call.  Recorded per call: the entry point's name; every integer / float / enum argument by value; per pointer
argument NULL or not, and the same for every pointer field of a by-reference struct (its scalar fields by value); for a `_hip` entry point
whether the stream argument is torch's current stream on the current device, and the current device's index.  Tensors are compared by their
bytes (NaN planes equal themselves), dtype, shape and strides.  The parent package is `git archive <parent> v2v_amd | tar -x -C
$V2V_PARENT_DIR` with the tree's libv2v_hip.so copied beside it (the library is the parent's byte for byte, README.md).
"""
import ctypes as C
import json
import numbers
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PARENT = os.path.abspath(os.environ.get("V2V_PARENT_DIR", os.path.join(ROOT, "parent_package")))
N, T, H, W = 2, 3, 32, 32


def describe(arg):
    """One argument as the comparison sees it."""
    if arg is None:
        return "NULL"
    if isinstance(arg, numbers.Real):                               # Python and NumPy numbers alike
        return int(arg) if isinstance(arg, numbers.Integral) else float(arg)
    if isinstance(arg, C.c_void_p):
        return "ptr" if arg.value else "NULL"
    if isinstance(arg, C.Structure):
        return {name: (("ptr" if getattr(arg, name) else "NULL") if ctype is C.c_void_p else getattr(arg, name)) for name, ctype in arg._fields_}
    if isinstance(arg, C.Array):
        return list(arg)
    if hasattr(arg, "_obj"):                                        # byref(...)
        return {"byref": describe(arg._obj)}
    if hasattr(arg, "value"):                                       # c_uint64, c_float, ...
        return arg.value
    raise RuntimeError(f"argument of a kind the record does not know: {arg!r}")


def run(which, out_path):
    sys.path.insert(0, PARENT if which == "parent" else ROOT)
    sys.path.insert(1, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import v2v_amd
    from v2v_amd import _lib
    want_dir = PARENT if which == "parent" else ROOT
    assert os.path.dirname(os.path.dirname(os.path.abspath(v2v_amd.__file__))) == want_dir, v2v_amd.__file__
    from v2v_amd import convlstm as CL  # noqa: F401
    from v2v_amd import esim, frontend, loader, loss_ops, metrics, nernet, postops, v2e, voxel, voxel_cache
    from v2v_amd.hyper import HyperE2VID
    from v2v_amd.unet import E2VIDRecurrent, EVFlowNet, FireNet
    import loss_inputs
    import metrics_reference as MR
    import nernet_inputs
    from convgru_stock import kwargs
    from hyper_stock import KW as HYPER_KW, g26, g26_state, sparse_voxels
    from seeded_weights import load_seeded, seeded_input

    real = _lib.lib()
    current = []

    class Recorder:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def call(*args):
                rec = {"name": name, "device": torch.cuda.current_device()}
                if name.endswith("_hip"):
                    rec["stream_is_current"] = (args[-1].value or 0) == torch.cuda.current_stream().cuda_stream
                    rec["args"] = [describe(a) for a in args[:-1]]
                else:
                    rec["args"] = [describe(a) for a in args]
                current.append(rec)
                return fn(*args)
            return call
    _lib._lib = Recorder()

    tensors, calls = {}, {}

    def flat(prefix, v):
        if v is None:
            return
        if isinstance(v, dict):
            for k, x in v.items():
                flat(f"{prefix}.{k}", x)
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                flat(f"{prefix}.{i}", x)
        elif isinstance(v, np.ndarray):
            if v.dtype.kind in "biuf":
                flat(prefix, torch.from_numpy(np.ascontiguousarray(v)))
        elif isinstance(v, torch.Tensor):
            t = v.detach()
            tensors[prefix] = t.cpu().contiguous().reshape(-1).view(torch.uint8).clone()
            tensors[prefix + "#meta"] = (str(v.dtype), tuple(v.shape), tuple(v.stride()))
        else:
            tensors[prefix + "#meta"] = repr(v)

    side = torch.cuda.Stream()

    def case(name, fn, on_side=False):
        torch.cuda.synchronize()
        current.clear()
        try:
            if on_side:
                with torch.cuda.stream(side):
                    res = fn()
            else:
                res = fn()
        except (ValueError, AssertionError, IndexError, TypeError, KeyError, NotImplementedError) as e:     # a refusal is a result too; a device error is not
            res = {"raised": f"{type(e).__name__}: {e}"}
        torch.cuda.synchronize()
        flat(name, res)
        calls[name] = [dict(r) for r in current]

    def both(name, fn):
        case(name, fn)
        case(name + "@side_stream", fn, on_side=True)

    g = torch.Generator().manual_seed(20)

    def rand(*shape, dtype=torch.float32, lo=0.0, hi=1.0):
        return (torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo).to(dtype).cuda()

    # ---- ESIM and v2e ---------------------------------------------------------------------------------------------------------------------
    params = [0.2, 0.2, 0.05, 5e-4, 1.0]
    u8 = esim.synth_clips(2, 6, 10, 16, dtype=torch.uint8, seed=5)
    f32 = esim.synth_clips(1, 6, 8, 12, seed=6)

    def esim_sum_u8():
        stats = torch.zeros((2, _lib.VOXEL_STATS_WORDS), dtype=torch.int32, device="cuda")
        counts = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
        out = esim.esim_voxel_batch(u8, params, bin_mode="sum", num_bins=5, counts=counts, clip_keys=torch.tensor([[7, 0], [9, 3]]), pad_to=16, stats=stats)
        return out, stats, counts
    both("esim.batch_u8_sum_stats_counts_keys_pad16", esim_sum_u8)
    replay = [rand(1, 8, 12, dtype=torch.float64), rand(1, 8, 12, dtype=torch.float64), rand(1, 8, 12, dtype=torch.float64, lo=-1.0),
              rand(1, 5, 8, 12, dtype=torch.float64, lo=-1.0)]
    case("esim.batch_f32_bilinear_replay", lambda: esim.esim_voxel_batch(f32, params, bin_mode="bilinear", num_bins=5, rng_mode="replay", replay=replay))
    case("esim.batch_b0", lambda: esim.esim_voxel_batch(u8[:0], params, bin_mode="sum", num_bins=5))
    hw = 16 * 16
    flat_clips = (torch.arange(9 * hw, dtype=torch.int64) * 37 % 251).to(torch.uint8).cuda()            # clip 0: 4 stored frames, clip 1: 5
    offs = torch.tensor([0, 4 * hw], dtype=torch.int64, device="cuda")
    index = torch.tensor([[0, 1, 1, 2, 3, 3], [4, 3, 2, 1, 0, 0]], dtype=torch.int32, device="cuda")
    pk_params = torch.tensor([params, [0.3, 0.25, 0.0, 0.0, 0.0]], dtype=torch.float64, device="cuda")
    pk_keys = torch.tensor([[7, 0], [9, 3]], dtype=torch.int64, device="cuda")
    stored = torch.tensor([4, 5], dtype=torch.int32, device="cuda")
    case("esim.packed", lambda: esim.esim_voxel_packed(flat_clips, offs, index, 16, 16, pk_params, pk_keys))
    case("esim.packed_stored_frames", lambda: esim.esim_voxel_packed(flat_clips, offs, index, 16, 16, pk_params, pk_keys, stored_frames=stored))
    case("esim.synth_clips_f32", lambda: esim.synth_clips(1, 2, 4, 8))
    case("esim.synth_clips_u8", lambda: esim.synth_clips(2, 3, 8, 8, dtype=torch.uint8, clip_id0=4))
    for tag, dt in (("bf16", torch.bfloat16), ("u8", torch.uint8), ("f16", torch.float16)):     # refused output dtypes: KeyError at the call site, no launch
        case(f"esim.batch_out_dtype_{tag}_refused", lambda dt=dt: esim.esim_voxel_batch(u8, params, bin_mode="sum", num_bins=5, out_dtype=dt))
    case("esim.synth_clips_f64_refused", lambda: esim.synth_clips(1, 2, 4, 8, dtype=torch.float64))
    case("esim.algorithmic_bytes_bf16_refused", lambda: torch.tensor(esim.algorithmic_bytes(torch.bfloat16, 2, 6, 8, 12, "bilinear", 5)))
    case("esim.algorithmic_bytes", lambda: torch.tensor(esim.algorithmic_bytes(torch.float32, 2, 6, 8, 12, "bilinear", 5)))

    vp = v2e.make_params(24, "pn_related", 0.5, 0.1, 0.0, 0.1, 30, 0.1, 0, 5.0, 0.1, 0.1)
    v8 = esim.synth_clips(2, 6, 8, 12, dtype=torch.uint8, seed=8)

    def v2e_counts(**kw):
        counts = torch.zeros((2, 2), dtype=torch.int64, device="cuda")
        return v2e.v2e_voxel_batch(v8, vp, bin_mode="sum", num_bins=5, seed=3, counts=counts, **kw), counts
    v2e_replay = {"pos_thres": rand(2, 8, 12, dtype=torch.float64, lo=0.2, hi=0.4), "neg_thres": rand(2, 8, 12, dtype=torch.float64, lo=0.2, hi=0.4),
                  "noise_rate": rand(2, 8, 12, lo=0.5, hi=2.0), "leak_randn": rand(2, 5, 8, 12, dtype=torch.float64, lo=-1.0),
                  "shot_pos": (rand(2, 5, 8, 12) < 0.05).to(torch.int64), "shot_neg": (rand(2, 5, 8, 12) < 0.05).to(torch.int64)}
    both("v2e.native", lambda: v2e.v2e_voxel_batch(v8, vp, bin_mode="sum", num_bins=5, seed=3))
    case("v2e.native_counts", v2e_counts)
    case("v2e.replay", lambda: v2e.v2e_voxel_batch(v8, vp, bin_mode="bilinear", num_bins=5, rng_mode="replay", replay=v2e_replay))
    case("v2e.replay_counts", lambda: v2e_counts(rng_mode="replay", replay=v2e_replay))
    for tag, dt in (("bf16", torch.bfloat16), ("u8", torch.uint8)):
        case(f"v2e.out_dtype_{tag}_refused", lambda dt=dt: v2e.v2e_voxel_batch(v8, vp, bin_mode="sum", num_bins=5, seed=3, out_dtype=dt))

    # ---- event lists: every event on a pixel of its own, so no cell takes two terms and no sum depends on the order of the atomics -------------
    eh, ew, ne = 8, 10, 12
    cells = np.random.default_rng(3).permutation(eh * ew)[:ne]
    xs, ys = (cells % ew).astype(np.int64), (cells // ew).astype(np.int64)
    ts = np.arange(ne, dtype=np.float64) / (ne - 1)
    ps = (np.arange(ne) % 2).astype(np.float64)
    none = [np.zeros(0), np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)]
    txs, tys, tts, tps = torch.from_numpy(xs).cuda(), torch.from_numpy(ys).cuda(), torch.from_numpy(ts).float().cuda(), torch.from_numpy(ps * 2 - 1).float().cuda()
    both("voxel.make_voxel_interp", lambda: voxel.make_voxel([ts, xs, ys, ps], eh, ew, 5, True))
    case("voxel.make_voxel_discrete", lambda: voxel.make_voxel([ts, xs, ys, ps], eh, ew, 5, False))
    case("voxel.make_voxel_none", lambda: voxel.make_voxel(none, eh, ew))
    case("voxel.events_to_voxel", lambda: voxel.events_to_voxel(xs, ys, ts, ps * 2 - 1, 5, (eh, ew)))
    case("voxel.events_to_voxel_none", lambda: voxel.events_to_voxel(none[1], none[2], none[0], none[3], 5, (eh, ew)))
    case("voxel.events_to_voxel_torch", lambda: voxel.events_to_voxel_torch(txs, tys, tts, tps, 5, sensor_size=(eh, ew)))
    case("voxel.events_to_voxel_torch_discrete", lambda: voxel.events_to_voxel_torch(txs, tys, tts, tps, 5, sensor_size=(eh, ew), temporal_bilinear=False))
    case("voxel.events_to_voxel_torch_none", lambda: voxel.events_to_voxel_torch(txs[:0], tys[:0], tts[:0], tps[:0], 5, sensor_size=(eh, ew)))
    case("voxel.events_to_neg_pos_voxel", lambda: voxel.events_to_neg_pos_voxel(xs, ys, ts, ps, 5, (eh, ew)))
    case("voxel.events_to_neg_pos_voxel_torch", lambda: voxel.events_to_neg_pos_voxel_torch(txs, tys, tts, tps, 5, sensor_size=(eh, ew)))
    case("voxel.events_to_image", lambda: voxel.events_to_image(xs, ys, ps, (eh, ew)))
    case("voxel.events_to_image_none", lambda: voxel.events_to_image(none[1], none[2], none[3], (eh, ew)))
    case("voxel.events_to_image_torch", lambda: voxel.events_to_image_torch(txs, tys, tps, sensor_size=(eh, ew)))
    case("voxel.events_to_image_torch_none", lambda: voxel.events_to_image_torch(txs[:0], tys[:0], tps[:0], sensor_size=(eh, ew)))
    case("voxel.events_to_image_torch_bilinear", lambda: voxel.events_to_image_torch(txs.float() * 0.5 + 0.25, tys.float() * 0.5 + 0.25, tps, sensor_size=(eh, ew),
                                                                                       interpolation="bilinear"))
    case("voxel.interpolate_to_image", lambda: voxel.interpolate_to_image(txs, tys, torch.full((ne,), 0.25), torch.full((ne,), 0.5), tps,
                                                                           torch.zeros((eh + 1, ew + 1), dtype=torch.float32, device="cuda")))
    case("voxel.voxel_grids_fixed_n_torch", lambda: voxel.voxel_grids_fixed_n_torch(txs, tys, tts, tps, 5, 4, sensor_size=(eh, ew)))
    case("voxel.voxel_grids_fixed_t_torch", lambda: voxel.voxel_grids_fixed_t_torch(txs, tys, tts, tps, 5, 0.3, sensor_size=(eh, ew)))
    case("voxel.events_to_voxel_timesync_torch", lambda: voxel.events_to_voxel_timesync_torch(txs, tys, tts, tps, 5, 0.2, 0.8, sensor_size=(eh, ew)))
    case("voxel.make_voxels_segmented", lambda: voxel.make_voxels_segmented([ts, xs, ys, ps], [0, 5, 5, ne], eh, ew))
    case("voxel.make_voxels_segmented_none", lambda: voxel.make_voxels_segmented(none, [0, 0, 0], eh, ew))

    fix = os.path.join(ROOT, "tests", "golden", "g16_monash_sequence.npz")
    both("voxel_cache.sequence_voxels", lambda: voxel_cache.sequence_voxels(fix, temporal_bilinear=False))
    tmp = tempfile.mkdtemp()
    case("voxel_cache.convert", lambda: voxel_cache.convert(fix, os.path.join(tmp, "c.npz"), False))
    case("voxel_cache.testh5_to_cache", lambda: voxel_cache.testh5_to_cache(fix, os.path.join(tmp, "t.npz"), {"num_bins": 5, "dataset_name": "hqf"}))

    # ---- post-ops -----------------------------------------------------------------------------------------------------------------------------
    vox = esim.esim_voxel_batch(u8, params, bin_mode="sum", num_bins=5, seed=2)                         # [2,1,5,10,16], integer-valued
    st = torch.zeros((2, _lib.VOXEL_STATS_WORDS), dtype=torch.int32, device="cuda")
    esim.esim_voxel_batch(u8, params, bin_mode="sum", num_bins=5, seed=2, stats=st)
    both("postops.normalize_and_pad_radix", lambda: postops.normalize_and_pad(vox))
    case("postops.normalize_and_pad_count", lambda: postops.normalize_and_pad(vox, method="count"))
    case("postops.pad_events_no_workspace", lambda: postops.pad_events(vox))
    case("postops.normalize_batch_voxel", lambda: postops.normalize_batch_voxel(vox))
    case("postops.scales_from_stats", lambda: postops.scales_from_stats(st, 5 * 10 * 16))
    sc = postops.scales_from_stats(st, 5 * 10 * 16)
    case("postops.apply_scales", lambda: postops.apply_scales(vox, sc))
    case("postops.apply_scales_none", lambda: postops.apply_scales(vox, None))
    case("postops.voxel_scales_radix", lambda: postops.voxel_scales_radix(vox))
    case("postops.voxel_scales_count", lambda: postops.voxel_scales_radix(vox, method="count"))

    # ---- front end and loader -------------------------------------------------------------------------------------------------------------------
    raw = (torch.arange(4 * 40 * 48 * 3, dtype=torch.int64) * 29 % 253).to(torch.uint8).reshape(4, 40, 48, 3).cuda()
    idx = [0, 1, 1, 2, 3]
    both("frontend.prepare_clip", lambda: frontend.prepare_clip(raw, 24, 3, 5, True, 16, idx))
    case("frontend.prepare_clip_shake_no_imgs", lambda: frontend.prepare_clip(raw, 24, 3, 5, False, 16, idx, all_di=[0, 1, 2, 1, 0], all_dj=[2, 1, 0, 1, 2],
                                                                                want_imgs=False))
    case("frontend.prepare_clip_bgr_out", lambda: frontend.prepare_clip(raw, 24, 3, 5, False, 16, idx, color_mode="gray_in_bgr_out"))
    raw_b = torch.stack([raw, raw.flip(0)])
    table = [[3, 5, 24, 1], [0, 0, 32, 0]]
    case("frontend.prepare_clips_batch", lambda: frontend.prepare_clips_batch(raw_b, table, [idx, idx[::-1]], 16))
    case("frontend.prepare_clips_batch_imgs", lambda: frontend.prepare_clips_batch(raw_b, table, [idx, idx[::-1]], 16, color_mode="gray_in_bgr_out", want_imgs=True))
    pinned = raw_b.cpu().pin_memory()
    case("frontend.prepare_clips_batch_pinned_host", lambda: frontend.prepare_clips_batch(pinned, table, [idx, idx[::-1]], 16))

    src = esim.synth_clips(2, 4, 8, 12, dtype=torch.uint8, seed=9)
    both("loader.clip_frames_f32", lambda: loader.clip_frames_f32(src))
    case("loader.clip_frames_f32_pick", lambda: loader.clip_frames_f32(src, pick=[0, 2, 3]))
    case("loader.clip_frames_f32_first_frames", lambda: loader.clip_frames_f32(src, frames=2))
    pick = torch.tensor([[0, 3, 1], [4, 2, 0]], dtype=torch.int32, device="cuda")
    case("loader.clip_frames_packed", lambda: loader.clip_frames_packed(flat_clips, offs, pick, 16, 16))
    case("loader.clip_frames_packed_stored_frames", lambda: loader.clip_frames_packed(flat_clips, offs, pick, 16, 16, stored_frames=stored))

    # ---- networks, launch by launch -------------------------------------------------------------------------------------------------------------
    ev = torch.from_numpy(sparse_voxels(41, N, T, 5, H, W)).cuda()
    e2_kw = lambda block: kwargs(block, num_output_channels=1)   # noqa: E731

    def seeded(net, seed=7):
        load_seeded(net, seed)
        return net.cuda().eval()

    def hyper():
        net = HyperE2VID(dict(HYPER_KW)).cuda().eval()
        net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in g26_state(g26()).items()}, strict=True)
        return net

    nets = {"e2vid_convlstm": lambda: seeded(E2VIDRecurrent(e2_kw("convlstm"))), "firenet": lambda: seeded(FireNet()),
            "evflownet": lambda: seeded(EVFlowNet(dict(num_bins=5))), "hyper": hyper}

    def states_of(net):
        st_ = {"states": getattr(net, "states", None)}
        if hasattr(net, "prev_recs"):
            st_["prev_recs"] = net.prev_recs
        return st_

    with torch.no_grad():
        for name, make in nets.items():
            net = make()

            def loop():
                net.reset_states()
                outs = [net(ev[:, t]) for t in range(T)]
                return {"out": outs, **states_of(net)}

            def seq():
                net.reset_states()
                return {"out": net.forward_sequence(ev), **states_of(net)}
            case(f"infer.{name}.loop", loop)
            case(f"infer.{name}.seq", seq)
            if name == "e2vid_convlstm":
                case(f"infer.{name}.seq@side_stream", seq, on_side=True)
            del net

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
    case("train.evflownet", train_case(lambda: seeded(EVFlowNet(dict(num_bins=5), trainable=True)), 2))

    # ---- losses and LPIPS -------------------------------------------------------------------------------------------------------------------------
    pa = {k: torch.from_numpy(v).cuda() for k, v in loss_inputs.pair_inputs("b").items()}
    pair = (pa["image0"], pa["image1"], pa["processed0"], pa["processed1"], pa["flow01"])
    n_pair = pa["image0"].shape[0]
    both("loss.warp_bilinear", lambda: loss_ops.warp_bilinear(pa["image0"], pa["flow01"]))
    case("loss.warp_bilinear_adjoint", lambda: loss_ops.warp_bilinear_adjoint(pa["processed0"], pa["flow01"]))
    gout = torch.ones((3, n_pair), device="cuda")
    for tag, wts in (("tc", (1.0, 0.0, 0.0)), ("all", (0.5, 1.0, 2.0)), ("no_tc", (0.0, 1.0, 1.0))):
        case(f"loss.tc_loss_fwd_{tag}", lambda wts=wts: loss_ops.tc_loss_fwd(*pair, weights=wts))
        case(f"loss.tc_loss_bwd_{tag}", lambda wts=wts: loss_ops.tc_loss_bwd(*pair, gout, weights=wts))
    case("loss.tc_loss_fwd_no_tc_none_inputs", lambda: loss_ops.tc_loss_fwd(None, pair[1], None, pair[3], None, weights=(0.0, 1.0, 1.0)))
    case("loss.tc_loss_fwd_output_images", lambda: loss_ops.tc_loss_fwd(*pair, output_images=True))
    sq = {k: torch.from_numpy(v).cuda() for k, v in loss_inputs.seq_inputs().items()}
    sb, st_len = sq["pred"].shape[:2]
    gseq = torch.ones((3, sb, st_len), device="cuda")
    for L0 in (1, 2, st_len):
        case(f"loss.seq_loss_fwd_L0_{L0}", lambda L0=L0: loss_ops.seq_loss_fwd(sq["pred"], sq["frame"], sq["flow"], L0))
        case(f"loss.seq_loss_bwd_L0_{L0}", lambda L0=L0: loss_ops.seq_loss_bwd(sq["pred"], sq["frame"], sq["flow"], L0, gseq))
    case("loss.seq_loss_fwd_no_tc", lambda: loss_ops.seq_loss_fwd(sq["pred"], sq["frame"], sq["flow"], 2, weights=(0.0, 1.0, 1.0)))

    lx = rand(2, 3, 16, 16)
    lw, lb = rand(64, 3, 3, 3, lo=-0.2, hi=0.2), rand(64, lo=-0.1, hi=0.1)
    shift, scale = torch.tensor([-0.030, -0.088, -0.188], device="cuda"), torch.tensor([0.458, 0.448, 0.450], device="cuda")
    act = rand(2, 16, 16, 64, lo=-1.0).to(torch.bfloat16)
    act1 = rand(2, 16, 16, 64, lo=-1.0).to(torch.bfloat16)
    half = rand(2, 8, 8, 64, lo=-1.0).to(torch.bfloat16)
    both("lpips.stem", lambda: loss_ops.lpips_stem(lx, lw, lb, shift, scale, normalize=True))
    case("lpips.stem_one_channel_bf16_out", lambda: loss_ops.lpips_stem(lx[:, :1].to(torch.bfloat16), lw, lb, shift, scale,
                                                                          out=torch.empty((2, 16, 16, 64), dtype=torch.bfloat16, device="cuda")))
    case("lpips.stem_bwd", lambda: loss_ops.lpips_stem_bwd(act, lw, scale, 3, normalize=True))
    case("lpips.pool", lambda: loss_ops.lpips_pool(act))
    case("lpips.pool_bwd", lambda: loss_ops.lpips_pool_bwd(half, act))
    case("lpips.pool_bwd_dtap_relu", lambda: loss_ops.lpips_pool_bwd(half, act, dtap=act1, relu_mask=True))
    case("lpips.compare_fwd", lambda: loss_ops.lpips_compare_fwd(act, act1, rand(64), torch.zeros(2, device="cuda")))
    case("lpips.compare_bwd", lambda: loss_ops.lpips_compare_bwd(act, act1, rand(64), torch.ones(2, device="cuda")))

    # ---- metrics and NER-Net ------------------------------------------------------------------------------------------------------------------------
    mp, mi = (torch.from_numpy(v).cuda() for v in MR.image_case("i8x9"))
    both("metrics.image_metrics", lambda: metrics.image_metrics(mp, mi))
    case("metrics.image_metrics_ssim_map", lambda: metrics.image_metrics(mp, mi, ssim_map=True))
    case("metrics.image_metrics_T0", lambda: metrics.image_metrics(mp[:0], mi[:0], ssim_map=True))
    fp, fg, fe = (torch.from_numpy(np.repeat(v, 2, axis=0)).cuda()[::2] for v in MR.flow_case("f13x17"))   # every other frame of a twice as long tensor
    assert fp.stride(0) == 2 * fp[0].numel()
    case("metrics.flow_metrics_strided", lambda: metrics.flow_metrics(fp, fg, fe))
    case("metrics.flow_metrics_T0", lambda: metrics.flow_metrics(fp[:0], fg[:0], fe[:0]))

    Cb, nh, nw, nb = 5, 6, 7, 2
    ws_, bs_ = nernet_inputs.exact_mlp([1, 16, 16, 1], 4)
    ws_, bs_ = [w.cuda() for w in ws_], [b.cuda() for b in bs_]
    rows = nernet_inputs.exact_rows(1, 60, Cb, nb, nh, nw)
    rows2 = torch.cat([nernet_inputs.exact_rows(2, 30, Cb, nb, nh, nw), nernet_inputs.exact_rows(3, 30, Cb, nb, nh, nw)])
    lv = lambda events, **kw: nernet.learned_voxel(events, ws_, bs_, (Cb, nh, nw), nernet_inputs.SLOPE, **kw)   # noqa: E731
    both("nernet.learned_voxel", lambda: lv(rows, batch_size=nb))
    case("nernet.learned_voxel_batch_from_rows_normalize", lambda: lv(rows, normalize=True))
    case("nernet.learned_voxel_n0", lambda: lv(rows[:0], batch_size=nb))
    case("nernet.learned_voxel_n0_return_t", lambda: lv(rows[:0], batch_size=nb, return_t=True))
    case("nernet.learned_voxel_offsets", lambda: lv(rows2, batch_size=nb, offsets=[0, 30, 60]))
    case("nernet.learned_voxel_return_t", lambda: lv(rows, batch_size=nb, return_t=True))
    case("nernet.learned_voxel_combined", lambda: lv(rows.float(), batch_size=nb, combined=True))

    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    torch.save({"tensors": tensors, "calls": calls}, out_path)
    print(f"{which}: {len(calls)} cases, {sum(1 for k in tensors if not k.endswith('#meta'))} tensors, "
          f"{sum(len(v) for v in calls.values())} library calls -> {out_path}", flush=True)


def compare(out_jsonl):
    import torch
    for needed in (os.path.join(PARENT, "v2v_amd", "_lib.py"), os.path.join(PARENT, "v2v_amd", "libv2v_hip.so")):
        if not os.path.exists(needed):
            print(f"{needed} is missing.  Set the parent package up first:\n"
                  f"    mkdir -p {PARENT} && git archive <parent> v2v_amd | tar -x -C {PARENT}\n"
                  f"    cp {os.path.join(ROOT, 'v2v_amd', 'libv2v_hip.so')} {os.path.join(PARENT, 'v2v_amd')}/      # or build it there: make -C v2v_amd/csrc",
                  flush=True)
            return 2
    os.makedirs(os.path.dirname(os.path.abspath(out_jsonl)), exist_ok=True)
    tmp = tempfile.mkdtemp()
    paths = {}
    for which in ("parent", "new"):
        paths[which] = os.path.join(tmp, f"ab_calls_{which}.pt")
        rc = subprocess.call(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "run", which, paths[which]])
        if rc != 0:
            print(f"{which}: child ended with {rc}; stopping", flush=True)
            return rc
    a, b = torch.load(paths["parent"]), torch.load(paths["new"])
    bad = 0
    with open(out_jsonl, "w") as f:
        for name in sorted(set(a["calls"]) | set(b["calls"])):
            ca, cb = a["calls"].get(name), b["calls"].get(name)
            keys = sorted(k for k in set(a["tensors"]) | set(b["tensors"]) if k.split("#")[0] == name or k.startswith(name + "."))
            n_t = n_diff = 0
            for k in keys:
                va, vb = a["tensors"].get(k), b["tensors"].get(k)
                if k.endswith("#meta"):
                    same = va == vb
                else:
                    n_t += 1
                    same = va is not None and vb is not None and va.shape == vb.shape and torch.equal(va, vb)
                if not same:
                    n_diff += 1
                    print("DIFFERENT", k, va if k.endswith("#meta") else "", vb if k.endswith("#meta") else "", flush=True)
            if ca != cb:
                for i, (ra, rb) in enumerate(zip(ca or [], cb or [])):
                    if ra != rb:
                        print("CALL DIFFERS", name, i, json.dumps(ra), json.dumps(rb), flush=True)
                        break
            hip = [r for r in (cb or []) if r["name"].endswith("_hip")]
            row = {"case": name, "tensors": n_t, "different": n_diff, "calls_parent": len(ca or []), "calls_new": len(cb or []),
                   "launches": len(hip), "streams_current": all(r["stream_is_current"] for r in hip), "call_lists_identical": ca == cb,
                   "raised": next((v for k, v in b["tensors"].items() if k == name + ".raised#meta"), None)}
            bad += n_diff + (ca != cb) + (not row["streams_current"])
            f.write(json.dumps(row) + "\n")
            print(json.dumps(row), flush=True)
    for p in paths.values():
        os.remove(p)
    print("RESULT:", "every tensor bit-identical, every call list identical" if bad == 0 else f"{bad} DEFECTS", flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2], sys.argv[3])
    else:
        sys.exit(compare(sys.argv[2]))
