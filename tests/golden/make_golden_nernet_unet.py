"""Golden G36 (tests/golden/g36_nernet_unet.npz): the reference's UNetNIAM_STcell_GCB (model/nernet/unet.py:139-238, the recurrent network
of config/test_nernet_original.yaml) run in float32 on the CPU, in eval mode, on seeded weights.

    python tests/golden/make_golden_nernet_unet.py REFERENCE_DIR        (the reference checkout; or V2V_REFERENCE in the environment)

Weights are a recipe (tests/seeded_weights.py: seed and gain below, every tensor of the state_dict, LayerNorm and PReLU weights
included), the input is a recipe too (tests/nernet_unet_stock.py:sparse_events: real-valued event tensors, 60 % zeros).
  case A   1 x 10 x 40 x 56, T = 4: the deepest level is 5 x 7, so the device runs it on a canvas larger than the frame
  case B   2 x 10 x 48 x 64, T = 3: batch 2, canvas = frame
Stored per case and step: `image`, and -- the yardstick of the GPU tests -- the (max, rms) error of the reference's OWN network under CPU
bf16 autocast against its float32 self.  Case A also stores h_t, c_t (three levels) and m_t after the last step, each with its own
autocast error, so that a failure can be localised; these state arrays keep the upper 24 bits of every float32 (relative error < 7e-5,
two orders below the bars they serve) so that the file stays below 830 KB.  Plus the state_dict's key list and shapes.
The generator asserts that the fixture is not degenerate: image rms >= 0.05 at every step; at the last step of either case no gate of any
cell (i, f, g, i', f', g', o, as |tanh| for g) has a mean within 0.02 of 0 or 1; the softmax of every context block is neither uniform nor
one-hot (largest weight between 2 / (H W) and 0.5).  Only arrays go into the file.  Regenerates byte for byte."""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("V2V_REFERENCE")
if not REF:
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)
for m in ("cv2", "h5py", "ffmpeg", "torchvision", "torchvision.transforms", "matplotlib", "matplotlib.pyplot"):   # absent here; only IO code touches them
    sys.modules.setdefault(m, types.ModuleType(m))

from nernet_unet_stock import KWARGS, sparse_events  # noqa: E402
from seeded_weights import seeded_state  # noqa: E402

SEED, GAIN = 3601, 2.2
CASES = {"a": (36011, (4, 1, 10, 40, 56)), "b": (36012, (3, 2, 10, 48, 64))}


def seeded_tensors(shapes, seed=SEED, gain=GAIN):
    return {k: torch.from_numpy(v) for k, v in seeded_state(shapes, seed, gain).items()}


def err(a, b):
    d = (a.double() - b.double()).abs()
    return np.array([float(d.max()), float((d ** 2).mean().sqrt())])


def keep24(t):
    return (t.contiguous().numpy().view(np.int32) & np.int32(-256)).view(np.float32)


def run(net, xs):
    net.states = None
    return [net(xs[t])["image"].float() for t in range(xs.shape[0])]


def states(net):
    return [t.float() for t in net.h_t] + [t.float() for t in net.c_t] + [net.m_t.float()]


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    with contextlib.redirect_stdout(io.StringIO()):
        import model.nernet.unet as nu
        net = nu.UNetNIAM_STcell_GCB(dict(KWARGS)).eval()
    sd = net.state_dict()
    net.load_state_dict(seeded_tensors({k: tuple(v.shape) for k, v in sd.items()}))
    out = dict(seed=np.array(SEED), gain=np.array(GAIN), keys=np.array(list(sd)), shapes=np.array([",".join(map(str, v.shape)) for v in sd.values()]))
    seen = {}
    for i, enc in enumerate(net.encoders):
        enc.recurrent_block.register_forward_pre_hook(lambda mod, args, i=i: seen.__setitem__(("cell", i), [a.float() for a in args]))
        enc.GCB.conv_mask.register_forward_hook(lambda mod, args, res, i=i: seen.__setitem__(("mask", i), res.float()))
    with torch.no_grad():
        for name, (in_seed, shape) in CASES.items():
            xs = torch.from_numpy(sparse_events(in_seed, *shape))
            img = run(net, xs)
            st = states(net)
            for i, enc in enumerate(net.encoders):          # the gates of the last step, recomputed from the cell's own convolutions on its inputs
                x, h, c, m = seen[("cell", i)]
                cell = enc.recurrent_block
                gx, gh, gm = cell.conv_x(x).chunk(7, 1), cell.conv_h(h).chunk(4, 1), cell.conv_m(m).chunk(3, 1)
                gates = {"i": torch.sigmoid(gx[0] + gh[0]), "f": torch.sigmoid(gx[1] + gh[1] + 1), "g": torch.tanh(gx[2] + gh[2]).abs(),
                         "i'": torch.sigmoid(gx[3] + gm[0]), "f'": torch.sigmoid(gx[4] + gm[1] + 1), "g'": torch.tanh(gx[5] + gm[2]).abs()}
                gates["f_lag"] = torch.sigmoid(gates["f"] - torch.exp(torch.sigmoid(cell.LAG_conv(x))) * gates["i"])
                means = {k: round(float(v.mean()), 3) for k, v in gates.items()}
                assert all(0.02 < v < 0.98 for v in means.values()), (name, i, means)
                w = torch.softmax(seen[("mask", i)].flatten(1), 1)
                hw = w.shape[1]
                assert 2.0 / hw < float(w.max(1).values.min()) and float(w.max()) < 0.5, (name, i, float(w.max()), hw)
                print(f"g36 {name} encoder {i}: gate means {means}, largest pooling weight {float(w.max()):.4f} (uniform {1 / hw:.4f})")
            with torch.autocast("cpu", dtype=torch.bfloat16):
                img16 = run(net, xs)
                st16 = states(net)
            e_img = np.stack([err(a, b) for a, b in zip(img16, img)])
            rms = [float((i ** 2).mean().sqrt()) for i in img]
            assert min(rms) >= 0.05 and (e_img > 0).all(), rms
            out.update({f"{name}__in_seed": np.array(in_seed), f"{name}__in_shape": np.array(shape), f"{name}__image": torch.stack(img).numpy(),
                        f"{name}__bf16_autocast_err_image": e_img})
            print(f"g36 {name}: image rms {[round(r, 3) for r in rms]}, reference bf16-autocast error {e_img.tolist()}")
            if name == "a":
                for key, t, t16 in zip(["h0", "h1", "h2", "c0", "c1", "c2", "m"], st, st16):
                    out[f"a__state_{key}"] = keep24(t)
                    out[f"a__bf16_autocast_err_{key}"] = err(t16, t)
                    print(f"g36 a state {key}: rms {float((t ** 2).mean().sqrt()):.3f}, autocast error {out[f'a__bf16_autocast_err_{key}'].tolist()}")
    path = os.path.join(HERE, "g36_nernet_unet.npz")
    np.savez_compressed(path, **out)
    print(f"g36_nernet_unet.npz: {os.path.getsize(path) / 1024:.1f} KiB")
    assert os.path.getsize(path) < 830 * 1024


if __name__ == "__main__":
    main()
