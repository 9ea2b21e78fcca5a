"""Golden G27 (tests/golden/g27_flownet_convgru.npz): the reference's FlowNet (model/model.py:111-139: UNetFlow, the recurrent UNet with a
3-channel prediction -- the E2VID+ network of config/test_e2vid++_original.yaml) run in float32 on the CPU, in eval mode, on seeded weights,
once per recurrent block type ('convlstm', 'convgru'); plus one bare ConvGRU(64, 64, 3) (model/submodules.py:238-278) over 4 steps.

    python tests/golden/make_golden_flownet.py REFERENCE_DIR        (the reference checkout; or V2V_REFERENCE in the environment)

Weights are a recipe (tests/seeded_weights.py; network seed 2701, gain 1.6 for both block types -- image and flow stay O(1) over the three
steps, their standard deviations are printed; bare cell seed 2702, gain 3.0, so that its gates leave the linear range); the input is
sparse integer voxels like G18's, [3, 2, 5, 64, 64].  Stored per block type: per step `image` and `flow`, the state_dict's key list and
shapes, and -- the yardstick of the GPU tests -- per step the (max, rms) error of the reference's OWN network under CPU bf16 autocast
against its float32 self, for image and for flow (asserted non-zero here).  Only arrays go into the file.  Regenerates byte for byte."""
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
for m in ("cv2", "h5py", "ffmpeg", "torchvision", "torchvision.transforms"):   # absent here; only IO / augmentation code touches them
    sys.modules.setdefault(m, types.ModuleType(m))

from convgru_stock import BLOCKS, kwargs, sparse_voxels  # noqa: E402
from seeded_weights import load_seeded, seeded_input  # noqa: E402

SEED, GAIN, CELL_SEED, CELL_GAIN, VOX_SEED = 2701, 1.6, 2702, 3.0, 2727


def err(a, b):
    d = (a.double() - b.double()).abs()
    return np.array([float(d.max()), float((d ** 2).mean().sqrt())])


def run(net, vox):
    net.reset_states()
    outs = [net(vox[t]) for t in range(vox.shape[0])]
    return [o["image"].float() for o in outs], [o["flow"].float() for o in outs]


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    with contextlib.redirect_stdout(io.StringIO()):
        import model.model as mm
        import model.submodules as sm
    out = dict(net__seed=np.array(SEED), net__gain=np.array(GAIN), net__vox_seed=np.array(VOX_SEED))
    vox = sparse_voxels(VOX_SEED, 3, 2, 5, 64, 64)
    out["net__vox"] = vox.astype(np.int8)
    x = torch.from_numpy(vox)
    with torch.no_grad():
        for block in BLOCKS:
            with contextlib.redirect_stdout(io.StringIO()):
                net = mm.FlowNet(kwargs(block)).eval()
            load_seeded(net, SEED, gain=GAIN)
            sd = net.state_dict()
            img, flow = run(net, x)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                img16, flow16 = run(net, x)
            e_img, e_flow = np.stack([err(a, b) for a, b in zip(img16, img)]), np.stack([err(a, b) for a, b in zip(flow16, flow)])
            assert (e_img > 0).all() and (e_flow > 0).all()
            out.update({f"{block}__image": torch.stack(img).numpy(), f"{block}__flow": torch.stack(flow).numpy(),
                        f"{block}__keys": np.array(list(sd)), f"{block}__shapes": np.array([",".join(map(str, v.shape)) for v in sd.values()]),
                        f"{block}__bf16_autocast_err_image": e_img, f"{block}__bf16_autocast_err_flow": e_flow})
            print(f"g27 {block}: {len(sd)} keys, image std {[round(float(i.std()), 3) for i in img]}, flow std {[round(float(i.std()), 3) for i in flow]}, "
                  f"reference bf16-autocast error image {e_img.tolist()} flow {e_flow.tolist()}")
        cell = sm.ConvGRU(64, 64, 3).eval()
        load_seeded(cell, CELL_SEED, gain=CELL_GAIN)
        xs = torch.relu(torch.from_numpy(seeded_input(27020, 4, 2, 64, 8, 16)))
        h, states = None, []
        for t in range(4):
            h = cell(xs[t], h)
            states.append(h)
        csd = cell.state_dict()
        out.update(cell__seed=np.array(CELL_SEED), cell__gain=np.array(CELL_GAIN), cell__x_seed=np.array(27020), cell__keys=np.array(list(csd)),
                   cell__shapes=np.array([",".join(map(str, v.shape)) for v in csd.values()]), cell__states=torch.stack(states).numpy())
        print(f"g27 cell: state std {[round(float(s.std()), 3) for s in states]}, |max| {float(torch.stack(states).abs().max()):.3f}")
    path = os.path.join(HERE, "g27_flownet_convgru.npz")
    np.savez_compressed(path, **out)
    print(f"g27_flownet_convgru.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
