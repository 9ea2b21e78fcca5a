"""Golden G28 (tests/golden/g28_firenet.npz): the reference's FireNet (model/model.py:264-311) run in float32 on the CPU, in eval mode, on
seeded weights.

    python tests/golden/make_golden_firenet.py REFERENCE_DIR        (the reference checkout; or V2V_REFERENCE in the environment)

Weights are a recipe (tests/seeded_weights.py; seed 2801, gain 2.5 -- the image and both states stay O(0.1 .. 1), their standard deviations
are printed); two inputs of sparse integer voxels like G18's (tests/firenet_stock.py: SHAPES): `a` = 4 steps of [2, 5, 32, 48] (voxel seed
2828) and `b` = 2 steps of the odd-sized [1, 5, 19, 37] (voxel seed 2829: an odd pixel count, partial tiles on both axes).  Stored: the
state_dict's key list and shapes; per input the images, the two final states, and -- the yardstick of the GPU tests -- per step the
(max, rms) error of the reference's OWN network under CPU bf16 autocast against its float32 self, and the same for the final states
(asserted non-zero here).  Only arrays go into the file.  Regenerates byte for byte."""
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

from firenet_stock import INPUTS, SHAPES  # noqa: E402
from convgru_stock import sparse_voxels  # noqa: E402
from seeded_weights import load_seeded  # noqa: E402

SEED, GAIN, VOX_SEED = 2801, 2.5, 2828


def err(a, b):
    d = (a.double() - b.double()).abs()
    return np.array([float(d.max()), float((d ** 2).mean().sqrt())])


def run(net, vox):
    net.reset_states()
    imgs = [net(vox[t])["image"].float() for t in range(vox.shape[0])]
    return imgs, [s.float() for s in net.states]


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    with contextlib.redirect_stdout(io.StringIO()):
        import model.model as mm
        net = mm.FireNet().eval()
    load_seeded(net, SEED, gain=GAIN)
    sd = net.state_dict()
    out = dict(net__seed=np.array(SEED), net__gain=np.array(GAIN), net__vox_seed=np.array(VOX_SEED), net__keys=np.array(list(sd)),
               net__shapes=np.array([",".join(map(str, v.shape)) for v in sd.values()]))
    with torch.no_grad():
        for i, name in enumerate(INPUTS):
            x = torch.from_numpy(sparse_voxels(VOX_SEED + i, *SHAPES[name]))
            img, st = run(net, x)
            with torch.autocast("cpu", dtype=torch.bfloat16):
                img16, st16 = run(net, x)
            e_img = np.stack([err(a, b) for a, b in zip(img16, img)])
            e_st = np.stack([err(a, b) for a, b in zip(st16, st)])
            assert (e_img > 0).all() and (e_st > 0).all()
            out.update({f"{name}__image": torch.stack(img).numpy(), f"{name}__states": torch.stack(st).numpy(),
                        f"{name}__bf16_autocast_err_image": e_img, f"{name}__bf16_autocast_err_states": e_st})
            print(f"g28 {name}: {len(sd)} keys, image std {[round(float(v.std()), 3) for v in img]}, final state std "
                  f"{[round(float(s.std()), 3) for s in st]}, reference bf16-autocast error image {e_img.tolist()} states {e_st.tolist()}")
    path = os.path.join(HERE, "g28_firenet.npz")
    np.savez_compressed(path, **out)
    print(f"g28_firenet.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
