"""Golden G25 (tests/golden/g25_evflow.npz): the reference's flow network EVFlowNet (model/model.py:226-261) = model/unet.py:UNet
(:313-352) with EVFlowNet's hard-coded kwargs, run in float32 on the CPU on seeded weights, plus its two new single layers.

    python tests/golden/make_golden_evflow.py REFERENCE_DIR        (the reference checkout; or V2V_REFERENCE in the environment)

model/model.py imports cv2 through utils, so the network is built from model.unet.UNet directly with the hard-coded kwargs (that IS
the network) and its keys are stored with the `unet.` prefix EVFlowNet gives them.  Weights are a recipe (tests/seeded_weights.py, seed
2501, gain 2.4: flow std ~0.7 -- gain 1.7 gives std 0.24, too small to tell a dead decoder from a live one); the input is sparse integer
voxels like G18's.  Stored as the yardstick of the GPU tests: flow__bf16_autocast_err = (max, rms) of the reference's OWN network under
CPU bf16 autocast against its float32 self on the same input.  Regenerates byte for byte."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("V2V_REFERENCE")
if not REF:
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REF)

from seeded_weights import load_seeded, seeded_input  # noqa: E402
import model.submodules as sm  # noqa: E402
import model.unet as un  # noqa: E402

KW = dict(num_bins=5, base_num_channels=32, num_encoders=4, num_residual_blocks=2, num_output_channels=2, skip_type="concat", norm=None,
          use_upsample_conv=True, kernel_size=3, channel_multiplier=2)                      # model/model.py:234-245
SEED, GAIN = 2501, 2.4


def err(a, b):
    d = (a.double() - b.double()).abs()
    return np.array([float(d.max()), float((d ** 2).mean().sqrt())])


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    out = {}
    with torch.no_grad():
        with contextlib.redirect_stdout(io.StringIO()):
            net = un.UNet(dict(KW)).eval()
        probe = load_seeded(net, SEED, gain=GAIN)
        g = np.random.Generator(np.random.PCG64(2525))
        vox = g.integers(-3, 4, size=(2, 5, 64, 64)).astype(np.float32)
        vox[g.random(vox.shape) < 0.6] = 0.0                                               # sparse, like event counts
        x = torch.from_numpy(vox)
        flow = net(x)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            flow16 = net(x)
        sd = net.state_dict()
        out.update(evflow__vox=vox.astype(np.int8), evflow__flow=flow.numpy(), evflow__seed=np.array(SEED), evflow__gain=np.array(GAIN),
                   evflow__keys=np.array(["unet." + k for k in sd]), evflow__shapes=np.array([",".join(map(str, v.shape)) for v in sd.values()]),
                   evflow__n_params=np.array(sum(v.numel() for v in sd.values())),
                   evflow__weight_probe=np.concatenate([probe[k].ravel()[:3] for k in list(probe)[::5]]),
                   flow__bf16_autocast_err=err(flow16.float(), flow))
        print(f"g25 evflow: {len(sd)} keys, {int(out['evflow__n_params'])} parameters, flow std {float(flow.std()):.3f}, range "
              f"{float(flow.min()):.2f} .. {float(flow.max()):.2f}, reference bf16-autocast error {out['flow__bf16_autocast_err']}")
        # the stem: ConvLayer(5, 64, 3, stride 2, padding 1)
        m = sm.ConvLayer(5, 64, 3, stride=2, padding=1).eval()
        load_seeded(m, 2502)
        xs = seeded_input(25020, 2, 5, 32, 32)
        out.update(stem__seed=np.array(2502), stem__x_seed=np.array(25020), stem__x_shape=np.array(xs.shape), stem__y=m(torch.from_numpy(xs)).numpy())
        # the last concat decoder: UpsampleConvLayer(128, 32, 3, padding 1) on cat(x, skip)
        m = sm.UpsampleConvLayer(128, 32, 3, padding=1).eval()
        load_seeded(m, 2503)
        xd, xk = seeded_input(25030, 2, 64, 16, 16), seeded_input(25031, 2, 64, 16, 16)
        out.update(catdec__seed=np.array(2503), catdec__x_seeds=np.array([25030, 25031]), catdec__x_shape=np.array(xd.shape),
                   catdec__y=m(torch.cat([torch.from_numpy(xd), torch.from_numpy(xk)], 1)).numpy())
    path = os.path.join(HERE, "g25_evflow.npz")
    np.savez_compressed(path, **out)
    print(f"g25_evflow.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
