"""Golden G26 (tests/golden/g26_hyper.npz): the reference's HyperE2VID (model/hyper_model.py: the recurrent E2VID network whose
decoders[0] is the per-pixel dynamic DynamicUpsampleLayer) run in float32 on the CPU, in eval mode, on seeded weights; plus one
DynamicUpsampleLayer on its own with its context and atoms.

    python tests/golden/make_golden_hyper.py REFERENCE_DIR        (the reference checkout; or V2V_REFERENCE in the environment)

Weights are a recipe (tests/hyper_weights.py on tests/seeded_weights.py; network seed 2601, gain 1.7 -- gain 2.4 makes the image feedback
through prev_recs blow up over three steps; layer seed 2602, gain 1.0, compositional coefficients x 1/32 so that its output stays O(1)); the input is sparse integer voxels
like G18's.  Stored as yardsticks of the GPU tests: per step the (max, rms) error of the reference's OWN network under CPU bf16 autocast
against its float32 self (states and prev_recs carried by each run itself), and feedback_effect = max |image_1 - image_1 with prev_recs
zeroed before step 1|.  Large layer intermediates (context, atoms) are stored for the first image only.  Regenerates byte for byte."""
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

from hyper_weights import load_hyper  # noqa: E402
from seeded_weights import seeded_input  # noqa: E402
import model.hyper_model as hm  # noqa: E402

KW = dict(num_bins=5, skip_type="sum", recurrent_block_type="convlstm", kernel_size=5, channel_multiplier=2, num_encoders=3,
          base_num_channels=32, num_residual_blocks=2, use_upsample_conv=True, norm="none", num_output_channels=1,
          use_dynamic_decoder=True)                                                       # config/train_v2v_hyper_10k.yaml:21-33
SEED, GAIN, LAYER_SEED, LAYER_GAIN, LAYER_COEFF_SCALE = 2601, 1.7, 2602, 1.0, 1.0 / 32


def err(a, b):
    d = (a.double() - b.double()).abs()
    return np.array([float(d.max()), float((d ** 2).mean().sqrt())])


def run(net, vox, zero_prev_before=None):
    net.reset_states()
    imgs = []
    for t in range(vox.shape[0]):
        if zero_prev_before == t:
            net.prev_recs = torch.zeros_like(net.prev_recs)
        imgs.append(net(vox[t])["image"].float())
    return imgs


def main():
    torch.manual_seed(0)
    torch.set_num_threads(4)
    out = {}
    with torch.no_grad():
        with contextlib.redirect_stdout(io.StringIO()):
            net = hm.HyperE2VID(dict(KW)).eval()
        probe = load_hyper(net, SEED, gain=GAIN)
        sd = net.state_dict()
        g = np.random.Generator(np.random.PCG64(2626))
        vox = g.integers(-3, 4, size=(3, 2, 5, 64, 64)).astype(np.float32)
        vox[g.random(vox.shape) < 0.6] = 0.0                                              # sparse, like event counts
        x = torch.from_numpy(vox)
        imgs = run(net, x)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            imgs16 = run(net, x)
        cut = run(net, x, zero_prev_before=1)
        out.update(net__vox=vox.astype(np.int8), net__images=torch.stack(imgs).numpy(), net__seed=np.array(SEED), net__gain=np.array(GAIN),
                   net__keys=np.array(list(sd)), net__shapes=np.array([",".join(map(str, v.shape)) for v in sd.values()]),
                   net__n_elems=np.array(sum(v.numel() for v in sd.values())),
                   net__weight_probe=np.concatenate([np.asarray(probe[k], dtype=np.float32).ravel()[:3] for k in list(probe)[::5]]),
                   net__bf16_autocast_err=np.stack([err(a, b) for a, b in zip(imgs16, imgs)]),
                   feedback_effect=np.array(float((imgs[1] - cut[1]).abs().max())),
                   bases=sd["unetrecurrent.decoders.0.dynamic_atom_generation.bases"].numpy())
        print(f"g26 hyper: {len(sd)} keys, {int(out['net__n_elems'])} state elements, image std {[round(float(i.std()), 3) for i in imgs]}, "
              f"reference bf16-autocast error {out['net__bf16_autocast_err'].tolist()}, feedback effect {float(out['feedback_effect']):.3f}")
        # one DynamicUpsampleLayer(256, 128, 5, padding 2, 6 fused channels)
        m = hm.DynamicUpsampleLayer(256, 128, 5, padding=2, in_fuse_channels=6).eval()
        load_hyper(m, LAYER_SEED, gain=LAYER_GAIN, coeff_scale=LAYER_COEFF_SCALE)
        lx, lev, lprev = seeded_input(26020, 2, 256, 8, 8), seeded_input(26021, 2, 5, 64, 64), seeded_input(26022, 2, 1, 64, 64)
        ctx = m.context_fusion(torch.from_numpy(lev), torch.from_numpy(lprev))
        atoms = m.dynamic_atom_generation(ctx)
        y = m(torch.from_numpy(lx), torch.from_numpy(lev), torch.from_numpy(lprev))
        lsd = m.state_dict()
        out.update(layer__seed=np.array(LAYER_SEED), layer__gain=np.array(LAYER_GAIN), layer__coeff_scale=np.array(LAYER_COEFF_SCALE), layer__x_seeds=np.array([26020, 26021, 26022]),
                   layer__keys=np.array(list(lsd)), layer__shapes=np.array([",".join(map(str, v.shape)) for v in lsd.values()]),
                   layer__context=ctx[:1].numpy(), layer__atoms=atoms[:1].numpy(), layer__y=y.numpy())
        print(f"g26 layer: context |max| {float(ctx.abs().max()):.2f}, atoms |max| {float(atoms.abs().max()):.2f}, output |max| "
              f"{float(y.abs().max()):.2f} std {float(y.std()):.3f}")
    path = os.path.join(HERE, "g26_hyper.npz")
    np.savez_compressed(path, **out)
    print(f"g26_hyper.npz: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
