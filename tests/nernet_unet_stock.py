"""NER-Net's recurrent network (UNetNIAM_STcell_GCB of the reference, model/nernet/unet.py:139-238, in the configuration of
config/test_nernet_original.yaml) restated with torch.nn.functional on a dict keyed like the module's state_dict, written from the
network's formulas; plus the seeded input recipe of golden G36 and the crop arithmetic.  A helper module, not a test.  The restatement is
the yardstick wherever G36 does not reach (real frame sizes); tests/test_nernet_unet.py holds it to G36 at 1e-5 first.

    KWARGS                      the unet_kwargs of the shipped configuration
    state_shapes(num_bins)      ordered {state_dict key: shape} of the network, the reference's registration order
    step(sd, x, state)          one time step: x [B, 2 * num_bins, H, W] (H, W multiples of 8) -> (image [B,1,H,W], new state)
    run(sd, xs, autocast=False) a sequence from the zero state -> (list of images, last state)
    sparse_events(seed, ...)    G36's input recipe: real-valued event tensors, 60 % zeros
    crop_sizes(h, w)            (padded h, padded w, top, left): CropParameters(w, h, 3) in four integers
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

KWARGS = dict(num_bins=5, skip_type="sum", recurrent_network="NIAM_STcell_GCB", recurrent_block_type="", num_encoders=3, base_num_channels=32,
              num_residual_blocks=2, use_upsample_conv=True, norm="", crop_size=224, mlp_layers=[1, 50, 50, 50, 1], use_cnn_representation=True,
              normalize=False, combine_voxel=False, RepCNN_kernel_size=3, RepCNN_padding=1, RepCNN_channel=64, RepCNN_num_layers=1, num_output_channels=1)
WIDTHS = (32, 64, 128, 256)


def state_shapes(num_bins=5):
    s = {"head.conv2d.weight": (32, 2 * num_bins, 5, 5), "head.conv2d.bias": (32,)}
    for i in range(3):
        ci, co, r, p = WIDTHS[i], WIDTHS[i + 1], WIDTHS[i] // 4, f"encoders.{i}."
        s.update({p + "conv.conv2d.weight": (co, ci, 5, 5), p + "conv.conv2d.bias": (co,), p + "conv_mem.conv2d.weight": (co, ci, 5, 5),
                  p + "conv_mem.conv2d.bias": (co,), p + "recurrent_block.conv_x.0.weight": (7 * co, co, 3, 3),
                  p + "recurrent_block.conv_h.0.weight": (4 * co, co, 3, 3), p + "recurrent_block.conv_m.0.weight": (3 * co, co, 3, 3),
                  p + "recurrent_block.conv_o.0.weight": (co, 2 * co, 3, 3), p + "recurrent_block.conv_last.weight": (co, 2 * co, 1, 1),
                  p + "recurrent_block.LAG_conv.weight": (co, co, 1, 1), p + "conv_1x1.weight": (ci, ci, 1, 1), p + "conv_1x1.bias": (ci,),
                  p + "GCB.conv_mask.weight": (1, ci, 1, 1), p + "GCB.conv_mask.bias": (1,), p + "GCB.channel_add_conv.0.weight": (r, ci, 1, 1),
                  p + "GCB.channel_add_conv.0.bias": (r,), p + "GCB.channel_add_conv.1.weight": (r, 1, 1), p + "GCB.channel_add_conv.1.bias": (r, 1, 1),
                  p + "GCB.channel_add_conv.2.weight": (1,), p + "GCB.channel_add_conv.3.weight": (ci, r, 1, 1), p + "GCB.channel_add_conv.3.bias": (ci,)})
    for i in range(2):
        for c in ("conv1", "conv2"):
            s.update({f"resblocks.{i}.{c}.weight": (256, 256, 3, 3), f"resblocks.{i}.{c}.bias": (256,)})
    for name in ("decoders", "m_t_UpsampleLayer"):
        for i in range(3):
            s.update({f"{name}.{i}.conv2d.weight": (WIDTHS[2 - i], WIDTHS[3 - i], 5, 5), f"{name}.{i}.conv2d.bias": (WIDTHS[2 - i],)})
    s.update({"pred.conv2d.weight": (1, 32, 1, 1), "pred.conv2d.bias": (1,)})
    return s


def _gcb(sd, p, x):
    g = F.conv2d(x, sd[p + "conv_1x1.weight"], sd[p + "conv_1x1.bias"])
    w = torch.softmax(F.conv2d(g, sd[p + "GCB.conv_mask.weight"], sd[p + "GCB.conv_mask.bias"]).flatten(2), dim=2)          # [B,1,HW]
    ctx = torch.matmul(g.flatten(2).unsqueeze(1), w.unsqueeze(3)).reshape(g.shape[0], g.shape[1], 1, 1)
    q = p + "GCB.channel_add_conv."
    t = F.conv2d(ctx, sd[q + "0.weight"], sd[q + "0.bias"])
    t = F.prelu(F.layer_norm(t, t.shape[1:], sd[q + "1.weight"], sd[q + "1.bias"]), sd[q + "2.weight"])
    return x + g + F.conv2d(t, sd[q + "3.weight"], sd[q + "3.bias"])


def _nam(sd, p, x, h, c, m):
    xc, hc, mc = (F.conv2d(t, sd[p + f"conv_{k}.0.weight"], padding=1) for t, k in ((x, "x"), (h, "h"), (m, "m")))
    ix, fx, gx, ipx, fpx, gpx, ox = xc.chunk(7, 1)
    ih, fh, gh, oh = hc.chunk(4, 1)
    im, fm, gm = mc.chunk(3, 1)
    i_t = torch.sigmoid(ix + ih)
    f_t = torch.sigmoid(torch.sigmoid(fx + fh + 1.0) - torch.exp(torch.sigmoid(F.conv2d(x, sd[p + "LAG_conv.weight"]))) * i_t)
    c_new = f_t * c + i_t * torch.tanh(gx + gh)
    m_new = torch.sigmoid(fpx + fm + 1.0) * m + torch.sigmoid(ipx + im) * torch.tanh(gpx + gm)
    mem = torch.cat([c_new, m_new], 1)
    h_new = torch.sigmoid(ox + oh + F.conv2d(mem, sd[p + "conv_o.0.weight"], padding=1)) * torch.tanh(F.conv2d(mem, sd[p + "conv_last.weight"]))
    return h_new, c_new, m_new


def _up(sd, p, x):
    x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    return torch.relu(F.conv2d(x, sd[p + "conv2d.weight"], sd[p + "conv2d.bias"], padding=2))


def step(sd, x, state=None):
    """state: dict(h=[3], c=[3], m=tensor) or None (zero).  Returns (image, new state)."""
    b, _, hh, ww = x.shape
    if state is None:
        z = [torch.zeros((b, WIDTHS[i + 1], hh >> (i + 1), ww >> (i + 1)), dtype=x.dtype, device=x.device) for i in range(3)]
        state = dict(h=list(z), c=list(z), m=torch.zeros((b, 32, hh, ww), dtype=x.dtype, device=x.device))
    head = torch.relu(F.conv2d(x, sd["head.conv2d.weight"], sd["head.conv2d.bias"], padding=2))
    h, c, m, cur, ms = list(state["h"]), list(state["c"]), state["m"], head, []
    for i in range(3):
        p = f"encoders.{i}."
        xg = _gcb(sd, p, cur)
        xc = torch.relu(F.conv2d(xg, sd[p + "conv.conv2d.weight"], sd[p + "conv.conv2d.bias"], stride=2, padding=2))
        mc = torch.relu(F.conv2d(m, sd[p + "conv_mem.conv2d.weight"], sd[p + "conv_mem.conv2d.bias"], stride=2, padding=2))
        h[i], c[i], m = _nam(sd, p + "recurrent_block.", xc, h[i], c[i], mc)
        cur = h[i]
        ms.append(m)
    for i in range(3):
        m = _up(sd, f"m_t_UpsampleLayer.{i}.", m + ms[2 - i])
    y = cur
    for i in range(2):
        p = f"resblocks.{i}."
        t = torch.relu(F.conv2d(y, sd[p + "conv1.weight"], sd[p + "conv1.bias"], padding=1))
        y = torch.relu(F.conv2d(t, sd[p + "conv2.weight"], sd[p + "conv2.bias"], padding=1) + y)
    for i in range(3):
        y = _up(sd, f"decoders.{i}.", y + h[2 - i])
    img = F.conv2d(y + head, sd["pred.conv2d.weight"], sd["pred.conv2d.bias"])
    return img, dict(h=h, c=c, m=m)


def run(sd, xs, autocast=False):
    """xs [T,B,C,H,W] -> ([T] images float32, last state); autocast: bfloat16 autocast on xs's device"""
    state, imgs = None, []
    with torch.no_grad(), torch.autocast(xs.device.type, dtype=torch.bfloat16, enabled=autocast):
        for t in range(xs.shape[0]):
            img, state = step(sd, xs[t], state)
            imgs.append(img.float())
    return imgs, state


def sparse_events(seed, *shape):
    """real-valued event tensors with 60 % zeros: N(0,1) values kept where an independent uniform draw is above 0.6"""
    g = np.random.Generator(np.random.PCG64(int(seed)))
    v = g.standard_normal(shape).astype(np.float32)
    return v * (g.random(shape) > 0.6).astype(np.float32)


def crop_sizes(h, w):
    """frames are padded to multiples of 8 (three encoders), the larger half of the padding on top / left"""
    ph, pw = (h + 7) // 8 * 8, (w + 7) // 8 * 8
    return ph, pw, math.ceil(0.5 * (ph - h)), math.ceil(0.5 * (pw - w))
