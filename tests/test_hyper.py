"""HyperE2VID on the device kernels (v2v_amd.hyper): the per-pixel dynamic decoder (context staging, BatchNorm-folded bases_net, atoms, the
fused dynamic convolution) and the recurrent network around it.

Yardsticks.  Golden G26 (tests/golden/make_golden_hyper.py) = the reference's own HyperE2VID in float32, eval mode, on seeded weights
(tests/hyper_weights.py), three steps with the states and prev_recs carried, plus one DynamicUpsampleLayer with its context and atoms;
tests/hyper_stock.py restates layer and network in stock PyTorch and is pinned to G26 here on the CPU (1e-4).  Bars: the single layer
3e-2 max / 6e-3 rms (tests/test_unet_golden.py's single-layer bar) times max(1, |y|max) as tests/test_convlstm.py scales it; the network
at every step at most 2.5 x the reference's own CPU bf16-autocast error of that step stored in G26 (the factor tests/test_evflow.py uses
for the same yardstick); other sizes against hyper_stock in float32 on the same weights with the same network bar.  Each GPU test prints
its figures before it asserts.  The six kernels one by one, bit-exact at ragged shapes: tests/test_hyper_ops.py."""
import ctypes as C

import numpy as np
import pytest

from hyper_stock import KW, LAYER, err, g26 as load_g26, g26_layer_state, g26_state, sparse_voxels, stock_sequence
from seeded_weights import seeded_input

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def g26():
    return load_g26()


# ---- no GPU needed ----------------------------------------------------------------------------------------------------------------
def test_package_network_has_the_reference_state_dict(g26):
    import torch
    from v2v_amd.hyper import DynamicUpsampleLayer, HyperE2VID
    net = HyperE2VID(dict(KW))
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g26["net__keys"]] and len(sd) == 47
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g26["net__shapes"]]
    assert sum(v.numel() for v in sd.values()) == int(g26["net__n_elems"]) == 10150455
    res = net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in g26_state(g26).items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    dec = net.unetrecurrent.decoders[0]
    assert isinstance(dec, DynamicUpsampleLayer) and [type(m).__name__ for m in dec.dynamic_atom_generation.bases_net] == \
        ["Conv2d", "BatchNorm2d", "Tanh", "Conv2d", "BatchNorm2d", "Tanh"]
    for key in ("bases_net.0.weight", "bases_net.1.running_mean", "bases_net.4.num_batches_tracked"):
        assert LAYER + "dynamic_atom_generation." + key in sd
    assert net.num_bins == 5 and net.num_encoders == 3 and net.prev_recs is None and net.states == [None] * 3
    layer = DynamicUpsampleLayer(256, 128, 5, padding=2, in_fuse_channels=6)
    assert list(layer.state_dict().keys()) == [str(k) for k in g26["layer__keys"]]
    # without the dynamic decoder the subclass is the E2VID network
    from v2v_amd.hyper import UNetRecurrent
    from v2v_amd.unet import UpsampleConvLayer
    assert isinstance(UNetRecurrent(dict(KW, use_dynamic_decoder=False)).decoders[0], UpsampleConvLayer)


def test_seeded_weight_recipe_reproduces_the_generators_bits(g26):
    vals = g26_state(g26)
    probe = np.concatenate([np.asarray(vals[k], dtype=np.float32).ravel()[:3] for k in list(vals)[::5]])
    assert np.array_equal(probe, g26["net__weight_probe"])
    bn = LAYER + "dynamic_atom_generation.bases_net.1."
    assert vals[bn + "running_var"].min() >= 0.5 and abs(vals[bn + "weight"] - 1).max() <= 0.17 + 1e-6 and vals[bn + "num_batches_tracked"] == 0


def test_fourier_bessel_bases_equal_the_reference_buffer(g26):
    from v2v_amd.hyper import fourier_bessel_bases
    b = fourier_bessel_bases(5, 6)
    assert tuple(b.shape) == (12, 25) and str(b.dtype) == "torch.float32"
    assert np.abs(b.numpy() - g26["bases"]).max() <= 1e-6
    assert np.abs(b.numpy()[:6].reshape(6, 5, 5)[:, [0, 4]]).max() == 0.0          # the 3 x 3 scale is zero-padded to 5 x 5


def test_stock_restatement_equals_the_reference_on_cpu(g26):
    import torch
    from hyper_stock import stock_layer
    torch.set_num_threads(4)
    with torch.no_grad():
        p = {k: torch.from_numpy(np.asarray(v)) for k, v in g26_state(g26).items()}
        seq = stock_sequence(torch.from_numpy(g26["net__vox"].astype(np.float32)).transpose(0, 1), p)
        assert err(seq.transpose(0, 1).numpy(), g26["net__images"])[0] <= 1e-4
        pl = {k: torch.from_numpy(np.asarray(v)) for k, v in g26_layer_state(g26).items()}
        x, ev, prev = (torch.from_numpy(seeded_input(s, *sh)) for s, sh in zip(g26["layer__x_seeds"], ((2, 256, 8, 8), (2, 5, 64, 64), (2, 1, 64, 64))))
        ctx, atoms, y = stock_layer(x, ev, prev, pl)
        assert err(ctx[:1].numpy(), g26["layer__context"])[0] <= 1e-4 and err(atoms[:1].numpy(), g26["layer__atoms"])[0] <= 1e-4
        assert err(y.numpy(), g26["layer__y"])[0] <= 1e-4
        # the context's x1/4 bilinear resampling is the mean of the central 2 x 2 of every 4 x 4 block (what the staging kernel computes)
        cat = torch.cat([ev, prev], 1)
        mean = cat.reshape(2, 6, 16, 4, 16, 4)[:, :, :, 1:3, :, 1:3].mean((3, 5))
        assert float((mean - torch.nn.functional.interpolate(cat, scale_factor=0.25, mode="bilinear", align_corners=False)).abs().max()) <= 1e-6


def test_batchnorm_fold_equals_conv_then_eval_batchnorm():
    import torch
    from v2v_amd.hyper import fold_batchnorm
    conv, bn = torch.nn.Conv2d(32, 64, 3, padding=1), torch.nn.BatchNorm2d(64).eval()
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        bn.weight.copy_(1 + 0.2 * torch.randn(64, generator=g)), bn.bias.copy_(torch.randn(64, generator=g))
        bn.running_mean.copy_(torch.randn(64, generator=g)), bn.running_var.copy_(0.5 + torch.rand(64, generator=g))
        x = torch.randn((2, 32, 12, 12), generator=g)
        w, b = fold_batchnorm(conv, bn)
        assert float((torch.nn.functional.conv2d(x, w, b, padding=1) - bn(conv(x))).abs().max()) <= 1e-5


def test_unsupported_configurations_raise_on_the_cpu():
    import torch
    from v2v_amd.hyper import DynamicUpsampleLayer, HyperE2VID
    for bad in (dict(skip_type="concat"), dict(recurrent_block_type="convgru"), dict(kernel_size=3), dict(base_num_channels=64),
                dict(channel_multiplier=3), dict(norm="BN"), dict(use_upsample_conv=False), dict(num_output_channels=3), dict(num_encoders=4),
                dict(num_encoders=2)):
        with pytest.raises(ValueError):
            HyperE2VID(dict(KW, **bad))
    net = HyperE2VID(dict(KW)).eval()
    with torch.no_grad():
        for h, w in ((100, 128), (128, 72), (180, 240)):
            with pytest.raises(ValueError, match="multiples of 16"):
                net(torch.zeros((1, 5, h, w)))
        with pytest.raises(ValueError, match="multiples of 16"):
            net.forward_sequence(torch.zeros((1, 2, 5, 100, 128)))
        with pytest.raises(ValueError):
            net.forward_sequence(torch.zeros((1, 5, 64, 64)))
    for args, kw in (((128, 64, 5), dict(padding=2)), ((256, 128, 3), dict(padding=1)), ((256, 128, 5), dict(padding=2, num_atoms=4)),
                     ((256, 128, 5), dict(padding=2, in_fuse_channels=9)), ((256, 128, 5), dict(padding=2, activation="tanh"))):
        with pytest.raises(ValueError):
            DynamicUpsampleLayer(*args, **kw)


def test_forward_refuses_training_mode_and_autograd():
    import torch
    from v2v_amd.hyper import DynamicUpsampleLayer, HyperE2VID
    net = HyperE2VID(dict(KW))
    assert net.training
    with torch.no_grad(), pytest.raises(RuntimeError, match="eval"):
        net(torch.zeros((1, 5, 64, 64)))
    layer = DynamicUpsampleLayer(256, 128, 5, padding=2, in_fuse_channels=6)
    x, ev, prev = torch.zeros((1, 256, 8, 8)), torch.zeros((1, 5, 64, 64)), torch.zeros((1, 1, 64, 64))
    with torch.no_grad(), pytest.raises(RuntimeError, match="eval"):
        layer(x, ev, prev)
    with pytest.raises(RuntimeError, match="inference-only"):
        layer.eval()(x, ev, prev)


def test_new_entry_points_validate_their_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from v2v_amd import _lib as L
    lib = L.lib()
    ok, ok2, mis, out = C.c_void_p(4096), C.c_void_p(8192), C.c_void_p(4098), C.c_void_p(1 << 20)
    ctx = lambda **kw: lib.v2v_hyper_context_hip(kw.get("ev", ok), 5 * 64 * 64, 64 * 64, 64, 1, kw.get("prev", ok2), kw.get("b", 2), kw.get("c", 5),  # noqa: E731
                                                 kw.get("h", 64), kw.get("w", 64), kw.get("dst", out), None)
    assert ctx(ev=None) == L.ERR_NULL and ctx(prev=None) == L.ERR_NULL and ctx(dst=None) == L.ERR_NULL
    assert ctx(c=8) == L.ERR_SHAPE and ctx(c=0) == L.ERR_SHAPE and ctx(h=62) == L.ERR_SHAPE and ctx(w=0) == L.ERR_SHAPE and ctx(b=0) == L.ERR_SHAPE
    assert ctx(b=1 << 20, h=64, w=64) == L.ERR_SHAPE                                                  # B*H*W >= 2^31
    assert ctx(dst=mis) == L.ERR_ALIGN and ctx(ev=mis) == L.ERR_ALIGN
    cc = lambda **kw: lib.v2v_hyper_context_conv_hip(kw.get("x", ok), kw.get("wgt", ok), kw.get("bias", ok), kw.get("b", 2), kw.get("h", 12), 15,  # noqa: E731
                                                     kw.get("cin", 6), kw.get("out", out), None)
    assert cc(x=None) == L.ERR_NULL and cc(wgt=None) == L.ERR_NULL and cc(bias=None) == L.ERR_NULL and cc(out=None) == L.ERR_NULL
    assert cc(cin=9) == L.ERR_SHAPE and cc(cin=0) == L.ERR_SHAPE and cc(h=0) == L.ERR_SHAPE and cc(b=1 << 24, h=1 << 10) == L.ERR_SHAPE
    assert cc(x=mis) == L.ERR_ALIGN and cc(out=mis) == L.ERR_ALIGN and cc(out=ok) == L.ERR_PARAM
    assert lib.v2v_tanh_bf16_hip(None, 64, ok, None) == L.ERR_NULL and lib.v2v_tanh_bf16_hip(ok, 64, None, None) == L.ERR_NULL
    assert lib.v2v_tanh_bf16_hip(ok, 12, ok, None) == L.ERR_SHAPE and lib.v2v_tanh_bf16_hip(ok, 1 << 31, ok, None) == L.ERR_SHAPE
    assert lib.v2v_tanh_bf16_hip(mis, 64, ok, None) == L.ERR_ALIGN
    assert lib.v2v_hyper_atoms_hip(None, ok, 16, out, None) == L.ERR_NULL and lib.v2v_hyper_atoms_hip(ok, None, 16, out, None) == L.ERR_NULL
    assert lib.v2v_hyper_atoms_hip(ok, ok, 16, None, None) == L.ERR_NULL
    assert lib.v2v_hyper_atoms_hip(ok, ok, 0, out, None) == L.ERR_SHAPE and lib.v2v_hyper_atoms_hip(ok, ok, 1 << 24, out, None) == L.ERR_SHAPE
    assert lib.v2v_hyper_atoms_hip(ok, ok, 16, C.c_void_p(4098), None) == L.ERR_ALIGN
    assert lib.v2v_hyper_dynconv_packed_elems(256, 128, 6, 5) == 256 * 128 * 6
    for cin, cout, atoms, ks in ((128, 128, 6, 5), (256, 64, 6, 5), (256, 128, 4, 5), (256, 128, 6, 3)):
        assert lib.v2v_hyper_dynconv_packed_elems(cin, cout, atoms, ks) == -1
    assert lib.v2v_hyper_dynconv_pack_weights_hip(None, 256, 128, 6, ok, None) == L.ERR_NULL
    assert lib.v2v_hyper_dynconv_pack_weights_hip(ok, 256, 128, 6, None, None) == L.ERR_NULL
    assert lib.v2v_hyper_dynconv_pack_weights_hip(ok, 128, 128, 6, ok2, None) == L.ERR_SHAPE
    assert lib.v2v_hyper_dynconv_pack_weights_hip(ok, 256, 128, 6, mis, None) == L.ERR_ALIGN
    dyn = lambda **kw: lib.v2v_hyper_dynconv_nhwc_hip(kw.get("x", ok), kw.get("atoms", ok2), kw.get("packed", ok), kw.get("bias", ok), 1, kw.get("b", 2),  # noqa: E731
                                                      kw.get("h", 16), kw.get("w", 16), kw.get("cin", 256), kw.get("cout", 128), kw.get("na", 6),
                                                      kw.get("ks", 5), kw.get("out", out), None)
    for name in ("x", "atoms", "packed", "bias", "out"):
        assert dyn(**{name: None}) == L.ERR_NULL, name
    assert dyn(cin=128) == L.ERR_SHAPE and dyn(cout=256) == L.ERR_SHAPE and dyn(na=5) == L.ERR_SHAPE and dyn(ks=3) == L.ERR_SHAPE
    assert dyn(b=0) == L.ERR_SHAPE and dyn(h=0) == L.ERR_SHAPE and dyn(b=4096, h=64, w=64) == L.ERR_SHAPE   # 2^32 input elements
    assert dyn(x=mis) == L.ERR_ALIGN and dyn(packed=mis) == L.ERR_ALIGN and dyn(atoms=C.c_void_p(4100)) == L.ERR_ALIGN
    assert dyn(out=ok) == L.ERR_PARAM                                                                 # out aliases x
    assert b"alias" in lib.v2v_last_error()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------
def _package_net(g26):
    import torch
    from v2v_amd.hyper import HyperE2VID
    net = HyperE2VID(dict(KW)).cuda().eval()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in g26_state(g26).items()}, strict=True)
    return net


def _steps(net, vox, **kw):
    import torch
    net.reset_states()
    with torch.no_grad():
        return [net(vox[t], **kw)["image"] for t in range(vox.shape[0])]


@gpu
@pytest.mark.parametrize("layout", ["nchw_f32", "channels_last_bf16"])
def test_dynamic_layer_vs_reference(g26, layout):
    """Measured on an MI355X, both layouts alike: context 3.44e-3 max / 7.8e-4 rms, atoms 3.20e-3 / 4.9e-4, output 2.17e-2 / 3.31e-3 at |y|max 6.52
    (bar 3e-2 / 6e-3 x max(1, |y|max)); DESIGN 4.12."""
    import contextlib
    import torch
    from v2v_amd.hyper import DynamicUpsampleLayer
    layer = DynamicUpsampleLayer(256, 128, 5, padding=2, in_fuse_channels=6).cuda().eval()
    layer.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in g26_layer_state(g26).items()}, strict=True)
    x, ev, prev = (torch.from_numpy(seeded_input(s, *sh)).cuda() for s, sh in zip(g26["layer__x_seeds"], ((2, 256, 8, 8), (2, 5, 64, 64), (2, 1, 64, 64))))
    cl = layout == "channels_last_bf16"
    if cl:
        x, ev = x.to(torch.bfloat16).contiguous(memory_format=torch.channels_last), ev.contiguous(memory_format=torch.channels_last)
    with torch.no_grad(), (torch.autocast("cuda", dtype=torch.bfloat16) if cl else contextlib.nullcontext()):
        ctx = layer.context(ev, prev)
        atoms = layer.atoms(ev, prev)
        y = layer(x, ev, prev)
    assert tuple(y.shape) == (2, 128, 16, 16) and y.dtype == (torch.bfloat16 if cl else torch.float32)
    assert y.is_contiguous(memory_format=torch.channels_last) if cl else y.is_contiguous()
    for name, got, want in (("context", ctx[:1].permute(0, 3, 1, 2), g26["layer__context"]), ("atoms", atoms[:1].permute(0, 4, 3, 1, 2), g26["layer__atoms"]),
                            ("output", y, g26["layer__y"])):
        assert tuple(got.shape) == want.shape, name
        mx, rms = err(got.float().cpu().numpy(), want)
        scale = max(1.0, float(np.abs(want).max()))
        print(f"dynamic layer {name} [{layout}] vs G26: max {mx:.3e} rms {rms:.3e} (|want|max {float(np.abs(want).max()):.2f}, bar x {scale:.2f})")
        assert mx <= 3e-2 * scale and rms <= 6e-3 * scale, (name, layout, mx, rms, scale)


@gpu
def test_network_vs_reference_over_three_steps(g26):
    """Measured on an MI355X, error / the reference's own bf16-autocast error of the step (bar 2.5 x): max 1.05, 0.98, 1.24; rms 1.06, 0.99, 1.09
    (2.998e-2 / 7.18e-3, 2.879e-2 / 6.98e-3, 3.698e-2 / 7.54e-3); DESIGN 4.12."""
    import torch
    net = _package_net(g26)
    vox = torch.from_numpy(g26["net__vox"].astype(np.float32)).cuda()
    imgs = _steps(net, vox)
    assert net.prev_recs is imgs[-1] or torch.equal(net.prev_recs, imgs[-1])
    bad = []
    for t, img in enumerate(imgs):
        assert img.dtype == torch.float32 and tuple(img.shape) == (2, 1, 64, 64)
        mx, rms = err(img.cpu().numpy(), g26["net__images"][t])
        amx, arms = (float(v) for v in g26["net__bf16_autocast_err"][t])
        print(f"HyperE2VID step {t} vs G26: max {mx:.3e} ({mx / amx:.2f} x autocast) rms {rms:.3e} ({rms / arms:.2f} x autocast)")
        if not (mx <= 2.5 * amx and rms <= 2.5 * arms):
            bad.append((t, mx, rms, amx, arms))
    assert not bad, bad


@gpu
def test_previous_reconstruction_feeds_the_dynamic_decoder(g26):
    import torch
    net = _package_net(g26)
    vox = torch.from_numpy(g26["net__vox"].astype(np.float32)).cuda()
    kept = _steps(net, vox[:2])[1]
    net.reset_states()
    with torch.no_grad():
        net(vox[0])
        net.prev_recs = torch.zeros_like(net.prev_recs)
        cut = net(vox[1])["image"]
    moved = float((kept - cut).abs().max())
    print(f"step-1 image with / without prev_recs: max difference {moved:.3f} (reference: {float(g26['feedback_effect']):.3f})")
    assert moved >= 0.5 * float(g26["feedback_effect"])


@gpu
def test_gt_image_mixing_equals_feeding_the_mixed_image_by_hand(g26):
    import torch
    net = _package_net(g26)
    vox = torch.from_numpy(g26["net__vox"].astype(np.float32)).cuda()
    gt = torch.from_numpy(seeded_input(77, 2, 1, 64, 64)).cuda()
    with torch.no_grad():
        net.reset_states()
        first = net(vox[0])["image"]
        a = net(vox[1], gt_image=gt, beta=0.5)["image"]
        net.reset_states()
        net(vox[0])
        net.prev_recs = first * (1 - 0.5) + gt * 0.5
        b = net(vox[1])["image"]
        net.reset_states()
        net(vox[0])
        c = net(vox[1], gt_image=gt, beta=0)["image"]                       # beta 0: gt_image is ignored
        net.reset_states()
        net(vox[0])
        d = net(vox[1])["image"]
    assert torch.equal(a, b) and torch.equal(c, d) and not torch.equal(a, d)


@gpu
def test_forward_sequence_equals_the_per_step_loop_bit_for_bit(g26):
    import torch
    ev = torch.from_numpy(sparse_voxels(61, 2, 4, 5, 64, 96)).cuda()
    net = _package_net(g26)                                                  # first call after load_state_dict: packs inside the sequence
    with torch.no_grad():
        seq = net.forward_sequence(ev)
        states_seq = net.states
    assert tuple(seq.shape) == (2, 4, 1, 64, 96) and seq.dtype == torch.float32
    loop = _steps(net, ev.transpose(0, 1))
    for t in range(4):
        assert torch.equal(seq[:, t], loop[t]), t
    for (h1, c1), (h2, c2) in zip(states_seq, net.states):
        assert torch.equal(h1, h2) and torch.equal(c1, c2)
    net.reset_states()
    with torch.no_grad():
        assert torch.equal(net.forward_sequence(ev), seq)
        # an in-place weight update is seen (the BatchNorm fold is repacked)
        net.unetrecurrent.decoders[0].dynamic_atom_generation.bases_net[1].running_mean.add_(0.25)
        net.reset_states()
        assert not torch.equal(net.forward_sequence(ev), seq)
    assert float(seq.abs().max()) > 0.1


@gpu
@pytest.mark.parametrize("n,h,w", [(1, 192, 240), (1, 272, 352), (12, 128, 128)])
def test_network_at_other_sizes_vs_stock_float32(g26, n, h, w):
    """180 x 240 padded to 192 x 240, 260 x 346 padded to 272 x 352 (deepest level 34 x 44), and the training shape; two steps, so the
    second runs on carried states and a fed-back image.  Measured on an MI355X (x G26's autocast error of the step, max / rms): 192 x 240
    1.11 / 1.10 and 1.16 / 1.07; 272 x 352 1.20 / 1.11 and 1.31 / 1.08; 12 x 128^2 1.24 / 1.09 and 1.23 / 1.05; DESIGN 4.12."""
    import torch
    net = _package_net(g26)
    p = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in g26_state(g26).items()}
    ev = torch.from_numpy(sparse_voxels(62, n, 2, 5, h, w)).cuda()
    with torch.no_grad():
        want = stock_sequence(ev, p)
        got = net.forward_sequence(ev)
    bad = []
    for t in range(2):
        mx, rms = err(got[:, t].cpu().numpy(), want[:, t].cpu().numpy())
        amx, arms = (float(v) for v in g26["net__bf16_autocast_err"][t])
        print(f"HyperE2VID {n} x {h} x {w} step {t} vs stock float32: max {mx:.3e} ({mx / amx:.2f} x) rms {rms:.3e} ({rms / arms:.2f} x G26's autocast error)")
        if not (mx <= 2.5 * amx and rms <= 2.5 * arms):
            bad.append((t, mx, rms, amx, arms))
    assert not bad, bad
