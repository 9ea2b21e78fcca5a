"""EVFlowNet on the device kernels (v2v_amd.unet.EVFlowNet / UNet): the stem, the concat-skip upsampling and the network's forward.

Yardsticks.  Golden G25 (tests/golden/make_golden_evflow.py) = the reference's own UNet with EVFlowNet's kwargs in float32 on seeded
weights, its stem and its last concat decoder; tests/evflow_stock.py restates the network in stock PyTorch and is pinned to G25 here on
the CPU.  Bars: single layers 3e-2 max / 6e-3 rms (tests/test_unet_golden.py's single-layer bar: one bf16 rounding of inputs and weights,
K <= 2304, one rounding of the output; both layers here have K <= 1152); the network at most 2.5 x the reference's own CPU bf16-autocast
error stored in G25 (2.5e-2 max / 5.1e-3 rms); other sizes at most 2 x the stock network's own bf16-autocast error on the same input
+ 1e-3.  Each GPU test prints its figures before it asserts.
Measured on an MI355X: network / G25 autocast error = 0.94 (max) and 0.97 (rms); see DESIGN 4.11."""
import ctypes as C

import numpy as np
import pytest

from evflow_stock import KW, err, g25 as load_g25, g25_state, sparse_voxels, stock_flow
from seeded_weights import load_seeded, seeded_input, seeded_state

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def g25():
    return load_g25()


# ---- no GPU needed ----------------------------------------------------------------------------------------------------------------
def test_package_evflownet_has_the_reference_state_dict(g25):
    import torch
    from v2v_amd.unet import EVFlowNet
    net = EVFlowNet(dict(num_bins=5, skip_type="sum", kernel_size=5, num_encoders=3))        # the hard-coded kwargs win (model/model.py:245)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g25["evflow__keys"]] and len(sd) == 26
    assert [",".join(map(str, v.shape)) for v in sd.values()] == [str(s) for s in g25["evflow__shapes"]]
    assert sum(v.numel() for v in sd.values()) == int(g25["evflow__n_params"]) == 14125346
    vals = g25_state(g25)
    res = net.load_state_dict({k: torch.from_numpy(v) for k, v in vals.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert net.num_bins == 5 and net.num_encoders == 4 and net.reset_states() is None
    assert [type(m).__name__ for m in (net.unet.encoders, net.unet.resblocks, net.unet.decoders)] == ["ModuleList"] * 3 and net.unet.pred is not None


def test_seeded_weight_recipe_reproduces_the_generators_bits(g25):
    vals = g25_state(g25)
    probe = np.concatenate([vals[k].ravel()[:3] for k in list(vals)[::5]])
    assert np.array_equal(probe, g25["evflow__weight_probe"])


def test_stock_restatement_equals_the_reference_on_cpu(g25):
    import torch
    import torch.nn.functional as F
    torch.set_num_threads(4)
    p = {k: torch.from_numpy(v) for k, v in g25_state(g25).items()}
    with torch.no_grad():
        flow = stock_flow(torch.from_numpy(g25["evflow__vox"].astype(np.float32)), p)
        assert err(flow.numpy(), g25["evflow__flow"])[0] <= 1e-4
        s = seeded_state({"weight": (64, 5, 3, 3), "bias": (64,)}, int(g25["stem__seed"]))
        x = torch.from_numpy(seeded_input(g25["stem__x_seed"], *g25["stem__x_shape"]))
        y = F.relu(F.conv2d(x, torch.from_numpy(s["weight"]), torch.from_numpy(s["bias"]), stride=2, padding=1))
        assert err(y.numpy(), g25["stem__y"])[0] <= 1e-4
        s = seeded_state({"weight": (32, 128, 3, 3), "bias": (32,)}, int(g25["catdec__seed"]))
        a, b = (torch.from_numpy(seeded_input(sd, *g25["catdec__x_shape"])) for sd in g25["catdec__x_seeds"])
        u = F.interpolate(torch.cat([a, b], 1), scale_factor=2, mode="bilinear", align_corners=False)
        y = F.relu(F.conv2d(u, torch.from_numpy(s["weight"]), torch.from_numpy(s["bias"]), padding=1))
        assert err(y.numpy(), g25["catdec__y"])[0] <= 1e-4


def test_unsupported_configurations_raise_on_the_cpu():
    import torch
    from v2v_amd.convlstm import ConvLayer
    from v2v_amd.unet import EVFlowNet, UNet, UpsampleConvLayer
    for bad in (dict(skip_type="sum"), dict(kernel_size=5), dict(norm="BN"), dict(use_upsample_conv=False), dict(num_encoders=3),
                dict(base_num_channels=64), dict(num_output_channels=4), dict(num_bins=9)):
        with pytest.raises(ValueError):
            UNet(dict(KW, **bad))
    net = EVFlowNet(dict(num_bins=5))
    with pytest.raises(ValueError, match="level 4 is 17 x 22"):                 # MVSEC 260 x 346 padded to 272 x 352: before anything is launched
        net(torch.zeros((1, 5, 272, 352)))
    with pytest.raises(ValueError, match="multiples of 16"):
        net(torch.zeros((1, 5, 100, 128)))
    with pytest.raises(ValueError):
        net.forward_sequence(torch.zeros((1, 1, 5, 272, 352)))
    net.unet.check_size(128, 128)
    net.unet.check_size(192, 240)
    assert net.default_chunk(128, 128) == 1023
    # the few-channel forms of ConvLayer: the head (32 outputs, stride 1) and the stem (64 outputs, 3x3, stride 2); nothing else
    assert ConvLayer(5, 64, 3, stride=2, padding=1).stem and not ConvLayer(5, 64, 3, stride=2, padding=1).head
    assert ConvLayer(5, 32, 3, stride=1, padding=1).head
    for args in ((5, 64, 3, 1, 1), (5, 64, 5, 2, 2), (5, 32, 3, 2, 1), (5, 128, 3, 2, 1)):
        with pytest.raises(ValueError):
            ConvLayer(*args)
    ConvLayer(32, 2, 1, activation=None, trainable=True)                         # the prediction layer: <= 3 outputs, trainable
    with pytest.raises(ValueError):
        ConvLayer(32, 4, 1, activation=None)
    with torch.no_grad():
        with pytest.raises(ValueError):                                          # concat is the decoder's skip
            ConvLayer(64, 64, 3, padding=1)(torch.zeros((1, 64, 8, 8)), torch.zeros((1, 64, 8, 8)), skip_type="concat")
        with pytest.raises(ValueError):
            UpsampleConvLayer(128, 32, 3, padding=1)(torch.zeros((1, 64, 8, 8)), torch.zeros((1, 64, 8, 8)), skip_type="product")
        with pytest.raises(ValueError, match="in_channels"):
            UpsampleConvLayer(128, 32, 3, padding=1)(torch.zeros((1, 64, 8, 8)), torch.zeros((1, 32, 8, 8)), skip_type="concat")


def test_new_entry_points_validate_their_arguments_without_a_gpu():
    import __graft_entry__ as ge
    ge.build()
    from v2v_amd import _lib as L
    lib = L.lib()
    ok, mis = C.c_void_p(4096), C.c_void_p(4098)
    # stem
    assert lib.v2v_conv_stem_packed_elems() == 2 * 64 * 64
    assert lib.v2v_conv_stem_pack_weights_hip(None, 5, ok, None) == L.ERR_NULL
    assert lib.v2v_conv_stem_pack_weights_hip(ok, 9, ok, None) == L.ERR_SHAPE
    assert lib.v2v_conv_stem_pack_weights_hip(ok, 5, mis, None) == L.ERR_ALIGN
    assert lib.v2v_conv_stem_nhwc_hip(None, ok, ok, 1, 1, 32, 32, ok, None) == L.ERR_NULL
    assert lib.v2v_conv_stem_nhwc_hip(ok, ok, ok, 1, 1, 32, 32, None, None) == L.ERR_NULL
    for h, w in ((17, 32), (32, 24), (8, 32), (0, 32)):
        assert lib.v2v_conv_stem_nhwc_hip(ok, ok, ok, 1, 1, h, w, C.c_void_p(8192), None) == L.ERR_SHAPE
    assert lib.v2v_conv_stem_nhwc_hip(mis, ok, ok, 1, 1, 32, 32, C.c_void_p(8192), None) == L.ERR_ALIGN
    assert lib.v2v_conv_stem_nhwc_hip(ok, ok, ok, 1, 1, 32, 32, ok, None) == L.ERR_PARAM            # out aliases x8
    # concat-skip upsampling
    out = C.c_void_p(1 << 20)
    assert lib.v2v_upsample2x_cat_nhwc_hip(None, 64, ok, 64, 1, 8, 8, out, None) == L.ERR_NULL
    assert lib.v2v_upsample2x_cat_nhwc_hip(ok, 64, None, 64, 1, 8, 8, out, None) == L.ERR_NULL      # C2 > 0 needs the skip
    assert lib.v2v_upsample2x_cat_nhwc_hip(ok, 64, ok, 64, 1, 8, 8, None, None) == L.ERR_NULL
    for c1, c2 in ((12, 64), (64, 4), (0, 64), (64, -8)):
        assert lib.v2v_upsample2x_cat_nhwc_hip(ok, c1, ok, c2, 1, 8, 8, out, None) == L.ERR_SHAPE
    assert lib.v2v_upsample2x_cat_nhwc_hip(ok, 64, ok, 64, 0, 8, 8, out, None) == L.ERR_SHAPE
    assert lib.v2v_upsample2x_cat_nhwc_hip(ok, 1024, ok, 1024, 4096, 64, 64, out, None) == L.ERR_SHAPE   # output >= 2^31 elements
    assert lib.v2v_upsample2x_cat_nhwc_hip(mis, 64, ok, 64, 1, 8, 8, out, None) == L.ERR_ALIGN
    assert lib.v2v_upsample2x_cat_nhwc_hip(ok, 64, mis, 64, 1, 8, 8, out, None) == L.ERR_ALIGN
    assert lib.v2v_upsample2x_cat_nhwc_hip(ok, 64, C.c_void_p(8192), 64, 1, 8, 8, ok, None) == L.ERR_PARAM   # out aliases x
    assert lib.v2v_upsample2x_cat_nhwc_hip(ok, 64, C.c_void_p(8192), 0, 1, 8, 8, out, None) == L.ERR_PARAM   # a skip with C2 = 0
    # its adjoint
    assert lib.v2v_upsample2x_cat_bwd_nhwc_hip(None, 1, 8, 8, 128, 0, 64, out, None) == L.ERR_NULL
    assert lib.v2v_upsample2x_cat_bwd_nhwc_hip(ok, 1, 8, 8, 128, 0, 64, None, None) == L.ERR_NULL
    for ctot, c0, c in ((128, 0, 12), (128, 4, 64), (128, 72, 64), (132, 0, 64), (128, -8, 64), (128, 0, 0)):
        assert lib.v2v_upsample2x_cat_bwd_nhwc_hip(ok, 1, 8, 8, ctot, c0, c, out, None) == L.ERR_SHAPE
    assert lib.v2v_upsample2x_cat_bwd_nhwc_hip(mis, 1, 8, 8, 128, 0, 64, out, None) == L.ERR_ALIGN
    assert lib.v2v_upsample2x_cat_bwd_nhwc_hip(ok, 1, 8, 8, 128, 64, 64, mis, None) == L.ERR_ALIGN
    # prediction backward, 1..3 outputs
    assert lib.v2v_conv1x1_bwd_cout_workspace_bytes(4096, 32, 2) == 2 * 2 * 33 * 4
    for m, c, cout in ((4096, 32, 0), (4096, 32, 4), (4096, 24, 2), (4096, 256, 2), (0, 32, 2)):
        assert lib.v2v_conv1x1_bwd_cout_workspace_bytes(m, c, cout) == -1
        assert lib.v2v_conv1x1_bwd_cout_nhwc_hip(ok, ok, None, ok, m, c, cout, out, ok, ok, ok, None) == L.ERR_SHAPE
    for k in range(7):
        a = [ok, ok, None, ok, 4096, 32, 2, out, ok, ok, ok, None]
        a[[0, 1, 3, 7, 8, 9, 10][k]] = None
        assert lib.v2v_conv1x1_bwd_cout_nhwc_hip(*a) == L.ERR_NULL
    assert lib.v2v_conv1x1_bwd_cout_nhwc_hip(ok, mis, None, ok, 4096, 32, 2, out, ok, ok, ok, None) == L.ERR_ALIGN
    assert lib.v2v_conv1x1_bwd_cout_nhwc_hip(ok, ok, mis, ok, 4096, 32, 2, out, ok, ok, ok, None) == L.ERR_ALIGN
    assert lib.v2v_conv1x1_bwd_cout_nhwc_hip(mis, ok, None, ok, 4096, 32, 2, out, ok, ok, ok, None) == L.ERR_ALIGN
    # the convolution with the tile of another batch: v2v_conv_nhwc_hip's checks
    conv = lambda **kw: lib.v2v_conv_nhwc_like_hip(kw.get("x", ok), ok, ok, None, 1, 4, kw.get("h", 16), kw.get("w", 16), kw.get("cin", 64), 128, kw.get("ks", 3),  # noqa: E731
                                                   kw.get("stride", 1), kw.get("out", out), kw.get("like", 2), None)
    assert conv(x=None) == L.ERR_NULL and conv(out=None) == L.ERR_NULL
    assert conv(ks=4) == L.ERR_PARAM and conv(stride=3) == L.ERR_PARAM and conv(like=-1) == L.ERR_PARAM
    assert conv(cin=48) == L.ERR_SHAPE and conv(h=3, w=3) == L.ERR_SHAPE                              # 9 output pixels: not whole groups of 4
    assert conv(x=mis) == L.ERR_ALIGN and conv(out=ok) == L.ERR_PARAM


# ---- GPU: identities (exact) --------------------------------------------------------------------------------------------------------
def _bf16(seed, *shape):
    import torch
    return torch.from_numpy(seeded_input(seed, *shape)).cuda().to(torch.bfloat16)


@gpu
@pytest.mark.parametrize("b,h,w,c", [(2, 16, 16, 64), (3, 5, 7, 8), (12, 64, 64, 64), (1, 12, 15, 512)])
def test_concat_upsampling_is_the_existing_upsampling_per_channel_slice(b, h, w, c):
    import torch
    from v2v_amd.nhwc_ops import upsample2x_cat_nhwc, upsample2x_nhwc
    x, s = _bf16(1, b, h, w, c), _bf16(2, b, h, w, 2 * c)
    assert torch.equal(upsample2x_cat_nhwc(x, None), upsample2x_nhwc(x, None))                       # C2 = 0: the existing entry, bit for bit
    both = upsample2x_cat_nhwc(x, s)
    assert tuple(both.shape) == (b, 2 * h, 2 * w, 3 * c)
    assert torch.equal(both, torch.cat([upsample2x_nhwc(x, None), upsample2x_nhwc(s, None)], dim=3))
    ref = torch.nn.functional.interpolate(torch.cat([x, s], 3).permute(0, 3, 1, 2).float(), scale_factor=2, mode="bilinear", align_corners=False)
    mx, _ = err(both.permute(0, 3, 1, 2).float().cpu().numpy(), ref.cpu().numpy())
    print(f"concat upsampling vs float32 interpolate(cat): max {mx:.3e}")
    assert mx <= 2.0 ** -8 * float(ref.abs().max())                                                   # one bf16 rounding of the result


@gpu
@pytest.mark.parametrize("b,h,w,ctot,c0,c", [(2, 16, 16, 128, 0, 128), (2, 16, 16, 128, 0, 64), (2, 16, 16, 128, 64, 64), (3, 5, 7, 24, 8, 16)])
def test_concat_upsampling_adjoint_is_the_existing_adjoint_on_a_slice(b, h, w, ctot, c0, c):
    import torch
    from v2v_amd.nhwc_ops import upsample2x_bwd_nhwc, upsample2x_cat_bwd_nhwc
    d = _bf16(3, b, 2 * h, 2 * w, ctot)
    got = upsample2x_cat_bwd_nhwc(d, c0, c)
    assert tuple(got.shape) == (b, h, w, c)
    assert torch.equal(got, upsample2x_bwd_nhwc(d[..., c0:c0 + c].contiguous()))                     # whole width: the existing entry itself


@gpu
@pytest.mark.parametrize("with_skip", [False, True])
def test_prediction_backward_with_one_output_is_the_existing_kernel(with_skip):
    import torch
    from v2v_amd.nhwc_ops import conv1x1_bwd_cout_nhwc, conv1x1_bwd_nhwc
    x, s = _bf16(4, 2, 64, 64, 32), (_bf16(5, 2, 64, 64, 32) if with_skip else None)
    dy = torch.from_numpy(seeded_input(6, 2, 64, 64, 1)).cuda() / 8192
    w = torch.from_numpy(seeded_input(7, 1, 32, 1, 1)).cuda()
    for a, b in zip(conv1x1_bwd_cout_nhwc(dy, x, s, w), conv1x1_bwd_nhwc(dy, x, s, w)):
        assert torch.equal(a, b)


@gpu
@pytest.mark.parametrize("cout", [2, 3])
def test_prediction_backward_for_several_outputs(cout):
    import torch
    from v2v_amd.nhwc_ops import conv1x1_bwd_cout_nhwc
    x = _bf16(8, 3, 32, 48, 32)
    dy = torch.from_numpy(seeded_input(9, 3, 32, 48, cout)).cuda()
    w = torch.from_numpy(seeded_input(10, cout, 32, 1, 1)).cuda()
    dx, dw, db = conv1x1_bwd_cout_nhwc(dy, x, None, w)
    wb = w.reshape(cout, 32).to(torch.bfloat16).double()
    dyd, xd = dy.reshape(-1, cout).double(), x.reshape(-1, 32).double()
    for name, got, want in (("dx", dx.reshape(-1, 32), dyd @ wb), ("dw", dw.reshape(cout, 32), dyd.t() @ xd), ("db", db, dyd.sum(0))):
        rel = float((got.double() - want).norm() / want.norm())
        print(f"conv1x1 backward, {cout} outputs, {name}: rel {rel:.3e}")
        assert rel <= (2.0 ** -8 if name == "dx" else 1e-5), name                                     # dx: one bf16 rounding; dw, db: fp32 sums
    again = conv1x1_bwd_cout_nhwc(dy, x, None, w)
    assert all(torch.equal(a, b) for a, b in zip((dx, dw, db), again))


def _package_net(g25, trainable=False):
    import torch
    from v2v_amd.unet import EVFlowNet
    net = EVFlowNet(dict(num_bins=5), trainable=trainable).cuda()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in g25_state(g25).items()}, strict=True)
    return net


@gpu
@pytest.mark.parametrize("n,t,size,chunk", [(2, 3, 64, None), (2, 3, 64, 4), (10, 8, 128, None)])
def test_forward_sequence_equals_the_per_step_loop_bit_for_bit(g25, n, t, size, chunk):
    import torch
    net = _package_net(g25).eval()
    ev = torch.from_numpy(sparse_voxels(31, n, t, 5, size, size)).cuda()
    with torch.no_grad():
        seq = net.forward_sequence(ev, chunk=chunk)
        assert tuple(seq.shape) == (n, t, 2, size, size) and seq.dtype == torch.float32
        for k in range(t):
            assert torch.equal(seq[:, k], net(ev[:, k])["flow"]), k
        assert float(seq.abs().max()) > 0.1


# ---- GPU: against G25 ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("layout", ["nchw_f32", "channels_last_bf16"])
def test_stem_and_concat_decoder_vs_reference(g25, layout):
    import torch
    from v2v_amd.convlstm import ConvLayer
    from v2v_amd.unet import UpsampleConvLayer

    def prep(v):
        v = torch.from_numpy(v).cuda()
        return v.to(torch.bfloat16).contiguous(memory_format=torch.channels_last) if layout == "channels_last_bf16" else v
    stem = ConvLayer(5, 64, 3, stride=2, padding=1).cuda().eval()
    load_seeded(stem, int(g25["stem__seed"]))
    dec = UpsampleConvLayer(128, 32, 3, padding=1).cuda().eval()
    load_seeded(dec, int(g25["catdec__seed"]))
    with torch.no_grad():
        ys = stem(prep(seeded_input(g25["stem__x_seed"], *g25["stem__x_shape"])))
        a, b = (prep(seeded_input(sd, *g25["catdec__x_shape"])) for sd in g25["catdec__x_seeds"])
        yd = dec(a, b, skip_type="concat")
    for name, y in (("stem", ys), ("catdec", yd)):
        assert tuple(y.shape) == g25[name + "__y"].shape
        mx, rms = err(y.float().cpu().numpy(), g25[name + "__y"])
        print(f"{name} [{layout}] vs G25: max {mx:.3e} rms {rms:.3e}")
        assert mx <= 3e-2 and rms <= 6e-3, (name, layout, mx, rms)


@gpu
def test_stem_applies_event_scales_while_it_reads():
    import torch
    from v2v_amd.convlstm import ConvLayer
    stem = ConvLayer(5, 64, 3, stride=2, padding=1).cuda().eval()
    load_seeded(stem, 41)
    vox = torch.from_numpy(sparse_voxels(42, 2, 5, 32, 32)).cuda()
    scales = torch.tensor([[2.0, 3.0], [1.0, 4.0]], device="cuda")
    normed = torch.where(vox > 0, vox / scales[:, 1].reshape(2, 1, 1, 1), vox / scales[:, 0].reshape(2, 1, 1, 1))
    with torch.no_grad():
        assert torch.equal(stem(vox, scales=scales), stem(normed))


@gpu
def test_network_vs_reference(g25):
    """Measured on an MI355X: 2.31e-2 max / 4.91e-3 rms = 0.94 x / 0.97 x the reference's own bf16-autocast error (bar: 2.5 x)."""
    import torch
    net = _package_net(g25).eval()
    vox = torch.from_numpy(g25["evflow__vox"].astype(np.float32)).cuda()
    with torch.no_grad():
        out = net(vox)
    flow = out["flow"]
    assert flow.dtype == torch.float32 and tuple(flow.shape) == (2, 2, 64, 64) and flow.is_contiguous()
    assert tuple(out["image"].shape) == (2, 1, 64, 64) and float(out["image"].abs().max()) == 0.0
    mx, rms = err(flow.cpu().numpy(), g25["evflow__flow"])
    amx, arms = (float(v) for v in g25["flow__bf16_autocast_err"])
    print(f"EVFlowNet vs G25: max {mx:.3e} ({mx / amx:.2f} x autocast) rms {rms:.3e} ({rms / arms:.2f} x autocast)")
    assert mx <= 2.5 * amx and rms <= 2.5 * arms, (mx, rms, amx, arms)


@gpu
@pytest.mark.parametrize("n,h,w", [(12, 128, 128), (1, 192, 240), (3, 64, 96)])
def test_network_at_other_sizes_vs_stock_float32(g25, n, h, w):
    import torch
    net = _package_net(g25).eval()
    p = {k: torch.from_numpy(v).cuda() for k, v in g25_state(g25).items()}
    vox = torch.from_numpy(sparse_voxels(51, n, 5, h, w)).cuda()
    with torch.no_grad():
        want = stock_flow(vox, p)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            auto = stock_flow(vox, p).float()
        got = net(vox)["flow"]
    mx, rms = err(got.cpu().numpy(), want.cpu().numpy())
    amx, arms = err(auto.cpu().numpy(), want.cpu().numpy())
    print(f"EVFlowNet {n} x {h} x {w} vs stock float32: max {mx:.3e} rms {rms:.3e}; stock bf16 autocast: max {amx:.3e} rms {arms:.3e}")
    assert mx <= 2 * amx + 1e-3 and rms <= 2 * arms + 1e-3, (mx, rms, amx, arms)
