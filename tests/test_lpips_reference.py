"""LPIPS-VGG without a GPU: golden G30 is what its generator says and the stock restatement (tests/lpips_stock.py) reproduces it; autograd's
max-pool tie rule is the one the pool-backward kernel implements; LPIPSVGG carries the reference's 33 keys; everything that must raise
raises; the new C-ABI entry points validate their arguments."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_stock
import lpips_weights as LW


@pytest.fixture(scope="module")
def g30(golden):
    return golden("g30_lpips_vgg.npz")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from v2v_amd import _lib
    return _lib


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def test_g30_is_what_its_generator_says(g30):
    want = set(LW.LIN_KEYS) | {"shift", "scale"}
    for name, shape in LW.CASES.items():
        want |= {f"{name}__{k}" for k in ("pred", "target", "dist64", "dpred64", "dist32", "dpred32", "dist16", "dpred16")}
        pred, target = LW.case_inputs(name)
        assert np.array_equal(g30[f"{name}__pred"], pred) and np.array_equal(g30[f"{name}__target"], target)
        assert pred.min() >= 0 and pred.max() <= 1
        for tag, dt in (("64", np.float64), ("32", np.float32), ("16", np.float32)):
            assert g30[f"{name}__dist{tag}"].shape == shape[:1] and g30[f"{name}__dist{tag}"].dtype == dt
            assert g30[f"{name}__dpred{tag}"].shape == shape and g30[f"{name}__dpred{tag}"].dtype == dt
    assert set(g30) == want
    assert all(np.isfinite(v).all() for v in g30.values())
    assert sum(g30[k].size for k in LW.LIN_KEYS) == 1472 and all(float(g30[k].min()) > 0 for k in LW.LIN_KEYS)
    assert [g30[k].shape for k in LW.LIN_KEYS] == [(1, c, 1, 1) for c in LW.CHANNELS]
    assert g30["shift"].shape == g30["scale"].shape == (1, 3, 1, 1)
    assert float(np.abs(g30["close__pred"] - g30["close__target"]).max()) < 0.3
    assert float(g30["close__dist64"].max()) < 0.1 * float(g30["a__dist64"].min())


@pytest.mark.parametrize("name", sorted(LW.CASES))
def test_stock_restatement_reproduces_g30(g30, name):
    state = LW.golden_state(g30)
    pred, target = (torch.from_numpy(g30[f"{name}__{k}"]) for k in ("pred", "target"))
    d64, g64 = lpips_stock.dist_and_grad(state, pred, target, dtype=torch.float64)
    assert rel(d64, g30[f"{name}__dist64"]) < 1e-12 and rel(g64, g30[f"{name}__dpred64"]) < 1e-12
    # float32: the same operators in the same order; a few thousand roundings of summation noise at the most
    d32, g32 = lpips_stock.dist_and_grad(state, pred, target, dtype=torch.float32)
    assert rel(d32, g30[f"{name}__dist32"]) < 1e-6 and rel(g32, g30[f"{name}__dpred32"]) < 1e-4
    # and the float32 run is a float32 run of the float64 one
    assert rel(g30[f"{name}__dist32"], g30[f"{name}__dist64"]) < 1e-5 and rel(g30[f"{name}__dpred32"], g30[f"{name}__dpred64"]) < 1e-3


def test_autograd_routes_a_max_pool_tie_to_the_first_maximum_in_row_major_order():
    x = torch.tensor([[3., 3., 1., 2., 0., 0.],
                      [3., 3., 2., 2., 0., 0.],
                      [1., 2., 5., 1., 4., 7.],
                      [2., 2., 1., 5., 7., 4.]], dtype=torch.float64)[None, None].requires_grad_(True)
    y = F.max_pool2d(x, 2, 2)
    assert y[0, 0].tolist() == [[3., 2., 0.], [2., 5., 7.]]
    (y * torch.arange(1, 7, dtype=torch.float64).reshape(1, 1, 2, 3)).sum().backward()
    assert x.grad[0, 0].tolist() == [[1., 0., 0., 2., 3., 0.],
                                     [0., 0., 0., 0., 0., 0.],
                                     [0., 4., 5., 0., 0., 6.],
                                     [0., 0., 0., 0., 0., 0.]]


def test_lpipsvgg_has_the_33_reference_keys_and_is_frozen(g30):
    from v2v_amd.lpips import LPIPSVGG
    m = LPIPSVGG()
    assert list(m.state_dict()) == LW.reference_keys() and len(m.state_dict()) == 33
    shapes = LW.backbone_shapes()
    assert all(tuple(m.state_dict()[k].shape) == tuple(s) for k, s in shapes.items())
    res = m.load_state_dict(LW.golden_state(g30), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(m.lin3.model[1].weight, torch.from_numpy(g30["lin3.model.1.weight"]))
    assert not m.training and not any(p.requires_grad for p in m.parameters())
    m.train()
    assert not m.training and not any(sub.training for sub in m.modules())
    assert sum(p.numel() for p in m.parameters()) == 14_714_688 + 1472


def test_everything_that_must_raise_raises_without_a_gpu():
    from v2v_amd import losses, loss_ops
    from v2v_amd.lpips import LPIPSVGG, check_size
    for net in ("alex", "squeeze"):
        with pytest.raises(ValueError, match="vgg"):
            LPIPSVGG(net=net)
        with pytest.raises(ValueError, match="vgg"):
            losses.perceptual_loss(net=net, state_dict={})
    with pytest.raises(ValueError, match="spatial"):
        LPIPSVGG(spatial=True)
    with pytest.raises(ValueError, match="pnet_tune"):
        LPIPSVGG(pnet_tune=True)
    for h, w in ((32, 32), (16, 64), (48, 64), (128, 128), (64, 16)):
        check_size(h, w)
    m = LPIPSVGG()
    img = torch.zeros(2, 1, 32, 32)
    for h, w in ((16, 16), (24, 64), (32, 40), (48, 48), (16, 32), (8, 128)):
        with pytest.raises(ValueError, match="multiples of 16"):
            m(torch.zeros(1, 1, h, w), torch.zeros(1, 1, h, w))
    with pytest.raises(ValueError, match="target"):
        m(img, img.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        m(img, img[:1])
    with pytest.raises(ValueError):
        m(torch.zeros(2, 2, 32, 32), img)
    with pytest.raises(ValueError):
        m(img.double(), img.double())
    with pytest.raises(ValueError, match="chunk"):
        m(img, img, chunk=0)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="GPU"):
            m(img, img)                                        # valid arguments: no CPU fallback
        with pytest.raises(RuntimeError, match="GPU"):
            loss_ops.lpips_pool(torch.zeros(1, 2, 2, 8, dtype=torch.bfloat16))
    try:
        import torchvision  # noqa: F401
        import PerceptualSimilarity  # noqa: F401
    except ImportError:
        with pytest.raises(RuntimeError, match="state_dict="):
            losses.perceptual_loss()
    with pytest.raises(RuntimeError, match="[Mm]issing|[Uu]nexpected"):
        losses.perceptual_loss(state_dict={"lin0.model.1.weight": torch.zeros(1, 64, 1, 1)}, use_gpu=False)


def test_perceptual_loss_loads_a_state_dict_without_a_gpu(g30):
    from v2v_amd import losses
    state = LW.golden_state(g30)
    loss = losses.perceptual_loss(weight=0.5, state_dict=state, use_gpu=False)
    assert loss.weight == 0.5 and not loss.model.training
    assert all(torch.equal(v, state[k]) for k, v in loss.model.state_dict().items())
    del state["scaling_layer.shift"], state["scaling_layer.scale"]              # vgg.pth + the backbone alone: the constants stay
    loss = losses.perceptual_loss(state_dict=state, use_gpu=False)
    assert torch.equal(loss.model.scaling_layer.scale, torch.from_numpy(g30["scale"]))


def test_lpips_exports_reject_null_shape_and_alignment_errors(L):
    lib = L.lib()
    d, odd = C.c_void_p(4096), C.c_void_p(4100)
    # stem: 1 or 3 channels, float32 / bf16 input, [B,H,W,64] below 2^31
    assert lib.v2v_lpips_stem_hip(None, L.F32, 1, 1, 16, 16, d, d, d, d, 1, d, None) == L.ERR_NULL
    assert lib.v2v_lpips_stem_hip(d, L.F32, 1, 1, 16, 16, d, d, None, d, 1, d, None) == L.ERR_NULL
    assert lib.v2v_lpips_stem_hip(d, L.U8, 1, 1, 16, 16, d, d, d, d, 1, d, None) == L.ERR_DTYPE
    assert lib.v2v_lpips_stem_hip(d, L.F32, 1, 2, 16, 16, d, d, d, d, 1, d, None) == L.ERR_SHAPE
    assert lib.v2v_lpips_stem_hip(d, L.F32, 0, 1, 16, 16, d, d, d, d, 1, d, None) == L.ERR_SHAPE
    assert lib.v2v_lpips_stem_hip(d, L.F32, 2048, 3, 128, 128, d, d, d, d, 1, d, None) == L.ERR_SHAPE          # 2^31 elements
    assert lib.v2v_lpips_stem_hip(d, L.F32, 1, 1, 16, 16, d, d, d, d, 1, odd, None) == L.ERR_ALIGN
    assert lib.v2v_lpips_stem_bwd_hip(None, 1, 1, 16, 16, d, d, 1, d, None) == L.ERR_NULL
    assert lib.v2v_lpips_stem_bwd_hip(d, 1, 4, 16, 16, d, d, 1, d, None) == L.ERR_SHAPE
    assert lib.v2v_lpips_stem_bwd_hip(odd, 1, 3, 16, 16, d, d, 1, d, None) == L.ERR_ALIGN
    # pool: even H and W, C % 8
    assert lib.v2v_lpips_pool_hip(None, 1, 2, 2, 64, d, None) == L.ERR_NULL
    assert lib.v2v_lpips_pool_hip(d, 1, 3, 2, 64, d, None) == L.ERR_SHAPE
    assert lib.v2v_lpips_pool_hip(d, 1, 2, 2, 12, d, None) == L.ERR_SHAPE
    assert lib.v2v_lpips_pool_hip(d, 1, 2, 2, 64, odd, None) == L.ERR_ALIGN
    assert lib.v2v_lpips_pool_bwd_hip(d, None, None, 0, 1, 2, 2, 64, d, None) == L.ERR_NULL
    assert lib.v2v_lpips_pool_bwd_hip(d, d, None, 0, 1, 2, 5, 64, d, None) == L.ERR_SHAPE
    assert lib.v2v_lpips_pool_bwd_hip(d, d, odd, 1, 1, 2, 2, 64, C.c_void_p(8192), None) == L.ERR_ALIGN
    assert lib.v2v_lpips_pool_bwd_hip(d, d, None, 1, 1, 2, 2, 64, d, None) == L.ERR_PARAM                       # dx aliases dy
    # compare: the four VGG widths
    assert lib.v2v_lpips_compare_workspace_bytes(0, 4) < 0 < lib.v2v_lpips_compare_workspace_bytes(3, 65) == 32
    assert lib.v2v_lpips_compare_fwd_hip(d, d, d, 2, 4, 64, None, d, None) == L.ERR_NULL
    assert lib.v2v_lpips_compare_fwd_hip(d, d, d, 2, 4, 96, d, d, None) == L.ERR_SHAPE
    assert lib.v2v_lpips_compare_fwd_hip(d, d, d, 2, 0, 64, d, d, None) == L.ERR_SHAPE
    assert lib.v2v_lpips_compare_fwd_hip(d, odd, d, 2, 4, 64, d, d, None) == L.ERR_ALIGN
    assert lib.v2v_lpips_compare_bwd_hip(d, d, d, None, 2, 4, 64, d, None) == L.ERR_NULL
    assert lib.v2v_lpips_compare_bwd_hip(d, d, d, d, 2, 4, 1024, d, None) == L.ERR_SHAPE
    assert lib.v2v_lpips_compare_bwd_hip(d, d, d, d, 2, 4, 512, odd, None) == L.ERR_ALIGN
    assert b"v2v_lpips_compare_bwd_hip" in lib.v2v_last_error()
