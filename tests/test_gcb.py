"""NER-Net's global context block with the 1x1 convolution in front of it and the residual behind it (v2v_amd/csrc/v2v_gcb.hpp,
nhwc_ops.gcb_nhwc) against the reference's semantics (RecurrentConvLayer_NAM_GCB.forward and ContextBlock2d with pool 'att' and fusion
'channel_add', model/nernet/submodules.py:365-442, :768-770), restated with stock PyTorch ops in tests/gcb_stock.py:
    g = conv_1x1(x);  w = softmax over the pixels of conv_mask(g);  ctx = sum_p g[:, p] w[p]
    out = x + g + conv(PReLU(LayerNorm(conv(ctx))))

The bar is measured in the test, not assumed: the kernels do the reference's float32 arithmetic in another order and round the output to
bf16 once, so against float64 on the same operands an output element may be off by
    4 x (the largest error of the SAME formula in stock float32 PyTorch against float64)  +  one bf16 ulp of that element
and the float32 by-products by 4 x their own stock-float32 error + 8 float32 ulps of their largest term: ctx (a sum of up to 960 values
of g with weights adding up to 1) against the largest |g|, add -- evaluated on the package's OWN ctx, so that the pooling's error is
counted once -- against the largest |add|.  Every figure is printed per case."""
import pytest

from gcb_stock import gcb_ref as _gcb_ref, gcb_weights as _weights, mlp_ref as _mlp_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 32, 8, 8, None), (2, 32, 24, 40, None), (1, 64, 12, 20, None), (3, 128, 6, 10, None), (1, 32, 24, 40, (20, 35))]


def _run(x, ws, valid=None, canvas=None):
    """x [B,C,H,W] float (bf16-exact values) on the CPU -> (out [B,C,H,W] float32 on the CPU, ctx_add [B,2,C]) from the device kernels"""
    import torch
    from v2v_amd import nhwc_ops as N
    xn = (x if canvas is None else canvas).permute(0, 2, 3, 1).contiguous().to(torch.bfloat16).cuda()
    out, ca = N.gcb_nhwc(xn, N.pack_gcb_weights(*(t.cuda() for t in ws)), valid=valid, return_context=True)
    torch.cuda.synchronize()
    return out.float().permute(0, 3, 1, 2).cpu(), ca.cpu()


def _bf16_ulp(v):
    import torch
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -120))) - 7)


def _check(got, ca, x, ws, tag):
    """the bar of the module docstring; x = the valid pixels"""
    import torch
    want, ctx, _, g, _ = _gcb_ref(x, ws, torch.float64)
    o32, c32, _, _, _ = _gcb_ref(x, ws, torch.float32)
    add = _mlp_ref(ca[:, 0], ws, torch.float64)                     # the MLP on the package's OWN context: the pooling's error stays in "ctx"
    e_out, e_ctx, e_add = (float((p.double() - q).abs().max()) for p, q in ((o32, want), (c32, ctx), (_mlp_ref(ca[:, 0], ws, torch.float32), add)))
    err = (got.double() - want).abs()
    f32 = 8 * 2.0 ** -23
    figures = {"out": float(err.max()), "stock_f32_out": e_out, "ctx": float((ca[:, 0].double() - ctx).abs().max()), "stock_f32_ctx": e_ctx,
               "add": float((ca[:, 1].double() - add).abs().max()), "stock_f32_add": e_add, "largest_bf16_ulp": float(_bf16_ulp(want).max())}
    print(tag, figures)
    assert bool((err <= 4 * e_out + _bf16_ulp(want)).all()), figures
    assert figures["ctx"] <= 4 * e_ctx + f32 * float(g.abs().max()), figures
    assert figures["add"] <= 4 * e_add + f32 * float(add.abs().max()), figures


@pytest.mark.parametrize("b,c,h,w,valid", SHAPES)
def test_gcb_matches_the_float64_evaluation(b, c, h, w, valid):
    import torch
    g = torch.Generator().manual_seed(b + c + h + w)
    x = torch.randn((b, c, h, w), generator=g).to(torch.bfloat16).float()
    ws = _weights(c, g)
    got, ca = _run(x, ws, valid)
    hv, wv = valid or (h, w)
    _check(got[:, :, :hv, :wv], ca, x[:, :, :hv, :wv], ws, (b, c, h, w, valid))
    outside = torch.ones((h, w), dtype=torch.bool)
    outside[:hv, :wv] = False
    assert float(got[:, :, outside].abs().max()) == 0.0 if valid else not outside.any()
    again, ca2 = _run(x, ws, valid)
    assert torch.equal(got, again) and torch.equal(ca, ca2), "two runs differ"


def _pooling_case(c, h, w, seed):
    """operands whose g is exact in float32 in any order: x integers in -3..3, conv_1x1 weights multiples of 1/64 in [-1, 1], no bias; and the
    mask logit of a pixel is its x[0]: conv_1x1 passes channel 0 through, conv_mask reads channel 0 alone."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-3, 4, (1, c, h, w), generator=g).float()
    ws = _weights(c, g)
    ws[0] = torch.randint(-64, 65, (c, c, 1, 1), generator=g).float() / 64
    ws[0][0] = 0
    ws[0][0, 0] = 1
    ws[1] = torch.zeros(c)
    ws[2] = torch.zeros(1, c, 1, 1)
    ws[2][0, 0] = 1
    ws[3] = torch.zeros(1)
    return x, ws


def test_one_hot_logit_pools_that_pixel_alone():
    """one pixel's mask logit is +40, every other at most 3: the weights of the others are below e^-37, so ctx is that pixel's g (exact here)"""
    import torch
    x, ws = _pooling_case(32, 8, 12, seed=3)
    x[0, 0, 5, 7] = 40.0
    got, ca = _run(x, ws)
    g = _gcb_ref(x, ws, torch.float64)[3]
    assert float((ca[0, 0].double() - g[0, :, 5, 7]).abs().max()) <= 1e-6
    _check(got, ca, x, ws, "one-hot")


@pytest.mark.parametrize("span", [80, 100])
def test_logits_spanning_a_wide_range_do_not_overflow(span):
    """logits from -span to +span.  e^80 = 5.5e34 is within a factor 6 000 of float32's largest number, so an unshifted softmax is one
    product with g or a few thousand such pixels away from infinity; e^100 is past it outright.  Shifted by the maximum nothing overflows."""
    import torch
    x, ws = _pooling_case(64, 10, 12, seed=4)
    x[0, 0] = torch.linspace(-span, span, 120).round().reshape(10, 12)
    x[0, 0, 4, 4] = float(span)                                                             # two pixels share the maximum
    got, ca = _run(x, ws)
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(ca).all())
    _check(got, ca, x, ws, f"span {span}")


def test_values_outside_the_valid_extent_do_not_move_the_result():
    import torch
    g = torch.Generator().manual_seed(11)
    b, c, h, w, (hv, wv) = 1, 32, 24, 40, (20, 35)
    x = torch.randn((b, c, h, w), generator=g).to(torch.bfloat16).float()
    ws = _weights(c, g)
    x[:, :, hv:] = 0
    x[:, :, :, wv:] = 0
    huge = x.clone()
    huge[:, :, hv:] = 3e38
    huge[:, :, :, wv:] = -3e38
    clean, ca = _run(x, ws, (hv, wv))
    dirty, ca2 = _run(x, ws, (hv, wv), canvas=huge)
    assert torch.equal(clean, dirty) and torch.equal(ca, ca2)
    _check(dirty[:, :, :hv, :wv], ca2, x[:, :, :hv, :wv], ws, "huge outside")
    full, _ = _run(x, ws)                                                                   # pooled over the canvas: another result
    assert not torch.equal(full[:, :, :hv, :wv], clean[:, :, :hv, :wv])


def test_python_side_refuses_what_the_kernels_do_not_take():
    import torch
    from v2v_amd import nhwc_ops as N
    g = torch.Generator().manual_seed(1)
    packed = N.pack_gcb_weights(*(t.cuda() for t in _weights(32, g)))
    x = torch.zeros((1, 8, 8, 32), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match="valid extent 9 x 8"):
        N.gcb_nhwc(x, packed, valid=(9, 8))
    with pytest.raises(ValueError, match="pack_gcb_weights"):
        N.gcb_nhwc(torch.zeros((1, 8, 8, 64), dtype=torch.bfloat16, device="cuda"), packed)
    with pytest.raises(ValueError, match="C must be 32, 64 or 128"):
        N.gcb_nhwc(torch.zeros((1, 8, 8, 96), dtype=torch.bfloat16, device="cuda"), N.pack_gcb_weights(*(t.cuda() for t in _weights(96, g))))
    with pytest.raises(ValueError, match="GCB.channel_add_conv.1.weight"):
        ws = _weights(32, g)
        ws[6] = ws[6][:4]
        N.pack_gcb_weights(*(t.cuda() for t in ws))
