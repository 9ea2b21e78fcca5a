"""The head for 9 to 16 input channels (nhwc_ops.to_nhwc16_bf16 / pack_head16in_weights / conv_head16in_nhwc, v2v_amd/csrc/v2v_nam_head.hpp):
relu(conv5x5(x, pad 2) + bias) -> 32 channels, exact on integers as tests/test_forward_ops.py pins the other forward operators: inputs in
-3..3 and weights in -2..2 are exact in bf16, biases are quarters, so every sum (at most 25 * 16 * 6 + 2) is exact in fp32 in any order and
the device result must be the float64 result rounded once to bf16, bit for bit.  The weights are random, hence asymmetric: a transposed tap
or a swapped row / column shows."""
import pytest

pytestmark = pytest.mark.gpu

# (B, C, H, W): the issue's sizes at 10 and 16 channels, batch 2, and a frame whose pixels fill neither a wave (32) nor a workgroup (128)
SHAPES = [(1, 10, 16, 16), (1, 16, 16, 16), (1, 10, 24, 40), (1, 16, 24, 40), (1, 10, 40, 56), (1, 16, 40, 56), (2, 10, 24, 40), (1, 13, 9, 13)]


def _ints(gen, shape, lo, hi):
    import torch
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _device(x, w, bias, relu=True):
    import torch
    from v2v_amd import nhwc_ops as N
    out = N.conv_head16in_nhwc(N.to_nhwc16_bf16(x.cuda()), N.pack_head16in_weights(w.cuda()), bias.cuda(), relu=relu)
    torch.cuda.synchronize()
    return out.permute(0, 3, 1, 2).cpu()


def _want(x, w, bias, relu=True):
    import torch
    import torch.nn.functional as F
    y = F.conv2d(x.double(), w.double(), bias.double(), padding=2)
    return (torch.relu(y) if relu else y).to(torch.bfloat16)


@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape", SHAPES)
def test_head_exact_on_integers(shape, relu):
    import torch
    b, c, h, w = shape
    gen = torch.Generator().manual_seed(sum(shape))
    x, wt, bias = _ints(gen, shape, -3, 3), _ints(gen, (32, c, 5, 5), -2, 2), _ints(gen, (32,), -8, 8) / 4
    got, want = _device(x, wt, bias, relu), _want(x, wt, bias, relu)
    assert float(want.float().abs().max()) > 8 and torch.equal(got, want)


@pytest.mark.parametrize("shape", [(1, 10, 16, 16), (2, 16, 24, 40), (1, 10, 40, 56)])
def test_one_hot_inputs_at_the_corners_and_the_last_pixel(shape):
    """one input element set: the output is the (flipped) 5 x 5 window of that channel's weights around it, cut at the border"""
    import torch
    b, c, h, w = shape
    gen = torch.Generator().manual_seed(7)
    wt, bias = _ints(gen, (32, c, 5, 5), -2, 2), torch.zeros(32)
    for k, (y, x0) in enumerate([(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h - 1, w - 1)]):
        x = torch.zeros(shape)
        x[b - 1 if k == 4 else 0, (3 * k + 1) % c, y, x0] = 1.0                   # the fifth: the last pixel of the last image
        got, want = _device(x, wt, bias, relu=False), _want(x, wt, bias, relu=False)
        assert int((want != 0).sum()) > 32 and torch.equal(got, want), (k, y, x0)


def test_layout_pads_the_channels_and_takes_any_strides():
    import torch
    from v2v_amd import nhwc_ops as N
    gen = torch.Generator().manual_seed(3)
    big = torch.randn((2, 20, 12, 18), generator=gen).cuda()
    for x in (big[:, :10], big[:, 4:20], big[:, 1:14, 2:10, ::2], big[:, :12].permute(0, 1, 3, 2)):
        want = torch.zeros((x.shape[0], x.shape[2], x.shape[3], 16), dtype=torch.bfloat16, device="cuda")
        want[..., :x.shape[1]] = x.permute(0, 2, 3, 1).to(torch.bfloat16)
        assert torch.equal(N.to_nhwc16_bf16(x), want)


def test_python_side_refuses_what_the_kernels_do_not_take():
    import torch
    from v2v_amd import nhwc_ops as N
    with pytest.raises(ValueError, match="9 <= C <= 16"):
        N.to_nhwc16_bf16(torch.zeros((1, 3, 8, 8), device="cuda"))
    with pytest.raises(ValueError, match="9 <= Cin <= 16"):
        N.pack_head16in_weights(torch.zeros((32, 3, 5, 5), device="cuda"))
    with pytest.raises(ValueError, match="pack_head16in_weights"):
        N.conv_head16in_nhwc(torch.zeros((1, 8, 8, 16), dtype=torch.bfloat16, device="cuda"), torch.zeros(5, dtype=torch.bfloat16, device="cuda"),
                             torch.zeros(32, device="cuda"))
