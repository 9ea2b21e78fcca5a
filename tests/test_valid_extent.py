"""The valid-extent helper of the canvas path (nhwc_ops.valid_extent_nhwc, v2v_amd/csrc/v2v_gcb.hpp): exact by construction, so every
check is torch.equal.  A canvas is an NHWC tensor larger than the frame it carries (NER-Net pads to multiples of 8, the matrix-core
kernels want more); what lies outside the valid extent must be zero for a convolution to see the reference's zero padding, and must
repeat the last valid row / column for the x2 upsampling to see the reference's clamped neighbour."""
import pytest

pytestmark = pytest.mark.gpu

# (B, H, W, C), (Hv, Wv): a row and a column outside, rows only, columns only, several rows outside, a one-pixel extent, more than one block
CASES = [((2, 6, 8, 32), (5, 7)), ((1, 8, 8, 64), (7, 8)), ((1, 8, 8, 64), (8, 6)), ((3, 12, 16, 8), (7, 9)), ((1, 4, 4, 8), (1, 1)), ((2, 24, 32, 128), (23, 30))]


def _expected(x, hv, wv, replicate):
    import torch
    want = torch.zeros_like(x)
    want[:, :hv, :wv] = x[:, :hv, :wv]
    if replicate:
        h, w = x.shape[1:3]
        if hv < h:
            want[:, hv, :wv] = x[:, hv - 1, :wv]
        if wv < w:
            want[:, :hv, wv] = x[:, :hv, wv - 1]
        if hv < h and wv < w:
            want[:, hv, wv] = x[:, hv - 1, wv - 1]
    return want


@pytest.mark.parametrize("shape,valid", CASES)
@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
@pytest.mark.parametrize("replicate", [False, True])
def test_outside_cleared_inside_untouched_edge_replicated(shape, valid, dtype, replicate):
    import torch
    from v2v_amd import nhwc_ops as N
    g = torch.Generator().manual_seed(sum(shape) + valid[0])
    x = (torch.randn(shape, generator=g) + 3).to(getattr(torch, dtype)).cuda()      # no zero anywhere: a cleared element shows
    want = _expected(x, *valid, replicate)
    got = N.valid_extent_nhwc(x.clone(), valid, replicate=replicate)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert torch.equal(got[:, :valid[0], :valid[1]], x[:, :valid[0], :valid[1]]) and float(got[:, :valid[0], :valid[1]].float().abs().min()) > 0


def test_full_extent_changes_nothing():
    import torch
    from v2v_amd import nhwc_ops as N
    x = torch.randn((1, 6, 8, 32), generator=torch.Generator().manual_seed(2)).bfloat16().cuda()
    assert torch.equal(N.valid_extent_nhwc(x.clone(), (6, 8), replicate=True), x)


@pytest.mark.parametrize("shape,valid", [((2, 6, 8, 32), (5, 7)), ((1, 8, 8, 64), (7, 8)), ((1, 8, 8, 64), (8, 6)), ((1, 24, 32, 128), (23, 30))])
@pytest.mark.parametrize("with_skip", [False, True])
def test_upsampling_a_prepared_canvas_equals_upsampling_the_cropped_tensor(shape, valid, with_skip):
    """inside twice the extent, bit for bit: the kernel's 0.75 in[i] + 0.25 in[i + 1] at the last valid row / column reads the replicated
    neighbour where the cropped tensor's upsampling reads its clamped one.  With the sum skip both operands are prepared."""
    import torch
    from v2v_amd import nhwc_ops as N
    g = torch.Generator().manual_seed(sum(shape))
    hv, wv = valid
    x, skip = (torch.randn(shape, generator=g).bfloat16().cuda() for _ in range(2))
    skip = skip if with_skip else None
    want = N.upsample2x_nhwc(x[:, :hv, :wv].contiguous(), None if skip is None else skip[:, :hv, :wv].contiguous())
    N.valid_extent_nhwc(x, valid, replicate=True)
    if skip is not None:
        N.valid_extent_nhwc(skip, valid, replicate=True)
    got = N.upsample2x_nhwc(x, skip)
    torch.cuda.synchronize()
    assert torch.equal(got[:, :2 * hv, :2 * wv], want)
    cleared = N.valid_extent_nhwc(got, (2 * hv, 2 * wv))                              # "its output is cleared outside twice the extent"
    assert torch.equal(cleared[:, :2 * hv, :2 * wv], want) and float(cleared[:, 2 * hv:].float().abs().max() if hv < shape[1] else 0) == 0
