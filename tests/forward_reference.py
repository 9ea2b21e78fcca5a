"""Float64 references of the forward operators of v2v_amd/nhwc_ops.py that store bfloat16, on the CPU: what "right" means for the
convolutions of v2v_amd/csrc/v2v_convlstm.hpp (conv_nhwc on every tile, the halo tiles, the head, the stem), the two upsampling kernels,
the prediction layer and the 16-channel family of v2v_narrow.hpp.

Every function takes and returns NCHW float64 tensors and is a plain formula written from the reference network's semantics
(model/submodules.py: ConvLayer :6-33, UpsampleConvLayer :68-96, ResidualBlock :143-177; model/unet.py :58-64, :304-307, :350), not from the
kernels.  The results are NOT rounded at the end: the caller rounds once (`.to(torch.bfloat16)`), so the unrounded value stays available to
the checks on it (how many outputs round, how many are ties).  Roundings INSIDE an operator -- the bf16 skip sum, the residual block's
intermediate -- are part of the formula, through backward_reference.bf16_round.
tests/test_forward_reference.py checks each of them against the stock PyTorch operator in float64 (to 1e-12), tests/test_forward_ops.py compares
the device kernels with them.
"""
import torch

from backward_reference import F64, bf16_round, ref_conv_fwd, upsample2x_matrix


def ref_conv(x, w, bias, stride=1, residual=None, relu=False):
    """conv_nhwc: [relu](conv_ks(x, stride, pad ks // 2) + bias [+ residual]), unrounded."""
    out = ref_conv_fwd(x, w, bias, stride)
    if residual is not None:
        out = out + residual
    return torch.relu(out) if relu else out


def pad8(w):
    """[Cout, Cin <= 8, ks, ks] -> [Cout, 8, ks, ks], the channels Cin..7 zero."""
    out = torch.zeros((w.shape[0], 8, w.shape[2], w.shape[3]), dtype=F64)
    out[:, :w.shape[1]] = w
    return out


def ref_conv_pad8(x8, w, bias, stride=1, relu=False):
    """conv_head_nhwc (stride 1, ks 3 / 5), conv_stem_nhwc (stride 2, ks 3), conv_head16_nhwc (stride 1, ks 3): the same convolution on an
    input of 8 channels of which the weight w [Cout, Cin <= 8, ks, ks] reads the first Cin; whatever x8 holds beyond them does not count."""
    return ref_conv(x8, pad8(w), bias, stride, None, relu)


def ref_resblock16(x, w1, b1, w2, b2):
    """resblock16_nhwc: mid = bf16(relu(conv1(x) + b1)), out = relu(conv2(mid) + b2 + x) -> (mid unrounded, out unrounded)."""
    mid = ref_conv(x, w1, b1, relu=True)
    return mid, ref_conv(bf16_round(mid), w2, b2, residual=x, relu=True)


def skip_sum(x, skip):
    """bf16(x + skip), the stock bf16 add in front of the decoder layers and the prediction layer; x itself without a skip."""
    return x if skip is None else bf16_round(x + skip)


def ref_upsample2x(x, skip=None):
    """upsample2x_nhwc: up2(bf16(x + skip)), out[2m + a, 2n + c] with the weights 1/16 {9, 3, 3, 1} on the clamped neighbours = U_H s U_W^T."""
    s = skip_sum(x, skip)
    return torch.einsum("jk,bckm,lm->bcjl", upsample2x_matrix(s.shape[2]), s, upsample2x_matrix(s.shape[3]))


def ref_upsample2x_cat(x, skip=None):
    """upsample2x_cat_nhwc: cat(up2(x), up2(skip)) along the channels (no sum, so no rounding in front)."""
    return ref_upsample2x(x) if skip is None else torch.cat([ref_upsample2x(x), ref_upsample2x(skip)], 1)


def ref_conv1x1(x, skip, w, bias):
    """conv1x1_nhwc: bias + sum_c bf16(w[o, c]) bf16(x + skip)[c], unrounded (the float32 output is this value, the bf16 output its rounding)."""
    wb = bf16_round(w.reshape(w.shape[0], -1))
    return torch.einsum("oc,bchw->bohw", wb, skip_sum(x, skip)) + bias.view(1, -1, 1, 1)


# ---- what the integer recipes of tests/test_forward_ops.py rest on ------------------------------------------------------------------------
def abs_sum_conv(x, w, bias, stride=1, residual=None):
    """sum |x| |w| + |bias| + |residual| per output: the largest magnitude any partial sum of the operator can reach, in any order."""
    return ref_conv(x.abs(), w.abs(), bias.abs(), stride, None if residual is None else residual.abs())


def rounds(v):
    """Elements the output rounding does something to or is at risk on: above 256 in magnitude, or with a fraction bf16 does not hold."""
    return (v.abs() > 256) | (bf16_round(v) != v)


def ties(v):
    """Elements exactly halfway between two neighbouring bf16 values: |v - bf16(v)| is half an ulp of v's binade (2^(e - 8) for
    |v| = m 2^e, 0.5 <= m < 1)."""
    _, e = torch.frexp(v.abs())
    return (v != 0) & ((v - bf16_round(v)).abs() * 2 == torch.ldexp(torch.ones_like(v), e - 8))
