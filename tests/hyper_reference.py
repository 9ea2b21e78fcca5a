"""Float64 references of the six kernels of v2v_amd/csrc/v2v_hyper.hpp (HyperE2VID's dynamic decoder), on the CPU: what "right" means for
hyper_context_nhwc8, context_conv_nhwc, tanh_bf16_, hyper_atoms, pack_dynconv_weights and dynconv_nhwc of v2v_amd/nhwc_ops.py.

Every function is an explicit formula over indices (slices and loops over the taps) in the kernels' own layouts -- NHWC activations, atoms
[B,H,W,25,6] -- and calls none of the operators under test.  tests/test_hyper_reference.py checks each of them against tests/hyper_stock.py
in float64 (1e-12) and against golden G26; tests/test_hyper_ops.py compares the device kernels with them.

The roundings a kernel makes on purpose are arguments (`round_weight`, `round_features`): on, the formula is the kernel's contract; off, it
is the real-number expression of the stock graph.  The seeded integer operands of the exact GPU cases are built here too (`*_case`), so that
the conditions they rest on (sums below 256, outputs that are not all zero, features that do round) are asserted on the CPU.
"""
import functools

import torch

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
N_TAPS, N_ATOMS, N_BASES, N_COEFF, COEFF_PAD, CIN, COUT = 25, 6, 12, 72, 128, 256, 128

# the shapes (B, H, W) of the dynamic convolution's tests: the smallest that reach every path of the 8 x 16 tile with its 2-pixel halo --
# one pixel; less than the halo; one short of a tile; one past it (a 1-row / 1-column partial tile whose halo is the neighbour tile); whole
# tiles in a batch; partial tiles in a batch (image seams between partial tiles); partial tiles in both directions with three images
DYNCONV_SHAPES = [(1, 1, 1), (1, 3, 5), (1, 7, 15), (1, 9, 17), (2, 8, 16), (2, 12, 20), (3, 10, 14)]


def bf16_round(t):
    """t -> the float64 values of rne_bf16(rne_f32(t)): what a kernel that forms t in float32 and rounds it to bfloat16 keeps."""
    return t.to(F32).to(BF16).to(F64)


# ---- the formulas -------------------------------------------------------------------------------------------------------------------
def ref_context(events, prev):
    """events [B,C,H,W], prev [B,1,H,W] -> [B,H/4,W/4,8] (NHWC, channels C+1..7 zero):
    out[b, y, x, c] = 0.25 (v[4y+1, 4x+1] + v[4y+1, 4x+2] + v[4y+2, 4x+1] + v[4y+2, 4x+2]),  v = cat(events, prev)[b, c]."""
    v = torch.cat([events.to(F64), prev.to(F64)], 1)
    b, c, hh, ww = v.shape
    assert hh % 4 == 0 and ww % 4 == 0 and c <= 8
    out = torch.zeros((b, hh // 4, ww // 4, 8), dtype=F64)
    mean = 0.25 * (v[:, :, 1::4, 1::4] + v[:, :, 1::4, 2::4] + v[:, :, 2::4, 1::4] + v[:, :, 2::4, 2::4])
    out[..., :c] = mean.permute(0, 2, 3, 1)
    return out


def ref_context_conv(x8, weight, bias, round_weight=True):
    """x8 [B,h,w,8] (only the first Cin channels are read), weight [32,Cin,3,3], bias [32] -> [B,h,w,32]:
    out[b, y, x, o] = bias[o] + sum_{c < Cin, ky, kx} w[o, c, ky, kx] x8[b, y + ky - 1, x + kx - 1, c], zero outside the image;
    round_weight: w = rne_bf16(weight), as the kernel rounds it."""
    w = bf16_round(weight) if round_weight else weight.to(F64)
    cin = w.shape[1]
    b, h, wd, _ = x8.shape
    xp = torch.zeros((b, h + 2, wd + 2, cin), dtype=F64)
    xp[:, 1:1 + h, 1:1 + wd] = x8[..., :cin].to(F64)
    out = bias.to(F64).view(1, 1, 1, -1).repeat(b, h, wd, 1)
    for ky in range(3):
        for kx in range(3):
            out += torch.einsum("bhwc,oc->bhwo", xp[:, ky:ky + h, kx:kx + wd], w[:, :, ky, kx])
    return out


def ref_atoms(coeff, bases):
    """coeff [..., >= 72] PRE-activation coefficients (index m * 12 + k; columns from 72 on are padding and never read), bases [12,25] ->
    atoms [..., 25, 6]:  atoms[p, l, m] = sum_k tanh(coeff[p, m * 12 + k]) bases[k, l]."""
    lead = tuple(coeff.shape[:-1])
    t = torch.tanh(coeff[..., :N_COEFF].to(F64)).reshape(-1, N_ATOMS, N_BASES)
    out = torch.zeros((t.shape[0], N_TAPS, N_ATOMS), dtype=F64)
    for k in range(N_BASES):
        out += bases[k].to(F64).view(1, N_TAPS, 1) * t[:, :, k].unsqueeze(1)
    return out.reshape(lead + (N_TAPS, N_ATOMS))


def tap_offset(l):
    """Window tap l -> (dy, dx) in -2..2: the tap reads the input at p + (dy, dx)."""
    return l // 5 - 2, l % 5 - 2


def ref_features(x, atoms, round_features=True):
    """x [B,H,W,C], atoms [B,H,W,25,6] -> F [B,H,W,C,6]:  F[p, c, m] = sum_l atoms[p, l, m] x[p + tap_offset(l), c], zero outside the image;
    round_features: F = rne_bf16(F), what the kernel hands to the matrix cores."""
    b, h, w, c = x.shape
    xp = torch.zeros((b, h + 4, w + 4, c), dtype=F64)
    xp[:, 2:2 + h, 2:2 + w] = x.to(F64)
    feat = torch.zeros((b, h, w, c, N_ATOMS), dtype=F64)
    for l in range(N_TAPS):
        dy, dx = tap_offset(l)
        feat += xp[:, 2 + dy:2 + dy + h, 2 + dx:2 + dx + w, :, None] * atoms[:, :, :, l, None, :].to(F64)
    return bf16_round(feat) if round_features else feat


def ref_dynconv(x, atoms, weight, bias, relu, round_features=True, round_weight=True):
    """x [B,H,W,256], atoms [B,H,W,25,6], weight [128, 256 * 6(, 1, 1)] (column c * 6 + m), bias [128] -> y [B,H,W,128] float64, NOT rounded:
    y[p, o] = bias[o] + sum_{c, m} w[o, c * 6 + m] F[p, c, m]  (ref_features), then max(y, 0) when relu."""
    w = weight.reshape(weight.shape[0], -1)
    w = bf16_round(w) if round_weight else w.to(F64)
    feat = ref_features(x, atoms, round_features)
    y = torch.einsum("bhwk,ok->bhwo", feat.reshape(feat.shape[:3] + (-1,)), w) + bias.to(F64).view(1, 1, 1, -1)
    return torch.clamp_min(y, 0.0) if relu else y


def ref_pack(weight):
    """weight [128, 256 * 6] (any dtype) -> the packed stream as [4 * 6 * 128 * 64] of the same dtype:
    wp[((cb * 6 + m) * 128 + col) * 64 + k] = weight[col, (cb * 64 + k) * 6 + m]."""
    w = weight.reshape(COUT, -1)
    assert w.shape[1] == CIN * N_ATOMS
    return w.reshape(COUT, CIN // 64, 64, N_ATOMS).permute(1, 3, 0, 2).contiguous().reshape(-1)          # [col, cb, k, m] -> [cb, m, col, k]


def bf16_ulp(v):
    """The spacing of bfloat16 at |v| (float64 tensor; subnormals: 2^-133)."""
    _, e = torch.frexp(v.abs().to(F64))                                      # |v| = f 2^e, f in [0.5, 1)
    e = torch.where(v == 0, torch.full_like(e, -125), torch.clamp(e, min=-125))
    return torch.ldexp(torch.ones_like(v, dtype=F64), e - 8)


# ---- seeded operands of the exact cases ---------------------------------------------------------------------------------------------
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * int(k) for i, k in enumerate(key)) + 20260)


def _ints(g, k, *shape):
    return torch.randint(-k, k + 1, shape, generator=g).to(F64)


def _sparse_signs(g, keep, *shape):
    """+-1 where kept (probability `keep`), else 0."""
    sign = torch.randint(0, 2, shape, generator=g).to(F64) * 2 - 1
    return sign * (torch.rand(shape, generator=g) < keep)


@functools.lru_cache(maxsize=None)
def dynconv_weight_ints():
    """W [128, 1536] in {-1, 0, 1} at density 1/8 and bias [128], integers in -8..8: shared by every integer case."""
    g = _gen(7)
    return _sparse_signs(g, 1 / 8, COUT, CIN * N_ATOMS), _ints(g, 8, COUT)


@functools.lru_cache(maxsize=None)
def dynconv_ints_case(b, h, w):
    """(x, atoms, W, bias, F, y) of the integer case: x in {-1, 0, 1} at density 1/2, atoms drawn from {-1, 0, 1} and kept at density 1/5
    (dense on the 1 x 1 image, where only the centre tap can act), W and bias of dynconv_weight_ints.  |F| <= 25 is exact in bf16, so every
    fp32 sum is an integer below 2^24: exact in any order.  y is before the ReLU."""
    g = _gen(b, h, w)
    x = _sparse_signs(g, 1 / 2, b, h, w, CIN)
    atoms = _ints(g, 1, b, h, w, N_TAPS, N_ATOMS)
    if (h, w) != (1, 1):
        atoms = atoms * (torch.rand(atoms.shape, generator=g) < 1 / 5)
    wgt, bias = dynconv_weight_ints()
    return x, atoms, wgt, bias, ref_features(x, atoms), ref_dynconv(x, atoms, wgt, bias, relu=False)


@functools.lru_cache(maxsize=None)
def dynconv_rounding_case():
    """(x, atoms, W, bias, F before its rounding, y) at (1, 9, 17): x in -8..8, dense atoms in -4..4, the sparse W.  |F| passes 256, so F's
    round-to-nearest-even (ties included: F is an integer) changes it; y, an integer below 2^24, is before the ReLU and the output's rounding.
    Signs: independent zero-mean draws leave |F| at 63 rms and above 256 for 2e-5 of the features, so the rounding would hardly act.  Here
    the sign of x is one per channel and the sign of an atom one per m (magnitudes drawn freely): the 25 products of one F then share their
    sign and |F| is 235 +- 43 inside the image, while x, the atoms, F and y all keep both signs."""
    g = _gen(1, 9, 17, 3)
    x = _ints(g, 8, 1, 9, 17, CIN).abs() * (torch.randint(0, 2, (CIN,), generator=g).to(F64) * 2 - 1)
    atoms = _ints(g, 4, 1, 9, 17, N_TAPS, N_ATOMS).abs() * torch.tensor([1.0, -1.0, -1.0, 1.0, -1.0, 1.0], dtype=F64)
    wgt, bias = dynconv_weight_ints()
    return x, atoms, wgt, bias, ref_features(x, atoms, round_features=False), ref_dynconv(x, atoms, wgt, bias, relu=False)


# (Cin, B, h, w) of the context convolution's integer case: B h w 4 work-items are never a multiple of the 256-wide block
CONTEXT_CONV_CASES = [(cin, b, h, w) for cin in (1, 6, 8) for b, h, w in ((3, 1, 1), (2, 1, 7), (3, 5, 3), (2, 13, 17))]


@functools.lru_cache(maxsize=None)
def context_conv_ints_case(cin, b, h, w):
    """(x8, weight, bias, want): x8 [B,h,w,8] and weight [32,Cin,3,3] integers in -2..2, bias in -4..4.  The channels from Cin on hold
    integers too, not zeros: the kernel must give them a zero weight."""
    g = _gen(cin, b, h, w, 5)
    x8, wgt, bias = _ints(g, 2, b, h, w, 8), _ints(g, 2, 32, cin, 3, 3), _ints(g, 4, 32)
    return x8, wgt, bias, ref_context_conv(x8, wgt, bias)
