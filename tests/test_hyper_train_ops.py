"""The dynamic decoder's backward operators and BatchNorm on batch statistics, one by one (v2v_amd/nhwc_ops.py; kernels: the training
section of v2v_amd/csrc/v2v_hyper.hpp), at B = 2, 12 x 20 pixels at the dynamic convolution's scale: partial tiles and tile seams on both
axes (tiles are 8 x 16) and a batch stride.  Each operator equals its float64 formula bit for bit on small integers (every sum exact in its
output type), stays within its output rounding on real values, and gives equal bits twice."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

B, H, W = 2, 12, 20
CORNERS = ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (7, 15), (7, 16), (8, 15), (8, 16))   # image corners, around a tile corner


@pytest.fixture(scope="module")
def ops():
    from v2v_amd import _lib, nhwc_ops
    _lib.require_gpu()
    return nhwc_ops


def _gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def ints(seed, shape, lo, hi, keep=1.0):
    g = _gen(seed)
    v = torch.randint(lo, hi + 1, shape, generator=g).double()
    if keep < 1.0:
        v = v * (torch.rand(shape, generator=g) < keep)
    return v.cuda()


def reals(seed, shape, scale=1.0):
    return (torch.randn(shape, generator=_gen(seed)) * scale).to(torch.bfloat16).double().cuda()       # bf16 values, as float64


# ---- the float64 formulas (x [B,H,W,256], atoms [B,H,W,25,6], dF [B,H,W,256,6], dz [B,H,W,128], w [128,1536]) ----
def ref_features(x, atoms):
    xp = torch.nn.functional.pad(x, (0, 0, 2, 2, 2, 2))
    f = 0
    for l in range(25):
        dy, dx = divmod(l, 5)
        f = f + xp[:, dy:dy + H, dx:dx + W, :, None] * atoms[:, :, :, l, None, :]
    return f


def ref_df(dz, w):
    return (dz.reshape(-1, 128) @ w).reshape(B, H, W, 256, 6)


def ref_datoms(x, df):
    xp = torch.nn.functional.pad(x, (0, 0, 2, 2, 2, 2))
    return torch.stack([(xp[:, l // 5:l // 5 + H, l % 5:l % 5 + W, :, None] * df).sum(3) for l in range(25)], 3)


def ref_dx(atoms, df):
    out = torch.zeros((B, H + 4, W + 4, 256), dtype=torch.float64, device=df.device)
    for l in range(25):
        dy, dx = divmod(l, 5)
        out[:, dy:dy + H, dx:dx + W] += (atoms[:, :, :, l, None, :] * df).sum(-1)
    return out[:, 2:-2, 2:-2]


def ref_dw(dz, f):
    return torch.einsum("bhwo,bhwcm->ocm", dz, f).reshape(128, 1536)


def to_kernel_df(df):
    """[B,H,W,256,6] -> the kernels' bf16 [B,H,W,4,6,64]."""
    return df.reshape(B, H, W, 4, 64, 6).permute(0, 1, 2, 3, 5, 4).contiguous().to(torch.bfloat16)


def from_kernel_df(df):
    return df.double().permute(0, 1, 2, 3, 5, 4).reshape(B, H, W, 256, 6)


def bf(t):
    return t.to(torch.bfloat16).contiguous()


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def onehot_df():
    """dF that is non-zero only at the image corners and around a tile corner, another (channel, atom) at each."""
    df = torch.zeros((B, H, W, 256, 6), dtype=torch.float64, device="cuda")
    for i, (y, x) in enumerate(CORNERS):
        df[i % B, y, x, (37 * i + 5) % 256, i % 6] = 1.0
        df[(i + 1) % B, y, x, (91 * i + 64) % 256, (i + 3) % 6] = -2.0
    return df


# ---- exact on integers -----------------------------------------------------------------------------------------------------------------
def test_df_equals_the_formula_bit_for_bit_on_integers(ops):
    dz, w = ints(1, (B, H, W, 128), -2, 2), ints(2, (128, 1536), -1, 1)          # |sum| <= 256: exact in bf16
    got = ops.dynconv_df_nhwc(bf(dz), ops.pack_dynconv_weights_t(w.float().reshape(128, 1536, 1, 1)))
    assert torch.equal(from_kernel_df(got), ref_df(dz, w))
    assert same_bits(got, ops.dynconv_df_nhwc(bf(dz), ops.pack_dynconv_weights_t(w.float().reshape(128, 1536, 1, 1))))


@pytest.mark.parametrize("which", ["dense", "onehot"])
def test_datoms_equals_the_formula_bit_for_bit_on_integers(ops, which):
    x = ints(3, (B, H, W, 256), -2, 2)
    df = ints(4, (B, H, W, 256, 6), -1, 1) if which == "dense" else onehot_df()
    got = ops.dynconv_datoms_nhwc(bf(x), to_kernel_df(df))
    assert torch.equal(got.double(), ref_datoms(x, df))                              # |sum| <= 512 < 2^24
    assert same_bits(got, ops.dynconv_datoms_nhwc(bf(x), to_kernel_df(df)))


@pytest.mark.parametrize("which", ["dense", "onehot"])
def test_dx_equals_the_formula_bit_for_bit_on_integers(ops, which):
    atoms = ints(5, (B, H, W, 25, 6), -1, 1)
    df = ints(6, (B, H, W, 256, 6), -1, 1) if which == "dense" else onehot_df()
    got = ops.dynconv_dx_nhwc(atoms.float().contiguous(), to_kernel_df(df))
    assert torch.equal(got.double(), ref_dx(atoms, df))                              # |sum| <= 150 (300 one-hot): exact in bf16
    assert same_bits(got, ops.dynconv_dx_nhwc(atoms.float().contiguous(), to_kernel_df(df)))


def test_dx_equals_autograd_of_the_stock_dynamic_convolution_on_integers(ops):
    from hyper_stock import stock_dynconv
    x = ints(7, (B, 256, H, W), -2, 2).requires_grad_(True)
    atoms = ints(8, (B, H, W, 25, 6), -1, 1)
    w = ints(9, (128, 1536), -1, 1)
    dz = ints(10, (B, H, W, 128), -1, 1) * (torch.arange(128, device="cuda") == 35)           # one channel: |dF| <= 1, |dX| <= 150
    p = {"dynamic_conv.compositional_coefficients": w.reshape(128, 1536, 1, 1), "dynamic_conv.bias": torch.zeros(128, dtype=torch.float64, device="cuda")}
    y = stock_dynconv(x, atoms.permute(0, 4, 3, 1, 2), p)
    y.backward(dz.permute(0, 3, 1, 2))
    df = ops.dynconv_df_nhwc(bf(dz), ops.pack_dynconv_weights_t(w.float().reshape(128, 1536, 1, 1)))
    got = ops.dynconv_dx_nhwc(atoms.float().contiguous(), df)
    assert torch.equal(got.double(), x.grad.permute(0, 2, 3, 1))


def test_dw_and_db_equal_the_formula_bit_for_bit_on_integers(ops):
    dz = ints(11, (B, H, W, 128), -2, 2)
    x, atoms = ints(12, (B, H, W, 256), -1, 1), ints(13, (B, H, W, 25, 6), -1, 1)     # |F| <= 25: exact in bf16; |dW| <= 2 * 25 * 480 < 2^24
    dw, db = ops.dynconv_wgrad_nhwc(bf(dz), bf(x), atoms.float().contiguous())
    assert torch.equal(dw.double().reshape(128, 1536), ref_dw(dz, ref_features(x, atoms)))
    assert torch.equal(db.double(), dz.sum((0, 1, 2)))
    dw2, db2 = ops.dynconv_wgrad_nhwc(bf(dz), bf(x), atoms.float().contiguous())
    assert same_bits(dw, dw2) and same_bits(db, db2)


def test_dw_sees_every_pixel_once_one_hot_at_corners_and_seams(ops):
    """dz one-hot at the image corners and around a tile corner, x = 1 everywhere, atoms = 1 at ONE tap: dW counts the window pixels
    inside the image, exactly."""
    dz = torch.zeros((B, H, W, 128), dtype=torch.float64, device="cuda")
    for i, (y, x) in enumerate(CORNERS):
        dz[i % B, y, x, (17 * i + 3) % 128] = 1.0
    x = ints(14, (B, H, W, 256), -2, 2)
    atoms = torch.zeros((B, H, W, 25, 6), dtype=torch.float64, device="cuda")
    for i, (y, xx) in enumerate(CORNERS):
        atoms[i % B, y, xx, (3 * i) % 25, i % 6] = 1.0
        atoms[i % B, y, xx, (3 * i + 11) % 25, (i + 2) % 6] = -1.0
    dw, _ = ops.dynconv_wgrad_nhwc(bf(dz), bf(x), atoms.float().contiguous())
    assert torch.equal(dw.double().reshape(128, 1536), ref_dw(dz, ref_features(x, atoms)))


# ---- real values: within the output rounding of float64 on the bf16 operands --------------------------------------------------------------
def _report(name, got, ref, bound):
    excess = float(((got - ref).abs() - bound).max())
    rel = float((got - ref).norm() / ref.norm())
    print(f"{name}: relative L2 error {rel:.3e}, worst (|error| - bound) {excess:.3e}")
    assert excess <= 0.0, name


def test_real_valued_results_are_within_their_output_rounding(ops):
    """bound = 2^-8 |ref| for a bf16 store (none for a float32 result) + n 2^-24 sum |terms|: the worst case of n float32 additions.  dW also
    carries the bf16 rounding of the recomputed features, 2^-8 sum_p |dz| |F|."""
    dz, w = reals(20, (B, H, W, 128)), reals(21, (128, 1536), 0.05)
    x, atoms32 = reals(22, (B, H, W, 256)), (torch.randn((B, H, W, 25, 6), generator=_gen(23)) * 0.2).float().cuda()
    atoms = atoms32.double()
    e24 = 2.0 ** -24
    df_k = ops.dynconv_df_nhwc(bf(dz), ops.pack_dynconv_weights_t(w.float().reshape(128, 1536, 1, 1)))
    ref = ref_df(dz, w)
    _report("dF", from_kernel_df(df_k), ref, 2.0 ** -8 * ref.abs() + 128 * e24 * ref_df(dz.abs(), w.abs()))
    df = from_kernel_df(df_k)                                                    # the bf16 dF the next kernels read
    ref = ref_datoms(x, df)
    _report("dAtoms", ops.dynconv_datoms_nhwc(bf(x), df_k).double(), ref, 256 * e24 * ref_datoms(x.abs(), df.abs()))
    ref = ref_dx(atoms, df)
    _report("dX", ops.dynconv_dx_nhwc(atoms32, df_k).double(), ref, 2.0 ** -8 * ref.abs() + 150 * e24 * ref_dx(atoms.abs(), df.abs()))
    f, fa = ref_features(x, atoms), ref_features(x.abs(), atoms.abs())
    dw, db = ops.dynconv_wgrad_nhwc(bf(dz), bf(x), atoms32)
    _report("dW", dw.double().reshape(128, 1536), ref_dw(dz, f), (2.0 ** -8 + (B * H * W + 25) * e24) * ref_dw(dz.abs(), fa))
    _report("db", db.double(), dz.sum((0, 1, 2)), B * H * W * e24 * dz.abs().sum((0, 1, 2)))


# ---- BatchNorm on batch statistics --------------------------------------------------------------------------------------------------------
def _bn_case(cs, cv, seed, integer=False):
    m = (B, H // 4 * 2, W // 4 * 2)                                              # [2, 6, 10] rows at the context's scale
    z = ints(seed, m + (cs,), -8, 8) if integer else reals(seed, m + (cs,), 1.5) + reals(seed + 1, (cs,), 1.0)
    z = z.to(torch.bfloat16).double()                                           # what the convolution stores
    if cv < cs:
        z[..., cv:] = 0.0                                                        # the padding columns of the 72-output convolution
    g = _gen(seed + 2)
    gamma, beta = (1.0 + 0.1 * torch.randn(cv, generator=g)).float().cuda(), (0.3 * torch.randn(cv, generator=g)).float().cuda()
    dy = (torch.randn(m + (cs,), generator=g)).float().cuda()
    return z, gamma, beta, dy


def _ulp(t):
    return float(t.abs().max()) * 2.0 ** -23


@pytest.mark.parametrize("cs,cv", [(64, 64), (128, 72)])
def test_batchnorm_mean_is_exact_on_integers(ops, cs, cv):
    z, _, _, _ = _bn_case(cs, cv, 30, integer=True)
    mean, var, _ = ops.hyper_bn_stats(bf(z))
    rows = z.reshape(-1, cs)
    assert torch.equal(mean, rows.mean(0).float())                               # the float64 mean, rounded once
    assert torch.equal(var[cv:], torch.zeros_like(var[cv:]))
    assert same_bits(mean, ops.hyper_bn_stats(bf(z))[0])


@pytest.mark.parametrize("cs,cv", [(64, 64), (128, 72)])
def test_batchnorm_statistics_and_backward_against_float64(ops, cs, cv):
    """Bar for every float32 result: 4 x the error of float32 F.batch_norm on the same data + one float32 ulp of the largest value (both as
    maxima over the tensor).  dz is stored as bf16: its bar adds that store's rounding, 2^-8 |ref|."""
    from v2v_amd.train import _update_running_stats
    F = torch.nn.functional
    z, gamma, beta, dy = _bn_case(cs, cv, 40)
    rows64, n = z.reshape(-1, cs)[:, :cv], z.numel() // cs
    # float64 formula
    mean64, var64 = rows64.mean(0), rows64.var(0, unbiased=False)
    xhat = (rows64 - mean64) / torch.sqrt(var64 + 1e-5)
    dy64 = dy.double().reshape(-1, cs)[:, :cv]
    dbeta64, dgamma64 = dy64.sum(0), (dy64 * xhat).sum(0)
    dz64 = gamma.double() / torch.sqrt(var64 + 1e-5) * (dy64 - dbeta64 / n - xhat * dgamma64 / n)
    run_mean64, run_var64 = 0.9 * 0.25 + 0.1 * mean64, 0.9 * 1.5 + 0.1 * var64 * n / (n - 1)
    # float32 F.batch_norm on the same data
    z32 = rows64.float().reshape(n, cv, 1, 1).requires_grad_(True)
    g32, b32 = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rm, rv = torch.full((cv,), 0.25, device="cuda"), torch.full((cv,), 1.5, device="cuda")
    F.batch_norm(z32, rm, rv, g32, b32, True, 0.1, 1e-5).backward(dy64.float().reshape(n, cv, 1, 1))
    rm1, rv1 = torch.zeros((cv,), device="cuda"), torch.zeros((cv,), device="cuda")       # momentum 1: the batch's own mean / unbiased variance
    F.batch_norm(z32.detach(), rm1, rv1, None, None, True, 1.0, 1e-5)
    # the kernels
    zk = bf(z)
    mean, var, rstd = ops.hyper_bn_stats(zk)
    dz, dgamma, dbeta, dzsum = ops.hyper_bn_bwd(dy.contiguous(), zk, mean, rstd, gamma, beta, tanh=False)
    bn = torch.nn.BatchNorm2d(cv).cuda()
    with torch.no_grad():
        bn.running_mean.fill_(0.25), bn.running_var.fill_(1.5)
    _update_running_stats(bn, mean, var, n)
    assert int(bn.num_batches_tracked) == 1
    for name, got, ref, t32 in (("mean", mean[:cv], mean64, rm1), ("var", var[:cv], var64, rv1.double() * (n - 1) / n),
                                ("dgamma", dgamma, dgamma64, g32.grad), ("dbeta", dbeta, dbeta64, b32.grad),
                                ("running_mean", bn.running_mean, run_mean64, rm), ("running_var", bn.running_var, run_var64, rv)):
        err, err32 = float((got.double() - ref).abs().max()), float((t32.double() - ref).abs().max())
        print(f"BatchNorm {cs}/{cv} {name}: error {err:.3e}, float32 F.batch_norm's {err32:.3e}")
        assert err <= 4.0 * err32 + _ulp(ref), name
    err32 = float((z32.grad.double().reshape(n, cv) - dz64).abs().max())
    got = dz.double().reshape(-1, cs)
    excess = float(((got[:, :cv] - dz64).abs() - 2.0 ** -8 * dz64.abs()).max())
    print(f"BatchNorm {cs}/{cv} dz: worst error beyond the bf16 store {excess:.3e}, float32 F.batch_norm's error {err32:.3e}")
    assert excess <= 4.0 * err32 + _ulp(dz64)
    assert float(dzsum.abs().max()) <= n * _ulp(dz64)                            # zero in exact arithmetic: n float32 roundings at most
    if cv < cs:
        assert torch.equal(got[:, cv:], torch.zeros_like(got[:, cv:]))           # the padded columns carry no gradient
        out = ops.hyper_bn_apply(zk, mean, rstd, gamma, beta, tanh=False)
        assert torch.equal(out[..., cv:].float(), torch.zeros_like(out[..., cv:].float()))
    dz2 = ops.hyper_bn_bwd(dy.contiguous(), zk, mean, rstd, gamma, beta, tanh=False)
    assert same_bits(dz, dz2[0]) and same_bits(dgamma.clone(), dz2[1].clone()) and same_bits(dbeta.clone(), dz2[2].clone())


def test_batchnorm_apply_and_tanh_backward_against_float64(ops):
    """y = tanh(bn(z)) as bf16: within the store's rounding + 2^-20 (the hardware exp2 / rcp behind tanh); dz through the tanh derivative
    1 - y^2 within its bf16 store + 1e-5 of the largest |dz|."""
    z, gamma, beta, dy = _bn_case(64, 64, 50)
    zk = bf(z)
    mean, var, rstd = ops.hyper_bn_stats(zk)
    y = ops.hyper_bn_apply(zk, mean, rstd, gamma, beta, tanh=True).double()
    z64 = z.clone().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    rows = z64.reshape(-1, 64)
    y64 = torch.tanh(g64 * (rows - rows.mean(0)) / torch.sqrt(rows.var(0, unbiased=False) + 1e-5) + b64)
    assert float(((y.reshape(-1, 64) - y64.detach()).abs() - 2.0 ** -8 * y64.detach().abs()).max()) <= 2.0 ** -20
    dyb = bf(dy.double())
    y64.backward(dyb.double().reshape(-1, 64))
    dz, dgamma, dbeta, _ = ops.hyper_bn_bwd(dyb, zk, mean, rstd, gamma, beta, tanh=True)
    ref = z64.grad.reshape(-1, 64)
    scale = float(ref.abs().max())
    excess = float(((dz.double().reshape(-1, 64) - ref).abs() - 2.0 ** -8 * ref.abs()).max())
    print(f"BatchNorm + tanh: dz worst error beyond the bf16 store {excess:.3e} (largest |dz| {scale:.3e}), dgamma error "
          f"{float((dgamma.double() - g64.grad).abs().max()):.3e}, dbeta error {float((dbeta.double() - b64.grad).abs().max()):.3e}")
    assert excess <= 1e-5 * scale
    assert float((dgamma.double() - g64.grad).abs().max()) <= 1e-5 * float(g64.grad.abs().max())
    assert float((dbeta.double() - b64.grad).abs().max()) <= 1e-5 * float(b64.grad.abs().max())


# ---- the atoms' adjoint ----------------------------------------------------------------------------------------------------------------------
def _atoms_case(seed, saturated):
    m = (B, 3, 5)
    datoms = ints(seed, m + (25, 6), -3, 3).float().contiguous()
    g = _gen(seed + 1)
    if saturated:
        pre = torch.where(torch.rand(m + (128,), generator=g) < 0.5, -64.0, 64.0)
    else:
        pre = torch.randn(m + (128,), generator=g) * 1.5
    bases = torch.randn((12, 25), generator=g).float().cuda()
    return datoms, pre.to(torch.bfloat16).cuda().contiguous(), bases


def test_atoms_backward_is_exactly_zero_where_tanh_saturates(ops):
    datoms, pre, bases = _atoms_case(60, True)                                   # tanh(+-64) = +-1 exactly: zero slope
    out = ops.hyper_atoms_bwd(datoms, pre, bases)
    assert torch.equal(out, torch.zeros_like(out))


def test_atoms_backward_against_float64(ops):
    """The forward atoms test's bar: 2^-20 per tanh (hardware exp2 / rcp) against sums of 25 float32 terms -> 1e-5 of the largest value."""
    datoms, pre, bases = _atoms_case(61, False)
    out = ops.hyper_atoms_bwd(datoms, pre, bases)
    c = torch.tanh(pre.double()[..., :72]).reshape(B, 3, 5, 6, 12)
    ref = (1 - c * c) * torch.einsum("bhwlm,kl->bhwmk", datoms.double(), bases.double())
    err = float((out.double()[..., :72].reshape(B, 3, 5, 6, 12) - ref).abs().max())
    print(f"atoms backward: max error {err:.3e}, largest value {float(ref.abs().max()):.3e}")
    assert err <= 1e-5 * float(ref.abs().max())
    assert torch.equal(out[..., 72:], torch.zeros_like(out[..., 72:]))           # the padding columns
    assert same_bits(out, ops.hyper_atoms_bwd(datoms, pre, bases))
