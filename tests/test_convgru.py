"""The ConvGRU step on the matrix cores (two launches: gates, candidate; v2v_amd/csrc/v2v_convgru.hpp) against the reference's module
semantics (model/submodules.py:260-278), restated with stock PyTorch ops:
    u = sigmoid(update_gate(cat(x, h)));  r = sigmoid(reset_gate(cat(x, h)));  o = tanh(out_gate(cat(x, h * r)));  h' = h (1 - u) + o u

Tolerances are tests/test_convlstm.py's own (the kernel multiplies in bf16 and accumulates in fp32):
  * against the fp64 evaluation on the SAME bf16-rounded operands: 2e-5 absolute (summation order + hardware exp/rcp)
  * against the plain fp32 module on unrounded operands: 2e-2 absolute (a CPU emulation of this scheme -- bf16 operands, hr rounded to
    bf16, fp32 state -- on these input recipes gives 0.85-1.2e-2, max over six shapes up to 2x64x64x64)
The hidden state is carried in fp32 beside its bf16 copy: test_slow_update_sequence_keeps_what_a_bf16_state_loses pins that."""
import numpy as np
import pytest

TOL_SAME_OPERANDS = 2e-5
TOL_FP32_MODULE = 2e-2


def _bf16_round(t):
    import torch
    return t.to(torch.bfloat16).to(torch.float32)


def _case(b, c, h, w, seed):
    """test_convlstm.py's recipe with three [C, 2C, 3, 3] weights (update, reset, out) and their biases."""
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((b, c, h, w), generator=g)
    hp = torch.tanh(torch.randn((b, c, h, w), generator=g))
    k = 1.0 / np.sqrt(2 * c * 9)
    ws = [(torch.rand((c, 2 * c, 3, 3), generator=g) * 2 - 1) * k * 3 for _ in range(3)]
    bs = [(torch.rand((c,), generator=g) * 2 - 1) * 0.5 for _ in range(3)]
    return x, hp, ws, bs


def _conv(x, w, b, dtype):
    import torch.nn.functional as F
    return F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), padding=1)


def _ref_gru(x, h, ws, bs, dtype):
    """The reference's forward (:272-276) in `dtype` on CPU; x, h [B,C,H,W]."""
    import torch
    xh = torch.cat([x, h], 1)
    u, r = torch.sigmoid(_conv(xh, ws[0], bs[0], dtype)), torch.sigmoid(_conv(xh, ws[1], bs[1], dtype))
    o = torch.tanh(_conv(torch.cat([x.to(dtype), h.to(dtype) * r], 1), ws[2], bs[2], dtype))
    return h.to(dtype) * (1 - u) + o * u


def _nchw(t):
    return t.permute(0, 3, 1, 2).cpu()


def _pack(CL, ws, bs, dev):
    import torch
    return CL.pack_gru_weights(*(w.to(dev) for w in ws)), torch.cat(bs[:2]).to(dev), bs[2].to(dev)


# the shape list of test_convlstm.py::test_step_matches_reference_semantics (partial last tiles included); its tile_rows column is replaced
# by explicit (gates, candidate) instance codes so that every shipped instance runs: gates 1 64x128, 2 128x128, 3 128x256, 4 256x256,
# 5 64x256 K-split; candidate 1 128x64, 2 128x128 K-split, 3 128x256, 4 256x256, 5 64x128 K-split; (0, 0) = picked by shape
@pytest.mark.gpu
@pytest.mark.parametrize("shape,tiles", [((2, 64, 16, 16), (0, 0)), ((2, 64, 16, 16), (2, 1)), ((2, 64, 16, 16), (1, 1)), ((1, 128, 8, 24), (0, 0)),
                                          ((3, 64, 12, 16), (1, 1)), ((1, 256, 8, 8), (0, 0)), ((2, 64, 64, 64), (0, 0)), ((2, 64, 16, 16), (1, 0)),
                                          ((1, 128, 16, 32), (4, 2)), ((4, 128, 32, 32), (3, 2)), ((4, 128, 32, 32), (0, 0)), ((8, 64, 64, 64), (0, 0)),
                                          ((1, 256, 24, 30), (0, 0)), ((1, 64, 6, 6), (0, 0)), ((1, 64, 6, 6), (1, 1)), ((1, 128, 6, 6), (3, 5)),
                                          ((3, 64, 10, 14), (2, 1)), ((5, 128, 12, 10), (0, 0)),
                                          ((1, 256, 24, 30), (4, 4)), ((1, 256, 8, 8), (5, 3)), ((1, 128, 6, 6), (5, 5)), ((5, 128, 12, 10), (2, 1))])
def test_step_matches_reference_semantics(shape, tiles):
    import torch
    from v2v_amd import convlstm as CL
    b, c, h, w = shape
    x, hp, ws, bs = _case(b, c, h, w, seed=sum(shape) + 10 * tiles[0] + tiles[1])
    dev = "cuda"
    packed, b_gates, b_out = _pack(CL, ws, bs, dev)
    xn = CL._to_nhwc_bf16(x.to(dev)).contiguous()
    h32 = hp.to(dev).permute(0, 2, 3, 1).contiguous()                          # the fp32 master, unrounded
    h_bf16, h_f32, u, hr, h_nchw = CL.convgru_step(xn, h32.to(torch.bfloat16), h32, packed, b_gates, b_out, nchw_dtype=torch.float32,
                                                   tile_gates=tiles[0], tile_cand=tiles[1])
    torch.cuda.synchronize()
    f64 = torch.float64
    xr, hr_in, wr = _bf16_round(x), _bf16_round(hp), [_bf16_round(v) for v in ws]
    xh = torch.cat([xr, hr_in], 1)
    want_u, want_r = torch.sigmoid(_conv(xh, wr[0], bs[0], f64)), torch.sigmoid(_conv(xh, wr[1], bs[1], f64))
    got_u, got_hr, got_h = _nchw(u).double(), _nchw(hr).double(), _nchw(h_f32).double()
    figures = {"u": float((got_u - want_u).abs().max()), "hr": float((got_hr - hp.double() * want_r).abs().max())}
    # the candidate on the package's OWN hr and u (a rounding flip in hr must not leak into this figure)
    want_h = hp.double() * (1 - got_u) + torch.tanh(_conv(torch.cat([xr.double(), got_hr], 1), wr[2], bs[2], f64)) * got_u
    figures["h"] = float((got_h - want_h).abs().max())
    figures["fp32_module"] = float((got_h.float() - _ref_gru(x, hp, ws, bs, torch.float32)).abs().max())
    print(shape, tiles, figures)
    assert figures["u"] < TOL_SAME_OPERANDS
    assert figures["hr"] <= 2.0 ** -8                                           # a bf16 rounding of a value in [-1, 1]
    assert figures["h"] < TOL_SAME_OPERANDS
    assert torch.equal(h_bf16, h_f32.to(torch.bfloat16))                        # the next step's operand: RNE of the fp32 state
    assert torch.equal(h_nchw, h_f32.permute(0, 3, 1, 2).contiguous())
    assert figures["fp32_module"] < TOL_FP32_MODULE


@pytest.mark.gpu
def test_zero_state_and_in_place_state():
    import torch
    from v2v_amd import convlstm as CL
    x, _, ws, bs = _case(2, 64, 8, 16, seed=5)
    dev = "cuda"
    packed, b_gates, b_out = _pack(CL, ws, bs, dev)
    xn = CL.nchw_to_nhwc_bf16(x.to(dev))
    zh, z32 = torch.zeros_like(xn), torch.zeros(xn.shape, dtype=torch.float32, device=dev)
    a = CL.convgru_step(xn, None, None, packed, b_gates, b_out)                 # prev_state=None (:267-269): K over x only in both launches
    bb = CL.convgru_step(xn, zh, z32, packed, b_gates, b_out)
    # same sums in another order: fp32 rounding apart (test_convlstm.py's margins) -- 2e-6 on the fp32 outputs, one bf16 ulp on the bf16 state
    assert float((a[1] - bb[1]).abs().max()) < 2e-6 and float((a[2] - bb[2]).abs().max()) < 2e-6
    assert float((a[0].float() - bb[0].float()).abs().max()) <= 2.0 ** -8
    assert int(a[3].view(torch.int16).abs().max()) == 0 and int(bb[3].view(torch.int16).abs().max()) == 0      # hr = 0
    assert bool(a[1].isfinite().all()) and float(a[1].abs().max()) > 0.1
    buf = a[1].clone()
    out_of_place = CL.convgru_step(xn, a[0], a[1], packed, b_gates, b_out)
    in_place = CL.convgru_step(xn, a[0], buf, packed, b_gates, b_out, h_f32_out=buf)
    assert in_place[1].data_ptr() == buf.data_ptr() and torch.equal(in_place[1], out_of_place[1]) and torch.equal(in_place[0], out_of_place[0])


def test_shape_errors_are_reported_without_a_gpu():
    """Argument checks of the C ABI run before any HIP call."""
    import ctypes as C
    from v2v_amd import _lib
    L = _lib.lib()
    ng, nc = C.c_uint64(0), C.c_uint64(0)
    assert L.v2v_convgru_packed_bytes(64, C.byref(ng), C.byref(nc)) == 0 and (ng.value, nc.value) == (2 * 64 * 2 * 64 * 9 * 2, 64 * 2 * 64 * 9 * 2)
    assert L.v2v_convgru_packed_bytes(48, C.byref(ng), C.byref(nc)) == _lib.ERR_SHAPE
    assert L.v2v_convgru_packed_bytes(64, None, C.byref(nc)) == _lib.ERR_NULL
    bufs = [(C.c_char * 4096)() for _ in range(6)]
    p, q, u, hr, hs, h32 = (C.cast(b, C.c_void_p) for b in bufs)

    def step(x=p, h=None, hf=None, B=1, H=8, W=8, Cc=64, u_ws=u, hr_ws=hr, h_state=hs, h_f32=h32, nchw=None, dt=_lib.F32, tg=0, tc=0):
        return L.v2v_convgru_step_hip(x, h, hf, q, q, q, q, B, H, W, Cc, u_ws, hr_ws, h_state, h_f32, nchw, dt, tg, tc, None)
    assert step(Cc=32) == _lib.ERR_SHAPE                                        # C % 64
    assert step(H=5, W=5) == _lib.ERR_SHAPE                                     # H*W % 4
    assert step(tg=6) == _lib.ERR_PARAM and step(tc=-1) == _lib.ERR_PARAM
    assert step(tg=3) == _lib.ERR_PARAM and step(tc=2) == _lib.ERR_PARAM        # 256-column gates / 128-column candidate tiles need C % 128
    assert step(Cc=128, tg=3, tc=3) == _lib.ERR_PARAM                           # 256-column candidate tiles need C % 256
    assert step(h=p, hf=None) == _lib.ERR_NULL                                  # the bf16 state without its fp32 master
    assert step(h_state=p) == _lib.ERR_PARAM and step(hr_ws=p) == _lib.ERR_PARAM and step(hr_ws=hs) == _lib.ERR_PARAM   # aliases
    assert step(u_ws=h32) == _lib.ERR_PARAM
    assert step(x=None) == _lib.ERR_NULL and b"x/packed" in L.v2v_last_error()
    assert step(u_ws=None) == _lib.ERR_NULL and step(hr_ws=None) == _lib.ERR_NULL
    assert step(nchw=p, dt=_lib.U8) == _lib.ERR_DTYPE
    assert L.v2v_convgru_pack_weights_hip(p, p, p, 48, q, q, None) == _lib.ERR_SHAPE
    assert L.v2v_convgru_pack_weights_hip(p, None, p, 64, q, q, None) == _lib.ERR_NULL


@pytest.mark.gpu
def test_packing_is_exact():
    """The two packed streams against their documented layout (v2v_convgru.hpp), restated with tensor views."""
    import torch
    from v2v_amd import convlstm as CL
    g = torch.Generator().manual_seed(3)
    for c in (64, 128, 256):
        w_u, w_r, w_o = (torch.randn((c, 2 * c, 3, 3), generator=g).cuda() for _ in range(3))
        pg, pc = CL.pack_gru_weights(w_u, w_r, w_o)
        pgc, pcc = (256 if c % 128 == 0 else 128), (256 if c % 256 == 0 else 128 if c % 128 == 0 else 64)
        # gates: [t][tap][cc][q][gate][c32][k] <- weight_gate[t * P/2 + q * 32 + c32, cc * 64 + k, ky, kx]
        both = torch.stack([w_u, w_r])                                          # [gate, C, 2C, 3, 3]
        v = both.view(2, c // (pgc // 2), pgc // 64, 32, 2 * c // 64, 64, 3, 3).permute(1, 6, 7, 4, 2, 0, 3, 5).contiguous().to(torch.bfloat16).reshape(-1)
        assert torch.equal(pg, v)
        # candidate: [t][tap][cc][n][k] <- out_gate.weight[t * P + n, cc * 64 + k, ky, kx]
        v = w_o.view(c // pcc, pcc, 2 * c // 64, 64, 3, 3).permute(0, 4, 5, 2, 1, 3).contiguous().to(torch.bfloat16).reshape(-1)
        assert torch.equal(pc, v)


@pytest.mark.gpu
def test_slow_update_sequence_keeps_what_a_bf16_state_loses():
    """C = 64, 2x16x16, update-gate bias -8 (u ~ 3e-4: every step moves h by less than half a bf16 ulp of it), |h0| in [0.5, 0.95], 64 steps of
    N(0,1) inputs, against the fp32 module.  Bar: max |h64 - h64_fp32| < 1e-2.  A CPU emulation of this design (fp32 state beside its bf16
    copy) gives 2.3e-3, the same emulation with a bf16-only state 4.1e-2: the bar sits about 4x from each."""
    import torch
    from v2v_amd import convlstm as CL
    x, hp, ws, bs = _case(2, 64, 16, 16, seed=11)
    bs[0] = torch.full((64,), -8.0)
    g = torch.Generator().manual_seed(3)
    h0 = _bf16_round(torch.sign(torch.randn(hp.shape, generator=g)) * (0.5 + 0.45 * torch.rand(hp.shape, generator=g)))
    dev = "cuda"
    packed, b_gates, b_out = _pack(CL, ws, bs, dev)
    h32 = h0.to(dev).permute(0, 2, 3, 1).contiguous()
    hb = h32.to(torch.bfloat16)
    ref = h0.clone()
    for _ in range(64):
        xt = torch.randn(x.shape, generator=g)
        ref = _ref_gru(xt, ref, ws, bs, torch.float32)
        hb, h32 = CL.convgru_step(CL.nchw_to_nhwc_bf16(xt.to(dev)), hb, h32, packed, b_gates, b_out)[:2]
    err = float((_nchw(h32) - ref).abs().max())
    moved = float((ref - h0).abs().mean())
    print(f"slow update: max |h64 - h64_fp32| = {err:.3e}, mean |h64_fp32 - h0| = {moved:.3e}")
    assert moved > 1e-3                                                         # the sequence does move the state
    assert err < 1e-2


@pytest.mark.gpu
def test_module_is_a_drop_in_over_a_sequence():
    """Same constructor / parameter names / forward contract as the reference's ConvGRU; the bare cell of golden G27 (4 steps, the
    reference's own float32 states) within TOL_FP32_MODULE; a cloned float32 prev_state gives the bits of the carried master."""
    import torch
    from convgru_stock import g27
    from seeded_weights import seeded_input, seeded_state
    from v2v_amd import convlstm as CL
    g = g27()
    shapes = {str(k): tuple(int(v) for v in str(s).split(",")) for k, s in zip(g["cell__keys"], g["cell__shapes"])}
    fused = CL.ConvGRU(64, 64, 3).cuda().eval()
    assert list(fused.state_dict()) == list(shapes) and {k: tuple(v.shape) for k, v in fused.state_dict().items()} == shapes
    vals = seeded_state(shapes, int(g["cell__seed"]), float(g["cell__gain"]))
    fused.load_state_dict({k: torch.from_numpy(v) for k, v in vals.items()}, strict=True)
    xs = torch.relu(torch.from_numpy(seeded_input(int(g["cell__x_seed"]), 4, 2, 64, 8, 16))).cuda()
    want = torch.from_numpy(g["cell__states"])
    with torch.no_grad():
        s = s_clone = None
        for t in range(4):
            s = fused(xs[t], s)
            assert s.shape == want[t].shape and s.dtype == torch.float32 and s.is_contiguous()
            e = float((s.cpu() - want[t]).abs().max())
            print(f"bare ConvGRU step {t}: max error vs the reference's float32 state {e:.3e}")
            assert e < TOL_FP32_MODULE
            s2 = fused(xs[t], s_clone)                                           # prev_state rebuilt from a float32 clone: same bits
            assert torch.equal(s2, s)
            s_clone = s.clone()
        sb = fused(xs[1].to(torch.bfloat16), s)                                  # under autocast the layers in front hand over bfloat16
        assert sb.dtype == torch.bfloat16 and torch.equal(sb, fused(xs[1].to(torch.bfloat16).float(), s).to(torch.bfloat16))
    with pytest.raises(RuntimeError):
        fused(xs[0], None)                                                       # grad mode: loud, no silent graph break
    with pytest.raises(ValueError), torch.no_grad():
        CL.ConvGRU(32, 32, 3).cuda().eval()(xs[0][:, :32].contiguous(), None)     # hidden_size % 64 != 0: refused, no fallback
    with pytest.raises(ValueError):
        CL.ConvGRU(64, 64, 5)
    with pytest.raises(ValueError, match="backward"):
        CL.ConvGRU(64, 64, 3, trainable=True)


@pytest.mark.gpu
def test_wide_cache_serves_no_stale_weights():
    """ConvGRU(64, 64, 3): its packed streams AND its concatenated float32 biases sit in one cache entry keyed on all six parameters.
    1 x 64 x 4 x 4 channels-last bfloat16 input, a non-zero previous state (tests/stale_weights.py)."""
    import torch
    from seeded_weights import seeded_input
    from stale_weights import check_no_stale_weights
    from v2v_amd import convlstm as CL
    x = torch.from_numpy(seeded_input(2701, 1, 64, 4, 4)).cuda().to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    state = torch.tanh(torch.from_numpy(seeded_input(2702, 1, 64, 4, 4))).cuda()

    def make():
        torch.manual_seed(27)
        return CL.ConvGRU(64, 64, 3).cuda().eval()
    check_no_stale_weights(make, x, state)
