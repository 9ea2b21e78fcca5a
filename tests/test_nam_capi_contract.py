"""CPU-side checks of the SECOND binding table (v2v_amd/_lib.py:HEADERS_MORE), in the shape of test_capi_contract.py: the rows against
include/v2v_nam.h's prototypes, what every `_hip` entry point answers to a NULL / zero call through the library's one error slot, and the
shape errors of the global context block and the valid-extent helper.  No GPU: every call here fails argument validation before any HIP
call.  The first table (ABI 6: five headers, 124 rows) stays what test_capi_contract.py pins; this one is additive."""
import ctypes as C
import os
import re

import pytest

import test_capi_contract as base
from capi_calls import _D, _d, _zero

L = base.L                                             # the module-scoped fixture: build() + v2v_amd._lib


NULL_CALLS = {
    "v2v_nam_pack_weights_hip": (-1, "v2v_nam_pack_weights_hip: a weight or the packed pointer is NULL"),
    "v2v_nam_step_hip": (-1, "v2v_nam_step_hip: x/m_t/packed is NULL"),
    "v2v_gcb_nhwc_hip": (-1, "v2v_gcb_nhwc_hip: x/out/ctx_add is NULL"),
    "v2v_conv_head16in_pack_weights_hip": (-1, "v2v_conv_head16in_pack_weights_hip: weight/packed is NULL"),
    "v2v_to_nhwc16_bf16_hip": (-1, "v2v_to_nhwc16_bf16_hip: src/dst is NULL"),
    "v2v_conv_head16in_nhwc_hip": (-1, "v2v_conv_head16in_nhwc_hip: x16/packed/bias/out is NULL"),
    "v2v_valid_extent_nhwc_hip": (-1, "v2v_valid_extent_nhwc_hip: x is NULL"),
}


def test_second_table_matches_the_header_in_order(L):
    assert list(L.HEADERS_MORE) == ["v2v_nam.h"]
    protos, table = base._header_prototypes("v2v_nam.h"), L.HEADERS_MORE["v2v_nam.h"]
    assert list(protos) == list(table), "the header's table lists the header's entry points, in the header's order"
    for name, (res, args) in table.items():
        want_res, want_args = protos[name]
        assert base._ctypes_class(res) == want_res, name
        got = [base._ctypes_class(t) for t in args]
        assert got == want_args, (name, len(got), len(want_args), [i for i, (g, w) in enumerate(zip(got, want_args)) if g != w])
    assert '#include "v2v_hip.h"' in re.sub(r"/\*.*?\*/", "", open(os.path.join(base.ROOT, "include", "v2v_nam.h")).read(), flags=re.S)


def test_second_table_is_additive(L):
    assert not set(L.SIGNATURES_MORE) & set(L.SIGNATURES), "no name appears in both tables"
    assert L.SIGNATURES_MORE == {n: s for t in L.HEADERS_MORE.values() for n, s in t.items()}
    assert not set(L.SIGNATURES_MORE) & set(L.EXPORTS) and "v2v_nam.h" not in L.HEADERS
    lib = L.lib()
    for name, (res, args) in L.SIGNATURES_MORE.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args), name
    assert lib.v2v_version() == L.ABI_VERSION == 6
    assert sorted(NULL_CALLS) == sorted(n for n in L.SIGNATURES_MORE if n.endswith("_hip"))


@pytest.mark.parametrize("name", sorted(NULL_CALLS))
def test_null_call_status_and_message(L, name):
    lib = L.lib()
    status, message = NULL_CALLS[name]
    assert getattr(lib, name)(*_zero(L.SIGNATURES_MORE[name][1])) == status
    assert lib.v2v_last_error().decode() == message and message.startswith(name + ":")
    assert lib.v2v_hyper_train_last_error() == lib.v2v_last_error()


def _gcb(x=None, B=1, H=8, W=8, Cn=32, Hv=8, Wv=8, ws=_d(12), ws_bytes=1 << 20, ctx=_d(13), out=_d(14), eps=1e-5, w=None):
    x = _d() if x is None else x
    weights = [_d(k + 1) for k in range(11)] if w is None else w
    return [x] + weights + [eps, B, H, W, Cn, Hv, Wv, ws, ws_bytes, ctx, out, None]


_ODD = C.c_void_p(_D + 8)                              # 8-byte aligned only


def _nam(x=None, h=_d(2), c=_d(3), B=1, H=6, W=6, Cn=64, alpha=_d(5), o_pre=_d(6), m_state=_d(7), tile=0, Hv=None, Wv=None, h_state=_d(10)):
    x = _d() if x is None else x
    return [x, _d(1), h, c, _d(4), B, H, W, Cn, alpha, o_pre, m_state, None, _d(8), _d(9), h_state, _d(11), None, 0, tile, H if Hv is None else Hv, W if Wv is None else Wv, None]


VALIDATION_CASES = {
    "nam C = 96": ("v2v_nam_step_hip", lambda: _nam(Cn=96), -2, "v2v_nam_step_hip: C must be 64, 128 or 256 (got 96)"),
    "nam pack C = 96": ("v2v_nam_pack_weights_hip", lambda: [_d(k) for k in range(6)] + [96, _d(6), None], -2, "v2v_nam_pack_weights_hip: C must be 64, 128 or 256 (got 96)"),
    "nam missing workspace": ("v2v_nam_step_hip", lambda: _nam(o_pre=None), -1, "v2v_nam_step_hip: a workspace (alpha_ws/o_pre_ws) is NULL"),
    "nam half a state": ("v2v_nam_step_hip", lambda: _nam(c=None), -1, "v2v_nam_step_hip: h_prev and c_prev come together (both NULL: the zero state)"),
    "nam pixels": ("v2v_nam_step_hip", lambda: _nam(H=5, W=7), -2, "v2v_nam_step_hip: need B,H,W >= 1, (H*W) % 4 == 0 and B*H*W*C < 2^31 (got 1x5x7x64)"),
    "nam extent larger than the canvas": ("v2v_nam_step_hip", lambda: _nam(Hv=7), -2,
                                          "v2v_nam_step_hip: the valid extent 7 x 6 must lie inside the canvas 6 x 6 and hold a pixel"),
    "nam h_state align": ("v2v_nam_step_hip", lambda: _nam(h_state=_ODD), -6,
                          "v2v_nam_step_hip: x/m_t/h_prev/packed/m_state/c_state_bf16/h_state/h_nchw need 16-byte, the float32 buffers 4-byte alignment"),
    "nam tile": ("v2v_nam_step_hip", lambda: _nam(tile=3), -8, "v2v_nam_step_hip: tile must be 0 (by shape), 1 or 2 (got 3)"),
    "nam in place": ("v2v_nam_step_hip", lambda: _nam(m_state=_d(1)), -8,
                     "v2v_nam_step_hip: m_state / c_state_bf16 / h_state must not alias an operand a later launch or a neighbouring tile reads, "
                     "the workspaces not each other or a state"),
    "nam align": ("v2v_nam_step_hip", lambda: _nam(x=_ODD), -6,
                  "v2v_nam_step_hip: x/m_t/h_prev/packed/m_state/c_state_bf16/h_state/h_nchw need 16-byte, the float32 buffers 4-byte alignment"),
    "gcb C = 96": ("v2v_gcb_nhwc_hip", lambda: _gcb(Cn=96), -2, "v2v_gcb_nhwc_hip: C must be 32, 64 or 128 (got 96)"),
    "gcb extent larger than the canvas": ("v2v_gcb_nhwc_hip", lambda: _gcb(H=24, W=40, Hv=25, Wv=40), -2,
                                          "v2v_gcb_nhwc_hip: the valid extent 25 x 40 must lie inside the canvas 24 x 40 and hold a pixel"),
    "gcb empty extent": ("v2v_gcb_nhwc_hip", lambda: _gcb(Hv=0), -2, "v2v_gcb_nhwc_hip: the valid extent 0 x 8 must lie inside the canvas 8 x 8 and hold a pixel"),
    "gcb missing workspace": ("v2v_gcb_nhwc_hip", lambda: _gcb(ws=None), -1, "v2v_gcb_nhwc_hip: workspace is NULL (v2v_gcb_workspace_bytes gives its size)"),
    "gcb short workspace": ("v2v_gcb_nhwc_hip", lambda: _gcb(ws_bytes=271), -2, "v2v_gcb_nhwc_hip: the workspace holds 271 bytes, the call needs 272"),
    "gcb missing weight": ("v2v_gcb_nhwc_hip", lambda: _gcb(w=[_d(k + 1) for k in range(10)] + [None]), -1, "v2v_gcb_nhwc_hip: a weight pointer is NULL"),
    "gcb batch": ("v2v_gcb_nhwc_hip", lambda: _gcb(B=0), -2, "v2v_gcb_nhwc_hip: need 1 <= B <= 65535 and H, W >= 1 (got 0 x 8 x 8)"),
    "gcb in place": ("v2v_gcb_nhwc_hip", lambda: _gcb(out=_d()), -8, "v2v_gcb_nhwc_hip: out must not alias x (x is read again after the pooling)"),
    "gcb align": ("v2v_gcb_nhwc_hip", lambda: _gcb(x=_ODD), -6, "v2v_gcb_nhwc_hip: x/out need 16-byte, the float32 buffers 4-byte alignment"),
    "head 3 channels": ("v2v_conv_head16in_pack_weights_hip", lambda: [_d(), 3, _d(1), None], -2,
                        "v2v_conv_head16in_pack_weights_hip: this head takes 9 to 16 input channels, v2v_conv_head_nhwc_hip takes up to 8 (got 3)"),
    "head layout 3 channels": ("v2v_to_nhwc16_bf16_hip", lambda: [_d(), 64, 64, 8, 1, 1, 3, 8, 8, _d(1), None], -2,
                               "v2v_to_nhwc16_bf16_hip: this layout takes 9 to 16 channels, v2v_to_nhwc8_bf16_hip takes up to 8 (got 3)"),
    "head size": ("v2v_conv_head16in_nhwc_hip", lambda: [_d(), _d(1), _d(2), 1, 1, 0, 8, _d(3), None], -2,
                  "v2v_conv_head16in_nhwc_hip: need B,H,W >= 1 and B*H*W*32 < 2^31 (got 1 x 0 x 8)"),
    "head align": ("v2v_conv_head16in_nhwc_hip", lambda: [_ODD, _d(1), _d(2), 1, 1, 8, 8, _d(3), None], -6, "v2v_conv_head16in_nhwc_hip: x16/packed need 16-byte alignment"),
    "extent larger than the canvas": ("v2v_valid_extent_nhwc_hip", lambda: [_d(), 3, 1, 6, 8, 64, 6, 9, 0, None], -2,
                                      "v2v_valid_extent_nhwc_hip: the valid extent 6 x 9 must lie inside the canvas 6 x 8 and hold a pixel"),
    "extent channels": ("v2v_valid_extent_nhwc_hip", lambda: [_d(), 3, 1, 6, 8, 12, 5, 7, 0, None], -2,
                        "v2v_valid_extent_nhwc_hip: a pixel must be whole 16-byte pieces (C % 8 == 0) and the tensor below 2^31 elements (got C 12)"),
    "extent dtype": ("v2v_valid_extent_nhwc_hip", lambda: [_d(), 0, 1, 6, 8, 64, 5, 7, 0, None], -4, "v2v_valid_extent_nhwc_hip: dtype must be V2V_F32 or V2V_BF16"),
    "extent align": ("v2v_valid_extent_nhwc_hip", lambda: [_ODD, 1, 1, 6, 8, 64, 5, 7, 1, None], -6, "v2v_valid_extent_nhwc_hip: x needs 16-byte alignment"),
}


@pytest.mark.parametrize("case", sorted(VALIDATION_CASES))
def test_validation_status_and_message(L, case):
    name, args, status, message = VALIDATION_CASES[case]
    lib = L.lib()
    rc = getattr(lib, name)(*args())
    assert rc not in (L.OK, L.ERR_HIP), "the case must fail validation before any HIP call"
    assert rc == status
    assert lib.v2v_last_error().decode() == message


def test_workspace_size_and_its_refusals(L):
    lib = L.lib()
    assert lib.v2v_gcb_workspace_bytes(1, 8, 8, 32) == 2 * 34 * 4                     # two 32-pixel tiles of (m, S, V[32])
    assert lib.v2v_gcb_workspace_bytes(2, 23, 30, 128) == 2 * 22 * 130 * 4            # 690 pixels: 21 whole tiles and a partial one
    assert lib.v2v_gcb_workspace_bytes(1, 8, 8, 96) == L.ERR_SHAPE
    assert lib.v2v_last_error().decode() == "v2v_gcb_workspace_bytes: C must be 32, 64 or 128 (got 96)"
    assert lib.v2v_gcb_workspace_bytes(1, 0, 8, 32) == L.ERR_SHAPE
    assert [lib.v2v_nam_packed_elems(c) for c in (64, 128, 256)] == [180 * c * c for c in (64, 128, 256)]     # M and C: 4C x 2C x 9 each, H: 2C x 2C x 9
    assert lib.v2v_conv_head16in_packed_elems() == 25 * 32 * 16
    assert lib.v2v_nam_packed_elems(96) == L.ERR_SHAPE and lib.v2v_last_error().decode() == "v2v_nam_packed_elems: C must be 64, 128 or 256 (got 96)"


def test_full_extent_needs_no_launch(L):
    """canvas = valid: V2V_OK without touching the pointer or the GPU"""
    assert L.lib().v2v_valid_extent_nhwc_hip(_d(), 3, 1, 6, 8, 64, 6, 8, 1, None) == L.OK
