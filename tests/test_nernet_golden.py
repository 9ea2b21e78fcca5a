"""CPU-side checks of NER-Net's learned voxelisation (v2v_amd/nernet.py, include/v2v_nernet.h) against golden G32
(tests/golden/g32_nernet_voxelization.npz, written by tests/golden/make_golden_nernet.py from the reference's own module): the drop-ins'
state dicts, the stock restatement the GPU tests lean on (tests/nernet_stock.py) bit for bit, what must raise without a GPU, and the C
entry points' argument validation.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from torch import nn

import nernet_stock as NS
import seeded_weights as SW
from capi_calls import _D, _d, _zero

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET_KW = {"RepCNN_kernel_size": 3, "RepCNN_padding": 1, "RepCNN_channel": 16, "RepCNN_num_layers": 4}
SD_CFGS = {"mlp30": ([1, 30, 30, 1], False, False), "mlp30_cnn": ([1, 30, 30, 1], True, False), "mlp50": ([1, 50, 50, 50, 1], False, False),
           "mlp50_cnn": ([1, 50, 50, 50, 1], True, False), "mlp30_combined_cnn": ([1, 30, 30, 1], True, True)}


@pytest.fixture(scope="module")
def g32(golden):
    return golden("g32_nernet_voxelization.npz")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from v2v_amd import _lib
    return _lib


@pytest.fixture
def one_thread():
    """G32 was written with one CPU thread: the GEMM's blocking, and with it the last bits, depends on the thread count"""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _case_names():
    z = np.load(os.path.join(ROOT, "tests", "golden", "g32_nernet_voxelization.npz"))
    return [str(c) for c in z["cases"]]


def test_golden_lists_the_recorded_configurations(g32):
    assert sorted(str(n) for n in g32["sd__names"]) == sorted(SD_CFGS)
    assert len(g32["cases"]) == 19 and g32["real_c5_f64__events"].shape == (4000, 5)


@pytest.mark.parametrize("name", sorted(SD_CFGS))
def test_state_dict_keys_and_shapes_are_the_references(g32, name):
    from v2v_amd import nernet
    mlp, cnn, comb = SD_CFGS[name]
    sd = nernet.Voxelization(NET_KW, cnn, voxel_dimension=(5, 12, 20), mlp_layers=mlp, combine_voxel=comb).state_dict()
    assert list(sd) == [str(k) for k in g32[f"sd__{name}__keys"]]
    assert [list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()] == g32[f"sd__{name}__shapes"].tolist()
    assert any(k.startswith("quantization_layer.value_layer.mlp.0.") for k in sd) and (not cnn or any(k.startswith("ConvLayer.cnn.") for k in sd))


@pytest.mark.parametrize("name", sorted(SD_CFGS))
def test_a_reference_shaped_state_dict_loads_strictly(g32, name):
    from v2v_amd import nernet
    mlp, cnn, comb = SD_CFGS[name]
    shapes = {str(k): tuple(int(v) for v in s if v >= 0) for k, s in zip(g32[f"sd__{name}__keys"], g32[f"sd__{name}__shapes"])}
    state = {k: (torch.from_numpy(v) if "num_batches" not in k else torch.tensor(3)) for k, v in SW.seeded_state(shapes, 5).items()}
    net = nernet.Voxelization(NET_KW, cnn, voxel_dimension=(5, 12, 20), mlp_layers=mlp, combine_voxel=comb)
    net.load_state_dict(state, strict=True)
    assert torch.equal(net.quantization_layer.value_layer.mlp[1].weight, state["quantization_layer.value_layer.mlp.1.weight"])
    # ValueLayer.forward stays plain torch: the same numbers as the stock MLP on the CPU
    x = torch.linspace(-2, 2, 37)
    stock = NS.StockValueLayer(mlp, nn.LeakyReLU(negative_slope=0.1))
    stock.load_state_dict(net.quantization_layer.value_layer.state_dict())
    with torch.no_grad():
        assert torch.equal(net.quantization_layer.value_layer(x), stock(x))


def _stock_layer(g32, name):
    Cb, H, W, B, norm, comb, seed = (int(v) for v in g32[f"{name}__cfg"])
    slope = float(g32[f"{name}__slope"][0])
    layer = NS.StockQuantization((Cb, H, W), [int(v) for v in g32[f"{name}__mlp"]], nn.ReLU() if slope == 0.0 else nn.LeakyReLU(negative_slope=slope),
                                 bool(norm), bool(comb))
    SW.load_seeded(layer.value_layer, seed)
    return layer, B


@pytest.mark.parametrize("name", _case_names())
def test_stock_restatement_reproduces_the_golden_bit_for_bit(g32, name, one_thread):
    layer, B = _stock_layer(g32, name)
    events = torch.from_numpy(g32[f"{name}__events"])
    before = events.clone()
    with torch.no_grad():
        out, tn = layer(events, return_t=True)
    assert torch.equal(events, before), "the restatement leaves its input untouched"
    assert out.dtype == torch.float32 and out.shape[0] == B
    assert np.array_equal(tn.numpy(), g32[f"{name}__tn"], equal_nan=True)
    assert np.array_equal(out.numpy(), g32[f"{name}__out"], equal_nan=True)
    # the recorded truth is the float64 evaluation of the same layer, and the recorded error norms are the reference's against it
    wts = [m.weight.detach() for m in layer.value_layer.mlp]
    bss = [m.bias.detach() for m in layer.value_layer.mlp]
    truth = NS.truth64(events, tn, wts, bss, layer.dim, float(g32[f"{name}__slope"][0]), layer.normalize, layer.combined)
    np.testing.assert_allclose(truth.numpy(), g32[f"{name}__truth"], rtol=1e-12, atol=1e-12)
    err = np.abs(g32[f"{name}__out"].astype(np.float64) - g32[f"{name}__truth"])
    np.testing.assert_allclose(g32[f"{name}__err"], [err.max(), np.sqrt((err ** 2).mean())], rtol=1e-9, atol=0)


@pytest.mark.parametrize("mlp", [[1, 1], [1, 30, 30, 30, 30, 30, 1], [1, 129, 1], [1, 0, 1], [2, 30, 1], [1, 30, 2]])
def test_unsupported_mlp_layers_raise_before_any_launch(mlp):
    from v2v_amd import nernet
    with pytest.raises((ValueError, AssertionError)):
        nernet.QuantizationLayer_trail((5, 12, 20), mlp)
    with pytest.raises((ValueError, AssertionError)):
        nernet.Voxelization(NET_KW, False, (5, 12, 20), mlp)


def test_other_activations_raise():
    from v2v_amd import nernet
    with pytest.raises(ValueError, match="LeakyReLU or nn.ReLU"):
        nernet.QuantizationLayer_trail((5, 12, 20), [1, 30, 1], nn.Tanh())
    assert nernet.QuantizationLayer_trail((5, 12, 20), [1, 30, 1], nn.ReLU()).slope == 0.0
    assert nernet.QuantizationLayer_trail((5, 12, 20), [1, 30, 1], nn.LeakyReLU(0.25)).slope == 0.25


def test_float64_rows_into_the_combined_layer_raise_a_type_error():
    from v2v_amd import nernet
    layer = nernet.QuantizationLayer_trail_combined((5, 12, 20), [1, 30, 30, 1])
    with torch.no_grad(), pytest.raises(TypeError, match="float32 rows only"):
        layer(torch.zeros((4, 5), dtype=torch.float64))
    w, b = layer._params()
    with torch.no_grad(), pytest.raises(TypeError, match="float32 rows only"):
        nernet.learned_voxel(torch.zeros((4, 5), dtype=torch.float64), w, b, (5, 12, 20), 0.1, combined=True, batch_size=1)


def test_grad_mode_call_raises():
    from v2v_amd import nernet
    net = nernet.Voxelization(NET_KW, False, (5, 12, 20), [1, 30, 30, 1])
    with pytest.raises(RuntimeError, match="inference-only"):
        net(torch.zeros((4, 5), dtype=torch.float64))


def test_compute_call_raises_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from v2v_amd import nernet
    net = nernet.Voxelization(NET_KW, False, (5, 12, 20), [1, 30, 30, 1])
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        net(torch.zeros((4, 5), dtype=torch.float64))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU fallback"):
        net.forward_sequence([torch.zeros((4, 5), dtype=torch.float64)])


def test_pack_mlp_layout():
    from v2v_amd import nernet
    layer = nernet.QuantizationLayer_trail((5, 12, 20), [1, 7, 20, 1])
    w, b = layer._params()
    p = nernet.pack_mlp(w, b)
    kp = 32
    assert p.numel() == 4 * kp + kp * kp + kp and p.dtype == torch.float32
    assert torch.equal(p[:7], w[0].detach()[:, 0]) and torch.equal(p[kp:kp + 7], b[0].detach()) and not p[7:kp].any()
    m = p[2 * kp:2 * kp + kp * kp].view(kp, kp)
    assert torch.equal(m[:20, :7], w[1].detach()) and not m[20:].any() and not m[:, 7:].any()
    assert torch.equal(p[2 * kp + kp * kp:2 * kp + kp * kp + 20], b[1].detach())
    assert torch.equal(p[-2 * kp:-2 * kp + 20], w[2].detach()[0]) and p[-kp] == b[2].detach()[0]


# ---- the C entry points (include/v2v_nernet.h) -------------------------------------------------------------------------------------------
def test_every_entry_point_has_a_stub_in_the_integration_guide(L):
    """the header against the binding table, the library and the refused zero call: tests/test_capi_contract.py"""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in L.HEADERS["v2v_nernet.h"]:
        assert name in doc, f"{name} has no stub in INTEGRATION.md"


def _stats_args(**kw):
    return [kw.get("events", _d()), kw.get("dt", 2), kw.get("n", 10), kw.get("seg", None), kw.get("T", 1), kw.get("B", 1), kw.get("ws", _d(1)), None]


def _fused_args(layers=(1, 30, 30, 1), **kw):
    host = (C.c_int * len(layers))(*layers)
    return [kw.get("events", _d()), kw.get("dt", 2), kw.get("n", 10), kw.get("seg", None), kw.get("T", 1), kw.get("B", 1), kw.get("bins", 5),
            kw.get("H", 12), kw.get("W", 20), kw.get("packed", _d(2)), kw.get("layers", host), len(layers), 0.1, kw.get("normalize", 0),
            kw.get("combined", 0), kw.get("ws", _d(1)), kw.get("out", _d(3)), kw.get("t_out", None), None]


def test_argument_validation_answers_without_a_gpu(L):
    lib = L.lib()
    st, fu = lib.v2v_learned_voxel_stats_hip, lib.v2v_learned_voxel_hip
    assert st(*_zero(L.SIGNATURES["v2v_learned_voxel_stats_hip"][1])) == L.ERR_NULL
    assert lib.v2v_last_error().decode() == "v2v_learned_voxel_stats_hip: events/workspace is NULL"
    assert fu(*_zero(L.SIGNATURES["v2v_learned_voxel_hip"][1])) == L.ERR_NULL
    assert lib.v2v_last_error().decode() == "v2v_learned_voxel_hip: events/workspace is NULL"
    assert st(*_stats_args(dt=0)) == L.ERR_DTYPE
    assert st(*_stats_args(n=-1)) == L.ERR_SHAPE
    assert st(*_stats_args(n=(1 << 31) // 5 + 1)) == L.ERR_SHAPE and b"below 2^31" in lib.v2v_last_error()
    assert st(*_stats_args(T=2)) == L.ERR_NULL and b"seg_offsets" in lib.v2v_last_error()
    assert st(*_stats_args(events=C.c_void_p(_D + 4))) == L.ERR_ALIGN
    assert st(*_stats_args(events=C.c_void_p(_D + 4), dt=1, ws=C.c_void_p(_D + 4))) == L.ERR_ALIGN
    assert fu(*_fused_args(packed=None)) == L.ERR_NULL
    assert fu(*_fused_args(layers=(1, 129, 1))) == L.ERR_SHAPE and b"1..128" in lib.v2v_last_error()
    assert fu(*_fused_args(layers=(1, 1))) == L.ERR_SHAPE
    assert fu(*_fused_args(layers=(2, 30, 1))) == L.ERR_SHAPE
    assert fu(*_fused_args(combined=1)) == L.ERR_DTYPE and b"float32 rows only" in lib.v2v_last_error()
    assert fu(*_fused_args(bins=0)) == L.ERR_SHAPE
    assert fu(*_fused_args(bins=1, normalize=1)) == L.ERR_SHAPE
    assert fu(*_fused_args(H=1 << 16, W=1 << 16)) == L.ERR_SHAPE and b"below 2^31" in lib.v2v_last_error()
    assert fu(*_fused_args(out=C.c_void_p(_D + 2))) == L.ERR_ALIGN
    assert fu(*_fused_args(t_out=C.c_void_p(_D + 2))) == L.ERR_ALIGN
    assert lib.v2v_learned_voxel_workspace_bytes(8, 3) == 8 * 3 * 24
    assert lib.v2v_learned_voxel_workspace_bytes(0, 3) == L.ERR_SHAPE
    layers = (C.c_int * 5)(1, 50, 50, 50, 1)
    assert lib.v2v_learned_voxel_packed_elems(layers, 5) == 4 * 64 + 2 * (64 * 64 + 64)
    assert lib.v2v_learned_voxel_packed_elems(None, 5) == L.ERR_NULL
