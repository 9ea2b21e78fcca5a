"""Training surface without a GPU: the backward entry points of the C ABI validate their arguments, and trainable=True changes
neither the module tree nor the state_dict keys of the reference's E2VIDRecurrent (model/model.py:194-223)."""
import ctypes as C
import inspect

import pytest

KW = dict(num_bins=5, skip_type="sum", recurrent_block_type="convlstm", num_encoders=3, base_num_channels=32,
          num_residual_blocks=2, use_upsample_conv=True, final_activation="", norm=None)


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from v2v_amd import _lib
    return _lib


def test_backward_exports_reject_null_and_bad_shapes(L):
    lib = L.lib()
    d = C.c_void_p(4096)
    # ConvLSTM step backward: x/packed/bias/dh/dgates/dc_prev required; C % 64
    assert lib.v2v_convlstm_step_bwd_hip(None, None, None, d, d, d, None, 2, 16, 16, 64, d, d, None) == L.ERR_NULL
    assert lib.v2v_convlstm_step_bwd_hip(d, None, None, d, d, d, None, 2, 16, 16, 48, d, d, None) == L.ERR_SHAPE
    # data gradient: the transposed convolution must be a shape the forward kernel takes (8 -> 40 channels is not)
    assert lib.v2v_conv_dgrad_nhwc_hip(None, d, None, 2, 32, 32, 64, 128, 5, 2, d, d, None) == L.ERR_NULL
    assert lib.v2v_conv_dgrad_nhwc_hip(d, d, None, 2, 32, 32, 40, 8, 5, 1, d, d, None) == L.ERR_SHAPE
    assert lib.v2v_conv_dgrad_nhwc_hip(d, d, None, 2, 31, 32, 64, 128, 5, 2, d, d, None) == L.ERR_SHAPE      # odd input for stride 2
    assert lib.v2v_conv_dgrad_packed_elems(64, 128, 5) == lib.v2v_conv_packed_elems(128, 64, 5) > 0
    assert lib.v2v_conv_dgrad_pack_weights_hip(None, 64, 128, 5, d, d, None) == L.ERR_NULL
    assert lib.v2v_conv_dgrad_pack_weights_hip(d, 40, 8, 5, d, d, None) == L.ERR_SHAPE
    # weight gradient: Cout a multiple of 32, Cin_out <= C1 + C2
    assert lib.v2v_conv_wgrad_nhwc_hip(None, d, 64, None, 0, 64, 2, 32, 32, 128, 5, 2, d, d, d, None) == L.ERR_NULL
    assert lib.v2v_conv_wgrad_nhwc_hip(d, d, 64, None, 0, 64, 2, 32, 32, 48, 5, 2, d, d, d, None) == L.ERR_SHAPE
    assert lib.v2v_conv_wgrad_nhwc_hip(d, d, 8, None, 0, 9, 2, 32, 32, 32, 5, 1, d, d, d, None) == L.ERR_SHAPE
    assert lib.v2v_conv_wgrad_workspace_bytes(2, 16, 16, 64, 48, 5) < 0 < lib.v2v_conv_wgrad_workspace_bytes(2, 16, 16, 64, 128, 5)
    # the rest
    assert lib.v2v_upsample2x_bwd_nhwc_hip(None, 2, 16, 16, 64, d, None) == L.ERR_NULL
    assert lib.v2v_upsample2x_bwd_nhwc_hip(d, 2, 16, 16, 12, d, None) == L.ERR_SHAPE
    assert lib.v2v_conv1x1_bwd_nhwc_hip(None, d, None, d, 64, 32, d, d, d, d, None) == L.ERR_NULL
    assert lib.v2v_conv1x1_bwd_nhwc_hip(d, d, None, d, 64, 48, d, d, d, d, None) == L.ERR_SHAPE
    assert lib.v2v_relu_bwd_nhwc_hip(None, None, 64, 32, d, None) == L.ERR_NULL
    assert lib.v2v_relu_bwd_nhwc_hip(d, None, 64, 12, d, None) == L.ERR_SHAPE


def test_trainable_network_has_the_reference_state_dict_keys():
    from v2v_amd.unet import E2VIDRecurrent
    a = E2VIDRecurrent(unet_kwargs=dict(KW), trainable=True)
    b = E2VIDRecurrent(unet_kwargs=dict(KW))
    assert list(a.state_dict()) == list(b.state_dict())
    assert [tuple(v.shape) for v in a.state_dict().values()] == [tuple(v.shape) for v in b.state_dict().values()]
    assert all(k.startswith("unetrecurrent.") for k in a.state_dict())
    assert len(a.state_dict()) == 30 and sum(p.numel() for p in a.parameters()) == 10_710_401
    from v2v_amd.convlstm import ConvLayer, ConvLSTM, ResidualBlock
    layers = [m for m in a.modules() if isinstance(m, (ConvLayer, ConvLSTM, ResidualBlock))]
    assert len(layers) == 1 + 3 + 3 + 2 + 3 + 1 and all(m.trainable for m in layers)


def test_trainable_defaults_to_false():
    from v2v_amd.convlstm import ConvLayer, ConvLSTM, ResidualBlock
    from v2v_amd.unet import E2VIDRecurrent, RecurrentConvLayer, UNetRecurrent, UpsampleConvLayer
    for cls in (E2VIDRecurrent, UNetRecurrent, ConvLayer, UpsampleConvLayer, ResidualBlock, ConvLSTM, RecurrentConvLayer):
        assert inspect.signature(cls).parameters["trainable"].default is False, cls
    net = E2VIDRecurrent(dict(KW))
    assert not net.trainable and not any(getattr(m, "trainable", False) for m in net.modules())


def test_yaml_params_reach_the_switch():
    """instantiate_from_config (utils/util.py:14-17) passes `params` as keyword arguments."""
    import importlib
    cfg = {"target": "v2v_amd.unet.E2VIDRecurrent", "params": {"unet_kwargs": dict(KW), "trainable": True}}
    mod, cls = cfg["target"].rsplit(".", 1)
    net = getattr(importlib.import_module(mod), cls)(**cfg.get("params", dict()))
    assert net.trainable and net.unetrecurrent.trainable and net.unetrecurrent.decoders[0].trainable
