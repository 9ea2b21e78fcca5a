"""What v2v_amd.convlstm.ConvLayer decides once, in its constructor -- which of its six layers it is -- and the one packed-weight cache every
layer shares (v2v_amd.nhwc_ops.packed_weights).  No GPU: the constructors and the cache run on the CPU."""
import pytest


def _build(what):
    from v2v_amd.convlstm import ConvLayer
    from v2v_amd.unet import UpsampleConvLayer
    return {"head": lambda: ConvLayer(5, 32, 5, padding=2),                        # the recurrent UNet's head
            "head16": lambda: ConvLayer(5, 16, 3, padding=1),                      # FireNet's head
            "stem": lambda: ConvLayer(5, 64, 3, stride=2, padding=1),              # EVFlowNet's first encoder
            "pred": lambda: ConvLayer(32, 1, 1, activation=None),                  # the prediction layer
            "conv": lambda: ConvLayer(32, 64, 5, stride=2, padding=2),             # an encoder convolution
            "upconv": lambda: UpsampleConvLayer(256, 128, 5, padding=2)}[what]()   # a decoder


# role -> (head, stem, head16, upsample): the flags as they were before `role` existed (head16 is a head)
FLAGS = {"head": (True, False, False, False), "head16": (True, False, True, False), "stem": (False, True, False, False),
         "pred": (False, False, False, False), "conv": (False, False, False, False), "upconv": (False, False, False, True)}


@pytest.mark.parametrize("role", list(FLAGS))
def test_constructor_arguments_decide_the_role(role):
    from v2v_amd.convlstm import ConvLayer
    layer = _build(role)
    assert layer.role == role
    assert (layer.head, layer.stem, layer.head16, layer.upsample) == FLAGS[role]
    assert layer.relu == (role != "pred") and layer.force_channels_last is False and layer.trainable is False and layer._packed == {}
    pack, fn, run = ConvLayer._ROLES[role]
    assert (pack is None) == (role == "pred") and hasattr(fn, "kernels") and callable(run)
    assert list(layer.state_dict()) == ["conv2d.weight", "conv2d.bias"]
    assert set(ConvLayer._ROLES) == set(FLAGS)


@pytest.mark.parametrize("n", [1, 3])
def test_packed_weights_repacks_when_any_member_changes_and_only_then(n):
    """A one-tensor key and a three-tensor key: no repack on a second call; exactly one after an in-place update of any single member;
    exactly one after replacing any single member by another tensor.  make gets the detached tensors."""
    import torch
    from v2v_amd.nhwc_ops import packed_weights
    members = [torch.full((4,), float(i), requires_grad=True) for i in range(n)]
    seen = []

    def make(*tensors):
        seen.append(tensors)
        return len(seen)

    def get():
        return packed_weights(cache, "slot", members[0] if n == 1 else tuple(members), make)
    cache = {}
    assert get() == 1 and get() == 1
    assert len(seen[0]) == n and all(not t.requires_grad and t.data_ptr() == m.data_ptr() for t, m in zip(seen[0], members))
    count = 1
    for i in range(n):
        with torch.no_grad():
            members[i].add_(1.0)                                                   # an optimizer step, copy_, load_state_dict
        count += 1
        assert get() == count and get() == count, f"in-place update of member {i}"
    kept = list(members)                                                           # the old tensors stay alive: no address is handed out again
    for i in range(n):
        members[i] = kept[i].detach().clone().requires_grad_(True)                 # load_state_dict(assign=True), a new Parameter
        count += 1
        assert get() == count and get() == count, f"member {i} replaced by another tensor"
    assert len(seen) == count and list(cache) == ["slot"]
    other = {}
    assert packed_weights(other, "slot", members[0] if n == 1 else tuple(members), make) == count + 1      # caches are per layer
