"""The stale-weight check of the layers whose packed-weight cache is keyed on SEVERAL tensors (tests/test_firenet.py, tests/test_convgru.py):
a layer that has run once must serve none of its cached packed weights after ANY of its parameters changed."""


def check_no_stale_weights(make, *inputs):
    """make() -> a fresh layer on the GPU in eval mode; inputs = what the layer is called on.  For every parameter in turn: call the layer,
    update that parameter in place (add_(0.25)), call again -- the result must equal, bit for bit, that of a freshly built layer that loaded
    the updated state_dict.  Then the same with the parameter's tensor REPLACED by a new one (load_state_dict(assign=True))."""
    import torch

    def fresh(layer):
        twin = make()
        twin.load_state_dict(layer.state_dict(), strict=True)
        return twin(*inputs)

    layer = make()
    names = [k for k, _ in layer.named_parameters()]
    assert names
    with torch.no_grad():
        for name in names:
            before = layer(*inputs)
            dict(layer.named_parameters())[name].add_(0.25)
            after = layer(*inputs)
            assert torch.equal(after, fresh(layer)), f"in-place update of {name}: stale packed weights"
            assert not torch.equal(after, before), f"{name} does not reach the output: the check would prove nothing"
        for name in names:
            before = layer(*inputs)
            state = dict(layer.state_dict())                               # the live tensors; one of them replaced by another tensor
            state[name] = state[name] + 0.25
            layer.load_state_dict(state, strict=True, assign=True)
            assert dict(layer.named_parameters())[name].data_ptr() == state[name].data_ptr()
            after = layer(*inputs)
            assert torch.equal(after, fresh(layer)), f"replaced tensor of {name}: stale packed weights"
            assert not torch.equal(after, before), name
