"""_lib.launch on the device: the entry point runs with the operand's device current and torch's current stream there as its last argument,
and its status becomes the exception _lib.check maps it to.  The library is replaced by a stub that records what it receives, so no kernel
runs in these -- but for one real launch on a side stream at the end."""
import pytest
import torch

pytestmark = pytest.mark.gpu

MESSAGE = b"the stub's message"


class StubLibrary:
    def __init__(self, status=0):
        self.status = status
        self.calls = []

    def v2v_fake_hip(self, *args):
        self.calls.append((args, torch.cuda.current_device()))
        return self.status

    def v2v_last_error(self):
        return MESSAGE


@pytest.fixture
def L():
    from v2v_amd import _lib
    return _lib


def _launch_on_stub(L, monkeypatch, status=0):
    stub = StubLibrary(status)
    monkeypatch.setattr(L, "_lib", stub)
    dev = torch.device("cuda", torch.cuda.device_count() - 1)
    return stub, dev


def test_launch_passes_the_current_stream_of_the_device_last(L, monkeypatch):
    stub, dev = _launch_on_stub(L, monkeypatch)
    assert L.launch("v2v_fake_hip", dev, 1, 2) is None
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        assert L.launch("v2v_fake_hip", dev, 1, 2) is None
    (on_default, d0), (on_side, d1) = stub.calls
    assert on_default[:2] == (1, 2) and len(on_default) == 3 and on_side[:2] == (1, 2) and len(on_side) == 3
    assert (on_default[2].value or 0) == torch.cuda.current_stream(dev).cuda_stream
    assert on_side[2].value == side.cuda_stream != torch.cuda.current_stream(dev).cuda_stream
    assert d0 == d1 == dev.index


def test_ok_returns_none(L, monkeypatch):
    stub, dev = _launch_on_stub(L, monkeypatch, L.OK)
    assert L.launch("v2v_fake_hip", dev) is None
    assert len(stub.calls) == 1 and len(stub.calls[0][0]) == 1


def test_err_bins_is_the_reference_assertion(L, monkeypatch):
    _, dev = _launch_on_stub(L, monkeypatch, L.ERR_BINS)
    with pytest.raises(AssertionError) as e:
        L.launch("v2v_fake_hip", dev, 1, 2)
    assert MESSAGE.decode() in str(e.value)


@pytest.mark.parametrize("code", ["ERR_SHAPE", "ERR_DTYPE", "ERR_MODE", "ERR_PARAM", "ERR_NULL", "ERR_ALIGN"])
def test_argument_errors_are_value_errors(L, monkeypatch, code):
    _, dev = _launch_on_stub(L, monkeypatch, getattr(L, code))
    with pytest.raises(ValueError) as e:
        L.launch("v2v_fake_hip", dev, 1, 2)
    assert MESSAGE.decode() in str(e.value)


def test_err_hip_is_a_v2v_error_with_its_code(L, monkeypatch):
    _, dev = _launch_on_stub(L, monkeypatch, L.ERR_HIP)
    with pytest.raises(L.V2VError) as e:
        L.launch("v2v_fake_hip", dev, 1, 2)
    assert e.value.code == L.ERR_HIP and MESSAGE.decode() in str(e.value)


def test_call_sites_still_refuse_the_dtypes_they_do_not_take():
    """DTYPE_CODES knows four dtypes; a call site takes its own few and refuses the rest before any launch, as it did with its private
    dictionary: KeyError(dtype) where a caller's dtype was looked up directly."""
    from v2v_amd import esim, v2e
    frames = esim.synth_clips(1, 6, 8, 8, dtype=torch.uint8)
    vp = v2e.make_params(24, "pn_related", 0.5, 0.1, 0.0, 0.1, 30, 0.1, 0, 5.0, 0.1, 0.1)
    for dtype in (torch.bfloat16, torch.uint8, torch.float16):
        with pytest.raises(KeyError):
            esim.esim_voxel_batch(frames, [0.2, 0.2, 0.0, 0.0, 0.0], num_bins=5, out_dtype=dtype)
        with pytest.raises(KeyError):
            v2e.v2e_voxel_batch(frames, vp, num_bins=5, out_dtype=dtype)
    for dtype in (torch.float64, torch.bfloat16):
        with pytest.raises(KeyError):
            esim.synth_clips(1, 2, 4, 8, dtype=dtype)
        with pytest.raises(KeyError):
            esim.algorithmic_bytes(dtype, 1, 6, 8, 8, "sum", 5)
    with pytest.raises(KeyError):
        esim.algorithmic_bytes(torch.float32, 1, 6, 8, 8, "sum", 5, out_dtype=torch.uint8)
    torch.cuda.synchronize()


def test_a_real_launch_on_a_side_stream():
    from v2v_amd import esim
    want = esim.synth_clips(1, 2, 4, 8)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = esim.synth_clips(1, 2, 4, 8)
    side.synchronize()
    torch.cuda.current_stream().synchronize()
    assert got.shape == (1, 2, 4, 8) and got.dtype == torch.float32
    assert torch.equal(got, got.round()) and float(got.min()) >= 0 and float(got.max()) <= 255
    assert torch.equal(got, want)
