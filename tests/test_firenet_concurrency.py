"""One FireNet step (the one-launch 16-channel kernels of v2v_amd/csrc/v2v_narrow.hpp) under CO-SCHEDULING with matrix-core work on another
stream, built like tests/test_convgru_concurrency.py: a ConvLSTM step / a rocBLAS bf16 GEMM runs on a second stream while the step runs,
and the image and both states (bf16 and fp32) must be the stand-alone ones (the library is built without packed float32 instructions,
DESIGN 4.9)."""
import pytest
import torch

import firenet_stock as S
from test_convgru_concurrency import _disturbers

pytestmark = pytest.mark.gpu


def test_firenet_step_does_not_depend_on_what_shares_the_cu():
    from v2v_amd.unet import FireNet
    g = S.g28()
    net = FireNet().cuda().eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in S.g28_state(g).items()}, strict=True)
    ev = torch.from_numpy(S.sparse_voxels(2860, 2, 12, 5, 64, 64)).cuda()
    with torch.no_grad():
        net.reset_states()
        net(ev[0])
        start = net.states

        def run():
            net.states = list(start)                                           # a fresh list: the step assigns into the live one
            img = net(ev[1])["image"]
            return [img] + [t for s in net._states for t in (s._v2v_gru[0], s._v2v_gru[1])]
        side = torch.cuda.Stream()
        solo = run()
        torch.cuda.synchronize()
        assert all(float(o.float().abs().max()) > 0 for o in solo)
        for name, disturb in _disturbers().items():
            for rep in range(6):
                with torch.cuda.stream(side):
                    for _ in range(24):
                        disturb()
                outs = [run() for _ in range(4)]
                torch.cuda.synchronize()
                for o in outs:
                    for k, (a, b) in enumerate(zip(o, solo)):
                        assert torch.equal(a, b), f"FireNet output {k} differs from its stand-alone result while {name} runs on another stream ({int((a != b).sum())} elements)"
