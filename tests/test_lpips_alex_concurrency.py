"""The LPIPS-AlexNet kernels (v2v_amd/csrc/v2v_alex.hpp) under CO-SCHEDULING with matrix-core work on another stream, built like
tests/test_metrics_concurrency.py: a ConvLSTM step / a rocBLAS bf16 GEMM runs on a second stream while the LPIPS of a sequence is taken,
and every output must be the stand-alone one bit for bit (no float atomics, slots added in a fixed order; the library is built without
packed float32 instructions)."""
import pytest
import torch

import lpips_alex_weights as LW
from test_convgru_concurrency import _disturbers

pytestmark = pytest.mark.gpu


def test_lpips_alex_does_not_depend_on_what_shares_the_cu(golden):
    from v2v_amd.lpips_alex import LPIPSAlex
    model = LPIPSAlex()
    model.load_state_dict(LW.golden_state(golden("g34_lpips_alex.npz")), strict=True)
    model = model.cuda()
    cases = [tuple(torch.from_numpy(v).cuda() for v in LW.case_inputs(name)) for name in ("b", "r180")]

    def run():
        outs = []
        for pred, target in cases:
            dist, taps = model.sequence(pred, target, divisor=1.0, taps=True)
            outs += [dist.view(torch.int32), taps.view(torch.int64)]
        return outs
    side = torch.cuda.Stream()
    victim = torch.cuda.Stream()
    solo = run()
    torch.cuda.synchronize()
    assert all(int(o.abs().max()) > 0 for o in solo)
    for name, disturb in _disturbers().items():
        for rep in range(6):
            with torch.cuda.stream(side):
                for _ in range(24):
                    disturb()
            with torch.cuda.stream(victim):
                outs = [run() for _ in range(4)]
            torch.cuda.synchronize()
            for o in outs:
                for k, (a, b) in enumerate(zip(o, solo)):
                    assert torch.equal(a, b), f"LPIPS output {k} differs from its stand-alone result while {name} runs on another stream ({int((a != b).sum())} elements)"
