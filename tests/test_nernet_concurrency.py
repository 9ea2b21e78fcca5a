"""The learned-voxelisation kernels (v2v_amd/csrc/v2v_nernet.hpp) under CO-SCHEDULING with matrix-core work on another stream, built like
tests/test_loss_concurrency.py: a ConvLSTM step / a rocBLAS bf16 GEMM runs on a second stream while the integer-exact case of
tests/nernet_inputs.py is voxelised; the grid must be the stand-alone one bit for bit (every sum of that case is exact in any order, and
the library is built without packed float32 instructions)."""
import pytest
import torch

import nernet_inputs as NI
from test_convgru_concurrency import _disturbers

pytestmark = pytest.mark.gpu


def test_learned_voxel_does_not_depend_on_what_shares_the_cu():
    from v2v_amd import nernet
    Cb, B, H, W = 5, 3, 12, 20
    ws, bs = NI.exact_mlp([1, 50, 50, 50, 1], 3)
    ws, bs = [v.cuda() for v in ws], [v.cuda() for v in bs]
    packed = nernet.pack_mlp(ws, bs)
    rows = NI.with_specials(NI.exact_rows(21, 4097, Cb, B, H, W), Cb, B, H, W).cuda()

    def run():
        with torch.no_grad():
            return nernet.learned_voxel(rows, ws, bs, (Cb, H, W), NI.SLOPE, batch_size=B, packed=packed)
    side = torch.cuda.Stream()
    victim = torch.cuda.Stream()
    solo = run()
    torch.cuda.synchronize()
    assert float(solo.abs().max()) > 0
    for name, disturb in _disturbers().items():
        for rep in range(6):
            with torch.cuda.stream(side):
                for _ in range(24):
                    disturb()
            with torch.cuda.stream(victim):
                outs = [run() for _ in range(4)]
            torch.cuda.synchronize()
            for o in outs:
                assert torch.equal(o, solo), f"the grid differs from its stand-alone result while {name} runs on another stream ({int((o != solo).sum())} cells)"
