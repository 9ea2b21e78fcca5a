"""CPU test: the four float32 4-pixel device-noise ESIM instances (symmetric-only and by-polarity, bilinear and SUM bins) run at 4 waves
per SIMD, i.e. within 128 vector registers, and without scratch memory (a prologue that requests the frame ring in front of the barrier
costs three of them 32..48 bytes of scratch, docs/experiments/README.md).  Read from the code objects of the built library through tools/kernel_resources.py, like
tests/test_kernel_resources.py; the kernels are named by their template arguments only:
esim_voxel_kernel<input, pixels per work-item, bin mode, RNG, noise, float64 output, external noise, symmetric only, frame index>."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "v2v_amd", "libv2v_hip.so")

# float32 input (1), 4 pixels, {SUM (0), bilinear (1)}, Philox (1), noise, float32 grid, internal noise, {by polarity, symmetric only}, no frame index
INSTANCES = [f"esim_voxel_kernel<1, 4, {bins}, 1, true, false, false, {sym}, false>" for bins in (0, 1) for sym in ("false", "true")]


@pytest.fixture(scope="module")
def resources():
    if not os.path.exists(SO):
        import __graft_entry__
        __graft_entry__.build()
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.from_so(SO)


@pytest.mark.parametrize("instance", INSTANCES)
def test_float32_four_pixel_noise_instances_fit_four_waves_without_scratch(resources, instance):
    hit = [r for r in resources.values() if instance in r["demangled"]]
    assert len(hit) == 1, instance
    r = hit[0]
    assert r["vgpr"] <= 128, (instance, r["vgpr"])
    assert r.get("scratch_bytes", 0) == 0 and r.get("vgpr_spill", 0) == 0 and r["scratch_instructions"] == 0, (instance, r)
