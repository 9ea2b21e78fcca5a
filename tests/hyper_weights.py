"""Deterministic weights for golden G26 (HyperE2VID): tests/seeded_weights.py's recipe, then the entries that recipe cannot fill sensibly
(it draws every tensor uniform in +-gain / sqrt(fan_in)): the Fourier-Bessel `bases` buffer keeps the module's own values, BatchNorm's
running_var is positive (0.5 + 4 |v|), its weight near 1 (1 + 0.1 v), num_batches_tracked 0.  `compositional_coefficients` does not end
in "weight", so the recipe draws it with the fan-in of the 1-D tensor before it (+-gain): the network golden keeps that (its image stays
O(1) through the 1x1 prediction), the single-layer golden multiplies it by coeff_scale = 1/32 so that the layer's output is O(1).  Shared by the generator
(tests/golden/make_golden_hyper.py, which loads the result into the REFERENCE's modules) and the tests (v2v_amd's modules, same keys)."""
import numpy as np

from seeded_weights import seeded_state


def hyper_state(shapes, seed, gain, bases, coeff_scale=1.0):
    """shapes: ordered {state_dict key: shape}; bases: the float32 [12,25] value every `...bases` key keeps.  Returns {key: ndarray}."""
    vals = seeded_state(shapes, seed, gain)
    for k, v in vals.items():
        if k.endswith(".bases") or k == "bases":
            vals[k] = np.asarray(bases, dtype=np.float32).reshape(v.shape)
        elif k.endswith("running_var"):
            vals[k] = (0.5 + 4.0 * np.abs(v)).astype(np.float32)
        elif k.endswith("num_batches_tracked"):
            vals[k] = np.zeros(v.shape, dtype=np.int64)
        elif k.endswith("compositional_coefficients"):
            vals[k] = (v * np.float32(coeff_scale)).astype(np.float32)
        elif k.endswith("weight") and v.ndim == 1:                  # BatchNorm's scale
            vals[k] = (1.0 + 0.1 * v).astype(np.float32)
    return vals


def load_hyper(module, seed, gain=1.0, coeff_scale=1.0):
    """Fill `module` (the reference's or the package's; its own `bases` buffers are kept) with hyper_state values; returns the dict."""
    import torch
    sd = module.state_dict()
    bases = next(v for k, v in sd.items() if k.endswith("bases")).detach().cpu().numpy()
    vals = hyper_state({k: tuple(v.shape) for k, v in sd.items()}, seed, gain, bases, coeff_scale)
    module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vals.items()}, strict=True)
    return vals
