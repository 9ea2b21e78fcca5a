"""Integer-exact inputs for the learned-voxelisation tests (tests/test_nernet_ops.py, tests/test_nernet_concurrency.py).

The MLP has 0/1 weights (two ones per row of a hidden layer) and 0/1 biases; the activation slope is 0.25; times are integers that
normalise to themselves (first row of a batch at t = 0, last at t = C - 1, C - 1 a power of two).  Every activation is then a multiple of
0.25^(hidden layers) <= 1/64 below 2^7, every term t_n * MLP a multiple of 1/64 below 2^10, and a cell's sum is exact in float32 in ANY order
as long as the sum of its terms' magnitudes stays below 2^18 (the tests assert that on the float64 restatement)."""
import numpy as np
import torch

SLOPE = 0.25


def exact_mlp(mlp_layers, seed):
    """-> (weights, biases): float32 tensors shaped like nn.Linear's"""
    g = np.random.Generator(np.random.PCG64([seed, len(mlp_layers), max(mlp_layers)]))
    ws, bs = [], []
    for i, (fin, fout) in enumerate(zip(mlp_layers[:-1], mlp_layers[1:])):
        w = np.zeros((fout, fin), dtype=np.float32)
        if fin == 1:
            w[:, 0] = g.integers(0, 2, fout)
            w[g.integers(0, fout), 0] = 1
        else:
            for j in range(fout):
                w[j, g.choice(fin, size=min(2, fin), replace=False)] = 1
        ws.append(torch.from_numpy(w))
        bs.append(torch.from_numpy(g.integers(0, 2, fout).astype(np.float32)))
    return ws, bs


def exact_rows(seed, n, C, B, H, W, dtype=torch.float64, pol=(-1, 1)):
    """[n, 5] rows with interleaved batch ids (the last row has B - 1) and integer times: per batch id with two rows or more the first row
    has t = 0 and the last t = C - 1, so the normalisation is the identity on integers; a batch id with one row keeps its raw integer t."""
    g = np.random.Generator(np.random.PCG64([seed, n, C, B]))
    ev = np.zeros((n, 5))
    ev[:, 0] = g.integers(0, W, n)
    ev[:, 1] = g.integers(0, H, n)
    ev[:, 2] = g.integers(0, C, n)
    ev[:, 3] = g.choice(pol, n)
    b = (np.arange(n) + (B - 1) - (n - 1)) % B
    ev[:, 4] = b
    for bi in range(B):
        idx = np.nonzero(b == bi)[0]
        if len(idx) >= 2:
            ev[idx[0], 2], ev[idx[-1], 2] = 0, C - 1
        elif len(idx) == 1:
            ev[idx[0], 2] = max(C - 2, 1)
    return torch.from_numpy(ev).to(dtype)


def with_specials(ev, C, B, H, W):
    """Overwrite a few middle rows (never a batch's first or last) with the index corner cases: past the grid's end (clamped to the last
    cell), negative (wrapped once), below -numel (dropped; put_ raises there) and raw 0 polarity (p01 = 0.5)."""
    n = ev.shape[0]
    if n < 40:
        return ev
    ev = ev.clone()
    numel = 2 * C * H * W * B
    k = n // 2
    ev[k + 0, 0], ev[k + 0, 1] = W - 1, H - 1 + 2 * C * B * H                         # far past the end
    ev[k + 1, 0], ev[k + 1, 1] = W - 1, 3 * H
    ev[k + 2, 0], ev[k + 2, 1], ev[k + 2, 3] = -3.0, 0, -1                            # wraps for batch 0 / bin 0
    ev[k + 2, 4] = 0
    ev[k + 3, 0], ev[k + 3, 1], ev[k + 3, 3], ev[k + 3, 4] = -float(numel) - 5, 0, -1, 0      # below -numel in bin 0 (dropped), wraps in the others
    ev[k + 4, 3] = 0                                                                  # raw 0/1 polarity
    ev[k + 5, 3] = 0
    ev[k + 6, 0] = float(numel) * 4                                                   # clamped in every bin
    return ev
