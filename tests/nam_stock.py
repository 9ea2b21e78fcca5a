"""NER-Net's NAM cell restated with stock PyTorch ops (the semantics of NAM_withoutGCB.forward, model/nernet/submodules.py:585-642 of the
reference, written from its formulas), the input recipe of the operator tests, and a CPU emulation of the device kernels' arithmetic.  A
helper module, not a test: tests/test_nam_step.py and tests/test_nam_concurrency.py import it.

    nam_case(b, c, h, w, seed)        tests/test_convgru.py::_case's recipe for the cell: N(0,1) input, tanh(N(0,1)) states, weights uniform
                                      +-3 / sqrt(fan_in of the gate they feed) rounded to bf16
    nam_ref(x, m, h, c, ws, dtype)    the cell in `dtype` on the CPU -> dict(m, alpha, c, o_pre, h)
    nam_emulate(...)                  bf16 operands, float32 accumulation in a shuffled order in steps of 16 (one MFMA), float32 gates,
                                      c' and m' rounded to bf16 in front of the last convolutions: what the three launches compute
"""
import numpy as np
import torch
import torch.nn.functional as F

KEYS = ("conv_x", "conv_h", "conv_m", "conv_o", "conv_last", "lag")

# the operator tests' shapes (tests/test_convgru.py's list: every column tiling, partial last tiles)
SHAPES = [(2, 64, 16, 16), (1, 128, 8, 24), (3, 64, 12, 16), (1, 256, 8, 8), (1, 64, 6, 6), (5, 128, 12, 10), (1, 256, 24, 30)]


def bf16_round(t):
    return t.to(torch.bfloat16).to(torch.float32)


def nam_case(b, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((b, c, h, w), generator=g)
    m, hp, cp = (torch.tanh(torch.randn((b, c, h, w), generator=g)) for _ in range(3))
    u = lambda *s: torch.rand(s, generator=g) * 2 - 1                                       # noqa: E731
    k3, k1 = 3.0 / np.sqrt(2 * c * 9), 3.0 / np.sqrt(2 * c)                                 # a gate sums two 3x3 convolutions of C channels
    ws = {"conv_x": u(7 * c, c, 3, 3) * k3, "conv_h": u(4 * c, c, 3, 3) * k3, "conv_m": u(3 * c, c, 3, 3) * k3, "conv_o": u(c, 2 * c, 3, 3) * k3,
          "conv_last": u(c, 2 * c, 1, 1) * k1, "lag": u(c, c, 1, 1) * 3.0 / np.sqrt(c)}
    return x, m, hp, cp, {k: bf16_round(v) for k, v in ws.items()}


def nam_gates(xc, hc, mc, lag, c_prev, m_prev):
    """the cell's arithmetic behind its first three convolutions: xc [B,7C,..], hc [B,4C,..] or None, mc [B,3C,..], lag [B,C,..]"""
    ix, fx, gx, ipx, fpx, gpx, ox = xc.chunk(7, 1)
    ih, fh, gh, oh = hc.chunk(4, 1) if hc is not None else (0, 0, 0, 0)
    im, fm, gm = mc.chunk(3, 1)
    i_t = torch.sigmoid(ix + ih)
    alpha = torch.exp(torch.sigmoid(lag))
    f_t = torch.sigmoid(torch.sigmoid(fx + fh + 1) - alpha * i_t)
    c_new = i_t * torch.tanh(gx + gh) + (f_t * c_prev if c_prev is not None else 0)
    m_new = torch.sigmoid(fpx + fm + 1) * m_prev + torch.sigmoid(ipx + im) * torch.tanh(gpx + gm)
    return {"m": m_new, "alpha": alpha, "c": c_new, "o_pre": ox + oh}


def nam_out(o_pre, c_new, m_new, ws, dtype):
    mem = torch.cat([c_new.to(dtype), m_new.to(dtype)], 1)
    return torch.sigmoid(o_pre.to(dtype) + F.conv2d(mem, ws["conv_o"].to(dtype), padding=1)) * torch.tanh(F.conv2d(mem, ws["conv_last"].to(dtype)))


def nam_ref(x, m, h, c, ws, dtype):
    """x, m [B,C,H,W]; h, c the previous state or both None (zero)"""
    w = {k: v.to(dtype) for k, v in ws.items()}
    x, m = x.to(dtype), m.to(dtype)
    out = nam_gates(F.conv2d(x, w["conv_x"], padding=1), F.conv2d(h.to(dtype), w["conv_h"], padding=1) if h is not None else None,
                    F.conv2d(m, w["conv_m"], padding=1), F.conv2d(x, w["lag"]), c.to(dtype) if c is not None else None, m)
    out["h"] = nam_out(out["o_pre"], out["c"], out["m"], ws, dtype)
    return out


def _conv_shuffled(parts, gen):
    """sum over parts of conv2d(x, w, padding) in float32, the K = sum(Cin * taps) products added in a shuffled order, 16 at a time"""
    cols, wts = [], []
    for x, w in parts:
        cols.append(F.unfold(x.float(), w.shape[2], padding=w.shape[2] // 2))               # [B, Cin * taps, L]
        wts.append(w.float().flatten(1))
    col, wt = torch.cat(cols, 1), torch.cat(wts, 1)
    perm = torch.randperm(col.shape[1], generator=gen)
    acc = torch.zeros((col.shape[0], wt.shape[0], col.shape[2]))
    for k0 in range(0, len(perm), 16):
        idx = perm[k0:k0 + 16]
        acc = acc + torch.einsum("nk,bkl->bnl", wt[:, idx], col[:, idx])
    b, _, hh, ww = parts[0][0].shape
    return acc.reshape(b, -1, hh, ww)


def nam_emulate(x, m, h, c, ws, seed=0):
    """the device scheme on the CPU (operands rounded to bf16 here; c stays float32) -> dict(m, alpha, c, o_pre, h) in float32"""
    gen = torch.Generator().manual_seed(seed)
    xr, mr, hr = bf16_round(x), bf16_round(m), bf16_round(h) if h is not None else None
    cx = ws["conv_x"].chunk(7, 0)
    ch = ws["conv_h"].chunk(4, 0) if h is not None else None
    cm = ws["conv_m"].chunk(3, 0)
    pair = lambda wx, second, wsec: _conv_shuffled([(xr, wx)] + ([(second, wsec)] if second is not None else []), gen)   # noqa: E731
    xc = [pair(cx[k], hr, ch[k] if ch else None) for k in range(3)] + [pair(cx[3 + k], mr, cm[k]) for k in range(3)] + [pair(cx[6], hr, ch[3] if ch else None)]
    zero = torch.zeros_like(xc[0])
    out = nam_gates(torch.cat(xc, 1), torch.cat([zero] * 4, 1), torch.cat([zero] * 3, 1), _conv_shuffled([(xr, ws["lag"])], gen),
                    c.float() if c is not None else None, mr)
    mem = torch.cat([bf16_round(out["c"]), bf16_round(out["m"])], 1)
    out["h"] = torch.sigmoid(out["o_pre"] + _conv_shuffled([(mem, ws["conv_o"])], gen)) * torch.tanh(_conv_shuffled([(mem, ws["conv_last"])], gen))
    return out


if __name__ == "__main__":                                     # the figures quoted in tests/test_nam_step.py's docstring
    worst = {}
    for shape in SHAPES:
        for zero_state in (False, True):
            x, m, h, c, ws = nam_case(*shape, seed=sum(shape))
            if zero_state:
                h = c = None
            emu = nam_emulate(x, m, h, c, ws)
            same = nam_ref(bf16_round(x), bf16_round(m), bf16_round(h) if h is not None else None, c, ws, torch.float64)
            same["h"] = nam_out(emu["o_pre"], bf16_round(emu["c"]), bf16_round(emu["m"]), ws, torch.float64)
            plain = nam_ref(x, m, h, c, ws, torch.float32)
            fig = {"same_operands": max(float((emu[k].double() - same[k]).abs().max()) for k in same),
                   "fp32_module": max(float((emu[k] - plain[k]).abs().max()) for k in plain)}
            print(shape, "zero state" if zero_state else "", fig)
            for k, v in fig.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("worst", worst)
