"""Integer-lattice cases for vk_conv_bwd_onepass and their float64 reference, by the method of tests/conv_lattice.py (no GPU needed;
tests/test_bwd_onepass_cpu.py checks this module, tests/test_bwd_onepass_gpu.py runs the kernel on its cases).

One case is a whole backward of a small-channel convolution, C = K = 16 or 32:
    dz = a * g + b * z + c                      g, z integers in [-2, 2], a from {0.5, 1, 2}, b from {-0.5, 0, 0.5}, c integers in [-3, 3]
    V  = relu(z1 * scale + shift)               z1 integers in [-2, 2], scale from {0.5, 1, 2}, integer shift in [-3, 3]
    dx = d conv2d(x, wf) / dx applied to dz     wf ternary
    y  = dx * [z1 * scale + shift > 0],  sums = sum y, sum y * z1 per channel
    dw = d conv2d(V, w) / dw applied to dz
Every dz and V is a multiple of 0.5 of magnitude at most 8 / 7, every dx a multiple of 0.5, every dw a multiple of 0.25: whatever the
order of accumulation, every partial sum is exact in fp32 while it stays below 2^22 (quarters), and every stored value is exact in bf16
(8 significant bits) while a multiple of 0.5 stays below 128.  `check` asserts exactly that on the reference alone.

Densities.  E[dz^2] = E[a^2] E[g^2] + E[b^2] E[z^2] + E[c^2] = 1.75 * 2 + 1/6 * 2 + 4 = 7.8; dx is a sum of 9 K density terms +-dz, so its
variance is 70 K density.  Sigma = 18 keeps 6 sigma below 128: density 0.28 at K = 16, 0.14 at K = 32."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from conv_lattice import TWO24, exact_in, ints, lat_int, lat_scale, strip_partial, ternary

MAPS = [(2, 72, 40), (1, 132, 20), (3, 6, 96)]
HALF_LIM = 128.0                    # multiples of 0.5 below this are exact in bf16 (and in f16)
DENSITY = {16: 0.28, 32: 0.14}


def lat_b(C):
    c = torch.arange(C)
    return torch.tensor([-0.5, 0.0, 0.5], dtype=torch.float64)[(c // 3) % 3]


def cases():
    return [(CK, N, H, W, 700 + 10 * i + CK) for CK in (16, 32) for i, (N, H, W) in enumerate(MAPS)]


def case_id(c):
    return f"c{c[0]}_n{c[1]}_{c[2]}x{c[3]}"


def build(case):
    CK, N, H, W, seed = case
    gen = torch.Generator().manual_seed(seed)
    b = SimpleNamespace(case=case, CK=CK, N=N, H=H, W=W)
    b.g, b.z, b.z1 = (ints((N, CK, H, W), -2, 2, gen) for _ in range(3))
    b.coef = torch.stack([lat_scale(CK, 0), lat_b(CK), lat_int(CK, 3, 7)])               # [3][K]: a, b, c
    b.scale, b.shift = lat_scale(CK, 1), lat_int(CK, 2, 7)
    view = lambda t: t.view(1, -1, 1, 1)
    b.dz = view(b.coef[0]) * b.g + view(b.coef[1]) * b.z + view(b.coef[2])
    pre = b.z1 * view(b.scale) + view(b.shift)
    b.V = torch.relu(pre)
    b.wf = ternary((CK, CK, 3, 3), DENSITY[CK], gen)                                     # forward weights [K][C][3][3]
    b.w_dgrad = b.wf.permute(1, 0, 2, 3).contiguous()                                    # as the data gradient indexes them: [C][K][3][3]
    xin = torch.zeros(N, CK, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, b.wf, padding=1).backward(b.dz)
    b.dx = xin.grad
    xa = torch.zeros_like(xin, requires_grad=True)
    F.conv2d(xa, b.wf.abs(), padding=1).backward(b.dz.abs())
    b.dx_absdot = xa.grad
    b.y = b.dx * (pre > 0)
    b.sums = torch.stack([b.y.sum(dim=(0, 2, 3)), (b.y * b.z1).sum(dim=(0, 2, 3))])
    wv = torch.zeros(CK, CK, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(b.V, wv, padding=1).backward(b.dz)
    b.dw = wv.grad
    wa = torch.zeros_like(wv, requires_grad=True)
    F.conv2d(b.V, wa, padding=1).backward(b.dz.abs())
    b.dw_absdot = wa.grad
    return b


def check(b):
    """The exactness conditions, on the reference alone.  Returns the figures it checked."""
    fig = {}
    for name in ("g", "z", "z1", "dz", "V", "dx", "y"):
        t = getattr(b, name)
        fig["max_" + name] = t.abs().max().item()
        assert bool((t * 2 == (t * 2).round()).all()), f"{name}: not a multiple of 0.5"
        assert fig["max_" + name] < HALF_LIM, f"{name} reaches {fig['max_' + name]}"
        for dtn in ("bf16", "f16"):
            assert exact_in(t, dtn), f"{name} is not exact in {dtn}"
    # any order of accumulation: the data gradient's sums are halves, the weight gradient's quarters
    fig["dx_absdot"] = b.dx_absdot.max().item()
    fig["dw_absdot"] = b.dw_absdot.max().item()
    assert 2 * fig["dx_absdot"] < TWO24 and 4 * fig["dw_absdot"] < TWO24
    # the weight gradient of one strip (16 columns, up to 256 rows) is bounded by the whole map's, which the line above covers; the
    # BN-backward sums stay in fp32 over a strip: halves
    fig["strip"] = max(strip_partial(b.y), strip_partial(b.y * b.z1))
    assert 2 * fig["strip"] < TWO24
    assert bool((b.dw * 4 == (b.dw * 4).round()).all())
    return fig
