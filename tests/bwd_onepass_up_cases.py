"""Integer-lattice cases for the upsampled-source form of vk_conv_bwd_onepass and their float64 reference, by the method of
tests/bwd_onepass_cases.py (no GPU needed; tests/test_bwd_onepass_up_cpu.py checks this module, tests/test_up_bwd_onepass_gpu.py runs the
kernel on its cases).

One case is the whole backward of a 32 -> 16 convolution whose source is upsampled x2 by nearest neighbour (decoder block 4 conv1):
    dz = a * g + b * z + c                      g, z [N][16][H][W] integers in [-2, 2], the coefficient lattices of bwd_onepass_cases
    V  = up2(relu(z1 * scale + shift))          z1 [N][32][H/2][W/2] integers in [-2, 2], scale from {0.5, 1, 2}, integer shift in [-3, 3]
    dx = d conv2d(x, wf) / dx applied to dz     wf [16][32][3][3] ternary; full resolution, 32 channels
    p  = the 2 x 2 sums of dx                   [N][32][H/2][W/2]
    y  = p * [z1 * scale + shift > 0],  sums = sum y, sum y * z1 per channel
    dw = d conv2d(V, w) / dw applied to dz
Every dz and V is a multiple of 0.5, so every dx and every pooled value is a multiple of 0.5 and every dw a multiple of 0.25; `check`
asserts on the reference alone that the stored and intermediate values stay below 128 (exact in bf16 and f16) and every partial sum
below 2^24 in halves / quarters.

Density.  dx is a sum of 9 * 16 * density terms +-dz with E[dz^2] = 7.8 (bwd_onepass_cases); the pooled value adds four of them, which
share the dz they read only in part: its variance is at most 4 * 4 * 9 * 16 * 7.8 * density (fully correlated) and about a quarter of
that when the four are independent.  Density 0.07 puts sigma between 18 and 35; the drawn maxima are what `check` decides on: pooled
maxima 102.5 - 108.5 on the three maps.  A draw that fails `check` is answered by a lower density, never by a wider `check`."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from bwd_onepass_cases import HALF_LIM, MAPS, lat_b
from conv_lattice import TWO24, exact_in, ints, lat_int, lat_scale, strip_partial, ternary

C_SRC, K_OUT = 32, 16
DENSITY = 0.07


def cases():
    return [(N, H, W, 900 + 10 * i) for i, (N, H, W) in enumerate(MAPS)]


def case_id(c):
    return f"up_n{c[0]}_{c[1]}x{c[2]}"


def build(case):
    N, H, W, seed = case
    assert H % 2 == 0 and W % 2 == 0
    gen = torch.Generator().manual_seed(seed)
    b = SimpleNamespace(case=case, N=N, H=H, W=W)
    b.g, b.z = (ints((N, K_OUT, H, W), -2, 2, gen) for _ in range(2))
    b.z1 = ints((N, C_SRC, H // 2, W // 2), -2, 2, gen)
    b.coef = torch.stack([lat_scale(K_OUT, 0), lat_b(K_OUT), lat_int(K_OUT, 3, 7)])      # [3][16]: a, b, c
    b.scale, b.shift = lat_scale(C_SRC, 1), lat_int(C_SRC, 2, 7)
    view = lambda t: t.view(1, -1, 1, 1)
    b.dz = view(b.coef[0]) * b.g + view(b.coef[1]) * b.z + view(b.coef[2])
    pre = b.z1 * view(b.scale) + view(b.shift)
    b.Vs = torch.relu(pre)                                                               # at the source's resolution
    b.V = F.interpolate(b.Vs, scale_factor=2, mode="nearest")
    b.wf = ternary((K_OUT, C_SRC, 3, 3), DENSITY, gen)                                   # forward weights [K][C][3][3]
    b.w_dgrad = b.wf.permute(1, 0, 2, 3).contiguous()                                    # as the data gradient indexes them: [C][K][3][3]
    xin = torch.zeros(N, C_SRC, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, b.wf, padding=1).backward(b.dz)
    b.dx = xin.grad
    xa = torch.zeros_like(xin, requires_grad=True)
    F.conv2d(xa, b.wf.abs(), padding=1).backward(b.dz.abs())
    b.dx_absdot = xa.grad
    b.pooled = F.avg_pool2d(b.dx, 2) * 4.0
    b.y = b.pooled * (pre > 0)
    b.sums = torch.stack([b.y.sum(dim=(0, 2, 3)), (b.y * b.z1).sum(dim=(0, 2, 3))])
    wv = torch.zeros(K_OUT, C_SRC, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(b.V, wv, padding=1).backward(b.dz)
    b.dw = wv.grad
    wa = torch.zeros_like(wv, requires_grad=True)
    F.conv2d(b.V, wa, padding=1).backward(b.dz.abs())
    b.dw_absdot = wa.grad
    return b


def check(b):
    """The exactness conditions, on the reference alone.  Returns the figures it checked."""
    fig = {}
    for name in ("g", "z", "z1", "dz", "Vs", "dx", "pooled", "y"):
        t = getattr(b, name)
        fig["max_" + name] = t.abs().max().item()
        assert bool((t * 2 == (t * 2).round()).all()), f"{name}: not a multiple of 0.5"
        assert fig["max_" + name] < HALF_LIM, f"{name} reaches {fig['max_' + name]}"
        for dtn in ("bf16", "f16"):
            assert exact_in(t, dtn), f"{name} is not exact in {dtn}"
    # any order of accumulation: the data gradient's sums are halves (the pooled value adds four of them), the weight gradient's quarters
    fig["dx_absdot"] = b.dx_absdot.max().item()
    fig["dw_absdot"] = b.dw_absdot.max().item()
    assert 2 * 4 * fig["dx_absdot"] < TWO24 and 4 * fig["dw_absdot"] < TWO24
    # the BN-backward sums stay in fp32 over a strip (at most 128 x 8 pooled pixels, inside the 256 x 16 window of strip_partial): halves
    fig["strip"] = max(strip_partial(b.y), strip_partial(b.y * b.z1))
    assert 2 * fig["strip"] < TWO24
    assert bool((b.dw * 4 == (b.dw * 4).round()).all())
    return fig
