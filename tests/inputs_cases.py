"""Cases, restatements and derived bounds shared by tests/test_inputs_cpu.py and tests/test_vk_inputs_gpu.py (vk.inputs).

Stem sweep.  The maps are those of tests/test_conv_sweep_gpu.py and the operands come from the same generators in the same order as its
``stem_operands``, with ``cin`` in place of 3: integers in [-2, 2], ternary weights, so every fp32 partial sum is exact and the kernels
are compared with float64 by equality.  test_inputs_cpu.py proves on the reference alone that the conditions for that hold.

The mix.  ``mix_ref`` composes ``fma32`` of tests/averaging_ref.py exactly as include/vk_unet.h states vk_input_mix.

Bounds (u = 2^-24, the unit round-off of fp32):

* ``luma_bound``: a gray value v replicated, normalised per channel to t_j = (v/255 - mean_j) / std_j and stored in fp32 (relative error
  u each), mixed with the fp32-rounded luma row (relative error u each) by three fmas (one rounding each, of a partial sum that is at
  most S (1 + u)^2 in magnitude, S = sum_j |M_j t_j|): |result - (v/255 - mean_g) / std_g| <= (2 u + u^2) S + 3 u (1 + u)^4 S < 6 u S.

* ``gray_stem_bound``: a colour stem on a replicated plane g against the gray stem whose weight is the sum of the three
  (``adapt_first_conv``), both in fp32.  With A = conv(|g|, |w_0| + |w_1| + |w_2|) per output element, gamma_n = n u / (1 - n u) and E
  the exact value sum (w_0 + w_1 + w_2) g: the colour result is an fp32 dot product of 147 terms in some order (with or without fused
  multiply-adds), within ``colour_term`` = gamma_147 A of E; the summed weight ws = fl(fl(w_0 + w_1) + w_2) is within gamma_2 (|w_0| +
  |w_1| + |w_2|) of the exact sum, and its 49-term fp32 dot product within gamma_49 conv(|g|, |ws|) <= gamma_49 (1 + gamma_2) A of its
  own exact value, so the gray result is within ``gray_term`` = (gamma_2 + gamma_49 (1 + gamma_2)) A of E.  Together |colour - gray| <=
  colour_term + gray_term = (147 + 49 + 2) u (1 + O(u)) A < 200 u A.  tests/test_inputs_cpu.py holds each side to its own term."""
import numpy as np
import torch

import conv_lattice as CL
from averaging_ref import fma32

U32 = 2.0 ** -24
CINS = (1, 2, 4)
STEM_MAPS = [(3, 2, 2), (1, 8, 32), (1, 66, 34), (2, 40, 104)]          # forward and weight gradient
DGRAD_MAPS = [(2, 8, 32), (1, 40, 96), (1, 72, 32)]                     # data gradient (H % 8 == 0, W % 32 == 0)
DTYPES = ("f32", "bf16", "f16")
DW0 = 5.0                                                               # dw is accumulated into: it starts from a constant
MIX_HW = (1, 5, 4096 + 3)

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
LUMA_WEIGHTS = (0.299, 0.587, 0.114)


def stem_operands(N, H, W, cin, seed):
    g = torch.Generator().manual_seed(seed)
    x = CL.ints((N, cin, H, W), -2, 2, g)
    w = CL.ternary((64, cin, 7, 7), 1.0, g)
    dz = CL.ints((N, 64, H // 2, W // 2), -2, 2, g)
    return x, w, dz


def bn_fold(dz, seed):
    """(z, a, b, c, a dz + b z + c) with the dyadic coefficients of the existing sweep."""
    g = torch.Generator().manual_seed(seed)
    z = CL.ints(tuple(dz.shape), -2, 2, g)
    a, bb, cc = CL.lat_scale(64, 0), CL.lat_int(64, 1, 3), CL.lat_int(64, 2, 5) * 0.5
    return z, a, bb, cc, a.view(1, -1, 1, 1) * dz + bb.view(1, -1, 1, 1) * z + cc.view(1, -1, 1, 1)


def mix_ref(x3, M, b):
    """x3 fp32 [N][3][hw], M [cout][3], b [cout] -> fp32 [N][cout][hw]: fma(M2, x2, fma(M1, x1, fma(M0, x0, b)))."""
    x3 = np.asarray(x3, dtype=np.float32)
    M, b = np.asarray(M, dtype=np.float32), np.asarray(b, dtype=np.float32)
    out = np.empty((x3.shape[0], M.shape[0], x3.shape[2]), dtype=np.float32)
    for o in range(M.shape[0]):
        acc = np.full(x3[:, 0].shape, b[o], dtype=np.float32)
        for j in range(3):
            acc = fma32(x3[:, j], M[o, j], acc)
        out[:, o] = acc
    return out


def luma_row():
    std_g = sum(w * s for w, s in zip(LUMA_WEIGHTS, IMAGENET_STD))
    return [w * s / std_g for w, s in zip(LUMA_WEIGHTS, IMAGENET_STD)]


def luma_closed_form(v):
    """float64 (v/255 - mean_g) / std_g and S = sum_j |M_j t_j| for gray values v."""
    v = np.asarray(v, dtype=np.float64)
    mean_g = sum(w * m for w, m in zip(LUMA_WEIGHTS, IMAGENET_MEAN))
    std_g = sum(w * s for w, s in zip(LUMA_WEIGHTS, IMAGENET_STD))
    t = [(v / 255.0 - m) / s for m, s in zip(IMAGENET_MEAN, IMAGENET_STD)]
    S = sum(abs(Mj * tj) for Mj, tj in zip(luma_row(), t))
    return (v / 255.0 - mean_g) / std_g, t, S


def luma_bound(S):
    return 6.0 * U32 * S


def gamma(n):
    return n * U32 / (1.0 - n * U32)


def gray_stem_A(gray, w3):
    """conv(|g|, sum_j |w_j|), float64 [N][64][H/2][W/2] (gray [N][1][H][W], w3 [64][3][7][7])."""
    return torch.nn.functional.conv2d(gray.double().abs(), w3.double().abs().sum(1, keepdim=True), stride=2, padding=3)


def colour_term(A):
    return gamma(147) * A


def gray_term(A):
    return (gamma(2) + gamma(49) * (1.0 + gamma(2))) * A


def gray_stem_bound(gray, w3):
    """200 u conv(|g|, sum_j |w_j|) >= colour_term + gray_term."""
    return 200.0 * U32 * gray_stem_A(gray, w3)
