"""Inputs and the covering sets shared by tests/test_lovasz_cpu.py and tests/test_lovasz_gpu.py.  Inputs are those of
tests/seglosses_cases.py (logits 3 * randn, 5 % or uniform foreground, one class absent when C > 1, 10 % ignored entries); the
quantised variants round the logits to multiples of 0.25, which makes thousands of exactly equal errors (the tie order then decides
the gradient)."""
import numpy as np
import torch

import lovasz_ref as LR
import seglosses_cases as K

IGN = K.IGN
SHAPES = K.SHAPES

# (mode, C, per_image, ignore, shape index, quantised)
HINGE = [("binary", 1, False, False, 0, False), ("binary", 1, True, True, 1, False), ("binary", 1, False, True, 0, True),
         ("multilabel", 1, False, False, 1, False), ("multilabel", 4, True, False, 0, False), ("multilabel", 4, False, True, 1, False),
         ("multilabel", 16, True, True, 1, True), ("multilabel", 16, False, False, 0, False)]
# (C, per_image, ignore, shape index, quantised).  d0 of each case (the relative L2 distance between the reference gradient formed from
# fp32-rounded probabilities and from float64 ones, measured on the CPU by softmax_d0 below), in this order:
#   2.4e-09, 0 (no swap), 5.1e-06, 9.1e-06, 6.3e-09, 0, 0
SOFTMAX = [(2, False, False, 0, False), (3, True, True, 1, False), (4, False, True, 0, False), (4, True, False, 1, True),
           (5, True, False, 0, False), (16, False, True, 1, False), (16, True, False, 0, True)]


def ident(case):
    return "-".join(str(c) for c in case)


def inputs(mode, C, ignore, shape_index, quantised, seed=3):
    N, H, W = SHAPES[shape_index]
    x, t = K.make_inputs(mode, C, N, H, W, ignore, seed=seed)
    if quantised:
        x = torch.round(x * 4.0) / 4.0
    return x, t


def softmax_d0(x, t, per_image, ign):
    """relative L2 distance of the reference gradient between fp32-rounded and float64 probabilities"""
    _, g64, _ = LR.softmax(x.numpy(), t.numpy(), per_image, ign)
    _, g32, _ = LR.softmax(x.numpy(), t.numpy(), per_image, ign, fp32_probs=True)
    return float(np.linalg.norm(g32 - g64) / np.linalg.norm(g64))
