"""Restatement of vk_kp_loss (csrc/kp_loss.hip) in float64 numpy: value, positives and gradient from the definitions of
include/vk_unet.h, with nothing of the kernel's structure (no tiles, no partial rows, no fp32).  No GPU is needed.

A configuration is a dict: heat, bce (lists of planes), w_heat, w_bce, alpha, beta, thr (the threshold as the float32 the kernel
compares with), pos_weight (None or a list of C numbers).  Weights, threshold and pos_weight are converted to float32 first, as the
configuration structure holds them, and then used exactly."""
from __future__ import annotations

import numpy as np


def cfg(heat=(), bce=(), w_heat=1.0, w_bce=1.0, alpha=2, beta=4, thr=1.0, pos_weight=None) -> dict:
    return dict(heat=sorted(int(c) for c in heat), bce=sorted(int(c) for c in bce), w_heat=float(np.float32(w_heat)),
                w_bce=float(np.float32(w_bce)), alpha=int(alpha), beta=int(beta), thr=float(np.float32(thr)),
                pos_weight=None if pos_weight is None else [float(np.float32(v)) for v in pos_weight])


def pieces(x):
    """log p, log(1 - p), p, 1 - p of float64 logits, without overflow."""
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    l1p = np.log1p(e)
    r = 1.0 / (1.0 + e)
    p = np.where(x >= 0, r, e * r)
    omp = np.where(x >= 0, e * r, r)
    return -(np.maximum(-x, 0.0) + l1p), -(np.maximum(x, 0.0) + l1p), p, omp


def heat_elements(x, y, c: dict):
    """-> (value per entry, d value / dx per entry, positive mask)"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    lp, l1mp, p, omp = pieces(x)
    a, b = c["alpha"], c["beta"]
    with np.errstate(invalid="ignore"):
        pos = y >= c["thr"]
    v_pos = -(omp ** a) * lp
    v_neg = -((1.0 - y) ** b) * (p ** a) * l1mp
    g_pos = a * p * (omp ** a) * lp - omp ** (a + 1)
    g_neg = ((1.0 - y) ** b) * (p ** (a + 1) - a * (p ** a) * omp * l1mp)
    return np.where(pos, v_pos, v_neg), np.where(pos, g_pos, g_neg), pos


def bce_elements(x, y, pw: float):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    lp, l1mp, p, omp = pieces(x)
    l1p = -lp - np.maximum(-x, 0.0)
    v = np.maximum(x, 0.0) - x * y + l1p + (pw - 1.0) * y * (-lp)
    g = p - y - (pw - 1.0) * y * omp
    return v, g


def evaluate(x, y, c: dict, grad_scale: float = 1.0) -> dict:
    """x, y [N][C][HW] -> dict(total, heat, bce, positives int64 [16], grad float64 [N][C][HW] = grad_scale * d total / dx (0 on the
    planes without a rule), coef float64 [C])"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    N, C, HW = x.shape
    grad = np.zeros_like(x)
    coef = np.zeros(C)
    positives = np.zeros(16, np.int64)
    heat = bce = 0.0
    for q in c["heat"]:
        v, g, pos = heat_elements(x[:, q], y[:, q], c)
        P = int(pos.sum())
        positives[q] = P
        heat += v.sum() / max(P, 1)
        coef[q] = c["w_heat"] / (len(c["heat"]) * max(P, 1))
        grad[:, q] = coef[q] * g
    if c["heat"]:
        heat /= len(c["heat"])
    n_all = N * HW * len(c["bce"])
    for q in c["bce"]:
        v, g = bce_elements(x[:, q], y[:, q], 1.0 if c["pos_weight"] is None else c["pos_weight"][q])
        bce += v.sum() / n_all
        coef[q] = c["w_bce"] / n_all
        grad[:, q] = coef[q] * g
    total = (c["w_heat"] * heat if c["heat"] else 0.0) + (c["w_bce"] * bce if c["bce"] else 0.0)
    return dict(total=total, heat=heat, bce=bce, positives=positives, grad=grad * float(grad_scale), coef=coef)
