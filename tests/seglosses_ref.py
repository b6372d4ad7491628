"""float64 restatement of the vk.seglosses contract in closed form: the per-class sums, every term's value and the analytic gradient
that csrc/seg_loss.hip computes.  tests/test_seglosses_cpu.py checks it against torch autograd of the formulas written naively (and
against torch.nn.functional where torch has the loss); the GPU tests compare the kernels to it.

``spec`` is what ``LossSum.spec(C)`` returns: dict(mode, ignore_index, terms={kind: options}) with kind in pix / focal / dice /
jaccard / tversky, every options dict holding its weight ``w``.  A term whose denominator is empty (every entry ignored) is 0."""
import torch

KINDS = ("pix", "focal", "dice", "jaccard", "tversky")


def _softplus_neg(x):
    return (-x).clamp_min(0) + torch.log1p(torch.exp(-x.abs()))


def evaluate(x, target, spec):
    """x [N,C,H,W] (any float dtype, evaluated in float64), target per mode.  Returns dict(total, pix, focal, dice, jaccard, tversky:
    float64 scalars, unweighted term values; dlogits: float64 d total / dx in x's shape)."""
    shape = x.shape
    N, C = shape[0], shape[1]
    mode, ign, terms = spec["mode"], spec["ignore_index"], spec["terms"]
    x = x.detach().double().reshape(N, C, -1)
    HW = x.shape[2]
    if mode == "multiclass":
        t = target.reshape(N, HW)
        mpx = (t != ign) if ign is not None else torch.ones_like(t, dtype=torch.bool)
        m = mpx.double().view(N, 1, HW).expand(N, C, HW)
        y = torch.nn.functional.one_hot(torch.where(mpx, t, torch.zeros_like(t)), C).permute(0, 2, 1).double() * m
        logp = torch.log_softmax(x, dim=1)
        p = logp.exp()
        n_valid = mpx.sum().double()           # pixels
        n_all = float(N * HW)
    else:
        y0 = target.detach().double().expand(shape).reshape(N, C, HW)
        m = (y0 != ign).double() if ign is not None else torch.ones_like(y0)
        y = y0 * m
        p = torch.sigmoid(x)
        n_valid = m.sum()                      # entries
        n_all = float(N * C * HW)
    sig = torch.sigmoid(x)
    zero = torch.zeros((), dtype=torch.float64, device=x.device)
    out = {k: zero for k in KINDS}
    dl = torch.zeros_like(x)

    if "pix" in terms:
        o = terms["pix"]
        sf = o["smooth_factor"]
        den = n_valid if o["denom"] == "valid" else torch.as_tensor(n_all, dtype=torch.float64, device=x.device)
        if den > 0:
            if mode == "multiclass":
                nll = -(logp * y).sum(dim=1)
                smooth = -logp.sum(dim=1) * m[:, 0]
                out["pix"] = ((1 - sf) * nll + sf / C * smooth).sum() / den
                g = (p - (1 - sf) * y - sf / C) * m
            else:
                pw = torch.ones(C, dtype=torch.float64, device=x.device) if o["pos_weight"] is None else \
                    torch.tensor(o["pos_weight"], dtype=torch.float64, device=x.device)
                pw = pw.view(1, C, 1)
                ys = (1 - y) * sf + y * (1 - sf)
                lw = 1 + (pw - 1) * ys
                out["pix"] = (((1 - ys) * x + lw * _softplus_neg(x)) * m).sum() / den
                g = ((1 - ys) - lw * (1 - sig)) * m
            dl += o["w"] * g / den
    if "focal" in terms:
        o = terms["focal"]
        gamma, alpha = o["gamma"], o["alpha"]
        if n_valid > 0:
            b = x.clamp_min(0) - x * y + torch.log1p(torch.exp(-x.abs()))
            q = -torch.expm1(-b)
            pt = torch.exp(-b)
            aw = alpha * y + (1 - alpha) * (1 - y) if alpha is not None else torch.ones_like(y)
            qg = q ** gamma if gamma != 0 else torch.ones_like(q)
            dqg = gamma * q ** (gamma - 1) if gamma != 0 else torch.zeros_like(q)
            out["focal"] = (qg * b * aw * m).sum() / n_valid
            dl += o["w"] * aw * (qg + dqg * pt * b) * (sig - y) * m / n_valid
    G = torch.zeros_like(x)
    pm = p * m
    I, P, T = (pm * y).sum(dim=(0, 2)), pm.sum(dim=(0, 2)), y.sum(dim=(0, 2))
    for kind in ("dice", "jaccard", "tversky"):
        if kind not in terms:
            continue
        o = terms[kind]
        smooth, eps = o["smooth"], o["eps"]
        if kind == "dice":
            nI, dI, dP, dT = 2.0, 0.0, 1.0, 1.0
        elif kind == "jaccard":
            nI, dI, dP, dT = 1.0, -1.0, 1.0, 1.0
        else:
            nI, dI, dP, dT = 1.0, 1.0 - o["alpha"] - o["beta"], o["alpha"], o["beta"]
        num = nI * I + smooth
        raw = dI * I + dP * P + dT * T + smooth
        cl = (raw > eps).double()
        den = raw.clamp_min(eps)
        score = num / den
        keep = (T > 0).double()
        if o["classes"] is not None:
            sel = torch.zeros(C, dtype=torch.float64, device=x.device)
            sel[o["classes"]] = 1.0
            K = len(o["classes"])
        else:
            sel = torch.ones(C, dtype=torch.float64, device=x.device)
            K = C
        keep = keep * sel
        if o["log_loss"]:
            l = -torch.log(score.clamp_min(eps))
            dls = torch.where(score > eps, -1.0 / score, torch.zeros_like(score))
        else:
            l = 1 - score
            dls = -torch.ones_like(score)
        mean = (l * keep).sum() / K
        outer = o["w"] / K
        if kind == "tversky" and o["gamma"] != 1.0:
            outer = outer * o["gamma"] * mean ** (o["gamma"] - 1.0)
            mean = mean ** o["gamma"]
        out[kind] = mean
        nd2 = num / (den * den) * cl
        a = outer * dls * keep * (nI / den - nd2 * dI)
        b_ = outer * dls * keep * (-nd2 * dP)
        G += (a.view(1, C, 1) * y + b_.view(1, C, 1)) * m
    if mode == "multiclass":
        dl += p * (G - (G * p).sum(dim=1, keepdim=True))
    else:
        dl += G * p * (1 - p)
    out["total"] = sum(terms[k]["w"] * out[k] for k in terms)
    out["dlogits"] = dl.reshape(shape)
    return out


def components(res):
    """[total, pix, focal, dice, jaccard, tversky] as a float64 tensor (loss_out[:6])"""
    return torch.stack([res["total"].reshape(())] + [res[k].reshape(()) for k in KINDS])
