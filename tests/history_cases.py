"""Engine state sweep: histories of calls on one model (the veteran) and the probes that follow them, written as data, and the
harness that runs them.  A probe is run on the veteran and on its twin — a fresh model of the same class with the veteran's state dict,
requires_grad flags, module modes and compute dtype, but no plans, no gradients and new optimizers — and everything observable must be
torch.equal: logits, loss buffer, gradients, which .grad is None, x.grad, BatchNorm buffers, num_batches_tracked and the parameters.
No tolerance: both sides launch the same kernels on the same bits, so any difference is state that leaked from the veteran's past.

Nothing here touches the GPU at import; tests/test_engine_history_cpu.py checks the tables, tests/test_vk_unet_history_gpu.py runs them.

The one place where the twin is not plan-less: an eval forward that a TRAINING plan of the veteran serves.  csrc/engine.hip run_conv
sends a 3x3 layer to vk_conv_fwd_splitk iff `!training && h->splitk_bytes`, and layout_workspace gives splitk_bytes to eval plans only
(`!tr && N*S*SW <= 4*512*512`): a fresh eval plan of these small shapes reduces over channel splits, the training plan does not, so the
two routes differ by summation order.  For such a probe the twin creates the same (empty) training plan first (`Side.mirror_plans`)."""
import contextlib
import copy
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple
from unittest import mock

import torch

# ---------------------------------------------------------------------------------------------- shapes, dtypes, operations
A = (2, 64, 64)
B = (1, 96, 64)          # not square: the plan key holds (height, width)
C = (3, 64, 64)
F32, BF16, F16 = "f32", "bf16", "f16"
DTYPES = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
ROUTES = ("default", "multilabel", "multiclass", "seg", "seg_mc", "lovasz")
OPT_KINDS = ("fused", "stock", "groups")
ENC_W, DEC_W, STEM_W = "encoder.layer2.0.conv1.weight", "decoder.blocks.1.conv1.0.weight", "encoder.conv1.weight"


def eval_fwd(shape, dtype):
    """model.eval() forward under torch.no_grad(); the modes are restored after the call"""
    return ("eval_fwd", shape, dtype)


def eval_fwd_grad(shape, dtype):
    """model.eval() forward with grad mode on: lands on a training plan"""
    return ("eval_fwd_grad", shape, dtype)


def autograd_step(shape, dtype, zero=True):
    """forward (under autocast for 16 bit), BCE or CE + vk.DiceLoss on the device, backward()"""
    return ("autograd_step", shape, dtype, zero)


def fused_step(shape, dtype, route="default", zero=True):
    return ("fused_step", shape, dtype, route, zero)


def opt_step(kind):
    return ("opt_step", kind)


def load_state(seed):
    return ("load_state", seed)


def mul_weights():
    """with torch.no_grad(): p.mul_(1.01) on one encoder and one decoder weight"""
    return ("mul_weights",)


def freeze(prefix):
    return ("freeze", prefix)


def unfreeze(prefix):
    return ("unfreeze", prefix)


def bn_mode(prefix, mode):
    return ("bn_mode", prefix, mode)


def want_dx(on):
    return ("want_dx", bool(on))


def per_stage(on):
    return ("per_stage", bool(on))


def baseline(*names):
    """the veteran alone runs these probes; their logits are what `probe(..., differs=True)` must then differ from"""
    return ("baseline", names)


def probe(*names, differs=False):
    return ("probe", names, differs)


OP_NAMES = ("eval_fwd", "eval_fwd_grad", "autograd_step", "fused_step", "opt_step", "load_state", "mul_weights", "freeze", "unfreeze",
            "bn_mode", "want_dx", "per_stage")
MARKERS = ("baseline", "probe")

# what a history operation does to the state (rows of the coverage matrix) and what a probe exercises (its columns)
TRANSITIONS = ("train_plan", "eval_plan", "eval_on_train_plan", "optimizer_write", "state_load", "inplace_write", "freeze", "bn_mode",
               "want_dx", "per_stage", "loss_route", "accumulate")
PROBE_KINDS = ("eval_fwd", "eval_fwd_grad", "fused_step", "autograd_step", "opt_step", "accumulate")


# ---------------------------------------------------------------------------------------------- probes
# name -> operations, run on the veteran and on the twin.  `{r}` in a route is the family's default fused route.
TRAIN_A16, TRAIN_A32, EVAL_B16, EVAL_B32 = "fused A/bf16", "fused A/f32", "eval B/f16", "eval B/f32"
PROBES: Dict[str, Tuple[tuple, ...]] = {
    "train A/bf16": (autograd_step(A, BF16),),
    "eval B/f32": (eval_fwd(B, F32),),
    "eval A/bf16": (eval_fwd(A, BF16),),
    "fused A/f32": (fused_step(A, F32, "{r}"),),
    "eval B/f16": (eval_fwd(B, F16),),
    "fused C/bf16": (fused_step(C, BF16, "{r}"),),
    "eval A/f32": (eval_fwd(A, F32),),
    "fused A/bf16": (fused_step(A, BF16, "{r}"),),
    "autograd A/f32": (autograd_step(A, F32),),
    "evalgrad A/bf16": (eval_fwd_grad(A, BF16),),
    "fused A/f16": (fused_step(A, F16, "{r}"),),
    "step+update fused": (fused_step(A, BF16, "{r}"), opt_step("fused"), eval_fwd(A, BF16)),
    "step+update stock": (autograd_step(A, F32), opt_step("stock"), eval_fwd(A, F32)),
    "step+update groups": (fused_step(A, BF16, "{r}"), opt_step("groups"), eval_fwd(B, F32)),
    "route default": (fused_step(A, BF16, "default"),),
    "route seg": (fused_step(A, BF16, "seg"),),
    "route lovasz": (fused_step(A, BF16, "lovasz"),),
    "route multilabel": (fused_step(A, BF16, "multilabel"),),
    "route multiclass": (fused_step(A, BF16, "multiclass"),),
    "route seg_mc": (fused_step(A, BF16, "seg_mc"),),
    # accumulation: the same launch sequence on both sides, no claim on gA + gB
    "acc same plan": (fused_step(A, BF16, "{r}"), fused_step(A, BF16, "{r}", zero=False)),
    "acc A then C": (fused_step(A, BF16, "{r}"), fused_step(C, BF16, "{r}", zero=False)),
    "acc fused then autograd": (fused_step(A, BF16, "{r}"), autograd_step(A, BF16, zero=False)),
}
SEVEN = ("train A/bf16", "eval B/f32", "eval A/bf16", "fused A/f32", "eval B/f16", "fused C/bf16", "eval A/f32")
ACCUMULATION = ("acc same plan", "acc A then C", "acc fused then autograd")
FOUR_PLANS_TRAIN, FOUR_PLANS_EVAL = (TRAIN_A16, TRAIN_A32), (EVAL_B16, EVAL_B32)
FLAG_PROBES = ("fused A/bf16", "train A/bf16", "fused A/f32", "autograd A/f32", "eval A/bf16")


# ---------------------------------------------------------------------------------------------- families
@dataclass(frozen=True)
class Family:
    name: str
    cls: str                      # attribute path under the package
    kwargs: Tuple[Tuple[str, object], ...]
    route: str                    # what "{r}" stands for: the fused route this family trains with
    full: bool = False            # runs every history (resnet34, binary); the others: plans interleaved and weights change

    @property
    def classes(self):
        return dict(self.kwargs).get("classes", 1)


FAMILIES = {f.name: f for f in (
    Family("resnet34", "Unet", (("encoder_name", "resnet34"), ("classes", 1)), "default", full=True),
    Family("multiclass3", "multiclass.Unet", (("encoder_name", "resnet34"), ("classes", 3)), "multiclass"),
    Family("resnet18", "encoders.Unet", (("encoder_name", "resnet18"), ("classes", 1)), "default"),
    Family("resnet50", "encoders.Unet", (("encoder_name", "resnet50"), ("classes", 1)), "default"),
)}


# ---------------------------------------------------------------------------------------------- histories
@dataclass(frozen=True)
class History:
    name: str
    entries: Tuple[tuple, ...]
    families: Tuple[str, ...] = ("resnet34",)


def _weights_change():
    """plans A/bf16 and A/f32 (training), B/f16 and B/f32 (eval) exist; then each kind of write.  Around a write: the training probes,
    then the eval probes as the baseline; the write; the eval probes first (nothing but the write lies between their two runs — a
    training forward in between would move the running statistics they read), then the training probes, whose train-mode logits do
    not read the running statistics."""
    e = [fused_step(A, BF16, "{r}"), fused_step(A, F32, "{r}"), eval_fwd(B, F16), eval_fwd(B, F32)]
    for write in ([opt_step("fused")], [opt_step("stock")], [opt_step("groups")], [load_state(7)], [mul_weights()]):
        e += [baseline(*FOUR_PLANS_TRAIN, *FOUR_PLANS_EVAL)] + write + [probe(*FOUR_PLANS_EVAL, *FOUR_PLANS_TRAIN, differs=True)]
    return tuple(e)


ALL_FAMILIES = tuple(FAMILIES)
HISTORIES = {h.name: h for h in (
    History("plans interleaved", (
        autograd_step(A, BF16), eval_fwd(B, F32), eval_fwd(A, BF16), fused_step(A, F32, "{r}"), eval_fwd(B, F16),
        fused_step(C, BF16, "{r}"), eval_fwd(A, F32),
        probe(*SEVEN, "fused A/bf16", "evalgrad A/bf16", "fused A/f16"),
        probe(*ACCUMULATION),
        probe("step+update fused", "step+update stock", "step+update groups"),
    ), families=ALL_FAMILIES),
    History("weights change", _weights_change(), families=ALL_FAMILIES),
    History("freeze encoder", (
        fused_step(A, BF16), opt_step("fused"), freeze("encoder."), fused_step(A, BF16), probe(*FLAG_PROBES, "step+update fused"),
        unfreeze("encoder."), fused_step(A, BF16), probe(*FLAG_PROBES),
    )),
    History("freeze single tensors", (
        fused_step(A, BF16), opt_step("stock"), freeze(ENC_W), fused_step(A, BF16), probe(*FLAG_PROBES),
        freeze(STEM_W), fused_step(A, BF16), probe(*FLAG_PROBES, "step+update stock"),
        unfreeze(""), fused_step(A, BF16), probe(*FLAG_PROBES),
    )),
    History("bn modes", (
        fused_step(A, BF16), bn_mode("encoder", "eval"), fused_step(A, BF16), probe(*FLAG_PROBES, "eval B/f32"),
        bn_mode("encoder", "train"), fused_step(A, BF16), probe(*FLAG_PROBES),
    )),
    History("input gradient", (
        want_dx(True), autograd_step(A, BF16), probe(*FLAG_PROBES),
        want_dx(False), autograd_step(A, BF16), probe(*FLAG_PROBES),
        want_dx(True), autograd_step(A, BF16), probe(*FLAG_PROBES),
    )),
    History("per stage", (
        fused_step(A, BF16), per_stage(True), fused_step(A, BF16), probe(*FLAG_PROBES),
        per_stage(False), fused_step(A, BF16), probe(*FLAG_PROBES),
    )),
    History("loss routes", (
        fused_step(A, BF16, "default"), fused_step(A, BF16, "seg"), fused_step(A, BF16, "lovasz"), fused_step(A, BF16, "default"),
        fused_step(A, BF16, "seg"), probe("route default", "route seg", "route lovasz", "train A/bf16"),
    )),
    History("loss routes, 3 classes", (
        fused_step(A, BF16, "multilabel"), fused_step(A, BF16, "multiclass"), fused_step(A, BF16, "seg_mc"),
        fused_step(A, BF16, "multilabel"), probe("route multilabel", "route multiclass", "route seg_mc", "train A/bf16"),
    ), families=("multiclass3",)),
)}


def cases():
    """(family name, history name) of every test case"""
    return [(f, h.name) for h in HISTORIES.values() for f in h.families]


# what must stay covered: transition kind -> probe kinds that follow it in some history (tests/test_engine_history_cpu.py)
REQUIRED = {
    "train_plan": {"eval_fwd", "eval_fwd_grad", "fused_step", "autograd_step", "opt_step", "accumulate"},
    "eval_plan": {"eval_fwd", "fused_step", "autograd_step", "accumulate"},
    "eval_on_train_plan": {"eval_fwd", "fused_step", "autograd_step", "accumulate"},
    "optimizer_write": {"eval_fwd", "fused_step"},
    "state_load": {"eval_fwd", "fused_step"},
    "inplace_write": {"eval_fwd", "fused_step"},
    "freeze": {"eval_fwd", "fused_step", "autograd_step", "opt_step"},
    "bn_mode": {"eval_fwd", "fused_step", "autograd_step"},
    "want_dx": {"eval_fwd", "fused_step", "autograd_step"},
    "per_stage": {"eval_fwd", "fused_step", "autograd_step"},
    "loss_route": {"fused_step", "autograd_step"},
    "accumulate": {"accumulate"},
}


def transitions_of(entries) -> List[set]:
    """per entry, the transition kinds it stands for (empty for markers).  An eval forward is `eval_on_train_plan` when a training plan
    of its (shape, dtype) came earlier in the history, else `eval_plan`."""
    out, train_keys, routes = [], set(), set()
    for e in entries:
        k, t = e[0], set()
        if k in ("autograd_step", "fused_step", "eval_fwd_grad"):
            t.add("train_plan")
            train_keys.add((e[1], e[2]))
            if k == "fused_step":
                if routes and e[3] not in routes:
                    t.add("loss_route")
                routes.add(e[3])
            if k != "eval_fwd_grad" and not e[-1]:
                t.add("accumulate")
        elif k == "eval_fwd":
            t.add("eval_on_train_plan" if (e[1], e[2]) in train_keys else "eval_plan")
        elif k == "opt_step":
            t.add("optimizer_write")
        elif k == "load_state":
            t.add("state_load")
        elif k == "mul_weights":
            t.add("inplace_write")
        elif k in ("freeze", "unfreeze"):
            t.add("freeze")
        elif k in ("bn_mode", "want_dx", "per_stage"):
            t.add(k)
        out.append(t)
    return out


def probe_kinds(name) -> set:
    ops = PROBES[name]
    kinds = {op[0] for op in ops}
    if any(op[0] in ("autograd_step", "fused_step") and not op[-1] for op in ops):
        kinds = {"accumulate"}
    return kinds


def coverage() -> Dict[str, set]:
    """transition kind -> probe kinds that follow it: every probe marker covers the transitions since the start of its history (the
    state they left is still there), and an accumulation probe is itself the `accumulate` transition"""
    cov = {t: set() for t in TRANSITIONS}
    for h in HISTORIES.values():
        seen = set()
        for e, t in zip(h.entries, transitions_of(h.entries)):
            seen |= t
            if e[0] == "probe":
                for name in e[1]:
                    kinds = probe_kinds(name)
                    for s in seen | ({"accumulate"} if kinds == {"accumulate"} else set()):
                        cov[s] |= kinds
    return cov


# ---------------------------------------------------------------------------------------------- inputs
def seed_of(*key) -> int:
    return zlib.crc32(":".join(str(k) for k in key).encode())


def draw_inputs(key, shape, classes, route):
    """(x, y) on the CPU, seeded by `key`: x fp32 [N,3,H,W]; y fp32 {0,1} [N,classes,H,W], or int64 labels [N,H,W], every one valid, for
    the multiclass routes"""
    g = torch.Generator().manual_seed(seed_of(*key))
    N, H, W = shape
    x = torch.randn(N, 3, H, W, generator=g)
    if route in ("multiclass", "seg_mc"):
        return x, torch.randint(0, classes, (N, H, W), generator=g)
    return x, (torch.rand(N, classes, H, W, generator=g) < 0.3).float()


# ---------------------------------------------------------------------------------------------- the harness (needs the GPU to run)
def device():
    return torch.device("cuda:0")


def new_model(vk, family: Family, compute_dtype=torch.float32, init=True):
    cls = vk
    for part in family.cls.split("."):
        cls = getattr(cls, part)
    kw = dict(family.kwargs, encoder_weights=None, compute_dtype=compute_dtype)
    if init:
        return cls(**kw).to(device())
    # a twin: every tensor the default initialisation would draw is overwritten by the strict load_state_dict that follows
    with mock.patch.object(cls, "_default_init", lambda self: None):
        return cls(**kw).to(device())


def warm_state(vk, family: Family, seed=11):
    """State dict of a model whose running statistics have seen data: 25 train-mode forwards without a graph (at the initial
    running_mean = 0 / running_var = 1 an eval forward barely normalises and its 16-bit activations can overflow)."""
    torch.manual_seed(seed)
    m = new_model(vk, family).train()
    with torch.no_grad():
        for k in range(25):
            m(draw_inputs(("warm", family.name, k), A, 1, "default")[0].to(device()))
    torch.cuda.synchronize()
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def other_state(sd, seed):
    """`sd` drawn again from another seed: every float tensor times (1 + 0.02 u), u uniform in [0, 1) (variances stay positive), every
    num_batches_tracked set to a number of its own"""
    g = torch.Generator().manual_seed(seed_of("state", seed))
    out = {}
    for i, (k, v) in enumerate(sd.items()):
        if v.dtype == torch.int64:
            out[k] = torch.full_like(v, 100 + seed + i)
        else:
            out[k] = v * (1.0 + 0.02 * torch.rand(v.shape, generator=g).to(v.device))
    return out


class Side:
    """One model with what the operations need around it: optimizers by kind, the want_dx flag, what the last operation produced."""

    def __init__(self, vk, family: Family, model, warm):
        self.vk, self.family, self.model, self.warm = vk, family, model, warm
        self.opts: Dict[str, torch.optim.Optimizer] = {}
        self.want_dx = False
        self.logits = self.loss = self.xgrad = None
        self._losses = {}

    # ------------------------------------------------------------------ pieces
    def optimizer(self, kind):
        if kind not in self.opts:
            vk, m = self.vk, self.model
            if kind == "fused":
                self.opts[kind] = vk.adamw_for(m, lr=1e-3, weight_decay=1e-4)
            elif kind == "stock":
                self.opts[kind] = torch.optim.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
            else:
                self.opts[kind] = vk.adamw_for(m, lr=1e-3, groups=vk.finetune_groups(m, lr=1e-3, encoder_lr_scale=0.1))
                assert len(self.opts[kind].param_groups) == 2
        return self.opts[kind]

    def loss_object(self, route):
        if route not in self._losses:
            Ls, Lv = self.vk.seglosses, self.vk.lovasz
            self._losses[route] = {
                "seg": lambda: 0.5 * Ls.FocalLoss("binary", alpha=0.25) + Ls.TverskyLoss("binary", alpha=0.3, beta=0.7),
                "lovasz": lambda: Ls.BCEWithLogitsLoss() + 0.5 * Lv.LovaszLoss("binary"),
                "seg_mc": lambda: Ls.CrossEntropyLoss() + Ls.DiceLoss("multiclass"),
            }[route]()
        return self._losses[route]

    def route_buffers(self, plan) -> Dict[str, torch.Tensor]:
        """the result buffers of the three fused loss routes that exist on `plan`"""
        out = {"mode": plan.loss_out}
        if plan._seg_out is not None:
            out["seg"] = plan._seg_out
        if plan._lovasz_out is not None:
            out["lovasz"] = plan._lovasz_out[0]
            out["lovasz picked"] = plan._lovasz_out[2]
        return out

    @contextlib.contextmanager
    def eval_mode(self):
        flags = [(mod, mod.training) for mod in self.model.modules()]
        self.model.eval()
        try:
            yield
        finally:
            for mod, f in flags:
                mod.training = f

    def mirror_plans(self, veteran_model, op):
        """See the module docstring: an eval forward that a training plan of the veteran serves runs on the same kind of plan here."""
        if op[0] != "eval_fwd":
            return False
        (N, H, W), dt = op[1], DTYPES[op[2]]
        S = H if H == W else (H, W)
        if (N, S, dt, True) in veteran_model._plans:
            self.model.plan_for(N, S, dt, True)
            return True
        return False

    # ------------------------------------------------------------------ one operation
    def run(self, op, key, monkeypatch=None):
        """Run `op` with inputs seeded by `key`; returns {route buffer name: (before, after)} of a fused step's plan, else None."""
        m, fam, kind = self.model, self.family, op[0]
        self.xgrad = None
        if kind in ("eval_fwd", "eval_fwd_grad"):
            x = draw_inputs(key, op[1], fam.classes, fam.route)[0].to(device())
            with self.eval_mode(), (torch.no_grad() if kind == "eval_fwd" else torch.enable_grad()), _autocast(op[2]):
                self.logits = m(x).detach()
            self.loss = None
        elif kind == "autograd_step":
            x, y = draw_inputs(key, op[1], fam.classes, fam.route)
            x, y = x.to(device()), y.to(device())
            if self.want_dx:
                x.requires_grad_(True)
            if op[3]:
                m.zero_grad(set_to_none=True)
            with _autocast(op[2]):
                lg = m(x)
            if y.dtype == torch.int64:
                loss = torch.nn.CrossEntropyLoss()(lg, y) + self.vk.multiclass.DiceLoss(mode="multiclass")(lg, y)
            else:
                loss = torch.nn.BCEWithLogitsLoss()(lg, y) + self.vk.DiceLoss(mode="binary")(lg, y)
            loss.backward()
            self.logits, self.loss = lg.detach(), loss.detach().reshape(1)
            self.xgrad = x.grad
        elif kind == "fused_step":
            route = fam.route if op[3] == "{r}" else op[3]
            x, y = draw_inputs(key, op[1], fam.classes, route)
            if op[4]:
                m.zero_grad(set_to_none=True)
            kw = dict(grad_scale=1024.0 if op[2] == F16 else 1.0, dtype=DTYPES[op[2]])
            if route in ("multilabel", "multiclass"):
                kw["mode"] = route
            elif route != "default":
                kw["loss"] = self.loss_object(route)
            N, H, W = op[1]
            plan = m._plans.get((N, H if H == W else (H, W), DTYPES[op[2]], True))
            before = {k: v.clone() for k, v in self.route_buffers(plan).items()} if plan is not None else {}
            out = m.loss_and_backward(x.to(device()), y.to(device()), **kw)
            torch.cuda.synchronize()
            self.logits, self.loss = m.last_logits, out.clone()
            plan = m._plans[(N, H if H == W else (H, W), DTYPES[op[2]], True)]
            after = self.route_buffers(plan)
            return {k: (before[k], after[k].clone()) for k in before}, _route_group(route)
        elif kind == "opt_step":
            self.optimizer(op[1]).step()
        elif kind == "load_state":
            m.load_state_dict(other_state(self.warm, op[1]), strict=True)
        elif kind == "mul_weights":
            params = dict(m.named_parameters())
            with torch.no_grad():
                params[ENC_W].mul_(1.01)
                params[DEC_W].mul_(1.01)
        elif kind in ("freeze", "unfreeze"):
            hit = [p.requires_grad_(kind == "unfreeze") for n, p in m.named_parameters() if n.startswith(op[1])]
            assert hit, op
        elif kind == "bn_mode":
            m.get_submodule(op[1]).train(op[2] == "train")
        elif kind == "want_dx":
            self.want_dx = op[1]
        elif kind == "per_stage":
            if op[1]:
                monkeypatch.setenv("VK_BACKWARD_PER_STAGE", "1")
            else:
                monkeypatch.delenv("VK_BACKWARD_PER_STAGE", raising=False)
        else:
            raise KeyError(op)
        return None

    def observe(self) -> Dict[str, object]:
        torch.cuda.synchronize()
        m = self.model
        none = [p.grad is None for p in m.parameters()]
        grads = m._flat["grads"]
        return {
            "logits": None if self.logits is None else self.logits.clone(),
            "loss": None if self.loss is None else self.loss.clone(),
            "grad is None": none,
            "flat_grads": None if all(none) or grads is None else grads.clone(),
            "x.grad": None if self.xgrad is None else self.xgrad.clone(),
            "bufs": m._flat["bufs"].clone(),
            "nbt": m._flat["nbt"].clone(),
            "flat_params": m.flat_params.clone(),
        }


def _route_group(route):
    return {"seg": "seg", "seg_mc": "seg", "lovasz": "lovasz"}.get(route, "mode")


def _autocast(dtype):
    return torch.autocast("cuda", dtype=DTYPES[dtype]) if dtype != F32 else torch.autocast("cuda", enabled=False)


def twin(veteran: Side, probe_ops=()) -> Side:
    """A fresh model with the veteran's state and flags (module docstring), and fresh optimizers of the kinds `probe_ops` step, loaded
    with the state of the veteran's (a deep copy: FusedAdamW's state dict hands out its moment buffers themselves)."""
    v = veteran.model
    t = new_model(veteran.vk, veteran.family, compute_dtype=v.compute_dtype, init=False)
    t.load_state_dict(v.state_dict(), strict=True)
    for pv, pt in zip(v.parameters(), t.parameters()):
        pt.requires_grad_(pv.requires_grad)
    for mv, mt in zip(v.modules(), t.modules()):
        mt.training = mv.training
    side = Side(veteran.vk, veteran.family, t, veteran.warm)
    side.want_dx = veteran.want_dx
    for op in probe_ops:
        if op[0] == "opt_step" and op[1] in veteran.opts:
            side.optimizer(op[1]).load_state_dict(copy.deepcopy(veteran.opts[op[1]].state_dict()))
    assert not t._plans and t._flat["grads"] is None and all(p.grad is None for p in t.parameters())
    return side


def first_difference(a, b) -> Optional[str]:
    """None when the two observed items are equal (tensors: torch.equal), else where they differ first"""
    if a is None or b is None or isinstance(a, list):
        return None if a == b else "veteran %s, twin %s" % (_short(a), _short(b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return "veteran %s %s, twin %s %s" % (a.dtype, tuple(a.shape), b.dtype, tuple(b.shape))
    if torch.equal(a, b):
        return None
    ne = (a != b).flatten()
    i = int(ne.nonzero()[0])
    return "element %d of %d (%d differ): veteran %r, twin %r" % (i, ne.numel(), int(ne.sum()), a.flatten()[i].item(), b.flatten()[i].item())


def _short(v):
    if isinstance(v, list):
        return "[%d of %d None]" % (sum(v), len(v))
    return "None" if v is None else "a tensor %s" % (tuple(v.shape),)


def assert_finite(obs, where):
    for k, v in obs.items():
        if isinstance(v, torch.Tensor) and v.is_floating_point():
            assert torch.isfinite(v).all(), "%s: %s is not finite" % (where, k)


def assert_equal(obs_v, obs_t, where):
    assert_finite(obs_v, where + " (veteran)")
    assert_finite(obs_t, where + " (twin)")
    assert list(obs_v) == list(obs_t)
    for k in obs_v:
        d = first_difference(obs_v[k], obs_t[k])
        assert d is None, "%s: %s differs: %s" % (where, k, d)


@dataclass
class Report:
    probes: int = 0
    mirrored: List[str] = field(default_factory=list)     # eval probes that ran on a training plan on both sides
    baselines: Dict[str, torch.Tensor] = field(default_factory=dict)


def run_probe(veteran: Side, hname, last_index, pname, monkeypatch, report: Report, on_eval_f32=None):
    """Twin first (it copies the veteran's state as the history left it), then the probe on both; equality after every operation of
    the probe.  Returns the veteran's logits after the probe's first operation."""
    ops = PROBES[pname]
    t = twin(veteran, ops)
    veteran.model.zero_grad(set_to_none=True)
    first = None
    for k, op in enumerate(ops):
        key = (hname, "probe", pname, k)
        where = "history %r, after operation #%d %r: probe %r, operation %d %r" % (
            hname, last_index, _entry(veteran, hname, last_index), pname, k, op)
        if t.mirror_plans(veteran.model, op):
            report.mirrored.append(pname)
        veteran.run(op, key, monkeypatch)
        t.run(op, key, monkeypatch)
        ov, ot = veteran.observe(), t.observe()
        assert_equal(ov, ot, where)
        if first is None:
            first = ov["logits"]
        if on_eval_f32 is not None and op[0] == "eval_fwd" and op[2] == F32:
            on_eval_f32(t, draw_inputs(key, op[1], veteran.family.classes, veteran.family.route)[0], ot["logits"])
    report.probes += 1
    return first


def _entry(side, hname, index):
    return HISTORIES[hname].entries[index] if index >= 0 else None


def run_history(vk, family: Family, hname, warm, monkeypatch, on_eval_f32=None) -> Tuple[Side, Report]:
    """The veteran lives through `hname`; every probe marker runs its probes.  A fused step of the history also checks that the result
    buffers of the other loss routes of its plan are left alone."""
    h = HISTORIES[hname]
    m = new_model(vk, family, init=False)
    m.load_state_dict(warm, strict=True)
    m.train()
    veteran, report = Side(vk, family, m, warm), Report()
    last = -1
    for i, e in enumerate(h.entries):
        if e[0] == "baseline":
            for pname in e[1]:              # (no zero_grad of its own: the write that follows may be an optimizer's and needs the gradients)
                for k, op in enumerate(PROBES[pname]):
                    veteran.run(op, (hname, "probe", pname, k), monkeypatch)
                    if k == 0:
                        report.baselines[pname] = veteran.observe()["logits"]
        elif e[0] == "probe":
            for pname in e[1]:
                logits = run_probe(veteran, hname, last, pname, monkeypatch, report, on_eval_f32)
                if e[2]:
                    assert not torch.equal(logits, report.baselines[pname]), (
                        "history %r: the write #%d %r left the logits of probe %r as they were" % (hname, last, h.entries[last], pname))
        else:
            res = veteran.run(e, (hname, i), monkeypatch)
            last = i
            if res is not None:
                bufs, group = res
                for name, (before, after) in bufs.items():
                    if not name.startswith(group):
                        assert torch.equal(before, after), (
                            "history %r, operation #%d %r: the result buffer %r of another loss route changed" % (hname, i, e, name))
    return veteran, report
