"""Fine-tuning with frozen parameters, the parts that need no GPU: the engine's trainable-mask entry point on a host-only handle, the
host side of the segmented AdamW (block table), the gradient reducer with frozen buckets (gloo, world 2) and FusedAdamW over frozen or
partial parameter sets."""
import ctypes as C
import importlib
import os
import socket
import sys
from pathlib import Path

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parents[1]


def _handle(vk, training=1):
    L = vk.lib()
    cfg = vk._lib.vk_unet_config(2, 64, vk._lib.VK_BF16, training)
    h = C.c_void_p()
    vk._lib.check(L.vk_unet_create(C.byref(cfg), C.byref(h)))
    return L, h


def test_set_trainable_takes_one_flag_per_parameter_tensor(vk):
    L, h = _handle(vk)
    try:
        n = sum(1 for i in range(L.vk_unet_num_tensors(h)) if _info(vk, L, h, i).kind in (0, 1))
        assert n == 140
        for flags in ([1] * 140, [0] * 140, [i % 3 == 0 for i in range(140)], [1] * 140):
            arr = (C.c_uint8 * 140)(*flags)
            assert L.vk_unet_set_trainable(h, arr, 140) == 0
        for bad in (139, 141, 0):
            arr = (C.c_uint8 * max(bad, 1))()
            assert L.vk_unet_set_trainable(h, arr, bad) == -1          # VK_ERR_ARG
            assert b"parameter tensors" in L.vk_last_error_string()
        assert L.vk_unet_set_trainable(h, None, 140) == -1
    finally:
        L.vk_unet_destroy(h)
    L, h = _handle(vk, training=0)            # an inference plan takes the flags too (they only act on backward)
    try:
        assert L.vk_unet_set_trainable(h, (C.c_uint8 * 140)(*([0] * 140)), 140) == 0
    finally:
        L.vk_unet_destroy(h)


def _info(vk, L, h, i):
    ti = vk._lib.vk_tensor_info()
    vk._lib.check(L.vk_unet_tensor_info(h, i, C.byref(ti)))
    return ti


def test_adamw_segment_block_table(vk):
    """One row per chunk of VK_ADAMW_SEGMENT_CHUNK elements of every segment, in segment order; bad segments are refused."""
    L = vk.lib()
    chunk = 4096
    seg = torch.tensor([[0, 1, 0], [100, 100 + chunk, 3], [9000, 9000 + 2 * chunk + 5, 7], [50000, 50003, 139]], dtype=torch.int64)
    sp = C.cast(seg.data_ptr(), C.POINTER(C.c_int64))
    n = L.vk_adamw_segment_blocks(4, sp, None, 0)
    assert n == 1 + 1 + 3 + 1
    blocks = torch.full((n, 2), -1, dtype=torch.int32)
    assert L.vk_adamw_segment_blocks(4, sp, C.cast(blocks.data_ptr(), C.POINTER(C.c_int32)), n) == n
    assert blocks.tolist() == [[0, 0], [1, 0], [2, 0], [2, 1], [2, 2], [3, 0]]
    assert L.vk_adamw_segment_blocks(4, sp, C.cast(blocks.data_ptr(), C.POINTER(C.c_int32)), n - 1) == -1     # does not fit
    bad = torch.tensor([[10, 10, 0]], dtype=torch.int64)                                                      # empty segment
    assert L.vk_adamw_segment_blocks(1, C.cast(bad.data_ptr(), C.POINTER(C.c_int64)), None, 0) == -1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    sys.path.insert(0, str(ROOT))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    vk = importlib.import_module("vickers-hardness-unet_amd")
    # ten buckets handed over tail-first like the engine's stages; rank-dependent values
    n = 5000
    cuts = [0, 40, 900, 1500, 2100, 2600, 3100, 3900, 4500, 4800, n]
    ranges = list(zip(cuts[:-1], cuts[1:]))[::-1]
    g = torch.Generator().manual_seed(1000 + rank)
    local = torch.randn(n, generator=g, dtype=torch.float64).float()
    gathered = [torch.zeros_like(local) for _ in range(world)]
    dist.all_gather(gathered, local)
    mean = torch.stack(gathered).mean(0)
    out = {}
    for frozen in ({3, 4, 5, 6, 7, 8}, {0, 9}, {8}, set()):
        for pol in ("eager", "deferred", "tail"):
            fp = local.clone()
            red = vk.GradientReducer(lambda fp=fp: fp, world_size=world, scale_grads=True, policy=pol, defer_until=9)
            counts = []
            for i, rg in enumerate(ranges):
                if i in frozen:
                    red.bucket_ready(i, rg, trainable=False)
                else:
                    red.bucket_ready(i, rg)
                counts.append(len(red._handles))
            issued = list(red._ranges)
            red.finish()
            ok = not red.in_flight
            for i, (b0, b1) in enumerate(ranges):
                want = local[b0:b1] if i in frozen else mean[b0:b1]
                ok = ok and torch.allclose(fp[b0:b1], want, rtol=1e-6, atol=1e-7)
                if i in frozen:
                    ok = ok and torch.equal(fp[b0:b1], local[b0:b1])          # never touched: stays rank-local, bit for bit
            # no collective covers a frozen bucket
            for a0, a1 in issued:
                ok = ok and not any(a0 < ranges[i][1] and ranges[i][0] < a1 for i in frozen)
            out[(tuple(sorted(frozen)), pol)] = (bool(ok), counts)
    q.put((rank, out))
    dist.destroy_process_group()


def test_gradient_reducer_gloo_world2_frozen_buckets():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for rank, out in res:
        for key, (ok, _) in out.items():
            assert ok, (rank, key)
        enc = (3, 4, 5, 6, 7, 8)
        # encoder frozen: "deferred" still flushes buckets 0-2 (one collective) when stage 8 — a frozen one — is done, bucket 9 after it
        assert out[(enc, "deferred")][1] == [0] * 8 + [1, 2]
        assert out[(enc, "eager")][1] == [1, 2, 3, 3, 3, 3, 3, 3, 3, 4]
        assert out[(enc, "tail")][1] == [0] * 10
        assert out[((8,), "deferred")][1] == [0] * 8 + [1, 2]
        assert out[((0, 9), "deferred")][1] == [0] * 8 + [1, 1]
        assert out[((), "deferred")][1] == [0] * 8 + [1, 2]


def test_fused_adamw_accepts_frozen_and_partial_parameter_sets(vk):
    m = vk.Unet(encoder_weights=None)
    m.encoder.requires_grad_(False)
    trainable = [p for p in m.parameters() if p.requires_grad]
    assert 0 < len(trainable) < 140
    opt = vk.FusedAdamW((p for p in m.parameters() if p.requires_grad), lr=1e-3, weight_decay=1e-4).attach(m)
    assert len(opt.param_groups[0]["params"]) == len(trainable)
    opt2 = vk.FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4).attach(m)      # frozen tensors in the group are fine
    assert len(opt2.param_groups[0]["params"]) == 140
    vk.adamw_for(m, lr=1e-3)
    other = vk.Unet(encoder_weights=None)
    with pytest.raises(vk.VkError):
        vk.FusedAdamW(list(trainable) + [next(other.parameters())], lr=1e-3).attach(m)
    with pytest.raises(vk.VkError):
        vk.FusedAdamW(other.parameters(), lr=1e-3).attach(m)


def test_fused_adamw_state_dict_per_tensor_steps(vk):
    """Per-tensor step counts round-trip through the state dict; the one-counter format still loads as "every tensor at `step`"."""
    m = vk.Unet(encoder_weights=None)
    opt = vk.adamw_for(m, lr=1e-3)
    n = m.flat_params.numel()
    sd = opt.state_dict()
    steps = [0] * 110 + [3] * 30
    sd["fused"] = {"step": 3, "exp_avg": torch.zeros(n), "exp_avg_sq": torch.zeros(n), "steps": steps}
    opt2 = vk.adamw_for(m, lr=1e-3)
    opt2.load_state_dict(sd)
    assert opt2.tensor_steps() == steps and opt2.step_count == 3
    assert opt2.state_dict()["fused"]["steps"] == steps
    sd["fused"] = {"step": 7, "exp_avg": torch.zeros(n), "exp_avg_sq": torch.zeros(n)}
    opt2.load_state_dict(sd)
    assert opt2.tensor_steps() == [7] * 140 and opt2.step_count == 7
    assert "steps" not in opt2.state_dict()["fused"]
