"""tests/bwd_onepass_up_cases.py without a GPU: every case of the exact tier of tests/test_up_bwd_onepass_gpu.py meets the exactness
conditions on its float64 reference alone (none skipped), and the reference is sensitive to the faults the tier is there to catch."""
import pytest
import torch
import torch.nn.functional as F

import bwd_onepass_up_cases as UC

CASES = UC.cases()


@pytest.mark.parametrize("case", CASES, ids=[UC.case_id(c) for c in CASES])
def test_case_is_exact_in_both_types(case):
    b = UC.build(case)
    fig = UC.check(b)
    print({k: round(v, 2) for k, v in fig.items()})
    assert fig["max_dz"] <= 8.0 and fig["max_Vs"] <= 7.0
    # not degenerate: the mask keeps and drops pixels, every coefficient class occurs, the constant c is there to leak
    keep = (b.y != 0).double().mean().item()
    assert 0.2 < keep < 0.9
    assert set(b.coef[0].tolist()) == {0.5, 1.0, 2.0} and set(b.coef[1].tolist()) == {-0.5, 0.0, 0.5} and (b.coef[2] != 0).any()
    assert b.dw.abs().max().item() > 0 and (b.wf != 0).double().mean().item() > 0.03
    assert b.y.shape == (b.N, 32, b.H // 2, b.W // 2) and b.dw.shape == (16, 32, 3, 3)


def test_reference_sees_a_leaked_constant_a_wrong_source_pixel_and_a_wrong_channel():
    """dz = c in the padding ring instead of 0 changes the pooled gradient on the border; V read at the neighbouring source pixel changes
    dw; coefficients shifted by 8 channels change dz."""
    b = UC.build(CASES[0])
    dzp = F.pad(b.dz, (1, 1, 1, 1))
    ring = torch.ones_like(dzp)
    ring[:, :, 1:-1, 1:-1] = 0
    leaked = dzp + ring * b.coef[2].view(1, -1, 1, 1)
    xin = torch.zeros(b.N, 32, b.H + 2, b.W + 2, dtype=torch.float64, requires_grad=True)
    F.conv2d(xin, b.wf, padding=1).backward(leaked)
    assert not torch.equal(F.avg_pool2d(xin.grad[:, :, 1:-1, 1:-1], 2) * 4.0, b.pooled)
    shifted = F.interpolate(b.Vs.roll(1, dims=3), scale_factor=2, mode="nearest")
    wv = torch.zeros(16, 32, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(shifted, wv, padding=1).backward(b.dz)
    assert not torch.equal(wv.grad, b.dw)
    rolled = b.coef.roll(8, dims=1)
    dz2 = rolled[0].view(1, -1, 1, 1) * b.g + rolled[1].view(1, -1, 1, 1) * b.z + rolled[2].view(1, -1, 1, 1)
    assert not torch.equal(dz2, b.dz)
