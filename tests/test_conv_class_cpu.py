"""The two class predicates of the convolution host layer answer what they answered before they were rewritten on top of
halo_class() / wh64_class(): vk_conv_uses_halo_pack and vk_conv_wgrad_batch_supports over the descriptor table of
conv_class_cases.py, once per diagnostic switch.  Host-only (no GPU): the library is loaded, nothing is launched.  The expected
answers are literals recorded from the earlier library, so the same file passes against that library through VK_LIB."""
import pytest

import conv_class_cases as cc


@pytest.fixture()
def clean_env(monkeypatch):
    for s in cc.SWITCHES:
        monkeypatch.delenv(s, raising=False)
    return monkeypatch


def test_table_covers_every_environment():
    assert set(cc.EXPECTED) == set(cc.ENVS)
    assert all(len(row) == len(cc.CASES) and set(row) <= set("0123") for row in cc.EXPECTED.values())
    # the default row holds every class: neither, pack only, pack and batch; a switch moves some rows and not all
    assert {"0", "2", "3"} <= set(cc.EXPECTED[""])
    for env in cc.ENVS[1:]:
        assert cc.EXPECTED[env] != cc.EXPECTED[""], env


@pytest.mark.parametrize("env", cc.ENVS, ids=[e or "default" for e in cc.ENVS])
def test_predicates_equal_recorded_answers(vk, clean_env, env):
    L = vk.lib()
    if env:
        name, value = env.split("=")
        clean_env.setenv(name, value)
    got = cc.evaluate(L, vk._lib.vk_conv_desc, vk._lib.vk_src)
    want = cc.EXPECTED[env]
    bad = [(i, cc.CASES[i], want[i], got[i]) for i in range(len(want)) if want[i] != got[i]]
    assert not bad, f"{len(bad)} of {len(want)} descriptors differ under {env or 'no switch'}; first: {bad[0]}"


def test_null_descriptor(vk):
    L = vk.lib()
    assert L.vk_conv_uses_halo_pack(None) == 0
    assert L.vk_conv_wgrad_batch_supports(None) == 0
