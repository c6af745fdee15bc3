"""CPU: the host side of the stage-3 batch maker (mmsr/data/ref_pairs.py) and of the one-launch resampler under it
(c2m_amd.ops.pil_bicubic_resize2d_u8): the augment draws, the validation geometry, the window / LDS plan the wrapper
chooses the kernel by, the argument checks and the ABI declaration."""
import os
import random
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hand_flags(rng, n, use_flip, use_rot):
    out = []
    for _ in range(n):
        f = 0
        if use_flip:
            f |= 1 if rng.random() < 0.5 else 0
        if use_rot:
            f |= 2 if rng.random() < 0.5 else 0
            f |= 4 if rng.random() < 0.5 else 0
        out.append(f)
    return out


@pytest.mark.parametrize("use_flip,use_rot,draws", [(True, True, 3), (True, False, 1), (False, True, 2), (False, False, 0)])
def test_flags_follow_the_reference_draw_order_and_gating(use_flip, use_rot, draws):
    from mmsr.data.ref_pairs import draw_flags
    a, hand = random.Random(17), random.Random(17)
    flags = draw_flags(a, 9, use_flip, use_rot)
    assert flags == _hand_flags(hand, 9, use_flip, use_rot)
    assert a.getstate() == hand.getstate()
    counted = random.Random(17)
    for _ in range(9 * draws):
        counted.random()
    assert a.getstate() == counted.getstate()              # exactly `draws` draws per sample, none with both switches off
    allowed = (1 if use_flip else 0) | (6 if use_rot else 0)
    assert all(f & ~allowed == 0 for f in flags)
    if draws == 3:
        assert {f & 1 for f in flags} == {0, 1} and {f & 2 for f in flags} == {0, 2} and {f & 4 for f in flags} == {0, 4}


def test_generator_owns_its_random_stream():
    from mmsr.data.ref_pairs import RefPairGenerator, draw_flags
    random.seed(5)
    before = random.getstate()
    g1, g2 = RefPairGenerator(seed=3), RefPairGenerator(seed=3)
    assert draw_flags(g1.flip_rng, 6) == draw_flags(g2.flip_rng, 6)
    assert random.getstate() == before                     # the global generator is neither read nor reseeded
    assert (g1.phase, g1.gt_size, g1.scale, g1.use_flip, g1.use_rot) == ("train", 160, 4, True, True)


@pytest.mark.parametrize("in_hw,ref_hw,scale,want", [
    ((43, 58), (50, 47), 4, ((40, 56), (48, 44), (48, 56), True)),
    ((40, 56), (40, 56), 4, ((40, 56), (40, 56), (40, 56), False)),
    ((41, 59), (43, 57), 4, ((40, 56), (40, 56), (40, 56), False)),     # equal after the mod-crop: no padding
    ((64, 48), (32, 96), 4, ((64, 48), (32, 96), (64, 96), True)),
    ((33, 35), (31, 31), 2, ((32, 34), (30, 30), (32, 34), True)),
    ((9, 9), (7, 5), 3, ((9, 9), (6, 3), (9, 9), True)),
])
def test_validation_geometry(in_hw, ref_hw, scale, want):
    from mmsr.data.ref_pairs import val_geometry
    assert val_geometry(in_hw, ref_hw, scale) == want
    assert val_geometry(torch.Size(in_hw), torch.Size(ref_hw), scale) == want


def test_validation_geometry_rejects_an_image_below_one_cell():
    from mmsr.data.ref_pairs import val_geometry
    with pytest.raises(ValueError):
        val_geometry((3, 40), (40, 40), 4)


def test_generator_checks_its_arguments():
    import c2m_amd
    from mmsr.data.ref_pairs import RefPairGenerator
    with pytest.raises(ValueError):
        RefPairGenerator(phase="test")
    with pytest.raises(ValueError):
        RefPairGenerator(gt_size=162, scale=4)
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)     # noqa: E731
    gen = RefPairGenerator(gt_size=16, seed=0)
    with pytest.raises(TypeError):
        gen(torch.zeros(2, 3, 16, 16), u8(2, 3, 16, 16))
    with pytest.raises(TypeError):
        gen(u8(2, 3, 16, 16), [u8(3, 16, 16), u8(16, 16)])
    with pytest.raises(TypeError):
        gen(u8(2, 1, 16, 16), u8(2, 3, 16, 16))
    with pytest.raises(ValueError):
        gen(u8(2, 3, 16, 20), u8(2, 3, 16, 16))            # not gt_size x gt_size
    with pytest.raises(ValueError):
        gen(u8(2, 3, 16, 16), [u8(3, 16, 16)])             # one Ref for two inputs
    with pytest.raises(c2m_amd.C2MError):                  # host tensors: there is no CPU path to fall back to
        gen(u8(2, 3, 16, 16), u8(2, 3, 20, 24))
    val = RefPairGenerator(phase="val")
    with pytest.raises(TypeError):
        val(u8(1, 3, 16, 16), u8(3, 16, 16))
    with pytest.raises(ValueError):
        val(u8(3, 2, 16), u8(3, 16, 16))


def test_operator_rejects_cpu_tensors_and_bad_flags():
    import c2m_amd
    from c2m_amd import ops
    with pytest.raises(c2m_amd.C2MError):
        ops.pil_bicubic_resize2d_u8(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), 2, 2)
    assert ops._pil2d_flags(None, 3) is None
    assert ops._pil2d_flags([0, 7, 2], 3) == [0, 7, 2]
    assert ops._pil2d_flags(torch.tensor([1, 4], dtype=torch.uint8), 2) == [1, 4]
    for bad, n in (([0, 1], 3), ([8], 1), ([-1], 1), (5, 1), (["a"], 1)):
        with pytest.raises(c2m_amd.C2MError):
            ops._pil2d_flags(bad, n)
    assert (ops.PIL2D_FLIP_H, ops.PIL2D_FLIP_V, ops.PIL2D_TRANSPOSE) == (1, 2, 4)


def _hand_window(n_in, n_out, tile):
    from c2m_amd import ops
    start, count, _ = ops.pil_bicubic_tables(n_in, n_out)
    best = 0
    for t0 in range(0, n_out, tile):
        rows = range(t0, min(t0 + tile, n_out))
        best = max(best, max(int(start[i] + count[i]) for i in rows) - min(int(start[i]) for i in rows))
    return best


def test_plan_states_the_window_and_the_fallback_rule():
    """The wrapper takes the one-launch kernel exactly when one workgroup's LDS (tables' tiles + source window + the
    horizontally resampled window) fits the budget; the constants are the header's."""
    from c2m_amd import ops
    hdr = open(os.path.join(REPO, "include", "c2m_hip.h")).read()
    assert int(re.search(r"#define C2M_PIL2D_TILE (\d+)", hdr).group(1)) == ops._PIL2D_TILE == 32
    assert int(re.search(r"#define C2M_PIL2D_LDS_BUDGET (\d+)", hdr).group(1)) == ops._PIL2D_LDS_BUDGET
    down, up = ops.pil_bicubic2d_plan(160, 160, 40, 40), ops.pil_bicubic2d_plan(40, 40, 160, 160)
    assert down.fused and up.fused
    assert (down.win_h, down.win_w) == (_hand_window(160, 40, 32),) * 2 and down.Kh == down.Kv == 16
    assert 32 * 4 <= down.win_h <= 32 * 4 + 2 * 8           # 32 output pixels x ratio 4 + the support of 2 x 4 per side
    assert (up.win_h, up.win_w) == (_hand_window(40, 160, 32),) * 2 and up.win_h <= 8 + 4
    mixed = ops.pil_bicubic2d_plan(50, 30, 17, 61)
    assert (mixed.win_h, mixed.win_w) == (_hand_window(50, 17, 32), _hand_window(30, 61, 32))
    # bytes: 4 x 32 starts / counts, 32 rows of each table at an odd pitch, the two uint8 windows (pitches: win_w to 4; 40)
    for p in (down, up, mixed):
        want = 4 * (4 * 32 + 32 * (p.Kh | 1) + 32 * (p.Kv | 1)) + p.win_h * ((p.win_w + 3) // 4 * 4) + p.win_h * 40
        assert p.lds_bytes == want
    big = ops.pil_bicubic2d_plan(400, 400, 10, 10)
    assert not big.fused and big.lds_bytes > ops._PIL2D_LDS_BUDGET and (big.win_h, big.win_w) == (400, 400)
    tall = ops.pil_bicubic2d_plan(400, 40, 10, 10)         # 160 taps on one axis alone: above the 48 KiB default, in budget
    assert tall.fused and 48 * 1024 < tall.lds_bytes <= 64 * 1024 and not ops.pil_bicubic2d_plan(400, 100, 10, 25).fused
    assert ops.pil_bicubic2d_plan(50, 30, 50, 30).fused     # no axis changes: identity tables, a 32-pixel window


def test_new_entry_points_are_declared_and_exported():
    import c2m_amd
    from c2m_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "c2m_hip.h")).read(), flags=re.S)
    m = re.search(r"int c2m_pil_bicubic2d_u8\((.*?)\);", hdr, flags=re.S)
    assert m and re.search(r"size_t c2m_pil_bicubic2d_lds_bytes\(", hdr)
    L = c2m_amd.lib()
    assert len(L.c2m_pil_bicubic2d_u8.argtypes) == len(m.group(1).split(",")) == 22
    assert L.c2m_pil_bicubic2d_lds_bytes(0, 4, 4, 4) == 0 and L.c2m_abi_version() == _lib.ABI_VERSION
    assert "ref_pairs.hip" in open(os.path.join(REPO, "c2-matching_amd", "csrc", "Makefile")).read()
