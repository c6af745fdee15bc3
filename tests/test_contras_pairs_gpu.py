"""GPU: the stage 1-2 pair generator's kernels (csrc/contras_pairs.hip) and the generator built on them.

The resampler is integer arithmetic: equality with mmsr.data.pil_bicubic.pil_bicubic_resize on the CPU and with Pillow's
own results (tests/golden/contras_pairs_pillow.npz) is the bound.  The warp is checked against a float64 restatement of
its rule written below; parity with OpenCV is unpinned."""
import os
import random

import numpy as np
import pytest
import torch

import make_golden_contras_pairs as mgp

pytestmark = pytest.mark.gpu

COORD_SEEDS = (0, 1, 3, 5)     # homography draws whose sampled coordinates keep the margin asserted in _coord_margin


def _batch(name, B):
    return torch.from_numpy(np.stack([mgp.image(name, b) for b in range(B)]))


def _f32_of(u8):
    """uint8 / 255 as the reference forms it: an IEEE float32 division (numpy), not a multiplication by 1/255."""
    a = u8.cpu().numpy() if isinstance(u8, torch.Tensor) else u8
    return a.astype(np.float32) / np.float32(255)


# ---- resampler ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B", [("c52", 3), ("c160", 4)])
def test_resampler_down_and_back_is_bit_exact(dev, golden_dir, name, B):
    from c2m_amd import ops
    from mmsr.data.pil_bicubic import pil_bicubic_resize
    g = np.load(os.path.join(golden_dir, "contras_pairs_pillow.npz"))
    img = _batch(name, B)
    H, W = img.shape[-2:]
    lq = ops.pil_bicubic_resize_u8(img.to(dev), H // 4, W // 4)
    assert lq.dtype == torch.uint8 and tuple(lq.shape) == (B, 3, H // 4, W // 4)
    want_lq = pil_bicubic_resize(img, H // 4, W // 4)
    assert torch.equal(lq.cpu(), want_lq)
    assert np.array_equal(lq[0].cpu().numpy(), g[f"{name}/lq"])
    up, up_f = ops.pil_bicubic_resize_u8(lq, H, W, as_float=True)
    assert torch.equal(up.cpu(), pil_bicubic_resize(want_lq, H, W))
    assert np.array_equal(up[0].cpu().numpy(), g[f"{name}/up"])
    assert up_f.dtype == torch.float32 and np.array_equal(up_f.cpu().numpy(), _f32_of(up))
    lq2, lq_f = ops.pil_bicubic_resize_u8(img.to(dev), H // 4, W // 4, as_float=True)
    assert torch.equal(lq2, lq) and np.array_equal(lq_f.cpu().numpy(), _f32_of(lq))


def test_resampler_non_integer_ratio_and_single_axes(dev, golden_dir):
    from c2m_amd import ops
    from mmsr.data.pil_bicubic import pil_bicubic_resize
    g = np.load(os.path.join(golden_dir, "contras_pairs_pillow.npz"))
    img = torch.from_numpy(mgp.image("c50"))                                   # [3,50,30]: no batch dimension
    odd = ops.pil_bicubic_resize_u8(img.to(dev), 17, 11)
    assert np.array_equal(odd.cpu().numpy(), g["c50/odd"]) and torch.equal(odd.cpu(), pil_bicubic_resize(img, 17, 11))
    b = _batch("c50", 2)
    for oh, ow in ((50, 11), (17, 30), (50, 30), (61, 43), (200, 120)):       # one axis, none, odd up-sampling, x4
        got, got_f = ops.pil_bicubic_resize_u8(b.to(dev), oh, ow, as_float=True)
        assert torch.equal(got.cpu(), pil_bicubic_resize(b, oh, ow)), (oh, ow)
        assert np.array_equal(got_f.cpu().numpy(), _f32_of(got)), (oh, ow)
    same = ops.pil_bicubic_resize_u8(b.to(dev), 50, 30)
    assert torch.equal(same.cpu(), b)


def test_resampler_takes_a_non_contiguous_slice_like_its_neighbours(dev):
    """The neighbouring operators make a non-contiguous input contiguous (ops._dev_f32); so does this one."""
    import c2m_amd
    from c2m_amd import ops
    from mmsr.data.pil_bicubic import pil_bicubic_resize
    big = _batch("c52", 4)
    sl = big.to(dev)[::2, :, :, 4:36]                                           # batch stride 2, a column window
    assert not sl.is_contiguous()
    got = ops.pil_bicubic_resize_u8(sl, 13, 8)
    assert torch.equal(got.cpu(), pil_bicubic_resize(big[::2, :, :, 4:36].contiguous(), 13, 8))
    with pytest.raises(c2m_amd.C2MError):
        ops.pil_bicubic_resize_u8(sl.float(), 13, 8)
    with pytest.raises(c2m_amd.C2MError):
        ops.pil_bicubic_resize_u8(sl, 0, 8)


# ---- warp -----------------------------------------------------------------------------------------------------------

def restate_warp(src, M):
    """float64 restatement of the warp's rule.  src uint8 [B,3,H,W] (numpy), M [B,3,3] -> (dst [B,3,H,W], coords [B,H,W,3]).
    Positions are formed with the operation order of the rule ((m0 x + m1 y) + m2, 32 X / Wd, rint = half to even)."""
    B, _, H, W = src.shape
    Mi = np.linalg.inv(M)
    s = np.zeros((B, 3, H + 2, W + 2), dtype=np.float64)           # one pixel of zero border on every side
    s[:, :, 1:-1, 1:-1] = src.astype(np.float64) / 255.0
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    dst = np.zeros((B, 3, H, W), dtype=np.float64)
    coords = np.zeros((B, H, W, 3), dtype=np.float64)
    for b in range(B):
        m, mi = M[b], Mi[b]
        X, Y, Wd = ((mi[r, 0] * x + mi[r, 1] * y) + mi[r, 2] for r in range(3))
        with np.errstate(divide="ignore", invalid="ignore"):
            sx = np.where(Wd != 0, np.clip(np.rint(32.0 * X / Wd), -2.0 ** 31, 2.0 ** 31 - 1), 0.0).astype(np.int64)
            sy = np.where(Wd != 0, np.clip(np.rint(32.0 * Y / Wd), -2.0 ** 31, 2.0 ** 31 - 1), 0.0).astype(np.int64)
        x0, y0, a, bb = sx >> 5, sy >> 5, (sx & 31) / 32.0, (sy & 31) / 32.0

        def tap(yy, xx):
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            return np.where(inside, s[b][:, np.clip(yy + 1, 0, H + 1), np.clip(xx + 1, 0, W + 1)], 0.0)
        dst[b] = (tap(y0, x0) * (1 - a) * (1 - bb) + tap(y0, x0 + 1) * a * (1 - bb) + tap(y0 + 1, x0) * (1 - a) * bb
                  + tap(y0 + 1, x0 + 1) * a * bb)
        c = [(m[r, 0] * x + m[r, 1] * y) + m[r, 2] for r in range(3)]
        coords[b] = np.stack([c[0] / c[2], c[1] / c[2], c[2] / c[2]], -1)
    return dst, coords


def numpy_coords(M, H, W):
    """The reference's host computation of the transformed coordinates (np.dot with the stacked pixel grid)."""
    gx, gy = np.meshgrid(np.arange(W), np.arange(H))
    grid = np.stack((gx, gy, np.ones(gx.shape)), axis=0).reshape(3, -1)
    t = np.dot(M, grid)
    t /= t[2, :]
    return t.transpose(1, 0).reshape(H, W, 3)


def coords_rel_err(got, M, H, W):
    """Largest error of `got` [B,H,W,3] against numpy_coords, relative to the magnitude of what was summed: a coordinate is
    (m0 x + m1 y + m2) / c2, and where the three terms cancel (a coordinate crossing 0) the rounding of either evaluation
    order is relative to |m0 x| + |m1 y| + |m2|, not to the small sum.  Away from cancellation this is the plain
    relative error."""
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    worst = 0.0
    for b in range(len(M)):
        ref = numpy_coords(M[b], H, W)
        mag = np.stack([np.abs(M[b][r, 0]) * x + np.abs(M[b][r, 1]) * y + np.abs(M[b][r, 2]) for r in range(3)], -1)
        mag = mag / np.abs((M[b][2, 0] * x + M[b][2, 1] * y) + M[b][2, 2])[..., None]
        assert (mag >= np.abs(ref) * (1 - 1e-12)).all()
        err = np.abs(got[b] - ref)
        assert (err[mag == 0] == 0).all()                # nothing was summed there: both evaluations give exactly 0
        worst = max(worst, float((err[mag > 0] / mag[mag > 0]).max()))
    return worst


def _check_warp(dev, src, M, min_outside=None):
    from c2m_amd import ops
    want, want_c = restate_warp(src.numpy(), M)
    f32, u8, coords = ops.warp_perspective_u8(src.to(dev), M)
    assert f32.dtype == torch.float32 and u8.dtype == torch.uint8 and coords.dtype == torch.float64
    assert tuple(f32.shape) == tuple(src.shape) == tuple(u8.shape) and tuple(coords.shape) == (src.shape[0],) + tuple(src.shape[2:]) + (3,)
    err = float(np.abs(f32.cpu().numpy().astype(np.float64) - want).max())
    print(f"warp max abs err vs float64 restatement: {err:.3e}")
    assert err <= 1e-6
    assert torch.equal(u8, (f32 * 255).to(torch.uint8))
    rel = coords_rel_err(coords.cpu().numpy(), M, *src.shape[2:])
    print(f"coords max rel err vs numpy: {rel:.3e}")
    assert rel <= 1e-12
    assert coords_rel_err(want_c, M, *src.shape[2:]) <= 1e-12
    if min_outside is not None:
        frac = float((want.max(1) == 0).mean())
        assert frac >= min_outside, frac
    return f32, u8, coords


def test_warp_identity_is_the_input_bit_for_bit(dev):
    from c2m_amd import ops
    src = torch.from_numpy(np.random.RandomState(1).randint(0, 256, size=(2, 3, 48, 64)).astype(np.uint8))
    f32, u8, coords = ops.warp_perspective_u8(src.to(dev), np.eye(3))          # one matrix for the whole batch
    assert torch.equal(u8.cpu(), src)
    assert np.array_equal(f32.cpu().numpy(), _f32_of(src))
    gx, gy = np.meshgrid(np.arange(64.0), np.arange(48.0))
    grid = np.stack([gx, gy, np.ones_like(gx)], -1)
    assert np.array_equal(coords.cpu().numpy(), np.stack([grid, grid]))
    _check_warp(dev, src, np.stack([np.eye(3)] * 2))


def test_warp_integer_translation_shifts_and_zero_fills(dev):
    src = torch.from_numpy(np.random.RandomState(2).randint(1, 256, size=(2, 3, 48, 64)).astype(np.uint8))
    M = np.array([[1.0, 0.0, 5.0], [0.0, 1.0, -3.0], [0.0, 0.0, 1.0]])
    f32, u8, coords = _check_warp(dev, src, np.stack([M, M]))
    want = np.zeros((2, 3, 48, 64), dtype=np.uint8)
    want[:, :, :45, 5:] = src.numpy()[:, :, 3:, :59]                            # dst(x, y) = src(x - 5, y + 3)
    assert np.array_equal(u8.cpu().numpy(), want)
    assert np.array_equal(f32.cpu().numpy(), _f32_of(want))
    assert np.array_equal(coords.cpu().numpy()[0, 7, 9], np.array([14.0, 4.0, 1.0]))


def test_warp_sheared_homography_on_a_non_square_image(dev):
    src = torch.from_numpy(np.random.RandomState(3).randint(0, 256, size=(2, 3, 48, 64)).astype(np.uint8))
    M = np.array([[[1.02, 0.21, -3.3], [-0.04, 0.97, 2.6], [2.0e-4, -3.0e-4, 1.0]],
                  [[0.93, -0.17, 6.1], [0.08, 1.05, -4.4], [-4.0e-4, 1.0e-4, 1.01]]])
    _check_warp(dev, src, M)


def test_warp_with_odd_width_takes_the_scalar_stores(dev):
    """W % 4 != 0: rows do not start on the 4-pixel boundary the vector stores need; also more than one block."""
    src = torch.from_numpy(np.random.RandomState(4).randint(0, 256, size=(3, 3, 37, 53)).astype(np.uint8))
    M = np.array([[[1.01, 0.1, -2.2], [-0.06, 0.98, 1.7], [1.0e-4, 2.0e-4, 1.0]]] * 3)
    M[1, 0, 2], M[2, 1, 2] = 4.0, -6.5
    _check_warp(dev, src, M)


def test_warp_batch_of_drawn_homographies_at_the_training_size(dev):
    from mmsr.data.contras_pairs import sample_pair_homography
    rs = np.random.RandomState(11)
    M = np.stack([sample_pair_homography(rs)[1] for _ in range(4)])
    _check_warp(dev, _batch("c160", 4), M)


def test_warp_that_sends_a_third_of_the_image_outside(dev):
    src = torch.from_numpy(np.random.RandomState(5).randint(1, 256, size=(1, 3, 48, 64)).astype(np.uint8))
    M = np.array([[[1.0, 0.05, 23.5], [0.02, 1.0, -1.25], [0.0, 1.0e-4, 1.0]]])
    _check_warp(dev, src, M, min_outside=0.3)


def test_warp_checks_its_arguments(dev):
    import c2m_amd
    from c2m_amd import ops
    src = torch.zeros(2, 3, 8, 8, dtype=torch.uint8, device=dev)
    for bad_src, M in ((src.float(), np.eye(3)), (src[:, :2], np.eye(3)), (src, np.zeros((3, 3))), (src, np.eye(4)),
                       (src, np.stack([np.eye(3)] * 3))):
        with pytest.raises(c2m_amd.C2MError):
            ops.warp_perspective_u8(bad_src, M)
    sl = torch.zeros(2, 3, 8, 16, dtype=torch.uint8, device=dev)[..., ::2]     # non-contiguous: made contiguous
    assert ops.warp_perspective_u8(sl, torch.eye(3, dtype=torch.float64))[1].shape == (2, 3, 8, 8)


# ---- coordinates ----------------------------------------------------------------------------------------------------

def _coord_margin(t):
    """Distance of every sampled coordinate from a validity threshold (10, size - 10) and from a rounding half of x / 4."""
    size = 160
    f = t / 4.0
    return min(float(np.abs(t - 10).min()), float(np.abs(t - (size - 10)).min()), 4.0 * float(np.abs(f - np.floor(f) - 0.5).min()))


def test_coordinates_give_the_host_computations_correspondences(dev):
    from c2m_amd import ops
    from mmsr.data.contras_pairs import sample_pair_homography
    M = np.stack([sample_pair_homography(np.random.RandomState(s))[1] for s in COORD_SEEDS])
    host = np.stack([numpy_coords(m, 160, 160) for m in M])
    sampled = host[:, ::4, ::4, :2]
    for b in range(len(M)):
        assert _coord_margin(sampled[b]) >= 1e-6
        x, y = sampled[b, ..., 0], sampled[b, ..., 1]
        assert int(((x > 10) & (x < 150) & (y > 10) & (y < 150)).sum()) >= 128
    _, _, coords = ops.warp_perspective_u8(torch.zeros(len(M), 3, 160, 160, dtype=torch.uint8, device=dev), M)
    rel = coords_rel_err(coords.cpu().numpy(), M, 160, 160)
    assert rel <= 1e-12, rel
    got = ops.contras_correspondences(coords, 40, 40)
    want = ops.contras_correspondences(torch.from_numpy(host).to(dev), 40, 40)
    for k in ("ids", "pos2", "offsets"):
        assert torch.equal(got[k], want[k]), k
    assert got["counts"] == want["counts"] and min(got["counts"]) >= 128


# ---- end to end -----------------------------------------------------------------------------------------------------

KEYS = ("img_in", "img_in_lq", "img_in_up", "img_ref", "img_ref_lq", "img_ref_up", "transformed_coordinate")


def _check_dict(d, B, H, W):
    assert sorted(d) == sorted(KEYS)
    for k in KEYS[:-1]:
        s = (H // 4, W // 4) if k.endswith("_lq") else (H, W)
        assert d[k].dtype == torch.float32 and tuple(d[k].shape) == (B, 3) + s and d[k].is_cuda, k
        assert float(d[k].min()) >= 0.0 and float(d[k].max()) <= 1.0
    tc = d["transformed_coordinate"]
    assert tc.dtype == torch.float64 and tuple(tc.shape) == (B, H, W, 3)


def test_generator_without_flips_is_the_two_operators_composed(dev):
    from c2m_amd import ops
    from mmsr.data.contras_pairs import ContrasPairGenerator, sample_pair_homography
    from mmsr.data.pil_bicubic import make_lq_and_up
    img = _batch("c160", 4)
    rs = np.random.RandomState(31)
    M = np.stack([sample_pair_homography(rs)[1] for _ in range(4)])
    d = ContrasPairGenerator(use_flip=False, use_rot=False, seed=31)(img.to(dev))           # draws the same matrices
    d2 = ContrasPairGenerator(use_flip=False, use_rot=False, seed=77)(img.to(dev), matrices=M)
    _check_dict(d, 4, 160, 160)
    for k in KEYS:
        assert torch.equal(d[k], d2[k]), k
    assert np.array_equal(d["img_in"].cpu().numpy(), _f32_of(img))
    lq, up = make_lq_and_up(img)
    assert np.array_equal(d["img_in_lq"].cpu().numpy(), _f32_of(lq)) and np.array_equal(d["img_in_up"].cpu().numpy(), _f32_of(up))
    f32, u8, coords = ops.warp_perspective_u8(img.to(dev), M)
    assert torch.equal(d["img_ref"], f32) and torch.equal(d["transformed_coordinate"], coords)
    r_lq = ops.pil_bicubic_resize_u8(u8, 40, 40)
    r_up = ops.pil_bicubic_resize_u8(r_lq, 160, 160)
    assert np.array_equal(d["img_ref_lq"].cpu().numpy(), _f32_of(r_lq)) and np.array_equal(d["img_ref_up"].cpu().numpy(), _f32_of(r_up))
    rlq_cpu, rup_cpu = make_lq_and_up(u8.cpu())
    assert torch.equal(r_lq.cpu(), rlq_cpu) and torch.equal(r_up.cpu(), rup_cpu)


def test_generator_with_flips_follows_its_seeded_draws(dev):
    from mmsr.data.contras_pairs import ContrasPairGenerator, sample_pair_homography
    from mmsr.data.pil_bicubic import make_lq_and_up
    img = _batch("c160", 4)
    d = ContrasPairGenerator(seed=6)(img.to(dev))
    _check_dict(d, 4, 160, 160)
    hand, rs = random.Random(6), np.random.RandomState(6)
    aug, flags = [], []
    for b in range(4):
        s = img[b]
        h, v, r = hand.random() < 0.5, hand.random() < 0.5, hand.random() < 0.5
        flags.append((h, v, r))
        s = s.flip(2) if h else s
        s = s.flip(1) if v else s
        aug.append(s.transpose(1, 2) if r else s)
    assert any(any(f) for f in flags)
    aug = torch.stack(aug).contiguous()
    assert np.array_equal(d["img_in"].cpu().numpy(), _f32_of(aug))
    assert np.array_equal(d["img_in_up"].cpu().numpy(), _f32_of(make_lq_and_up(aug)[1]))
    M = np.stack([sample_pair_homography(rs)[1] for _ in range(4)])
    d2 = ContrasPairGenerator(use_flip=False, use_rot=False)(aug.to(dev), matrices=M)
    for k in KEYS:
        assert torch.equal(d[k], d2[k]), k


def _opt(stage):
    net = {"type": "ContrasExtractorSep"}
    o = {"model_type": "TeacherContrasModel" if stage == 1 else "StudentContrasDistillationModel", "gpu_ids": [0],
         "is_train": True, "dist": False, "path": {"strict_load": True},
         "train": {"lr_g": 1e-4, "margin": 1.0, "safe_radius": 4, "scaling_steps": 2}}
    if stage == 1:
        o["network_g"] = dict(net)
    else:
        o["network_student"], o["network_teacher"] = dict(net), dict(net)
        o["train"].update(temperature=0.15, distill_weight=15)
    return o


@pytest.mark.parametrize("stage", [1, 2])
def test_generated_batch_trains_both_models(dev, stage):
    import warnings
    import mmsr.models as models
    from c2m_amd import ops
    from mmsr.data.contras_pairs import ContrasPairGenerator
    torch.manual_seed(3)
    d = ContrasPairGenerator(seed=12)(_batch("c160", 2).to(dev))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model = models.create_model(_opt(stage))
    model.feed_data(d)
    student = model.net_g if stage == 1 else model.net_student
    if stage == 2:
        assert torch.equal(model.img_in_lq, d["img_in_up"])
    model.optimize_parameters(0)
    assert np.isfinite(model.log_dict["loss"])
    grads = [p.grad for p in student.parameters() if p.requires_grad]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    # the loss's rows are the valid correspondences counted on the host from the coordinates
    t = d["transformed_coordinate"].cpu().numpy()[:, ::4, ::4, :2]
    host = [int(((t[b, ..., 0] > 10) & (t[b, ..., 0] < 150) & (t[b, ..., 1] > 10) & (t[b, ..., 1] < 150)).sum()) for b in range(2)]
    host = [n if n >= 128 else 0 for n in host]
    with torch.no_grad():
        rows = ops.contras_loss_rows(model.output["dense_features1"].detach(), model.output["dense_features2"].detach(),
                                     d["transformed_coordinate"])
    assert rows["counts"] == host and int(rows["pos"].numel()) == sum(host) and sum(host) > 0
