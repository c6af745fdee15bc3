"""GPU: the one-launch 2-D resampler (csrc/ref_pairs.hip, ops.pil_bicubic_resize2d_u8) and the stage-3 batch maker built
on it (mmsr/data/ref_pairs.py).

Everything compared here is integer arithmetic or an exact quotient: the bound is equality -- with the two-pass operator,
with mmsr.data.pil_bicubic.pil_bicubic_resize on the CPU and with Pillow's own results
(tests/golden/contras_pairs_pillow.npz)."""
import os
import random
import warnings

import numpy as np
import pytest
import torch

import make_golden_contras_pairs as mgp

pytestmark = pytest.mark.gpu

KEYS = ("img_in", "img_in_lq", "img_in_up", "img_ref", "img_ref_lq", "img_ref_up")


def _batch(name, B):
    return torch.from_numpy(np.stack([mgp.image(name, b) for b in range(B)]))


def _rand(seed, *shape):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, size=shape).astype(np.uint8))


def _f32_of(u8):
    """uint8 / 255 as the reference forms it: an IEEE float32 division (numpy), not a multiplication by 1/255."""
    a = u8.cpu().numpy() if isinstance(u8, torch.Tensor) else u8
    return a.astype(np.float32) / np.float32(255)


def _orient(img, f):
    """The reference's augment on one [3,H,W] image: hflip, vflip, transpose, in that order."""
    s = img.flip(2) if f & 1 else img
    s = s.flip(1) if f & 2 else s
    return (s.transpose(1, 2) if f & 4 else s).contiguous()


def _check_resize(dev, img, oh, ow, flags=None, fused=True):
    """img uint8 on the CPU -> asserts fused == two-pass == CPU (on the torch-oriented image), floats exact; returns the
    fused uint8 result on the CPU."""
    from c2m_amd import ops
    from mmsr.data.pil_bicubic import pil_bicubic_resize
    H, W = img.shape[-2:]
    assert ops.pil_bicubic2d_plan(H, W, oh, ow).fused is fused
    o = img if flags is None else torch.stack([_orient(img[b], f) for b, f in enumerate(flags)])
    got, got_f, got_o = ops.pil_bicubic_resize2d_u8(img.to(dev), oh, ow, flags=flags, as_float=True, oriented_float=True)
    assert got.dtype == torch.uint8 and got_f.dtype == torch.float32 and got_o.dtype == torch.float32
    assert tuple(got.shape) == tuple(img.shape[:-2]) + (oh, ow) == tuple(got_f.shape) and tuple(got_o.shape) == tuple(img.shape)
    assert torch.equal(got, ops.pil_bicubic_resize_u8(o.to(dev), oh, ow)), (H, W, oh, ow)
    assert torch.equal(got.cpu(), pil_bicubic_resize(o, oh, ow)), (H, W, oh, ow)
    assert np.array_equal(got_f.cpu().numpy(), _f32_of(got)), (H, W, oh, ow)
    assert np.array_equal(got_o.cpu().numpy(), _f32_of(o)), (H, W, oh, ow)
    alone = ops.pil_bicubic_resize2d_u8(img.to(dev), oh, ow, flags=flags)
    assert isinstance(alone, torch.Tensor) and torch.equal(alone, got)
    return got.cpu()


# ---- fused vs two-pass vs CPU ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,B", [("c52", 3), ("c160", 4)])
def test_fused_down_and_back_is_bit_exact(dev, golden_dir, name, B):
    g = np.load(os.path.join(golden_dir, "contras_pairs_pillow.npz"))
    img = _batch(name, B)
    H, W = img.shape[-2:]
    lq = _check_resize(dev, img, H // 4, W // 4)
    assert np.array_equal(lq[0].numpy(), g[f"{name}/lq"])
    up = _check_resize(dev, lq, H, W)
    assert np.array_equal(up[0].numpy(), g[f"{name}/up"])


def test_fused_odd_ratios_single_axes_and_identity(dev, golden_dir):
    from c2m_amd import ops
    g = np.load(os.path.join(golden_dir, "contras_pairs_pillow.npz"))
    img = torch.from_numpy(mgp.image("c50"))                                   # [3,50,30]: no batch dimension
    assert np.array_equal(_check_resize(dev, img, 17, 11).numpy(), g["c50/odd"])
    _check_resize(dev, img, 61, 43)
    b = _batch("c50", 2)
    for oh, ow in ((50, 11), (17, 30), (50, 30), (61, 43)):                   # one axis, the other, none, odd up-sampling
        _check_resize(dev, b, oh, ow)
    same = ops.pil_bicubic_resize2d_u8(b.to(dev), 50, 30)                      # nothing to do: the input, as a new tensor
    assert torch.equal(same.cpu(), b)
    _check_resize(dev, img[0], 17, 11)                                         # a single [H, W] plane


def test_fused_tile_edges_small_planes_and_ragged_widths(dev):
    tiny = _rand(1, 2, 3, 8, 8)
    lq = _check_resize(dev, tiny, 2, 2)                                        # a plane smaller than one 32 x 32 tile
    _check_resize(dev, lq, 8, 8)
    src = _rand(2, 2, 3, 50, 30)
    for oh, ow in ((33, 65), (32, 64), (33, 32), (32, 33), (31, 63)):          # one pixel past / on / before a tile boundary
        _check_resize(dev, src, oh, ow)
    _check_resize(dev, _rand(3, 1, 3, 132, 260), 33, 65)                       # the same boundaries when down-sampling by 4
    _check_resize(dev, _rand(4, 2, 3, 37, 53), 10, 13)                         # widths that are no multiple of 4, in and out
    _check_resize(dev, _rand(5, 2, 3, 10, 13), 37, 53)
    _check_resize(dev, _rand(6, 1, 3, 1, 1), 5, 3)


def test_fused_batch_of_many_planes(dev):
    """More planes (600) than CUs and than one row of a 2-D grid of tiles would hold: the plane index comes from the block
    index alone."""
    _check_resize(dev, _rand(7, 200, 3, 12, 20), 5, 7)
    _check_resize(dev, _rand(8, 40, 3, 16, 16), 40, 36)                        # four tiles per plane


def test_non_contiguous_input_and_argument_errors(dev):
    import c2m_amd
    from c2m_amd import ops
    from mmsr.data.pil_bicubic import pil_bicubic_resize
    big = _batch("c52", 4)
    sl = big.to(dev)[::2, :, :, 4:36]
    assert not sl.is_contiguous()
    got = ops.pil_bicubic_resize2d_u8(sl, 13, 8, flags=[1, 2])
    want = torch.stack([_orient(big[::2, :, :, 4:36][b], f) for b, f in enumerate((1, 2))])
    assert torch.equal(got.cpu(), pil_bicubic_resize(want, 13, 8))
    for bad in (lambda: ops.pil_bicubic_resize2d_u8(sl.float(), 13, 8), lambda: ops.pil_bicubic_resize2d_u8(sl, 0, 8),
                lambda: ops.pil_bicubic_resize2d_u8(sl, 13, 8, flags=[1]), lambda: ops.pil_bicubic_resize2d_u8(sl, 13, 8, flags=[1, 8]),
                lambda: ops.pil_bicubic_resize2d_u8(sl, 13, 8, flags=torch.tensor([1, 2], device=dev)),
                lambda: ops.pil_bicubic_resize2d_u8(sl[0, 0, 0], 13, 8)):
        with pytest.raises(c2m_amd.C2MError):
            bad()


# ---- orientation ----------------------------------------------------------------------------------------------------

def test_all_eight_orientations_in_one_launch(dev):
    img = _batch("c160", 8)
    lq = _check_resize(dev, img, 40, 40, flags=list(range(8)))
    assert len({lq[b].numpy().tobytes() for b in range(8)}) == 8               # eight different images came out
    _check_resize(dev, lq, 160, 160, flags=[7, 6, 5, 4, 3, 2, 1, 0])
    _check_resize(dev, _rand(9, 8, 3, 33, 33), 33, 33, flags=list(range(8)))   # orientation alone, two tiles per axis
    _check_resize(dev, _rand(10, 8, 3, 37, 37), 50, 21, flags=list(range(8)))


def test_flips_on_a_non_square_batch(dev):
    _check_resize(dev, _batch("c52", 4), 13, 9, flags=[0, 1, 2, 3])
    _check_resize(dev, _batch("c50", 4), 61, 43, flags=[3, 2, 1, 0])


def test_transpose_of_a_non_square_plane_is_rejected(dev):
    import c2m_amd
    from c2m_amd import ops
    x = _batch("c52", 2).to(dev)
    for flags in ([0, 4], [7, 0]):
        with pytest.raises(c2m_amd.C2MError):
            ops.pil_bicubic_resize2d_u8(x, 13, 9, flags=flags)


# ---- fallback -------------------------------------------------------------------------------------------------------

def test_window_over_the_lds_budget_takes_the_two_passes(dev):
    """400 -> 10: one output tile would need the whole 400 x 400 plane and 160-tap tables in LDS (pil_bicubic2d_plan)."""
    _check_resize(dev, _rand(11, 3, 3, 400, 400), 10, 10, flags=[3, 4, 0], fused=False)
    _check_resize(dev, _rand(12, 1, 3, 400, 100), 10, 25, fused=False)
    _check_resize(dev, _rand(13, 1, 3, 400, 40), 10, 10, flags=[2])           # 160 taps on one axis alone still fit (55 KiB)


# ---- the generator --------------------------------------------------------------------------------------------------

def _seed_with_every_flag(B):
    """The first seed whose B x 3 draws set each of the three flags at least once and leave each clear at least once."""
    for s in range(1000):
        r = random.Random(s)
        fl = [(r.random() < 0.5, r.random() < 0.5, r.random() < 0.5) for _ in range(B)]
        if all({f[k] for f in fl} == {False, True} for k in range(3)):
            return s
    raise AssertionError("no seed found")


def _check_dict(d, B, H, W, keys=KEYS):
    assert sorted(d) == sorted(keys)
    for k in KEYS:
        s = (H // 4, W // 4) if k.endswith("_lq") else (H, W)
        if k == "img_in" and "original_size" in d:
            s = tuple(d["original_size"])
        assert d[k].dtype == torch.float32 and tuple(d[k].shape) == (B, 3) + s and d[k].is_cuda, k
        assert float(d[k].min()) >= 0.0 and float(d[k].max()) <= 1.0


def _hand_train(img, refs, seed, gt=160, scale=4):
    from mmsr.data.pil_bicubic import pil_bicubic_resize
    hand = random.Random(seed)
    want = {k: [] for k in KEYS}
    flags = []
    for b in range(img.shape[0]):
        ref = pil_bicubic_resize(refs[b], gt, gt)
        f = (hand.random() < 0.5) | (hand.random() < 0.5) << 1 | (hand.random() < 0.5) << 2
        flags.append(f)
        for name, x in (("img_in", img[b]), ("img_ref", ref)):
            o = _orient(x, f)
            lq = pil_bicubic_resize(o, gt // scale, gt // scale)
            want[name].append(o), want[name + "_lq"].append(lq), want[name + "_up"].append(pil_bicubic_resize(lq, gt, gt))
    return {k: _f32_of(torch.stack(v)) for k, v in want.items()}, flags


def test_train_phase_is_the_hand_composition_of_its_seeded_draws(dev):
    from mmsr.data.ref_pairs import RefPairGenerator
    B = 4
    seed = _seed_with_every_flag(B)
    img = _batch("c160", B)
    refs = [_rand(20 + b, 3, *((120, 100) if b % 2 else (90, 130))) for b in range(B)]     # a list with two sizes
    want, flags = _hand_train(img, refs, seed)
    assert all(any(f & bit for f in flags) for bit in (1, 2, 4))
    gen = RefPairGenerator(phase="train", gt_size=160, scale=4, seed=seed)
    d = gen(img.to(dev), [r.to(dev) for r in refs])
    _check_dict(d, B, 160, 160)
    for k in KEYS:
        assert np.array_equal(d[k].cpu().numpy(), want[k]), k
    # Ref as one tensor; the generator's stream has moved on by B x 3 draws
    hand = random.Random(seed)
    for _ in range(3 * B):
        hand.random()
    assert gen.flip_rng.getstate() == hand.getstate()
    ref_t = _rand(30, B, 3, 100, 180)
    d2 = RefPairGenerator(seed=seed)(img.to(dev), ref_t.to(dev))
    want2, _ = _hand_train(img, ref_t, seed)
    for k in KEYS:
        assert np.array_equal(d2[k].cpu().numpy(), want2[k]), k
    # a Ref already at the GT size is used as it is, and the switches gate the orientation
    d3 = RefPairGenerator(use_flip=False, use_rot=False, seed=seed)(img.to(dev), img.flip(0).to(dev))
    assert np.array_equal(d3["img_in"].cpu().numpy(), _f32_of(img)) and np.array_equal(d3["img_ref"].cpu().numpy(), _f32_of(img.flip(0)))
    assert torch.equal(d3["img_ref_up"], d3["img_in_up"].flip(0))


def _hand_val(img_in, img_ref, scale=4):
    from mmsr.data.pil_bicubic import pil_bicubic_resize
    crop = lambda x: x[:, :x.shape[1] - x.shape[1] % scale, :x.shape[2] - x.shape[2] % scale]   # noqa: E731
    gt, ref = crop(img_in), crop(img_ref)
    hp, wp = max(gt.shape[1], ref.shape[1]), max(gt.shape[2], ref.shape[2])
    pad = torch.zeros(2, 3, hp, wp, dtype=torch.uint8)
    pad[0, :, :gt.shape[1], :gt.shape[2]] = gt
    pad[1, :, :ref.shape[1], :ref.shape[2]] = ref
    lq = pil_bicubic_resize(pad, hp // scale, wp // scale)
    up = pil_bicubic_resize(lq, hp, wp)
    return gt.contiguous(), pad, lq, up


def test_val_phase_crops_pads_and_reports_the_original_size(dev):
    from mmsr.data.ref_pairs import RefPairGenerator
    img_in, img_ref = _rand(40, 3, 43, 58) | 1, _rand(41, 3, 50, 47) | 1      # (no zero pixels: the zero band is padding)
    d = RefPairGenerator(phase="val", scale=4)(img_in.to(dev), img_ref.to(dev))
    assert d["padding"] is True and d["original_size"] == (40, 56)
    _check_dict(d, 1, 48, 56, keys=KEYS + ("padding", "original_size"))
    gt, pad, lq, up = _hand_val(img_in, img_ref)
    assert tuple(gt.shape) == (3, 40, 56) and tuple(pad.shape) == (2, 3, 48, 56)
    assert d["img_in"].is_contiguous() and np.array_equal(d["img_in"].cpu().numpy(), _f32_of(gt[None]))
    ref = d["img_ref"].cpu().numpy()
    assert np.array_equal(ref, _f32_of(pad[1:])) and (ref[..., :48, :44] > 0).all() and not ref[..., :, 44:].any()
    for k, want in (("img_in_lq", lq[:1]), ("img_in_up", up[:1]), ("img_ref_lq", lq[1:]), ("img_ref_up", up[1:])):
        assert np.array_equal(d[k].cpu().numpy(), _f32_of(want)), k
    # the input's own zero band (rows 40..47) went through the resampler as zeros
    assert not pad[0, :, 40:].any() and np.array_equal(d["img_in_lq"].cpu().numpy(), _f32_of(lq[:1]))
    same = RefPairGenerator(phase="val")(img_in.to(dev), _rand(42, 3, 41, 59).to(dev))     # equal after the mod-crop
    assert same["padding"] is False and same["original_size"] == (40, 56)
    _check_dict(same, 1, 40, 56, keys=KEYS + ("padding", "original_size"))
    gt2, pad2, lq2, up2 = _hand_val(img_in, _rand(42, 3, 41, 59))
    assert np.array_equal(same["img_in"].cpu().numpy(), _f32_of(gt2[None])) and np.array_equal(same["img_ref"].cpu().numpy(), _f32_of(pad2[1:]))
    assert np.array_equal(same["img_ref_up"].cpu().numpy(), _f32_of(up2[1:])) and np.array_equal(same["img_in_lq"].cpu().numpy(), _f32_of(lq2[:1]))


# ---- end to end -----------------------------------------------------------------------------------------------------

def _stage3_opt():
    return {"dist": False, "gpu_ids": [0], "is_train": True, "path": {}, "scale": 4,
            "network_g": {"type": "RestorationNet", "ngf": 64, "n_blocks": 2, "groups": 8},
            "network_map": {"type": "CorrespondenceGenerationArch", "patch_size": 3, "stride": 1,
                            "vgg_layer_list": ["relu1_1", "relu2_1", "relu3_1"], "vgg_type": "vgg19"},
            "network_extractor": {"type": "ContrasExtractorSep"},
            "train": {"lr_g": 1e-4, "lr_offset": 1e-4, "lr_relu2_offset": 1e-5, "lr_relu3_offset": 1e-6,
                      "weight_decay_g": 0, "beta_g": [0.9, 0.999], "pixel_weight": 1.0}}


def _model():
    from mmsr.models.ref_restoration_model import RefRestorationModel
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # random VGG weights: intended
        return RefRestorationModel(_stage3_opt())


def test_generated_train_batch_drives_one_training_step(dev):
    from mmsr.data.ref_pairs import RefPairGenerator
    d = RefPairGenerator(phase="train", gt_size=160, scale=4, seed=12)(_batch("c160", 2).to(dev), _rand(50, 2, 3, 120, 140).to(dev))
    model = _model()
    model.feed_data(d)
    assert torch.equal(model.gt, d["img_in"]) and torch.equal(model.match_img_in, d["img_in_up"])
    model.optimize_parameters(1)
    assert np.isfinite(float(model.log_dict["l_g_pix"]))
    grads = [p.grad for p in model.net_g.parameters() if p.requires_grad]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    assert tuple(model.output.shape) == (2, 3, 160, 160)


def test_generated_val_dicts_drive_the_validation_loop(dev):
    from mmsr.data.ref_pairs import RefPairGenerator
    gen = RefPairGenerator(phase="val", scale=4)
    items = [gen(_rand(60, 3, 43, 58).to(dev), _rand(61, 3, 50, 47).to(dev)),
             gen(_rand(62, 3, 66, 50).to(dev), _rand(63, 3, 41, 75).to(dev))]
    assert [i["padding"] for i in items] == [True, True] and items[1]["original_size"] == (64, 48)
    assert tuple(items[1]["img_ref"].shape) == (1, 3, 64, 72)
    res = _model().nondist_validation(items, 0, None, False)
    assert res["count"] == 2
    assert all(np.isfinite(res[k]) for k in ("psnr", "psnr_y", "ssim_y")) and res["psnr"] > 0
