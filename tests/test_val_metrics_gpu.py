"""GPU: the one-pass validation kernel (csrc/val_metrics.hip, c2m_amd.ops.val_metrics) against the float64 torch
composition of mmsr/utils/metrics.py evaluated on the same tensors moved to the CPU (itself pinned to the reference by
tests/test_metrics.py), and the model's validation loop on both paths.

Tolerances (derived, not measured; the measured maxima are in DESIGN.md section 14):
  sr_u8 / gt_u8   bit-exact: integer result of identical fp32 operations
  PSNR            1e-9 dB: the squared-difference sums are integers below 2^53, exact in any order
  PSNR_Y          1e-8 dB: float64 sum of <= 4e5 terms, relative order error <= N eps ~ 1e-10, x 8.7 dB per unit of it
  SSIM_Y          1e-9: a 121-term float64 windowed mean of values <= 65025 is off by <= ~2e-9, over denominators >= C2 = 58.5
"""
import json
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"psnr": 1e-9, "psnr_y": 1e-8, "ssim_y": 1e-9}


def _pair(B, H, W, seed):
    """B distinct image pairs, uniform in [-0.2, 1.2] so that the clamp acts; GT = SR + noise."""
    g = torch.Generator().manual_seed(seed)
    sr = torch.rand(B, 3, H, W, generator=g) * 1.4 - 0.2
    gt = sr + (torch.rand(B, 3, H, W, generator=g) - 0.5) * 0.2
    return sr, gt


_yardstick = {}


def _reference(key, sr, gt, crop):
    """metrics.validation_metrics and the uint8 images on the CPU, computed once per key and never modified."""
    from mmsr.utils import metrics
    if key not in _yardstick:
        m = metrics.validation_metrics(sr, gt, crop_border=crop)
        u8 = tuple(metrics.tensor2img_device(t).to(torch.uint8) for t in (sr, gt))
        _yardstick[key] = (m, u8)
    return _yardstick[key]


def _close(got, want, tol, what):
    got, want = got.cpu(), want.cpu()
    assert got.dtype == torch.float64 and got.shape == want.shape, what
    for b, (x, y) in enumerate(zip(got.tolist(), want.tolist())):
        print(f"{what}[{b}]: fused {x!r} reference {y!r} |diff| {abs(x - y) if math.isfinite(y) else 0.0:.3e}")
        assert x == y or abs(x - y) <= tol, (what, b, x, y)


def _check(dev, sr, gt, crop, key, valid_hw=None, sr_dev=None, gt_dev=None):
    """sr, gt: CPU tensors (already cut to the valid window: what the yardstick sees); sr_dev / gt_dev: what the op is given."""
    from c2m_amd import ops
    want, (s8, g8) = _reference(key, sr, gt, crop)
    sr_dev = sr.to(dev) if sr_dev is None else sr_dev
    gt_dev = gt.to(dev) if gt_dev is None else gt_dev
    for order in ("bgr", "rgb"):
        got = ops.val_metrics(sr_dev, gt_dev, crop_border=crop, valid_hw=valid_hw, images=order)
        for k in ("psnr", "psnr_y", "ssim_y"):
            _close(got[k], want[k], TOL[k], f"{key} {k}")
        for name, ref in (("sr_u8", s8), ("gt_u8", g8)):
            ref = ref if order == "bgr" else ref.flip(-1)
            assert got[name].dtype == torch.uint8 and torch.equal(got[name].cpu(), ref), (key, name, order)
    plain = ops.val_metrics(sr_dev, gt_dev, crop_border=crop, valid_hw=valid_hw)
    assert sorted(plain) == ["psnr", "psnr_y", "ssim_y"]
    for k in plain:
        assert torch.equal(plain[k], got[k]), k       # the image stores change no sum
    return got


def _tile_shapes():
    from c2m_amd import ops
    th, tw = ops.val_metrics_tile()
    crop = 4
    # a cropped window of (t + 10) pixels gives t outputs: one more than a tile, one fewer than two tiles, per direction
    return th, tw, [(th + 11 + 2 * crop, tw + 11 + 2 * crop, crop), (2 * th + 9 + 2 * crop, 2 * tw + 9 + 2 * crop, crop),
                    (th + 11 + 2 * crop, 2 * tw + 9 + 2 * crop, crop), (2 * th + 9 + 2 * crop, tw + 11 + 2 * crop, crop)]


@pytest.mark.parametrize("H,W,crop", [(19, 19, 4), (21, 37, 0), (37, 41, 4), (45, 77, 4)])
def test_small_shapes_agree_with_the_cpu_composition(dev, H, W, crop):
    sr, gt = _pair(3, H, W, 100 + H)
    _check(dev, sr, gt, crop, ("small", H, W, crop))


def test_windows_one_past_a_tile_and_one_short_of_two(dev):
    th, tw, shapes = _tile_shapes()
    assert th >= 1 and tw >= 1
    for H, W, crop in shapes:
        sr, gt = _pair(3, H, W, 200 + H + W)
        _check(dev, sr, gt, crop, ("tile", H, W, crop))


@pytest.mark.parametrize("B", [1, 3])
def test_valid_window_of_padded_tensors(dev, B):
    sr, gt = _pair(B, 80, 104, 300 + B)
    _check(dev, sr[..., :75, :101].contiguous(), gt[..., :75, :101].contiguous(), 4, ("valid", B), valid_hw=(75, 101),
           sr_dev=sr.to(dev), gt_dev=gt.to(dev))


def test_a_cropped_view_is_read_in_place(dev):
    from c2m_amd import ops
    sr, gt = _pair(3, 50, 61, 400)
    sd, gd = sr.to(dev), gt.to(dev)
    vs, vg = sd[..., :45, :53], gd[..., 2:47, 5:58]
    assert not vs.is_contiguous() and not vg.is_contiguous()
    a = ops.val_metrics(vs, vg, images="bgr")
    b = ops.val_metrics(vs.contiguous(), vg.contiguous(), images="bgr")
    for k in a:
        assert torch.equal(a[k], b[k]), k
    _check(dev, sr[..., :45, :53].contiguous(), gt[..., 2:47, 5:58].contiguous(), 4, "view", sr_dev=vs, gt_dev=vg)
    # a permuted tensor has no unit innermost stride: an error, not a copy
    with pytest.raises(ops._lib.C2MError):
        ops.val_metrics(sd.transpose(-1, -2), gd.transpose(-1, -2))


def test_rounding_ties_and_the_extreme_pair(dev):
    H, W = 37, 41
    sr, gt = _pair(3, H, W, 500)
    k = torch.arange(3 * H * W, dtype=torch.float32) % 255
    sr[1] = ((k + 0.5) / 255).reshape(3, H, W)           # products with 255 that land on .5: half to even decides
    p = sr[1].clamp(0, 1) * 255.0
    assert int((p - p.floor() == 0.5).sum()) > 100        # (ties do occur in fp32)
    sr[2], gt[2] = 0.0, 1.0
    got = _check(dev, sr, gt, 4, "values")
    assert abs(float(got["psnr"][2])) < 1e-9              # mse 255^2


def test_identical_images_give_inf_and_exactly_one(dev):
    from c2m_amd import ops
    sr, _ = _pair(3, 45, 77, 600)
    m = ops.val_metrics(sr.to(dev), sr.clone().to(dev))
    assert bool(torch.isinf(m["psnr"]).all()) and bool(torch.isinf(m["psnr_y"]).all())
    assert m["ssim_y"].tolist() == [1.0, 1.0, 1.0]


def test_golden_pairs_of_the_reference(dev, golden_dir):
    from make_golden import metric_images
    from mmsr.utils import metrics
    gold = np.load(f"{golden_dir}/metrics_golden.npz")
    rgb = lambda t: (t / 255.0).flip(-1).movedim(-1, 0).contiguous()  # noqa: E731  (planar, as a network's output)
    for k in range(3):
        a, b = (torch.from_numpy(x) for x in metric_images(k))
        m = metrics.validation_metrics_fused(rgb(b)[None].to(dev), rgb(a)[None].to(dev), crop_border=4)
        assert abs(float(m["psnr"][0]) - float(gold[f"psnr{k}"])) < 1e-4
        assert abs(float(m["psnr_y"][0]) - float(gold[f"psnr_y{k}"])) < 1e-4
        assert abs(float(m["ssim_y"][0]) - float(gold[f"ssim_y{k}"])) < 1e-6
        u8 = metrics.tensor2img_u8(rgb(a).to(dev))
        assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), a.numpy().astype(np.uint8))


def test_the_torch_composition_divides_on_the_gpu_as_on_the_cpu(dev):
    """torch turns `cuda_tensor / 255.0` into a multiplication with the fp32 reciprocal; under metrics.true_scalar_division the
    composition on the GPU is the CPU's (the reference's) arithmetic again, which is what C2M_VAL_FUSED=0 reports."""
    from mmsr.utils import metrics
    v = torch.arange(256, dtype=torch.float32)
    with metrics.true_scalar_division():
        q = v.to(dev) / 255.0
        r = v.to(dev).div_(255.0)
        untouched = (v / 255.0, v.to(dev) / torch.full((256,), 255.0, device=dev), v.to(dev).double() / 3)
    assert torch.equal(q.cpu(), v / 255.0) and torch.equal(r.cpu(), v / 255.0) and q.dtype == torch.float32
    assert torch.equal(untouched[0], v / 255.0) and torch.equal(untouched[1].cpu(), v / 255.0)
    assert untouched[2].dtype == torch.float64 and torch.equal(untouched[2].cpu(), v.double() / 3)
    sr, gt = _pair(3, 45, 77, 100 + 45)
    want, _ = _reference(("small", 45, 77, 4), sr, gt, 4)
    with metrics.true_scalar_division():
        got = metrics.validation_metrics(sr.to(dev), gt.to(dev), crop_border=4)
    for k in ("psnr", "psnr_y", "ssim_y"):
        _close(got[k], want[k], TOL[k], f"torch composition on the GPU {k}")


def test_two_calls_return_the_same_bits(dev):
    from c2m_amd import ops
    th, tw = ops.val_metrics_tile()
    sr, gt = _pair(3, 3 * th + 25, 2 * tw + 31, 700)
    sd, gd = sr.to(dev), gt.to(dev)
    first = ops.val_metrics_sums(sd, gd)[0]
    second = ops.val_metrics_sums(sd, gd)[0]
    assert first.dtype == torch.float64 and tuple(first.shape) == (3, 3)
    assert torch.equal(first.view(torch.int64), second.view(torch.int64))


def test_rejected_inputs(dev):
    from c2m_amd import C2MError, ops
    sr, gt = _pair(1, 18, 30, 800)
    with pytest.raises(C2MError):
        ops.val_metrics(sr.to(dev), gt.to(dev), crop_border=4)       # cropped window 10 x 22
    with pytest.raises(C2MError):
        ops.val_metrics(gt.to(dev).transpose(-1, -2).contiguous(), sr.to(dev).transpose(-1, -2).contiguous(), crop_border=4)
    sr, gt = _pair(1, 19, 19, 801)
    with pytest.raises(C2MError):
        ops.val_metrics(sr, gt)                                        # CPU tensors
    with pytest.raises(C2MError):
        ops.tensor_to_u8(sr)
    assert tuple(ops.tensor_to_u8(sr[0, :, :5, :7].to(dev)).shape) == (5, 7, 3)   # the image alone has no size limit


# ---- the model's validation loop ---------------------------------------------------------------------------------------------

def _rand(seed, *shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _stage3_opt():
    return {"dist": False, "gpu_ids": [0], "is_train": True, "path": {}, "scale": 4,
            "network_g": {"type": "RestorationNet", "ngf": 64, "n_blocks": 2, "groups": 8},
            "network_map": {"type": "CorrespondenceGenerationArch", "patch_size": 3, "stride": 1,
                            "vgg_layer_list": ["relu1_1", "relu2_1", "relu3_1"], "vgg_type": "vgg19"},
            "network_extractor": {"type": "ContrasExtractorSep"},
            "train": {"lr_g": 1e-4, "lr_offset": 1e-4, "lr_relu2_offset": 1e-5, "lr_relu3_offset": 1e-6,
                      "weight_decay_g": 0, "beta_g": [0.9, 0.999], "pixel_weight": 1.0}}


def _model(opt=None):
    from mmsr.models.ref_restoration_model import RefRestorationModel
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # random VGG weights: intended
        return RefRestorationModel(opt or _stage3_opt())


def _val_items(dev):
    from mmsr.data.ref_pairs import RefPairGenerator
    gen = RefPairGenerator(phase="val", scale=4)
    return [gen(_rand(60, 3, 43, 58).to(dev), _rand(61, 3, 50, 47).to(dev)),
            gen(_rand(62, 3, 66, 50).to(dev), _rand(63, 3, 41, 75).to(dev))]


_CHILD = """
import json, sys
sys.path[:0] = [sys.argv[1] + "/c2-matching_amd", sys.argv[1] + "/tests/golden", sys.argv[1] + "/tests"]
import torch
import test_val_metrics_gpu as t
from mmsr.models import ref_restoration_model as rrm
from mmsr.utils import metrics
calls = {"fused": 0, "torch": 0}
for name, key in (("validation_metrics_fused", "fused"), ("validation_metrics", "torch")):
    def counted(*a, _f=getattr(metrics, name), _k=key, **kw):
        calls[_k] += 1
        return _f(*a, **kw)
    setattr(metrics, name, counted)
res = t._model().nondist_validation(t._val_items(torch.device("cuda:0")), 0, None, False)
print("RESULT " + json.dumps({"res": res, "calls": calls, "switch": rrm._VAL_FUSED}))
"""


def _validate_in_child(fused):
    env = dict(os.environ, C2M_VAL_FUSED=fused)
    out = subprocess.run([sys.executable, "-c", _CHILD, REPO], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def test_the_model_reports_the_same_numbers_on_both_paths(dev):
    """nondist_validation with C2M_VAL_FUSED at 1 and at 0, each in a fresh process, held to the tolerances above.  The
    torch side evaluates metrics.validation_metrics on the GPU under metrics.true_scalar_division (see the test above)."""
    one, zero = _validate_in_child("1"), _validate_in_child("0")
    assert one["switch"] is True and one["calls"] == {"fused": 2, "torch": 0}
    assert zero["switch"] is False and zero["calls"] == {"fused": 0, "torch": 2}
    assert one["res"]["count"] == zero["res"]["count"] == 2
    for k in ("psnr", "psnr_y", "ssim_y"):
        print(f"model {k}: fused {one['res'][k]!r} torch {zero['res'][k]!r} |diff| {abs(one['res'][k] - zero['res'][k]):.3e}")
    for k in ("psnr", "psnr_y", "ssim_y"):
        assert abs(one["res"][k] - zero["res"][k]) <= TOL[k], k


def test_save_img_writes_the_models_sr_as_png(dev, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from mmsr.utils import metrics
    opt = _stage3_opt()
    opt["path"] = {"visualization": str(tmp_path / "vis")}
    model = _model(opt)
    items = _val_items(dev)
    items[0]["lq_path"] = ["/data/CUFED5/007_0.png"]
    outs, run = [], model.test

    def recording_test():
        outs.append(run().clone())
        return outs[-1]
    model.test = recording_test
    res = model.nondist_validation(items, 1234, None, True)
    assert res["count"] == 2 and len(outs) == 2
    paths = [tmp_path / "vis" / "007_0" / "007_0_1234.png", tmp_path / "vis" / "1" / "1_1234.png"]
    written = sorted(p for p in (tmp_path / "vis").rglob("*") if p.is_file())
    assert written == sorted(paths)
    for item, sr, path in zip(items, outs, paths):
        oh, ow = item["original_size"]
        want = metrics.tensor2img_device(sr[..., :oh, :ow]).flip(-1).to(torch.uint8)[0].cpu().numpy()
        got = np.asarray(Image.open(path))
        assert got.shape == (oh, ow, 3) and got.dtype == np.uint8 and np.array_equal(got, want), path
    model.feed_data(items[0])
    model.test()
    vis = model.get_current_visuals()
    assert list(vis) == ["img_in_lq", "rlt", "gt"] and all(not v.is_cuda for v in vis.values())
    assert torch.equal(vis["rlt"], model.output.cpu())
