"""GPU: the Ref padding-band path -- convolutions launched on the live tiles only + band fill from a template -- returns the
bits of the full launch (c2m_amd.ops.vgg_stack_forward(live=...), csrc/ref_band.hip, roi_tiles_y / roi_tiles_x of the convolution descriptors).

Every comparison is torch.equal.  Canvases are the smallest with real tile structure at all three scales (128 x 160 and
160 x 128: H % 32 == 0 for the two pools and the 8-row tiles; the coarsest scale is then 32 x 40 / 40 x 32 pixels, one full
and one partial 32-wide tile), B = 2."""
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu

CANVAS = (128, 160)
# live extents on the 128 x 160 canvas: live + 2 (the radius of the second full-resolution layer) tile-aligned in both axes,
# one pixel past and one pixel short of the tile edge, tiny, rectangular both ways
LIVES = [(62, 94), (63, 95), (61, 93), (8, 8), (40, 100), (100, 40)]


def _ref(B, H, W, lives, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    ref = torch.zeros((B, 3, H, W), device=dev)
    for b, (lh, lw) in enumerate(lives):
        ref[b, :, :lh, :lw] = torch.rand((3, lh, lw), generator=g, device=dev) * 0.9 + 0.05   # never exactly 0 inside
    return ref


def _seed_convs(mod, seed):
    torch.manual_seed(seed)
    for m in mod.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.kaiming_normal_(m.weight)
            torch.nn.init.uniform_(m.bias, -0.5, 0.5)
    return mod


@pytest.fixture(scope="module")
def towers(dev):
    from mmsr.models.archs.contras_extractor_arch import ContrasExtractorSep
    from mmsr.models.archs.corres_generation_arch import CorrespondenceGenerationArch
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # random VGG weights: intended
        ext = _seed_convs(ContrasExtractorSep(), 1).eval().to(dev)
        mp = _seed_convs(CorrespondenceGenerationArch(3, 1, ["relu3_1", "relu2_1", "relu1_1"], "vgg19"), 2).eval().to(dev)
    return ext, mp


def _same_taps(a, b):
    from c2m_amd import ops
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
        ba, bb = ops.bordered_of(a[k]), ops.bordered_of(b[k])
        assert (ba is None) == (bb is None)
        if ba is not None:   # the whole zero-bordered buffer and the group-major twin, borders included
            assert torch.equal(ba.buf, bb.buf), k
            assert (ba.grouped8 is None) == (bb.grouped8 is None)
            if ba.grouped8 is not None:
                assert torch.equal(ba.grouped8, bb.grouped8), k


def _vgg_taps(mp, ref, live):
    from c2m_amd import ops
    v = mp.vgg
    with torch.no_grad(), ops.conv_flavour("f16x2"):
        return ops.vgg_stack_forward(v.vgg_net._modules, ref, taps=v.layer_name_list, mean=v.mean, std=v.std,
                                     grouped8_taps=v.grouped8_taps, fast=True, live=live)


def _ext_tower(ext, ref, live):
    from c2m_amd import ops
    t = ext.feature_extraction_image2
    with torch.no_grad(), ops.conv_flavour("f16x2"):
        return ops.vgg_stack_forward(t.model._modules, ref, mean=t.mean, std=t.std, last_nchw=True, live=live)


# ---- the live extent ---------------------------------------------------------------------------------------------------------
def test_live_extent(dev):
    from c2m_amd import ops
    ref = _ref(2, 128, 160, [(30, 100), (70, 20)], dev)
    assert ops.ref_live_extent(ref) == (70, 100)                       # the batch maximum of both axes
    assert ops.ref_live_extent(torch.zeros((1, 3, 16, 20), device=dev)) == (0, 0)
    z = torch.zeros((2, 3, 33, 35), device=dev)                        # W % 4 != 0: the scalar path
    z[1, 2, 17, 9] = -1e-30
    z[0, 0, 5, 31] = float("nan")                                     # not 0.0 either
    assert ops.ref_live_extent(z) == (18, 32)
    z[:] = -0.0                                                        # -0.0 == 0.0
    assert ops.ref_live_extent(z) == (0, 0)


@pytest.mark.parametrize("where", ["last_row", "last_column", "padding"])
def test_non_zero_padding_reports_the_full_extent_and_skips_nothing(dev, towers, where):
    from c2m_amd import ops
    ext, mp = towers
    H, W = CANVAS
    ref = _ref(2, H, W, [(60, 60), (60, 60)], dev)
    if where == "last_row":
        ref[1, 1, H - 1, 3] = 0.5
        ref[0, 0, 2, W - 1] = 0.5
    elif where == "last_column":
        ref[0, 2, H - 1, W - 1] = 1e-20
    else:
        ref[:, :, 60:, :] = 0.25
        ref[:, :, :, 60:] = 0.25
    live = ops.ref_live_extent(ref)
    assert live == (H, W)
    assert ops.ref_band_plan(ops.stack_geometry(mp.vgg.vgg_net._modules), H, W, *live) is None
    ops.count_conv_flops(True)
    try:
        full = _vgg_taps(mp, ref, None)
        f_full = ops.conv_flops_of_last_steps()
        band = _vgg_taps(mp, ref, live)
        f_band = ops.conv_flops_of_last_steps()
    finally:
        ops.count_conv_flops(False)
    assert f_band == f_full                                           # every tile launched, no template
    _same_taps(full, band)


# ---- single layers: ROI launch + fill against the full launch ----------------------------------------------------------------
@pytest.fixture(scope="module")
def layer_case(dev):
    """A band-shaped 64-channel input (the first layer's output on a zero-padded image), its template, one 64 -> 64 layer."""
    from c2m_amd import ops
    H, W = CANVAS
    g = torch.Generator(device=dev).manual_seed(5)
    w1 = torch.randn((64, 3, 3, 3), generator=g, device=dev) * 0.3
    b1 = torch.rand(64, generator=g, device=dev) - 0.3
    w2 = torch.randn((64, 64, 3, 3), generator=g, device=dev) * 0.06
    b2 = torch.rand(64, generator=g, device=dev) - 0.3
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225], device=dev).view(1, 3, 1, 1)
    return dict(H=H, W=W, w1=w1, b1=b1, w2=w2, b2=b2, mean=mean, std=std)


@pytest.mark.parametrize("live", LIVES)
def test_first_layer_with_twin(dev, layer_case, live):
    from c2m_amd import ops
    c = layer_case
    H, W = c["H"], c["W"]
    ref = _ref(2, H, W, [live, (live[0] // 2, live[1])], dev, seed=live[0])
    plan = ops.ref_band_plan(["conv"], H, W, *live)
    roi, (th, tw) = plan["convs"][0]["roi"], plan["convs"][0]["tile"]
    Ht, Wt = plan["template"]
    kw = dict(act=ops.ACT_RELU, mean=c["mean"], std=c["std"])

    def run(img, **extra):
        B, _, h, w = img.shape
        bo = ops._bordered_empty(B, 64, h, w, dev, grouped8=True)
        if extra:   # poison what the ROI launch must leave to the fill
            bo.interior().fill_(float("nan"))
            bo.grouped8[:, :, 1:h + 1, 1:w + 1].fill_(float("nan"))
        ops.conv3x3_rgb64(img, c["w1"], c["b1"], out=bo.interior(), out2_grouped8=bo.grouped8, **kw, **extra)
        return bo
    full, tmpl = run(ref), run(torch.zeros((1, 3, Ht, Wt), device=dev))
    part = run(ref, roi_tiles=roi)
    rh, rw = min(roi[0] * th, H), min(roi[1] * tw, W)
    assert (rh, rw) != (H, W)
    assert torch.equal(part.interior()[:, :, :rh, :rw], full.interior()[:, :, :rh, :rw])
    assert bool(torch.isnan(part.interior()[:, :, rh:, :]).all()) and bool(torch.isnan(part.interior()[:, :, :, rw:]).all())
    m = ops.band_margin(1, 1)
    ops.band_fill(part.interior(), tmpl.interior(), rh, rw, m, m)
    ops.band_fill(part.grouped8, tmpl.grouped8, rh, rw, m, m, layout="grouped8")
    assert torch.equal(part.buf, full.buf) and torch.equal(part.grouped8, full.grouped8)


@pytest.mark.parametrize("algo", ["split16", "split"])
@pytest.mark.parametrize("mode", ["nhwc", "nhwc_pool2", "nchw"])
@pytest.mark.parametrize("live", LIVES)
def test_one_layer_every_epilogue(dev, layer_case, live, mode, algo):
    from c2m_amd import ops
    c = layer_case
    H, W = c["H"], c["W"]
    ref = _ref(2, H, W, [(live[0] // 2, live[1]), live], dev, seed=live[1])
    plan = ops.ref_band_plan(["conv", "conv"], H, W, *live)
    pc = plan["convs"][1]
    Ht, Wt = plan["template"]
    kw = dict(act=ops.ACT_RELU, mean=c["mean"], std=c["std"])
    x = ops.conv3x3_rgb64(ref, c["w1"], c["b1"], **kw)
    tx = ops.conv3x3_rgb64(torch.zeros((1, 3, Ht, Wt), device=dev), c["w1"], c["b1"], **kw)
    ckw = dict(act=ops.ACT_RELU, out_mode=mode, algo=algo)
    full = ops.conv3x3(x, c["w2"], c["b2"], **ckw)
    tmpl = ops.conv3x3(tx, c["w2"], c["b2"], **ckw)
    part = ops.conv3x3(x, c["w2"], c["b2"], roi_tiles=pc["roi"], **ckw)
    rh, rw = min(pc["roi"][0] * 8, H), min(pc["roi"][1] * 32, W)
    so = 1
    if mode == "nhwc_pool2":
        rh, rw, so = rh // 2, rw // 2, 2
    assert torch.equal(part[:, :, :rh, :rw], full[:, :, :rh, :rw])
    m = ops.band_margin(pc["radius"], so)
    ops.band_fill(part, tmpl, rh, rw, m, m, layout="nchw" if mode == "nchw" else "nhwc")
    assert torch.equal(part, full)
    ops.range_flag_set(dev)   # (explicit f16 x 2 calls report into the per-device flag: leave it clear)


# ---- the two Ref-side towers -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canvas,live", [(CANVAS, lv) for lv in LIVES] + [((160, 128), (94, 62)), ((160, 128), (33, 70))])
def test_vgg_taps_and_extractor_tower(dev, towers, canvas, live):
    from c2m_amd import ops
    ext, mp = towers
    H, W = canvas
    ref = _ref(2, H, W, [live, (max(live[0] - 9, 1), live[1])], dev, seed=sum(live))
    assert ops.ref_live_extent(ref) == live
    ops.count_conv_flops(True)
    try:
        full = _vgg_taps(mp, ref, None)
        f_full = ops.conv_flops_of_last_steps(executed=True)
        band = _vgg_taps(mp, ref, live)
        f_band = ops.conv_flops_of_last_steps(executed=True)
    finally:
        ops.count_conv_flops(False)
    _same_taps(full, band)
    assert f_band != f_full                                           # the band path ran (ROI launches + template are what is counted)
    e_full, e_band = _ext_tower(ext, ref, None), _ext_tower(ext, ref, live)
    assert list(e_full) == ["conv3_1"] and torch.equal(e_full["conv3_1"], e_band["conv3_1"])
    assert not ops.range_flag_set(dev)                                # finite copies of computed values: no range report


def test_counted_flops_are_those_of_the_tiles_launched(dev, towers):
    from c2m_amd import ops
    _, mp = towers
    H, W = CANVAS
    live = (40, 60)
    ref = _ref(2, H, W, [live, live], dev)
    layers = mp.vgg.vgg_net._modules
    plan = ops.ref_band_plan(ops.stack_geometry(layers), H, W, *live)
    Ht, Wt = plan["template"]
    convs = [m for m in layers.values() if isinstance(m, torch.nn.Conv2d)]
    want = 0.0
    for k, (m, pc) in enumerate(zip(convs, plan["convs"])):
        s = pc["scale"]
        rh, rw = min(pc["roi"][0] * pc["tile"][0], H // s), min(pc["roi"][1] * pc["tile"][1], W // s)
        kk = 27 if k == 0 else 9 * m.in_channels
        want += 2.0 * m.out_channels * kk * (2 * rh * rw + (Ht // s) * (Wt // s))
    ops.count_conv_flops(True)
    try:
        _vgg_taps(mp, ref, live)
        got = ops.conv_flops_of_last_steps()
    finally:
        ops.count_conv_flops(False)
    assert got == want


def test_canvas_sized_ref_declines_and_returns_the_same_tensors(dev, towers):
    from c2m_amd import ops
    ext, mp = towers
    H, W = CANVAS
    ref = _ref(2, H, W, [(H, W), (50, 50)], dev)
    assert ops.ref_live_extent(ref) == (H, W)
    _same_taps(_vgg_taps(mp, ref, None), _vgg_taps(mp, ref, (H, W)))
    assert torch.equal(_ext_tower(ext, ref, None)["conv3_1"], _ext_tower(ext, ref, (H, W))["conv3_1"])


def test_edge_strips_are_not_the_interior_constant(dev, towers):
    """The band is not constant: the last rows / columns see the zero padding outside the canvas.  A 'constant band' fill gets
    exactly these wrong."""
    _, mp = towers
    H, W = CANVAS
    live = (30, 40)
    ref = _ref(2, H, W, [live, live], dev)
    full, band = _vgg_taps(mp, ref, None), _vgg_taps(mp, ref, live)
    for name in ("relu1_1", "relu2_1", "relu3_1"):
        f, b = full[name], band[name]
        h, w = f.shape[2:]
        interior = f[0, :, h - 6, w - 6]
        assert torch.equal(f[0, :, h - 7, w - 7], interior)                        # deep in the band: constant
        assert not torch.equal(f[0, :, h - 1, w - 6], interior)                    # bottom strip
        assert not torch.equal(f[0, :, h - 6, w - 1], interior)                    # right strip
        assert not torch.equal(f[0, :, h - 1, w - 1], f[0, :, h - 1, w - 6])       # corner
        assert torch.equal(b[:, :, h - 3:, :], f[:, :, h - 3:, :]) and torch.equal(b[:, :, :, w - 3:], f[:, :, :, w - 3:])
        assert not torch.equal(f[0, :, 0, w - 6], interior)                        # top strip right of the live region
        assert torch.equal(b[:, :, :3, :], f[:, :, :3, :])


# ---- through the modules ---------------------------------------------------------------------------------------------------
def test_two_samples_with_different_extents_through_the_modules(dev, towers):
    from c2m_amd import ops
    ext, mp = towers
    H, W = CANVAS
    ref = _ref(2, H, W, [(30, 100), (70, 20)], dev)
    up = torch.rand((2, 3, H, W), generator=torch.Generator(device=dev).manual_seed(3), device=dev)
    outs = []
    for mode in (0, 1):
        with torch.no_grad(), ops.ref_band_mode(mode), warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)   # a range-guard re-run would warn
            outs.append((ext(up, ref), mp.vgg(ref)))
    (f0, t0), (f1, t1) = outs
    assert torch.equal(f0["dense_features1"], f1["dense_features1"]) and torch.equal(f0["dense_features2"], f1["dense_features2"])
    _same_taps(t0, t1)
    for owner in (ext, mp.vgg, ext.feature_extraction_image2):
        assert not getattr(owner, "_c2m_conv_bf16x3", False)          # the range flag stayed clear


def test_index_map_values_and_sr_are_unchanged(dev):
    """LR 40, Ref live 100 on the 160 canvas: extractor -> match -> VGG taps -> restoration with the path off and on."""
    import bench
    from c2m_amd import ops
    ext, mp, net = bench.build_models(dev)
    g = torch.Generator(device=dev).manual_seed(11)
    lq = torch.rand((1, 3, 40, 40), generator=g, device=dev)
    up = torch.nn.functional.interpolate(lq, scale_factor=4, mode="bicubic", align_corners=False).clamp(0, 1)
    ref = torch.zeros((1, 3, 160, 160), device=dev)
    ref[:, :, :100, :100] = torch.rand((1, 3, 100, 100), generator=g, device=dev)

    class Owner:
        pass
    res = []
    for mode in (0, 1):
        owner = Owner()

        def whole():
            feats = ext(up, ref)
            idx, val = mp.match(feats)
            pre, ref_feat = mp(feats, ref)
            return idx, val, pre.max_idx, net(lq, pre, ref_feat)
        with torch.no_grad(), ops.ref_band_mode(mode):
            res.append(ops.f16_range_guard(owner, whole, dev))
        assert not getattr(owner, "_c2m_conv_bf16x3", False)
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(res[1][3]).all())


def test_extent_is_read_once_per_step(dev, towers, monkeypatch):
    from c2m_amd import ops
    ext, mp = towers
    H, W = CANVAS
    ref = _ref(2, H, W, [(30, 100), (70, 20)], dev)
    up = torch.rand((2, 3, H, W), device=dev)
    calls = []
    real = ops.ref_live_extent
    monkeypatch.setattr(ops, "ref_live_extent", lambda img: calls.append(1) or real(img))

    class Owner:
        pass
    with torch.no_grad():
        ops.f16_range_guard(Owner(), lambda: (ext(up, ref), mp.vgg(ref)), dev)
        assert len(calls) == 1
        ops.f16_range_guard(Owner(), lambda: (ext(up, ref), mp.vgg(ref)), dev)   # the next step reads it again: nothing is kept
        assert len(calls) == 2
        with ops.ref_band_mode(0):
            ops.f16_range_guard(Owner(), lambda: (ext(up, ref), mp.vgg(ref)), dev)
        assert len(calls) == 2
