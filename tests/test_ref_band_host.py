"""CPU: the host arithmetic of the Ref padding-band path (c2m_amd.ops.ref_band_plan and friends; csrc/ref_band.hip).

No kernel runs here: the plan is pure integer arithmetic, the tile shapes come from a host-side library call, and the fill's
edge-distance clamp is checked on a numpy model of a band-shaped map."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geometry(vgg_type, upto):
    from mmsr.models.archs.vgg_arch import NAMES
    names = NAMES[vgg_type][:NAMES[vgg_type].index(upto) + 1]
    return ["conv" if n.startswith("conv") else "pool" for n in names if not n.startswith("relu")]


def test_tile_shapes_are_the_kernels():
    from c2m_amd import ops
    assert ops.conv_roi_tile(False) == (8, 32)      # split kernels: 32 x 8 pixels
    assert ops.conv_roi_tile(True)[0] == 8          # first-layer kernel: rows of 8 as well


@pytest.mark.parametrize("vgg_type,upto", [("vgg19", "relu3_1"), ("vgg16", "conv3_1")])
def test_plan_of_the_flagship_shapes(vgg_type, upto):
    """live 500 on a 640 canvas: live + radius = 502 / 253 / 128 pixels and 16 x 63, 8 x 32, 4 x 16 of 20 x 80, 10 x 40, 5 x 20
    split-kernel tiles at 640 / 320 / 160 -- derived from the layer list of both Ref-side towers."""
    from c2m_amd import ops
    geo = _geometry(vgg_type, upto)
    assert geo == ["conv", "conv", "pool", "conv", "conv", "pool", "conv"]
    plan = ops.ref_band_plan(geo, 640, 640, 500, 500)
    convs = plan["convs"]
    assert [c["scale"] for c in convs] == [1, 1, 2, 2, 4]
    assert [c["radius"] for c in convs] == [1, 2, 4, 6, 10]
    assert [c["extent"] for c in convs] == [(501, 501), (502, 502), (252, 252), (253, 253), (128, 128)]
    # (rows, columns) of tiles: the issue's "16 x 63" is columns x rows
    assert [c["tiles"] for c in convs[1:]] == [(80, 20), (40, 10), (40, 10), (20, 5)]
    assert [c["roi"] for c in convs[1:]] == [(63, 16), (32, 8), (32, 8), (16, 4)]
    th, tw = ops.conv_roi_tile(True)
    assert convs[0]["tile"] == (th, tw) and convs[0]["roi"] == (-(-501 // th), -(-501 // tw))
    for c in convs[1:]:
        frac = c["roi"][0] * c["roi"][1] / (c["tiles"][0] * c["tiles"][1])
        assert 0.62 < frac < 0.65
    # template: every side >= 2 R + 2 tiles of the coarsest scale, pools stay aligned from both ends
    Ht, Wt = plan["template"]
    assert Ht >= 2 * 10 + 2 * 4 * 8 and Wt >= 2 * 10 + 2 * 4 * 32 and Ht % 16 == 0 and Wt % 16 == 0


def test_plan_declines():
    from c2m_amd import ops
    geo = _geometry("vgg19", "relu3_1")
    assert ops.ref_band_plan(geo, 640, 640, 640, 640) is None          # no padding
    assert ops.ref_band_plan(geo, 640, 640, None, None) is None
    assert ops.ref_band_plan(geo, 640, 640, 639, 636) is None          # saves less than a tile row / column at every layer
    assert ops.ref_band_plan(geo, 642, 640, 100, 100) is None          # the pools would not align from the bottom edge
    assert ops.ref_band_plan(geo, 16, 16, 4, 4) is None                # no interior at the coarsest scale
    one_axis = ops.ref_band_plan(geo, 640, 640, 640, 500)              # full height, padded width: columns only
    assert all(c["roi"][0] == c["tiles"][0] and c["roi"][1] < c["tiles"][1] for c in one_axis["convs"])


def test_rectangular_and_tiny_extents():
    from c2m_amd import ops
    geo = _geometry("vgg16", "conv3_1")
    p = ops.ref_band_plan(geo, 128, 160, 8, 8)
    assert [c["roi"] for c in p["convs"]] == [(2, 1), (2, 1), (1, 1), (1, 1), (1, 1)]
    p = ops.ref_band_plan(geo, 128, 160, 62, 94)        # 62 + 2 = 64, 94 + 2 = 96: tile-aligned at full resolution
    assert p["convs"][1]["extent"] == (64, 96) and p["convs"][1]["roi"] == (8, 3)
    p = ops.ref_band_plan(geo, 128, 160, 63, 95)        # one past the tile edge
    assert p["convs"][1]["roi"] == (9, 4)
    p = ops.ref_band_plan(geo, 128, 160, 0, 0)          # an all-zero batch still launches one tile
    assert all(min(c["roi"]) >= 1 for c in p["convs"])


def _band_map(H, W, margin):
    """A map that depends on the distances to the four edges up to `margin` and is constant beyond."""
    def axis(n):
        v = np.arange(n)
        return np.minimum(v, margin) * 100 + np.minimum(n - 1 - v, margin)
    return axis(H)[:, None] * 10000 + axis(W)[None, :]


@pytest.mark.parametrize("H,W,Ht,Wt,margin", [(32, 40, 12, 20, 3), (7, 9, 7, 30, 3), (40, 32, 9, 9, 4)])
def test_template_clamp_reproduces_a_band_map(H, W, Ht, Wt, margin):
    from c2m_amd import ops
    # the map "sees" an edge within margin - 1 pixels; the clamp has one pixel to spare, as band_margin gives it
    full, tmpl = _band_map(H, W, margin - 1), _band_map(Ht, Wt, margin - 1)
    sy = [ops.band_src_index(y, H, Ht, margin) for y in range(H)]
    sx = [ops.band_src_index(x, W, Wt, margin) for x in range(W)]
    assert min(sy) >= 0 and max(sy) < Ht and min(sx) >= 0 and max(sx) < Wt
    assert np.array_equal(tmpl[np.ix_(sy, sx)], full)
    # right / bottom strips and the corner are NOT the interior constant
    assert full[-1, W // 2] != full[H // 2, W // 2] and full[H // 2, -1] != full[H // 2, W // 2] and full[-1, -1] != full[-1, W // 2]


def test_band_margin():
    from c2m_amd import ops
    assert [ops.band_margin(r, s) for r, s in ((1, 1), (2, 1), (2, 2), (6, 2), (6, 4), (10, 4))] == [2, 3, 2, 4, 3, 4]


def test_flops_count_the_tiles_launched():
    from c2m_amd import ops
    assert ops._roi_pixels(None, 640, 640) == (640, 640)
    assert ops._roi_pixels((63, 16), 640, 640) == (504, 512)
    assert ops._roi_pixels((80, 20), 640, 640) == (640, 640)
    assert ops._roi_pixels((3, 2), 20, 40) == (20, 40)                   # partial edge tiles count their pixels inside the map
    th, tw = ops.conv_roi_tile(True)
    assert ops._roi_pixels((63, 8), 640, 640, rgb64=True) == (min(63 * th, 640), min(8 * tw, 640))


def test_header_and_library_agree_on_the_new_entry_points():
    import c2m_amd
    hdr = open(os.path.join(REPO, "include", "c2m_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(c2m_amd.LIB_PATH)
    for name in ("c2m_conv3x3_roi_tile", "c2m_ref_live_extent_f32", "c2m_band_fill_f32"):
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
    # ABI 6: the ROI is two fields of the convolution descriptors, the fused DCNv2 forward one entry point with a descriptor
    for name in ("c2m_conv3x3_nhwc_roi_f32", "c2m_conv3x3_rgb64_roi_f32", "c2m_dcn_v2_forward_nhwc_f32", "c2m_dcn_v2_forward_nhwc_f16x2"):
        assert not re.search(r"\b%s\b" % name, hdr), name
        assert not hasattr(lib, name), name
    assert lib.c2m_abi_version() == 6
    # the fill refuses geometries whose clamp zones would overlap, before anything is launched (no GPU needed)
    L = c2m_amd._lib.lib()
    assert L.c2m_band_fill_f32(None, 16, 1, 4, 4, 40, 4, 4, 160, 0, 640, 16, 12, 20, 4, 80, 0, 4, 32, 3, 3, 0) != 0
    assert L.c2m_conv3x3_roi_tile(0, None, None) != 0
    # the ROI rule of both descriptors, checked before any launch: fake (non-null, 16-byte aligned) pointers are never read
    INVALID_ARG, UNSUPPORTED, fake = 1, 2, 0x1000
    _lib = c2m_amd._lib
    assert {"roi_tiles_y", "roi_tiles_x"} <= {n for n, _ in _lib.Conv3x3Desc._fields_}
    d = _lib.Conv3x3Desc(B=1, H=16, W=64, Cin=32, Cout=32, nsrc=1, wr=fake, out=fake, out_pix_pitch=32, out_row_pitch=32 * 64,
                         out_img_pitch=32 * 64 * 16, algo=5)
    d.src[0] = _lib.ConvSrc(ptr=fake, C=32, pix_pitch=32, row_pitch=32 * 64, img_pitch=32 * 64 * 16)
    r = _lib.Conv3x3Rgb64Desc(image=fake, B=1, H=16, W=64, weight=fake, out=fake, out_pix_pitch=64, out_row_pitch=64 * 64,
                              out_img_pitch=64 * 64 * 16)
    for roi in ((1, 0), (0, 1), (-1, 1), (1, -1), (-1, -1)):
        d.roi_tiles_y, d.roi_tiles_x = r.roi_tiles_y, r.roi_tiles_x = roi
        assert L.c2m_conv3x3_nhwc_f32(None, d) == INVALID_ARG, roi
        assert L.c2m_conv3x3_rgb64_f32(None, r) == INVALID_ARG, roi
    d.roi_tiles_y, d.roi_tiles_x = r.roi_tiles_y, r.roi_tiles_x = 100, 1     # larger than the full grid
    assert L.c2m_conv3x3_nhwc_f32(None, d) == INVALID_ARG and L.c2m_conv3x3_rgb64_f32(None, r) == INVALID_ARG
    d.roi_tiles_y, d.roi_tiles_x, d.algo = 1, 1, 0                            # C2M_CONV_DIRECT has no ROI launch
    assert L.c2m_conv3x3_nhwc_f32(None, d) == UNSUPPORTED
    assert L.c2m_conv3x3_nhwc_f32(None, None) == INVALID_ARG and L.c2m_conv3x3_rgb64_f32(None, None) == INVALID_ARG
    # the fused DCNv2 forward: no descriptor, and an arithmetic it does not have
    assert L.c2m_dcn_v2_forward_nhwc(None, None) == INVALID_ARG
    g = _lib.DcnNhwcDesc(B=1, C=64, H=8, W=8, Co=64, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dh=1, dw=1, dg=8, input_bordered=fake,
                         wt=fake, bias=fake, offset=fake, mask=fake, output=fake, arith=2)
    assert L.c2m_dcn_v2_forward_nhwc(None, g) == INVALID_ARG
