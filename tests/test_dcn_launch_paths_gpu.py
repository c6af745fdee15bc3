"""DCNv2 forward / backward on the launch paths that only larger maps, batches and channel counts select (the shapes of
tests/test_dcn_gpu.py flip none of these switches):

  group 1  the 8 x 4 pixel patch per wave (`tile2d`) of dcn_fwd_nhwc_kernel and dcn_bwd_offmask_kernel, next to sizes
           that must keep the row mapping;
  group 2  the k-tile split over grid.z of dcn_bwd_data_kernel / dcn_bwd_offmask_kernel with more than one tile per z
           block, a short last block and empty blocks;
  group 3  the chunk loop of dcn_bwd_weight_kernel iterating, across samples and over ragged chunks;
  group 4  forward instantiations no other test launches (eight groups per weight chunk, Co > 256).

Every input is a per-pixel random offset / mask field with a band of far out-of-range samples.  Small shapes are compared
with the C oracle at the tolerances of tests/test_dcn_gpu.py; the larger ones (groups 2 and 3; the oracle would take far
too long) with torch_port.dcn_v2_reference in float64 on the device and its autograd gradients, at the same 1e-4 rule,
after one test has shown that this reference and the oracle agree.  The host's launch rules are restated below and every
parametrised shape asserts, through them, the property it is here for."""
import contextlib
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_S1, _P1 = (1, 1), (1, 1)
GRADS = ("grad_input", "grad_offset", "grad_mask", "grad_weight", "grad_bias")


# ---------------------------------------------------------------------------------------------------------------------
# The host's launch rules (c2-matching_amd/csrc/dcn_v2.hip), restated.  THESE ARE COPIES: when a rule changes in the host
# code the restatement has to follow, or the shapes below stop asserting what they are here for.
# ---------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def tile2d(Ho, Wo):
    """8 x 4 pixel patch per wave instead of 32 consecutive pixels: dcn_fwd_nhwc_kernel (`const bool tile2d = ...`) and
    dcn_bwd_offmask_kernel (`if ((g.Wo % 8 == 0) && (g.Ho % 4 == 0))`)."""
    return Wo % 8 == 0 and Ho % 4 == 0


def z_split(B, C, HWo, taps=9):
    """-> (nkt, nz, kt_per, live z blocks) of the two backward data kernels.  c2m_dcn_v2_backward_f32: `nkt = g.KtotPad /
    32`, `nz = ceil_div(2048, ceil_div(HWo, 128) * B)` clamped to [1, nkt] = grid.z; the kernels: `kt_per = (nkt +
    gridDim.z - 1) / gridDim.z`, block z runs tiles [z * kt_per, min(nkt, (z + 1) * kt_per))."""
    nkt = _cdiv(C * taps, 32)
    nz = min(max(_cdiv(2048, _cdiv(HWo, 128) * B), 1), nkt)
    kt_per = _cdiv(nkt, nz)
    return nkt, nz, kt_per, _cdiv(nkt, kt_per)


def weight_split(B, C, HWo, taps=9):
    """-> (chunks per sample, chunks in all, nsplit) of dcn_bwd_weight_kernel.  c2m_dcn_v2_backward_f32: `chunks_per_b =
    ceil_div(HWo, dcn::PCH)` (PCH = 64 pixels), `nsplit = ceil_div(1024, nkt)` capped at `B * chunks_per_b` = grid.y; block
    y runs chunks y, y + nsplit, y + 2 nsplit, ..."""
    chunks_per_b = _cdiv(HWo, 64)
    total = B * chunks_per_b
    return chunks_per_b, total, min(_cdiv(1024, _cdiv(C * taps, 32)), total)


def bwd_select(C, dg, Co):
    """Kernels of c2m_dcn_v2_backward_f32.  bwd_ws(): `nhwc` = channels-last offset/mask kernel (without grad_input) and
    weight kernel <MT, true>; copad2(): COH = CoPad2 / 2 of both data kernels; weight kernel MT = CoPad / 32."""
    cpg = C // dg
    copad2 = 64 if Co <= 64 else 128 if Co <= 128 else 256
    return {"nhwc": cpg in (8, 16, 32) and C % 32 == 0, "cpg": cpg, "coh": copad2 // 2, "mt": _cdiv(Co, 32)}


def fwd_select(C, dg, Co, arith):
    """The dcn_fwd_nhwc_kernel instantiation of a forward on arithmetic "fp32" / "bf16" / "f16x2", or None where the
    geometry has none (NCHW kernel; the reduced arithmetics need 16 channels per -- possibly virtual -- group).  use_nhwc()
    without its 2 GiB limits, kernel_geom(), fwd_mt() / copad_fwd(), fwd_nhwc_has() and the `gc` rule of select_fwd_nhwc();
    `zblocks` = grid.z of launch_fwd_nhwc().  The refusal of the reduced arithmetics below 16 channels per group is not in
    select_fwd_nhwc(): it copies f16x2_geom() (`kernel_geom(g).CPG >= 16`, what ops.dcn_f16x2_ok reports) and dcn_forward()
    (`bf16 = want_bf16 && nhwc && gk.CPG >= 16`: such a call computes in fp32)."""
    cpg = C // dg
    if cpg not in (8, 16, 32) or dg % 2 != 0:
        return None
    split = cpg == 8 and dg % 4 == 0
    if split:
        cpg, dg = 16, dg // 2
    if arith != "fp32" and cpg < 16:
        return None
    need = _cdiv(Co, 32)
    mt = 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8
    copad = _cdiv(Co, mt * 32) * mt * 32
    if mt == 8 and not (arith != "fp32" and cpg == 32):
        mt = 4
    fit = (64 if mt == 8 else 32) * 1024 // (cpg * mt * 32 * (2 if arith == "bf16" else 4))
    gc = 8 if fit >= 8 and dg % 8 == 0 else 4 if fit >= 4 and dg % 4 == 0 else 2
    return {"cpg": cpg, "split": split, "mt": mt, "gc": gc, "copad": copad, "zblocks": copad // (mt * 32)}


# ---------------------------------------------------------------------------------------------------------------------
# inputs, references, comparisons
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env(dev):
    import c2m_amd
    import c2m_oracle as oracle
    import synth
    yield c2m_amd.ops, oracle, synth
    for cache in (_inputs, _small, _large):   # the shared references live as long as this module's tests
        cache.cache_clear()
    torch.cuda.empty_cache()


def _t(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(dev)   # (a copy: the shared references stay read-only)


def _out_size(H, W, st):
    return (H + 2 - 3) // st[0] + 1, (W + 2 - 3) // st[1] + 1


def _case(synth, B, C, H, W, Co, st, dg, seed, off_scale=3.0):
    """3x3 / pad 1 inputs in the style of test_dcn_gpu._case: per-pixel random offsets and masks, output row 0 a band of far
    out-of-range samples (+40 is beyond every input used with it), integer row coordinates on the last row."""
    Ho, Wo = _out_size(H, W, st)
    assert H <= 40 - 1 - 3.5 * off_scale   # |gaussish| < 3.47: the band's row coordinate is beyond the input
    x = synth.gaussish((B, C, H, W), seed)
    w = (synth.gaussish((Co, C, 3, 3), seed + 1) * (1.0 / np.sqrt(C * 9))).astype(np.float32)
    b = synth.gaussish((Co,), seed + 2)
    off = synth.gaussish((B, 18 * dg, Ho, Wo), seed + 3) * off_scale
    off[:, :, 0, :] += 40.0
    off[:, 0::2, -1, :] = np.round(off[:, 0::2, -1, :])
    msk = synth.uniform((B, 9 * dg, Ho, Wo), seed + 4, 0.0, 1.0)
    go = synth.gaussish((B, Co, Ho, Wo), seed + 5)
    return x, w, b, off, msk, go


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _inputs(B, C, H, W, Co, st, dg, off_scale):
    import synth
    return _frozen(*_case(synth, B, C, H, W, Co, st, dg, 900, off_scale))


@functools.lru_cache(maxsize=None)
def _small(B, C, H, W, Co, st, dg, kind):
    """-> (x, w, b, off, msk), grad_output, the oracle's result `kind` ("fwd", "bf16" or "bwd") of a small shape, each
    computed once per module and read-only.  The backward draws offsets of scale 2, the forwards of scale 3, as the cases of
    test_dcn_gpu.py do."""
    import c2m_oracle as oracle
    *inp, go = _inputs(B, C, H, W, Co, st, dg, 2.0 if kind == "bwd" else 3.0)
    if kind == "bwd":
        res = _frozen(*oracle.dcn_v2_backward(*inp, go, st, _P1, _S1, dg))
    else:
        fn = oracle.dcn_v2_forward if kind == "fwd" else oracle.dcn_v2_forward_bf16
        res, = _frozen(fn(*inp, st, _P1, _S1, dg))
    return tuple(inp), go, res


def _kinkfree_inputs(dev, B, C, H, W, Co, dg, seed):
    """Inputs for the float64 reference: offsets integer + uniform(0.1, 0.9), so that no sample sits on a bilinear kink
    (where one-sided derivatives differ by convention) nor on the in-range limit; output row 0 is displaced beyond the map
    in both coordinates, row 1 beyond it on the other side."""
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((B, C, H, W), generator=g, device=dev)
    w = torch.randn((Co, C, 3, 3), generator=g, device=dev) * (1.0 / math.sqrt(9 * C))
    b = torch.randn((Co,), generator=g, device=dev)
    off = torch.round(torch.randn((B, 18 * dg, H, W), generator=g, device=dev) * 2.0)
    off[:, :, 0, :] += float(H + W)
    off[:, :, 1, :] -= float(H + W)
    off += torch.rand((B, 18 * dg, H, W), generator=g, device=dev) * 0.8 + 0.1
    msk = torch.rand((B, 9 * dg, H, W), generator=g, device=dev)
    go = torch.randn((B, Co, H, W), generator=g, device=dev)
    return x, w, b, off, msk, go


def _ref64_grads(x, w, b, off, msk, go, dg):
    import torch_port
    args = [a.double().requires_grad_() for a in (x, w, b, off, msk)]
    out = torch_port.dcn_v2_reference(*args, _S1, _P1, _S1, dg=dg)
    gx, gw, gb, goff, gmsk = torch.autograd.grad(out, args, go.double())
    return out.detach(), (gx, goff, gmsk, gw, gb)


@functools.lru_cache(maxsize=None)
def _large(dev, B, C, H, W, Co, dg):
    """Inputs of a larger shape and the float64 gradients, computed once per module and shared by its cases."""
    inputs = _kinkfree_inputs(dev, B, C, H, W, Co, dg, 1000 + C + H)
    return inputs, _ref64_grads(*inputs, dg)[1]


def _check(name, got, want, rel):
    """|got - want|max <= rel * max(1, |want|max), the rule of test_dcn_gpu.py; prints the figure first.  NaN fails."""
    got = got if isinstance(got, torch.Tensor) else torch.from_numpy(np.array(got))
    want = (want if isinstance(want, torch.Tensor) else torch.from_numpy(np.array(want))).to(got.device)
    assert tuple(got.shape) == tuple(want.shape), name
    err, tol = float((got.double() - want.double()).abs().max()), rel * max(1.0, float(want.abs().max()))
    print(f"{name}: max err {err:.3e} (tolerance {tol:.3e})")
    assert err <= tol, f"{name}: max err {err} > {tol}"


def _check_bf16(got, want16):
    """The two bounds of test_forward_bf16_mma_matches_bf16_oracle against the oracle with the kernel's bf16 roundings."""
    got = got.cpu().numpy()
    rel16 = float(np.linalg.norm(got - want16) / np.linalg.norm(want16))
    err, tol = float(np.abs(got - want16).max()), 2e-3 * max(1.0, float(np.abs(want16).max()))
    print(f"bf16: rel16 {rel16:.3e} (bound 3e-4), max err {err:.3e} (bound {tol:.3e})")
    assert rel16 < 3e-4, f"bf16 MFMA forward vs bf16 oracle: {rel16}"
    assert err < tol


@contextlib.contextmanager
def _nan_prefilled_outputs():
    """ops.dcn_v2_backward takes its gradient tensors from torch.empty_like, and dcn_bwd_offmask_kernel writes grad_offset /
    grad_mask by plain stores into them, with no zero fill.  While this context is open those tensors start as NaN, so an
    element a kernel fails to write fails the comparison, whatever the allocator hands out.  Yields the list of tensors
    handed out, for the caller to see that its outputs were among them."""
    empty_like, made = torch.empty_like, []

    def nan_like(t, **kw):
        made.append(torch.full_like(t, float("nan"), **kw))
        return made[-1]

    torch.empty_like = nan_like
    try:
        yield made
    finally:
        torch.empty_like = empty_like


def _backward_vs(ops, inputs, want, st, dg, need_input_grad):
    """All returned gradients of one backward, into NaN-prefilled outputs, against `want`."""
    x, w, b, off, msk, go = inputs
    with _nan_prefilled_outputs() as made:
        got = ops.dcn_v2_backward(x, w, b, off, msk, go, st, 1, 1, dg, need_input_grad=need_input_grad)
    assert (got[0] is None) == (not need_input_grad)
    assert all(any(g_ is m for m in made) for g_ in got if g_ is not None)   # (the guard above saw every output)
    for name, g_, w_ in zip(GRADS, got, want):
        if g_ is not None:
            _check(name, g_, w_, 1e-4)


# ---------------------------------------------------------------------------------------------------------------------
# group 1: the 8 x 4 patch mapping, forward and backward
# ---------------------------------------------------------------------------------------------------------------------
# (C, dg, Co, stride) -> what fwd_select must say per arithmetic: (channels per kernel group, virtual groups, MT) or None
PATCH_GEOMS = {
    (64, 8, 64, 1): {"fp32": (16, True, 2), "bf16": (16, True, 2), "f16x2": (16, True, 2)},        # virtual 16-channel groups
    (128, 8, 128, 1): {"fp32": (16, False, 4), "bf16": (16, False, 4), "f16x2": (16, False, 4)},   # 16-channel groups
    (256, 8, 256, 1): {"fp32": (32, False, 4), "bf16": (32, False, 8), "f16x2": (32, False, 8)},   # 32; fp32 splits Co over z
    (48, 6, 24, 1): {"fp32": (8, False, 1), "bf16": None, "f16x2": None},                          # 8-channel groups unsplit
    (64, 2, 96, 2): {"fp32": (32, False, 4), "bf16": (32, False, 4), "f16x2": (32, False, 4)},     # 32-channel groups, stride 2
}
# output size -> (patch mapping, waves with pixels, workgroups)
PATCH_SIZES = {
    (4, 8): (True, 1, 1),      # one patch; three waves of the block lie past HWo and clamp their tile
    (8, 16): (True, 4, 1),     # exactly one workgroup
    (12, 24): (True, 9, 3),    # three patches per row; the last workgroup is partly idle
    (4, 12): (False, 2, 1),    # Wo % 8 != 0
    (6, 16): (False, 3, 1),    # Ho % 4 != 0
}
_PATCH_CASES = [(g, s) for g in PATCH_GEOMS for s in PATCH_SIZES]
_ids = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)   # noqa: E731


def _assert_patch_case(geom, size):
    C, dg, Co, _ = geom
    want_patch, waves, wgs = PATCH_SIZES[size]
    Ho, Wo = size
    assert tile2d(Ho, Wo) == want_patch
    assert _cdiv(Ho * Wo, 32) == waves and _cdiv(Ho * Wo, 128) == wgs
    for arith, want in PATCH_GEOMS[geom].items():
        sel = fwd_select(C, dg, Co, arith)
        assert (sel and (sel["cpg"], sel["split"], sel["mt"])) == want, (arith, sel)
    assert fwd_select(256, 8, 256, "fp32")["zblocks"] == 2 and fwd_select(256, 8, 256, "bf16")["zblocks"] == 1


@pytest.mark.parametrize("geom,size", _PATCH_CASES, ids=_ids)
def test_patch_forward_matches_oracle(env, dev, geom, size):
    """fp32 and bf16-MFMA forward at the geometry's own stride (the planar entry points)."""
    ops, _, _ = env
    C, dg, Co, s = geom
    st = (s, s)
    _assert_patch_case(geom, size)
    shape = (2, C, size[0] * s, size[1] * s, Co, st, dg)
    inp, _, want = _small(*shape, "fwd")
    assert want.shape[2:] == size
    args = [_t(a, dev) for a in inp]
    f32 = ops.dcn_v2_forward(*args, st, 1, 1, dg)
    _check("fp32 forward", f32, want, 2e-5)
    if PATCH_GEOMS[geom]["bf16"]:
        b16 = ops.dcn_v2_forward(*args, st, 1, 1, dg, bf16_mma=True)
        _check_bf16(b16, _small(*shape, "bf16")[2])
        assert not torch.equal(b16, f32)     # (it really ran the other arithmetic)


@pytest.mark.parametrize("geom,size", _PATCH_CASES, ids=_ids)
def test_patch_forward_nhwc_matches_oracle(env, dev, geom, size):
    """The fused path's entry point (stride 1 by its ABI, so the stride-2 geometry runs at stride 1 here): f16 x 2 forward,
    and the channels-last store with the fused lrelu."""
    ops, _, _ = env
    C, dg, Co, _ = geom
    _assert_patch_case(geom, size)
    inp, _, want = _small(2, C, size[0], size[1], Co, _S1, dg, "fwd")
    x, w, b, off, msk = (_t(a, dev) for a in inp)
    bo = ops.BorderedNHWC(x)
    cl = ops.dcn_v2_forward_nhwc(bo, w, b, off, msk, dg, act=ops.ACT_LRELU, slope=0.1, algo="fp32")
    _check("fp32 channels-last + lrelu", cl, np.where(want > 0, want, 0.1 * want), 2e-5)
    assert ops.dcn_f16x2_ok(w, dg) == (PATCH_GEOMS[geom]["f16x2"] is not None)
    if PATCH_GEOMS[geom]["f16x2"]:
        f16 = ops.dcn_v2_forward_nhwc(bo, w, b, off, msk, dg, nhwc_out=False, algo="f16x2")
        _check("f16x2 forward", f16, want, 2e-5)
        assert not torch.equal(f16, ops.dcn_v2_forward_nhwc(bo, w, b, off, msk, dg, nhwc_out=False, algo="fp32"))
        cl16 = ops.dcn_v2_forward_nhwc(bo, w, b, off, msk, dg, act=ops.ACT_LRELU, slope=0.1, algo="f16x2")
        _check("f16x2 channels-last + lrelu", cl16, np.where(want > 0, want, 0.1 * want), 2e-5)


@pytest.mark.parametrize("need_input_grad", [True, False], ids=["data", "offmask"])
@pytest.mark.parametrize("geom,size", _PATCH_CASES, ids=_ids)
def test_patch_backward_matches_oracle(env, dev, geom, size, need_input_grad):
    """All returned gradients, with grad_input (dcn_bwd_data_kernel, row mapping throughout) and without (channels-last
    geometries: dcn_bwd_offmask_kernel, which takes the patch mapping)."""
    ops, _, _ = env
    C, dg, Co, s = geom
    st = (s, s)
    _assert_patch_case(geom, size)
    assert bwd_select(C, dg, Co)["nhwc"] == (C != 48)
    inp, go, want = _small(2, C, size[0] * s, size[1] * s, Co, st, dg, "bwd")
    _backward_vs(ops, [_t(a, dev) for a in inp + (go,)], want, st, dg, need_input_grad)


# ---------------------------------------------------------------------------------------------------------------------
# the float64 reference of groups 2 and 3 against the oracle
# ---------------------------------------------------------------------------------------------------------------------
def test_float64_reference_agrees_with_oracle(env, dev):
    ops, oracle, _ = env
    B, C, H, W, Co, dg = 2, 32, 9, 11, 40, 4
    inputs = _kinkfree_inputs(dev, B, C, H, W, Co, dg, 77)
    out64, grads64 = _ref64_grads(*inputs, dg)
    x, w, b, off, msk, go = (a.cpu().numpy() for a in inputs)
    frac = off - np.floor(off)
    assert 0.09 < frac.min() and frac.max() < 0.91 and off[:, :, 0].min() > H + W - 10 and off[:, :, 1].max() < 10 - H - W
    assert float(np.ptp(off[:, :, 2:], axis=(2, 3)).min()) > 0 and float(np.ptp(msk, axis=(2, 3)).min()) > 0   # no uniform field
    _check("forward", out64, oracle.dcn_v2_forward(x, w, b, off, msk, _S1, _P1, _S1, dg), 1e-4)
    for name, g64, gor in zip(GRADS, grads64, oracle.dcn_v2_backward(x, w, b, off, msk, go, _S1, _P1, _S1, dg)):
        _check(name, g64, gor, 1e-4)


# ---------------------------------------------------------------------------------------------------------------------
# group 2: k tiles split over grid.z with more than one tile per block
# ---------------------------------------------------------------------------------------------------------------------
ZSPLIT = [
    # B, C, dg, Co, H, W -> nkt, nz, kt_per, live z blocks, the last live block is short, patch mapping; COH, weight MT
    ((4, 32, 4, 32, 64, 128), (9, 8, 2, 5, True, True), (32, 1)),     # z0..3 two tiles, z4 one, z5..7 none; 8-channel groups
    ((4, 32, 4, 32, 66, 125), (9, 8, 2, 5, True, False), (32, 1)),    # row mapping; 129 chunks per sample, the last with 58 pixels
    ((2, 96, 6, 96, 64, 80), (27, 26, 2, 14, True, True), (64, 3)),   # z13 short, z14..25 empty; 16-channel groups
    ((2, 96, 3, 40, 64, 80), (27, 26, 2, 14, True, True), (32, 2)),   # 32-channel groups, odd group count, o < Co guards
    ((2, 256, 8, 256, 40, 48), (72, 69, 2, 36, False, True), (128, 8)),   # z36 and above empty; nsplit 15 of 60 chunks
]


@pytest.mark.parametrize("need_input_grad", [True, False], ids=["data", "offmask"])
@pytest.mark.parametrize("shape,split,kern", ZSPLIT, ids=[_ids(c[0]) for c in ZSPLIT])
def test_backward_z_split_matches_float64(env, dev, shape, split, kern, need_input_grad):
    ops, _, _ = env
    B, C, dg, Co, H, W = shape
    nkt, nz, kt_per, live = z_split(B, C, H * W)[:4]
    assert (nkt, nz, kt_per, live, nkt % kt_per != 0, tile2d(H, W)) == split
    assert nz < nkt and kt_per > 1 and live < nz          # several tiles per z block, and z blocks without any
    sel = bwd_select(C, dg, Co)
    assert sel["nhwc"] and (sel["coh"], sel["mt"]) == kern
    if shape[:3] == (4, 32, 4):
        assert sel["cpg"] == 8 and weight_split(B, C, H * W)[0] == (129 if W == 125 else 128) and (H * W) % 64 == (58 if W == 125 else 0)
    if shape[:3] == (2, 96, 6):
        assert sel["cpg"] == 16
    if shape[:3] == (2, 96, 3):   # the backward takes the channels-last kernels, the forward the NCHW kernel
        assert sel["cpg"] == 32 and dg % 2 == 1 and Co % 32 != 0 and fwd_select(C, dg, Co, "fp32") is None
    if C == 256:
        assert weight_split(B, C, H * W)[1:] == (60, 15)
    inputs, want = _large(dev, B, C, H, W, Co, dg)
    _backward_vs(ops, inputs, want, _S1, dg, need_input_grad)


# ---------------------------------------------------------------------------------------------------------------------
# group 3: the weight gradient's chunk loop
# ---------------------------------------------------------------------------------------------------------------------
def _chunk_sequences(B, C, HWo):
    """What the blocks' chunk sequences of weight_split() contain: iteration counts, whether a sequence crosses into another
    sample, and where in a sequence the ragged (last of a sample, when HWo % 64 != 0) chunks sit."""
    per_b, total, nsplit = weight_split(B, C, HWo)
    iters, where, crosses = set(), set(), False
    for y in range(nsplit):
        seq = list(range(y, total, nsplit))
        iters.add(len(seq))
        crosses |= len({ch // per_b for ch in seq}) > 1
        for n, ch in enumerate(seq):
            if HWo % 64 != 0 and ch % per_b == per_b - 1:
                where.add("first" if n == 0 else "last" if n == len(seq) - 1 else "middle")
    return iters, where, crosses


WCHUNK = [
    # B, C, dg, Co, H, W -> chunks per sample, pixels of the last, chunks, nsplit; channels-last kernel, MT; ragged positions
    ((3, 256, 8, 256, 26, 26), (11, 36, 33, 15), (True, 8), {"first", "last"}),
    ((4, 256, 8, 256, 26, 26), (11, 36, 44, 15), (True, 8), {"first", "middle", "last"}),   # [6, 21, 36]: ragged between full ones
    ((3, 64, 8, 32, 50, 50), (40, 4, 120, 57), (True, 1), {"first", "last"}),    # MT = 1: four-way pixel-pair split
    ((3, 64, 8, 64, 50, 50), (40, 4, 120, 57), (True, 2), {"first", "last"}),    # MT = 2: two-way
    ((4, 48, 6, 24, 49, 49), (38, 33, 152, 74), (False, 1), {"first", "middle", "last"}),   # the planar <MT, false> loop
]


@pytest.mark.parametrize("shape,chunks,kern,ragged", WCHUNK, ids=[_ids(c[0]) for c in WCHUNK])
def test_backward_weight_chunk_loop_matches_float64(env, dev, shape, chunks, kern, ragged):
    """All five gradients; grad_weight is the point: every block runs two or three chunks (the register prefetch of chunk
    n + 1 is consumed), its sequence crosses samples, and a ragged chunk opens one sequence (full chunks of the next sample
    follow it) and closes another (full chunks precede it); with B = 4 at 26x26 one also sits between two full chunks."""
    ops, _, _ = env
    B, C, dg, Co, H, W = shape
    per_b, total, nsplit = weight_split(B, C, H * W)
    assert (per_b, H * W - (per_b - 1) * 64, total, nsplit) == chunks and nsplit < total
    sel = bwd_select(C, dg, Co)
    assert (sel["nhwc"], sel["mt"]) == kern
    iters, where, crosses = _chunk_sequences(B, C, H * W)
    assert iters == {2, 3} and crosses and where == ragged
    inputs, want = _large(dev, B, C, H, W, Co, dg)
    _backward_vs(ops, inputs, want, _S1, dg, True)


# ---------------------------------------------------------------------------------------------------------------------
# group 4: forward instantiations no other test selects
# ---------------------------------------------------------------------------------------------------------------------
FWD_LEFTOVERS = [
    # C, dg, Co -> arithmetics to run, what fwd_select must say for each
    ((128, 8, 64), {a: {"cpg": 16, "split": False, "mt": 2, "gc": 8} for a in ("fp32", "bf16", "f16x2")}),
    ((128, 16, 64), {a: {"cpg": 16, "split": True, "mt": 2, "gc": 8} for a in ("fp32", "bf16", "f16x2")}),   # virtual groups
    ((256, 8, 24), {a: {"cpg": 32, "split": False, "mt": 1, "gc": 8} for a in ("fp32", "bf16", "f16x2")}),
    ((256, 8, 64), {"bf16": {"cpg": 32, "split": False, "mt": 2, "gc": 8}}),                # (fp32 gets GC = 4 there)
    # fp32: z blocks 2 (partly) and 3 (wholly) lie past Co; reduced arithmetics: MT = 8 with CoPad = 512
    ((64, 2, 288), {"fp32": {"cpg": 32, "mt": 4, "gc": 2, "copad": 512, "zblocks": 4},
                    "bf16": {"cpg": 32, "mt": 8, "gc": 2, "copad": 512, "zblocks": 2},
                    "f16x2": {"cpg": 32, "mt": 8, "gc": 2, "copad": 512, "zblocks": 2}}),
]


@pytest.mark.parametrize("size", [(9, 11), (8, 16)], ids=_ids)
@pytest.mark.parametrize("geom,ariths", FWD_LEFTOVERS, ids=[_ids(c[0]) for c in FWD_LEFTOVERS])
def test_forward_selection_leftovers_match_oracle(env, dev, geom, ariths, size):
    ops, _, _ = env
    C, dg, Co = geom
    for arith, want in ariths.items():
        sel = fwd_select(C, dg, Co, arith)
        assert sel is not None and {k: sel[k] for k in want} == want, (arith, sel)
    assert fwd_select(256, 8, 64, "fp32")["gc"] == 4
    assert tile2d(*size) == (size == (8, 16))
    if Co == 288:
        assert (fwd_select(C, dg, Co, "fp32")["zblocks"] - 1) * 128 >= Co
    shape = (2, C, size[0], size[1], Co, _S1, dg)
    inp, _, want = _small(*shape, "fwd")
    x, w, b, off, msk = (_t(a, dev) for a in inp)
    f32 = ops.dcn_v2_forward(x, w, b, off, msk, 1, 1, 1, dg)
    if "fp32" in ariths:
        _check("fp32 forward", f32, want, 2e-5)
    if "bf16" in ariths:
        b16 = ops.dcn_v2_forward(x, w, b, off, msk, 1, 1, 1, dg, bf16_mma=True)
        _check_bf16(b16, _small(*shape, "bf16")[2])
        assert not torch.equal(b16, f32)
    if "f16x2" in ariths:
        assert ops.dcn_f16x2_ok(w, dg)
        f16 = ops.dcn_v2_forward_nhwc(ops.BorderedNHWC(x), w, b, off, msk, dg, nhwc_out=False, algo="f16x2")
        _check("f16x2 forward", f16, want, 2e-5)
        assert not torch.equal(f16, f32)
