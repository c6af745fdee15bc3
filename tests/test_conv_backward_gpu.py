"""GPU tests of the hand-written conv3x3 backward at the sizes and edges that select its code paths: the weight gradient
(csrc/conv3x3_wgrad.hip through ops.conv3x3_wgrad), the data gradient (ops.conv3x3_dgrad: the bf16 x 3 split kernel on the
kind-5 weight image) and the autograd function that joins them (ops._Conv3x3Fn).

The reference everywhere is float64 torch.autograd through F.conv2d(torch.cat(srcs, 1), w, b, padding=1) on the same
device, fed the float32 inputs converted to float64; the error of a gradient tensor is max|got - want| / max|want|."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")


@pytest.fixture(scope="module")
def ops(dev):
    import c2m_amd
    return c2m_amd.ops


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(shape, generator=g, device=dev) * scale


def _relerr(got, want):
    return float((got.double() - want).abs().max()) / max(1e-300, float(want.abs().max()))


def _ref_grads(xs, w, gy, dtype=torch.float64):
    """(grad_weight, grad of cat(xs)) of conv2d(cat(xs), w, padding=1) under grad_out = gy, by torch.autograd in `dtype`."""
    x = torch.cat([x_.detach().to(dtype) for x_ in xs], 1).contiguous().requires_grad_(True)
    w_ = w.detach().to(dtype).requires_grad_(True)
    F.conv2d(x, w_, None, padding=1).backward(gy.detach().to(dtype).contiguous())
    return w_.grad, x.grad


def _ref_wgrad(xs, gy):
    """float64 weight gradient alone (the weight's values do not enter it)."""
    x = torch.cat([x_.detach().double() for x_ in xs], 1).contiguous()
    w_ = torch.zeros((gy.shape[1], x.shape[1], 3, 3), dtype=torch.float64, device=x.device, requires_grad=True)
    F.conv2d(x, w_, None, padding=1).backward(gy.detach().double().contiguous())
    return w_.grad


def _ref_dgrad(gy, w):
    """float64 data gradient alone (the input's values do not enter it)."""
    B, _, H, W = gy.shape
    x = torch.zeros((B, w.shape[1], H, W), dtype=torch.float64, device=gy.device, requires_grad=True)
    F.conv2d(x, w.detach().double(), None, padding=1).backward(gy.detach().double().contiguous())
    return x.grad


def _policy(B, cins, Cout, H, W):
    """The weight-gradient launch geometry, from the library's own workspace size (a host call, no launch)."""
    import c2m_amd
    Cin = sum(cins)
    nbytes = c2m_amd.lib().c2m_conv3x3_wgrad_workspace_bytes(B, H, W, Cin, Cout)
    per_image = Cout * Cin * 9 * 4
    assert nbytes > 0 and nbytes % per_image == 0
    nslice = nbytes // per_image
    segs_x = (W + 31) // 32
    nseg = B * H * segs_x
    blocks = (Cin // 32) * ((Cout + 63) // 64)
    return dict(nslice=nslice, segs_x=segs_x, nseg=nseg, blocks=blocks, per_slice=-(-nseg // nslice), nbytes=nbytes,
                by_blocks=-(-768 // blocks), by_nseg=(nseg + 7) // 8, rows=H * segs_x)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the two linear operators at product size
# ---------------------------------------------------------------------------------------------------------------------
PRODUCT_B = 32
PRODUCT_CASES = [
    # layer of ref_restoration_arch.py, [Cin per source], Cout, H, W      (configs[3] at the global batch: 32 pairs, LR 40)
    ("body_conv", [64], 64, 40, 40),
    ("small_offset_conv1", [64, 256], 256, 40, 40),
    ("small_offset_conv2", [256], 256, 40, 40),
    ("head_small", [64, 256], 64, 40, 40),
    ("small_dcn_head", [256], 216, 40, 40),
    ("medium_offset_conv1", [64, 128], 128, 80, 80),
    ("upsample_conv", [64], 256, 80, 80),
    ("large_offset_conv1", [64, 64], 64, 160, 160),
    ("large_dcn_head", [64], 216, 160, 160),
    ("tail_conv", [64], 32, 160, 160),
]


@pytest.mark.parametrize("case", PRODUCT_CASES, ids=[c[0] for c in PRODUCT_CASES])
def test_wgrad_and_dgrad_at_product_size(ops, dev, case):
    """ops.conv3x3_wgrad and ops.conv3x3_dgrad called directly (linear in grad_out: no activation kink) on the shapes at
    which RestorationNet chooses them, against float64.  The bar follows the reference, not the kernels: the stock float32
    backward (MIOpen, what the product falls back to) is measured against float64 on the same inputs inside the test and
    the hand-written kernel is held to max(1e-5, 2 x that) -- both are fp32 accumulations of the same terms in different
    orders, a lost segment / halo column / slice is off by 1e-3 or more.  A 216-channel head's data gradient is called
    as _Conv3x3Fn calls it (zero-padded to 224 channels).

    Measured on an MI355X (table per shape in DESIGN.md 6.4): weight gradient e_kernel 5.3e-7 ... 1.8e-6 against e_stock
    5.8e-7 ... 4.2e-6, data gradient e_kernel 7.2e-7 ... 2.2e-6 against e_stock 3.0e-7 ... 7.5e-7 -- the 1e-5 floor of the
    bar is what binds on every shape."""
    name, cins, Cout, H, W = case
    B, Cin = PRODUCT_B, sum(cins)
    xs = [_cl(_rand((B, c, H, W), dev, 1000 + k)) for k, c in enumerate(cins)]
    gy = _cl(_rand((B, Cout, H, W), dev, 1010, 1.0 / math.sqrt(B * H * W)))
    w = _rand((Cout, Cin, 3, 3), dev, 1011, 1.0 / math.sqrt(9 * Cin))
    pol = _policy(B, cins, Cout, H, W)
    got_w = ops.conv3x3_wgrad(xs, gy, Cout)
    if Cout % 16 != 0:
        pad = 16 - Cout % 16
        got_x = ops.conv3x3_dgrad(_cl(F.pad(gy, (0, 0, 0, 0, 0, pad))), F.pad(w, (0, 0, 0, 0, 0, 0, 0, pad)))
    else:
        got_x = ops.conv3x3_dgrad(gy, w)
    assert tuple(got_w.shape) == (Cout, Cin, 3, 3) and tuple(got_x.shape) == (B, Cin, H, W)
    stock_w, stock_x = _ref_grads(xs, w, gy, torch.float32)
    want_w, want_x = _ref_grads(xs, w, gy, torch.float64)
    ek_w, es_w = _relerr(got_w, want_w), _relerr(stock_w, want_w)
    ek_x, es_x = _relerr(got_x, want_x), _relerr(stock_x, want_x)
    print(f"\nPRODUCT {name} {cins}->{Cout} {B}x{H}x{W} nslice={pol['nslice']} per_slice={pol['per_slice']} "
          f"wgrad e_kernel={ek_w:.3e} e_stock={es_w:.3e} | dgrad e_kernel={ek_x:.3e} e_stock={es_x:.3e}")
    del xs, gy, stock_w, stock_x, want_w, want_x, got_w, got_x
    torch.cuda.empty_cache()
    assert ek_w < max(1e-5, 2.0 * es_w), ("grad_weight", ek_w, es_w)
    assert ek_x < max(1e-5, 2.0 * es_x), ("dx", ek_x, es_x)


def test_product_shapes_reach_the_384_slice_bound(dev):
    p = _policy(PRODUCT_B, [64], 32, 160, 160)                              # tail_conv: 2 blocks
    assert p["nslice"] == 384 == p["by_blocks"] < p["by_nseg"]
    assert p["nslice"] * p["per_slice"] - p["nseg"] >= p["per_slice"]       # ... with an empty trailing slice
    assert _policy(PRODUCT_B, [64, 256], 64, 40, 40)["blocks"] == 10 and _policy(PRODUCT_B, [256], 256, 40, 40)["blocks"] == 32


# ---------------------------------------------------------------------------------------------------------------------
# 2. the slice policy, made visible
# ---------------------------------------------------------------------------------------------------------------------
POLICY_CASES = {
    # name: (B, [Cin per source], Cout, H, W)
    "one_slice": (2, [32], 32, 4, 32),                   # 8 segments
    "nseg_bound": (2, [64], 64, 40, 40),                 # 160 segments / 8 = 20 slices of a possible 384
    "blocks_bound_384": (32, [64], 64, 100, 8),          # 3 200 segments, 2 blocks: 768 / 2 = 384 slices of 9 (28 of them empty)
    # an empty trailing slice needs nslice * per_slice - nseg >= per_slice; under the (nseg + 7) / 8 bound that cannot
    # happen (per_slice <= 8 and the shortfall is < 8), so it takes the 768 / blocks bound: 40 blocks -> 20 slices,
    # 161 = 7 * 23 segments -> per_slice 9, slices 18 and 19 start past the last segment
    "empty_trailing_slice": (7, [64, 256], 256, 23, 20),
    "many_blocks_few_slices": (8, [64, 256], 64, 40, 40),   # 10 blocks -> 77 slices of 9 for 640 segments
    "boundary_inside_a_row": (2, [64], 64, 11, 70),      # 3 segments per row, slices of 8
    "boundary_between_images": (4, [32], 32, 8, 32),     # slices of 8 segments = one image each
    "slice_spans_two_images": (3, [32], 32, 5, 31),      # slices of 8 segments over images of 5
}
POLICY_CHECKS = {
    "one_slice": lambda p: p["nslice"] == 1,
    "nseg_bound": lambda p: 1 < p["nslice"] == p["by_nseg"] < p["by_blocks"],
    "blocks_bound_384": lambda p: p["nslice"] == 384 == p["by_blocks"] < p["by_nseg"],
    "empty_trailing_slice": lambda p: p["nslice"] * p["per_slice"] - p["nseg"] >= p["per_slice"],
    "many_blocks_few_slices": lambda p: p["blocks"] == 10 and p["nslice"] == 77 == p["by_blocks"] < p["by_nseg"],
    "boundary_inside_a_row": lambda p: p["nslice"] > 1 and p["segs_x"] >= 2 and p["per_slice"] % p["segs_x"] != 0,
    "boundary_between_images": lambda p: p["nslice"] > 1 and p["per_slice"] % p["rows"] == 0,
    "slice_spans_two_images": lambda p: p["nslice"] > 1 and p["per_slice"] % p["rows"] != 0 and p["per_slice"] > p["rows"],
}


@pytest.mark.parametrize("name", list(POLICY_CASES))
def test_wgrad_slice_policy_cases(ops, dev, name):
    """Each regime of wgrad_slices / per_slice, asserted from c2m_conv3x3_wgrad_workspace_bytes (slice count = bytes /
    (Cout Cin 9 4)), then run against float64 at the small tests' 1e-5."""
    B, cins, Cout, H, W = POLICY_CASES[name]
    p = _policy(B, cins, Cout, H, W)
    assert POLICY_CHECKS[name](p), p
    xs = [_cl(_rand((B, c, H, W), dev, 1100 + k)) for k, c in enumerate(cins)]
    gy = _cl(_rand((B, Cout, H, W), dev, 1110))
    got = ops.conv3x3_wgrad(xs, gy, Cout)
    err = _relerr(got, _ref_wgrad(xs, gy))
    print(f"\nPOLICY {name} {p} err={err:.3e}")
    assert err < 1e-5, (name, err)


# ---------------------------------------------------------------------------------------------------------------------
# 3. geometry edges of the weight gradient
# ---------------------------------------------------------------------------------------------------------------------
EDGE_HW = [(1, 1), (1, 40), (40, 1), (2, 32), (3, 33), (5, 31), (2, 65)]


@pytest.mark.parametrize("H,W", EDGE_HW)
def test_wgrad_geometry_edges_with_images_of_different_magnitude(ops, dev, H, W):
    """B = 3: every segment row has a neighbour image before and after it in the flattened (b, y, segment) walk.  The
    images differ by 1e3 and 1e-3 in magnitude, and each image's contribution is checked on its own -- in the batch-of-3
    launch (grad_out zero on the other two images) and as a batch-of-1 launch, the three of them summed in float64 -- so
    a halo row taken from the neighbouring image shows at full scale."""
    B, C, Co = 3, 64, 64
    mag = torch.tensor([1.0, 1e3, 1e-3], device=dev).view(3, 1, 1, 1)
    x = _cl(_rand((B, C, H, W), dev, 1200) * mag)
    gy = _cl(_rand((B, Co, H, W), dev, 1201))
    want_all = _ref_wgrad([x], gy)
    err = _relerr(ops.conv3x3_wgrad([x], gy, Co), want_all)
    assert err < 1e-5, ("batch", err)
    total = torch.zeros_like(want_all)
    for b in range(B):
        want_b = _ref_wgrad([x[b:b + 1]], gy[b:b + 1])
        g_only = torch.zeros_like(gy)
        g_only[b] = gy[b]
        err = _relerr(ops.conv3x3_wgrad([x], g_only, Co), want_b)
        assert err < 1e-5, ("image in the batch", b, err)
        one = ops.conv3x3_wgrad([x[b:b + 1]], gy[b:b + 1], Co)
        err = _relerr(one, want_b)
        assert err < 1e-5, ("image alone", b, err)
        total += one.double()
    assert _relerr(total, want_all) < 1e-5


@pytest.mark.parametrize("Cout", [6, 10, 30, 70])
def test_wgrad_cout_not_a_multiple_of_4_reads_the_scalar_tail(ops, dev, Cout):
    """grad_out as a channel slice (start and pixel pitch multiples of 4) of a wider channels-last tensor whose other
    channels are NaN: the last channel quad of the slice is loaded element by element (Cout = 70: a second, mostly empty
    64-cout block)."""
    B, C, H, W = 2, 32, 9, 37
    x = _cl(_rand((B, C, H, W), dev, 1300))
    wide = _cl(torch.full((B, 80, H, W), NAN, device=dev))
    gy = wide[:, 4:4 + Cout]
    gy.copy_(_rand((B, Cout, H, W), dev, 1301))
    assert gy.data_ptr() % 16 == 0 and gy.stride(3) % 4 == 0 and gy.stride(1) == 1
    got = ops.conv3x3_wgrad([x], gy, Cout)
    assert bool(torch.isfinite(got).all())
    err = _relerr(got, _ref_wgrad([x], gy))
    assert err < 1e-5, err


def test_wgrad_sources_as_views(ops, dev):
    """A channel slice between NaN channels; the interior of a bordered buffer whose border is NaN (zero padding comes
    from the predicate, never from memory); two sources of unequal width, both orders."""
    B, H, W, Co = 2, 13, 37, 64
    gy = _cl(_rand((B, Co, H, W), dev, 1400))
    big = _cl(torch.full((B, 128, H, W), NAN, device=dev))
    x = big[:, 32:96]
    x.copy_(_rand((B, 64, H, W), dev, 1401))
    got = ops.conv3x3_wgrad([x], gy, Co)
    assert bool(torch.isfinite(got).all()) and _relerr(got, _ref_wgrad([x], gy)) < 1e-5
    bo = ops._bordered_empty(B, 64, H, W, dev)
    bo.buf.fill_(NAN)
    xb = bo.interior()
    xb.copy_(x)
    got_b = ops.conv3x3_wgrad([xb], gy, Co)
    assert torch.equal(got_b, got)
    for cins in ([32, 96], [96, 32]):
        xs = [_cl(_rand((B, c, H, W), dev, 1410 + k)) for k, c in enumerate(cins)]
        got = ops.conv3x3_wgrad(xs, gy, Co)
        assert tuple(got.shape) == (Co, 128, 3, 3) and _relerr(got, _ref_wgrad(xs, gy)) < 1e-5, cins


def test_wgrad_rejects_bad_arguments_before_launch(ops, dev):
    """Host-side argument checks: a 48-channel source (32-channel blocks), a grad_out slice whose pointer is not 16-byte
    aligned, a grad_out of the wrong shape."""
    import c2m_amd
    B, H, W = 1, 6, 10
    gy = _cl(_rand((B, 64, H, W), dev, 1500))
    with pytest.raises(c2m_amd.C2MError):
        ops.conv3x3_wgrad([_cl(_rand((B, 48, H, W), dev, 1501))], gy, 64)
    x = _cl(_rand((B, 32, H, W), dev, 1502))
    wide = _cl(_rand((B, 72, H, W), dev, 1503))
    with pytest.raises(c2m_amd.C2MError):
        ops.conv3x3_wgrad([x], wide[:, 2:66], 64)
    with pytest.raises(c2m_amd.C2MError):
        ops.conv3x3_wgrad([x], gy, 32)
    with pytest.raises(c2m_amd.C2MError):
        ops.conv3x3_wgrad([x], _cl(_rand((B, 64, H, W + 1), dev, 1504)), 64)
    torch.cuda.synchronize(dev)


# ---------------------------------------------------------------------------------------------------------------------
# 4. determinism and the workspace
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,case", [("384_slices", POLICY_CASES["blocks_bound_384"]), ("two_sources", (2, [64, 64], 64, 33, 70))])
def test_wgrad_is_deterministic_and_reads_only_what_it_wrote(ops, dev, name, case):
    """Two calls give the same bits; and after the allocator's free blocks of exactly the workspace's and the result's
    sizes have been filled with NaN (torch.empty hands them out again) the bits are still the same, i.e. every element of
    the workspace that the reduce reads and every element of grad_weight was written by this launch."""
    B, cins, Cout, H, W = case
    p = _policy(B, cins, Cout, H, W)
    if name == "384_slices":
        assert p["nslice"] == 384
    xs = [_cl(_rand((B, c, H, W), dev, 1600 + k)) for k, c in enumerate(cins)]
    gy = _cl(_rand((B, Cout, H, W), dev, 1610))
    first = ops.conv3x3_wgrad(xs, gy, Cout)
    again = ops.conv3x3_wgrad(xs, gy, Cout)
    assert bool(torch.isfinite(first).all()) and torch.equal(first, again)
    del again
    poison = [torch.full((p["nbytes"] // 4,), NAN, dtype=torch.float32, device=dev) for _ in range(2)]
    poison += [torch.full((Cout, sum(cins), 3, 3), NAN, dtype=torch.float32, device=dev) for _ in range(2)]
    ptrs = {t.data_ptr() for t in poison}
    torch.cuda.synchronize(dev)
    del poison
    third = ops.conv3x3_wgrad(xs, gy, Cout)
    assert torch.equal(first, third)
    print(f"\nPOISON {name}: grad_weight landed on a poisoned block: {third.data_ptr() in ptrs}")


# ---------------------------------------------------------------------------------------------------------------------
# 5. data gradient edges
# ---------------------------------------------------------------------------------------------------------------------
DGRAD_CHANNELS = [(64, 64), (16, 32), (224, 256), (64, 320)]     # Cout -> Cin


@pytest.mark.parametrize("H,W", EDGE_HW)
def test_dgrad_geometry_edges(ops, dev, H, W):
    B = 3
    for Cout, Cin in DGRAD_CHANNELS:
        gy = _cl(_rand((B, Cout, H, W), dev, 1700))
        w = _rand((Cout, Cin, 3, 3), dev, 1701, 1.0 / math.sqrt(9 * Cout))
        got = ops.conv3x3_dgrad(gy, w)
        assert tuple(got.shape) == (B, Cin, H, W)
        err = _relerr(got, _ref_dgrad(gy, w))
        assert err < 1e-5, (Cout, Cin, err)


def test_dgrad_grad_out_as_a_channel_slice(ops, dev):
    B, H, W = 2, 11, 37
    wide = _cl(torch.full((B, 128, H, W), NAN, device=dev))
    gy = wide[:, 16:80]
    gy.copy_(_rand((B, 64, H, W), dev, 1710))
    w = _rand((64, 96, 3, 3), dev, 1711, 1.0 / 24.0)
    got = ops.conv3x3_dgrad(gy, w)
    assert bool(torch.isfinite(got).all()) and _relerr(got, _ref_dgrad(gy, w)) < 1e-5


def test_dgrad_weight_image_follows_data_writes(ops, dev):
    """The kind-5 (rotated / transposed) weight image alone in the cache: after a `.data` write (no version bump) plus
    ops.refresh_weight_caches the data gradient follows the new weights and equals a cold-cache call bit for bit."""
    ops.clear_weight_caches()
    gy = _cl(_rand((2, 64, 12, 40), dev, 1720))
    w = torch.nn.Parameter(_rand((64, 96, 3, 3), dev, 1721, 1.0 / 24.0))
    before = ops.conv3x3_dgrad(gy, w)
    assert _relerr(before, _ref_dgrad(gy, w)) < 1e-5
    v0 = w._version
    w.data.mul_(-1.7).add_(_rand((64, 96, 3, 3), dev, 1722, 0.01))
    assert w._version == v0
    assert ops.refresh_weight_caches([w]) >= 1
    after = ops.conv3x3_dgrad(gy, w)
    assert not torch.equal(after, before)
    assert _relerr(after, _ref_dgrad(gy, w)) < 1e-5
    ops.clear_weight_caches()
    assert torch.equal(ops.conv3x3_dgrad(gy, w), after)


def test_dgrad_rejects_cout_not_a_multiple_of_16(ops, dev):
    import c2m_amd
    with pytest.raises(c2m_amd.C2MError):
        ops.conv3x3_dgrad(_cl(_rand((1, 24, 6, 10), dev, 1730)), _rand((24, 32, 3, 3), dev, 1731))
    with pytest.raises(c2m_amd.C2MError):
        ops.conv3x3_dgrad(_cl(_rand((1, 32, 6, 10), dev, 1732)), _rand((16, 32, 3, 3), dev, 1733))
    torch.cuda.synchronize(dev)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the autograd function's host logic
# ---------------------------------------------------------------------------------------------------------------------
def _autograd_check(ops, dev, cins, Cout, act, slope=0.1, B=2, H=20, W=24, nchw_src=False, gy_mode="cl", bias="rand",
                    w_grad=True, src_grad=None, zero_image=None, seed=1800):
    """act(conv3x3_autograd(xs, w, b)) forward and backward against float64.

    The function masks grad_out by the sign of its own saved float32 output; a float64 reference that masks by its own
    pre-activation differs at full scale wherever the two signs differ, which is not a kernel error.  So the reference
    backward takes its mask from the kernel's output y (grad_out * where(y > 0, 1, slope) through the float64 conv), and
    the forward is asserted on its own: |y - y64| <= 1e-5 max(1, max|y64|), and every element whose sign differs has
    |y64| below that bound."""
    src_grad = [True] * len(cins) if src_grad is None else src_grad
    xs = []
    for k, c in enumerate(cins):
        x = _rand((B, c, H, W), dev, seed + k)
        if zero_image is not None:
            x[zero_image] = 0.0
        xs.append((x if nchw_src else _cl(x)).requires_grad_(src_grad[k]))
    Cin = sum(cins)
    w = _rand((Cout, Cin, 3, 3), dev, seed + 10, 1.0 / math.sqrt(9 * Cin)).requires_grad_(w_grad)
    b = None if bias is None else (torch.zeros(Cout, device=dev) if bias == "zero" else _rand((Cout,), dev, seed + 11)).requires_grad_(True)
    y = ops.conv3x3_autograd(xs, w, b, act=act, slope=slope)
    assert tuple(y.shape) == (B, Cout, H, W)
    if gy_mode == "sum":
        gy = torch.ones_like(y)
        y.sum().backward()                    # grad_out arrives as an expanded scalar: all strides 0
    else:
        gy = _rand((B, Cout, H, W), dev, seed + 12)
        gy = gy.contiguous() if gy_mode == "nchw" else _cl(gy)
        y.backward(gy)
    yk = y.detach()

    xs64 = [x.detach().double().requires_grad_(True) for x in xs]
    w64 = w.detach().double().requires_grad_(True)
    b64 = None if b is None else b.detach().double().requires_grad_(True)
    pre = F.conv2d(torch.cat(xs64, 1), w64, b64, padding=1)
    eff = 1.0 if act == ops.ACT_NONE else (slope if act == ops.ACT_LRELU else 0.0)
    with torch.no_grad():
        y64 = pre if act == ops.ACT_NONE else torch.where(pre > 0, pre, pre * eff)
        bound = 1e-5 * max(1.0, float(y64.abs().max()))
        assert float((yk.double() - y64).abs().max()) <= bound
        if act != ops.ACT_NONE:
            flipped = (yk > 0) != (y64 > 0)
            assert float((y64.abs() * flipped).max()) <= bound
            g_eff = gy.double() * torch.where(yk > 0, 1.0, eff)
        else:
            g_eff = gy.double()
    pre.backward(g_eff)

    pairs = []
    if w_grad:
        pairs.append(("w", w.grad, w64.grad))
    else:
        assert w.grad is None
    if b is not None:
        pairs.append(("b", b.grad, b64.grad))
    for k, (x, x64) in enumerate(zip(xs, xs64)):
        if src_grad[k]:
            assert x.grad is not None and x.grad.shape == x.shape
            pairs.append((f"x{k}", x.grad, x64.grad))
        else:
            assert x.grad is None
    for nm, got, want in pairs:
        err = _relerr(got, want)
        assert err < 1e-5, (nm, err)
    return xs, w, yk, gy


def test_autograd_nchw_contiguous_sources(ops, dev):
    xs, _, _, _ = _autograd_check(ops, dev, [64, 32], 64, 2, nchw_src=True)
    assert all(x.is_contiguous() and x.grad.shape == x.shape for x in xs)


@pytest.mark.parametrize("gy_mode", ["sum", "nchw"])
@pytest.mark.parametrize("act", [0, 2])
def test_autograd_grad_out_layouts(ops, dev, gy_mode, act):
    _autograd_check(ops, dev, [64], 64, act, gy_mode=gy_mode, seed=1820)


def test_autograd_without_bias(ops, dev):
    _autograd_check(ops, dev, [32, 32], 48, 1, bias=None, seed=1830)


def test_autograd_frozen_weight_launches_no_weight_gradient(ops, dev):
    import c2m_amd
    seen = {}
    for w_grad in (True, False):
        c2m_amd.profile_enable(True)
        try:
            c2m_amd.profile_collect()
            _autograd_check(ops, dev, [64], 64, 2, w_grad=w_grad, seed=1840)
            torch.cuda.synchronize(dev)
            seen[w_grad] = {n for n, _ in c2m_amd.profile_collect(capacity=4096)}
        finally:
            c2m_amd.profile_enable(False)
    assert "conv3x3_wgrad" in seen[True] and "conv3x3_split" in seen[True]
    assert "conv3x3_wgrad" not in seen[False] and "conv3x3_split" in seen[False]


@pytest.mark.parametrize("src_grad", [(False, True), (True, False)])
def test_autograd_one_of_two_sources_requires_a_gradient(ops, dev, src_grad):
    _autograd_check(ops, dev, [64, 64], 64, 2, src_grad=list(src_grad), seed=1850)


@pytest.mark.parametrize("Cout", [40, 72, 216])
def test_autograd_cout_padded_to_a_multiple_of_16(ops, dev, Cout):
    _autograd_check(ops, dev, [32, 32], Cout, 0, seed=1860)
    _autograd_check(ops, dev, [64, 32], Cout, 2, seed=1865)


@pytest.mark.parametrize("act,slope", [(2, 0.2), (2, 0.0), (1, 0.1)])
def test_autograd_activation_masks_and_exact_zeros(ops, dev, act, slope):
    """LeakyReLU slopes other than 0.1 and ReLU; one input image all zero with zero bias, so a whole image of outputs is
    exactly 0 and the mask at out == 0 is exercised: gradient factor 0 for ReLU, `slope` for LeakyReLU (torch.where(out > 0,
    ...), as F.relu / F.leaky_relu define it)."""
    _autograd_check(ops, dev, [64], 64, act, slope=slope, seed=1870)
    xs, w, yk, gy = _autograd_check(ops, dev, [32, 32], 64, act, slope=slope, bias="zero", zero_image=0, seed=1880)
    assert float(yk[0].abs().max()) == 0.0 and float(yk[1].abs().max()) > 0.0
    factor = slope if act == ops.ACT_LRELU else 0.0
    got0 = torch.cat([x.grad[:1] for x in xs], 1)
    if factor == 0.0:
        assert float(got0.abs().max()) == 0.0
    else:
        assert _relerr(got0, _ref_dgrad(gy[:1] * factor, w)) < 1e-5    # image 0: dx = slope * conv^T(grad_out)
    # ... and torch's own activations agree about the factor at exactly 0
    z = torch.zeros(4, device=dev, requires_grad=True)
    (F.leaky_relu(z, slope) if act == ops.ACT_LRELU else F.relu(z)).sum().backward()
    assert float((z.grad - factor).abs().max()) < 1e-7
