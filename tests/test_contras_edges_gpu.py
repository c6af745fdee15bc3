"""GPU: the fused contrastive loss (csrc/contras_loss.hip) in the regimes test_contras_gpu.py never enters -- a partly
inactive hinge, every admitted channel count, non-square and unequal maps with gradients, skipped first / middle samples
next to ragged row counts, non-unit upstream gradients, the parameter ranges, feature scale and all-zero vectors, exact
ties, input layout, and the run-to-run spread of the atomic backward.  The reference is the float64 restatement of
test_contras_gpu.py throughout; every guard on an input is asserted on that restatement or on the host builder."""
import numpy as np
import pytest
import torch

import make_golden_contras as mgc
from test_contras_gpu import _check_grads, _compare, _homography_coords, _loss, restate

pytestmark = pytest.mark.gpu
synth = mgc.synth


# ---- inputs ---------------------------------------------------------------------------------------------------------

def _rule(coords, b, h1, w1, steps=2):
    """The restatement's own correspondence rule for sample b -> ids [n], pos2 [2, n] (y, x)."""
    t = coords[b, ::4, ::4, :2].reshape(-1, 2)
    x, y = t[:, 0], t[:, 1]
    ok = (x > 10) & (x < 4 * w1 - 10) & (y > 10) & (y < 4 * h1 - 10)
    ids = ok.nonzero()[:, 0]
    return ids, torch.stack([torch.round(y[ids] / 2 ** steps), torch.round(x[ids] / 2 ** steps)], 0).long()


def _gauss(shape, seed):
    return torch.from_numpy(synth.gaussish(shape, seed))


def _correlated(B, C, h1, w1, coords, sigma, seed, h2=None, w2=None, steps=2):
    """f1 random, f2 = sigma * noise + f1 carried through the correspondence: matched descriptors (CPU tensors)."""
    h2, w2 = h2 or h1, w2 or w1
    f1 = _gauss((B, C, h1, w1), seed)
    f2 = sigma * _gauss((B, C, h2, w2), seed + 1)
    for b in range(B):
        ids, p2 = _rule(coords, b, h1, w1, steps)
        if ids.numel() < 128:
            continue
        a = f2[b].numpy()
        a[:, p2[0].numpy(), p2[1].numpy()] = a[:, p2[0].numpy(), p2[1].numpy()] + f1[b].reshape(C, -1)[:, ids].numpy()
    return f1, f2


def _teacher(f1, f2, seed, amp=0.7):
    return f1 + amp * _gauss(tuple(f1.shape), seed), f2 + amp * _gauss(tuple(f2.shape), seed + 1)


def _active_share(f1, f2, coords, **k):
    """Share of rows with a positive hinge, from the restatement's per-row values."""
    _, rows = restate(f1.double(), f2.double(), coords, rows=True, **k)
    B, C = f1.shape[:2]
    act = tot = 0
    kept = [b for b in range(B) if _rule(coords, b, f1.shape[2], f1.shape[3], k.get("steps", 2))[0].numel() >= 128]
    for b, (_, _, neg1, neg2) in zip(kept, rows):
        ids, p2 = _rule(coords, b, f1.shape[2], f1.shape[3], k.get("steps", 2))
        d1 = torch.nn.functional.normalize(f1[b].double().reshape(C, -1), dim=0)[:, ids]
        d2 = torch.nn.functional.normalize(f2[b].double()[:, p2[0], p2[1]], dim=0)
        pos = 2 - 2 * (d1 * d2).sum(0)
        act += int((k.get("margin", 1.0) + pos - torch.min(neg1, neg2) > 0).sum())
        tot += ids.numel()
    return act / tot


def _to(dev, *ts):
    return [t.to(dev) for t in ts]


def _case_a(dev, B, C, h, w, stage, sigma=0.5, seed=7400, coord_seed=77):
    coords = _homography_coords(B, h, w, coord_seed)
    f1, f2 = _correlated(B, C, h, w, coords, sigma, seed)
    teacher = _teacher(f1, f2, seed + 10) if stage == 2 else None
    f1, f2, coords = _to(dev, f1, f2, coords)
    if teacher is not None:
        teacher = tuple(_to(dev, *teacher))
    return f1, f2, coords, teacher


# ---- A. correlated features: a partly inactive hinge ----------------------------------------------------------------

@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("shape,sigma", [((2, 64, 24, 36), 0.5), ((4, 256, 40, 40), 1.0)], ids=["small", "training"])
def test_partly_inactive_hinge(dev, shape, sigma, stage):
    """sigma per channel count, found on the CPU: active share 0.59 (C = 64, sigma 0.5) and 0.64 (C = 256, sigma 1.0)."""
    f1, f2, coords, teacher = _case_a(dev, *shape, stage, sigma=sigma)
    share = _active_share(f1, f2, coords)
    print(f"active share {share:.3f}")
    assert 0.2 <= share <= 0.8, f"input guard: active share {share:.3f}"
    _compare(f1, f2, coords, teacher=teacher)


# ---- B. channel sweep ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [16, 48, 80, 384, 512])
def test_channel_counts(dev, C):
    B, h, w = 2, 20, 28
    coords = _homography_coords(B, h, w, 7411)
    for b in range(B):
        assert _rule(coords, b, h, w)[0].numel() >= 128
    f1, f2 = _gauss((B, C, h, w), 7412 + C), _gauss((B, C, h, w), 7413 + C)
    teacher = _teacher(f1, f2, 7414 + C)
    f1, f2, coords, t1, t2 = _to(dev, f1, f2, coords, *teacher)
    _compare(f1, f2, coords, teacher=(t1, t2))


def test_unsupported_channel_counts_answer_on_the_device_too(dev):
    """C = 24 and C = 528 with real device buffers: C2M_ERR_UNSUPPORTED (2), and neither the output nor the workspace
    is touched."""
    import c2m_amd
    L = c2m_amd._lib.lib()
    for C in (24, 528):
        f = torch.ones(1, C, 20, 20, device=dev)
        ids = torch.arange(200, dtype=torch.int32, device=dev)
        pos2 = torch.zeros(200, 2, dtype=torch.int32, device=dev)
        off = torch.tensor([0, 200], dtype=torch.int32, device=dev)
        out = torch.full((1, 4), 7.0, device=dev)
        ws = torch.full((1 << 22,), 3, dtype=torch.uint8, device=dev)
        gf = torch.full_like(f, 5.0)
        st = L.c2m_contras_loss_forward_f32(None, f.data_ptr(), f.data_ptr(), None, None, 1, C, 20, 20, 20, 20, ids.data_ptr(),
                                            pos2.data_ptr(), off.data_ptr(), 200, 200, 1.0, 4.0, 0.15, out.data_ptr(),
                                            ws.data_ptr(), ws.numel())
        assert st == 2
        g = torch.ones(1, 2, device=dev)
        st = L.c2m_contras_loss_backward_f32(None, 1, C, 20, 20, 20, 20, ids.data_ptr(), pos2.data_ptr(), off.data_ptr(), 200,
                                             200, 1.0, 4.0, 0.15, 0, g.data_ptr(), gf.data_ptr(), gf.data_ptr(),
                                             ws.data_ptr(), ws.numel())
        assert st == 2
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((ws == 3).all()) and bool((gf == 5.0).all())


# ---- C. non-square and unequal maps, with gradients -------------------------------------------------------------------

@pytest.mark.parametrize("stage", [1, 2])
@pytest.mark.parametrize("h1,w1,dh,dw", [(24, 36, 0, 0), (33, 21, 0, 0), (24, 36, 5, 3), (33, 21, 5, 3)])
def test_non_square_and_unequal_maps(dev, h1, w1, dh, dw, stage):
    B, C = 2, 64
    coords = _homography_coords(B, h1, w1, 7421 + h1)
    for b in range(B):
        assert _rule(coords, b, h1, w1)[0].numel() >= 128
    f1, f2 = _correlated(B, C, h1, w1, coords, 0.6, 7422 + h1 + dh, h1 + dh, w1 + dw)
    teacher = _teacher(f1, f2, 7424) if stage == 2 else None
    f1, f2, coords = _to(dev, f1, f2, coords)
    if teacher is not None:
        teacher = tuple(_to(dev, *teacher))
    _compare(f1, f2, coords, teacher=teacher)


# ---- D. batch structure ---------------------------------------------------------------------------------------------

D_SHAPE = (4, 64, 24, 36)
D_FULL = dict(seed=7435, shift=1.0)      # sample 1: 705 rows = 22 x 32 + 1   (seeds and shifts found on the CPU with
D_CROP = dict(seed=7434, shift=40.0)     # sample 3: 287 rows =  8 x 32 + 31   the restatement's validity rule)
D_COUNTS = (0, 705, 0, 287)


def _case_d():
    B, C, h, w = D_SHAPE
    coords = torch.full((B, 4 * h, 4 * w, 2), 5.0)
    coords[1] = _homography_coords(1, h, w, **D_FULL)[0]
    coords[3] = _homography_coords(1, h, w, **D_CROP)[0]
    return coords


@pytest.mark.parametrize("stage", [1, 2])
def test_skipped_first_and_middle_samples_and_ragged_counts(dev, stage):
    from c2m_amd import ops
    B, C, h, w = D_SHAPE
    coords = _case_d()
    counts = [int(n) if n >= 128 else 0 for n in (_rule(coords, b, h, w)[0].numel() for b in range(B))]
    assert tuple(counts) == D_COUNTS and counts[1] % 32 == 1 and counts[3] % 32 == 31 and counts[1] > 2 * counts[3]
    f1, f2 = _correlated(B, C, h, w, coords, 0.6, 7433)
    teacher = _teacher(f1, f2, 7435) if stage == 2 else None
    f1, f2, coords = _to(dev, f1, f2, coords)
    if teacher is not None:
        teacher = tuple(_to(dev, *teacher))
    corr = ops.contras_correspondences(coords, h, w, 2)
    assert corr["counts"] == counts
    assert corr["offsets"].tolist() == [0, 0, counts[1], counts[1], counts[1] + counts[3]]
    _compare(f1, f2, coords, teacher=teacher)
    # the skipped samples' gradients are exact zeros even when the allocator hands back blocks full of NaNs
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    loss = _loss(a, b, coords, teacher=teacher)[0]
    junk = [torch.full_like(f1, float("nan")) for _ in range(2)] + [torch.full_like(f2, float("nan")) for _ in range(2)]
    torch.cuda.synchronize()
    del junk
    g1, g2 = torch.autograd.grad(loss, (a, b))
    for g in (g1, g2):
        assert bool(torch.isfinite(g).all())
        assert int(g[0].count_nonzero()) == 0 and int(g[2].count_nonzero()) == 0
        assert int(g[1].count_nonzero()) > 0 and int(g[3].count_nonzero()) > 0


# ---- E. upstream gradients --------------------------------------------------------------------------------------------

def _pair(f1, f2):
    a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    return a, b, a.detach().double().requires_grad_(True), b.detach().double().requires_grad_(True)


def _grads_match(expr_got, expr_want, a, b, da, db):
    g = torch.autograd.grad(expr_got, (a, b), retain_graph=True)
    w = torch.autograd.grad(expr_want, (da, db), retain_graph=True)
    _check_grads(g[0], w[0].float())
    _check_grads(g[1], w[1].float())
    return g


def test_upstream_gradients_scaled_and_single_terms(dev):
    f1, f2, coords, teacher = _case_a(dev, 2, 64, 24, 36, 2)
    t64 = tuple(t.double() for t in teacher)
    a, b, da, db = _pair(f1, f2)
    got = _loss(a, b, coords, teacher=teacher)
    want = restate(da, db, coords, teacher=t64)
    assert got[1].requires_grad is False and got[2].requires_grad is False      # pos_dist / neg_dist: documented constants
    assert got[0].requires_grad and got[3].requires_grad
    _grads_match(3.7 * got[0], 3.7 * want[0], a, b, da, db)
    gk = _grads_match(got[3], want[3], a, b, da, db)                             # the distillation term alone
    # distill_weight 0 and 15: the hinge alone, and a difference of exactly 15 x the distillation term's gradient
    g0 = _grads_match(_loss(a, b, coords, teacher=teacher, distill_weight=0.0)[0],
                      restate(da, db, coords, teacher=t64, wd=0.0)[0], a, b, da, db)
    g15 = _grads_match(_loss(a, b, coords, teacher=teacher, distill_weight=15.0)[0],
                       restate(da, db, coords, teacher=t64, wd=15.0)[0], a, b, da, db)
    for k in range(2):
        _check_grads(g15[k] - g0[k], 15.0 * gk[k])
    _check_grads(g0[0], torch.autograd.grad(_loss(a, b, coords)[0], (a, b))[0])   # wd = 0 is the stage-1 gradient


@pytest.mark.parametrize("which", [0, 1])
def test_backward_with_one_input_requiring_grad(dev, which):
    f1, f2, coords, teacher = _case_a(dev, 2, 64, 24, 36, 2)
    a, b, da, db = _pair(f1, f2)
    (a, b)[1 - which].requires_grad_(False)
    got = _loss(a, b, coords, teacher=teacher)
    got[0].backward()
    want = restate(da, db, coords, teacher=tuple(t.double() for t in teacher))
    want[0].backward()
    assert (a, b)[1 - which].grad is None
    _check_grads((a, b)[which].grad, (da, db)[which].grad.float())


def test_per_sample_upstream_weights(dev):
    """Different, non-unit weights on every sample's hinge and distillation term (grad_terms[2b], [2b+1]), against the
    restatement run sample by sample (B = 1 calls)."""
    from c2m_amd import ops
    B = 3
    f1, f2, coords, teacher = _case_a(dev, B, 64, 24, 36, 2, coord_seed=78)
    wgt = torch.tensor([[1.9, -0.6], [0.0, 2.3], [-1.1, 0.0]], device=dev)
    a, b, da, db = _pair(f1, f2)
    corr = ops.contras_correspondences(coords, 24, 36, 2)
    assert all(n >= 128 for n in corr["counts"])
    terms, dists = ops._ContrasLossFn.apply(a, b, teacher[0], teacher[1], corr, 1.0, 4, 0.15)
    assert not dists.requires_grad
    want = 0.
    for s in range(B):
        r = restate(da[s:s + 1], db[s:s + 1], coords[s:s + 1], teacher=(teacher[0][s:s + 1].double(), teacher[1][s:s + 1].double()),
                    wd=0.0)
        np.testing.assert_allclose(float(terms[s, 0].detach()), float(r[0].detach()), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(float(terms[s, 1].detach()), float(r[3].detach()), rtol=1e-5, atol=1e-6)
        want = want + float(wgt[s, 0]) * r[0] + float(wgt[s, 1]) * r[3]
    _grads_match((terms * wgt).sum(), want, a, b, da, db)


# ---- F. parameters ----------------------------------------------------------------------------------------------------

def test_temperature_one(dev):
    f1, f2, coords, teacher = _case_a(dev, 2, 64, 24, 36, 2)
    _compare(f1, f2, coords, teacher=teacher, temperature=1.0)


def _dist(x, ref):
    d = (x.double() - ref.double()).abs()
    return float(d.max()), float(d.pow(2).mean().sqrt())


def test_temperature_small_no_worse_than_twice_torch_fp32(dev):
    """tau = 0.02: logits of magnitude 50.  The bound is set by the float32 evaluation of the restatement itself: the
    kernel may be at most 2 x as far from the float64 result as torch's fp32 is (floor 1e-6 x scale).
    Measured on an MI355X (kernel distance / torch-fp32 distance): see DESIGN.md section 12."""
    f1, f2, coords, teacher = _case_a(dev, 2, 64, 24, 36, 2)
    a, b, da, db = _pair(f1, f2)
    fa, fb = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    got = _loss(a, b, coords, teacher=teacher, temperature=0.02)
    want = restate(da, db, coords, teacher=tuple(t.double() for t in teacher), tau=0.02)
    ref32 = restate(fa, fb, coords, teacher=teacher, tau=0.02)
    names = ("loss", "pos_dist", "neg_dist", "distill_loss")
    fails = []
    for n, g, w, r in zip(names, got, want, ref32):
        g, w, r = float(g.detach()), float(w.detach()), float(r.detach())
        dk, dr = abs(g - w), abs(r - w)
        print(f"tau=0.02 {n}: value {w:.6f}, kernel distance {dk:.3e}, torch fp32 distance {dr:.3e}")
        assert np.isfinite(g)
        if dk > max(2.0 * dr, 1e-6 * abs(w)):
            fails.append(f"{n}: kernel {dk:.3e} > 2 x fp32 {dr:.3e}")
    got[0].backward()
    want[0].backward()
    ref32[0].backward()
    for n, g, w, r in (("grad f1", a.grad, da.grad, fa.grad), ("grad f2", b.grad, db.grad, fb.grad)):
        assert bool(torch.isfinite(g).all())
        (km, kr), (rm, rr) = _dist(g, w), _dist(r, w)
        scale, rms = float(w.abs().max()), float(w.pow(2).mean().sqrt())
        print(f"tau=0.02 {n}: max|want| {scale:.3e}; kernel max-abs {km:.3e} rms {kr:.3e}; torch fp32 max-abs {rm:.3e} rms {rr:.3e}")
        if km > max(2.0 * rm, 1e-6 * scale):
            fails.append(f"{n} max-abs: kernel {km:.3e} > 2 x fp32 {rm:.3e}")
        if kr > max(2.0 * rr, 1e-6 * rms):
            fails.append(f"{n} rms: kernel {kr:.3e} > 2 x fp32 {rr:.3e}")
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("margin", [0.2, 3.0])
def test_margin_moves_rows_across_the_hinge(dev, margin):
    f1, f2, coords, teacher = _case_a(dev, 2, 64, 24, 36, 2)
    share, at_one = _active_share(f1, f2, coords, margin=margin), _active_share(f1, f2, coords)
    print(f"margin {margin}: active share {share:.3f} (margin 1.0: {at_one:.3f})")     # CPU: 0.11 / 1.00 against 0.59
    assert abs(share - at_one) >= 0.2, f"input guard: active share {share:.3f} against {at_one:.3f} at margin 1"
    _compare(f1, f2, coords, teacher=teacher, margin=margin)


@pytest.mark.parametrize("radius", [0, 1.5, 4])
def test_safe_radius(dev, radius):
    f1, f2, coords, teacher = _case_a(dev, 2, 64, 24, 36, 2)
    _compare(f1, f2, coords, teacher=teacher, safe_radius=radius)


@pytest.mark.parametrize("stage", [1, 2])
def test_scaling_steps_three_with_a_half_resolution_second_map(dev, stage):
    B, C, h, w = 2, 64, 24, 36
    coords = _homography_coords(B, h, w, 77)
    f1, f2 = _correlated(B, C, h, w, coords, 0.6, 7441, h // 2, w // 2, steps=3)
    teacher = _teacher(f1, f2, 7443) if stage == 2 else None
    f1, f2, coords = _to(dev, f1, f2, coords)
    if teacher is not None:
        teacher = tuple(_to(dev, *teacher))
    _compare(f1, f2, coords, teacher=teacher, scaling_steps=3)


# ---- G. feature scale and all-zero vectors ----------------------------------------------------------------------------

@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_feature_scale(dev, scale):
    f1, f2, coords, teacher = _case_a(dev, 2, 64, 24, 36, 2)
    base = _loss(f1, f2, coords, teacher=teacher)
    got = _compare(f1 * scale, f2 * scale, coords, teacher=teacher)
    for x, y in zip(got, base):
        np.testing.assert_allclose(float(x), float(y), rtol=1e-5, atol=1e-6)   # the loss is scale-invariant


@pytest.mark.parametrize("stage", [1, 2])
def test_all_zero_feature_vectors(dev, stage):
    """Three valid positions of f1 and three used positions of f2 hold an all-zero vector (a ReLU-terminated extractor
    can produce one).  F.normalize (eps 1e-12) defines value and gradient there: g / eps, ~1e12 x the rest."""
    B, C, h, w = 2, 64, 24, 36
    f1, f2, coords, teacher = _case_a(dev, B, C, h, w, stage)
    z1 = torch.zeros(B, h * w, dtype=torch.bool, device=dev)
    z2 = torch.zeros(B, h * w, dtype=torch.bool, device=dev)
    f1, f2 = f1.clone(), f2.clone()
    for b in range(B):
        ids, p2 = _rule(coords, b, h, w)
        n = ids.numel()
        for r in (5, n // 2, n - 7):
            z1[b, ids[r]] = True
            z2[b, p2[0, r + 3] * w + p2[1, r + 3]] = True
    f1.view(B, C, -1).permute(0, 2, 1)[z1] = 0.0
    f2.view(B, C, -1).permute(0, 2, 1)[z2] = 0.0
    assert int(z1.sum()) == 6 and int(z2.sum()) == 6
    assert int((f1.view(B, C, -1).abs().sum(1) == 0).sum()) == 6 and int((f2.view(B, C, -1).abs().sum(1) == 0).sum()) == 6
    a, b_, da, db = _pair(f1, f2)
    got = _loss(a, b_, coords, teacher=teacher)
    want = restate(da, db, coords, teacher=None if teacher is None else tuple(t.double() for t in teacher))
    for x, y in zip(got, want):
        np.testing.assert_allclose(float(x.detach()), float(y.detach()), rtol=1e-5, atol=1e-6)
    got[0].backward()
    want[0].backward()
    for name, g, wv, z in (("grad f1", a.grad, da.grad, z1), ("grad f2", b_.grad, db.grad, z2)):
        assert bool(torch.isfinite(g).all()), name
        zm = z.view(B, 1, h, w).expand_as(g)
        rest_w, rest_g = wv.masked_fill(zm, 0.0), g.masked_fill(zm, 0.0)
        _check_grads(rest_g, rest_w.float())
        zw, zg = wv[zm], g[zm].double()
        s_rest, s_zero = float(rest_w.abs().max()), float(zw.abs().max())
        err = float((zg - zw).abs().max())
        assert s_zero > 1e8 * s_rest, f"{name}: zeroed positions {s_zero:.3e}, the rest {s_rest:.3e}"
        assert err <= 1e-3 * s_zero, (f"{name} at the zeroed positions: max abs err {err:.3e} > 1e-3 x {s_zero:.3e} "
                                      f"(the other positions' gradients are of magnitude {s_rest:.3e})")


# ---- H. ties ------------------------------------------------------------------------------------------------------------

TIE_STEPS = (0, 4, 32 + 3, 128, 32 * 6 + 17, 32 * 11 + 5)   # same tile other lane half, next tile, same wave (+4 tiles), ...


def _tie_base(dev, seed):
    B, C, h, w = 2, 64, 24, 36
    coords = _homography_coords(B, h, w, 77)
    return B, C, h, w, coords, _gauss((B, C, h, w), seed), _gauss((B, C, h, w), seed + 1)


def test_argmin_ties_take_the_lowest_position_neg1(dev):
    """One f1 vector copied to six positions (two lane halves of one tile, other tiles of the same and of other waves);
    rows whose f2 vector is that vector (+ small noise) have all six as exact nearest negatives: neg1_idx is the lowest."""
    from c2m_amd import ops
    B, C, h, w, coords, f1, f2 = _tie_base(dev, 7451)
    expect = {}
    for b in range(B):
        p = 40 + 8 * b                      # p % 8 < 4: p and p + 4 sit in the two lane halves of one 32-column tile
        dups = [p + s for s in TIE_STEPS]
        v = f1[b, :, p // w, p % w].clone()
        for q in dups:
            f1[b, :, q // w, q % w] = v
        ids, p2 = _rule(coords, b, h, w)
        far = [r for r in range(ids.numel())
               if all(max(abs(int(ids[r]) // w - q // w), abs(int(ids[r]) % w - q % w)) > 4 for q in dups)]
        for r in (far[3], far[len(far) // 2], far[-5]):
            f2[b, :, p2[0, r], p2[1, r]] = v + 0.01 * _gauss((C,), 7453 + r)
            expect[(b, r)] = (p, dups)
    f1, f2, coords = _to(dev, f1, f2, coords)
    _, ref = restate(f1.double(), f2.double(), coords, rows=True)
    rows = ops.contras_loss_rows(f1, f2, coords)
    off = rows["offsets"].tolist()
    for (b, r), (p, dups) in expect.items():
        n1m = ref[b][0][r]
        others = n1m.clone()
        others[dups] = 99.0
        assert float((n1m[dups] - n1m.min()).abs().max()) < 1e-12 and float(others.min()) > float(n1m.min()) + 0.1   # input guard
        assert int(rows["neg1_idx"][off[b] + r]) == p, (b, r, int(rows["neg1_idx"][off[b] + r]), dups)
    _compare(f1, f2, coords)


def test_argmin_ties_take_the_lowest_row_neg2(dev):
    """The same for neg2: one f2 vector at the pos2 of six rows j0 + TIE_STEPS; rows whose f1 vector is that vector
    (+ small noise) tie exactly over them: neg2_idx is the lowest row that reads one of those pixels."""
    from c2m_amd import ops
    B, C, h, w, coords, f1, f2 = _tie_base(dev, 7461)
    expect = {}
    for b in range(B):
        ids, p2 = _rule(coords, b, h, w)
        n = ids.numel()
        j0 = 64 + 8 * b + 1
        js = [j0 + s for s in TIE_STEPS]
        assert js[-1] < n
        v = f2[b, :, p2[0, j0], p2[1, j0]].clone()
        pix = {(int(p2[0, j]), int(p2[1, j])) for j in js}
        for y, x in pix:
            f2[b, :, y, x] = v
        readers = [j for j in range(n) if (int(p2[0, j]), int(p2[1, j])) in pix]
        far = [r for r in range(n)
               if all(max(abs(int(p2[0, r]) - y), abs(int(p2[1, r]) - x)) > 4 for y, x in pix)]
        for r in (far[3], far[len(far) // 2], far[-5]):
            f1[b, :, int(ids[r]) // w, int(ids[r]) % w] = v + 0.01 * _gauss((C,), 7463 + r)
            expect[(b, r)] = (min(readers), readers)
    f1, f2, coords = _to(dev, f1, f2, coords)
    _, ref = restate(f1.double(), f2.double(), coords, rows=True)
    rows = ops.contras_loss_rows(f1, f2, coords)
    off = rows["offsets"].tolist()
    for (b, r), (low, readers) in expect.items():
        assert low == 64 + 8 * b + 1 and len(readers) >= len(TIE_STEPS)
        n2m = ref[b][1][r]
        others = n2m.clone()
        others[readers] = 99.0
        assert float((n2m[readers] - n2m.min()).abs().max()) < 1e-12 and float(others.min()) > float(n2m.min()) + 0.1  # input guard
        assert int(rows["neg2_idx"][off[b] + r]) == low, (b, r, int(rows["neg2_idx"][off[b] + r]), readers)
    _compare(f1, f2, coords)


def _ternary(shape, seed):
    """[B, 16, h, w] with exactly four non-zeros (+-1) per position: |x| = 2, every normalised dot a multiple of 1/4,
    exact in fp32 and fp64 alike."""
    B, C, h, w = shape
    u = synth.uniform((B, h, w, C), seed)
    s = np.sign(synth.uniform((B, h, w, C), seed + 1)).astype(np.float32)
    s[s == 0] = 1.0
    top = np.argsort(u, axis=-1)[..., -4:]
    out = np.zeros((B, h, w, C), np.float32)
    np.put_along_axis(out, top, np.take_along_axis(s, top, -1), -1)
    return torch.from_numpy(np.ascontiguousarray(out.transpose(0, 3, 1, 2)))


def test_hinge_tie_splits_the_gradient_in_halves(dev):
    """Features in {0, +-1} with four non-zeros of C = 16: all arithmetic up to the hinge is exact, so neg1 == neg2
    happens bitwise in the kernel and in float64 alike, and torch.minimum's 0.5 / 0.5 split is the expected gradient."""
    from c2m_amd import ops
    B, C, h, w = 2, 16, 24, 36
    coords = _homography_coords(B, h, w, 77).to(dev)
    f1, f2 = _ternary((B, C, h, w), 7471).to(dev), _ternary((B, C, h, w), 7473).to(dev)
    _, ref = restate(f1.double(), f2.double(), coords, rows=True)
    ties = sum(int((neg1 == neg2).sum()) for _, _, neg1, neg2 in ref)
    total = sum(int(neg1.numel()) for _, _, neg1, _ in ref)
    rows = ops.contras_loss_rows(f1, f2, coords)
    print(f"exact hinge ties: {ties} of {total} rows")
    assert ties >= 1, "input guard: no row with neg1 == neg2 in the restatement"
    tied = torch.cat([neg1 == neg2 for _, _, neg1, neg2 in ref])
    assert int((rows["neg1"] == rows["neg2"]).sum()) >= 1
    assert torch.equal(rows["neg1"] == rows["neg2"], tied)     # exact arithmetic: the same rows tie in fp32 and in fp64
    _compare(f1, f2, coords)


# ---- I. layout on entry -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stage", [1, 2])
def test_non_contiguous_inputs(dev, stage):
    """channels_last f1, f2 a slice of a larger tensor, the teacher maps a broadcast view and a transposed one."""
    B, C, h, w = 2, 64, 24, 36
    f1, f2, coords, teacher = _case_a(dev, B, C, h, w, stage)
    flat = None
    if teacher is not None:
        t1 = teacher[0][:1].expand(B, -1, -1, -1)                                   # one teacher map for the whole batch
        t2 = teacher[1].permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
        assert not t1.is_contiguous() and not t2.is_contiguous()
        teacher, flat = (t1, t2), (t1.contiguous(), t2.contiguous())
    c1, c2 = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
    base = _loss(c1, c2, coords, teacher=flat)
    base[0].backward()
    a = f1.clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    big = torch.full((B, C, h + 2, w + 4), 9.0, device=dev)
    big[:, :, 1:-1, 2:-2] = f2
    big.requires_grad_(True)
    b = big[:, :, 1:-1, 2:-2]
    assert not a.is_contiguous() and not b.is_contiguous()
    got = _loss(a, b, coords, teacher=teacher)
    for x, y in zip(got, base):
        assert torch.equal(x, y)                       # the forward is bitwise reproducible, whatever the layout
    got[0].backward()
    assert a.grad.shape == f1.shape and big.grad.shape == big.shape
    _check_grads(a.grad, c1.grad, tol=1e-5)            # (1e-5: the atomic backward's own spread, test_backward_spread)
    _check_grads(big.grad[:, :, 1:-1, 2:-2], c2.grad, tol=1e-5)
    inner = torch.zeros_like(big, dtype=torch.bool)
    inner[:, :, 1:-1, 2:-2] = True
    assert int(big.grad[~inner].count_nonzero()) == 0


# ---- J. run-to-run spread of the backward -------------------------------------------------------------------------------

def test_backward_spread(dev):
    """The backward sums with fp32 atomics, so it is reproducible only to rounding: three runs differ by at most
    1e-5 x max|grad|, an order below the 1e-4 accuracy bound."""
    f1, f2, coords, teacher = _case_a(dev, 4, 256, 40, 40, 2, sigma=1.0)
    runs = []
    for _ in range(3):
        a, b = f1.clone().requires_grad_(True), f2.clone().requires_grad_(True)
        _loss(a, b, coords, teacher=teacher)[0].backward()
        runs.append((a.grad, b.grad))
    for k, name in enumerate(("grad f1", "grad f2")):
        scale = float(runs[0][k].abs().max())
        spread = max(float((runs[i][k] - runs[j][k]).abs().max()) for i in range(3) for j in range(i))
        print(f"{name}: run-to-run max difference {spread:.3e} = {spread / scale:.2e} x max|grad|")
        assert spread <= 1e-5 * scale, f"{name}: {spread:.3e} > 1e-5 x {scale:.3e}"
