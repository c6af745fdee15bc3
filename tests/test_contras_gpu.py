"""GPU: the fused contrastive loss of the stage 1-2 extractor training (csrc/contras_loss.hip) against the reference's
own loss_function (tests/golden/contras_golden.npz, made by make_golden_contras.py) and against a float64 restatement,
plus the two models built on it."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import make_golden_contras as mgc

pytestmark = pytest.mark.gpu
S = mgc.SETTINGS


def restate(f1, f2, coords, margin=1.0, radius=4, steps=2, teacher=None, tau=0.15, wd=15.0, rows=False):
    """float64 restatement of the loss, sample by sample (the reference's algebra, written out).  f* are float64."""
    B, C, h1, w1 = f1.shape
    dev = f1.device
    loss = torch.zeros(1, dtype=torch.float64, device=dev)
    pos_s = neg_s = kl_s = 0.
    nv = 0
    out_rows = []
    gy, gx = torch.meshgrid(torch.arange(h1, device=dev), torch.arange(w1, device=dev), indexing="ij")
    grid = torch.stack([gy.reshape(-1), gx.reshape(-1)], 0)
    for b in range(B):
        t = coords[b, ::4, ::4, :2].reshape(-1, 2)
        x, y = t[:, 0], t[:, 1]
        ok = (x > 10) & (x < 4 * w1 - 10) & (y > 10) & (y < 4 * h1 - 10)
        ids = ok.nonzero()[:, 0]
        if ids.numel() < 128:
            continue
        p2 = torch.stack([torch.round(y[ids] / 2 ** steps), torch.round(x[ids] / 2 ** steps)], 0).long()
        D1 = F.normalize(f1[b].reshape(C, -1), dim=0)
        d1 = D1[:, ids]
        d2 = F.normalize(f2[b][:, p2[0], p2[1]], dim=0)
        pos = 2 - 2 * (d1 * d2).sum(0)
        in2 = (p2[:, :, None] - p2[:, None, :]).abs().max(0)[0] <= radius
        n2m = 2 - 2 * d1.t() @ d2 + 10. * in2
        g1 = grid[:, ids]
        in1 = (g1[:, :, None] - grid[:, None, :]).abs().max(0)[0] <= radius
        n1m = 2 - 2 * d2.t() @ D1 + 10. * in1
        neg2, neg1 = n2m.min(1)[0], n1m.min(1)[0]
        negm = torch.min(neg1, neg2)
        loss = loss + F.relu(margin + pos - negm).mean()
        if teacher is not None:
            T1 = F.normalize(teacher[0][b].reshape(C, -1), dim=0)[:, ids]
            T2 = F.normalize(teacher[1][b][:, p2[0], p2[1]], dim=0)
            lq = F.log_softmax(d1.t() @ d2 / tau, 1)
            lp = F.log_softmax(T1.t() @ T2 / tau, 1)
            kl = (lp.exp() * (lp - lq)).sum() / ids.numel()
            loss = loss + wd * kl
            kl_s = kl_s + kl
        pos_s, neg_s, nv = pos_s + pos.mean(), neg_s + negm.mean(), nv + 1
        if rows:
            out_rows.append((n1m, n2m, neg1, neg2))
    if nv == 0:
        raise NotImplementedError
    res = [loss / nv, pos_s / nv, neg_s / nv] + ([kl_s / nv] if teacher is not None else [])
    return (res, out_rows) if rows else res


def _t(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev, dtype)


def _case(case, dev):
    f1, f2, t1, t2, coords, _ = mgc.inputs(case)
    return [_t(a, dev) for a in (f1, f2, t1, t2, coords)]


def _loss(f1, f2, coords, teacher=None, **k):
    from c2m_amd import ops
    kw = dict(margin=S["margin"], safe_radius=S["safe_radius"], scaling_steps=S["scaling_steps"])
    kw.update(k)
    if teacher is not None:
        kw.setdefault("temperature", S["temperature"])
        kw.setdefault("distill_weight", S["distill_weight"])
    return ops.contras_loss(f1, f2, coords, teacher=teacher, **kw)


def _check_grads(got, want, tol=1e-4):
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    assert err <= tol * scale, f"max abs err {err:.3e} > {tol} x {scale:.3e}"


def test_golden_scalars_and_argmins(dev, golden_dir):
    from c2m_amd import ops
    g = np.load(os.path.join(golden_dir, "contras_golden.npz"))
    f1, f2, t1, t2, coords = _case("a", dev)
    assert np.array_equal(mgc.homographies("a"), g["a/homographies"])
    out = _loss(f1, f2, coords, teacher=(t1, t2))
    got = np.array([float(v) for v in out])
    np.testing.assert_allclose(got, g["a/scalars"], rtol=1e-5)
    rows = ops.contras_loss_rows(f1, f2, coords, teacher=(t1, t2))
    _, ref_rows = restate(*(a.double() for a in (f1, f2)), coords, teacher=(t1.double(), t2.double()), rows=True)
    off = rows["offsets"].tolist()
    kept = [b for b in range(3) if rows["counts"][b] > 0]
    assert kept == [0, 1]
    listed = []
    for k, b in enumerate(kept):
        n1m, n2m, _, _ = ref_rows[k]
        for name, m, key in (("neg1", n1m, "neg1_idx"), ("neg2", n2m, "neg2_idx")):
            want = g[f"a/argmin_{name}_{k}"]
            mine = rows[key][off[b]:off[b + 1]].cpu().numpy()
            top2 = torch.topk(m, 2, dim=1, largest=False).values
            close = ((top2[:, 1] - top2[:, 0]) < 1e-5).cpu().numpy()
            bad = np.nonzero((mine != want) & ~close)[0]
            assert bad.size == 0, f"{name} sample {b}: rows {bad[:10]} differ from the reference (margin >= 1e-5)"
            listed += [(b, name, int(i)) for i in np.nonzero((mine != want) & close)[0]]
    print("near-tie rows where the arg-min differs (allowed):", listed)


def test_golden_gradients(dev, golden_dir):
    g = np.load(os.path.join(golden_dir, "contras_golden.npz"))
    f1, f2, t1, t2, coords = _case("b", dev)
    f1.requires_grad_(True)
    f2.requires_grad_(True)
    out = _loss(f1, f2, coords, teacher=(t1, t2))
    np.testing.assert_allclose(np.array([float(v.detach()) for v in out]), g["b/scalars"], rtol=1e-5)
    out[0].backward()
    _check_grads(f1.grad.cpu(), torch.from_numpy(g["b/grad_f1"]))
    _check_grads(f2.grad.cpu(), torch.from_numpy(g["b/grad_f2"]))


def _homography_coords(B, h, w, seed, scale=1.0, shift=0.0):
    u = torch.from_numpy(mgc.synth.uniform((B, 6), seed).astype(np.float64))
    yy, xx = torch.meshgrid(torch.arange(4 * h, dtype=torch.float64), torch.arange(4 * w, dtype=torch.float64), indexing="ij")
    out = []
    for b in range(B):
        a, s = 0.2 * u[b, 0], scale * (1 + 0.1 * u[b, 1])
        cx, cy = 2.0 * w, 2.0 * h
        x = s * (torch.cos(a) * (xx - cx) - torch.sin(a) * (yy - cy)) + cx + 6 * u[b, 2] + shift
        y = s * (torch.sin(a) * (xx - cx) + torch.cos(a) * (yy - cy)) + cy + 6 * u[b, 3] + shift
        out.append(torch.stack([x, y], -1))
    return torch.stack(out).float()


def _compare(f1, f2, coords, teacher=None, grads=True, rtol=1e-5, **k):
    f1 = f1.clone().requires_grad_(grads)
    f2 = f2.clone().requires_grad_(grads)
    got = _loss(f1, f2, coords, teacher=teacher, **k)
    d1, d2 = f1.detach().double().requires_grad_(grads), f2.detach().double().requires_grad_(grads)
    tk = {kk: v for kk, v in k.items() if kk in ("margin",)}
    tk.update(radius=k.get("safe_radius", 4), steps=k.get("scaling_steps", 2))
    tk.update(tau=k.get("temperature", S["temperature"]), wd=k.get("distill_weight", S["distill_weight"]))
    want = restate(d1, d2, coords, teacher=None if teacher is None else (teacher[0].double(), teacher[1].double()), **tk)
    assert len(got) == len(want) == (3 if teacher is None else 4)
    assert got[0].shape == (1,)
    for a, b in zip(got, want):
        np.testing.assert_allclose(float(a), float(b), rtol=rtol, atol=1e-6)
    if grads:
        got[0].backward()
        want[0].backward()
        _check_grads(f1.grad, d1.grad.float())
        _check_grads(f2.grad, d2.grad.float())
    return got


def test_stage2_batch8_against_float64(dev):
    B, C, h = 8, 256, 40
    f1 = _t(mgc.synth.gaussish((B, C, h, h), 7301), dev)
    f2 = _t(mgc.synth.gaussish((B, C, h, h), 7302), dev)
    t1 = f1 + 0.7 * _t(mgc.synth.gaussish((B, C, h, h), 7303), dev)
    t2 = f2 + 0.7 * _t(mgc.synth.gaussish((B, C, h, h), 7304), dev)
    _compare(f1, f2, _homography_coords(B, h, h, 7305).to(dev), teacher=(t1, t2))


def test_stage1_without_teacher_against_float64(dev):
    B, C, h = 4, 256, 40
    f1 = _t(mgc.synth.gaussish((B, C, h, h), 7311), dev)
    f2 = _t(mgc.synth.gaussish((B, C, h, h), 7312), dev)
    _compare(f1, f2, _homography_coords(B, h, h, 7313).to(dev))


def test_every_candidate_inside_the_safe_radius(dev):
    """8x8 second map, contracted correspondences and a radius that covers both grids: every neg1 / neg2 candidate
    carries the +10 penalty, so min(neg1, neg2) >= 10 - 2 and the hinge is 0 (only the distillation term is live)."""
    B, C, h = 2, 64, 20
    f1 = _t(mgc.synth.gaussish((B, C, h, h), 7321), dev)
    f2 = _t(mgc.synth.gaussish((B, C, 8, 8), 7322), dev)
    t1 = f1 + _t(mgc.synth.gaussish((B, C, h, h), 7323), dev)
    t2 = f2 + _t(mgc.synth.gaussish((B, C, 8, 8), 7324), dev)
    yy, xx = torch.meshgrid(torch.arange(4 * h, dtype=torch.float32), torch.arange(4 * h, dtype=torch.float32), indexing="ij")
    coords = torch.stack([10.5 + xx * 0.24, 10.5 + yy * 0.24], -1)[None].repeat(B, 1, 1, 1).to(dev)
    got = _compare(f1, f2, coords, teacher=(t1, t2), safe_radius=25)
    assert float(got[2]) >= 8.0


def test_repeated_pos2_scatter_add(dev):
    """A contracting map: many rows share a pos2 (rounding collisions), so grad F2 sums several rows per pixel."""
    from c2m_amd import ops
    B, C, h = 2, 128, 40
    f1 = _t(mgc.synth.gaussish((B, C, h, h), 7331), dev)
    f2 = _t(mgc.synth.gaussish((B, C, h, h), 7332), dev)
    coords = _homography_coords(B, h, h, 7333, scale=0.35).to(dev)
    corr = ops.contras_correspondences(coords, h, h, 2)
    p = corr["pos2"][: corr["counts"][0]]
    assert torch.unique(p, dim=0).shape[0] < p.shape[0] // 4
    _compare(f1, f2, coords)


def test_all_samples_skipped_raises(dev):
    f = torch.randn(2, 32, 20, 20, device=dev)
    coords = torch.full((2, 80, 80, 2), 5.0, device=dev)
    with pytest.raises(NotImplementedError):
        _loss(f, f, coords)
    with pytest.raises(NotImplementedError):
        _loss(f, f, coords, teacher=(f, f))


def test_validation_size_forward(dev):
    """One whole-image validation sample (84 x 128 feature maps, ~10^4 rows against ~10^4 positions), forward only."""
    C, h, w = 256, 84, 128
    f1 = _t(mgc.synth.gaussish((1, C, h, w), 7341), dev)
    f2 = _t(mgc.synth.gaussish((1, C, h, w), 7342), dev)
    t1 = f1 + 0.7 * _t(mgc.synth.gaussish((1, C, h, w), 7343), dev)
    t2 = f2 + 0.7 * _t(mgc.synth.gaussish((1, C, h, w), 7344), dev)
    yy, xx = torch.meshgrid(torch.arange(4 * h, dtype=torch.float32), torch.arange(4 * w, dtype=torch.float32), indexing="ij")
    coords = torch.stack([xx * 0.98 + 3.0, yy * 0.98 + 2.0], -1)[None].to(dev)
    with torch.no_grad():
        _compare(f1, f2, coords, teacher=(t1, t2), grads=False)


def test_forward_is_bitwise_reproducible(dev):
    from c2m_amd import ops
    f1, f2, t1, t2, coords = _case("a", dev)
    a = [v.clone() for v in _loss(f1, f2, coords, teacher=(t1, t2))]
    b = [v.clone() for v in _loss(f1, f2, coords, teacher=(t1, t2))]
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    r1 = ops.contras_loss_rows(f1, f2, coords, teacher=(t1, t2))
    r2 = ops.contras_loss_rows(f1, f2, coords, teacher=(t1, t2))
    for k in ("pos", "neg1", "neg2", "neg1_idx", "neg2_idx"):
        assert torch.equal(r1[k], r2[k]), k


# ---- models ---------------------------------------------------------------------------------------------------------

def _opt(stage, tmp_path):
    net = {"type": "ContrasExtractorSep"}
    o = {"model_type": "TeacherContrasModel" if stage == 1 else "StudentContrasDistillationModel", "gpu_ids": [0],
         "is_train": True, "dist": False,
         "path": {"models": str(tmp_path), "training_state": str(tmp_path), "strict_load": True},
         "train": {"lr_g": 1e-4, "margin": 1.0, "safe_radius": 4, "scaling_steps": 2}}
    if stage == 1:
        o["network_g"] = dict(net)
    else:
        o["network_student"], o["network_teacher"] = dict(net), dict(net)
        o["train"].update(temperature=0.15, distill_weight=15)
    return o


def _batch(dev, B=2, size=160):
    g = torch.Generator().manual_seed(3)
    img_in = torch.rand(B, 3, size, size, generator=g)
    up = F.interpolate(F.interpolate(img_in, scale_factor=0.25, mode="bicubic", align_corners=False), scale_factor=4,
                       mode="bicubic", align_corners=False).clamp(0, 1)
    return {"img_in": img_in, "img_in_up": up, "img_ref": torch.rand(B, 3, size, size, generator=g),
            "transformed_coordinate": _homography_coords(B, size // 4, size // 4, 7351)}


@pytest.mark.parametrize("stage", [1, 2])
def test_model_step_updates_student_only_and_matches_restatement(dev, tmp_path, stage):
    import mmsr.models as models
    torch.manual_seed(0)
    model = models.create_model(_opt(stage, tmp_path))
    student = model.net_g if stage == 1 else model.net_student
    before = {k: v.detach().clone() for k, v in student.state_dict().items()}
    teacher_before = None if stage == 1 else {k: v.detach().clone() for k, v in model.net_teacher.state_dict().items()}
    model.feed_data(_batch(dev))
    model.optimize_parameters(1)
    keys = ["loss", "pos_dist", "neg_dist"] + (["distill_loss"] if stage == 2 else [])
    assert list(model.log_dict.keys()) == keys
    changed = [k for k, v in student.state_dict().items() if v.dtype.is_floating_point and not torch.equal(v, before[k])]
    assert any("weight" in k for k in changed)
    if stage == 2:
        for k, v in model.net_teacher.state_dict().items():
            assert torch.equal(v, teacher_before[k]), k
        assert all(p.grad is None for p in model.net_teacher.parameters())
    o = model.output
    teacher = None if stage == 1 else tuple(model.teacher_feat[k].double() for k in ("dense_features1", "dense_features2"))
    want = restate(o["dense_features1"].detach().double(), o["dense_features2"].detach().double(),
                   model.transformed_coordinates, teacher=teacher)
    np.testing.assert_allclose(model.log_dict["loss"], float(want[0]), rtol=1e-5)
    np.testing.assert_allclose(model.log_dict["pos_dist"], float(want[1]), rtol=1e-5)
    if stage == 2:
        np.testing.assert_allclose(model.log_dict["distill_loss"], float(want[3]), rtol=1e-4, atol=1e-6)
    # validation: mean of the loss over a loader (two batches)
    ds = type("D", (), {"opt": {"name": "val"}})()
    loader = type("L", (), {"dataset": ds, "__iter__": lambda s: iter([_batch(dev, 1), _batch(dev, 1)])})()
    stats = model.nondist_validation(loader, 1, None, False)
    assert np.isfinite(stats["loss_val"])
    # save / load round trip
    model.save(0, 7)
    label = "net_g" if stage == 1 else "net_student"
    path = os.path.join(str(tmp_path), f"{label}_7.pth")
    assert os.path.exists(path)
    o2 = _opt(stage, tmp_path)
    o2["path"]["pretrain_model_g" if stage == 1 else "pretrain_model_student"] = path
    m2 = models.create_model(copy.deepcopy(o2))
    s2 = (m2.net_g if stage == 1 else m2.net_student).state_dict()
    for k, v in student.state_dict().items():
        assert torch.equal(v, s2[k]), k
