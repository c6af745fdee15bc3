#!/usr/bin/env python3
"""Generates tests/golden/contras_golden.npz by running the REFERENCE's stage-2 loss (StudentContrasDistillationModel.
loss_function) on deterministic inputs, on the CPU.

Runs only where the reference checkout exists.  Nothing of the reference is copied: its model module is imported by path
(with make_golden.stub_third_party() standing in for packages not installed here) and `loss_function` is called on a
stub `self`.  Inputs are synth.py seeds plus seeded 3x3 homographies (stored); the tests rebuild the features and the
transformed coordinates with the functions below.

    python tests/golden/make_golden_contras.py

Case a: C=256, 40x40 maps, B=3 (sample 2 has < 128 valid correspondences) -> the four scalars and the per-row
        neg1 / neg2 arg-mins (recorded from the reference's own torch.min calls).
Case b: C=32, 24x24 maps, B=2 -> the four scalars and the full gradients wrt the student's two feature maps.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import synth  # noqa: E402

CASES = {"a": dict(B=3, C=256, h=40, w=40, seed=7100), "b": dict(B=2, C=32, h=24, w=24, seed=7200)}
SETTINGS = dict(margin=1.0, safe_radius=4, scaling_steps=2, temperature=0.15, distill_weight=15.0)


def homographies(case):
    """[B,3,3] float64: rotation / scale / shear / translation / mild perspective about the image centre, from synth seeds.
    The last sample of case a is pushed mostly off the image (fewer than 128 valid correspondences)."""
    c = CASES[case]
    B, S = c["B"], 4.0 * c["h"]
    u = synth.uniform((B, 8), c["seed"] + 1).astype(np.float64)
    Hs = []
    for b in range(B):
        ang, sc = 0.25 * u[b, 0], 1.0 + 0.15 * u[b, 1]
        sh, tx, ty = 0.1 * u[b, 2], 0.08 * S * u[b, 3], 0.08 * S * u[b, 4]
        px, py = 4e-4 * u[b, 5] * 160.0 / S, 4e-4 * u[b, 6] * 160.0 / S
        if case == "a" and b == B - 1:
            tx, ty = 0.8 * S, 0.75 * S
        A = np.array([[sc * np.cos(ang), -sc * np.sin(ang) + sh, 0.0], [sc * np.sin(ang), sc * np.cos(ang), 0.0],
                      [px, py, 1.0]])
        Cm = np.array([[1.0, 0.0, S / 2], [0.0, 1.0, S / 2], [0.0, 0.0, 1.0]])
        T = np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])
        Hs.append(T @ Cm @ A @ np.linalg.inv(Cm))
    return np.stack(Hs)


def coords_from_homographies(Hs, size):
    """[B, size, size, 2] float32: (x, y) of every image pixel (x = column, y = row) mapped through H, float64 math."""
    yy, xx = np.meshgrid(np.arange(size, dtype=np.float64), np.arange(size, dtype=np.float64), indexing="ij")
    p = np.stack([xx, yy, np.ones_like(xx)], -1)              # [S,S,3]
    q = np.einsum("bij,yxj->byxi", Hs, p)
    return (q[..., :2] / q[..., 2:3]).astype(np.float32)


def features(case):
    """student f1, f2 and teacher t1, t2: [B,C,h,w] float32 (the teacher is the student plus independent noise)."""
    c = CASES[case]
    shp = (c["B"], c["C"], c["h"], c["w"])
    f1, f2 = synth.gaussish(shp, c["seed"] + 2), synth.gaussish(shp, c["seed"] + 3)
    t1 = (f1 + 0.7 * synth.gaussish(shp, c["seed"] + 4)).astype(np.float32)
    t2 = (f2 + 0.7 * synth.gaussish(shp, c["seed"] + 5)).astype(np.float32)
    return f1, f2, t1, t2


def inputs(case):
    c = CASES[case]
    Hs = homographies(case)
    return features(case) + (coords_from_homographies(Hs, 4 * c["h"]), Hs)


def load_reference_student():
    import make_golden
    REF = make_golden.REF
    sys.path.insert(0, REF)
    make_golden.stub_third_party()
    spec = importlib.util.spec_from_file_location(
        "mmsr.models.student_contras_distillation_model", f"{REF}/mmsr/models/student_contras_distillation_model.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


class _RecordingTorch(types.ModuleType):
    """`torch` for the reference module: records the arg-min indices of every torch.min(x, dim=1) call."""

    def __init__(self):
        super().__init__("torch")
        self.records = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def min(self, *a, **k):
        r = torch.min(*a, **k)
        if k.get("dim") == 1:
            self.records.append(r[1].detach().numpy().astype(np.int32))
        return r


def run_reference(mod, case, with_grad):
    f1, f2, t1, t2, coords, Hs = inputs(case)
    s = SETTINGS
    stub = types.SimpleNamespace(device=torch.device("cpu"), margin=s["margin"], safe_radius=s["safe_radius"],
                                 scaling_steps=s["scaling_steps"], temperature=s["temperature"],
                                 distill_weight=s["distill_weight"])
    F1 = torch.from_numpy(f1).requires_grad_(with_grad)
    F2 = torch.from_numpy(f2).requires_grad_(with_grad)
    stub.output = {"dense_features1": F1, "dense_features2": F2}
    stub.teacher_feat = {"dense_features1": torch.from_numpy(t1), "dense_features2": torch.from_numpy(t2)}
    stub.transformed_coordinates = torch.from_numpy(coords)
    rec = _RecordingTorch()
    mod.torch = rec
    try:
        loss, pos, neg, kl = mod.StudentContrasDistillationModel.loss_function(stub)
    finally:
        mod.torch = torch
    out = {f"{case}/scalars": np.array([loss.item(), pos.item(), neg.item(), kl.item()], np.float64),
           f"{case}/homographies": Hs}
    if with_grad:
        loss.backward()
        out[f"{case}/grad_f1"] = F1.grad.numpy().astype(np.float32)
        out[f"{case}/grad_f2"] = F2.grad.numpy().astype(np.float32)
    else:
        # per valid sample: neg2 (over the valid list) then neg1 (over all positions) -- the order of the two calls
        assert len(rec.records) % 2 == 0
        for k in range(len(rec.records) // 2):
            out[f"{case}/argmin_neg2_{k}"] = rec.records[2 * k]
            out[f"{case}/argmin_neg1_{k}"] = rec.records[2 * k + 1]
    return out


def main():
    torch.set_num_threads(4)
    mod = load_reference_student()
    out = {}
    with torch.no_grad():
        out.update(run_reference(mod, "a", False))
    out.update(run_reference(mod, "b", True))
    for k, v in out.items():
        print(k, v.shape, v if v.size <= 4 else "")
    np.savez_compressed(os.path.join(HERE, "contras_golden.npz"), **out)


if __name__ == "__main__":
    main()
