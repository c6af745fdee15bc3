"""CPU: the stage 1-2 extractor-training pieces that need no GPU -- registry discovery of the two model classes, the
C-ABI entry points of the fused contrastive loss, and the batched host builder of the valid correspondences."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("c2m_contras_loss_workspace_bytes", "c2m_contras_loss_forward_f32", "c2m_contras_loss_backward_f32")


def test_registry_discovers_both_contrastive_models():
    import mmsr.models as models
    names = {n for m in models._model_modules for n in dir(m)}
    assert "TeacherContrasModel" in names and "StudentContrasDistillationModel" in names


def test_unknown_model_type_still_raises():
    import mmsr.models as models
    with pytest.raises(ValueError, match="not found"):
        models.create_model({"model_type": "NoSuchModel"})


def test_header_declares_and_library_exports_the_loss_entry_points():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "c2m_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(c2m_[a-z0-9_]+)\s*\(", hdr))
    assert set(SYMBOLS) <= declared
    import c2m_amd
    lib = ctypes.CDLL(c2m_amd.LIB_PATH)
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.c2m_abi_version() == 4


def test_workspace_query_and_argument_checks():
    import c2m_amd
    L = c2m_amd._lib.lib()
    s1 = L.c2m_contras_loss_workspace_bytes(8, 256, 40, 40, 12800, 0)
    s2 = L.c2m_contras_loss_workspace_bytes(8, 256, 40, 40, 12800, 1)
    assert s1 >= 4 * (8 * 1600 * 256 + 12800 * 256) and s2 - s1 >= 4 * 4 * 12800 * 256
    assert L.c2m_contras_loss_workspace_bytes(0, 256, 40, 40, 10, 0) == 0
    # checked before any device work: C % 16 (2), C <= 512 (2), a null map (1), a workspace too small (3)
    f = L.c2m_contras_loss_forward_f32
    assert f(None, *[ctypes.c_void_p(8)] * 4, 1, 24, 40, 40, 40, 40, *[ctypes.c_void_p(8)] * 3, 0, 0, 1.0, 4.0, 0.15,
             ctypes.c_void_p(8), ctypes.c_void_p(8), 1 << 30) == 2
    assert f(None, *[ctypes.c_void_p(8)] * 4, 1, 1024, 40, 40, 40, 40, *[ctypes.c_void_p(8)] * 3, 0, 0, 1.0, 4.0, 0.15,
             ctypes.c_void_p(8), ctypes.c_void_p(8), 1 << 30) == 2
    assert f(None, None, *[ctypes.c_void_p(8)] * 3, 1, 256, 40, 40, 40, 40, *[ctypes.c_void_p(8)] * 3, 0, 0, 1.0, 4.0, 0.15,
             ctypes.c_void_p(8), ctypes.c_void_p(8), 1 << 30) == 1
    assert f(None, *[ctypes.c_void_p(8)] * 4, 1, 256, 40, 40, 40, 40, *[ctypes.c_void_p(8)] * 3, 0, 0, 1.0, 4.0, 0.15,
             ctypes.c_void_p(8), ctypes.c_void_p(8), 16) == 3


def test_cpu_tensors_are_rejected():
    import c2m_amd
    with pytest.raises(c2m_amd.C2MError):
        c2m_amd.ops.contras_loss(torch.zeros(1, 16, 8, 8), torch.zeros(1, 16, 8, 8), torch.zeros(1, 32, 32, 2))


def _numpy_builder(coords, H1, W1, steps):
    """The reference's warp + skip test per sample, in numpy (round half to even = np.round)."""
    ids, pos2, counts = [], [], []
    for b in range(coords.shape[0]):
        t = coords[b, ::4, ::4, :2].reshape(-1, 2)
        x, y = t[:, 0], t[:, 1]
        ok = (x > 10) & (x < 4 * W1 - 10) & (y > 10) & (y < 4 * H1 - 10)
        k = np.nonzero(ok)[0]
        if k.size < 128:
            counts.append(0)
            continue
        counts.append(k.size)
        ids.append(k)
        pos2.append(np.stack([np.round(y[k] / 2 ** steps), np.round(x[k] / 2 ** steps)], 1))
    cat = lambda a, s: np.concatenate(a) if a else np.zeros(s)  # noqa: E731
    return cat(ids, (0,)).astype(np.int64), cat(pos2, (0, 2)).astype(np.int64), counts


def _coords_with_edges(B, H1, W1, seed):
    g = torch.Generator().manual_seed(seed)
    c = (torch.rand(B, 4 * H1, 4 * W1, 2, generator=g) * (4 * max(H1, W1) + 20) - 10)
    sub = c[:, ::4, ::4]
    # exact boundary values (strict comparisons) and exact halves after the /4 (half to even)
    edge = torch.tensor([10.0, 4 * W1 - 10.0, 10.0001, 4 * W1 - 10.0001, 18.0, 22.0, 26.0, 30.0, 14.0, 34.0])
    sub[:, 0, :10, 0] = edge
    sub[:, 1, :10, 1] = torch.tensor([10.0, 4 * H1 - 10.0, 10.0001, 4 * H1 - 10.0001, 18.0, 22.0, 26.0, 30.0, 14.0, 34.0])
    sub[:, 1, :10, 0] = 50.0
    sub[:, 0, :10, 1] = 50.0
    c[:, ::4, ::4] = sub
    return c


@pytest.mark.parametrize("H1,W1,steps", [(20, 20, 2), (16, 24, 2), (24, 16, 3)])
def test_host_builder_matches_numpy_restatement(H1, W1, steps):
    import c2m_amd
    c = _coords_with_edges(4, H1, W1, 11 + H1 + steps)
    c[2, ::4, ::4, 0] = 5.0                      # sample 2: nothing valid -> skipped
    r = c2m_amd.ops.contras_correspondences(c, H1, W1, steps)
    ids, pos2, counts = _numpy_builder(c.numpy(), H1, W1, steps)
    assert r["counts"] == counts and counts[2] == 0
    assert r["n_valid"] == sum(1 for n in counts if n > 0)
    assert r["offsets"].tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert np.array_equal(r["ids"].numpy(), ids) and r["ids"].dtype == torch.int32
    assert np.array_equal(r["pos2"].numpy(), pos2) and r["pos2"].dtype == torch.int32
    assert r["keep"].tolist() == [n > 0 for n in counts]


def test_host_builder_rounds_half_to_even_and_margins_are_strict():
    import c2m_amd
    H1 = W1 = 16
    c = torch.full((1, 64, 64, 2), 30.0)
    sub = c[:, ::4, ::4]
    xs = torch.tensor([10.0, 10.0 + 2 ** -10, 54.0, 54.0 - 2 ** -10, 18.0, 22.0, 26.0, 30.0, 14.0, 34.0, 42.0, 46.0, 50.0, 38.0, 12.0, 20.0])
    sub[0, 0, :, 0] = xs
    c[:, ::4, ::4] = sub
    r = c2m_amd.ops.contras_correspondences(c, H1, W1, 2)
    first = r["ids"][r["ids"] < 16].tolist()
    assert first == [k for k in range(16) if k not in (0, 2)]             # x == 10 and x == 4*W1-10 are invalid
    px = r["pos2"][: len(first), 1].tolist()
    want = {1: 3, 3: 13, 4: 4, 5: 6, 6: 6, 7: 8, 8: 4, 9: 8, 10: 10, 11: 12, 12: 12, 13: 10, 14: 3, 15: 5}
    # 18/4 = 4.5 -> 4, 22/4 = 5.5 -> 6, 26/4 = 6.5 -> 6, 30/4 = 7.5 -> 8, 14/4 = 3.5 -> 4, 34/4 = 8.5 -> 8, 42/4 = 10.5 -> 10
    assert px == [want[k] for k in first]
    assert r["pos2"][0, 0].item() == 8                                       # y = 30 -> 7.5 -> 8


def test_host_builder_rejects_a_grid_of_the_wrong_size():
    import c2m_amd
    with pytest.raises(ValueError):
        c2m_amd.ops.contras_correspondences(torch.zeros(1, 60, 64, 2), 16, 16)
