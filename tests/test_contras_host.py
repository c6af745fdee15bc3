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
    assert lib.c2m_abi_version() == 6


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
    # (x, y) drawn per axis from [-4, 4 * size + 4): some positions fall outside, yet every sample keeps >= 128 rows
    c = torch.rand(B, 4 * H1, 4 * W1, 2, generator=g) * torch.tensor([4.0 * W1 + 8, 4.0 * H1 + 8]) - 4
    sub = c[:, ::4, ::4]
    # exact boundary values (strict comparisons) and exact halves after the /4 (half to even)
    edge = torch.tensor([10.0, 4 * W1 - 10.0, 10.0001, 4 * W1 - 10.0001, 18.0, 22.0, 26.0, 30.0, 14.0, 34.0])
    sub[:, 0, :10, 0] = edge
    sub[:, 1, :10, 1] = torch.tensor([10.0, 4 * H1 - 10.0, 10.0001, 4 * H1 - 10.0001, 18.0, 22.0, 26.0, 30.0, 14.0, 34.0])
    sub[:, 1, :10, 0] = 50.0
    sub[:, 0, :10, 1] = 50.0
    c[:, ::4, ::4] = sub
    return c


@pytest.mark.parametrize("H1,W1,steps", [(20, 20, 2), (16, 24, 2), (24, 16, 3), (33, 21, 3), (24, 36, 2)])
def test_host_builder_matches_numpy_restatement(H1, W1, steps):
    import c2m_amd
    base = _coords_with_edges(4, H1, W1, 11 + H1 + steps)
    # skipped samples: the middle one (2), the first, the first and a middle one, two neighbours, the last, none
    for skipped in ((2,), (0,), (0, 2), (1, 2), (3,), ()):
        c = base.clone()
        for b in skipped:
            c[b, ::4, ::4, 0] = 5.0              # nothing valid -> skipped
        r = c2m_amd.ops.contras_correspondences(c, H1, W1, steps)
        ids, pos2, counts = _numpy_builder(c.numpy(), H1, W1, steps)
        assert r["counts"] == counts and [b for b in range(4) if counts[b] == 0] == list(skipped)   # the others are live
        assert r["n_valid"] == sum(1 for n in counts if n > 0) == 4 - len(skipped)
        off = r["offsets"].tolist()
        assert off == np.concatenate([[0], np.cumsum(counts)]).tolist() and r["offsets"].dtype == torch.int32
        assert all(off[b] == off[b + 1] for b in skipped) and all(off[b] <= off[b + 1] for b in range(4))
        assert np.array_equal(r["ids"].numpy(), ids) and r["ids"].dtype == torch.int32
        assert np.array_equal(r["pos2"].numpy(), pos2) and r["pos2"].dtype == torch.int32
        assert r["keep"].tolist() == [n > 0 for n in counts]
        for b in range(4):                       # ascending grid indices within every sample
            assert bool((r["ids"][off[b]:off[b + 1]].diff() > 0).all())


def test_unsupported_channel_counts_write_nothing():
    """C = 24 (not a multiple of 16) and C = 528 (above 512) answer C2M_ERR_UNSUPPORTED (2) from the forward and the
    backward before any device work: the buffers handed in (host memory here) keep their contents."""
    import c2m_amd
    L = c2m_amd._lib.lib()
    n = 200
    for C in (24, 528):
        f = np.ones(C * 400, np.float32)
        ids, pos2 = np.arange(n, dtype=np.int32), np.zeros(2 * n, np.int32)
        off = np.array([0, n], np.int32)
        out, gf = np.full(4, 7.0, np.float32), np.full(C * 400, 5.0, np.float32)
        ws, g = np.full(1 << 16, 3, np.uint8), np.ones(2, np.float32)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        assert L.c2m_contras_loss_forward_f32(None, p(f), p(f), None, None, 1, C, 20, 20, 20, 20, p(ids), p(pos2), p(off), n, n,
                                              1.0, 4.0, 0.15, p(out), p(ws), 1 << 30) == 2
        assert L.c2m_contras_loss_backward_f32(None, 1, C, 20, 20, 20, 20, p(ids), p(pos2), p(off), n, n, 1.0, 4.0, 0.15, 0,
                                               p(g), p(gf), p(gf), p(ws), 1 << 30) == 2
        assert (out == 7.0).all() and (gf == 5.0).all() and (ws == 3).all() and (f == 1.0).all()
        # the neighbours on the admitted side get past the channel check (and stop at the workspace size: 3)
    for C in (16, 512):
        assert L.c2m_contras_loss_forward_f32(None, *[ctypes.c_void_p(8)] * 4, 1, C, 20, 20, 20, 20, *[ctypes.c_void_p(8)] * 3,
                                              n, n, 1.0, 4.0, 0.15, ctypes.c_void_p(8), ctypes.c_void_p(8), 16) == 3


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
