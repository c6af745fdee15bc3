"""CPU: the host side of the stage 1-2 pair generator (mmsr/data/contras_pairs.py): the homography draws, the banded
Pillow coefficient tables the resampling kernel reads, and the Pillow fixture the GPU tests compare against."""
import os

import numpy as np
import pytest
import torch

import make_golden_contras_pairs as mgp


def _hand_corners(rs, size=160, perturb=(0, 10), window=160):
    """The draws of one sample written out one by one -> (rect1, rect2) as float32, corners tl, tr, bl, br."""
    x = rs.randint(perturb[1], max(size, size - window - perturb[1]))
    y = rs.randint(perturb[1], max(size, size - window - perturb[1]))
    src = [(x, y), (x + window, y), (x, y + window), (x + window, y + window)]
    dst = []
    for cx, cy in src:
        dx = rs.randint(perturb[0], perturb[1]) * rs.choice([-1.0, 1.0])
        dy = rs.randint(perturb[0], perturb[1]) * rs.choice([-1.0, 1.0])
        dst.append((cx + dx, cy + dy))
    return np.array(src, dtype=np.float32), np.array(dst, dtype=np.float32)


def _same_state(a, b):
    sa, sb = a.get_state(), b.get_state()
    return sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]


@pytest.mark.parametrize("seed", [0, 3, 11])
def test_homography_maps_the_corners_and_inverts(seed):
    from mmsr.data.contras_pairs import sample_pair_homography
    H, Hi = sample_pair_homography(np.random.RandomState(seed))
    assert H.dtype == np.float64 and Hi.dtype == np.float64 and H.shape == (3, 3) and Hi.shape == (3, 3)
    src, dst = _hand_corners(np.random.RandomState(seed))
    for (x, y), (u, v) in zip(src.astype(np.float64), dst.astype(np.float64)):
        p = H @ np.array([x, y, 1.0])
        assert abs(p[0] / p[2] - u) <= 1e-9 and abs(p[1] / p[2] - v) <= 1e-9
    assert np.abs(H @ Hi - np.eye(3)).max() <= 1e-12
    assert not np.array_equal(src, dst)


def test_homography_consumes_exactly_18_draws_in_order():
    from mmsr.data.contras_pairs import sample_pair_homography
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    for _ in range(3):                # three samples in a row stay in step with the hand-advanced generator
        sample_pair_homography(a)
        b.randint(10, 160), b.randint(10, 160)
        for _ in range(8):
            b.randint(0, 10), b.choice([-1.0, 1.0])
        assert _same_state(a, b)
    b.randint(0, 10)
    assert not _same_state(a, b)


def test_homography_is_reproducible_and_follows_size():
    from mmsr.data.contras_pairs import sample_pair_homography
    one = sample_pair_homography(np.random.RandomState(21))
    two = sample_pair_homography(np.random.RandomState(21))
    assert np.array_equal(one[0], two[0]) and np.array_equal(one[1], two[1])
    other = sample_pair_homography(np.random.RandomState(22))
    assert not np.array_equal(one[0], other[0])
    # size = (height, width): x is drawn against the width first, y against the height
    rs = np.random.RandomState(4)
    H, _ = sample_pair_homography(rs, size=(200, 320), perturb=(0, 10), window=160)
    hand = np.random.RandomState(4)
    x, y = hand.randint(10, 320), hand.randint(10, 200)
    moved = []
    for cx, cy in ((x, y), (x + 160, y), (x, y + 160), (x + 160, y + 160)):
        moved.append((cx + hand.randint(0, 10) * hand.choice([-1.0, 1.0]), cy + hand.randint(0, 10) * hand.choice([-1.0, 1.0])))
    p = H @ np.array([x, y, 1.0])
    assert abs(p[0] / p[2] - moved[0][0]) <= 1e-9 and abs(p[1] / p[2] - moved[0][1]) <= 1e-9
    assert _same_state(rs, hand)


def test_validation_pool_is_private_and_reproducible():
    from mmsr.data.contras_pairs import sample_pair_homography, validation_pool
    np.random.seed(123)
    a = validation_pool(5)
    drawn = np.random.rand()
    np.random.seed(456)
    b = validation_pool(5)
    np.random.seed(123)
    assert np.random.rand() == drawn                     # the global generator was neither read nor reseeded
    assert a.shape == (5, 3, 3) and a.dtype == np.float64 and np.array_equal(a, b)
    rs = np.random.RandomState(0)
    want = np.stack([sample_pair_homography(rs, (160, 160), (0, 10), 160)[1] for _ in range(5)])
    assert np.array_equal(a, want)
    assert np.array_equal(validation_pool(3), a[:3])


@pytest.mark.parametrize("sizes", [(160, 40), (40, 160), (52, 13), (50, 17), (7, 7)])
def test_banded_tables_are_the_band_of_the_dense_matrix(sizes):
    from c2m_amd import ops
    from mmsr.data import pil_bicubic
    n_in, n_out = sizes
    start, count, coeff = ops.pil_bicubic_tables(n_in, n_out)
    dense = pil_bicubic._coeff_matrix(n_in, n_out)
    assert start.dtype == count.dtype == coeff.dtype == torch.int32
    assert start.shape == (n_out,) and count.shape == (n_out,) and coeff.shape[0] == n_out
    assert coeff.shape[1] == int(count.max())
    rebuilt = torch.zeros_like(dense)
    for i in range(n_out):
        s, c = int(start[i]), int(count[i])
        assert 0 <= s and s + c <= n_in and c >= 1
        rebuilt[i, s:s + c] = coeff[i, :c].double()
        assert not coeff[i, c:].any()                    # padding
        nz = dense[i].nonzero()[:, 0]
        assert s <= int(nz.min()) and int(nz.max()) < s + c
    assert torch.equal(rebuilt, dense)
    # the int32 accumulator of the kernel: 255 * sum |c| + 2^21 < 2^31
    assert 255 * int(coeff.abs().sum(1).max()) + (1 << 21) < (1 << 31)
    if n_in == n_out:                                    # an unchanged axis resamples to itself
        assert torch.equal(dense, torch.eye(n_in, dtype=torch.float64) * (1 << 22))


def test_pillow_fixture_matches_the_installed_pillow(golden_dir):
    path = os.path.join(golden_dir, "contras_pairs_pillow.npz")
    assert os.path.getsize(path) < 100 * 1024
    g = np.load(path)
    want = mgp.expected()
    assert sorted(g.files) == sorted(want)
    for k, v in want.items():
        assert g[k].dtype == np.uint8 and np.array_equal(g[k], v), k
    assert g["c52/lq"].shape == (3, 13, 9) and g["c50/odd"].shape == (3, 17, 11) and g["c160/up"].shape == (3, 160, 160)


def test_fixture_agrees_with_the_python_restatement(golden_dir):
    """pil_bicubic_resize (the CPU-capable yardstick of the kernel) gives the fixture's numbers."""
    from mmsr.data.pil_bicubic import pil_bicubic_resize
    g = np.load(os.path.join(golden_dir, "contras_pairs_pillow.npz"))
    for name, c in mgp.CASES.items():
        img = torch.from_numpy(mgp.image(name))
        H, W = c["shape"][1:]
        lq = pil_bicubic_resize(img, H // 4, W // 4)
        assert np.array_equal(lq.numpy(), g[f"{name}/lq"])
        assert np.array_equal(pil_bicubic_resize(lq, H, W).numpy(), g[f"{name}/up"])
    assert np.array_equal(pil_bicubic_resize(torch.from_numpy(mgp.image("c50")), 17, 11).numpy(), g["c50/odd"])


def test_new_operators_reject_cpu_tensors():
    import c2m_amd
    with pytest.raises(c2m_amd.C2MError):
        c2m_amd.ops.pil_bicubic_resize_u8(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), 2, 2)
    with pytest.raises(c2m_amd.C2MError):
        c2m_amd.ops.warp_perspective_u8(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), np.eye(3))


def test_generator_draws_flips_and_checks_its_input():
    """The flip draws come from the generator's own random.Random, three per sample, before anything touches the GPU."""
    import random
    from mmsr.data.contras_pairs import ContrasPairGenerator
    gen = ContrasPairGenerator(seed=9)
    hand = random.Random(9)
    img = torch.arange(2 * 3 * 4 * 4, dtype=torch.uint8).reshape(2, 3, 4, 4)
    out = gen._augment(img)
    for b in range(2):
        s = img[b]
        h, v, r = hand.random() < 0.5, hand.random() < 0.5, hand.random() < 0.5
        if h:
            s = s.flip(2)
        if v:
            s = s.flip(1)
        if r:
            s = s.transpose(1, 2)
        assert torch.equal(out[b], s)
    assert gen.flip_rng.getstate() == hand.getstate()
    off = ContrasPairGenerator(use_flip=False, use_rot=False, seed=9)
    state = off.flip_rng.getstate()
    assert off._augment(img) is img and off.flip_rng.getstate() == state
    with pytest.raises(ValueError):
        ContrasPairGenerator(seed=0)(torch.zeros(1, 3, 10, 12, dtype=torch.uint8))      # not multiples of 4
    with pytest.raises(TypeError):
        ContrasPairGenerator(seed=0)(torch.zeros(1, 3, 8, 8))


def test_transpose_needs_a_square_batch():
    from mmsr.data.contras_pairs import ContrasPairGenerator
    img = torch.zeros(8, 3, 4, 8, dtype=torch.uint8)
    with pytest.raises(ValueError):                      # 8 samples: one of them draws the transpose (fixed seed)
        ContrasPairGenerator(use_flip=False, use_rot=True, seed=1)._augment(img)
    assert ContrasPairGenerator(use_flip=True, use_rot=False, seed=1)._augment(img).shape == img.shape
