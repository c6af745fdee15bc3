"""GPU parity tests of the correlation / index-search path.  Everything goes through the C-ABI (ctypes -> libc2m_hip.so).

Bar: index maps AND values bit-identical to the CPU oracle (same canonical fp32 order, see oracle/c2m_oracle.c), index
maps identical to the golden vectors produced by the reference's own Python."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env(dev):
    import c2m_amd
    import c2m_oracle as oracle
    import synth
    assert "gfx950" in c2m_amd.device_arch(), c2m_amd.device_arch()
    return c2m_amd.ops, oracle, synth


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def test_library_is_loaded_in_tree(env):
    import c2m_amd
    assert c2m_amd.LIB_PATH.endswith("c2-matching_amd/csrc/libc2m_hip.so")
    with open("/proc/self/maps") as f:
        assert "libc2m_hip.so" in f.read()


def test_feature_normalize_bit_exact(env, dev):
    ops, oracle, synth = env
    x = synth.gaussish((3, 256, 23, 17), 5)
    x[1, :, 4, 5] = 0.0  # an all-zero pixel exercises the 1e-12 clamp
    got = ops.feature_normalize(_t(x, dev)).cpu().numpy()
    want = np.stack([oracle.feature_normalize(x[b]) for b in range(3)])
    assert np.array_equal(got, want)


def _run_case(ops, oracle, dev, fi, fr, patch=3, s_in=1, s_ref=1, is_norm=True, norm_input=True, force_generic=False):
    idx, val = ops.feature_match_index_batched(_t(fi[None], dev), _t(fr[None], dev), patch, s_in, s_ref, is_norm, norm_input,
                                               force_generic=force_generic)
    oi, ov = oracle.feature_match_index(fi, fr, patch, s_in, s_ref, is_norm, norm_input)
    return idx[0].cpu().numpy(), val[0].cpu().numpy(), oi, ov


def test_golden_cases_bit_exact_vs_oracle_and_reference(env, dev, golden_dir):
    ops, oracle, _ = env
    from make_golden import build_inputs, corr_cases
    gold = np.load(f"{golden_dir}/corr_golden.npz")
    for k, (name, C, hq, hr, patch, s_in, s_ref, builder) in enumerate(corr_cases()):
        fi, fr = build_inputs(name, C, hq, hr, builder, 100 + 10 * k)
        for norm_input in (False, True):
            gi, gv, oi, ov = _run_case(ops, oracle, dev, fi, fr, patch, s_in, s_ref, True, norm_input)
            assert gi.dtype == np.int64
            assert np.array_equal(gi, oi), f"{name}: HIP index map != oracle"
            assert np.array_equal(gv, ov), f"{name}: HIP max_val != oracle (bitwise)"
            assert np.array_equal(gi, gold[f"{name}/idx"]), f"{name}: HIP index map != reference golden"
            np.testing.assert_allclose(gv, gold[f"{name}/val_ni{int(norm_input)}"], rtol=0, atol=2e-6)
        gi, gv, oi, ov = _run_case(ops, oracle, dev, fi, fr, patch, s_in, s_ref, False, False)
        assert np.array_equal(gi, oi) and np.array_equal(gv, ov), f"{name}: is_norm=False path"


@pytest.mark.parametrize("C,hq,hr", [(256, (17, 31), (45, 37)), (128, (16, 16), (3, 3)), (64, (3, 3), (33, 70)),
                                      (256, (30, 16), (16, 32)), (256, (44, 44), (62, 33))])
def test_fast_kernel_ragged_shapes(env, dev, C, hq, hr):
    ops, oracle, synth = env
    fi = oracle.feature_normalize(synth.gaussish((C,) + hq, 41))
    fr = oracle.feature_normalize(synth.gaussish((C,) + hr, 42))
    gi, gv, oi, ov = _run_case(ops, oracle, dev, fi, fr)
    assert np.array_equal(gi, oi) and np.array_equal(gv, ov)
    g2, v2, _, _ = _run_case(ops, oracle, dev, fi, fr, force_generic=True)
    assert np.array_equal(g2, oi) and np.array_equal(v2, ov)


def test_batched_samples_are_independent(env, dev):
    ops, oracle, synth = env
    B, C, h, w = 5, 256, 20, 24
    fi = np.stack([oracle.feature_normalize(synth.gaussish((C, h, w), 60 + b)) for b in range(B)])
    fr = np.stack([oracle.feature_normalize(synth.gaussish((C, h, w), 70 + b)) for b in range(B)])
    fr[3, :, :, 12:] = fr[3, :, :, :12]  # exact ties in one sample only
    idx, val = ops.feature_match_index_batched(_t(fi, dev), _t(fr, dev), 3, 1, 1, True, True)
    for b in range(B):
        oi, ov = oracle.feature_match_index(fi[b], fr[b], 3, 1, 1, True, True)
        assert np.array_equal(idx[b].cpu().numpy(), oi) and np.array_equal(val[b].cpu().numpy(), ov)


def test_exact_ties_across_x_tiles_and_rows(env, dev):
    """A ref map that repeats with period 12 horizontally and 10 vertically: every patch has exact duplicates in other
    28-column x-tiles of the sweep (visited later, some with LOWER index) and in other rows.  The reference's
    "first maximum" (lowest flat index) must win whichever tile finds it -- for both row-DMA flavours.  This test never looks at
    the filter's tables; tests/test_corr_rescore_gpu.py reaches the deferred re-score paths on purpose and asserts they were taken."""
    ops, oracle, synth = env
    for wr in (72, 70):   # 72: dwordx4 row DMA, 70: dword row DMA
        fi = oracle.feature_normalize(synth.gaussish((256, 20, 21), 51))
        base = synth.gaussish((256, 10, 12), 52)
        fr = oracle.feature_normalize(np.tile(base, (1, 4, 6))[:, :37, :wr].copy())
        gi, gv, oi, ov = _run_case(ops, oracle, dev, fi, fr)
        assert np.array_equal(gi, oi) and np.array_equal(gv, ov)
        assert int(oi.max()) < 10 * (wr - 2)   # ties resolved into the first vertical period


def _band_ref(oracle, synth, C, hr, seed, bands):
    """ref map with runs of bitwise-identical pixel rows: bands = [(first_row, last_row, x_from)], the run only holding
    for pixel columns >= x_from (0 = whole rows)."""
    fr = oracle.feature_normalize(synth.gaussish((C,) + hr, seed))
    for r0, r1, x0 in bands:
        fr[:, r0:r1 + 1, x0:] = fr[:, r0:r0 + 1, x0:]
    return np.ascontiguousarray(fr)


@pytest.mark.parametrize("hr,bands,expect", [
    ((40, 70), [(9, 20, 0)], {0: (12, 21), 1: (12, 21), 2: (12, 21)}),          # a run in the middle, every x-tile
    ((40, 70), [(0, 6, 0), (30, 39, 0)], {0: (33, 40)}),                         # two runs: the longer (bottom) one wins
    ((40, 70), [(0, 39, 56)], {0: (40, 40), 1: (40, 40), 2: (3, 40)}),           # constant columns: only x-tile 2 skips
    ((40, 70), [(5, 7, 0)], {0: (40, 40)}),                                      # 3 equal rows = 1 patch row: nothing to skip
    ((24, 33), [(4, 12, 0), (14, 23, 0)], {0: (17, 24), 1: (17, 24)}),
])
def test_duplicate_row_elimination_is_exact(env, dev, hr, bands, expect):
    """The MFMA kernel does not sweep ref rows that repeat the three rows before them (zero-padded Refs): index map and
    values must still equal the oracle's, which scores every candidate, and the skip table must be the expected one."""
    ops, oracle, synth = env
    C = 64
    fi = oracle.feature_normalize(synth.gaussish((C, 21, 19), 7))
    fr = _band_ref(oracle, synth, C, hr, 8, bands)
    # some queries ARE patches of the repeated band, so the duplicates are exact ties for the maximum
    fi[:, 2:5, 3:6] = fr[:, bands[0][0]:bands[0][0] + 3, hr[1] - 4:hr[1] - 1]
    idx, val, tab = ops.feature_match_index_batched(_t(fi[None], dev), _t(fr[None], dev), return_skip=True)
    oi, ov = oracle.feature_match_index(fi, fr, 3, 1, 1, True, False)
    assert np.array_equal(idx[0].cpu().numpy(), oi)
    assert np.array_equal(val[0].cpu().numpy(), ov)
    tab = tab[0].cpu().numpy()
    for xt, (a, b) in expect.items():
        assert tuple(tab[xt]) == (a, b), (xt, tab)
    gi, gv = ops.feature_match_index_batched(_t(fi[None], dev), _t(fr[None], dev), force_generic=True)
    assert np.array_equal(gi[0].cpu().numpy(), oi) and np.array_equal(gv[0].cpu().numpy(), ov)


def test_duplicate_rows_differ_per_sample(env, dev):
    ops, oracle, synth = env
    C = 128
    fi = np.stack([oracle.feature_normalize(synth.gaussish((C, 18, 18), 20 + b)) for b in range(3)])
    fr = np.stack([_band_ref(oracle, synth, C, (36, 36), 30, [(20, 35, 0)]),
                   _band_ref(oracle, synth, C, (36, 36), 31, []),
                   _band_ref(oracle, synth, C, (36, 36), 32, [(2, 30, 0)])])
    idx, val, tab = ops.feature_match_index_batched(_t(fi, dev), _t(fr, dev), return_skip=True)
    tab = tab.cpu().numpy()
    assert tab[0].tolist() == [[23, 36], [23, 36]] and tab[1].tolist() == [[36, 36], [36, 36]]
    assert tab[2].tolist() == [[5, 31], [5, 31]]
    for b in range(3):
        oi, ov = oracle.feature_match_index(fi[b], fr[b], 3, 1, 1, True, False)
        assert np.array_equal(idx[b].cpu().numpy(), oi) and np.array_equal(val[b].cpu().numpy(), ov)


def test_midsize_80(env, dev):
    ops, oracle, synth = env
    fi = oracle.feature_normalize(synth.gaussish((256, 80, 80), 81))
    fr = oracle.feature_normalize(synth.gaussish((256, 80, 80), 82))
    gi, gv, oi, ov = _run_case(ops, oracle, dev, fi, fr)
    assert np.array_equal(gi, oi) and np.array_equal(gv, ov)


def test_full_size_160_properties(env, dev):
    """BASELINE config 2 shape (one pair of the batch): fast == generic kernel bitwise over the whole map, oracle on
    a slice of query rows, zero-padded ref (500x500 inside 640x640 -> 125x125 inside 160x160 features) ties -> lowest
    index, and every reported maximum really is the score of the reported index."""
    ops, oracle, synth = env
    C, h = 256, 160
    fi = oracle.feature_normalize(synth.gaussish((C, h, h), 91))
    raw = synth.gaussish((C, h, h), 92)
    raw[:, 125:, :] = raw[:, 125:126, 125:126]
    raw[:, :, 125:] = raw[:, 125:126, 125:126]   # constant "padded" band: thousands of identical ref patches
    fr = oracle.feature_normalize(raw)
    fi[:, 150:, 150:] = fr[:, 130:131, 130:131]   # queries that match the constant band exactly
    ti, tr = _t(fi[None], dev), _t(fr[None], dev)
    idx, val, tab = ops.feature_match_index_batched(ti, tr, 3, 1, 1, True, True, return_skip=True)
    gidx, gval = ops.feature_match_index_batched(ti, tr, 3, 1, 1, True, True, force_generic=True)
    assert torch.equal(idx, gidx) and torch.equal(val, gval)
    # round 5: the last x-tile (patch columns 140 .. 157) lies wholly inside the constant band -- every one of its patches
    # repeats its left neighbour bit for bit and can never be the FIRST maximum -- and is not swept at all: (0, Hr) in the
    # skip table; x-tile 4 (112 .. 139) still holds candidates and keeps its duplicate-ROW entry
    tab = tab[0].cpu().numpy()
    assert tuple(tab[5]) == (0, h), tab
    assert tab[4][0] > 0 and tab[4][1] == h and all(tuple(tab[k]) == tuple(tab[4]) for k in range(5)), tab
    idx, val = idx[0].cpu().numpy(), val[0].cpu().numpy()
    rows = (0, 2)
    oi, ov = oracle.feature_match_index(fi, fr, 3, 1, 1, True, True, qrows=rows)
    assert np.array_equal(idx[rows[0]:rows[1]], oi[rows[0]:rows[1]]) and np.array_equal(val[rows[0]:rows[1]], ov[rows[0]:rows[1]])
    rows = (155, 158)
    oi, ov = oracle.feature_match_index(fi, fr, 3, 1, 1, True, True, qrows=rows)
    assert np.array_equal(idx[rows[0]:rows[1]], oi[rows[0]:rows[1]]) and np.array_equal(val[rows[0]:rows[1]], ov[rows[0]:rows[1]])
    # queries inside the constant block tie on every fully-constant ref patch (ry >= 125 OR rx >= 125):
    # the lowest such index is (ry, rx) = (0, 125)
    assert (idx[150:, 150:] == 125).all()
    assert idx.min() >= 0 and idx.max() < 158 * 158


def test_full_size_160_batch16_whole_maps_vs_reference_and_oracle(env, dev, golden_dir):
    """BASELINE configs[1]: ONE launch over a batch of 16 distinct 160x160x256 pairs.  Every whole index map equals the
    map the reference's own Python produced for that pair (tests/golden/corr_full160_golden.npz: its two-chunk path with
    the strict-> merge, constant-band ties) -- except at the fixture's listed fp32-indeterminate near-ties (3 of 399 424
    queries, float64 margins < 2e-7: the reference's oneDNN summation order decides those; there the HIP result must be
    the other listed candidate, which is the float64-true maximum).  Pairs 0 and 15 additionally equal the oracle on ALL
    rows, indices and values bitwise."""
    ops, oracle, _ = env
    from make_golden import FULL160_PAIRS, check_against_reference_golden, full160_inputs
    g = np.load(f"{golden_dir}/corr_full160_golden.npz")
    pairs = [full160_inputs(b) for b in range(FULL160_PAIRS)]
    fi = torch.stack([torch.from_numpy(p[0]) for p in pairs]).to(dev)
    fr = torch.stack([torch.from_numpy(p[1]) for p in pairs]).to(dev)
    idx, val = ops.feature_match_index_batched(fi, fr, 3, 1, 1, True, True)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    ntie = sum(check_against_reference_golden(idx[b], g[f"idx{b}"], g["near_ties"], b, "HIP") for b in range(FULL160_PAIRS))
    assert ntie == len(g["near_ties"])   # canonical order: the HIP kernel resolves every listed near-tie like the oracle
    np.testing.assert_allclose(val[0], g["val0"], rtol=0, atol=2e-6)
    for b in (0, FULL160_PAIRS - 1):
        oi, ov = oracle.feature_match_index(pairs[b][0], pairs[b][1], 3, 1, 1, True, True)
        assert np.array_equal(idx[b], oi) and np.array_equal(val[b], ov), f"pair {b}: HIP != oracle (bitwise)"


def test_cfg5_320_vs_reference_rows_and_oracle(env, dev, golden_dir):
    """BASELINE configs[4] feature size (320x320x256, Nq = Nr = 101124, the largest map any config asks for): the MFMA
    kernel equals the generic kernel bitwise on the whole map, the reference's output on three slices of query rows
    (golden) and the oracle bitwise on those rows."""
    ops, oracle, _ = env
    from make_golden import CFG5_ROWS, cfg5_inputs
    g = np.load(f"{golden_dir}/corr_cfg5_golden.npz")
    fi, fr = cfg5_inputs()
    ti, tr = _t(fi[None], dev), _t(fr[None], dev)
    idx, val = ops.feature_match_index_batched(ti, tr, 3, 1, 1, True, True)
    gidx, gval = ops.feature_match_index_batched(ti, tr, 3, 1, 1, True, True, force_generic=True)
    assert torch.equal(idx, gidx) and torch.equal(val, gval)
    idx, val = idx[0].cpu().numpy(), val[0].cpu().numpy()
    assert idx.shape == (318, 318) and idx.min() >= 0 and idx.max() < 318 * 318
    for (r0, r1) in CFG5_ROWS:
        assert np.array_equal(idx[r0:r1 - 2], g[f"idx_{r0}"]), f"rows {r0}: HIP index map != reference golden"
        np.testing.assert_allclose(val[r0:r1 - 2], g[f"val_{r0}"], rtol=0, atol=4e-6)   # oneDNN vs canonical order; values ~1
        oi, ov = oracle.feature_match_index(fi, fr, 3, 1, 1, True, True, qrows=(r0, r1 - 2))
        assert np.array_equal(idx[r0:r1 - 2], oi[r0:r1 - 2]) and np.array_equal(val[r0:r1 - 2], ov[r0:r1 - 2])
    # queries inside the constant band tie on every fully-constant ref patch: the lowest such index is (0, 125)
    assert (idx[316:, 300:] == 125).all()


def test_pre_offsets_bit_exact(env, dev, golden_dir):
    ops, oracle, synth = env
    g = np.load(f"{golden_dir}/pre_offset_golden.npz")
    B, C, h, w, s1, s2 = (int(v) for v in g["meta"])
    f1 = synth.gaussish((B, C, h, w), s1)
    f2 = synth.gaussish((B, C, h, w), s2)
    f2[1, :, :, 9:] = 0.0
    n1, n2 = ops.feature_normalize(_t(f1, dev)), ops.feature_normalize(_t(f2, dev))
    idx, _ = ops.feature_match_index_batched(n1, n2, 3, 1, 1, True, True)
    o3, o2, o1 = ops.build_pre_offsets(idx, h, w)
    assert np.array_equal(o3.cpu().numpy(), g["relu3_1"])
    assert np.array_equal(o2.cpu().numpy(), g["relu2_1"])
    assert np.array_equal(o1.cpu().numpy(), g["relu1_1"])
    # subset of scales
    (only2,) = ops.build_pre_offsets(idx, h, w, scales=(2,))
    assert torch.equal(only2, o2)


def test_errors_are_loud(env, dev):
    ops, _, _ = env
    import c2m_amd
    with pytest.raises(c2m_amd.C2MError):
        ops.feature_match_index_batched(torch.zeros(1, 4, 8, 8), torch.zeros(1, 4, 8, 8))  # CPU tensors: no fallback
    with pytest.raises(c2m_amd.C2MError):
        ops.feature_match_index_batched(torch.zeros(1, 4, 2, 8, device=dev), torch.zeros(1, 4, 8, 8, device=dev))
    with pytest.raises(c2m_amd.C2MError):
        ops.feature_normalize(torch.zeros(1, 4, 8, 8, device=dev, dtype=torch.float64))
    with pytest.raises(c2m_amd.C2MError):   # only scales 1, 2, 4 exist: anything else used to return uninitialised memory
        ops.build_pre_offsets(torch.zeros((1, 6, 6), dtype=torch.int64, device=dev), 8, 8, scales=(1, 3))


def test_mmsr_ref_map_util_signature(env, dev):
    ops, oracle, synth = env
    from mmsr.models.archs.ref_map_util import feature_match_index, sample_patches
    fi = oracle.feature_normalize(synth.gaussish((256, 12, 13), 3))
    fr = oracle.feature_normalize(synth.gaussish((256, 14, 11), 4))
    idx, val = feature_match_index(_t(fi, dev), _t(fr, dev), patch_size=3, input_stride=1, ref_stride=1, is_norm=True, norm_input=True)
    oi, ov = oracle.feature_match_index(fi, fr, 3, 1, 1, True, True)
    assert idx.dtype == torch.int64 and tuple(idx.shape) == (10, 11)
    assert np.array_equal(idx.cpu().numpy(), oi) and np.array_equal(val.cpu().numpy(), ov)
    p = sample_patches(_t(fr, dev), 3, 1)
    assert tuple(p.shape) == (256, 3, 3, 12 * 9)
    assert torch.equal(p[:, 1, 2, 9 + 4], _t(fr, dev)[:, 1 + 1, 4 + 2])


# ---------------------------------------------------------------------------------------------------------------------
# the two implementations of the MFMA path: f16-pipe pre-filter + exact re-score (default) and the exact fp32 sweep
# ---------------------------------------------------------------------------------------------------------------------
def _both_modes(ops, fi, fr, **kw):
    out = {}
    for mode in (1, 0):
        with ops.corr_filter_mode(mode), ops.record_corr_skip_table():
            idx, val = ops.feature_match_index_batched(fi, fr, 3, 1, 1, True, True, **kw)
            out[mode] = (idx.cpu().numpy(), val.cpu().numpy(), ops.last_corr_filter_tables())
    return out


@pytest.mark.parametrize("C,hq,hr,B", [(256, (40, 40), (40, 40), 3), (128, (33, 47), (52, 41), 2), (64, (20, 75), (61, 30), 2),
                                        (256, (16, 16), (90, 90), 1)])
def test_prefilter_equals_exact_sweep(env, dev, C, hq, hr, B):
    """Same index maps and values, bit for bit, from the pre-filter path and from the exact sweep; the pre-filter really
    produced its result (no domain fall-back) from short candidate lists that contain the arg-max."""
    ops, oracle, synth = env
    fi = np.stack([oracle.feature_normalize(synth.gaussish((C,) + hq, 300 + b)) for b in range(B)])
    fr = np.stack([oracle.feature_normalize(synth.gaussish((C,) + hr, 400 + b)) for b in range(B)])
    fr[0, :, hr[0] // 2:, :] = fr[0, :, hr[0] // 2:hr[0] // 2 + 1, :]      # a band of identical rows in sample 0
    r = _both_modes(ops, _t(fi, dev), _t(fr, dev))
    assert np.array_equal(r[1][0], r[0][0]) and np.array_equal(r[1][1], r[0][1])
    tab = r[1][2]
    assert int(tab["flags"][0]) == 0, "the pre-filter fell back to the exact sweep on in-domain inputs"
    cnt = tab["cnt"].cpu().numpy()
    assert cnt.min() >= 1 and np.mean(cnt == 1) > 0.8, np.bincount(cnt.ravel() + 1)
    cand = tab["cand"].cpu().numpy()
    one = cnt == 1
    assert np.array_equal(cand[..., 0][one], r[1][0].reshape(B, -1)[one])      # a single candidate IS the answer
    for b in range(B):
        oi, ov = oracle.feature_match_index(fi[b], fr[b], 3, 1, 1, True, True)
        assert np.array_equal(r[1][0][b], oi) and np.array_equal(r[1][1][b], ov)


def test_all_duplicate_middle_band_keeps_later_tiles_live(env, dev):
    """`dead_tiles_kernel` encodes a dead x-tile as (0, Hr) in the duplicate-row table, and both sweeps only honour
    such an entry on a TRAILING set of tiles (they subtract it from the step count up front).  The invariant is by construction --
    a tile is dead iff its first patch column lies beyond the LAST column that holds a non-duplicate patch -- so a band of
    all-duplicate patch columns in the MIDDLE of the ref map (x-tiles 1 .. 2 of 4 entirely constant) must leave the tiles behind it
    live: full maps, values included, equal the oracle's on both implementations, and the table shows no dead tile but the
    trailing one."""
    ops, oracle, synth = env
    C, hq, hr = 256, (18, 22), (24, 120)                       # four x-tiles of 28 patch columns (+ a ragged fifth)
    fi = oracle.feature_normalize(synth.gaussish((C,) + hq, 510))
    fr = oracle.feature_normalize(synth.gaussish((C,) + hr, 511))
    fr[:, :, 26:88] = fr[:, :, 26:27]                           # columns 26 .. 87 constant along x: patch columns 27 .. 85 repeat their left neighbour
    fr[:, :, 26:88] = fr[:, 3:4, 26:88]                         # ... and along y: every patch in x-tiles 1, 2 repeats its upper neighbour too
    fr[:, :, 110:] = fr[:, 5:6, 110:111]                        # a constant trailing band (last live patch column 110 < 112): x-tile 4 IS dead
    r = _both_modes(ops, _t(fi[None], dev), _t(fr[None], dev))
    oi, ov = oracle.feature_match_index(fi, fr, 3, 1, 1, True, True)
    for mode in (1, 0):
        assert np.array_equal(r[mode][0][0], oi) and np.array_equal(r[mode][1][0], ov), mode
    assert int(r[1][2]["flags"][0]) == 0
    with ops.record_corr_skip_table():
        ops.feature_match_index_batched(_t(fi[None], dev), _t(fr[None], dev), 3, 1, 1, True, True)
        skip = ops.last_corr_skip_table().cpu().numpy()[0]     # [x-tile][2]
    dead = [(int(a) == 0 and int(b) == hr[0]) for a, b in skip]
    assert dead[-1] and not any(dead[:-1]), skip               # only the trailing tile; the all-duplicate middle tiles are swept
    assert (oi % (hr[1] - 2)).max() >= 86                       # some query really picked a patch column behind the middle band


def test_filter_mode_reaches_launches_from_worker_threads(env, dev):
    """`with ops.corr_filter_mode(0)` opened on the main thread must still govern a launch made from a worker thread
    (nn.DataParallel replicas launch from such threads).  It does because the mode is a per-call argument of the library: the
    op wrapper reads the block's default on the launching thread and passes it in that launch's flags word; no per-thread
    library state exists.  Observed through the kernel names the profiler records."""
    import threading
    import c2m_amd
    ops, oracle, synth = env
    fi = _t(oracle.feature_normalize(synth.gaussish((256, 20, 20), 71))[None], dev)
    fr = _t(oracle.feature_normalize(synth.gaussish((256, 24, 24), 72))[None], dev)
    seen = {}

    def launch(tag):
        with torch.cuda.device(dev):
            ops.feature_match_index_batched(fi, fr, 3, 1, 1, True, True)
            torch.cuda.synchronize()

    for tag, mode in (("exact", 0), ("filter", 1)):
        c2m_amd.profile_enable(True)
        c2m_amd.profile_collect()
        with ops.corr_filter_mode(mode):
            th = threading.Thread(target=launch, args=(tag,))
            th.start()
            th.join()
        seen[tag] = {n for n, _ in c2m_amd.profile_collect()}
        c2m_amd.profile_enable(False)
    assert "corr_argmax_mfma" in seen["exact"] and "corr_filter" not in seen["exact"], seen
    assert "corr_filter" in seen["filter"], seen


def test_exact_sweep_argument_selects_the_path_per_call(env, dev):
    """`exact_sweep=True` runs the exact fp32 sweep alone, the default call the pre-filter, and an explicit `exact_sweep=False`
    wins over an enclosing `corr_filter_mode(0)`; all three give the same indices and values.  Kernel names from the profiler."""
    import c2m_amd
    ops, oracle, synth = env
    fi = _t(oracle.feature_normalize(synth.gaussish((256, 20, 20), 71))[None], dev)
    fr = _t(oracle.feature_normalize(synth.gaussish((256, 24, 24), 72))[None], dev)
    seen, res = {}, {}

    def launch(tag, **kw):
        c2m_amd.profile_enable(True)
        c2m_amd.profile_collect()
        try:
            res[tag] = ops.feature_match_index_batched(fi, fr, 3, 1, 1, True, True, **kw)
            torch.cuda.synchronize()
            seen[tag] = {n for n, _ in c2m_amd.profile_collect()}
        finally:
            c2m_amd.profile_enable(False)

    launch("exact", exact_sweep=True)
    launch("default")
    with ops.corr_filter_mode(0):
        launch("explicit", exact_sweep=False)
    assert "corr_argmax_mfma" in seen["exact"] and "corr_filter" not in seen["exact"], seen
    assert "corr_filter" in seen["default"] and "corr_filter" in seen["explicit"], seen
    for tag in ("default", "explicit"):
        assert torch.equal(res[tag][0], res["exact"][0]) and torch.equal(res[tag][1], res["exact"][1]), tag


def test_sums_of_squares_from_the_normalisation_kernel_change_nothing(env, dev):
    """Round 6: `feature_normalize(x, with_sumsq=True)` leaves the per-pixel sums of squares (the canonical fmaf chain over the
    stored normalised values) for the matcher, which then skips its own pass over each map.  Same normalised maps, same sums as
    the stand-alone pass (the values max_val is built from: query and ref patch norms), same index maps and values bit for bit -- and an in-place write to the map switches the shortcut off."""
    ops, oracle, synth = env
    a = _t(synth.gaussish((2, 256, 30, 26), 901), dev)
    r = _t(synth.gaussish((2, 256, 34, 40), 902), dev)
    n1, n2 = ops.feature_normalize(a), ops.feature_normalize(r)
    s1, s2 = ops.feature_normalize(a, with_sumsq=True), ops.feature_normalize(r, with_sumsq=True)
    assert torch.equal(n1, s1) and torch.equal(n2, s2)
    assert tuple(s1.c2m_sumsq.shape) == (2, 30 * 26) and float((s1.c2m_sumsq - 1.0).abs().max()) < 1e-5   # (normalised pixels)
    i0, v0 = ops.feature_match_index_batched(n1, n2, 3, 1, 1, True, True)
    i1, v1 = ops.feature_match_index_batched(s1, s2, 3, 1, 1, True, True)
    assert torch.equal(i0, i1) and torch.equal(v0, v1)
    for b in range(2):
        oi, ov = oracle.feature_match_index(oracle.feature_normalize(a[b].cpu().numpy()), oracle.feature_normalize(r[b].cpu().numpy()), 3, 1, 1, True, True)
        assert np.array_equal(i1[b].cpu().numpy(), oi) and np.array_equal(v1[b].cpu().numpy(), ov)
    s2[0, :, 20:, :] = s2[0, :, 20:21, :]                   # an in-place edit: the carried sums are stale now and must not be used
    assert ops._pre_sumsq(s2, 2, 34 * 40) is None
    i2, v2 = ops.feature_match_index_batched(s1, s2, 3, 1, 1, True, True)
    i3, v3 = ops.feature_match_index_batched(n1, torch.Tensor(s2.clone()), 3, 1, 1, True, True)
    assert torch.equal(i2, i3) and torch.equal(v2, v3)


def test_prefilter_leaves_its_domain_through_the_exact_sweep(env, dev):
    """|x| >= 3.99 (f16 pieces would overflow), a degenerate all-zero ref patch (1 / (|r| + 1e-5) > 2) and a NaN each raise the
    device flag; the result is then the exact sweep's -- the oracle's -- without a host round trip."""
    ops, oracle, synth = env
    base_i = oracle.feature_normalize(synth.gaussish((256, 24, 24), 11))
    base_r = oracle.feature_normalize(synth.gaussish((256, 30, 30), 12))
    big = base_r.copy(); big[7, 5, 9] = 6.0
    zero = base_r.copy(); zero[:, 10:14, 3:7] = 0.0
    for name, fr in (("large value", big), ("zero patch", zero)):
        with ops.record_corr_skip_table():
            idx, val = ops.feature_match_index_batched(_t(base_i[None], dev), _t(fr[None], dev), 3, 1, 1, True, True)
            flags = ops.last_corr_filter_tables()["flags"]
        assert int(flags[0]) != 0, name
        oi, ov = oracle.feature_match_index(base_i, fr, 3, 1, 1, True, True)
        assert np.array_equal(idx[0].cpu().numpy(), oi) and np.array_equal(val[0].cpu().numpy(), ov), name


def test_exact_sweep_alone_still_matches_the_oracle(env, dev):
    ops, oracle, synth = env
    fi = oracle.feature_normalize(synth.gaussish((256, 31, 29), 21))
    fr = oracle.feature_normalize(synth.gaussish((256, 40, 59), 22))
    fr[:, :, 30:] = fr[:, :, 1:30]   # exact ties
    with ops.corr_filter_mode(0):
        gi, gv, oi, ov = _run_case(ops, oracle, dev, fi, fr)
    assert np.array_equal(gi, oi) and np.array_equal(gv, ov)


def test_prefilter_near_ties_are_resolved_exactly(env, dev):
    """Ref patches that differ from another one by a few ulps of a few channels: their filter scores fall inside the band, the
    listed candidates are re-scored with the oracle's chain and the oracle's pick comes out (value included)."""
    ops, oracle, synth = env
    fi = oracle.feature_normalize(synth.gaussish((256, 22, 22), 31))
    fr = oracle.feature_normalize(synth.gaussish((256, 26, 52), 32))
    right = fr[:, :, :26].copy()
    rs = np.random.RandomState(5)
    mask = rs.rand(*right.shape) < 0.02
    right[mask] = np.nextafter(right[mask], np.float32(1.0))   # one ulp up on 2 % of the elements
    fr[:, :, 26:] = right
    with ops.record_corr_skip_table():
        gi, gv, oi, ov = _run_case(ops, oracle, dev, fi, fr)
        tab = ops.last_corr_filter_tables()
    assert np.array_equal(gi, oi) and np.array_equal(gv, ov)
    assert int(tab["flags"][0]) == 0 and float((tab["cnt"] >= 2).float().mean()) > 0.5   # the near-twins were both listed


# ---------------------------------------------------------------------------------------------------------------------
# the host dispatch arms no other small case selects: every C with Wr % 4 == 0 (16-byte row DMA), and the dword DMA at
# Wr % 4 == 0 behind a misaligned ref base
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dma_cases(env):
    """(fi, fr, {norm_input: (oracle idx, oracle val)}) per (C, Wr): one query tile against a 5-row ref of two (Wr = 32) or
    three (Wr = 60) x-tiles, the last one ragged at two patch columns.  Computed once, read-only."""
    _, oracle, synth = env
    cases = {}
    for C in (64, 128, 256):
        for Wr in (32, 60):
            fi = oracle.feature_normalize(synth.gaussish((C, 16, 16), 700 + C))
            fr = oracle.feature_normalize(synth.gaussish((C, 5, Wr), 800 + C + Wr))
            cases[C, Wr] = (fi, fr, {ni: oracle.feature_match_index(fi, fr, 3, 1, 1, True, ni) for ni in (False, True)})
    return cases


@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("Wr", [32, 60])
@pytest.mark.parametrize("C", [64, 128, 256])
def test_row_dma_arms_at_every_channel_count(env, dev, dma_cases, C, Wr, misaligned):
    """Wr % 4 == 0 with a 16-byte aligned ref selects corr_argmax_mfma_kernel<C, true>; the same map one float into a larger
    buffer (base % 16 == 4) selects <C, false>.  Either way, with and without norm_input, from the exact sweep and from the
    pre-filter path: the oracle's index map and values bit for bit, and the pre-filter produced its result itself."""
    ops, _, _ = env
    fi, fr, want = dma_cases[C, Wr]
    q = _t(fi[None], dev)
    if misaligned:
        buf = torch.empty(fr.size + 4, dtype=torch.float32, device=dev)
        r = buf[1:1 + fr.size].view(1, C, 5, Wr)
        r.copy_(_t(fr[None], dev))
        assert r.is_contiguous() and r.data_ptr() % 16 == 4
    else:
        r = _t(fr[None], dev)
        assert r.data_ptr() % 16 == 0
    for norm_input in (False, True):
        oi, ov = want[norm_input]
        got = {}
        for mode in (0, 1):
            with ops.corr_filter_mode(mode), ops.record_corr_skip_table():
                idx, val = ops.feature_match_index_batched(q, r, 3, 1, 1, True, norm_input)
                flags = ops.last_corr_filter_tables()["flags"]
            got[mode] = (idx[0].cpu().numpy(), val[0].cpu().numpy())
            assert np.array_equal(got[mode][0], oi) and np.array_equal(got[mode][1], ov), (mode, norm_input)
            if mode == 1:
                assert int(flags[0]) == 0, "the pre-filter fell back to the exact sweep on in-domain inputs"
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


@pytest.mark.parametrize("C", [64, 128, 96])
def test_feature_normalize_bit_exact_small_channel_counts(env, dev, C):
    """C = 64 / 128: the register kernels (test_feature_normalize_bit_exact covers 256); C = 96: the generic one."""
    ops, oracle, synth = env
    x = synth.gaussish((2, C, 7, 9), 60 + C)
    x[1, :, 3, 4] = 0.0
    got = ops.feature_normalize(_t(x, dev)).cpu().numpy()
    assert np.array_equal(got, np.stack([oracle.feature_normalize(x[b]) for b in range(2)]))


def test_filter_diagnostics_do_not_outlive_their_block(env, dev):
    """`record_corr_skip_table()` resets both diagnostics slots when a block opens: the pre-filter tables an earlier block
    recorded must not be readable in a later one.  Before the reset covered `filter` too, `last_corr_filter_tables()` returned
    the previous block's tables until the new block's first launch (the first assertion inside the second block failed there; a
    generic launch, which records nothing, then has to leave the slot empty as well)."""
    import c2m_amd
    ops, oracle, synth = env
    fi = _t(oracle.feature_normalize(synth.gaussish((64, 8, 8), 91))[None], dev)
    fr = _t(oracle.feature_normalize(synth.gaussish((64, 6, 7), 92))[None], dev)
    with ops.record_corr_skip_table():
        ops.feature_match_index_batched(fi, fr, 3, 1, 1, True, True)
        assert ops.last_corr_filter_tables()["cnt"].shape == (1, 36)
    with ops.record_corr_skip_table():
        with pytest.raises(c2m_amd.C2MError):
            ops.last_corr_filter_tables()
        with pytest.raises(c2m_amd.C2MError):
            ops.last_corr_skip_table()
        ops.feature_match_index_batched(fi, fr, 3, 1, 1, True, True, force_generic=True)
        with pytest.raises(c2m_amd.C2MError):
            ops.last_corr_filter_tables()
