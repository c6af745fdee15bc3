"""GPU tests of the correlation pre-filter's DEFERRED re-score paths (csrc/corr_filter.hip).

The filter hands a query's answer over in one of five ways: (1) one or two listed indices per hot lane, scored by
corr_resolve_kernel; (2) a whole-lane re-score request (`SCAN_FLAG | lane`, the lane's third-best filter score is inside the
band too); (3) a whole-map request (`cnt == -1`, more than KSLOT entries); (4) a running best parked as a 64-bit key and merged
with the scan results by atomicMax (a query with listed AND deferred entries); (5) a full work list (`flags[0]` raised on the
device, the exact sweep overwrites everything).  tests/test_corr_gpu.py reaches (1); this file reaches (2) - (5) on purpose and
reads the filter's tables to prove that it did.

Inputs are PLANTED COPIES: a 3x3xC patch P of a random channel-normalised ref map is written, bit for bit, to chosen ref
positions (never overlapping or touching, so the duplicate elimination leaves them alone) and into the query map.  A planted query
scores |P| = 3 (the Cauchy-Schwarz maximum) on every copy -- identical values, so all copies are inside the filter's band
(2 eps = 8.4e-5 |q| + 1e-6) -- and every other candidate is a near-orthogonal random patch.  Every case checks that on the CPU
in float64 first (copies bitwise equal and exactly where they were planted; min copy score - max other score >= 0.1, about
400 bands), then asserts
  (a) index map and max_val equal the CPU oracle's bit for bit, norm_input False and True,
  (b) the table facts of the case at the planted queries,
  (c) flags[1] (work-list length) == SCAN_FLAG entries within cnt + queries with cnt == -1, counted from the tables."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCAN_FLAG = 0x40000000   # corr_filter.hip: a cand entry that asks for a whole-lane re-score; the low 5 bits are the lane
SCAN_ITEMS = 8192        # corr_filter.h: capacity of the re-score work list
WP = 28                  # corr_filter.h: ref patch columns per x-tile; sweep lane j serves the columns j + 28 k
SCAN_STRIDE = 28 * 32    # corr_filter.hip, corr_scan_kernel: one group of lanes scores the positions p, p + 896, ... of an item
MARGIN = 0.1


@pytest.fixture(scope="module")
def env(dev):
    import c2m_amd
    import c2m_oracle as oracle
    import synth
    return c2m_amd.ops, oracle, synth


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------------------------------------------------------------
# construction and its CPU preconditions (no GPU needed: tests call these before they launch)
# ---------------------------------------------------------------------------------------------------------------------
def _random_maps(oracle, synth, C, hq, hr, seed):
    return (oracle.feature_normalize(synth.gaussish((C,) + hq, seed)), oracle.feature_normalize(synth.gaussish((C,) + hr, seed + 1)))


def _scores64(q, fr):
    """float64 scores of the 3x3xC query patch q against every ref patch: <q, r> / (|r| + 1e-5), [Hrp, Wrp]."""
    f, qq = fr.astype(np.float64), q.astype(np.float64)
    hrp, wrp = fr.shape[1] - 2, fr.shape[2] - 2
    ss = (f * f).sum(0)
    num, den = np.zeros((hrp, wrp)), np.zeros((hrp, wrp))
    for i, j in itertools.product(range(3), range(3)):
        num += np.tensordot(qq[:, i, j], f[:, i:i + hrp, j:j + wrp], axes=(0, 0))
        den += ss[i:i + hrp, j:j + wrp]
    return num / (np.sqrt(den) + 1e-5)


def _copies_of(p, fr):
    """bool [Hrp, Wrp]: ref patches that equal the 3x3xC patch p bit for bit."""
    u, pu = fr.view(np.uint32), np.ascontiguousarray(p).view(np.uint32)
    hrp, wrp = fr.shape[1] - 2, fr.shape[2] - 2
    m = np.ones((hrp, wrp), bool)
    for i, j in itertools.product(range(3), range(3)):
        m &= (u[:, i:i + hrp, j:j + wrp] == pu[:, i, j][:, None, None]).all(0)
    return m


class _Planter:
    """Plants bitwise copies into one (query map, ref map) pair and checks the preconditions every case relies on."""

    def __init__(self, fi, fr):
        self.fi, self.fr, self.ref_pos, self.q_pos, self.groups = fi, fr, [], [], []

    @staticmethod
    def _apart(a, b, gap):
        return abs(a[0] - b[0]) >= gap or abs(a[1] - b[1]) >= gap

    def plant(self, copies, queries):
        """copies: ref patch positions (row, col), the first one is the source P; queries: query patch positions that get P.
        Returns the group: flat ref indices of the copies (n = row * Wrp + col), flat query numbers."""
        wrp, wqp = self.fr.shape[2] - 2, self.fi.shape[2] - 2
        for c in copies:   # 3x3 patches with at least one free pixel row or column between them: neither overlapping nor adjacent
            assert 0 <= c[0] <= self.fr.shape[1] - 3 and 0 <= c[1] < wrp, c
            assert all(self._apart(c, o, 4) for o in self.ref_pos), (c, self.ref_pos)
            self.ref_pos.append(c)
        for q in queries:
            assert 0 <= q[0] <= self.fi.shape[1] - 3 and 0 <= q[1] < wqp, q
            assert all(self._apart(q, o, 3) for o in self.q_pos), (q, self.q_pos)
            self.q_pos.append(q)
        y0, x0 = copies[0]
        p = self.fr[:, y0:y0 + 3, x0:x0 + 3].copy()
        for y, x in copies[1:]:
            self.fr[:, y:y + 3, x:x + 3] = p
        for y, x in queries:
            self.fi[:, y:y + 3, x:x + 3] = p
        g = SimpleNamespace(p=p, copies=list(copies), queries=list(queries), n=sorted(y * wrp + x for y, x in copies),
                            q=[y * wqp + x for y, x in queries], lanes=sorted({x % WP for _, x in copies}))
        self.groups.append(g)
        return g

    def check(self):
        """After ALL groups are planted: copies bitwise equal and nowhere else, every planted query holds P, float64 margin."""
        wrp = self.fr.shape[2] - 2
        for g in self.groups:
            m = _copies_of(g.p, self.fr)
            assert sorted(np.flatnonzero(m).tolist()) == g.n, (g.copies, np.argwhere(m).tolist())
            for y, x in g.queries:
                assert np.array_equal(self.fi[:, y:y + 3, x:x + 3].view(np.uint32), g.p.view(np.uint32))
            s = _scores64(g.p, self.fr)
            margin = s[m].min() - s[~m].max()
            print(f"planted {g.copies}: copy score {s[m].min():.6f}, best other {s[~m].max():.4f}, margin {margin:.4f}")
            assert margin >= MARGIN, margin
            assert g.n[0] // wrp == min(y for y, _ in g.copies)


# ---------------------------------------------------------------------------------------------------------------------
# launch + the assertions every test makes
# ---------------------------------------------------------------------------------------------------------------------
def _work_items(cnt, cand):
    """[B, Nq] work-list entries each query asks for, from the tables: SCAN_FLAG entries within cnt, or one if cnt == -1."""
    listed = np.arange(cand.shape[-1])[None, None, :] < cnt[..., None]
    return (listed & ((cand & SCAN_FLAG) != 0)).sum(-1) + (cnt == -1)


def _launch(env, dev, fi, fr, fallback=False):
    """fi [B,C,Hq,Wq], fr [B,C,Hr,Wr] numpy.  Asserts (a) and (c) for norm_input False and True and flags[0]; returns the tables
    (numpy), the per-query work items, the skip table and the index map of the last launch."""
    ops, oracle, _ = env
    ti, tr = _t(fi, dev), _t(fr, dev)
    out = None
    for norm_input in (False, True):
        with ops.record_corr_skip_table():
            idx, val = ops.feature_match_index_batched(ti, tr, 3, 1, 1, True, norm_input)
            tab, skip = ops.last_corr_filter_tables(), ops.last_corr_skip_table()
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        cnt, cand, flags = tab["cnt"].cpu().numpy(), tab["cand"].cpu().numpy(), tab["flags"].cpu().numpy()
        items = _work_items(cnt, cand)
        print(f"norm_input={norm_input}: flags[0]={flags[0]} flags[1]={flags[1]} items from tables={items.sum()} "
              f"cnt histogram (from -1) {np.bincount(cnt.ravel() + 1).tolist()}")
        assert int(flags[1]) == int(items.sum()), (flags, items.sum())                                   # (c)
        assert (int(flags[0]) != 0) == fallback, flags
        for b in range(fi.shape[0]):                                                                      # (a)
            oi, ov = oracle.feature_match_index(fi[b], fr[b], 3, 1, 1, True, norm_input)
            assert np.array_equal(idx[b], oi), f"sample {b}, norm_input={norm_input}: index map != oracle at {np.argwhere(idx[b] != oi)[:8].tolist()}"
            assert np.array_equal(val[b], ov), f"sample {b}, norm_input={norm_input}: max_val != oracle (bitwise)"
        out = SimpleNamespace(cnt=cnt, cand=cand, flags=flags, items=items, skip=skip.cpu().numpy(), idx=idx.reshape(idx.shape[0], -1),
                              val=val.reshape(val.shape[0], -1), K=cand.shape[-1])
    return out


def _entries(t, b, q):
    return t.cand[b, q, :max(int(t.cnt[b, q]), 0)].tolist()


def _expect_listed(t, b, g):
    """every copy of group g is a plain listed index at its queries, nothing is deferred, the lowest copy wins"""
    for q in g.q:
        assert t.cnt[b, q] == len(g.n) and sorted(_entries(t, b, q)) == g.n, (t.cnt[b, q], _entries(t, b, q), g.n)
        assert t.items[b, q] == 0 and t.idx[b, q] == g.n[0]


def _expect_lane_scans(t, b, g, scan_lanes, listed=()):
    """group g's queries hold one SCAN_FLAG | lane entry per lane of scan_lanes plus the plain indices `listed`, nothing else"""
    want = sorted([SCAN_FLAG | j for j in scan_lanes] + list(listed))
    for q in g.q:
        assert sorted(_entries(t, b, q)) == want, ([hex(e) for e in _entries(t, b, q)], [hex(e) for e in want])
        assert t.items[b, q] == len(scan_lanes) and t.idx[b, q] == g.n[0]


def _expect_whole_map(t, b, g):
    for q in g.q:
        assert t.cnt[b, q] == -1 and t.items[b, q] == 1 and t.idx[b, q] == g.n[0], (t.cnt[b, q], t.idx[b, q], g.n)


# nine copies in nine lanes (0, 4, ..., 24, 2, 6) / eight in eight (1, 5, ..., 25, 3) / four lanes (2, 6, 10, 14) with two copies
# each, for a ref map of at least 24 x 60: rows 16 - 22, 8 - 14 and 0 - 2
NINE_LANES = [(16, 4 * k) for k in range(7)] + [(20, 30), (20, 34)]
EIGHT_LANES = [(8, 1 + 4 * k) for k in range(7)] + [(12, 31)]
FOUR_LANES_TWICE = [(0, 30), (0, 2), (0, 6), (0, 34), (0, 10), (0, 38), (0, 14), (0, 42)]


# ---------------------------------------------------------------------------------------------------------------------
# 1. two copies in one lane: both listed, the resolve kernel breaks the tie towards the lower index
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("copies", [[(10, 33), (18, 5)], [(10, 5), (18, 33)]], ids=["lower_index_in_x_tile_1", "lower_index_in_x_tile_0"])
def test_two_copies_in_one_lane_are_both_listed(env, dev, copies):
    """Ref 24 x 60 (Wrp = 58: two full x-tiles and a ragged one), lane 5.  The sweep meets the x-tile-0 copy first whichever has
    the lower flat index: cnt == 2, both indices listed, no work item, and the lower index wins."""
    _, oracle, synth = env
    fi, fr = _random_maps(oracle, synth, 64, (10, 11), (24, 60), 1100)
    pl = _Planter(fi, fr)
    g = pl.plant(copies, [(0, 0), (4, 5)])
    pl.check()
    assert g.lanes == [5]
    t = _launch(env, dev, fi[None], fr[None])
    _expect_listed(t, 0, g)


# ---------------------------------------------------------------------------------------------------------------------
# 2. three copies in one lane: the lane records only the first two it meets -> whole-lane re-score
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 128, 256])
def test_three_in_a_lane_winner_is_the_one_the_lane_never_recorded(env, dev, C):
    """Columns 1, 29, 57 (lane 1), the lowest flat index in the LAST x-tile: the sweep records the copies of x-tiles 0 and 1 and
    only knows of the third that its score is inside the band.  One SCAN_FLAG | 1 entry; the scan must find (3, 57)."""
    _, oracle, synth = env
    fi, fr = _random_maps(oracle, synth, C, (10, 11), (24, 60), 1200 + C)
    pl = _Planter(fi, fr)
    g = pl.plant([(15, 1), (9, 29), (3, 57)], [(0, 0), (4, 5)])
    pl.check()
    assert g.n[0] == 3 * 58 + 57 and g.lanes == [1]
    t = _launch(env, dev, fi[None], fr[None])
    _expect_lane_scans(t, 0, g, [1])


def test_three_in_one_column(env, dev):
    _, oracle, synth = env
    fi, fr = _random_maps(oracle, synth, 64, (10, 11), (24, 60), 1210)
    pl = _Planter(fi, fr)
    g = pl.plant([(14, 40), (2, 40), (8, 40)], [(2, 3)])
    pl.check()
    t = _launch(env, dev, fi[None], fr[None])
    _expect_lane_scans(t, 0, g, [40 - WP])


@pytest.mark.parametrize("hr,copies", [((452, 60), [(14, 1), (200, 29), (10, 57)]), ((448, 60), [(10, 1), (200, 29), (14, 57)])],
                         ids=["scan_group_meets_the_winner_second", "scan_group_meets_the_winner_first"])
def test_three_in_a_lane_two_copies_meet_in_one_scan_group(env, dev, hr, copies):
    """corr_scan_kernel breaks ties twice: inside a group of lanes (`n < bidx`, positions p, p + 896, ... of the lane's N = columns
    x Hrp candidates, p = column number * Hrp + row) and between groups (atomicMax on the key).  Only a lane with more than 896
    candidates makes one group meet two copies -- hence the tall ref map: the copies in columns 1 and 57 sit 896 positions apart,
    once with the lower flat index met second and once first."""
    _, oracle, synth = env
    fi, fr = _random_maps(oracle, synth, 64, (6, 7), hr, 1220)
    pl = _Planter(fi, fr)
    g = pl.plant(copies, [(1, 2)])
    pl.check()
    hrp = hr[0] - 2
    pos = {c: (c[1] // WP) * hrp + c[0] for c in copies}
    assert abs(pos[copies[0]] - pos[copies[2]]) == SCAN_STRIDE and min(copies) in (copies[0], copies[2])
    t = _launch(env, dev, fi[None], fr[None])
    _expect_lane_scans(t, 0, g, [1])


# ---------------------------------------------------------------------------------------------------------------------
# 3. ragged last x-tile: the lane's candidate count N = ((Wrp - lane + 27) / 28) * Hrp and the p -> n mapping
# ---------------------------------------------------------------------------------------------------------------------
def test_lane_scan_in_a_ragged_last_x_tile(env, dev):
    """Wr = 70: Wrp = 68 = 2 * 28 + 12.  Lane 11 (below the cut) has the columns 11, 39, 67; lane 12 (above) only 12 and 40.  In
    both, the copy with the lowest flat index sits in the lane's LAST column, so a count that drops that column loses the answer;
    a third group has a copy in the very last patch row and column of the map."""
    _, oracle, synth = env
    fi, fr = _random_maps(oracle, synth, 64, (12, 13), (24, 70), 1300)
    pl = _Planter(fi, fr)
    below = pl.plant([(16, 11), (8, 39), (2, 67)], [(0, 0)])
    above = pl.plant([(6, 12), (11, 12), (1, 40)], [(4, 5)])
    corner = pl.plant([(20, 11), (20, 39), (21, 67)], [(8, 9)])
    pl.check()
    assert 68 % WP == 12 and below.n[0] == 2 * 68 + 67 and above.n[0] == 68 + 40 and corner.n[-1] == 22 * 68 - 1
    t = _launch(env, dev, fi[None], fr[None])
    _expect_lane_scans(t, 0, below, [11])
    _expect_lane_scans(t, 0, above, [12])
    _expect_lane_scans(t, 0, corner, [11])


# ---------------------------------------------------------------------------------------------------------------------
# 4. listed and deferred entries in one query: the resolve kernel parks its running best as a key
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("single,triple", [((2, 10), [(6, 33), (12, 5), (18, 5)]), ((20, 10), [(2, 33), (8, 5), (14, 5)])],
                         ids=["listed_copy_has_the_lowest_index", "scanned_copy_has_the_lowest_index"])
def test_parked_key_meets_the_scan_results(env, dev, single, triple):
    """Lane 10 lists its single copy, lane 5 asks for a scan: the listed copy's (value, index) is parked in keys[q] and must
    survive the scan's atomicMax when its index is the lowest -- and lose when a scanned copy's is."""
    _, oracle, synth = env
    fi, fr = _random_maps(oracle, synth, 64, (10, 11), (24, 60), 1400)
    pl = _Planter(fi, fr)
    g = pl.plant([single] + triple, [(0, 0), (4, 5)])
    pl.check()
    assert g.lanes == [5, 10]
    t = _launch(env, dev, fi[None], fr[None])
    _expect_lane_scans(t, 0, g, [5], listed=[single[0] * 58 + single[1]])
    assert (t.cnt[0, g.q] == 2).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the KSLOT boundary
# ---------------------------------------------------------------------------------------------------------------------
def test_kslot_entries_are_listed_and_one_more_scans_the_whole_map(env, dev):
    """Exactly KSLOT = 8 entries (four lanes with two copies each; eight lanes with one) are all listed and resolved without a work
    item; nine entries make cnt == -1 and one whole-map work item.  Three queries of one map."""
    _, oracle, synth = env
    fi, fr = _random_maps(oracle, synth, 64, (12, 16), (24, 60), 1500)
    pl = _Planter(fi, fr)
    four2 = pl.plant(FOUR_LANES_TWICE, [(0, 0)])
    eight = pl.plant(EIGHT_LANES, [(4, 6)])
    nine = pl.plant(NINE_LANES, [(8, 12)])
    pl.check()
    assert four2.lanes == [2, 6, 10, 14] and len(eight.lanes) == 8 and len(nine.lanes) == 9
    t = _launch(env, dev, fi[None], fr[None])
    assert t.K == 8 == len(four2.n) == len(eight.n) and len(nine.n) == t.K + 1
    _expect_listed(t, 0, four2)
    _expect_listed(t, 0, eight)
    _expect_whole_map(t, 0, nine)


# ---------------------------------------------------------------------------------------------------------------------
# 6. whole-map scans with every score negative (pack_key's negative branch)
# ---------------------------------------------------------------------------------------------------------------------
def test_whole_map_scan_with_negative_scores(env, dev):
    """Every query pixel is -u, every ref pixel normalise(u + 0.3 noise), the ref periodic with period 3 along x and 4 along y
    (32 x 42: Nr = 1200, Nq = 120).  Every score is negative, and the best patch of the period repeats in every third column, i.e.
    in more than KSLOT lanes: every query asks for a whole-map scan, whose keys carry negative values."""
    _, oracle, synth = env
    C = 64
    u = oracle.feature_normalize(synth.gaussish((C, 1, 1), 1600))
    base = oracle.feature_normalize(u + 0.3 / np.sqrt(C) * synth.gaussish((C, 4, 3), 1601))
    fr = np.ascontiguousarray(np.tile(base, (1, 8, 14)))
    fi = np.ascontiguousarray(np.broadcast_to(-u, (C, 12, 14)))
    s = _scores64(fi[:, :3, :3], fr)
    assert s.max() < -1.0, s.max()
    t = _launch(env, dev, fi[None], fr[None])
    assert (t.val < 0).all()
    assert (t.idx // 40 < 4).all() and (t.idx % 40 < 3).all(), "ties must resolve into the first period"
    y, x = divmod(int(t.idx[0, 0]), 40)                         # (the oracle's pick: _launch compared the whole map)
    lanes = {int(c) % WP for _, c in np.argwhere(_copies_of(fr[:, y:y + 3, x:x + 3], fr))}
    assert len(lanes) > t.K, lanes
    assert (t.cnt == -1).all(), np.bincount(t.cnt.ravel() + 1)   # every query is the same patch, so "most" is all of them


# ---------------------------------------------------------------------------------------------------------------------
# 7. batch: the deferred queries of samples 1 and 2 must be scored on their own sample's maps
# ---------------------------------------------------------------------------------------------------------------------
def test_deferred_queries_of_later_samples_read_their_own_maps(env, dev):
    """B = 3 with different maps per sample: nothing deferred in sample 0, a lane scan in sample 1, a whole-map scan and a lane scan
    with a parked key in sample 2 (make_scorer derives the sample from a GLOBAL query number)."""
    _, oracle, synth = env
    pairs = [_random_maps(oracle, synth, 64, (10, 11), (24, 60), 1700 + 10 * b) for b in range(3)]
    p1, p2 = _Planter(*pairs[1]), _Planter(*pairs[2])
    lane = p1.plant([(15, 1), (9, 29), (3, 57)], [(3, 4)])
    p1.check()
    whole = p2.plant(NINE_LANES, [(3, 4)])
    parked = p2.plant([(0, 10), (4, 53), (8, 53), (12, 53)], [(7, 0)])   # lane 10 lists the winner, lane 25 is scanned
    p2.check()
    fi, fr = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    t = _launch(env, dev, fi, fr)
    assert t.items[0].sum() == 0 and t.cnt[0].min() >= 1
    _expect_lane_scans(t, 1, lane, [1])
    _expect_whole_map(t, 2, whole)
    _expect_lane_scans(t, 2, parked, [53 - WP], listed=[10])


# ---------------------------------------------------------------------------------------------------------------------
# 8. deferred queries at the edges of the 14-patch query tile and of the query map
# ---------------------------------------------------------------------------------------------------------------------
def test_deferred_queries_at_query_tile_and_map_edges(env, dev):
    """Hqp = 30, Wqp = 31 (no multiples of the query tile TPQ = 14): planted queries at patch rows / columns 13 and 14 (the two sides
    of the tile boundary) and in the last patch row and column, half of them lane scans, half whole-map scans."""
    _, oracle, synth = env
    fi, fr = _random_maps(oracle, synth, 64, (32, 33), (24, 60), 1800)
    pl = _Planter(fi, fr)
    lane = pl.plant([(11, 1), (7, 29), (2, 57)], [(13, 13), (29, 30)])
    whole = pl.plant(NINE_LANES, [(14, 30), (29, 14)])
    pl.check()
    t = _launch(env, dev, fi[None], fr[None])
    _expect_lane_scans(t, 0, lane, [1])
    _expect_whole_map(t, 0, whole)


# ---------------------------------------------------------------------------------------------------------------------
# 9. deferral next to the skip machinery
# ---------------------------------------------------------------------------------------------------------------------
def test_lane_scan_next_to_skipped_rows_and_a_dead_x_tile(env, dev):
    """Ref 40 x 70 with the pixel rows 9 - 20 identical (patch rows 12 - 20 of the sweep are skipped) and constant from pixel column
    54 on (the last live patch column is 54 < 56: x-tile 2 is dead), plus three copies in lane 5 of which the sweep meets the
    winner last.  The oracle's result from the filter itself, and the skip table still shows both."""
    _, oracle, synth = env
    fi, fr = _random_maps(oracle, synth, 64, (12, 13), (40, 70), 1900)
    fr[:, 9:21, :] = fr[:, 9:10, :]
    fr[:, :, 54:] = fr[:, 5:6, 54:55]
    pl = _Planter(fi, fr)
    g = pl.plant([(24, 5), (30, 5), (2, 33)], [(0, 0), (5, 6)])
    pl.check()
    assert np.array_equal(fr[:, 9:21, :], np.broadcast_to(fr[:, 9:10, :], fr[:, 9:21, :].shape))
    t = _launch(env, dev, fi[None], fr[None])
    _expect_lane_scans(t, 0, g, [5])
    assert t.skip[0].tolist() == [[12, 21], [12, 21], [0, 40]], t.skip


# ---------------------------------------------------------------------------------------------------------------------
# 10. the work list overflows / just does not
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,overflow", [(48, True), (44, False)])
def test_work_list_overflow_and_the_size_below_it(env, dev, h, overflow):
    """Ref 14 x 32, fully periodic with period 3 along y and 7 along x: every patch repeats in four lanes (28 / 7) with four or more
    copies each, so every query asks for at least four lane scans.  46 x 46 queries: >= 8464 items > 8192, flags[0] is raised on
    the device and the exact sweep produces the result; 42 x 42: >= 7056 items, the filter's own result stands."""
    _, oracle, synth = env
    C = 64
    fi = oracle.feature_normalize(synth.gaussish((C, h, h), 2000))
    fr = oracle.feature_normalize(np.ascontiguousarray(np.tile(synth.gaussish((C, 3, 7), 2001), (1, 5, 5))[:, :14, :32]))
    oi, _ = oracle.feature_match_index(fi, fr, 3, 1, 1, True, False)
    for n in np.unique(oi):   # lower bound of the construction, from the oracle's arg-max: >= 3 exact copies in >= 4 lanes
        y, x = divmod(int(n), 30)
        per_lane = np.bincount(np.argwhere(_copies_of(fr[:, y:y + 3, x:x + 3], fr))[:, 1] % WP, minlength=WP)
        assert (per_lane >= 3).sum() >= 4, (n, per_lane)
    nq = (h - 2) ** 2
    assert (4 * nq > SCAN_ITEMS) == overflow
    t = _launch(env, dev, fi[None], fr[None], fallback=overflow)
    print(f"work-list length at Hq = Wq = {h}: flags[1] = {t.flags[1]} (construction: >= {4 * nq})")
    assert (t.items[0] >= 4).all() and t.flags[1] >= 4 * nq
    if overflow:
        assert t.flags[1] > SCAN_ITEMS and t.flags[0] != 0
    else:
        assert t.flags[1] <= SCAN_ITEMS and t.flags[0] == 0
