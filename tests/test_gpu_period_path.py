"""k_period_path on the GPU against the numpy restatement of its definition (tests/period_path_cases.py): path, values,
score and status bit for bit -- the definition rounds every operation once and compares exactly, so there is no
tolerance.  Shapes: every P at which the workgroup takes another shape (one wavefront, a partial one, one to eight
states per thread), every W around the backtrace tile height T of that P (the plan query's), every band from 0 to the
halo and beyond P, jumps from 0 to 1e300."""

import numpy as np
import pytest

from period_path_cases import (PH_ST_NO_PERIOD, PH_ST_OK, period_path_ref, pinned_cost, random_cost, ridge_cost, tie_cost,
                               with_dead_frame, with_forbidden)

pytestmark = pytest.mark.gpu

PS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 1365, 8192)
JUMPS = (0.0, 0.25, 1e-3, 1e300)


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import default_engine

    return default_engine()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(got, want, what):
    """(path, values, score, status) of the engine against the restatement's, bit for bit."""
    path, values, score, status = (np.asarray(a) for a in got)
    wpath, wvalues, wscore, wstatus = want
    assert int(status) == wstatus, what
    assert path.dtype == np.int32 and np.array_equal(path, wpath), what
    assert np.array_equal(bits(values), bits(wvalues)), what
    assert bits(score) == bits(wscore), what


def check(eng, cost, band, jump, what):
    want = period_path_ref(cost, band, jump)
    same(eng.period_path(cost, band, jump), want, what)
    return want


def test_plan_query(eng):
    """The launch shape the other tests build their frame counts from."""
    last = None
    for P in PS:
        block, lds, tile = eng.period_path_plan(P)
        states = -(-P // 1024)  # per thread: as few as 1024 threads allow, and the same for every thread
        assert block == -(-(-(-P // states)) // 64) * 64 and block <= 1024 and block * states >= P
        assert lds <= eng.lds_bytes and tile >= 1
        assert tile * (-(-P // 16) * 16 + 4) <= lds  # the tile and its piece of the path fit the LDS
        assert last is None or tile <= last
        last = tile
    for P in (0, 8193):
        with pytest.raises(ValueError):
            eng.period_path_plan(P)


@pytest.mark.parametrize("P", PS)
def test_shapes_around_the_tile_height(eng, P):
    T = eng.period_path_plan(P)[2]
    frames = sorted({W for W in (1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 257) if W >= 1})
    bands = (0, 1, 8, 64, P + 3)
    seen = set()
    for k, W in enumerate(frames):
        band = bands[(k + P) % len(bands)]
        if band > 64:
            band = 64  # (the entry point takes at most 64; bands of P and more are test_band_beyond_the_table's)
        if W * min(band, P - 1) > 40000:  # the restatement's time, nothing else
            band = 8 if W * min(8, P - 1) <= 40000 else 1
        jump = JUMPS[(k + 2 * P) % len(JUMPS)]
        seen.add(band)
        cost = random_cost(P + W, W, P) if k % 2 == 0 else tie_cost(P + W, W, P)
        check(eng, cost, band, jump, f"P={P} W={W} band={band} jump={jump} ({'random' if k % 2 == 0 else 'ties'})")
    assert len(seen) >= 3


@pytest.mark.parametrize("band", [0, 1, 8, 64])
@pytest.mark.parametrize("jump", JUMPS)
def test_every_band_and_jump(eng, band, jump):
    for P, W in ((65, 37), (1365, 9), (2, 50), (1, 4)):
        check(eng, random_cost(7 * P + band, W, P), band, jump, f"P={P} W={W} band={band} jump={jump} random")
        check(eng, tie_cost(7 * P + band, W, P), band, jump, f"P={P} W={W} band={band} jump={jump} ties")


def test_every_count_of_states_per_thread(eng):
    """One kernel instantiation per count of states a thread holds, 1 .. 8 = ceil(P / 1024), and the workgroup is cut so
    that every thread holds that many: the first and last P of several counts."""
    for P in (1024, 1025, 2048, 2049, 3100, 4097, 5121, 6144, 6145, 7169, 8191):
        check(eng, random_cost(P, 6, P), 3, 0.01, f"P={P} random")
        check(eng, tie_cost(P, 6, P), 64, 0.0, f"P={P} ties")


def test_band_beyond_the_table(eng):
    """band >= P is the unbanded programme: P = 1 .. 64 with band = 64, against the restatement at band P - 1 too."""
    for P in (1, 2, 5, 33, 63, 64):
        for cost in (random_cost(P, 41, P), tie_cost(P, 41, P)):
            want = check(eng, cost, 64, 0.25, f"P={P} band=64")
            full = period_path_ref(cost, max(P - 1, 0), 0.25)
            assert np.array_equal(want[0], full[0]) and want[2] == full[2]


@pytest.mark.parametrize("band,P", [(1, 70), (8, 130), (64, 300)])
def test_ridges(eng, band, P):
    W = 40
    # a ridge that zig-zags by exactly +-band per frame is followed cell by cell
    cost = ridge_cost(W, P, band)
    want = check(eng, cost, band, 0.5, f"ridge +-{band}")
    assert np.array_equal(want[0], np.argmax(cost, axis=1)) and np.all(np.abs(np.diff(want[0])) == band)
    # one that steps band + 1 cannot be: the path leaves it
    cost = ridge_cost(W, P, band + 1)
    want = check(eng, cost, band, 0.5, f"ridge +-{band + 1} under band {band}")
    assert not np.array_equal(want[0], np.argmax(cost, axis=1)) and np.all(np.abs(np.diff(want[0])) <= band)


@pytest.mark.parametrize("P", [65, 1365])
def test_paths_pinned_to_the_halos(eng, P):
    for column in (0, P - 1):
        for band in (8, 64):
            want = check(eng, pinned_cost(30, P, column), band, 0.01, f"P={P} column {column} band {band}")
            assert np.all(want[0] == column)


def test_forbidden_entries_and_dead_frames(eng):
    for P, W in ((65, 50), (1365, 21)):
        cost = with_forbidden(random_cost(P, W, P), P + 1)
        assert np.isnan(cost).any() and np.isposinf(cost).any() and np.isneginf(cost).any()
        want = check(eng, cost, 8, 0.1, f"P={P} NaN, +inf and -inf entries")
        assert want[3] == PH_ST_OK and np.all(np.isfinite(want[1]))
        for frame in (0, W // 2, W - 1):
            want = check(eng, with_dead_frame(cost, frame), 8, 0.1, f"P={P} dead frame {frame}")
            assert want[3] == PH_ST_NO_PERIOD and np.all(want[0] == -1) and want[2] == -np.inf
    # all-forbidden tables of one frame and of one column
    for shape in ((1, 7), (9, 1)):
        want = check(eng, np.full(shape, np.nan), 3, 0.0, f"all NaN {shape}")
        assert want[3] == PH_ST_NO_PERIOD


def test_row_stride_and_the_gap_that_is_never_read(eng):
    import torch

    rng = np.random.default_rng(11)
    for P, W, ld, first in ((65, 30, 200, 3), (1365, 12, 1400, 0), (5, 9, 6, 1)):
        wide = np.full((W, ld), np.nan)
        wide[:, first : first + P] = rng.standard_normal((W, P))
        view = wide[:, first : first + P]
        assert not view.flags.c_contiguous
        want = period_path_ref(view, 4, 0.05)
        assert want[3] == PH_ST_OK
        same(eng.period_path(view, 4, 0.05), want, f"numpy view P={P} ld={ld}")
        t = torch.as_tensor(wide, device=f"cuda:{eng.device}")[:, first : first + P]
        got = eng.period_path(t, 4, 0.05)
        assert all(g.is_cuda for g in got)
        same([g.cpu().numpy() for g in got], want, f"tensor view P={P} ld={ld}")
        # a batch whose maps are slices of one wide array, and one whose layout has to be copied
        stack = np.full((3, W, ld), np.nan)
        for r in range(3):
            stack[r, :, first : first + P] = rng.standard_normal((W, P))
        got = eng.period_path(stack[:, :, first : first + P], 4, 0.05)
        for r in range(3):
            same([g[r] for g in got], period_path_ref(stack[r, :, first : first + P], 4, 0.05), f"batched view {r}")
        odd = np.asfortranarray(view)
        same(eng.period_path(odd, 4, 0.05), want, "a column-major table is copied")


def test_batches_are_their_maps_alone(eng):
    W, P, band, jump = 9, 130, 3, 0.125
    for R in (1, 300):
        cost = random_cost(R, R * W, P).reshape(R, W, P)
        cost[R // 2] = tie_cost(5, W, P)
        if R > 2:
            cost[2, 4] = np.nan  # one map without a path among the others
        path, values, score, status = eng.period_path(cost, band, jump)
        assert path.shape == (R, W) and values.shape == (R, W) and score.shape == (R,) and status.shape == (R,)
        for r in range(R):
            same((path[r], values[r], score[r], status[r]), period_path_ref(cost[r], band, jump), f"R={R} map {r}")
        for r in sorted({0, R // 2, min(2, R - 1), R - 1}):
            alone = eng.period_path(cost[r], band, jump)
            assert alone[0].shape == (W,) and alone[2].shape == ()
            same(alone, (path[r], values[r], score[r], int(status[r])), f"R={R} map {r} alone")
    empty = eng.period_path(np.zeros((0, W, P)), band, jump)
    assert empty[0].shape == (0, W) and empty[2].shape == (0,)
    assert eng.period_path(cost, band, jump, want_values=False)[1] is None


def test_device_tensor_on_a_side_stream_and_a_repeated_call(eng):
    import torch

    P, W = 1025, 600
    cost = random_cost(3, W, P)
    want = period_path_ref(cost, 8, 0.01)
    dev = torch.device("cuda", eng.device)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        t = torch.as_tensor(cost, device=dev)
        first = eng.period_path(t, 8, 0.01)
        second = eng.period_path(t, 8, 0.01)  # the same workspace again
        other = eng.period_path(t[: W // 2], 2, 0.0)  # and a smaller map in between two calls
        third = eng.period_path(t, 8, 0.01)
    side.synchronize()
    for got in (first, second, third):
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.float64
        same([g.cpu().numpy() for g in got], want, "side stream")
    same([g.cpu().numpy() for g in other], period_path_ref(cost[: W // 2], 2, 0.0), "side stream, smaller map")
    same(eng.period_path(cost, 8, 0.01), want, "numpy after tensors")


def test_largest_case(eng):
    W, P = 4096, 1365
    cost = random_cost(99, W, P)
    cost[:, 400] += 0.5 * np.sin(np.arange(W) / 50.0)
    check(eng, cost, 8, 1e-3, "W=4096 P=1365")
