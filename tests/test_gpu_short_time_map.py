"""ShortTime.period_map and ShortTime.contour on the GPU.

period_map is held, bit for bit, to the engine call of its kind on frames built on the host (the framing kernel is one
product rounded once and a cast, which numpy restates exactly), for every kind, with and without end padding, a window,
float32 and float64 frames and the two projection flags; and every partition into frame blocks to the unblocked map.
contour is held, bit for bit, to the numpy restatement of the path (tests/period_path_cases.py) run on the map it
returns, tracks the glide signal of the issue within +-1 on every frame, names the frame of an all-NaN map row, and
launches what it says it launches."""

import numpy as np
import pytest

from period_path_cases import glide_signal, period_path_ref

pytestmark = pytest.mark.gpu

N, HOP, L = 256, 64, 3000
KINDS = ("norm", "gamma", "orth", "ramanujan")
KERNEL = {"norm": "k_sweep", "gamma": "k_sweep", "orth": "k_orth_powers", "ramanujan": "k_ramanujan"}


@pytest.fixture(scope="module")
def eng():
    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import default_engine

    return default_engine()


@pytest.fixture(scope="module")
def recording():
    rng = np.random.default_rng(4)
    n = np.arange(L)
    return np.sin(2 * np.pi * n / 23.0) + 0.5 * ((n % 37) == 0) + 0.1 * rng.standard_normal(L)


def sqrt_hann(n):
    return np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * (np.arange(n) + 0.5) / n))


def host_frames(x, st):
    """The frames of ShortTime `st` as k_frames makes them: float64(sample) * window rounded once, cast to the frame
    dtype, zeros behind the end of the signal."""
    W = st.frame_count(x.size)
    idx = np.arange(W)[:, None] * st.hop + np.arange(st.frame_length)[None, :]
    fr = np.where(idx < x.size, x.astype(np.float64)[np.minimum(idx, x.size - 1)], 0.0)
    if st.window is not None:
        fr = fr * st.window[None, :]
    return fr.astype(st.dtype)


def engine_map(eng, fr, kind, lo, hi, trunc=False, orth=False):
    from pyperiod_amd import _ffi

    if kind in ("norm", "gamma"):
        mode = _ffi.PH_SWEEP_NORM if kind == "norm" else _ffi.PH_SWEEP_NORM_GAMMA
        return eng.sweep(fr, lo, hi, mode, trunc, orth)
    if kind == "orth":
        return eng.orth_powers(fr, hi + 1, normalize=True)[:, lo : hi + 1]
    return eng.ramanujan_norms(fr, lo, hi)[:, lo : hi + 1]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def launches(eng, call):
    eng.profile(True)
    try:
        res = call()
        return res, [n for n, _ in eng.profile_read()]
    finally:
        eng.profile(False)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pad_end,window,dtype", [(True, False, np.float64), (False, True, np.float64),
                                                  (True, True, np.float32), (False, False, np.float32)])
def test_period_map_is_the_engine_call_on_host_frames(eng, recording, kind, pad_end, window, dtype):
    from pyperiod_amd import ShortTime

    st = ShortTime(N, HOP, window=sqrt_hann(N) if window else None, pad_end=pad_end, dtype=dtype)
    fr = host_frames(recording, st)
    assert np.array_equal(st.frames(recording), fr)
    for lo, hi in ((2, None), (5, 40), (3, 12)):
        m = st.period_map(recording, kind=kind, min_length=lo, max_length=hi)
        top = N // 3 if hi is None else hi
        assert m.kind == kind and m.periods.dtype == np.int32 and np.array_equal(m.periods, np.arange(lo, top + 1))
        assert m.values.shape == (fr.shape[0], top - lo + 1) and m.values.dtype == np.float64
        assert np.array_equal(bits(m.values), bits(engine_map(eng, fr, kind, lo, top))), (kind, lo, hi)


@pytest.mark.parametrize("kind", ["norm", "gamma"])
@pytest.mark.parametrize("trunc,orth", [(True, False), (False, True), (True, True)])
def test_period_map_applies_the_projection_flags(eng, recording, kind, trunc, orth):
    from pyperiod_amd import ShortTime

    st = ShortTime(N, HOP, window=sqrt_hann(N), trunc_to_integer_multiple=trunc, orthogonalize=orth)
    fr = host_frames(recording, st)
    m = st.period_map(recording, kind=kind)
    assert np.array_equal(bits(m.values), bits(engine_map(eng, fr, kind, 2, N // 3, trunc, orth)))
    plain = ShortTime(N, HOP, window=sqrt_hann(N)).period_map(recording, kind=kind)
    assert not np.array_equal(bits(m.values), bits(plain.values))  # the flags reach the kernel


@pytest.mark.parametrize("kind", KINDS)
def test_every_partition_into_blocks_is_the_unblocked_map(eng, recording, kind):
    from pyperiod_amd import ShortTime

    st = ShortTime(N, HOP, window=sqrt_hann(N))
    W = st.frame_count(L)
    whole, names = launches(eng, lambda: st.period_map(recording, kind=kind))
    assert names == ["k_frames", KERNEL[kind]]
    for B in (1, 7, W - 1, W, W + 1):
        part, names = launches(eng, lambda: st.period_map(recording, kind=kind, block_frames=B))
        assert np.array_equal(bits(part.values), bits(whole.values)), (kind, B)
        assert np.array_equal(part.periods, whole.periods)
        assert names == ["k_frames", KERNEL[kind]] * min(-(-W // B), W), (kind, B)


def test_device_tensor_in_tensors_out(eng, recording):
    import torch

    from pyperiod_amd import ShortTime

    st = ShortTime(N, HOP, window=sqrt_hann(N), pad_end=False)
    used = (st.frame_count(L) - 1) * HOP + N  # whole frames only: the samples behind them are never read
    wide = torch.full((L + 64,), float("nan"), dtype=torch.float64, device=f"cuda:{eng.device}")
    wide[7 : 7 + used] = torch.as_tensor(recording[:used], device=wide.device)
    x = wide[7 : 7 + L]  # NaN before the signal, behind its last whole frame and behind its end
    for kind in KINDS:
        want = st.period_map(recording, kind=kind)
        got = st.period_map(x, kind=kind, block_frames=5)
        assert torch.is_tensor(got.values) and got.values.is_cuda and got.periods.is_cuda and got.periods.dtype == torch.int32
        assert np.array_equal(bits(got.values.cpu().numpy()), bits(want.values)), kind
        assert np.array_equal(got.periods.cpu().numpy(), want.periods)
    x32 = x.to(torch.float32)
    got = st.period_map(x32, kind="gamma")
    assert np.array_equal(bits(got.values.cpu().numpy()), bits(st.period_map(x32.cpu().numpy(), kind="gamma").values))
    c_np = st.contour(recording, return_map=True)
    c_t = st.contour(x, return_map=True)
    assert isinstance(c_t.periods, np.ndarray) and torch.is_tensor(c_t.map.values) and isinstance(c_np.map.values, np.ndarray)
    assert np.array_equal(c_t.periods, c_np.periods) and c_t.score == c_np.score
    assert np.array_equal(bits(c_t.salience), bits(c_np.salience))
    with pytest.raises(ValueError, match="cuda"):
        st.period_map(torch.zeros(L, dtype=torch.float64))


@pytest.mark.parametrize("kind", KINDS)
def test_contour_is_the_restatement_on_its_own_map(eng, recording, kind):
    from pyperiod_amd import ShortTime

    st = ShortTime(N, HOP, window=sqrt_hann(N))
    W = st.frame_count(L)
    for band, jump, lo, hi, B in ((8, 0.0, 2, None, None), (2, 0.01, 5, 60, 7), (0, 0.0, 3, 30, None), (64, 1e-3, 2, None, W)):
        c, names = launches(eng, lambda: st.contour(recording, kind=kind, band=band, jump=jump, min_length=lo, max_length=hi,
                                                     block_frames=B, return_map=True))
        blocks = 1 if B is None else -(-W // B)
        assert names == ["k_frames", KERNEL[kind]] * blocks + ["k_period_path"], (kind, B)
        path, values, score, status = period_path_ref(c.map.values, band, jump)
        assert status == 0
        assert c.periods.dtype == np.int32 and np.array_equal(c.periods, lo + path), (kind, band)
        assert np.array_equal(bits(c.salience), bits(values)) and bits(c.score) == bits(score)
        assert np.array_equal(c.map.periods, np.arange(lo, (N // 3 if hi is None else hi) + 1))
        plain = st.contour(recording, kind=kind, band=band, jump=jump, min_length=lo, max_length=hi, block_frames=B)
        assert plain.map is None and np.array_equal(plain.periods, c.periods) and plain.score == c.score


def test_contour_tracks_the_glide_signal(eng):
    from pyperiod_amd import ShortTime

    x, period_at = glide_signal()
    st = ShortTime(256, 64, pad_end=False)
    W = st.frame_count(x.size)
    truth = np.array([round(period_at(64 * f + 128)) for f in range(W)])
    c = st.contour(x, kind="gamma", band=2, jump=0.002, min_length=8, max_length=85, return_map=True)
    assert W == 61 and c.periods.shape == (W,)
    print("glide: contour error per frame", (c.periods - truth).tolist())
    assert np.all(np.abs(c.periods - truth) <= 1)  # every frame
    argmax = 8 + np.argmax(c.map.values, axis=1)
    print("glide: frames where the per-frame argmax is off by more than 1:", float(np.mean(np.abs(argmax - truth) > 1)))
    assert np.mean(np.abs(argmax - truth) > 1) >= 0.25  # and the map needs the path


def test_contour_names_the_frame_without_a_finite_value(eng, recording):
    from pyperiod_amd import ShortTime

    st = ShortTime(N, HOP, window=sqrt_hann(N))
    x = recording.copy()
    x[10 * HOP + 5] = np.nan  # in the frames 7 .. 10
    for B in (None, 4):
        with pytest.raises(ValueError, match="frame 7 "):
            st.contour(x, kind="gamma", block_frames=B)
    m = st.period_map(x, kind="gamma")
    dead = np.isnan(m.values).all(axis=1)
    assert np.flatnonzero(dead).tolist() == [7, 8, 9, 10] and np.all(np.isfinite(m.values[~dead]))
