"""ShortTime without a GPU: the frame count, argument validation, the new C-ABI symbols, and the numpy restatements of
framing (a loop over frames) and overlap-add (np.add.at) that tests/test_gpu_short_time.py holds the kernels to.

The restatement's own round trip (frames under a sqrt-Hann window, overlap-added and normalised) is held to the bound
the GPU tests use: per sample (T + 3) * 2^-52 * mag / den with T = K * ceil(N / hop) terms and mag = sum |ws * y| over
them -- both sides are float64 sums of at most T terms with one product rounding each and one division."""

import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT

ROUND_TRIP = [(1000, 64, 16), (1000, 64, 48), (333, 64, 1), (200, 64, 64), (50, 64, 7), (1000, 64, 80)]


# ------------------------------------------------------------------ restatements
def frames_ref(signal, N, hop, W, window=None, out_dtype=None):
    """frames[f, i] = out_dtype(float64(signal[f hop + i]) * window[i]) inside the signal, 0 behind it."""
    signal = np.asarray(signal)
    out = np.zeros((W, N), dtype=signal.dtype if out_dtype is None else out_dtype)
    for f in range(W):
        seg = signal[f * hop : f * hop + N].astype(np.float64)
        if window is not None:
            seg = seg * window[: seg.size]
        out[f, : seg.size] = seg
    return out


def overlap_add_ref(y, hop, L, counts=None, wa=None, ws=None, normalize=True):
    """-> (out, mag, den): the overlap-add of y (W, K, N), the sum of |ws * y| over the same terms, and the
    overlap-added window product (all ones without windows)."""
    y = np.asarray(y)
    if y.ndim == 2:
        y = y[:, None, :]
    W, K, N = y.shape
    wa = np.ones(N) if wa is None else wa
    ws = np.ones(N) if ws is None else ws
    num, mag, den = np.zeros(L), np.zeros(L), np.zeros(L)
    idx = np.arange(W)[:, None] * hop + np.arange(N)[None, :]  # sample of element (f, i)
    ok = idx < L
    kf = np.full(W, K) if counts is None else np.clip(np.asarray(counts, dtype=np.int64), 0, K)
    np.add.at(den, idx[ok], np.broadcast_to(wa * ws, (W, N))[ok])
    for k in range(K):  # np.add.at adds in index order: ascending f for every sample
        use = ok & (k < kf)[:, None]
        term = ws[None, :] * y[:, k].astype(np.float64)
        np.add.at(num, idx[use], term[use])
        np.add.at(mag, idx[use], np.abs(term)[use])
    if not normalize:
        return num, mag, np.ones(L)
    out = np.zeros(L)
    pos = den > 0
    out[pos] = num[pos] / den[pos]
    return out, mag, den


def ola_bound(mag, den, K, N, hop):
    """Per-sample bound (T + 3) 2^-52 mag / den, T = K ceil(N / hop); inf where den == 0 (checked separately)."""
    T = K * math.ceil(N / hop)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, (T + 3) * 2.0**-52 * mag / den, np.inf)


def sqrt_hann(N):
    return np.sqrt(0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N))


def brute_frame_count(L, N, hop, pad_end):
    """Count frame starts one by one: with padding, frames until the end of the signal is covered -- or, when hop > N
    leaves gaps, until the next frame would start behind the signal (such a frame would hold padding only, and ph_frames
    refuses it); without padding, while the frame is whole."""
    if L < N:
        if not pad_end:
            raise ValueError
        return 1
    w = 1
    if pad_end:
        while (w - 1) * hop + N < L and w * hop < L:
            w += 1
    else:
        while w * hop + N <= L:
            w += 1
    return w


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("pad_end", [True, False])
def test_frame_count_against_brute_force(pad_end):
    from pyperiod_amd import ShortTime

    for N in (1, 7, 64):
        for hop in (1, 3, 64, 80):
            st = ShortTime(N, hop, pad_end=pad_end)
            for L in range(1, 301):
                if L < N and not pad_end:
                    with pytest.raises(ValueError):
                        st.frame_count(L)
                    continue
                W = st.frame_count(L)
                assert W == brute_frame_count(L, N, hop, pad_end), (L, N, hop)
                assert (W - 1) * hop < L  # every frame starts inside the signal
                if hop <= N <= L:  # the closed forms, which need no clipping without gaps
                    assert W == (1 + math.ceil((L - N) / hop) if pad_end else 1 + (L - N) // hop)


def test_argument_validation():
    from pyperiod_amd import ShortTime

    with pytest.raises(ValueError):
        ShortTime(64, 16, window=np.ones(63))
    with pytest.raises(ValueError):
        ShortTime(64, 16, window=np.ones((2, 32)))
    bad = np.ones(64)
    bad[5] = np.nan
    with pytest.raises(ValueError):
        ShortTime(64, 16, window=bad)
    bad[5] = np.inf
    with pytest.raises(ValueError):
        ShortTime(64, 16, window=bad)
    with pytest.raises(ValueError):
        ShortTime(64, 0)
    with pytest.raises(ValueError):
        ShortTime(0, 1)
    with pytest.raises(ValueError):
        ShortTime(64, 16, pad_end=False).frame_count(63)
    assert ShortTime(64, 16, pad_end=True).frame_count(63) == 1
    with pytest.raises(ValueError):
        ShortTime(64, 16).analyze(np.zeros(100), method="find_periods")


def test_constructing_creates_no_engine(monkeypatch):
    import pyperiod_amd.engine as engine_mod
    from pyperiod_amd import ShortTime

    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(engine_mod.PeriodEngine, "__init__", boom)
    monkeypatch.setattr(engine_mod, "default_engine", boom)
    import sys

    monkeypatch.setattr(sys.modules["pyperiod_amd.ShortTime"], "default_engine", boom)  # (the name it imported)
    before = engine_mod._default
    st = ShortTime(64, 16, window=sqrt_hann(64), dtype=np.float32, trunc_to_integer_multiple=True)
    assert st.frame_count(1000) == 60
    assert engine_mod._default is before


def test_new_symbols_in_binding_and_header():
    from pyperiod_amd import _ffi

    text = open(os.path.join(ROOT, "include", "periodhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, arity in (("ph_frames", 11), ("ph_overlap_add", 13)):
        m = re.search(rf"\bint {name}\s*\(([^;]*)\);", text)
        assert m, name
        assert len(m.group(1).split(",")) == arity
        assert len(_ffi.SIGNATURES[name]) == arity
    assert re.search(r"#define PH_FLAG_OLA_NORM 64u", text) and _ffi.PH_FLAG_OLA_NORM == 64
    flags = [_ffi.PH_FLAG_TRUNC, _ffi.PH_FLAG_ORTH, _ffi.PH_FLAG_SINGLE, _ffi.PH_FLAG_DEVICE, _ffi.PH_FLAG_NOSYNC,
             _ffi.PH_FLAG_KEEP_WEIGHTS, _ffi.PH_FLAG_OLA_NORM]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)


def test_entry_points_reject_bad_arguments_without_gpu():
    """NULL pointers, sizes < 1, unknown dtypes and a frame behind the signal are refused before any HIP call."""
    import ctypes

    import __graft_entry__ as ge

    ge.build()
    from pyperiod_amd import _ffi

    lib = _ffi.load()
    buf = ctypes.addressof((ctypes.c_double * 64)())
    E = _ffi.PH_E_ARG
    assert lib.ph_frames(None, buf, 0, 64, 8, 4, 2, None, 0, 0, buf) == E
    assert b"ctx" in lib.ph_last_error()
    assert lib.ph_overlap_add(None, buf, 0, 2, 1, 8, 4, 12, None, None, None, 0, buf) == E
    assert b"ctx" in lib.ph_last_error()


def cpu_engine():
    """A PeriodEngine without a context that takes CPU tensors as if they lived on its device; reaching the library is
    an error.  Everything the binding checks about its arguments runs before that."""
    import torch

    from pyperiod_amd import _ffi
    from pyperiod_amd.engine import PeriodEngine, _Out

    class Reached(Exception):
        pass

    def prep(x):
        x = x.contiguous()
        code = {torch.float64: _ffi.PH_F64, torch.float32: _ffi.PH_F32}[x.dtype]
        return x, code, x.shape[0], x.shape[1], _ffi.PH_FLAG_DEVICE, _Out(x)

    def call(*a, **k):
        raise Reached

    eng = object.__new__(PeriodEngine)
    eng._prep, eng._call, eng._lib = prep, call, type("Lib", (), {"__getattr__": lambda self, name: name})()
    return eng, Reached


def test_numpy_side_array_next_to_a_tensor_is_a_type_error():
    """With torch input every side array is a tensor of the right dtype: a numpy array (or a tensor of another dtype) in
    its place raises TypeError in every method, before the library is called."""
    import torch

    eng, Reached = cpu_engine()
    x, i32 = torch.zeros((4, 16), dtype=torch.float64), lambda *shape: torch.ones(shape, dtype=torch.int32)
    win_t, win_n = torch.ones(16, dtype=torch.float64), np.ones(16)
    with pytest.raises(Reached):
        eng.overlap_add(x, 4, 28, i32(4), win_t, win_t)
    with pytest.raises(Reached):
        eng.frames(x[0], 16, 4, 1, win_t)
    with pytest.raises(Reached):
        eng.qo_fit(x, i32(4, 2), i32(4), max_period=5, window=win_t)
    with pytest.raises(Reached):
        eng.qo_get_periods(i32(4, 2), i32(4, 2), i32(4), x, ccap=4)
    bad = [
        lambda: eng.overlap_add(x, 4, 28, counts=np.ones(4, np.int32)),
        lambda: eng.overlap_add(x, 4, 28, counts=torch.ones(4, dtype=torch.int64)),
        lambda: eng.overlap_add(x, 4, 28, win_a=win_n),
        lambda: eng.overlap_add(x, 4, 28, win_s=win_n),
        lambda: eng.frames(x[0], 16, 4, 1, win_n),
        lambda: eng.qo_fit(x, np.ones((4, 2), np.int32), i32(4)),
        lambda: eng.qo_fit(x, i32(4, 2), np.ones(4, np.int32)),
        lambda: eng.qo_fit(x, i32(4, 2), i32(4), window=win_n),
        lambda: eng.qo_get_periods(np.ones((4, 2), np.int32), i32(4, 2), i32(4), x, ccap=4),
        lambda: eng.qo_get_periods(i32(4, 2), np.ones((4, 2), np.int32), i32(4), x, ccap=4),
        lambda: eng.qo_get_periods(i32(4, 2), i32(4, 2), np.ones(4, np.int32), x, ccap=4),
    ]
    for call in bad:
        with pytest.raises(TypeError, match="on the device of"):
            call()


@pytest.mark.parametrize("L,N,hop", ROUND_TRIP)
def test_restatement_round_trip(L, N, hop):
    from pyperiod_amd import ShortTime

    rng = np.random.default_rng(L * 1000 + hop)
    x = rng.standard_normal(L)
    w = sqrt_hann(N)
    W = ShortTime(N, hop).frame_count(L)
    fr = frames_ref(x, N, hop, W, w)
    out, mag, den = overlap_add_ref(fr, hop, L, None, w, w, True)
    pos = den > 0
    assert pos.sum() >= L // 2  # (hop = 80 > N leaves gaps, a Hann window its first sample)
    err = np.abs(out - x)[pos]
    assert np.all(err <= ola_bound(mag, den, 1, N, hop)[pos]), err.max()
    assert np.all(out[~pos] == 0.0)
