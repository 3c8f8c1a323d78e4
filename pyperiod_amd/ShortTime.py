"""``ShortTime``: the ``Periods`` algorithms over a long signal, frame by frame, on the MI355X engine.

The reference analyses one window per call; a user holds a recording.  ``ShortTime`` cuts the recording into
overlapping frames on the device (``PeriodEngine.frames``), runs one batched ``Periods`` algorithm over them and
overlap-adds the periodic bases it finds back onto the time axis (``PeriodEngine.overlap_add``).  The signal crosses
PCIe once in each direction (L samples up, the per-frame periods / powers and L doubles down); the ``(W, N)`` frames
and the ``(W, K, N)`` bases never leave the device.

    st = ShortTime(4096, 512, window=np.sqrt(np.hanning(4096)))
    res = st.analyze(recording, method="m_best", num=10)
    res.periodic, res.residual            # (L,) float64 each
"""

from __future__ import annotations

import math
from typing import NamedTuple, Optional
from warnings import warn

import numpy as np

from . import _ffi
from .engine import default_engine

_METHODS = ("m_best", "m_best_gamma", "best_correlation", "best_frequency", "small_to_large")


class ShortTimeResult(NamedTuple):
    """What ``ShortTime.analyze`` returns.  ``periods`` / ``powers`` are the per-frame arrays of the engine method
    (``(W, num)``; for small_to_large ``(W, cap)`` with ``counts[f]`` entries used per frame and zeros behind them);
    ``periodic`` is the overlap-added, window-normalised sum of the bases and ``residual = float64(signal) - periodic``."""

    periods: np.ndarray
    powers: np.ndarray
    periodic: np.ndarray
    residual: np.ndarray
    counts: Optional[np.ndarray] = None


def _first(mask):
    return int(np.flatnonzero(mask)[0])


class ShortTime:
    def __init__(self, frame_length, hop, window=None, pad_end=True, dtype=np.float64,
                 trunc_to_integer_multiple=False, orthogonalize=False):
        """`window`: None (rectangular) or `frame_length` finite samples, used as analysis and as synthesis window.
        `pad_end`: the last frame may run past the end of the signal (zero-padded) so that every sample is covered;
        False keeps whole frames only.  `dtype`: float64 or float32, the dtype of the frames (and so of the kernels that
        analyse them).  The two flags are those of ``Periods``.  Nothing here touches the GPU."""
        self.frame_length, self.hop = int(frame_length), int(hop)
        if self.frame_length < 1:
            raise ValueError("frame_length must be >= 1")
        if self.hop < 1:
            raise ValueError("hop must be >= 1")
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError("dtype must be float64 or float32")
        if window is not None:
            window = np.ascontiguousarray(window, dtype=np.float64)
            if window.shape != (self.frame_length,):
                raise ValueError(f"window must be 1-D with frame_length={self.frame_length} samples")
            if not np.all(np.isfinite(window)):
                raise ValueError("window must be finite")
        self.window = window
        self.pad_end = bool(pad_end)
        self._trunc_to_integer_multiple = bool(trunc_to_integer_multiple)
        self._orthogonalize = bool(orthogonalize)

    def frame_count(self, length) -> int:
        """Frames of a signal of `length` samples: 1 + ceil((L - N) / hop) with pad_end, 1 + (L - N) // hop without;
        a signal shorter than a frame is one padded frame, or ValueError without padding.  With hop > N (gaps between
        the frames) the padded count can name a last frame that starts at or behind the end of the signal: it would hold
        padding only, ph_frames refuses it, and it is not counted."""
        L, N = int(length), self.frame_length
        if L < 1:
            raise ValueError("the signal is empty")
        if L < N:
            if not self.pad_end:
                raise ValueError(f"signal of {L} samples is shorter than a frame of {N} and pad_end is False")
            return 1
        if not self.pad_end:
            return 1 + (L - N) // self.hop
        return min(1 + -((N - L) // self.hop), 1 + (L - 1) // self.hop)

    @staticmethod
    def _signal(signal):
        if type(signal).__module__.startswith("torch"):
            if signal.dim() != 1:
                raise ValueError("expected a 1-D signal")
            return signal
        arr = np.asarray(signal)
        if arr.ndim != 1:
            raise ValueError("expected a 1-D signal")
        if arr.dtype not in (np.dtype(np.float64), np.dtype(np.float32)):
            arr = arr.astype(np.float64)
        return np.ascontiguousarray(arr)

    def _device_window(self, like):
        if self.window is None or not type(like).__module__.startswith("torch"):
            return self.window
        import torch

        return torch.as_tensor(self.window, device=like.device)

    def frames(self, signal):
        """(W, frame_length) frames of `signal` in ``dtype``, windowed: numpy in, numpy out; a torch tensor on the
        engine's device gives a tensor."""
        x = self._signal(signal)
        return default_engine().frames(x, self.frame_length, self.hop, self.frame_count(x.shape[0]),
                                       self._device_window(x), self.dtype)

    def overlap_add(self, y, length, counts=None, normalize=True):
        """Overlap-add `y` (W, N) or (W, K, N) onto `length` samples with the window as synthesis window, divided by the
        overlap-added squared window when `normalize` (0.0 where that is zero)."""
        win = self._device_window(y)
        return default_engine().overlap_add(y, self.hop, length, counts, win, win, normalize)

    def analyze(self, signal, method="m_best", **kwargs):
        """Frame `signal`, run ``Periods.<method>`` (its keyword arguments in **kwargs) over the frames and overlap-add
        the bases: -> ShortTimeResult.  One upload of the signal, one download of the results; status words raise what
        the ``Periods`` method raises, with the first offending frame named."""
        if method not in _METHODS:
            raise ValueError(f"method must be one of {_METHODS}")
        import torch  # lazily, as QOPeriods.solve_quadratic does

        x = self._signal(signal)
        if type(x).__module__.startswith("torch"):
            x = x.detach().cpu().numpy()
        L, N = x.shape[0], self.frame_length
        W = self.frame_count(L)
        eng = default_engine()
        dev = torch.device("cuda", eng.device)
        trunc, orth = self._trunc_to_integer_multiple, self._orthogonalize
        xd = torch.as_tensor(x, device=dev)  # the one upload: L samples
        win = None if self.window is None else torch.as_tensor(self.window, device=dev)
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        fr = eng.frames(xd, N, self.hop, W, win, tdt)
        counts = None
        if method in ("m_best", "m_best_gamma"):
            if orth:
                warn("`Orthogonalize = True` has no effect in M-best.")
            num = int(kwargs.pop("num", 5))
            max_length = kwargs.pop("max_length", None)
            min_length = kwargs.pop("min_length", 2)
            self._no_more(kwargs, method)
            if max_length is None:
                max_length = math.floor(N / 3)
            if num > 0:
                per, pw, bases, st = eng.m_best(fr, num, max_length, min_length, method == "m_best_gamma", trunc, orth)
        elif method == "best_correlation":
            num = int(kwargs.pop("num", 5))
            max_length = kwargs.pop("max_length", None)
            ratio = kwargs.pop("ratio", 0.01)
            self._no_more(kwargs, method)
            if max_length is None:
                max_length = math.floor(N / 3)
            if num > 0:
                per, pw, bases, st = eng.best_correlation(fr, num, max_length, ratio, trunc, orth)
        elif method == "best_frequency":
            num = int(kwargs.pop("num", 5))
            win_size = kwargs.pop("win_size", None)
            self._no_more(kwargs, method)
            if win_size is None:
                win_size = N
            elif win_size < N:
                warn("win_size is smaller than the input signal length. It will be truncated and information will be lost.")
            if num > 0:
                per, pw, bases, st = eng.best_frequency(fr, win_size, num, trunc, orth)
        else:
            thresh = kwargs.pop("thresh", 0.1)
            n_periods = kwargs.pop("n_periods", None)
            self._no_more(kwargs, method)
            if n_periods is None:
                n_periods = math.floor(N / 2)
            num = 1
            counts, per, pw, bases, st = eng.small_to_large(fr, thresh, n_periods, trunc, orth)
        x64 = x.astype(np.float64)
        if num == 0:  # the reference's loops do not run: empty per-frame arrays, nothing periodic
            return ShortTimeResult(np.zeros((W, 0), np.uint32), np.zeros((W, 0)), np.zeros(L), x64)
        self._raise_status(st.cpu().numpy(), method)
        periodic = eng.overlap_add(bases, self.hop, L, counts, win, win, True).cpu().numpy()
        per, pw = per.cpu().numpy(), pw.cpu().numpy()
        if counts is None:
            return ShortTimeResult(per.view(np.uint32), pw, periodic, x64 - periodic)
        counts = counts.cpu().numpy()
        used = np.arange(per.shape[1])[None, :] < counts[:, None]
        return ShortTimeResult(np.where(used, per, 0), np.where(used, pw, 0.0), periodic, x64 - periodic, counts)

    @staticmethod
    def _no_more(kwargs, method):
        if kwargs:
            raise TypeError(f"{method}() got an unexpected keyword argument {next(iter(kwargs))!r}")

    @staticmethod
    def _raise_status(status, method):
        """The exceptions of Periods._raise_status / Periods.best_frequency, naming the first frame concerned."""
        if method == "small_to_large" or not np.any(status != _ffi.PH_ST_OK):
            return
        if method == "best_frequency":
            # the spectral peak was bin 0: the reference evaluates 2 * win_size / 0 and int(round(inf))
            raise OverflowError(f"cannot convert float infinity to integer (frame {_first(status != _ffi.PH_ST_OK)})")
        if np.any(status == _ffi.PH_ST_NO_PERIOD):
            raise TypeError(f"{method}: no candidate period has a positive norm (all-zero or NaN window) in frame "
                            f"{_first(status == _ffi.PH_ST_NO_PERIOD)}")
        if np.any(status == _ffi.PH_ST_ITER_CAP):
            raise RuntimeError(f"{method}: iteration bound reached before `num` periods were found in frame "
                               f"{_first(status == _ffi.PH_ST_ITER_CAP)}")
