"""``ShortTime``: the ``Periods`` algorithms over a long signal, frame by frame, on the MI355X engine.

The reference analyses one window per call; a user holds a recording.  ``ShortTime`` cuts the recording into
overlapping frames on the device (``PeriodEngine.frames``), runs one batched ``Periods`` algorithm over them and
overlap-adds the periodic bases it finds back onto the time axis (``PeriodEngine.overlap_add``).  The signal crosses
PCIe once in each direction (L samples up, the per-frame periods / powers and L doubles down); the ``(W, N)`` frames
and the ``(W, K, N)`` bases never leave the device.

    st = ShortTime(4096, 512, window=np.sqrt(np.hanning(4096)))
    res = st.analyze(recording, method="m_best", num=10)
    res.periodic, res.residual            # (L,) float64 each

``decompose`` splits the periodic part by period: the same pipeline, then one routed overlap-add
(``PeriodEngine.overlap_add_tracks``) of the same bases onto one waveform per track.

    dec = st.decompose(recording, method="m_best", num=10, max_tracks=8)
    dec.track_periods, dec.tracks, dec.other, dec.activity

Both take ``block_frames=B`` for a recording whose frames and bases do not fit the device at once: the frames are
analysed B at a time and every block's bases are added into a running sum of the size of the result
(``PeriodEngine.overlap_add_block``, then one ``overlap_add_finish``) -- the same result, bit for bit.

    res = st.analyze(recording, method="m_best", num=10, block_frames=256)

``decompose_qo`` is the same split by ``QOPeriods``: ``find_periods`` and ``get_periods`` on every frame -- one waveform
of p samples per period -- and one routed overlap-add that tiles those waveforms on the fly
(``PeriodEngine.overlap_add_periodic``), so no ``(W, K, N)`` array exists even on the device.

    dq = st.decompose_qo(recording, num=4, thresh=0.1)
    dq.track_periods, dq.tracks, dq.other, dq.periodic, dq.residual

``decompose_ramanujan`` is that split by ``RamanujanPeriods``: the Ramanujan norms of every frame (the time-period map
of the recording), a threshold against the frame, the recording or an absolute level that keeps at most `max_periods`
periods per frame (``PeriodEngine.ramanujan_select``), ``find_periods_with_weights``' fit of those lists and the same
routed overlap-add.

    dr = st.decompose_ramanujan(recording, thresh=0.2, reference="recording", max_periods=16)
    dr.norms, dr.over, dr.frame_status, dr.track_periods, dr.tracks, dr.periodic

``period_map`` is the time-period map of a recording for any of the periodic norms -- frames x periods, the periodicity
analogue of a spectrogram -- and ``contour`` the period of the recording at every frame: the best path through that map
(``PeriodEngine.period_path``), which a jump to a multiple of the true period costs more than it gains.

    m = st.period_map(recording, kind="gamma")          # m.periods (P,), m.values (W, P)
    c = st.contour(recording, kind="gamma", band=8, jump=0.002)
    c.periods, c.salience, c.score

``follow`` is the sound along such a track: one kernel cuts the frames from the recording itself and takes, frame by
frame, the projection onto the period the track names there (``PeriodEngine.follow``), and the routed overlap-add of
``decompose_qo`` tiles those single periods back onto the time axis -- no frames x samples array exists.

    f = st.follow(recording, c)                         # or an edited c.periods, or a list of tracks
    f.tracks, f.periodic, f.residual, f.powers

``contours`` finds the tracks of several sources by peeling: round k takes the best path through the map of what the
tracks before it left of every frame (``PeriodEngine.follow_residual``: ``follow``'s kernel, keeping the residual frames
it otherwise throws away), so the tracks are tracks of exactly what ``follow`` then extracts.

    cs = st.contours(recording, 2, kind="gamma", band=8, jump=0.002)
    cs.periods, cs.salience, cs.scores                  # (W, 2), (W, 2), (2,)
    st.follow(recording, cs).tracks                     # (2, L)
"""

from __future__ import annotations

import math
from functools import cached_property
from typing import NamedTuple, Optional
from warnings import warn

import numpy as np

from . import _ffi
from .engine import _is_torch, default_engine

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


class ShortTimeTracks(NamedTuple):
    """What ``ShortTime.decompose`` returns.  ``periods`` / ``powers`` / ``counts`` / ``periodic`` / ``residual`` are
    those of ``analyze``.  ``track_periods`` lists the T tracks, each a tuple of periods; ``tracks[t]`` (T, L) is the
    overlap-added, window-normalised sum of the bases whose period is in ``track_periods[t]``; ``other`` (L,) is the
    same sum over every used basis that is in no track (period-0 rows included) -- computed as a track of its own, not
    as a difference; ``activity[t, f]`` (T, W) is the sum of the ``powers`` of the track's bases in frame f."""

    periods: np.ndarray
    powers: np.ndarray
    periodic: np.ndarray
    residual: np.ndarray
    track_periods: list
    tracks: np.ndarray
    other: np.ndarray
    activity: np.ndarray
    counts: Optional[np.ndarray] = None


class ShortTimeRamanujan(NamedTuple):
    """What ``ShortTime.decompose_ramanujan`` returns: the fields of ``ShortTimeTracks`` (``periods`` / ``powers`` (W, K)
    are the blocks' periods and the mean square of each block's waveform over its period, zeros behind ``counts``), and
    ``norms`` (W, q_hi + 1), the Ramanujan norms of every frame -- the time-period map of the recording; ``over`` (W),
    the candidates of each frame before the cap (``over > counts`` marks a capped frame); ``frame_status`` (W) int8:
    0 fitted on the device, 1 fitted on the host, 2 nothing selected (a silent frame, all norms under the threshold, a
    NaN frame under ``reference="frame"``), 3 no fit exists.  Frames of status 2 and 3 contribute nothing."""

    periods: np.ndarray
    powers: np.ndarray
    periodic: np.ndarray
    residual: np.ndarray
    track_periods: list
    tracks: np.ndarray
    other: np.ndarray
    activity: np.ndarray
    counts: Optional[np.ndarray] = None
    norms: Optional[np.ndarray] = None
    over: Optional[np.ndarray] = None
    frame_status: Optional[np.ndarray] = None


class ShortTimeMap(NamedTuple):
    """What ``ShortTime.period_map`` returns: ``values[f, j]`` (W, P) float64 is the `kind` norm of frame f at period
    ``periods[j]`` (P,) int32 -- numpy arrays for a numpy signal, tensors on the engine's device for a tensor signal."""

    periods: object
    values: object
    kind: str


class ShortTimeContour(NamedTuple):
    """What ``ShortTime.contour`` returns: ``periods[f]`` (W,) int32 is the period of frame f on the best path through the
    time-period map, ``salience[f]`` (W,) float64 the map's value there, ``score`` the path's summed salience minus its
    jump penalties, ``map`` the ShortTimeMap when it was asked for."""

    periods: np.ndarray
    salience: np.ndarray
    score: float
    map: Optional[ShortTimeMap] = None


class ShortTimeContours(NamedTuple):
    """What ``ShortTime.contours`` returns: column k of ``periods`` (W, K) int32 is the period track of round k -- the
    best path through the map of what the tracks before it left of every frame -- and 0 where `floor` silenced it;
    ``salience`` (W, K) float64 is that round's map along its path (kept where the track is silent); ``scores`` (K,)
    float64 the paths' scores; ``maps`` the K ShortTimeMap when they were asked for, map k as round k's path saw it."""

    periods: np.ndarray
    salience: np.ndarray
    scores: np.ndarray
    maps: Optional[tuple] = None


class ShortTimeFollow(NamedTuple):
    """What ``ShortTime.follow`` returns: ``periods`` (W, T) int32 as given (column t is track t, an entry below 1 a
    silent frame); ``powers`` (W, T) float64, the drop of the frame's residual norm when column t's period was peeled,
    over the frame's norm, 0.0 where silent; ``tracks`` (T, L) the overlap-added, window-normalised waveform of every
    track; ``periodic`` (L,) the same sum over all blocks, a routed row of its own and not a sum of tracks;
    ``residual = float64(signal) - periodic``.  numpy arrays for a numpy signal, tensors for a tensor signal."""

    periods: object
    powers: object
    tracks: object
    periodic: object
    residual: object


_MAX_ROWS = 64  # rows per frame a 64-bit routing mask can name
# period_map's kinds; the sweep mode of the two that ph_sweep computes
_MAP_KINDS = {"norm": _ffi.PH_SWEEP_NORM, "gamma": _ffi.PH_SWEEP_NORM_GAMMA, "orth": None, "ramanujan": None}
_RAM_MAX_PERIOD = 30030  # ph_ramanujan_norms' record format
_PATH_MAX_BAND, _PATH_MAX_PERIODS = 64, 8192  # ph_period_path's limits


class _Recording:
    """A recording on its way through a pipeline (``ShortTime._upload``): uploaded once, framed block by block."""

    def __init__(self, x, W, eng, xd, win, tdt):
        self.x, self.L, self.W = x, x.shape[0], W  # the host signal (float64 or float32), its samples, its frames
        self.eng, self.xd, self.win, self.tdt = eng, xd, win, tdt  # engine, device signal and window (or None), frame dtype

    @cached_property
    def x64(self):
        """The float64 copy of the signal (residual = x64 - periodic), made when first asked for: L samples on the
        host, which a pipeline reads once the device has work to do."""
        return self.x.astype(np.float64)


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
        if _is_torch(signal):
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
        if self.window is None or not _is_torch(like):
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

    def analyze(self, signal, method="m_best", block_frames=None, **kwargs):
        """Frame `signal`, run ``Periods.<method>`` (its keyword arguments in **kwargs) over the frames and overlap-add
        the bases: -> ShortTimeResult.  One upload of the signal, one download of the results; status words raise what
        the ``Periods`` method raises, with the first offending frame named.

        `block_frames`: None -- all W frames and their ``(W, K, N)`` bases on the device at once -- or an int B >= 1:
        the signal goes up once, the frames are analysed B at a time and every block's bases are added into one running
        sum of L doubles (``PeriodEngine.overlap_add_block``), normalised once at the end (``overlap_add_finish``), so
        the device holds one block's frames and bases, whatever the length of the recording.  The result is field for
        field, bit for bit that of ``block_frames=None``; so is the exception, which is raised once every block has
        run."""
        B = self._block_frames(block_frames)
        self._known(method)
        return self._pipeline(signal, method, B, kwargs)

    def decompose(self, signal, method="m_best", tracks=None, max_tracks=8, block_frames=None, **kwargs):
        """``analyze``, and the periodic part split by period: -> ShortTimeTracks.  `tracks`: None -- the `max_tracks`
        strongest periods of the recording, one track each (``rank_periods``) -- or a list whose entries are a period or
        an iterable of periods, e.g. ``[12, (17, 34)]``.  The pipeline is that of ``analyze`` (same methods, keyword
        arguments and exceptions); afterwards only the per-frame periods / powers / counts come down, the routing masks
        (``track_masks``) go up, and one routed overlap-add (``PeriodEngine.overlap_add_tracks``) folds the bases onto
        T + 1 rows: the tracks and ``other``.  The ``(W, K, N)`` bases never leave the device.  K <= 64 bases per
        frame: `num` > 64 raises ValueError before anything is launched; for small_to_large K is known only once the
        method has run, so there the check comes after the method's kernels and before the two overlap-adds.

        `block_frames`: as in ``analyze`` -- B frames at a time, the bases of a block added into two running sums, (L)
        and (T + 1, L), under the block's masks; the same result and exceptions, bit for bit.  With `tracks` given the
        analysis runs once.  With ``tracks=None`` the ranking needs every frame before the first block can be routed,
        so the analysis runs TWICE: once for the per-frame results and ``periodic``, then, after ``rank_periods``, again
        block by block to fold the bases onto the tracks."""
        self._known(method)
        B = self._block_frames(block_frames)
        wanted, max_tracks, _, _ = self._track_args(tracks, max_tracks, tracks_first=True)
        if method != "small_to_large":
            self._routable(int(kwargs.get("num", 5)), "num=")
        return self._pipeline(signal, method, B, kwargs, wanted, max_tracks)

    @staticmethod
    def _known(method):
        if method not in _METHODS:
            raise ValueError(f"method must be one of {_METHODS}")

    @staticmethod
    def _routable(rows, named=""):
        """decompose's limit on the rows of a frame: refused as ``num=...`` before the launch, as counted after it."""
        if rows > _MAX_ROWS:
            raise ValueError(f"{named}{rows} bases per frame: decompose routes at most {_MAX_ROWS}")

    def _pipeline(self, signal, method, B, kwargs, wanted=None, max_tracks=None):
        """``analyze`` (`max_tracks` None) and ``decompose`` (`wanted`: the named tracks, or None for the `max_tracks`
        strongest), over blocks of `B` frames; None is one block of all W frames.  The signal goes up once.  Per block:
        ``frames`` on the slice of the device signal that starts at the block's first sample, the engine method, its
        periods / powers / counts / status down (``_host_results``), and the block's bases folded.  Then the status
        check and, for ``decompose``, the limit on the rows per frame.

        What differs is the fold.  The one block of an unblocked call stays alive past those checks and is folded by
        ``overlap_add_tracks`` and then ``overlap_add``, under masks from its own host results: ranked tracks need no
        second run.  A block of a blocked call is added into the running sums -- (L) first, then (T + 1, L) under the
        block's masks -- and released before the next block is made; ``overlap_add_finish`` ends each sum, in place.
        There, ranked tracks need every frame before the first block can be routed: a second run of the method folds
        the bases onto the tracks, and nothing else."""
        import torch

        N, hop, route = self.frame_length, self.hop, max_tracks is not None
        # (an unblocked call has its signal up and framed before the method's keyword arguments are read, a blocked
        # call after: which refusal a caller sees first, and after which launches, is part of the surface)
        rec = self._upload(signal) if B is None else None
        whole = self._frames(rec, 0, rec.W) if B is None else None
        num, run = self._method(method, kwargs)
        rec = rec or self._upload(signal)
        L, W, eng, win, dev = rec.L, rec.W, rec.eng, rec.win, rec.xd.device
        if num == 0:  # the reference's loops do not run: empty per-frame arrays, nothing periodic
            wanted = (wanted or []) if route else None
            return self._assemble(rec, np.zeros((W, 0), np.uint32), np.zeros((W, 0)), None, np.zeros(L), wanted,
                                  np.zeros((len(wanted or []) + 1, L)))

        def running_sum(rows):
            return torch.zeros((rows, L), dtype=torch.float64, device=dev)

        def finish(total):  # the end of a blocked run's sum, in place, and the result on the host
            return eng.overlap_add_finish(total, N, hop, W, win, win, True, out=total).cpu().numpy()

        def up(masks):  # (T + 1) * Wb words
            return torch.as_tensor(masks.view(np.int64), device=dev)

        def rows(parts):  # (W, cap): small_to_large's blocks differ in cap = max(16, largest count)
            if len(parts) == 1:
                return parts[0]
            cap = max(p.shape[1] for p in parts)
            return np.concatenate([np.pad(p, ((0, 0), (0, cap - p.shape[1]))) for p in parts])

        def run_blocks(acc, routed, masks_of):
            """One run of the method over the recording.  Blocked, every block is added into `acc` (1, L) and, under
            masks_of(f0, periods, counts) -> (T + 1, Wb) uint64 from its host results, into `routed` (T + 1, L), each
            where given; unblocked, the block is kept.  -> the recording's host periods, powers and counts, the masks
            (T + 1, W) or None, the kept (bases, counts) or None."""
            blocks = [(0, whole)] if B is None else (
                (f0, self._frames(rec, f0, min(B, W - f0))) for f0 in range(0, W, B))
            got, sts, msks, kmax, kept = [], [], [], 0, None
            for f0, fr in blocks:
                per, pw, bases, st, counts = run(eng, fr)
                rec.x64  # (the host's copy of L samples, made here the first time: the device is at work on the block)
                kmax = max(kmax, int(bases.shape[1]))
                if acc is not None:
                    eng.overlap_add_block(bases, hop, L, f0, acc, counts, None, win)
                sts.append(st.cpu().numpy())
                got.append(self._host_results(per, pw, counts))
                if masks_of is not None and bases.shape[1] <= _MAX_ROWS:  # (more rows: refused below, after every block)
                    msks.append(masks_of(f0, got[-1][0], got[-1][2]))
                    eng.overlap_add_block(bases, hop, L, f0, routed, counts, up(msks[-1]), win)
                if B is None:
                    kept = bases, counts
                del fr, per, pw, bases, st, counts  # the block's frames and bases go before the next block's come
            self._raise_status(np.concatenate(sts), method)
            if route:
                self._routable(kmax)
            pers, pws, cnts = zip(*got)
            return (rows(pers), rows(pws), None if cnts[0] is None else np.concatenate(cnts),
                    np.concatenate(msks, axis=1) if msks else None, kept)

        acc = routed = by_block = None
        if B is not None:
            acc = running_sum(1)
            if wanted is not None:  # named tracks: every block is routed as it comes
                routed, by_block = running_sum(len(wanted) + 1), lambda f0, p, c: self.track_masks(p, c, wanted)
        per, pw, counts, masks, kept = run_blocks(acc, routed, by_block)
        if route and masks is None:  # every other decompose: routed once the whole recording's results are down
            wanted = self._ranked(per, pw, counts, wanted, max_tracks)
            masks = self.track_masks(per, counts, wanted)
            if B is None:
                routed = eng.overlap_add_tracks(kept[0], up(masks), hop, L, kept[1], win, win, True)
            else:
                routed = running_sum(len(wanted) + 1)
                run_blocks(None, routed, lambda f0, p, c: masks[:, f0 : f0 + p.shape[0]])
        if B is None:
            periodic = eng.overlap_add(kept[0], hop, L, kept[1], win, win, True).cpu().numpy()
            routed = routed.cpu().numpy() if route else None
        else:
            periodic, routed = finish(acc)[0], finish(routed) if route else None
        return self._assemble(rec, per, pw, counts, periodic, wanted, routed, masks)

    def _assemble(self, rec, per, pw, counts, periodic, wanted=None, routed=None, masks=None):
        """The result of every pipeline from its host arrays: ShortTimeResult, or with `wanted` (T tracks) ShortTimeTracks
        from `routed`, whose rows T and up are ``other`` and whatever else the pipeline routed, and its `masks`."""
        if wanted is None:
            return ShortTimeResult(per, pw, periodic, rec.x64 - periodic, counts)
        T = len(wanted)
        return ShortTimeTracks(per, pw, periodic, rec.x64 - periodic, wanted, routed[:T], routed[T],
                               self._activity(masks, pw, T), counts)

    def _ranked(self, per, pw, counts, wanted, max_tracks):
        """The named tracks, or with none named one track for each of the `max_tracks` strongest periods."""
        return [(p,) for p in self.rank_periods(per, pw, counts, max_tracks)] if wanted is None else wanted

    @staticmethod
    def _host_results(per, pw, counts):
        """The per-frame device results as analyze returns them: (W, num) uint32 periods, or for small_to_large int32
        periods and powers with zeros behind counts[f]."""
        per, pw = per.cpu().numpy(), pw.cpu().numpy()
        if counts is None:
            return per.view(np.uint32), pw, None
        counts = counts.cpu().numpy()
        used = np.arange(per.shape[1])[None, :] < counts[:, None]
        return np.where(used, per, 0), np.where(used, pw, 0.0), counts

    def _upload(self, signal):
        """The one upload of L samples, no frames yet: -> _Recording."""
        import torch  # lazily, as QOPeriods.solve_quadratic does

        x = self._signal(signal)
        if _is_torch(x):
            x = x.detach().cpu().numpy()
        W = self.frame_count(x.shape[0])
        eng = default_engine()
        dev = torch.device("cuda", eng.device)
        return _Recording(x, W, eng, torch.as_tensor(x, device=dev),  # the one upload: L samples
                          None if self.window is None else torch.as_tensor(self.window, device=dev),
                          torch.float64 if self.dtype == np.float64 else torch.float32)

    def _frames(self, rec, f0, count):
        """The frames f0 .. f0 + count - 1 of an uploaded recording, on the device."""
        return rec.eng.frames(rec.xd[f0 * self.hop :], self.frame_length, self.hop, count, rec.win, rec.tdt)

    @staticmethod
    def _activity(masks, powers, T):
        """activity[t, f]: the powers of the rows of frame f that masks[t, f] names, added in ascending row order (the
        order of the kernels)."""
        activity = np.zeros((T, powers.shape[0]))
        for k in range(powers.shape[1]):
            bit = (masks[:T] >> np.uint64(k)) & np.uint64(1)
            activity += np.where(bit != 0, powers[None, :, k], 0.0)
        return activity

    def _method(self, method, kwargs):
        """The engine call behind `method`, its keyword arguments taken out of `kwargs` with the defaults, warnings and
        TypeError of ``Periods.<method>``: -> (num, run) with run(engine, frames) -> (periods, powers, bases, status,
        counts) on the device, counts None for every method but small_to_large (whose num is 1: it always runs)."""
        N = self.frame_length
        trunc, orth = self._trunc_to_integer_multiple, self._orthogonalize
        if method in ("m_best", "m_best_gamma"):
            if orth:
                warn("`Orthogonalize = True` has no effect in M-best.")
            num = int(kwargs.pop("num", 5))
            max_length = kwargs.pop("max_length", None)
            min_length = kwargs.pop("min_length", 2)
            self._no_more(kwargs, method)
            if max_length is None:
                max_length = math.floor(N / 3)
            gamma = method == "m_best_gamma"
            return num, lambda eng, fr: eng.m_best(fr, num, max_length, min_length, gamma, trunc, orth) + (None,)
        if method == "best_correlation":
            num = int(kwargs.pop("num", 5))
            max_length = kwargs.pop("max_length", None)
            ratio = kwargs.pop("ratio", 0.01)
            self._no_more(kwargs, method)
            if max_length is None:
                max_length = math.floor(N / 3)
            return num, lambda eng, fr: eng.best_correlation(fr, num, max_length, ratio, trunc, orth) + (None,)
        if method == "best_frequency":
            num = int(kwargs.pop("num", 5))
            win_size = kwargs.pop("win_size", None)
            self._no_more(kwargs, method)
            if win_size is None:
                win_size = N
            elif win_size < N:
                warn("win_size is smaller than the input signal length. It will be truncated and information will be lost.")
            return num, lambda eng, fr: eng.best_frequency(fr, win_size, num, trunc, orth) + (None,)
        thresh = kwargs.pop("thresh", 0.1)
        n_periods = kwargs.pop("n_periods", None)
        self._no_more(kwargs, method)
        if n_periods is None:
            n_periods = math.floor(N / 2)

        def small_to_large(eng, fr):
            counts, per, pw, bases, st = eng.small_to_large(fr, thresh, n_periods, trunc, orth)
            return per, pw, bases, st, counts

        return 1, small_to_large

    @staticmethod
    def _block_frames(block_frames):
        """None, or the frames per block as an int >= 1 (ValueError for a bool, a float, 0 or a negative value)."""
        if block_frames is None:
            return None
        if isinstance(block_frames, bool) or not isinstance(block_frames, (int, np.integer)) or block_frames < 1:
            raise ValueError(f"block_frames={block_frames!r} must be an int >= 1")
        return int(block_frames)

    # ------------------------------------------------------------------ the time-period map and a track through it
    def _map_args(self, kind, min_length, max_length):
        """The refusals of ``period_map`` that need no engine, in the order the docstring lists them: -> (lo, hi)."""
        if kind not in _MAP_KINDS:
            raise ValueError(f"kind must be one of {tuple(_MAP_KINDS)}")
        lo = int(min_length)
        if lo < 1:
            raise ValueError("min_length must be >= 1")
        hi = self.frame_length // 3 if max_length is None else int(max_length)
        if hi < lo:
            raise ValueError(f"max_length={hi} must be >= min_length={lo}")
        if kind == "ramanujan" and hi >= _RAM_MAX_PERIOD:
            raise ValueError(f"max_length={hi}: the Ramanujan norms take periods below {_RAM_MAX_PERIOD}")
        if kind in ("orth", "ramanujan") and (self._trunc_to_integer_multiple or self._orthogonalize):
            raise ValueError(f"kind={kind!r} has no projection that trunc_to_integer_multiple / orthogonalize could apply to")
        return lo, hi

    def _map_plan(self, eng, kind, lo, hi, dtype=None):
        """The kind's kernel asked whether it takes frames of this length and this range (the plan query of its entry
        point: its own refusals, raised as ValueError, and nothing launched).  `dtype`: the frames' (None: ``dtype``)."""
        trunc, orth = self._trunc_to_integer_multiple, self._orthogonalize
        dtype = self.dtype if dtype is None else dtype
        if kind in ("norm", "gamma"):
            eng.plan_info("sweep", self.frame_length, (lo, hi, _MAP_KINDS[kind]), dtype, trunc, orth)
        elif kind == "orth":
            eng.plan_info("orth_powers", self.frame_length, (hi + 1,), dtype)
        else:
            eng.plan_info("ramanujan", self.frame_length, (lo, hi), dtype)

    def _map_rows(self, eng, fr, kind, lo, hi):
        """(Wb, P): the columns lo .. hi of the kind's table for the frames `fr`, a view where the table is wider."""
        if kind in ("norm", "gamma"):
            return eng.sweep(fr, lo, hi, _MAP_KINDS[kind], self._trunc_to_integer_multiple, self._orthogonalize)
        if kind == "orth":
            return eng.orth_powers(fr, hi + 1, normalize=True)[:, lo : hi + 1]
        return eng.ramanujan_norms(fr, lo, hi)[:, lo : hi + 1]

    @staticmethod
    def _device_signal(x, eng):
        """The signal of ``_signal`` on the engine's device: -> (tensor, whether it came as one).  A numpy signal goes
        up here, once; a tensor on the engine's device is used where it lies."""
        import torch

        if not _is_torch(x):
            return torch.as_tensor(x, device=torch.device("cuda", eng.device)), False  # the one upload: L samples
        if not x.is_cuda or x.device.index != eng.device:
            raise ValueError(f"a tensor signal must live on cuda:{eng.device} (or pass a numpy array)")
        xd = x.detach()
        if xd.dtype not in (torch.float64, torch.float32):
            xd = xd.to(torch.float64)
        return xd.contiguous(), True

    def _map(self, signal, kind, lo, hi, B):
        """The (W, P) map of `signal` on the device and whether the signal came as a device tensor.  The signal goes up
        once (a tensor on the engine's device is used where it lies); the frames are cut on the device, all at once or
        `B` at a time, and every block's rows of the kind's table are written into one (W, P) tensor."""
        import torch

        x = self._signal(signal)
        eng = default_engine()
        self._map_plan(eng, kind, lo, hi)
        dev = torch.device("cuda", eng.device)
        xd, on_device = self._device_signal(x, eng)
        W = self.frame_count(xd.shape[0])
        win = None if self.window is None else torch.as_tensor(self.window, device=dev)
        rec = _Recording(xd, W, eng, xd, win, torch.float64 if self.dtype == np.float64 else torch.float32)
        if B is None or B >= W:
            return self._map_rows(eng, self._frames(rec, 0, W), kind, lo, hi), on_device
        values = torch.empty((W, hi - lo + 1), dtype=torch.float64, device=dev)
        for f0 in range(0, W, B):
            values[f0 : f0 + B] = self._map_rows(eng, self._frames(rec, f0, min(B, W - f0)), kind, lo, hi)
        return values, on_device

    def period_map(self, signal, kind="gamma", min_length=2, max_length=None, block_frames=None):
        """The time-period map of a recording: the frames x periods table of a periodic norm, the periodicity analogue
        of a spectrogram.  -> ShortTimeMap(periods (P,), values (W, P) float64, kind); column j is period
        ``min_length + j``, `max_length` defaults to ``frame_length // 3``.

        `kind`: "norm" -- ``periodic_norm(project(frame, p))``, "gamma" -- the same divided by p (both ``PeriodEngine.sweep``,
        with the constructor's trunc / orthogonalize flags), "orth" -- the normalised orthogonal period powers
        (``orth_powers``), "ramanujan" -- the Ramanujan norms (``ramanujan_norms``).

        The signal goes up once; the frames are cut on the device (window applied) all at once or `block_frames` at a
        time, and each block's rows are written into one (W, P) device tensor: every partition gives the same map, bit
        for bit.  A numpy signal returns numpy arrays; a tensor on the engine's device returns tensors and downloads
        nothing.  ValueError before any launch: an unknown `kind`, ``min_length < 1``, ``max_length < min_length``, a
        range the kind's kernel does not take, or either flag together with "orth" / "ramanujan"."""
        B = self._block_frames(block_frames)
        lo, hi = self._map_args(kind, min_length, max_length)
        values, on_device = self._map(signal, kind, lo, hi, B)
        return self._map_result(values, kind, lo, hi, on_device)

    @staticmethod
    def _map_result(values, kind, lo, hi, on_device):
        if on_device:
            import torch

            return ShortTimeMap(torch.arange(lo, hi + 1, dtype=torch.int32, device=values.device), values, kind)
        return ShortTimeMap(np.arange(lo, hi + 1, dtype=np.int32), values.cpu().numpy(), kind)

    def contour(self, signal, kind="gamma", band=8, jump=0.0, min_length=2, max_length=None, block_frames=None,
                return_map=False):
        """The period track of a recording: the path through its time-period map (``period_map``, same arguments) that
        maximises the summed map value minus ``jump * |step|`` over the paths that move at most `band` periods per frame
        (``PeriodEngine.period_path``: one launch on the map where it lies on the device).  Frame-wise maxima jump to
        multiples and near-multiples of the true period; the path does not, because a jump costs more than it gains.
        -> ShortTimeContour(periods (W,) int32 = min_length + path, salience (W,) float64 = the map along the path,
        score, map).  Only W integers, W doubles and the score come down; with ``return_map=True`` `map` is the
        ShortTimeMap (numpy for a numpy signal, tensors for a tensor signal), otherwise None.

        ValueError before any launch for what ``period_map`` refuses, `band` outside 0 .. 64, a negative or non-finite
        `jump`, or more than 8192 periods; after the launch when no path exists, naming the first frame whose map row
        has no finite value (a NaN sample in a frame makes its whole row NaN)."""
        B = self._block_frames(block_frames)
        lo, hi = self._map_args(kind, min_length, max_length)
        band, jump = self._path_args(band, jump, lo, hi)
        values, on_device = self._map(signal, kind, lo, hi, B)
        path, sal, score, status = default_engine().period_path(values, band, jump)
        if int(status.item()) != _ffi.PH_ST_OK:
            self._no_path("contour", values, band)
        periods = (path + lo).cpu().numpy().astype(np.int32, copy=False)
        return ShortTimeContour(periods, sal.cpu().numpy(), float(score.item()),
                                self._map_result(values, kind, lo, hi, on_device) if return_map else None)

    @staticmethod
    def _path_args(band, jump, lo, hi):
        """The refusals of the path through a map of the periods lo .. hi that need no engine: -> (band, jump)."""
        if isinstance(band, bool) or not isinstance(band, (int, np.integer)) or not 0 <= int(band) <= _PATH_MAX_BAND:
            raise ValueError(f"band={band!r} must be an int in 0 .. {_PATH_MAX_BAND}")
        if isinstance(jump, bool) or not isinstance(jump, (int, float, np.integer, np.floating)) or not (
                jump >= 0 and math.isfinite(jump)):
            raise ValueError(f"jump={jump!r} must be finite and >= 0")
        if hi - lo + 1 > _PATH_MAX_PERIODS:
            raise ValueError(f"{hi - lo + 1} periods: the path kernel takes at most {_PATH_MAX_PERIODS}")
        return int(band), float(jump)

    @staticmethod
    def _no_path(what, values, band):
        """The ValueError of a map without a path, naming the first frame whose row has no finite value."""
        import torch

        dead = (~torch.isfinite(values)).all(dim=1).cpu().numpy()
        if dead.any():
            raise ValueError(f"{what}: no path exists, the map row of frame {_first(dead)} has no finite value")
        raise ValueError(f"{what}: no path of band {band} connects the finite values of the map")

    def contours(self, signal, count, kind="gamma", band=8, jump=0.0, min_length=2, max_length=None, floor=None,
                 guard=None, block_frames=None, return_maps=False):
        """`count` period tracks of a recording with several sources, by peeling: track k is the best path
        (``contour``'s, same `kind`, `band`, `jump`, `min_length`, `max_length`) through the time-period map of what the
        tracks 0 .. k-1 left of every frame.  The second-best path through ONE map follows a multiple of the first
        track, not the second source; the map of the residual does not hold the first source any more.
        -> ShortTimeContours(periods (W, count) int32, salience (W, count) float64, scores (count,) float64, maps).

        Every round k = 0 .. count-1, the first included, is four steps on device tensors:
          1. residual frames: for every block of `block_frames` frames (None: all W), ``PeriodEngine.follow_residual``
             of the recording with the live entries (>= 1) of the columns 0 .. k-1 of `periods`, packed to the front
             (``pack_tracks``) and peeled in column order -- the subtraction ``follow`` performs, so the tracks found
             are tracks of exactly what ``follow`` then extracts.  The constructor's `trunc_to_integer_multiple`,
             `window` and `dtype` are honoured as in ``follow``;
          2. map: the kind's kernel on those float64 frames, the columns `min_length` .. `max_length`, into one (W, P)
             tensor.  With ``dtype=float32`` the frames are rounded to float32 once, as everywhere, but they come out
             of step 1 widened to float64 and every round runs the kind's float64 kernel on them (``contour`` runs
             the float32 one);
          3. guard: with ``guard=g`` (an int >= 0) the cells within g columns of an earlier track's live period in that
             frame are set to -inf, which the path kernel treats as forbidden; None forbids nothing;
          4. path: one ``PeriodEngine.period_path`` launch.  Column k is ``min_length + path`` and ``salience[:, k]``
             the map along it.  With `floor` set, the frames whose salience is not > floor get period 0: the track is
             silent there and later rounds do not peel it there; ``salience`` keeps the map's value.
        Per round only the status scalar comes down (and the row count inside ``pack_tracks``); at the end the (W, count)
        integers and doubles and the scores.  ``return_maps=True`` returns the maps as a tuple of ShortTimeMap, map k as
        the path of round k saw it, guard included: numpy for a numpy signal, tensors for a tensor signal.

        For float64 frames ``contours(x, 1, ...)`` is ``contour(x, ...)`` bit for bit, and ``follow`` takes the result
        wherever it takes a ShortTimeContour, its columns in order.

        ValueError before any launch for what ``contour`` refuses, `count` not an int in 1 .. 64, `guard` neither None
        nor an int >= 0, a `floor` that is not a finite number, or a ``ShortTime`` built with ``orthogonalize=True``
        (as in ``follow``: the whole projection is peeled); after a round's launch when that round has no path, with
        the round named."""
        if self._orthogonalize:
            raise ValueError("contours peels the whole projection, sub-periods included, as follow does: build the "
                             "ShortTime with orthogonalize=False")
        B = self._block_frames(block_frames)
        lo, hi = self._map_args(kind, min_length, max_length)
        band, jump = self._path_args(band, jump, lo, hi)
        if isinstance(count, bool) or not isinstance(count, (int, np.integer)) or not 1 <= int(count) <= _MAX_ROWS:
            raise ValueError(f"count={count!r} must be an int in 1 .. {_MAX_ROWS}")
        if guard is not None and (isinstance(guard, bool) or not isinstance(guard, (int, np.integer)) or guard < 0):
            raise ValueError(f"guard={guard!r} must be None or an int >= 0")
        if floor is not None and (isinstance(floor, bool) or not isinstance(floor, (int, float, np.integer, np.floating))
                                  or not math.isfinite(floor)):
            raise ValueError(f"floor={floor!r} must be None or a finite number")
        K = int(count)

        import torch

        x = self._signal(signal)
        eng = default_engine()
        self._map_plan(eng, kind, lo, hi, np.float64)
        dev = torch.device("cuda", eng.device)
        xd, on_device = self._device_signal(x, eng)
        N, hop, W, P = self.frame_length, self.hop, self.frame_count(xd.shape[0]), hi - lo + 1
        B = W if B is None or B >= W else B
        win = None if self.window is None else torch.as_tensor(self.window, device=dev)
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        periods = torch.zeros((W, K), dtype=torch.int32, device=dev)
        salience = torch.empty((W, K), dtype=torch.float64, device=dev)
        scores = torch.empty((K,), dtype=torch.float64, device=dev)
        cols = torch.arange(lo, hi + 1, dtype=torch.int32, device=dev)
        maps = []
        for k in range(K):
            packed, counts = self.pack_tracks(periods[:, :k])[:2] if k else (None, None)

            def rows(f0, Wb):
                fr = eng.follow_residual(xd, N, hop, f0, Wb, packed[f0 : f0 + Wb] if k else None,
                                         counts[f0 : f0 + Wb] if k else None, win, tdt, self._trunc_to_integer_multiple)
                return self._map_rows(eng, fr, kind, lo, hi)

            if B == W:
                values = rows(0, W)
            else:
                values = torch.empty((W, P), dtype=torch.float64, device=dev)
                for f0 in range(0, W, B):
                    values[f0 : f0 + B] = rows(f0, min(B, W - f0))
            if guard is not None:
                for t in range(k):
                    pt = periods[:, t : t + 1]
                    # (no two periods of the range lie more than hi apart: a wider guard is that one)
                    values.masked_fill_((pt >= 1) & ((cols[None, :] - pt).abs() <= min(int(guard), hi)), -math.inf)
            path, sal, score, status = eng.period_path(values, band, jump)
            if int(status.item()) != _ffi.PH_ST_OK:
                self._no_path(f"contours: round {k}", values, band)
            col = path + lo
            periods[:, k] = col if floor is None else torch.where(sal > float(floor), col, torch.zeros_like(col))
            salience[:, k], scores[k] = sal, score
            if return_maps:
                maps.append(self._map_result(values, kind, lo, hi, on_device))
        return ShortTimeContours(periods.cpu().numpy(), salience.cpu().numpy(), scores.cpu().numpy(),
                                 tuple(maps) if return_maps else None)

    def follow(self, signal, periods):
        """The sound of a recording along a period track: from every frame the projection onto the period the track
        names for that frame is taken (``Periods.project``, whole, sub-periods included) and the per-frame waveforms are
        overlap-added -> ShortTimeFollow(periods, powers, tracks, periodic, residual).

        `periods`: a ShortTimeContour, a ShortTimeContours (its columns in order), a (W,) or (W, T) integer array, an integer tensor on the engine's device, or a
        list of any of these, whose columns are stacked in list order.  Column t is track t; in a frame the columns are
        peeled left to right, each from what the ones before it left.  An entry below 1 means the track is silent in
        that frame, e.g. ``np.where(c.salience > s, c.periods, 0)``.

        The signal goes up once.  Each frame's live periods are packed to the front (``pack_tracks``), one ``ph_follow``
        launch cuts the frames inside the kernel and leaves one period per block, and one routed overlap-add
        (``PeriodEngine.overlap_add_periodic``, the window as analysis and synthesis window, normalised) tiles them onto
        T + 1 rows: the tracks and ``periodic``.  Nothing of W x frame_length samples exists, so there is nothing to
        block.  `trunc_to_integer_multiple` and `dtype` are honoured.  numpy in gives numpy out; a tensor signal gives
        tensors, and only the two scalars of the checks below come down.

        ValueError before anything is launched: a row count other than ``frame_count(L)``, T outside 1 .. 64, a period
        above ``frame_length``, a non-integer dtype, or a ``ShortTime`` built with ``orthogonalize=True``."""
        if self._orthogonalize:
            raise ValueError("follow takes the whole projection, sub-periods included: build the ShortTime with "
                             "orthogonalize=False")
        x = self._signal(signal)
        L, N = int(x.shape[0]), self.frame_length
        W = self.frame_count(L)
        per = self._follow_periods(periods, W)
        T = int(per.shape[1])
        packed, counts, masks, slot, live = self.pack_tracks(per)
        ccap = max(1, int(packed.sum(1).max()))

        import torch

        eng = default_engine()
        dev = torch.device("cuda", eng.device)
        xd, on_device = self._device_signal(x, eng)
        if _is_torch(per):
            if per.device != dev:
                raise ValueError(f"tensor periods must live on cuda:{eng.device} (or pass a numpy array)")
        else:
            per, packed, counts, slot, live = (torch.as_tensor(a, device=dev) for a in (per, packed, counts, slot, live))
            masks = torch.as_tensor(masks.view(np.int64), device=dev)
        win = None if self.window is None else torch.as_tensor(self.window, device=dev)
        tdt = torch.float64 if self.dtype == np.float64 else torch.float32
        seg, pw, _ = eng.follow(xd, N, self.hop, W, packed, counts, ccap, win, tdt, self._trunc_to_integer_multiple)
        rows = eng.overlap_add_periodic(seg, packed, counts, masks, N, self.hop, L, win, win, True)
        powers = torch.where(live, torch.gather(pw, 1, slot.clamp(min=0)), torch.zeros((), dtype=torch.float64, device=dev))
        if on_device:
            return ShortTimeFollow(per, powers, rows[:T], rows[T], xd.to(torch.float64) - rows[T])
        rows = rows.cpu().numpy()
        return ShortTimeFollow(per.cpu().numpy(), powers.cpu().numpy(), rows[:T], rows[T], x.astype(np.float64) - rows[T])

    def _follow_periods(self, periods, W):
        """`periods` of ``follow`` as one (W, T) int32 array -- a tensor if any part is one -- or ValueError."""
        cols = []
        for it in (periods if isinstance(periods, list) else [periods]):
            if isinstance(it, (ShortTimeContour, ShortTimeContours)):
                it = it.periods
            if _is_torch(it):
                if it.dtype.is_floating_point or it.dtype.is_complex or str(it.dtype) == "torch.bool":
                    raise ValueError(f"periods must be integers, not {it.dtype}")
                a = it.detach()
            else:
                a = np.asarray(it)
                if a.dtype.kind not in "iu":
                    raise ValueError(f"periods must be integers, not {a.dtype}")
            if a.ndim == 1:
                a = a.reshape(-1, 1)
            if a.ndim != 2 or a.shape[0] != W:
                raise ValueError(f"periods must be (W,) or (W, T) with W = frame_count(L) = {W} rows, "
                                 f"not {tuple(a.shape)}")
            cols.append(a)
        T = sum(int(a.shape[1]) for a in cols)
        if not 1 <= T <= _MAX_ROWS:
            raise ValueError(f"T={T} tracks: follow takes 1 .. {_MAX_ROWS}")
        tensors = [a for a in cols if _is_torch(a)]
        if tensors:
            import torch

            dev = tensors[0].device
            per = torch.cat([(a if _is_torch(a) else torch.as_tensor(np.ascontiguousarray(a).astype(np.int64), device=dev))
                             .to(device=dev, dtype=torch.int64) for a in cols], 1)
        else:
            per = np.concatenate([a.astype(np.int64) if a.dtype != np.uint64 else np.minimum(a, 2**31 - 1).astype(np.int64)
                                  for a in cols], 1)
        hi = int(per.max())
        if hi > self.frame_length:
            raise ValueError(f"period {hi} is longer than a frame of {self.frame_length} samples")
        if tensors:
            return per.clamp(min=-(2**31)).to(torch.int32)
        return np.maximum(per, -(2**31)).astype(np.int32)

    @staticmethod
    def pack_tracks(periods):
        """The block layout of ``follow`` for a (W, T) integer array or tensor of per-frame periods, T <= 64: each
        frame's live entries (>= 1) packed to the front in column order.  -> (packed (W, T) int32, zeros behind the
        live ones; counts (W,) int32; masks (T + 1, W) -- np.uint64, or torch.int64 with the same bits -- bit a of
        masks[t, f] set for the block a that column t became in frame f, row T naming every block; slot (W, T) int64,
        the block of column t where it is live; live (W, T) bool).  numpy ops for an array, torch ops on the tensor's
        device for a tensor."""
        W, T = (int(v) for v in periods.shape)
        live = periods >= 1
        if _is_torch(periods):
            import torch

            slot = torch.cumsum(live.to(torch.int64), 1) - 1
            counts = live.sum(1).to(torch.int32)
            f, t = torch.nonzero(live, as_tuple=True)
            packed = torch.zeros((W, T), dtype=torch.int32, device=periods.device)
            packed[f, slot[f, t]] = periods[f, t].to(torch.int32)
            bits = torch.where(live, torch.bitwise_left_shift(torch.ones_like(slot), slot.clamp(min=0)),
                               torch.zeros_like(slot))
            masks = torch.empty((T + 1, W), dtype=torch.int64, device=periods.device)
            masks[:T] = bits.T
            masks[T] = bits.sum(1)  # (distinct bits: the sum is their union, bit 63 included -- int64 wraps)
            return packed, counts, masks, slot, live
        slot = np.cumsum(live, 1, dtype=np.int64) - 1
        counts = live.sum(1).astype(np.int32)
        f, t = np.nonzero(live)
        packed = np.zeros((W, T), dtype=np.int32)
        packed[f, slot[f, t]] = periods[f, t]
        bits = np.where(live, np.uint64(1) << np.maximum(slot, 0).astype(np.uint64), np.uint64(0))
        masks = np.empty((T + 1, W), dtype=np.uint64)
        masks[:T] = bits.T
        masks[T] = bits.sum(1, dtype=np.uint64)
        return packed, counts, masks, slot, live

    def decompose_qo(self, signal, num, thresh, min_length=2, max_length=None, update_weights=True, tracks=None,
                     max_tracks=8, max_rows=2048):
        """``QOPeriods.find_periods`` followed by ``get_periods`` on every frame, and the per-period waveforms
        overlap-added onto tracks: -> ShortTimeTracks.  Plain selection, default test function, natural basis, no
        analysis window inside the fit (the ``ShortTime`` window shapes the frames); `trunc_to_integer_multiple` is the
        constructor's flag, `update_weights` either value; ``orthogonalize=True`` raises ValueError (that loop is stepped
        from the host).  `num` in 1 .. 64 is required (a 64-bit mask routes 64 blocks), `max_length` defaults to
        ``frame_length // 3``, `tracks` / `max_tracks` are those of ``decompose``.  `max_rows` caps the dictionary rows
        (weights) per frame the device loop is given room for.

        Everything runs on device tensors: ``frames`` -> ``qo_find_periods`` (frames that end PH_ST_CAP are re-run at
        the next capacity as a gathered sub-batch and scattered back, while that capacity is feasible and <= `max_rows`)
        -> ``qo_get_periods`` (one period per block, ``(W, ccap)``) -> per-block powers -> ONE
        ``overlap_add_periodic`` launch with T + 2 mask rows: the tracks, ``other`` and all blocks (``periodic``).  L
        samples go up, (T + 2) L doubles and the per-frame periods / counts / powers come down; no ``(W, K, N)`` array
        exists anywhere.  A frame the device loop does not finish (still not PH_ST_OK, or without a block) is downloaded,
        run through the 1-D ``QOPeriods.find_periods`` and packed back into the device arrays; such frames are named in
        a warning.  A frame with sum |x| <= 1e-16 (the reference's fixed all-zero answer) has no block.
        With ``update_weights=False`` the loop fits a period again whenever it is the strongest of the running residual
        (and once more when the test function stops it); the blocks of one period are added into one before the
        extraction (``_merge_repeats``: the tiles of a sum are the sum of the tiles), so every period of a frame is
        listed once, in the order first fitted.

        Result: ``periods`` / ``powers`` (W, K) are the blocks' periods and the mean square of each block's waveform over
        its period, zeros behind ``counts`` (blocks per frame); ``activity[t, f]`` sums the powers of the track's blocks
        in ascending block order; ``residual = float64(signal) - periodic``."""
        import torch

        if self._orthogonalize:
            raise ValueError("decompose_qo: orthogonal selection is stepped from the host and not offered here")
        if isinstance(num, bool) or not isinstance(num, (int, np.integer)) or not 1 <= int(num) <= _MAX_ROWS:
            raise ValueError(f"num={num!r}: decompose_qo needs 1 <= num <= {_MAX_ROWS} blocks per frame")
        wanted, max_tracks, max_rows, _ = self._track_args(tracks, max_tracks, max_rows)
        max_length = self.frame_length // 3 if max_length is None else int(max_length)
        fit = (int(num), thresh, int(min_length), max_length, bool(update_weights))
        rec = self._upload(signal)
        fr = self._frames(rec, 0, rec.W)
        silent = (fr.to(torch.float64).abs().sum(dim=1) <= 1e-16).cpu().numpy()
        blocks, st = self._qo_fit(torch, rec.eng, fr, fit, max_rows)
        blocks = self._qo_host_route(torch, fr, silent, st, blocks, fit)
        return self._block_tracks(torch, rec, blocks, wanted, max_tracks)

    def decompose_ramanujan(self, signal, thresh=0.2, min_length=2, max_length=None, reference="recording",
                            max_periods=16, tracks=None, max_tracks=8, max_rows=2048):
        """``RamanujanPeriods.find_periods_with_weights`` followed by ``get_periods`` on every frame, and the per-period
        waveforms overlap-added onto tracks: -> ShortTimeRamanujan.  Natural basis, no analysis window inside the fit
        (the ``ShortTime`` window shapes the frames).  `max_length` defaults to ``frame_length // 3``; `tracks` /
        `max_tracks` / `max_rows` are those of ``decompose_qo``.

        Selection (``PeriodEngine.ramanujan_select``): the candidates of a frame are the periods q with
        ``norms[q] / level > thresh`` and the `max_periods` (1 .. 64) strongest of them are kept, ties to the smaller
        period.  `reference` chooses the level:
          "frame"      the reference's rule: ``|max(norms)|`` of the frame itself, so a near-silent frame selects as many
                       periods as a loud one, and a frame with a NaN norm selects nothing;
          "recording"  the largest finite row maximum of the whole recording's norms (silent and NaN frames ignored;
                       when no frame has a finite positive maximum nothing is selected anywhere);
          a positive finite float: that value.

        Everything runs on device tensors after the one upload of the signal: ``frames`` -> ``ramanujan_norms`` -> the
        level (torch, no read-back) -> ``ramanujan_select`` -> ``qo_fit`` on the lists (frames that end PH_ST_CAP are
        re-run at the next capacity as a gathered sub-batch and scattered back: 512 rows, halved until `max_rows` and the
        LDS hold them, then doubled, `max_rows` itself being the last step) -> ``qo_get_periods`` and the block powers ->
        ONE ``overlap_add_periodic`` launch with T + 2 mask rows.  L samples go up; (T + 2) L doubles, the (W, q_hi + 1)
        norms and the per-frame periods / counts / powers come down.  A frame the device fit does not finish (an
        ill-conditioned or indefinite dictionary, more rows than `max_rows`) is downloaded, run through the 1-D
        ``find_periods_with_weights`` with the frame's device list as test function and packed back into the device
        arrays; such frames are named in one warning.  A frame whose dictionary is singular on the host as well keeps
        no block.

        Result: the fields of ``ShortTimeTracks`` with ``periods`` / ``powers`` / ``counts`` as in ``decompose_qo``, and
        ``norms`` (W, q_hi + 1), ``over`` (W) -- candidates before the cap, ``over > counts`` marks a capped frame --
        and ``frame_status`` (W) int8: 0 fitted on the device, 1 fitted on the host, 2 nothing selected, 3 no fit
        exists.  Frames of status 2 and 3 contribute nothing to ``periodic``."""
        import torch

        if isinstance(thresh, bool) or not isinstance(thresh, (int, float, np.integer, np.floating)) or not thresh > 0:
            raise ValueError(f"thresh={thresh!r}: decompose_ramanujan needs thresh > 0 (period 0 would be selected)")
        if (isinstance(max_periods, bool) or not isinstance(max_periods, (int, np.integer))
                or not 1 <= int(max_periods) <= _MAX_ROWS):
            raise ValueError(f"max_periods={max_periods!r}: decompose_ramanujan needs 1 <= max_periods <= {_MAX_ROWS}")
        level = None
        if not (isinstance(reference, str) and reference in ("frame", "recording")):
            ok = not isinstance(reference, (bool, str)) and isinstance(reference, (int, float, np.integer, np.floating))
            if not ok or not (reference > 0 and math.isfinite(reference)):
                raise ValueError(f"reference={reference!r}: must be 'frame', 'recording' or a positive finite number")
            level = float(reference)
        wanted, max_tracks, max_rows, min_length = self._track_args(tracks, max_tracks, max_rows, min_length)
        q_hi = self.frame_length // 3 if max_length is None else int(max_length)
        if q_hi < 1:
            raise ValueError(f"max_length={q_hi}: decompose_ramanujan needs periods up to at least 1")
        rec = self._upload(signal)
        W, eng, dev, fr = rec.W, rec.eng, rec.xd.device, self._frames(rec, 0, rec.W)
        norms = eng.ramanujan_norms(fr, min_length, q_hi)
        if reference == "frame":
            ref = None
        elif level is not None:
            ref = torch.full((W,), level, dtype=torch.float64, device=dev)
        else:
            rmax = norms.max(dim=1).values  # (a NaN anywhere in a row makes its maximum NaN)
            rmax = torch.where(torch.isfinite(rmax), rmax, rmax.new_full((), -math.inf)).max()
            ref = torch.where(rmax > 0, rmax, rmax.new_full((), math.nan)).expand(W).contiguous()
        per, cnt, over = eng.ramanujan_select(norms, float(thresh), ref, int(max_periods))
        keeps, wts, st = self._ram_fit(torch, eng, fr, per, cnt, q_hi, max_rows)
        cnt_h = cnt.cpu().numpy()
        blocks, status = self._ram_host_route(torch, fr, (per, keeps, cnt, wts), cnt_h, st, min_length, q_hi)
        tail = self._block_tracks(torch, rec, blocks, wanted, max_tracks)
        return ShortTimeRamanujan(*tail, norms.cpu().numpy(), over.cpu().numpy(), status)

    @staticmethod
    def _track_args(tracks, max_tracks, max_rows=1, min_length=1, tracks_first=False):
        """The arguments the decompose methods share, checked once: -> (track list or None, max_tracks, max_rows,
        min_length), the last three as ints.  Which refusal comes first is part of each method's surface:
        ``decompose`` reads `tracks` first (`tracks_first`), the block pipelines last."""
        wanted = ShortTime._track_list(tracks) if tracks_first and tracks is not None else None
        max_rows, max_tracks, min_length = int(max_rows), int(max_tracks), int(min_length)
        if max_rows < 1:
            raise ValueError("max_rows must be >= 1")
        if max_tracks < 0:
            raise ValueError("max_tracks must be >= 0")
        if min_length < 1:
            raise ValueError("min_length must be >= 1")
        if not tracks_first and tracks is not None:
            wanted = ShortTime._track_list(tracks)
        return wanted, max_tracks, max_rows, min_length

    def _block_tracks(self, torch, rec, blocks, wanted, max_tracks):
        """The tail of the block pipelines: one period per block, the tracks (ranked when none were named) and the one
        routed overlap-add, whose last row is ``periodic``.  -> ShortTimeTracks."""
        seg, per_h, pw_h, counts_h = self._qo_segments(torch, rec.eng, blocks)
        wanted = self._ranked(per_h, pw_h, counts_h, wanted, max_tracks)
        masks, routed = self._qo_route(torch, rec.eng, seg, blocks, per_h, counts_h, wanted, rec.L, rec.win)
        return self._assemble(rec, per_h, pw_h, counts_h, routed[len(wanted) + 1], wanted, routed, masks)

    @staticmethod
    def _rerun_capped(torch, dev, W, capacities, tensors, launch):
        """The capacity loop of the block pipelines.  `tensors`: the zero-initialised whole-batch results, the weights
        (W, 1) last; ``launch(idx, kcap)`` runs the frames `idx` (None: all of them, otherwise a device index tensor) at
        `kcap` dictionary rows and returns their tensors in that order and the device status words.  The first capacity
        runs the whole batch and its tensors are adopted as they are; every later one runs the frames whose last status
        was PH_ST_CAP, gathered by `launch` and scattered back here, the weights widened to `kcap` columns.  One status
        read-back per capacity.  -> the tensors and the host status words (PH_ST_CAP everywhere, and the zero tensors,
        when `capacities` is empty; a frame still PH_ST_CAP at the end keeps its last attempt)."""
        tensors = list(tensors)
        st = np.full(W, _ffi.PH_ST_CAP, dtype=np.int32)
        todo = np.arange(W)
        for kcap in capacities:
            idx = None if todo.size == W else torch.as_tensor(todo, device=dev)
            *got, s2 = launch(idx, kcap)
            if idx is None:
                tensors = got
            else:
                wts = tensors[-1]
                tensors[-1] = torch.cat([wts, wts.new_zeros((W, kcap - wts.shape[1]))], dim=1)
                for whole, part in zip(tensors, got):
                    whole[idx] = part
            st[todo] = s2.cpu().numpy()
            todo = todo[st[todo] == _ffi.PH_ST_CAP]
            if not todo.size:
                break
        return tensors, st

    def _ram_fit(self, torch, eng, fr, per, cnt, q_hi, max_rows):
        """``qo_fit`` on the lists per[f, :cnt[f]] at the capacities of ``_ram_capacities`` (``_rerun_capped``).
        -> rows per block and weights on the device, the host status words."""
        from .QOPeriods import _ram_capacities

        def launch(idx, kcap):
            k2, w2, _, s2 = (eng.qo_fit(fr, per, cnt, kcap, q_hi) if idx is None else
                             eng.qo_fit(fr[idx], per[idx], cnt[idx], kcap, q_hi))
            return k2, w2, s2

        (W, pcap), dev = per.shape, per.device
        zeros = (torch.zeros((W, pcap), dtype=torch.int32, device=dev),
                 torch.zeros((W, 1), dtype=torch.float64, device=dev))
        (keeps, wts), st = self._rerun_capped(
            torch, dev, W, _ram_capacities(eng, self.frame_length, q_hi, max_rows), zeros, launch)
        return keeps, wts, st

    def _ram_host_route(self, torch, fr, blocks, cnt_h, st, min_length, q_hi):
        """Frames with a list the device fit did not finish: the 1-D ``find_periods_with_weights`` on the same list,
        packed into the device arrays; a dictionary that is singular there too keeps no block.  -> the blocks as the
        extraction takes them and frame_status (W) int8."""
        from .RamanujanPeriods import RamanujanPeriods

        per, keeps, nb, wts = blocks
        status = np.where(cnt_h <= 0, 2, np.where(st == _ffi.PH_ST_OK, 0, 1)).astype(np.int8)
        unfinished = np.flatnonzero(status == 1)
        if unfinished.size:
            idx = torch.as_tensor(unfinished, device=fr.device)
            rows_h, lists_h = fr[idx].cpu().numpy(), per[idx].cpu().numpy()
            rp = RamanujanPeriods()
            packed = []
            for f, row, lst in zip(unfinished, rows_h, lists_h):
                lst = lst[: cnt_h[f]].astype(np.int64)
                try:
                    out, _ = rp.find_periods_with_weights(row, min_length, q_hi, test_function=lambda _norms, lst=lst: lst)
                except np.linalg.LinAlgError:
                    status[f] = 3
                    packed.append(([], [], np.zeros(0)))
                    continue
                wt = np.asarray(out["weights"], dtype=np.float64).reshape(-1)
                packed.append(self._pack_dictionary(wt, out["basis_dictionary"]))
            # (the lists and counts are ramanujan_select's own tensors: the host results go into copies)
            blocks = (per.clone(), keeps.clone(), nb.clone(), wts)
            per, keeps, nb, wts = self._pack_back(torch, blocks, unfinished, packed)
            warn(f"decompose_ramanujan: frames {unfinished.tolist()} were not finished by the device fit and ran on the host")
        return (per.contiguous(), keeps.contiguous(), nb.contiguous(), wts.contiguous()), status

    def _qo_fit(self, torch, eng, fr, fit, max_rows):
        """The device fit at the capacities of ``_qo_capacities`` (``_rerun_capped``); without a feasible capacity every
        frame goes the way of the unfinished ones.  -> (periods, rows, blocks per frame, weights) on the device and the
        host status words."""
        from .QOPeriods import _qo_capacities

        num, thresh, min_length, max_length, uw = fit
        (W, N), dev, trunc = fr.shape, fr.device, self._trunc_to_integer_multiple

        def launch(idx, kcap):
            p2, _, k2, c2, w2, _, s2 = eng.qo_find_periods(fr if idx is None else fr[idx], num, thresh, min_length,
                                                           max_length, kcap, trunc=trunc, update_weights=uw)
            nb2 = c2[:, 1]
            return p2, k2, nb2.contiguous() if idx is None else nb2, w2, s2

        zeros = [torch.zeros(shape, dtype=torch.int32, device=dev) for shape in ((W, num), (W, num), (W,))]
        zeros.append(torch.zeros((W, 1), dtype=torch.float64, device=dev))
        (per, keeps, nb, wts), st = self._rerun_capped(
            torch, dev, W, _qo_capacities(eng, N, self.dtype, num, max_length, uw, max_rows), zeros, launch)
        if not uw:  # a keeps entry of 0 stands for `period` rows
            keeps = torch.where(keeps == 0, per, keeps)
        return (per, keeps, nb, wts), st

    def _qo_host_route(self, torch, fr, silent, st, blocks, fit):
        """Frames the device loop did not finish: the 1-D call, packed into the device arrays.  Then the blocks as the
        extraction takes them: none for a silent frame, every period once, contiguous."""
        from .QOPeriods import QOPeriods

        num, thresh, min_length, max_length, uw = fit
        per, keeps, nb, wts = blocks
        dev, trunc = fr.device, self._trunc_to_integer_multiple
        nb_h = nb.cpu().numpy()
        unfinished = np.flatnonzero(~silent & ((st != _ffi.PH_ST_OK) | (nb_h == 0)))
        if unfinished.size:
            rows_h = fr[torch.as_tensor(unfinished, device=dev)].cpu().numpy()
            qo = QOPeriods(trunc_to_integer_multiple=trunc)
            packed = []
            for f, row in zip(unfinished, rows_h):
                out, _ = qo.find_periods(row, num, thresh, min_length, max_length, uw)
                wt = np.asarray(out["weights"], dtype=np.float64).reshape(-1)
                blocks = self._pack_dictionary(wt, out["basis_dictionary"], not uw)
                if sum(blocks[1]) != wt.size:
                    # (the fixed-weight loop fitted a period twice: the dictionary keeps one entry, the weights both
                    # blocks, and which rows belong to which cannot be told from the two)
                    raise ValueError(f"decompose_qo: the 1-D result of frame {int(f)} has {wt.size} weights for the "
                                     f"{sum(blocks[1])} rows of its dictionary")
                packed.append(blocks)
            pcap = max([num] + [len(p[0]) for p in packed])
            if pcap > _MAX_ROWS:
                raise ValueError(f"{pcap} blocks in frame {int(unfinished[0])}: decompose_qo routes at most {_MAX_ROWS}")
            per, keeps, nb, wts = self._pack_back(torch, (per, keeps, nb, wts), unfinished, packed)
            warn(f"decompose_qo: frames {unfinished.tolist()} were not finished by the device loop and ran on the host")
        if silent.any():
            nb[torch.as_tensor(np.flatnonzero(silent), device=dev)] = 0
        if not uw:  # the fixed-weight loop lists a period once per fit: one block per period for the extraction
            per, keeps, nb, wts = self._merge_repeats(torch, per, keeps, nb, wts, max(max_length, 1))
        per, keeps, nb, wts = per.contiguous(), keeps.contiguous(), nb.contiguous(), wts.contiguous()
        return per, keeps, nb, wts

    @staticmethod
    def _pack_back(torch, blocks, unfinished, packed):
        """The host results of the frames `unfinished` -- one ``_pack_dictionary`` triple each -- written into the device
        blocks (periods, rows, blocks per frame, weights): the first two widened to the longest list, the weights to the
        longest weight vector, zeros behind what a frame uses.  The tensors are written in place where they are wide
        enough.  -> the four tensors."""
        per, keeps, nb, wts = blocks
        W, dev, n = per.shape[0], per.device, len(packed)
        pcap = max([per.shape[1]] + [len(p[0]) for p in packed])
        kneed = max([wts.shape[1]] + [p[2].size for p in packed])
        if pcap > per.shape[1]:
            per = torch.cat([per, per.new_zeros((W, pcap - per.shape[1]))], dim=1)
            keeps = torch.cat([keeps, keeps.new_zeros((W, pcap - keeps.shape[1]))], dim=1)
        if kneed > wts.shape[1]:
            wts = torch.cat([wts, wts.new_zeros((W, kneed - wts.shape[1]))], dim=1)
        hp, hk = np.zeros((n, pcap), np.int32), np.zeros((n, pcap), np.int32)
        hw, hn = np.zeros((n, kneed)), np.zeros(n, np.int32)
        for j, (ps, ks, ws_) in enumerate(packed):
            hn[j] = len(ps)
            hp[j, : len(ps)], hk[j, : len(ps)], hw[j, : ws_.size] = ps, ks, ws_
        idx = torch.as_tensor(unfinished, device=dev)
        per[idx], keeps[idx] = torch.as_tensor(hp, device=dev), torch.as_tensor(hk, device=dev)
        wts[idx], nb[idx] = torch.as_tensor(hw, device=dev), torch.as_tensor(hn, device=dev)
        return per, keeps, nb, wts

    @staticmethod
    def _qo_segments(torch, eng, blocks):
        """One period per block (``qo_get_periods``) and its power.  -> the (W, ccap) segments on the device and the
        host periods, powers (zeros behind the blocks in use) and blocks per frame."""
        per, keeps, nb, wts = blocks
        (W, pcap), dev = per.shape, per.device
        slot = torch.arange(pcap, device=dev)[None, :]
        used = slot < nb[:, None]
        ends = torch.cumsum((per.clamp(min=0) * used).to(torch.int64), dim=1)  # (W, pcap): end of block a
        ccap = max(1, int(ends[:, -1].max().item()))  # the one word read back
        seg, gst = eng.qo_get_periods(per, keeps, nb, wts, ccap=ccap)
        gst = gst.cpu().numpy()
        nb_h = nb.cpu().numpy()
        bad = (gst != _ffi.PH_ST_OK) & ~((gst == _ffi.PH_ST_NO_PERIOD) & (nb_h <= 0))
        if bad.any():
            raise ValueError(f"decompose_qo: the dictionary of frame {_first(bad)} cannot be extracted "
                             f"(status {int(gst[_first(bad)])})")
        col = torch.arange(ccap, device=dev)[None, :]
        sq = seg * seg
        powers = torch.zeros((W, pcap), dtype=torch.float64, device=dev)
        for a in range(pcap):  # one pass over seg per block index
            hi = ends[:, a : a + 1]
            lo = hi - per[:, a : a + 1].clamp(min=0)
            inside = (col >= lo) & (col < hi) & used[:, a : a + 1]
            powers[:, a] = torch.where(inside, sq, sq.new_zeros(())).sum(dim=1) / per[:, a].clamp(min=1)
        per_h = np.where(used.cpu().numpy(), per.cpu().numpy(), 0)
        pw_h = np.where(per_h > 0, powers.cpu().numpy(), 0.0)
        counts_h = np.clip(nb_h, 0, pcap).astype(np.int32)
        return seg, per_h, pw_h, counts_h

    def _qo_route(self, torch, eng, seg, blocks, per_h, counts_h, wanted, L, win):
        """T mask rows for the tracks, one for `other` and one with every block (`periodic`), folded in one launch."""
        per, _, nb, _ = blocks
        T, W = len(wanted), per.shape[0]
        masks = np.empty((T + 2, W), np.uint64)
        masks[: T + 1] = self.track_masks(per_h, counts_h, wanted)
        low = (np.uint64(1) << np.minimum(counts_h, 63).astype(np.uint64)) - np.uint64(1)
        masks[T + 1] = np.where(counts_h >= 64, np.uint64(2**64 - 1), low)  # every block in use
        masks_d = torch.as_tensor(masks.view(np.int64), device=per.device)
        routed = eng.overlap_add_periodic(seg, per, nb, masks_d, self.frame_length, self.hop, L, win, win, True)
        return masks, routed.cpu().numpy()

    @staticmethod
    def _merge_repeats(torch, per, keeps, nb, wts, max_block):
        """The blocks of the fixed-weight loop with every period listed once: that loop fits a period again whenever
        it is the strongest of the running residual (and once more when the test function stops it), each time as a
        block of its own, and ``qo_get_periods`` refuses a period listed twice.  Blocks of one period are added -- the
        tiles of a sum are the sum of the tiles, so the reconstruction is unchanged -- into the slot of the first, in
        ascending block order; rows = the most any of them has.  Device tensors in, device tensors out; `max_block`
        bounds the rows of one block.  One word is read back (does anything repeat?)."""
        W, P = per.shape
        Kc = wts.shape[1]
        ar = torch.arange(P, device=per.device)
        used = ar[None, :] < nb[:, None]
        same = (per[:, :, None] == per[:, None, :]) & used[:, :, None] & used[:, None, :]
        first = same.to(torch.int8).argmax(dim=2)  # [f, a]: the first block with the period of block a
        lead = used & (first == ar[None, :])
        if bool((lead == used).all()):
            return per, keeps, nb, wts
        # new index of every used block (a frame without blocks has no first one: 0, an index like any other -- it is
        # used to gather below -- and no row of such a frame is moved)
        slot = torch.gather(torch.cumsum(lead.to(torch.int64), dim=1) - 1, 1, first).clamp(min=0)
        rows = (keeps * used).to(torch.int64)
        old_off = torch.cumsum(rows, dim=1) - rows
        where = torch.where(used, slot, torch.full_like(slot, P))  # unused blocks land in a column that is dropped
        new_per = per.new_zeros((W, P + 1)).scatter_(1, where, per)[:, :P]
        new_rows = rows.new_zeros((W, P + 1)).scatter_reduce_(1, where, rows, "amax")[:, :P]
        new_off = torch.cumsum(new_rows, dim=1) - new_rows
        new_wts = torch.zeros_like(wts)
        j = torch.arange(min(int(max_block), Kc), device=per.device)[None, :]
        for a in range(P):  # ascending a: one fixed order of addition; inside one a no two rows share a target
            valid = j < rows[:, a : a + 1]
            src = (old_off[:, a : a + 1] + j).clamp(max=Kc - 1)
            dst = (torch.gather(new_off, 1, slot[:, a : a + 1]) + j).clamp(max=Kc - 1)
            vals = torch.where(valid, torch.gather(wts, 1, src), wts.new_zeros(()))
            new_wts.scatter_add_(1, dst, vals)
        return new_per, new_rows.to(torch.int32), lead.sum(dim=1).to(torch.int32), new_wts

    @staticmethod
    def _pack_dictionary(weights, dictionary, zero_is_period=False):
        """A 1-D find_periods result as the blocks qo_get_periods takes: -> (periods, rows, weights) with the slice
        semantics of ``QOPeriods.get_periods`` (an entry with more rows than its period keeps `period` of them).
        `zero_is_period`: the fixed-weight loop writes 0 for a block that kept all `period` rows (``Pp(keep=0)``)."""
        from .QOPeriods import QOPeriods

        ps, ks, blocks, read = [], [], [], 0
        for q, r in dictionary.items():
            q, r = int(q), int(r)
            if zero_is_period and r == 0:
                r = q
            v = QOPeriods.concatenate_periods(weights[read:], {str(q): r})
            k = r if 0 <= r <= q else q
            read += r
            ps.append(q)
            ks.append(k)
            blocks.append(v[:k])
        return ps, ks, (np.concatenate(blocks) if blocks else np.zeros(0))

    @staticmethod
    def _track_list(tracks):
        """[12, (17, 34)] -> [(12,), (17, 34)]; ValueError for an empty list or entry, a period < 1 or a period in two
        tracks (twice in one track counts once)."""
        def walk(obj):  # the items of a non-str iterable, None for anything else (a str, a number, a 0-d array)
            if isinstance(obj, (str, bytes)):
                return None
            try:
                return list(obj)
            except TypeError:
                return None

        entries = walk(tracks)
        if entries is None:
            raise ValueError("tracks must be a list of periods or of iterables of periods")
        out, seen = [], set()
        for entry in entries:
            group = walk(entry)
            if group is None:
                group = [entry.item() if isinstance(entry, np.ndarray) else entry]
            if not group:
                raise ValueError("a track needs at least one period")
            ps = []
            for p in group:
                if isinstance(p, bool) or not isinstance(p, (int, np.integer)):
                    raise ValueError(f"track period {p!r} is not an integer")
                p = int(p)
                if p < 1:
                    raise ValueError(f"track period {p} must be >= 1")
                if p not in ps:
                    ps.append(p)
            if seen.intersection(ps):
                raise ValueError(f"period {sorted(seen.intersection(ps))[0]} is in two tracks")
            seen.update(ps)
            out.append(tuple(ps))
        if not out:
            raise ValueError("tracks must name at least one track")
        return out

    @staticmethod
    def _used(periods, counts):
        """(W, K) int64 periods and the mask of the entries in use (k < counts[f], counts clipped to [0, K])."""
        per = np.asarray(periods)
        if per.ndim != 2:
            raise ValueError("periods must be (W, K)")
        per = per.astype(np.int64)
        W, K = per.shape
        if counts is None:
            return per, np.ones((W, K), bool)
        cnt = np.asarray(counts)
        if cnt.shape != (W,):
            raise ValueError("counts must hold one entry per frame")
        return per, np.arange(K)[None, :] < np.clip(cnt.astype(np.int64), 0, K)[:, None]

    @staticmethod
    def rank_periods(periods, powers, counts=None, max_tracks=8):
        """The `max_tracks` strongest periods of a recording: over the distinct non-zero periods among the used entries
        of `periods` (W, K), the sum of their `powers` (NaN counts as 0), in descending order, ties to the smaller
        period.  -> list of ints."""
        per, used = ShortTime._used(periods, counts)
        pw = np.asarray(powers, dtype=np.float64)
        if pw.shape != per.shape:
            raise ValueError("powers must have the shape of periods")
        used = used & (per != 0)
        uniq, inv = np.unique(per[used], return_inverse=True)
        score = np.bincount(inv.ravel(), weights=np.nan_to_num(pw[used], nan=0.0, posinf=np.inf, neginf=-np.inf),
                            minlength=uniq.size)
        order = sorted(range(uniq.size), key=lambda j: (-score[j], uniq[j]))
        return [int(uniq[j]) for j in order[: max(int(max_tracks), 0)]]

    @staticmethod
    def track_masks(periods, counts, track_periods):
        """The routing masks of ``PeriodEngine.overlap_add_tracks`` for T tracks: (T + 1, W) uint64 with bit k of
        [t, f] set when entry k of frame f is in use (k < counts[f]; None: all) and periods[f, k] is in
        track_periods[t]; row T takes every used entry that is in no track, period 0 included.  K <= 64."""
        per, used = ShortTime._used(periods, counts)
        W, K = per.shape
        if K > _MAX_ROWS:
            raise ValueError(f"{K} entries per frame do not fit a 64-bit mask")
        groups = ShortTime._track_list(track_periods) if len(track_periods) else []
        T = len(groups)
        masks = np.zeros((T + 1, W), np.uint64)
        for k in range(K):
            bit = np.uint64(1) << np.uint64(k)
            taken = np.zeros(W, bool)
            for t, group in enumerate(groups):
                hit = used[:, k] & np.isin(per[:, k], group)
                masks[t, hit] |= bit
                taken |= hit
            masks[T, used[:, k] & ~taken] |= bit
        return masks

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
            raise TypeError(f"{method}: no candidate period has a positive norm (an all-zero window, or every sum NaN) in frame "
                            f"{_first(status == _ffi.PH_ST_NO_PERIOD)}")
        if np.any(status == _ffi.PH_ST_ITER_CAP):
            raise RuntimeError(f"{method}: iteration bound reached before `num` periods were found in frame "
                               f"{_first(status == _ffi.PH_ST_ITER_CAP)}")
