"""Batched host planner over the C ABI: one `PeriodEngine` per GPU.

Every method takes a batch of independent signal windows, row-major ``(W, N)``:
  * a numpy array  -> host-pointer call; the library stages data through its own device
    buffers and returns numpy arrays (this is what the drop-in classes use);
  * a torch CUDA tensor -> device-pointer call on torch's current stream; outputs are torch
    tensors on the same device and nothing crosses PCIe (what bench.py and the sharded
    multi-GPU path use).

No arithmetic of the path happens here; this file only shapes arguments for
``libperiod_hip.so`` and raises if the library or the GPU is missing.
"""

from __future__ import annotations

import ctypes as C
import os
import threading
from typing import NamedTuple

import numpy as np

from . import _factors, _ffi

_NP_DTYPES = {np.dtype(np.float64): _ffi.PH_F64, np.dtype(np.float32): _ffi.PH_F32}


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


class _Out:
    """Allocates outputs next to the input (numpy or torch) and hands out raw addresses."""

    def __init__(self, like):
        self.torch = _is_torch(like)
        self.stream = None  # hipStream_t handle the call must run on (None = the context's own)
        if self.torch:
            import torch

            self._t = torch
            self.device = like.device

    def empty(self, shape, dtype):
        if self.torch:
            tdt = {
                np.float64: self._t.float64,
                np.float32: self._t.float32,
                np.int32: self._t.int32,
                np.uint32: self._t.int32,  # same bits; viewed back by the caller if needed
            }[dtype]
            return self._t.empty(shape, dtype=tdt, device=self.device)
        return np.empty(shape, dtype=dtype)

    @staticmethod
    def addr(a):
        if a is None:
            return None
        if _is_torch(a):
            return a.data_ptr()
        return a.ctypes.data


class KernelPlan(NamedTuple):
    """One kernel of an entry point's launch plan (ph_plan_info; values are the PH_PLAN_* constants of _ffi)."""

    variant: int  # PH_PLAN_ONE, PH_PLAN_PAIR, PH_PLAN_FFT, PH_PLAN_CHIRP, PH_PLAN_DIRECT
    window: int  # PH_PLAN_LDS or PH_PLAN_HBM
    second: int  # PH_PLAN_NONE, PH_PLAN_LDS or PH_PLAN_HBM
    block: int
    lds_bytes: int
    small_means: int
    waves: int
    pad: int


def _side(mk, x, a, dtype, name, of="x", joint=False):
    """A side array of a call next to its main array `x`: with torch input a contiguous `dtype` tensor on x's device, with
    numpy input a contiguous numpy array (dtype None: as it is).  `joint`: `name` lists several arrays refused as one."""
    if not mk.torch:
        return np.ascontiguousarray(a, dtype=dtype)
    tname = np.dtype(dtype).name
    if not _is_torch(a) or a.dtype != getattr(mk._t, tname) or a.device != x.device:
        kind = f"{tname} tensors" if joint else f"{'an' if tname[0] == 'i' else 'a'} {tname} tensor"
        raise TypeError(f"{name} must be {kind} on the device of {of}")
    return a.contiguous()


def _masks(mk, x, masks, W, of):
    """The (T, W) routing masks of a routed overlap-add: np.uint64 / np.int64, or with torch input torch.int64."""
    if not mk.torch and (not isinstance(masks, np.ndarray) or masks.dtype not in (np.dtype(np.uint64), np.dtype(np.int64))):
        raise TypeError("masks must be a uint64 or int64 array")
    msk = _side(mk, x, masks, np.int64 if mk.torch else None, "masks", of)
    if msk.ndim != 2 or msk.shape[1] != W:
        raise ValueError("masks must be (T, W): one word per track and frame")
    return msk


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data


class PeriodEngine:
    """Owns one ``ph_ctx`` (one GPU, one stream)."""

    def __init__(self, device: int | None = None):
        self._lib = _ffi.load()
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        n = C.c_int(0)
        _ffi.check(self._lib.ph_device_count(C.byref(n)))
        if n.value < 1:
            raise _ffi.PeriodHipError("no HIP device visible; pyperiod_amd has no CPU fallback")
        self.device = device % n.value
        ctx = C.c_void_p()
        _ffi.check(self._lib.ph_create(self.device, C.byref(ctx)))
        self._ctx = ctx
        self._bound_stream = None
        self._lock = threading.Lock()
        cu, lds = C.c_int(0), C.c_int(0)
        _ffi.check(self._lib.ph_device_info(self._ctx, C.byref(cu), C.byref(lds)))
        self.num_cu, self.lds_bytes = cu.value, lds.value

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.ph_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ plumbing
    def _prep(self, x):
        """-> (array, dtype code, W, N, flags, out-factory); binds torch's stream if needed."""
        if _is_torch(x):
            import torch

            if not x.is_cuda:
                raise ValueError("torch input must live on the GPU (or pass a numpy array)")
            if x.device.index != self.device:
                raise ValueError(f"tensor on cuda:{x.device.index}, engine on cuda:{self.device}")
            if x.dim() != 2:
                raise ValueError("expected a (W, N) batch of windows")
            x = x.contiguous()
            code = {torch.float64: _ffi.PH_F64, torch.float32: _ffi.PH_F32}.get(x.dtype)
            if code is None:
                raise TypeError(f"unsupported dtype {x.dtype}")
            mk = _Out(x)
            # torch's default stream has the handle 0 (== NULL, "own stream" in the C ABI)
            mk.stream = torch.cuda.current_stream(x.device).cuda_stream or _ffi.PH_STREAM_DEFAULT
            return x, code, x.shape[0], x.shape[1], _ffi.PH_FLAG_DEVICE, mk
        x = np.asarray(x)
        if x.ndim != 2:
            raise ValueError("expected a (W, N) batch of windows")
        if x.dtype not in _NP_DTYPES:
            x = x.astype(np.float64)
        x = np.ascontiguousarray(x)
        return x, _NP_DTYPES[x.dtype], x.shape[0], x.shape[1], 0, _Out(x)

    def _call(self, mk, W, fn, *args, check=True):
        """One library call under the engine lock: the context is bound to the caller's stream
        (torch's current stream for device tensors, the context's own stream for numpy) and the
        entry point is invoked while the lock is held, so threads sharing an engine cannot launch
        on each other's stream.  An empty batch (W == 0, e.g. a trailing rank of a sharded run)
        makes no call: the outputs are already empty."""
        if W == 0:
            return _ffi.PH_OK
        with self._lock:
            want = mk.stream
            if want != self._bound_stream:
                _ffi.check(self._lib.ph_set_stream(self._ctx, C.c_void_p(want) if want else None))
                self._bound_stream = want
            rc = fn(self._ctx, *args)
        if check:
            _ffi.check(rc)
        return rc

    @staticmethod
    def _np_dtype(code):
        return np.float64 if code == _ffi.PH_F64 else np.float32

    @staticmethod
    def _flags(trunc, orth):
        return (_ffi.PH_FLAG_TRUNC if trunc else 0) | (_ffi.PH_FLAG_ORTH if orth else 0)

    @staticmethod
    def _orth(orth, max_p):
        if not orth:
            return None, None, None, None, 0
        off, q = _factors.orth_tables(int(max_p))
        return off, q, off.ctypes.data, q.ctypes.data, int(max_p)

    def sync(self):
        _ffi.check(self._lib.ph_sync(self._ctx))

    def timer_begin(self):
        _ffi.check(self._lib.ph_timer_begin(self._ctx))

    def timer_end(self) -> float:
        ms = C.c_float(0)
        _ffi.check(self._lib.ph_timer_end(self._ctx, C.byref(ms)))
        return float(ms.value)

    def profile(self, on: bool = True):
        """Start (or stop) bracketing every kernel launch with HIP events on the stream."""
        _ffi.check(self._lib.ph_profile_enable(self._ctx, 1 if on else 0))

    def profile_read(self):
        """-> [(kernel name, milliseconds)] for every launch since profile(True)."""
        n = C.c_int(0)
        buf = (C.c_float * 256)()
        _ffi.check(self._lib.ph_profile_read(self._ctx, buf, 256, C.byref(n)))
        return [(self._lib.ph_profile_name(self._ctx, i).decode(), float(buf[i])) for i in range(min(n.value, 256))]

    def max_window(self, dtype=np.float64, trunc=False, orth=False) -> int:
        n = C.c_int(0)
        code = _NP_DTYPES[np.dtype(dtype)]
        _ffi.check(self._lib.ph_max_window(self._ctx, code, self._flags(trunc, orth), C.byref(n)))
        return n.value

    # ------------------------------------------------------------------ kernels
    def periodic_norm(self, x, p=None):
        x, code, W, N, fl, mk = self._prep(x)
        out = mk.empty((W,), np.float64)
        self._call(mk, W, self._lib.ph_periodic_norm, mk.addr(x), code, W, N, int(p) if p else 0, fl, mk.addr(out))
        return out

    def project_batch(self, x, p_list, trunc=False, orth=False, single=False):
        """out[w, k, :] = project(x[w], p_list[k]); Periods.py:142-219."""
        x, code, W, N, fl, mk = self._prep(x)
        pl, pl_addr = _i32(np.atleast_1d(p_list))
        if pl.size < 1 or pl.min() < 1:
            raise ValueError("periods must be >= 1")
        keep = self._orth(orth, pl.max())
        out = mk.empty((W, pl.size, N), self._np_dtype(code))
        flags = fl | self._flags(trunc, orth) | (_ffi.PH_FLAG_SINGLE if single else 0)
        self._call(mk, W, self._lib.ph_project_batch, mk.addr(x), code, W, N, pl_addr, pl.size, keep[2], keep[3], keep[4],
                   flags, mk.addr(out))
        return out

    def sweep(self, x, p_lo, p_hi, mode=_ffi.PH_SWEEP_NORM, trunc=False, orth=False):
        """(W, p_hi-p_lo+1) float64 sweep values; Periods.py:501-510 / :324-331."""
        x, code, W, N, fl, mk = self._prep(x)
        keep = self._orth(orth and mode != _ffi.PH_SWEEP_MAXABS, p_hi)
        out = mk.empty((W, int(p_hi) - int(p_lo) + 1), np.float64)
        self._call(mk, W, self._lib.ph_sweep, mk.addr(x), code, W, N, int(p_lo), int(p_hi), int(mode), keep[2], keep[3],
                   keep[4], fl | self._flags(trunc, orth), mk.addr(out))
        return out

    def sweep_plan_info(self, p_lo, p_hi):
        """Pass plan of the norm sweeps over [p_lo, p_hi]: (passes, periods) -- every pass reads the
        LDS-resident window once and yields one to three candidate periods."""
        n_pass, n_per = C.c_int(0), C.c_int(0)
        _ffi.check(self._lib.ph_sweep_plan_info(self._ctx, int(p_lo), int(p_hi), C.byref(n_pass), C.byref(n_per)))
        return n_pass.value, n_per.value

    def _m_best_query(self, n, num, max_length, min_length, dtype, trunc, orth):
        """The arguments the three ph_m_best_*_info queries share (a missing max_length: the library's default)."""
        return (self._ctx, _NP_DTYPES[np.dtype(dtype)], int(n), int(num), int(min_length),
                -1 if max_length is None else int(max_length), self._flags(trunc, orth))

    def m_best_info(self, n, num=5, max_length=None, min_length=2, dtype=np.float64, trunc=False, orth=False):
        """(windows per workgroup, LDS bytes per sample and workgroup) of the step-1 kernel m_best would run:
        (2, 8) for the window-pair float screen, (1, itemsize) for the one-window fold."""
        wpw, bps = C.c_int(0), C.c_int(0)
        _ffi.check(self._lib.ph_m_best_info(*self._m_best_query(n, num, max_length, min_length, dtype, trunc, orth),
                                            C.byref(wpw), C.byref(bps)))
        return wpw.value, bps.value

    def m_best_plan_info(self, n, num=5, max_length=None, min_length=2, dtype=np.float64, trunc=False, orth=False):
        """(passes, periods) of one sweep of the step-1 kernel m_best would run (the window-pair kernel takes the
        periods up to 64 in chains, so it needs fewer passes than sweep_plan_info reports for the fp64 sweeps)."""
        n_pass, n_per = C.c_int(0), C.c_int(0)
        _ffi.check(self._lib.ph_m_best_plan_info(*self._m_best_query(n, num, max_length, min_length, dtype, trunc, orth),
                                                 C.byref(n_pass), C.byref(n_per)))
        return n_pass.value, n_per.value

    def m_best_screen_info(self, n, num=5, max_length=None, min_length=2, gamma=False, dtype=np.float64, trunc=False,
                           orth=False):
        """(plan entries, periods they fold, LDS elements read) per sweep and workgroup of the step-1 kernel m_best
        (gamma: m_best_gamma) would run.  The window-pair kernel folds p and p + 64 from one set of loads where it can,
        so it has fewer entries than periods (PH_PAIR_DUO=0: one pass per period)."""
        n_ent, n_scr, elems = C.c_int(0), C.c_int(0), C.c_longlong(0)
        _ffi.check(self._lib.ph_m_best_screen_info(*self._m_best_query(n, num, max_length, min_length, dtype, trunc, orth),
                                                   int(bool(gamma)), C.byref(n_ent), C.byref(n_scr), C.byref(elems)))
        return n_ent.value, n_scr.value, elems.value

    def m_best(self, x, num=5, max_length=None, min_length=2, gamma=False, trunc=False, orth=False, want_sweeps=False):
        """-> periods (W,num) uint32, powers (W,num) f64, bases (W,num,N), status (W) int32
        [, n_sweeps (W) int32 when want_sweeps].  A row whose list holds period 1 ends PH_ST_NO_PERIOD: the reference
        raises there."""
        x, code, W, N, fl, mk = self._prep(x)
        if max_length is None:
            max_length = N // 3
        max_length, min_length, num = int(max_length), int(min_length), int(num)
        keep = self._orth(orth, max_length)
        foff, fq = _factors.factor_tables(max(max_length, 1))
        periods = mk.empty((W, num), np.uint32)
        powers = mk.empty((W, num), np.float64)
        bases = mk.empty((W, num, N), self._np_dtype(code))
        status = mk.empty((W,), np.int32)
        sweeps = mk.empty((W,), np.int32) if want_sweeps else None
        self._call(mk, W, self._lib.ph_m_best, mk.addr(x), code, W, N, num, min_length, max_length, 1 if gamma else 0,
                   keep[2], keep[3], foff.ctypes.data, fq.ctypes.data, max(max_length, 1),
                   fl | self._flags(trunc, orth), mk.addr(periods), mk.addr(powers), mk.addr(bases), mk.addr(status),
                   mk.addr(sweeps))
        if min_length <= 1 and W:
            # a row that ends with period 1 (only min_length <= 1 offers it): the reference's step 2 asks for
            # get_factors(1, remove_1_and_n=True) and dies with KeyError (Periods.py:548) -- no result, so a status
            one = (periods == 1).any(1) & (status == _ffi.PH_ST_OK)
            if mk.torch:
                status.masked_fill_(one, _ffi.PH_ST_NO_PERIOD)  # (no read-back: the call stays asynchronous)
            else:
                status[one] = _ffi.PH_ST_NO_PERIOD
        if want_sweeps:
            return periods, powers, bases, status, sweeps
        return periods, powers, bases, status

    def small_to_large(self, x, thresh=0.1, n_periods=None, trunc=False, orth=False, cap=16, want_bases=True,
                       nosync=False):
        """-> counts (W), periods (W,cap) int32, powers (W,cap), bases (W,cap,N)|None, status (W).
        A window that accepts more than `cap` periods makes the library return PH_E_CAP -- for
        numpy and for device tensors alike (the library reads one device word back) -- and the
        call is repeated with the capacity the batch needs.  nosync=True (device tensors only)
        skips that read-back: the call stays asynchronous and the caller must look at `status`
        (PH_ST_CAP) / `counts` itself."""
        x, code, W, N, fl, mk = self._prep(x)
        if n_periods is None:
            n_periods = N // 2
        n_periods = int(n_periods)
        keep = self._orth(orth, max(n_periods, 1))
        fl |= _ffi.PH_FLAG_NOSYNC if (nosync and mk.torch) else 0
        while True:
            counts = mk.empty((W,), np.int32)
            periods = mk.empty((W, cap), np.int32)
            powers = mk.empty((W, cap), np.float64)
            bases = mk.empty((W, cap, N), self._np_dtype(code)) if want_bases else None
            status = mk.empty((W,), np.int32)
            rc = self._call(mk, W, self._lib.ph_small_to_large, mk.addr(x), code, W, N, float(thresh), n_periods,
                            keep[2], keep[3], keep[4], fl | self._flags(trunc, orth), int(cap), mk.addr(counts),
                            mk.addr(periods), mk.addr(powers), mk.addr(bases), mk.addr(status), check=False)
            if rc == _ffi.PH_E_CAP:
                cap = int(counts.max())
                continue
            _ffi.check(rc)
            return counts, periods, powers, bases, status

    def best_correlation(self, x, num=5, max_length=None, ratio=0.01, trunc=False, orth=False):
        x, code, W, N, fl, mk = self._prep(x)
        if max_length is None:
            max_length = N // 3
        max_length, num = int(max_length), int(num)
        keep = self._orth(orth, max(max_length, 1))
        periods = mk.empty((W, num), np.uint32)
        norms = mk.empty((W, num), np.float64)
        bases = mk.empty((W, num, N), self._np_dtype(code))
        status = mk.empty((W,), np.int32)
        self._call(mk, W, self._lib.ph_best_correlation, mk.addr(x), code, W, N, num, max_length, float(ratio), keep[2],
                   keep[3], keep[4], fl | self._flags(trunc, orth), mk.addr(periods), mk.addr(norms), mk.addr(bases),
                   mk.addr(status))
        return periods, norms, bases, status

    def best_frequency(self, x, win_size=None, num=5, trunc=False, orth=False):
        """Periods.best_frequency over a batch (Periods.py:351-398): periods (W, num) uint32, powers
        (W, num), bases (W, num, N), status (W) -- PH_ST_NO_PERIOD where the reference raises."""
        x, code, W, N, fl, mk = self._prep(x)
        win_size = N if win_size is None else int(win_size)
        num = int(num)
        keep = self._orth(orth, 2 * max(win_size, 1))
        periods = mk.empty((W, num), np.uint32)
        powers = mk.empty((W, num), np.float64)
        bases = mk.empty((W, num, N), self._np_dtype(code))
        status = mk.empty((W,), np.int32)
        for w0 in range(0, W, 65535):  # the spectrum kernel's grid.y holds the window index
            w1 = min(W, w0 + 65535)
            self._call(mk, w1 - w0, self._lib.ph_best_frequency, mk.addr(x[w0:w1]), code, w1 - w0, N, win_size, num,
                       keep[2], keep[3], keep[4], fl | self._flags(trunc, orth), mk.addr(periods[w0:w1]),
                       mk.addr(powers[w0:w1]), mk.addr(bases[w0:w1]), mk.addr(status[w0:w1]))
        return periods, powers, bases, status

    def ramanujan_norms(self, x, q_lo=2, q_hi=None):
        """(W, q_hi+1) float64; RamanujanPeriods.py:67-86."""
        x, code, W, N, fl, mk = self._prep(x)
        if not q_hi:
            q_hi = N // 3
        out = mk.empty((W, int(q_hi) + 1), np.float64)
        self._call(mk, W, self._lib.ph_ramanujan_norms, mk.addr(x), code, W, N, int(q_lo), int(q_hi), fl, mk.addr(out))
        return out

    def dict_project(self, x, basis):
        """RamanujanPeriods.project(x, basis) for an arbitrary dictionary (numpy only)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        basis = np.ascontiguousarray(basis, dtype=np.float64)
        if x.ndim != 1 or basis.ndim != 2 or basis.shape[1] != x.size:
            raise ValueError("x must be (N,) and basis (rows, N)")
        out = np.empty(basis.shape, dtype=np.float32)
        self._call(_Out(x), basis.shape[0], self._lib.ph_dict_project, x.ctypes.data, basis.ctypes.data, basis.shape[0],
                   x.size, 0, out.ctypes.data)
        return out

    def _window(self, mk, x, window, N):
        """One float64 analysis window of N samples for a batch: a numpy array, or with torch input a tensor on x's device."""
        win = _side(mk, x, window, np.float64, "window")
        if tuple(win.shape) != (N,):
            raise ValueError(f"window must hold N={N} samples")
        return win

    def qo_find_periods(self, x, num, thresh, min_length=2, max_length=None, kcap=512, trunc=False, update_weights=True,
                        window=None):
        """QOPeriods.find_periods (non-orthogonal selection, default test function) for a batch.
        -> periods (W,num) u32, norms (W,num), keeps (W,num) i32, counts (W,2) i32, weights (W,kcap) f64,
        residual (W,N), status (W).  trunc: trunc_to_integer_multiple selection; update_weights=False:
        the fixed-weight loop (PH_FLAG_KEEP_WEIGHTS) -- rows of block b are keeps[b], or periods[b] when
        keeps[b] == 0, and counts[w, 1] blocks include the re-fitted last one (periodhip.h).
        `window`: None, or with update_weights=False one float64 analysis window of N samples for the whole batch
        (ph_qo_greedy_win; with torch input a float64 tensor on x's device).  With update_weights=True a window raises
        ValueError: that loop is stepped from the host (sweep + qo_fit(window=...))."""
        x, code, W, N, fl, mk = self._prep(x)
        if window is not None and update_weights:
            raise ValueError("window needs update_weights=False here: the re-solved loop under a window is host-stepped")
        win = None if window is None else self._window(mk, x, window, N)
        fl |= (_ffi.PH_FLAG_TRUNC if trunc else 0) | (0 if update_weights else _ffi.PH_FLAG_KEEP_WEIGHTS)
        if max_length is None:
            max_length = N // 3
        num = int(num)
        periods = mk.empty((W, num), np.uint32)
        norms = mk.empty((W, num), np.float64)
        keeps = mk.empty((W, num), np.int32)
        counts = mk.empty((W, 2), np.int32)
        weights = mk.empty((W, int(kcap)), np.float64)
        resid = mk.empty((W, N), self._np_dtype(code))
        status = mk.empty((W,), np.int32)
        if win is not None:
            self._call(mk, W, self._lib.ph_qo_greedy_win, mk.addr(x), code, W, N, mk.addr(win), num, float(thresh),
                       int(min_length), int(max_length), int(kcap), fl, mk.addr(periods), mk.addr(norms), mk.addr(keeps),
                       mk.addr(counts), mk.addr(weights), mk.addr(resid), mk.addr(status))
            return periods, norms, keeps, counts, weights, resid, status
        self._call(mk, W, self._lib.ph_qo_find_periods, mk.addr(x), code, W, N, num, float(thresh), int(min_length),
                   int(max_length), int(kcap), fl, mk.addr(periods), mk.addr(norms), mk.addr(keeps), mk.addr(counts),
                   mk.addr(weights), mk.addr(resid), mk.addr(status))
        return periods, norms, keeps, counts, weights, resid, status

    def qo_feasible(self, n, dtype=np.float64, kcap=512, max_length=None, update_weights=True) -> bool:
        """Whether ph_qo_find_periods can run a window of n samples with `kcap` dictionary rows
        (bookkeeping + the work vectors of the conjugate-gradient solve must fit the workgroup's LDS).
        The fixed-weight loop (update_weights=False) keeps nothing but the window in LDS (its divisor set and weights
        live in HBM): every n and max_length is feasible."""
        if not update_weights:
            return True
        ok = C.c_int(0)
        code = _NP_DTYPES[np.dtype(dtype)]
        _ffi.check(self._lib.ph_qo_feasible(self._ctx, code, int(n), int(max_length if max_length is not None else n // 3),
                                            int(kcap), C.byref(ok)))
        return bool(ok.value)

    def qo_plan_info(self, n, dtype=np.float64, kcap=512, max_length=None, trunc=False, update_weights=True):
        """-> (placement, lds_bytes): where qo_find_periods would keep the residual window of n samples --
        _ffi.PH_QO_LDS_OVERLAY, PH_QO_LDS_BEHIND or PH_QO_HBM (periodhip.h) -- and the LDS one workgroup asks for.
        Nothing runs on the device."""
        fl = (_ffi.PH_FLAG_TRUNC if trunc else 0) | (0 if update_weights else _ffi.PH_FLAG_KEEP_WEIGHTS)
        lds, where = C.c_int(0), C.c_int(0)
        code = _NP_DTYPES[np.dtype(dtype)]
        _ffi.check(self._lib.ph_qo_plan_info(self._ctx, code, int(n), int(max_length if max_length is not None else n // 3),
                                             int(kcap), fl, C.byref(lds), C.byref(where)))
        return where.value, lds.value

    _PLAN_OPS = {"project": _ffi.PH_OP_PROJECT, "sweep": _ffi.PH_OP_SWEEP, "m_best": _ffi.PH_OP_M_BEST,
                 "small_to_large": _ffi.PH_OP_SMALL_TO_LARGE, "best_correlation": _ffi.PH_OP_BEST_CORRELATION,
                 "best_frequency": _ffi.PH_OP_BEST_FREQUENCY, "ramanujan": _ffi.PH_OP_RAMANUJAN,
                 "orth_powers": _ffi.PH_OP_ORTH_POWERS, "fold_sums": _ffi.PH_OP_FOLD_SUMS, "qo_fit": _ffi.PH_OP_QO_FIT,
                 "qo_fit_win": _ffi.PH_OP_QO_FIT_WIN, "qo_orth_select": _ffi.PH_OP_QO_ORTH_SELECT,
                 "qo_get_periods": _ffi.PH_OP_QO_GET_PERIODS}

    def plan_info(self, op, n, params=(), dtype=np.float64, trunc=False, orth=False):
        """-> tuple of one KernelPlan per kernel the entry point `op` ("project", "sweep", "m_best", ...) would launch
        for windows of n samples: m_best (step 1, step 2), best_frequency (spectrum, update), one otherwise.  `params`
        are the op's int parameters in the order periodhip.h lists for ph_plan_info.  Nothing runs on the device."""
        prm = np.ascontiguousarray(np.asarray(params, dtype=np.int32).reshape(-1))
        out = np.zeros(_ffi.PH_PLAN_LEN, dtype=np.int32)
        _ffi.check(self._lib.ph_plan_info(self._ctx, self._PLAN_OPS[op], _NP_DTYPES[np.dtype(dtype)], int(n),
                                          prm.ctypes.data if prm.size else None, int(prm.size), self._flags(trunc, orth),
                                          out.ctypes.data))
        recs = []
        for k in range(int(out[_ffi.PH_PLAN_KERNELS])):
            r = out[_ffi.PH_PLAN_K0 + k * _ffi.PH_PLAN_STRIDE:][:_ffi.PH_PLAN_STRIDE]
            recs.append(KernelPlan(*(int(v) for v in r)))
        return tuple(recs)

    def qo_fit_feasible(self, kcap, max_period, n=None, window=False) -> bool:
        """Whether ph_qo_fit / ph_ramanujan_fit -- with ``window=True`` ph_qo_fit_win on windows of `n` samples -- can run
        dictionaries of `kcap` rows with periods up to `max_period`: the answer of the plan query (the launch's own
        planning function), nothing runs and nothing is raised."""
        prm = np.array([int(kcap), int(max_period)], dtype=np.int32)
        out = np.zeros(_ffi.PH_PLAN_LEN, dtype=np.int32)
        op = _ffi.PH_OP_QO_FIT_WIN if window else _ffi.PH_OP_QO_FIT
        rc = self._lib.ph_plan_info(self._ctx, op, _ffi.PH_F64, max(1, int(max_period if n is None else n)), prm.ctypes.data,
                                    2, 0, out.ctypes.data)
        if rc not in (_ffi.PH_OK, _ffi.PH_E_ARG):
            _ffi.check(rc)
        return rc == _ffi.PH_OK

    def qo_fit(self, x, periods, n_periods=None, kcap=512, max_period=None, window=None):
        """Fit given period lists to a batch (QOPeriods.compute_reconstruction / get_subspaces + solve_quadratic,
        natural basis): -> keeps (W, pcap) i32, weights (W, kcap) f64, residual (W, N), status (W).
        `window`: None (ph_qo_fit) or one float64 analysis window of N samples for the whole batch (ph_qo_fit_win,
        solve_quadratic's ``window=``); with torch input a float64 tensor on x's device.
        `periods`: one 1-D list shared by all windows, or a (W, pcap) int32 array with `n_periods` (W) entries used per
        row (default: all pcap).  With torch input both are int32 tensors on x's device (n_periods required for 2-D
        lists) and `max_period` should be given (default N); for numpy it defaults to the largest entry."""
        x, code, W, N, fl, mk = self._prep(x)
        per = _side(mk, x, periods, np.int32, "periods")
        if mk.torch:
            if n_periods is None:
                n_periods = mk._t.full((W if per.dim() == 2 else 1,), per.shape[-1], dtype=mk._t.int32, device=x.device)
            npr = _side(mk, x, n_periods, np.int32, "n_periods")
            ndim, shape = per.dim(), tuple(per.shape)
            if max_period is None:
                max_period = N
        else:
            if per.shape[-1] == 0:  # an empty list still needs one readable entry
                per = np.zeros(per.shape[:-1] + (1,), dtype=np.int32)
                n_periods = np.zeros(W if per.ndim == 2 else 1, dtype=np.int32)
            if n_periods is None:
                n_periods = np.full(W if per.ndim == 2 else 1, per.shape[-1], dtype=np.int32)
            npr = _side(mk, x, np.atleast_1d(n_periods), np.int32, "n_periods")
            ndim, shape = per.ndim, per.shape
            if max_period is None:
                max_period = max(1, int(per.max()))
        if ndim not in (1, 2) or (ndim == 2 and shape[0] != W) or npr.shape[0] != (W if ndim == 2 else 1):
            raise ValueError("periods must be one list or (W, pcap), n_periods (W,) or (1,)")
        pcap = int(shape[-1])
        keeps = mk.empty((W, pcap), np.int32)
        weights = mk.empty((W, int(kcap)), np.float64)
        resid = mk.empty((W, N), self._np_dtype(code))
        status = mk.empty((W,), np.int32)
        if window is None:
            self._call(mk, W, self._lib.ph_qo_fit, mk.addr(x), code, W, N, mk.addr(per), mk.addr(npr), pcap,
                       pcap if ndim == 2 else 0, int(max_period), int(kcap), fl, mk.addr(keeps), mk.addr(weights),
                       mk.addr(resid), mk.addr(status))
            return keeps, weights, resid, status
        win = self._window(mk, x, window, N)
        self._call(mk, W, self._lib.ph_qo_fit_win, mk.addr(x), code, W, N, mk.addr(win), mk.addr(per), mk.addr(npr), pcap,
                   pcap if ndim == 2 else 0, int(max_period), int(kcap), fl, mk.addr(keeps), mk.addr(weights),
                   mk.addr(resid), mk.addr(status))
        return keeps, weights, resid, status

    def ramanujan_fit(self, x, q_lo=2, q_hi=None, thresh=0.2, pcap=64, kcap=512):
        """RamanujanPeriods.find_periods_with_weights (default test function) for a batch, three kernels on one stream:
        -> norms (W, q_hi+1) f64, periods (W, pcap) i32 ascending, counts (W) i32 (may exceed pcap: PH_ST_CAP),
        keeps (W, pcap) i32, weights (W, kcap) f64, residual (W, N), status (W)."""
        x, code, W, N, fl, mk = self._prep(x)
        if not q_hi:
            q_hi = N // 3
        q_hi, pcap, kcap = int(q_hi), int(pcap), int(kcap)
        norms = mk.empty((W, q_hi + 1), np.float64)
        periods = mk.empty((W, pcap), np.int32)
        counts = mk.empty((W,), np.int32)
        keeps = mk.empty((W, pcap), np.int32)
        weights = mk.empty((W, kcap), np.float64)
        resid = mk.empty((W, N), self._np_dtype(code))
        status = mk.empty((W,), np.int32)
        self._call(mk, W, self._lib.ph_ramanujan_fit, mk.addr(x), code, W, N, int(q_lo), q_hi, float(thresh), pcap, kcap, fl,
                   mk.addr(norms), mk.addr(periods), mk.addr(counts), mk.addr(keeps), mk.addr(weights), mk.addr(resid),
                   mk.addr(status))
        return norms, periods, counts, keeps, weights, resid, status

    def ramanujan_select(self, norms, thresh, ref=None, pcap=64):
        """The threshold of ramanujan_fit on given norms (W, q_hi + 1) float64, against a choosable level and capped
        (ph_ramanujan_select, one launch): -> periods (W, pcap) i32, counts (W) i32, over (W) i32.
        Candidates of row w are the q with norms[w, q] / m > thresh, m = ref[w] or -- `ref` None -- |max| of the row as
        numpy.max sees it; over[w] counts them.  At most `pcap` are kept: the largest norms, ties to the smaller
        period; counts[w] = min(over[w], pcap) and periods[w, :counts[w]] lists them ascending, zeros behind.
        `ref`: None or W float64 levels.  numpy in, numpy out; a float64 tensor on the engine's device (then `ref` is a
        float64 tensor there too) gives tensors on torch's current stream."""
        x, code, W, n, fl, mk = self._prep(norms if _is_torch(norms) else np.asarray(norms, dtype=np.float64))
        if code != _ffi.PH_F64:
            raise TypeError("norms must be float64")
        rf = None
        if ref is not None:
            rf = _side(mk, x, ref, np.float64, "ref", "norms")
            if tuple(rf.shape) != (W,):
                raise ValueError("ref must hold one level per row")
        pcap = int(pcap)
        periods = mk.empty((W, max(pcap, 0)), np.int32)
        counts = mk.empty((W,), np.int32)
        over = mk.empty((W,), np.int32)
        self._call(mk, W, self._lib.ph_ramanujan_select, mk.addr(x), W, n - 1, float(thresh), mk.addr(rf), pcap, fl,
                   mk.addr(periods), mk.addr(counts), mk.addr(over))
        return periods, counts, over

    def orth_powers(self, x, max_p=None, normalize=False, want_autocorr=False, want_eq3=False):
        """Orthogonal period powers (QOPeriods.get_best_period_orthogonal(return_powers=True)).
        -> pows (W, max_p) [, autocorr (W, N)] [, eq3 (W, max_p)]."""
        x, code, W, N, fl, mk = self._prep(x)
        if max_p is None:
            max_p = N // 2
        max_p = int(max_p)
        pows = mk.empty((W, max_p), np.float64)
        ac = mk.empty((W, N), np.float64) if want_autocorr else None
        e3 = mk.empty((W, max_p), np.float64) if want_eq3 else None
        self._call(mk, W, self._lib.ph_orth_powers, mk.addr(x), code, W, N, max_p, 1 if normalize else 0, fl,
                   mk.addr(ac), mk.addr(e3), mk.addr(pows))
        out = (pows,)
        if want_autocorr:
            out += (ac,)
        if want_eq3:
            out += (e3,)
        return out if len(out) > 1 else pows

    def qo_orth_select(self, x, max_p, trunc=False, want_powers=False):
        """The selection step of QOPeriods.find_periods under orthogonal selection for a batch of residuals, one launch:
        -> period (W) i32 = argmax of the normalised orthogonal powers over q < max_p (0 -> 1), norm (W) f64 =
        periodic_norm(project(x[w], period, trunc, orthogonalize=True), period), status (W) i32 (PH_ST_NO_PERIOD: a
        power or the norm is not finite) [, powers (W, max_p) f64 when want_powers]."""
        x, code, W, N, fl, mk = self._prep(x)
        max_p = int(max_p)
        keep = self._orth(True, max(max_p - 1, 1))
        period = mk.empty((W,), np.int32)
        norm = mk.empty((W,), np.float64)
        status = mk.empty((W,), np.int32)
        pows = mk.empty((W, max(max_p, 0)), np.float64) if want_powers else None
        self._call(mk, W, self._lib.ph_qo_orth_select, mk.addr(x), code, W, N, max_p, keep[2], keep[3], keep[4],
                   fl | (_ffi.PH_FLAG_TRUNC if trunc else 0), mk.addr(period), mk.addr(norm), mk.addr(pows), mk.addr(status))
        return (period, norm, status, pows) if want_powers else (period, norm, status)

    def qo_get_periods(self, periods, rows, counts, weights, max_period=None, ccap=None):
        """QOPeriods.get_periods for a batch of fitted dictionaries, one launch (ph_qo_get_periods):
        -> out (W, ccap) f64 -- segment a of row w (periods[w, a] doubles) starts at sum(periods[w, :a]), zeros behind
        the last -- and status (W) i32.
        `periods`, `rows` (W, pcap) int32: the blocks of every dictionary in order, `counts` (W) how many of them are
        used; `weights` (W, kcap) float64, block a of row w at sum(rows[w, :a]).  numpy arrays, or torch tensors on the
        engine's device (on torch's current stream; outputs are then tensors): the periods, keeps, counts[:, 1] and
        weights of qo_find_periods / qo_fit can be passed on as they are (with update_weights=False a keeps entry of 0
        means `period` rows and has to be replaced first).  `ccap` defaults to the largest sum of periods of the batch
        and `max_period` to the largest period (numpy) or ccap (torch); computing ccap from device tensors reads one
        word back, so pass it to stay asynchronous."""
        wts, code, W, kcap, fl, mk = self._prep(weights if _is_torch(weights) else np.asarray(weights, dtype=np.float64))
        per, rws, cnt = (_side(mk, wts, a, np.int32, "periods, rows and counts", "weights", joint=True)
                         for a in (periods, rows, counts))
        if mk.torch:
            t = mk._t
            shapes = tuple(per.shape), tuple(rws.shape), tuple(cnt.shape)
            if ccap is None:
                used = t.arange(per.shape[1], device=per.device)[None, :] < cnt[:, None]
                ccap = max(1, int((per.clamp(min=0).to(t.int64) * used).sum(dim=1).max().item())) if W else 1
            if max_period is None:
                max_period = min(int(ccap), 1 << 20)
        else:
            shapes = per.shape, rws.shape, cnt.shape
            if per.ndim == 2 and per.shape == rws.shape and cnt.shape == (W,):
                used = np.arange(per.shape[1])[None, :] < cnt[:, None]
                if ccap is None:
                    ccap = max(1, int((np.clip(per, 0, None).astype(np.int64) * used).sum(axis=1).max())) if W else 1
                if max_period is None:
                    max_period = int(min(max(1, (per * used).max() if per.size else 1), 1 << 20))
        if code != _ffi.PH_F64:
            raise TypeError("weights must be float64")
        if len(shapes[0]) != 2 or shapes[0] != shapes[1] or shapes[0][0] != W or shapes[2] != (W,) or shapes[0][1] < 1:
            raise ValueError("periods and rows must be (W, pcap) with pcap >= 1, counts (W,), weights (W, kcap)")
        pcap, ccap = int(shapes[0][1]), int(ccap)
        out = mk.empty((W, ccap), np.float64)
        status = mk.empty((W,), np.int32)
        self._call(mk, W, self._lib.ph_qo_get_periods, mk.addr(per), mk.addr(rws), mk.addr(cnt), W, pcap, mk.addr(wts),
                   int(kcap), int(max_period), ccap, fl, mk.addr(out), mk.addr(status))
        return out, status

    # ------------------------------------------------------------------ short-time framing
    def _dtype_code(self, mk, dtype, default):
        """PH_F64 / PH_F32 for a numpy or torch dtype (None: `default`)."""
        if dtype is None:
            return default
        if mk.torch and isinstance(dtype, mk._t.dtype):
            code = {mk._t.float64: _ffi.PH_F64, mk._t.float32: _ffi.PH_F32}.get(dtype)
        else:
            code = _NP_DTYPES.get(np.dtype(dtype))
        if code is None:
            raise TypeError(f"unsupported dtype {dtype}")
        return code

    def frames(self, signal, frame_length, hop, count=None, window=None, out_dtype=None):
        """Cut a 1-D signal of L samples into overlapping frames (ph_frames, one launch): -> (W, frame_length) with
        frames[f, i] = signal[f * hop + i] * window[i], zero behind the end of the signal, in `out_dtype` (default: the
        signal's).  `count` = W; default 1 + ceil((L - frame_length) / hop) (the last frame zero-padded), 1 when the
        signal is shorter than a frame.  `window`: None or frame_length float64 samples (with torch input a float64
        tensor on the signal's device).  A numpy signal is uploaded once (L elements) and numpy frames come back; a
        torch tensor on the engine's device gives a tensor, on torch's current stream."""
        if getattr(signal, "ndim", None) != 1:
            raise ValueError("expected a 1-D signal")
        x, code, _, L, fl, mk = self._prep(signal.reshape(1, -1))
        N, hop = int(frame_length), int(hop)
        if count is None:
            if N < 1 or hop < 1:
                raise ValueError("frame_length and hop must be >= 1")
            count = 1 + -((N - L) // hop) if L >= N else 1
        W = int(count)
        if W < 0:
            raise ValueError("count must be >= 0")
        ocode = self._dtype_code(mk, out_dtype, code)
        win = None if window is None else self._window(mk, x, window, N)
        out = mk.empty((W, N), self._np_dtype(ocode))
        self._call(mk, W, self._lib.ph_frames, mk.addr(x), code, L, N, hop, W, mk.addr(win), ocode, fl, mk.addr(out))
        return out

    def _ola_args(self, y, hop, length, counts, win_a, win_s):
        """What overlap_add and overlap_add_tracks share: -> (x, code, W, K, N, hop, L, flags, out-factory, counts,
        win_a, win_s), y flattened to (W, K * N) and the optional arrays checked against it."""
        if getattr(y, "ndim", None) not in (2, 3):
            raise ValueError("expected y of shape (W, N) or (W, K, N)")
        K, N = (1, y.shape[1]) if y.ndim == 2 else (y.shape[1], y.shape[2])
        if int(length) < 0:
            raise ValueError("length must be >= 0")
        x, code, W, _, fl, mk = self._prep(y.reshape(y.shape[0], K * N))
        return (x, code, W, K, N, int(hop), int(length), fl, mk) + self._ola_sides(mk, x, W, N, counts, win_a, win_s, "y")

    def _ola_sides(self, mk, x, W, N, counts, win_a, win_s, of):
        """The per-frame counts (None: all) and the two windows (None: all ones) of an overlap-add, checked against x."""
        cnt = None
        if counts is not None:
            cnt = _side(mk, x, counts, np.int32, "counts", of)
            if tuple(cnt.shape) != (W,):
                raise ValueError("counts must hold one entry per frame")
        wa = None if win_a is None else self._window(mk, x, win_a, N)
        ws = None if win_s is None else self._window(mk, x, win_s, N)
        return cnt, wa, ws

    def _ola_call(self, mk, shape, W, L, fn, *args, fl, normalize, out=None):
        """The float64 result of an overlap-add, a new array or `out`: one call of `fn` (flags and result last), or zeros
        when W or L is 0."""
        if out is None:
            out = mk.empty(shape, np.float64)
        if W == 0 or L == 0:
            out[...] = 0.0
            return out
        self._call(mk, W, fn, *args, fl | (_ffi.PH_FLAG_OLA_NORM if normalize else 0), mk.addr(out))
        return out

    def overlap_add(self, y, hop, length, counts=None, win_a=None, win_s=None, normalize=True):
        """Overlap-add a framed result (ph_overlap_add, one launch): y (W, N) or (W, K, N) -> (length,) float64,
        out[n] = sum over the frames f covering n and the rows k < counts[f] (default: all K) of
        win_s[n - f hop] * y[f, k, n - f hop]; with `normalize` divided by sum_f win_a * win_s where that is > 0 and
        exactly 0.0 elsewhere.  `counts` (W) int32, `win_a` / `win_s` (N) float64 or None (all ones): numpy arrays, or
        with torch input tensors on y's device."""
        x, code, W, K, N, hop, L, fl, mk, cnt, wa, ws = self._ola_args(y, hop, length, counts, win_a, win_s)
        return self._ola_call(mk, (L,), W, L, self._lib.ph_overlap_add, mk.addr(x), code, W, K, N, hop, L, mk.addr(cnt),
                              mk.addr(wa), mk.addr(ws), fl=fl, normalize=normalize)

    def overlap_add_tracks(self, y, masks, hop, length, counts=None, win_a=None, win_s=None, normalize=True):
        """Routed overlap-add (ph_overlap_add_tracks, one launch): y (W, N) or (W, K, N), K <= 64 -> (T, length) float64,
        out[t, n] = what overlap_add gives for the rows k < counts[f] of frame f whose bit k is set in masks[t, f].
        `masks` (T, W): np.uint64 or np.int64 (the same bits), or with torch input a torch.int64 tensor on y's device;
        masks may overlap, a row in no mask is never read.  `counts`, `win_a`, `win_s`, `normalize` as in overlap_add."""
        x, code, W, K, N, hop, L, fl, mk, cnt, wa, ws = self._ola_args(y, hop, length, counts, win_a, win_s)
        msk = _masks(mk, x, masks, W, "y")
        T = int(msk.shape[0])
        return self._ola_call(mk, (T, L), W, L, self._lib.ph_overlap_add_tracks, mk.addr(x), code, W, K, N, hop, L,
                              mk.addr(cnt), mk.addr(msk), T, mk.addr(wa), mk.addr(ws), fl=fl, normalize=normalize)

    def overlap_add_periodic(self, seg, periods, counts, masks, frame_length, hop, length, win_a=None, win_s=None,
                             normalize=True):
        """Routed overlap-add of periodic segments (ph_overlap_add_periodic, one launch): -> (T, length) float64,
        out[t, n] = what overlap_add_tracks gives for the blocks of `seg` tiled to `frame_length` samples, without the
        tiled (W, K, N) array.  `seg` (W, ccap) float64 and `periods` (W, pcap <= 64) int32 as qo_get_periods takes and
        returns them (block a of frame f is periods[f, a] doubles at sum(periods[f, :a])), `counts` (W) int32 blocks in
        use, `masks` (T, W) np.uint64 / np.int64 or a torch.int64 tensor: bit a of masks[t, f] routes block a of frame f
        to track t.  A frame's blocks from the first with a period < 1 or running past ccap on contribute nothing.
        numpy arrays, or torch tensors on the engine's device (on torch's current stream; the result is then a tensor);
        `win_a` / `win_s` (frame_length) float64 or None, `normalize` as in overlap_add."""
        N, hop, L = int(frame_length), int(hop), int(length)
        if L < 0:
            raise ValueError("length must be >= 0")
        if getattr(seg, "ndim", None) != 2:
            raise ValueError("expected seg of shape (W, ccap)")
        x, code, W, ccap, fl, mk = self._prep(seg)
        if code != _ffi.PH_F64:
            raise TypeError("seg must be float64")
        per = _side(mk, x, periods, np.int32, "periods", "seg")
        if per.ndim != 2 or per.shape[0] != W or per.shape[1] < 1:
            raise ValueError("periods must be (W, pcap) with pcap >= 1")
        pcap = int(per.shape[1])
        if pcap > 64:
            raise ValueError(f"pcap={pcap} blocks per frame do not fit a 64-bit mask")
        cnt = _side(mk, x, counts, np.int32, "counts", "seg")  # (not optional here: None is refused like any non-array)
        cnt, wa, ws = self._ola_sides(mk, x, W, N, cnt, win_a, win_s, "seg")
        msk = _masks(mk, x, masks, W, "seg")
        T = int(msk.shape[0])
        return self._ola_call(mk, (T, L), W, L, self._lib.ph_overlap_add_periodic, mk.addr(x), mk.addr(per), mk.addr(cnt),
                              mk.addr(msk), W, pcap, int(ccap), T, N, hop, L, mk.addr(wa), mk.addr(ws), fl=fl,
                              normalize=normalize)

    def _ola_acc(self, mk, x, acc, name, of):
        """The running sum of a blocked overlap-add, (L,) or (T, L) float64, as the library writes it in place: a
        C-contiguous numpy array, or with torch input a contiguous float64 tensor on x's device.  -> (T, L)."""
        if mk.torch:
            if not _is_torch(acc) or acc.dtype != mk._t.float64 or acc.device != x.device:
                raise TypeError(f"{name} must be a float64 tensor on the device of {of}")
            ok = acc.is_contiguous()
        else:
            if not isinstance(acc, np.ndarray) or acc.dtype != np.float64:
                raise TypeError(f"{name} must be a float64 array")
            ok = acc.flags.c_contiguous and acc.flags.writeable
        if acc.ndim not in (1, 2) or not ok:
            raise ValueError(f"{name} must be contiguous (and writable), of shape (L,) or (T, L)")
        return (1, int(acc.shape[0])) if acc.ndim == 1 else (int(acc.shape[0]), int(acc.shape[1]))

    def overlap_add_block(self, y, hop, length, first_frame, acc, counts=None, masks=None, win_s=None):
        """One block of a blocked overlap-add (ph_overlap_add_block, one launch): adds the frames first_frame ..
        first_frame + Wb - 1 of a recording of `length` samples, y (Wb, N) or (Wb, K, N), into `acc` in place and returns
        it.  `acc` (length,) or (1, length) float64 without `masks`; with `masks` (T, Wb) -- block-local, as
        overlap_add_tracks takes them, K <= 64 -- (T, length).  `counts` (Wb) int32, `win_s` (N) float64 or None.  numpy
        arrays, or torch tensors on the engine's device (on torch's current stream); acc is of y's kind.
        Zero acc before the first block, apply the blocks in ascending first_frame, every frame in exactly one block:
        overlap_add_finish then gives, bit for bit, what overlap_add (no masks) or overlap_add_tracks gives for all frames
        at once.  Only the samples the block's frames cover are read and written."""
        x, code, W, K, N, hop, L, fl, mk, cnt, _, ws = self._ola_args(y, hop, length, counts, None, win_s)
        T, La = self._ola_acc(mk, x, acc, "acc", "y")
        msk = None if masks is None else _masks(mk, x, masks, W, "y")
        if La != L or T != (1 if msk is None else int(msk.shape[0])):
            raise ValueError("acc must be (length,) without masks and (T, length) with masks (T, Wb)")
        self._call(mk, W, self._lib.ph_overlap_add_block, mk.addr(x), code, W, K, N, hop, L, int(first_frame), mk.addr(cnt),
                   mk.addr(msk), T, mk.addr(ws), fl, mk.addr(acc))
        return acc

    def overlap_add_finish(self, acc, frame_length, hop, frames, win_a=None, win_s=None, normalize=True, out=None):
        """The end of a blocked overlap-add (ph_overlap_add_finish, one launch): acc (L,) or (T, L) float64, the running sum
        of overlap_add_block over all `frames` frames of the recording -> the same shape, acc divided by the overlap-added
        window product of those frames where that is > 0 and exactly 0.0 elsewhere (`normalize` False: acc as it is).
        `out`: None (a new array) or an array of acc's kind and shape, acc itself included.  `win_a` / `win_s` as in
        overlap_add."""
        N, hop, W = int(frame_length), int(hop), int(frames)
        if W < 0:
            raise ValueError("frames must be >= 0")
        if _is_torch(acc):
            x, _, _, _, fl, mk = self._prep(acc.reshape(1, -1) if acc.dim() == 1 else acc)
        else:
            fl, mk = 0, _Out(acc)
            x = acc
        T, L = self._ola_acc(mk, x, acc, "acc", "acc")
        if out is not None and (self._ola_acc(mk, x, out, "out", "acc") != (T, L) or out.ndim != acc.ndim):
            raise ValueError("out must have the shape of acc")
        _, wa, ws = self._ola_sides(mk, x, W, N, None, win_a, win_s, "acc")
        return self._ola_call(mk, tuple(acc.shape), W, L, self._lib.ph_overlap_add_finish, mk.addr(acc), T, N, hop, L, W,
                              mk.addr(wa), mk.addr(ws), fl=fl, normalize=normalize, out=out)

    # ------------------------------------------------------------------ best path through a time-period map
    def period_path_plan(self, P):
        """-> (threads per workgroup, LDS bytes, rows of one backtrace tile) of the k_period_path launch for a map of P
        columns (ph_period_path_plan_info).  Nothing runs on the device."""
        block, lds, tile = C.c_int(0), C.c_int(0), C.c_int(0)
        _ffi.check(self._lib.ph_period_path_plan_info(self._ctx, int(P), C.byref(block), C.byref(lds), C.byref(tile)))
        return block.value, lds.value, tile.value

    def period_path(self, cost, band=8, jump=0.0, want_values=True):
        """The best path through a time-period map (ph_period_path, one launch): cost (W, P) or (R, W, P) float64 ->
        (path, values, score, status).  The path maximises the sum of cost[f, path[f]] minus jump * |path[f] - path[f-1]|
        over the paths that move at most `band` columns per frame; entries that are not finite are forbidden.  path
        (W,) int32, values (W,) float64 = cost[f, path[f]] (None without `want_values`), score a float64 and status an
        int32 scalar array; with a batch every result has the leading dimension R.  status PH_ST_NO_PERIOD: some frame has
        no reachable state, the path is all -1 and the values 0.
        A numpy array gives numpy results; a float64 tensor on the engine's device gives tensors, on torch's current
        stream.  The last dimension must be contiguous; a strided last-but-one dimension (a column slice of a wider
        map) is passed on as the row stride and not copied, anything else is."""
        if getattr(cost, "ndim", None) not in (2, 3):
            raise ValueError("expected cost of shape (W, P) or (R, W, P)")
        batched = cost.ndim == 3
        R, W, P = (int(v) for v in (cost.shape if batched else (1,) + tuple(cost.shape)))
        band = int(band)
        jump = float(jump)
        if _is_torch(cost):
            import torch

            if not cost.is_cuda or cost.device.index != self.device:
                raise ValueError(f"torch input must live on cuda:{self.device} (or pass a numpy array)")
            if cost.dtype != torch.float64:
                raise TypeError("cost must be float64")
            strides, fl = tuple(cost.stride()), _ffi.PH_FLAG_DEVICE
            mk = _Out(cost)
            mk.stream = torch.cuda.current_stream(cost.device).cuda_stream or _ffi.PH_STREAM_DEFAULT
        else:
            cost = np.asarray(cost)
            if cost.dtype != np.float64:
                raise TypeError("cost must be float64")
            strides, fl = tuple(s // 8 if s % 8 == 0 else -1 for s in cost.strides), 0
            mk = _Out(cost)
        ld = strides[-2] if W > 1 else max(P, 1)
        ok = P >= 1 and W >= 1 and (strides[-1] == 1 or P == 1) and ld >= P and (not batched or R <= 1 or strides[0] == W * ld)
        if not ok and P >= 1 and W >= 1:
            cost, ld = (cost.contiguous() if mk.torch else np.ascontiguousarray(cost)), P
        lead = (R,) if batched else ()
        path = mk.empty((R, W), np.int32)
        values = mk.empty((R, W), np.float64) if want_values else None
        score = mk.empty((R,), np.float64)
        status = mk.empty((R,), np.int32)
        if R > 0:
            self._call(mk, R, self._lib.ph_period_path, mk.addr(cost), R, W, P, int(ld), band, jump, fl, mk.addr(path),
                       mk.addr(values), mk.addr(score), mk.addr(status))
        return (path.reshape(lead + (W,)), None if values is None else values.reshape(lead + (W,)), score.reshape(lead),
                status.reshape(lead))

    # ------------------------------------------------------------------ extraction along a period track
    def follow_plan(self, n):
        """-> (threads per workgroup, LDS bytes, placement) of the k_follow launch for frames of n samples
        (ph_follow_plan_info); placement is PH_PLAN_LDS or PH_PLAN_HBM: where the residual frame and the period of means
        live.  Nothing runs on the device."""
        block, lds, placement = C.c_int(0), C.c_int(0), C.c_int(0)
        _ffi.check(self._lib.ph_follow_plan_info(self._ctx, int(n), C.byref(block), C.byref(lds), C.byref(placement)))
        return block.value, lds.value, placement.value

    def follow(self, signal, frame_length, hop, count, periods, counts, ccap, window=None, frame_dtype=None, trunc=False,
               seg=None):
        """The periodic components of a recording along per-frame periods (ph_follow, one launch): the frames of
        ``frames(signal, frame_length, hop, count, window, frame_dtype)`` are cut inside the kernel -- no (W, N) array
        exists -- and from frame f the projections onto periods[f, 0], periods[f, 1], ... are peeled one after the
        other (``Periods.project(residual, p, trunc, False, return_single_period=True)``, then the subtraction).
        -> (seg, powers, done): seg (W, ccap) float64 holds one period of every block, block a of frame f at
        sum(periods[f, :a]) -- the layout qo_get_periods returns and overlap_add_periodic takes; powers (W, pcap) float64
        the drop of the residual's periodic norm per block over the frame's norm, 0.0 behind done; done (W,) int32 the
        blocks written.  A frame's walk ends at counts[f] blocks (clipped to 0 .. pcap) or at the first period < 1,
        > frame_length or running past ccap; the elements of seg behind a frame's last block are never written (`seg`:
        an existing (W, ccap) float64 array of the signal's kind to write into, None for a new one).
        `periods` (W, pcap <= 64) and `counts` (W) int32, `window` None or frame_length float64 samples: numpy arrays,
        or with a tensor signal tensors on its device (on torch's current stream; the results are then tensors).
        `frame_dtype`: None (the signal's), float64 or float32 -- the dtype the frame is rounded to."""
        if getattr(signal, "ndim", None) != 1:
            raise ValueError("expected a 1-D signal")
        x, code, _, L, fl, mk = self._prep(signal.reshape(1, -1))
        N, hop, W, ccap = int(frame_length), int(hop), int(count), int(ccap)
        if W < 0:
            raise ValueError("count must be >= 0")
        fcode = self._dtype_code(mk, frame_dtype, code)
        per = _side(mk, x, periods, np.int32, "periods", "signal")
        if per.ndim != 2 or per.shape[0] != W or per.shape[1] < 1:
            raise ValueError("periods must be (W, pcap) with pcap >= 1")
        pcap = int(per.shape[1])
        cnt = _side(mk, x, counts, np.int32, "counts", "signal")
        if tuple(cnt.shape) != (W,):
            raise ValueError("counts must hold one entry per frame")
        win = None if window is None else self._window(mk, x, window, N)
        if seg is None:
            seg = mk.empty((W, max(ccap, 0)), np.float64)
        else:
            if _is_torch(seg) != mk.torch or (mk.torch and (seg.dtype != mk._t.float64 or seg.device != x.device)) or (
                    not mk.torch and (not isinstance(seg, np.ndarray) or seg.dtype != np.float64)):
                raise TypeError("seg must be a float64 array of the signal's kind, on its device")
            ok = seg.is_contiguous() if mk.torch else (seg.flags.c_contiguous and seg.flags.writeable)
            if tuple(seg.shape) != (W, ccap) or not ok:
                raise ValueError("seg must be contiguous (and writable), of shape (W, ccap)")
        powers = mk.empty((W, pcap), np.float64)
        done = mk.empty((W,), np.int32)
        self._call(mk, W, self._lib.ph_follow, mk.addr(x), code, L, N, hop, W, mk.addr(win), fcode, mk.addr(per),
                   mk.addr(cnt), pcap, ccap, fl | (_ffi.PH_FLAG_TRUNC if trunc else 0), mk.addr(seg), mk.addr(powers),
                   mk.addr(done))
        return seg, powers, done

    def follow_residual(self, signal, frame_length, hop, first, count, periods, counts, window=None, frame_dtype=None,
                        trunc=False):
        """The frames of a recording less the tracks named for them (ph_follow_residual, one launch of
        k_follow_residual): -> (count, frame_length) float64, row i what `follow` leaves of frame ``first + i`` after
        peeling periods[i, 0], periods[i, 1], ... -- the same cut, means and subtractions, bit for bit -- so
        ``frames(...)[first + i]`` widened to double minus the tiled blocks `follow` writes to seg, in order.  A row's
        walk ends at counts[i] blocks (clipped to 0 .. pcap) or at the first period < 1 or > frame_length; there is no
        ccap.  `periods` (count, pcap <= 64) and `counts` (count) int32 are local to the block of frames; both None (or
        pcap == 0): no tracks, the float64 frames themselves.  `window`, `frame_dtype`, `trunc` and the kinds of array
        as in `follow`."""
        if getattr(signal, "ndim", None) != 1:
            raise ValueError("expected a 1-D signal")
        x, code, _, L, fl, mk = self._prep(signal.reshape(1, -1))
        N, hop, f0, W = int(frame_length), int(hop), int(first), int(count)
        if W < 0:
            raise ValueError("count must be >= 0")
        fcode = self._dtype_code(mk, frame_dtype, code)
        if (periods is None) != (counts is None):
            raise ValueError("periods and counts come together (both None: no tracks)")
        per = cnt = None
        pcap = 0
        if periods is not None:
            per = _side(mk, x, periods, np.int32, "periods", "signal")
            if per.ndim != 2 or per.shape[0] != W:
                raise ValueError("periods must be (count, pcap)")
            pcap = int(per.shape[1])
            cnt = _side(mk, x, counts, np.int32, "counts", "signal")
            if tuple(cnt.shape) != (W,):
                raise ValueError("counts must hold one entry per frame")
            if pcap == 0:
                per = cnt = None
        win = None if window is None else self._window(mk, x, window, N)
        out = mk.empty((W, max(N, 0)), np.float64)
        self._call(mk, W, self._lib.ph_follow_residual, mk.addr(x), code, L, N, hop, f0, W, mk.addr(win), fcode,
                   mk.addr(per), mk.addr(cnt), pcap, fl | (_ffi.PH_FLAG_TRUNC if trunc else 0), mk.addr(out))
        return out

    def fold_sums(self, x, p_list, keep):
        """W = A x for natural-basis rows (QOPeriods.py:782): (W, sum(keep)) float64."""
        x, code, W, N, fl, mk = self._prep(x)
        pl, pl_addr = _i32(np.atleast_1d(p_list))
        kp, kp_addr = _i32(np.atleast_1d(keep))
        out = mk.empty((W, int(kp.sum())), np.float64)
        self._call(mk, W, self._lib.ph_fold_sums, mk.addr(x), code, W, N, pl_addr, kp_addr, pl.size, fl, mk.addr(out))
        return out

    def tile_sum(self, wts, n, p_list, keep, dtype=np.float64):
        """Reconstruction A^T w (QOPeriods.py:795): (W, n)."""
        wts2, code, W, S, fl, mk = self._prep(wts)
        if code != _ffi.PH_F64:
            raise TypeError("weights must be float64")
        pl, pl_addr = _i32(np.atleast_1d(p_list))
        kp, kp_addr = _i32(np.atleast_1d(keep))
        if int(kp.sum()) != S:
            raise ValueError("weights row length must equal sum(keep)")
        ocode = _NP_DTYPES[np.dtype(dtype)]
        out = mk.empty((W, int(n)), self._np_dtype(ocode))
        self._call(mk, W, self._lib.ph_tile_sum, mk.addr(wts2), W, int(n), pl_addr, kp_addr, pl.size, ocode, fl, mk.addr(out))
        return out


_default = None
_default_lock = threading.Lock()


def default_engine() -> PeriodEngine:
    """Process-wide engine on cuda:LOCAL_RANK (one process per GPU)."""
    global _default
    with _default_lock:
        if _default is None:
            _default = PeriodEngine()
        return _default
