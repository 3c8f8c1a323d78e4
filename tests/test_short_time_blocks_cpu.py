"""The two steps decompose_qo and decompose_ramanujan share, without a GPU: ShortTime._rerun_capped (the capacity loop)
under a scripted launch callable whose rows say which attempt wrote them, and ShortTime._pack_back (host results into
the device blocks) against a plain loop.  Both are plain tensor bookkeeping and run on torch CPU tensors."""

import numpy as np
import torch

from pyperiod_amd import ShortTime, _ffi

OK, CAP = _ffi.PH_ST_OK, _ffi.PH_ST_CAP
W = 7


class Scripted:
    """launch(idx, kcap) of _rerun_capped: row f of the first tensor is (f, kcap), row f of the weights kcap times
    1000 f + kcap, so every row names the attempt that wrote it; `script[kcap]` maps a frame to a status other than OK."""

    def __init__(self, script):
        self.script, self.calls, self.returned = script, [], []

    def __call__(self, idx, kcap):
        self.calls.append((None if idx is None else idx.tolist(), kcap))
        frames = np.arange(W) if idx is None else idx.numpy()
        tag = torch.as_tensor(np.stack([frames, np.full(frames.size, kcap)], axis=1).astype(np.int32))
        wts = torch.as_tensor(np.repeat(1000.0 * frames + kcap, kcap).reshape(frames.size, kcap))
        st = torch.as_tensor(np.array([self.script[kcap].get(int(f), OK) for f in frames], dtype=np.int32))
        self.returned.append((tag, wts))
        return tag, wts, st


def zeros():
    return torch.zeros((W, 2), dtype=torch.int32), torch.zeros((W, 1), dtype=torch.float64)


def rerun(capacities, script):
    launch = Scripted(script)
    (tag, wts), st = ShortTime._rerun_capped(torch, torch.device("cpu"), W, capacities, zeros(), launch)
    return launch, tag, wts, st


def test_rerun_runs_only_the_capped_frames_and_keeps_every_finished_row():
    launch, tag, wts, st = rerun([4, 8, 16], {4: {1: CAP, 3: CAP, 6: CAP, 2: 2}, 8: {3: CAP}, 16: {}})
    assert launch.calls == [(None, 4), ([1, 3, 6], 8), ([3], 16)]
    ended_at = [4, 8, 4, 16, 4, 4, 8]  # the attempt that ended each frame; frame 2 (status 2) was never run again
    assert tag.tolist() == [[f, k] for f, k in enumerate(ended_at)]
    assert wts.shape == (W, 16) and wts.dtype == torch.float64
    for f, k in enumerate(ended_at):
        assert np.all(wts[f, :k].numpy() == 1000.0 * f + k) and np.all(wts[f, k:].numpy() == 0.0), f
    assert st.dtype == np.int32 and st.tolist() == [OK, OK, 2, OK, OK, OK, OK]


def test_rerun_adopts_the_tensors_of_a_whole_batch_launch():
    launch, tag, wts, st = rerun([4, 8, 16], {4: {2: 2}})
    assert launch.calls == [(None, 4)]
    assert tag is launch.returned[0][0] and wts is launch.returned[0][1]
    assert st.tolist() == [OK, OK, 2, OK, OK, OK, OK]


def test_rerun_leaves_the_last_attempt_of_a_frame_the_ladder_does_not_finish():
    launch, tag, wts, st = rerun([4], {4: {3: CAP}})
    assert launch.calls == [(None, 4)]
    assert tag[3].tolist() == [3, 4] and np.all(wts[3].numpy() == 3004.0) and wts.shape == (W, 4)
    assert st.tolist() == [OK, OK, OK, CAP, OK, OK, OK]
    launch, tag, wts, st = rerun([4, 8], {4: {3: CAP}, 8: {3: CAP}})
    assert launch.calls == [(None, 4), ([3], 8)]
    assert tag[3].tolist() == [3, 8] and np.all(wts[3].numpy() == 3008.0) and st[3] == CAP


def test_rerun_without_a_capacity_launches_nothing():
    launch, tag, wts, st = rerun([], {})
    assert launch.calls == []
    assert tag.shape == (W, 2) and not tag.any() and wts.shape == (W, 1) and not wts.any()
    assert st.dtype == np.int32 and st.tolist() == [CAP] * W


def test_pack_back_against_a_loop():
    """40 frames, 9 of them unfinished (the first and the last among them): one triple with more blocks than pcap, one
    with more weights than the weights are wide, one empty.  Frames that are not named keep their bits."""
    rng = np.random.default_rng(5)
    Wf, pcap, kcap = 40, 4, 10
    per = rng.integers(1, 30, (Wf, pcap)).astype(np.int32)
    keeps = rng.integers(1, 30, (Wf, pcap)).astype(np.int32)
    nb = rng.integers(0, pcap + 1, Wf).astype(np.int32)
    wts = rng.standard_normal((Wf, kcap))
    wts[1, 2], wts[38, 0] = np.nan, -0.0  # bits, not values, are compared below
    unfinished = np.array([0, 3, 4, 11, 17, 18, 29, 33, 39])
    packed = []
    for j in range(unfinished.size):
        n = int(rng.integers(1, pcap + 1))
        ks = rng.integers(1, 3, n).tolist()
        packed.append((rng.integers(1, 30, n).tolist(), ks, rng.standard_normal(sum(ks))))
    packed[2] = ([5, 7, 9, 11, 13, 15], [1, 1, 1, 1, 1, 1], rng.standard_normal(6))  # 6 blocks > pcap
    packed[5] = ([12, 13], [6, 7], rng.standard_normal(13))  # 13 weights > kcap
    packed[7] = ([], [], np.zeros(0))
    args = tuple(torch.as_tensor(a.copy()) for a in (per, keeps, nb, wts))
    got = ShortTime._pack_back(torch, args, unfinished, packed)
    g_per, g_keeps, g_nb, g_wts = (t.numpy() for t in got)
    assert g_per.shape == g_keeps.shape == (Wf, 6) and g_nb.shape == (Wf,) and g_wts.shape == (Wf, 13)
    assert g_per.dtype == g_keeps.dtype == g_nb.dtype == np.int32 and g_wts.dtype == np.float64
    named = dict(zip(unfinished.tolist(), packed))
    for f in range(Wf):
        if f in named:
            ps, ks, ws = named[f]
            assert g_nb[f] == len(ps), f
            assert g_per[f, : len(ps)].tolist() == ps and not g_per[f, len(ps) :].any(), f
            assert g_keeps[f, : len(ps)].tolist() == ks and not g_keeps[f, len(ps) :].any(), f
            assert np.array_equal(g_wts[f, : ws.size], ws) and not g_wts[f, ws.size :].any(), f
        else:
            assert g_nb[f] == nb[f], f
            assert np.array_equal(g_per[f, :pcap], per[f]) and not g_per[f, pcap:].any(), f
            assert np.array_equal(g_keeps[f, :pcap], keeps[f]) and not g_keeps[f, pcap:].any(), f
            assert g_wts[f, :kcap].tobytes() == wts[f].tobytes() and not g_wts[f, kcap:].any(), f
    # nothing to widen: the tensors are written where they are
    args = tuple(torch.as_tensor(a.copy()) for a in (per, keeps, nb, wts))
    back = ShortTime._pack_back(torch, args, unfinished[:2], packed[:2])
    assert all(a is b for a, b in zip(args, back))
