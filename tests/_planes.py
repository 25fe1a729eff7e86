"""The hidden spike planes a head pass left in its workspace, and what every output of the pass is as a function of them.

A readout (include/snn_hip.h: any-time readouts) is a pure function of the spike planes of its pass: outputs and time sums are the LI
recursion on the first T' planes, counts are their popcounts, rate rows are quotients of those.  The helpers here read the planes back
(snn_debug_last_rpn_planes / snn_debug_last_det_planes), undo the split and word-major layouts, and restate the recursion in float64 and
the counts in integers - no threshold is involved, so nothing can flip.  tests/test_readouts_cpu.py ties li_fp64 to the oracle and pins
the layout helpers on synthetic buffers."""
import ctypes as C

import numpy as np
import torch

CUR_TOL = 1e-5            # the LI heads' bound of tests/test_gpu_stages.py (fp32 sums of <= 2048 products against fp64)


def li_constants(constants=None):
    """(a, b) = (dt * tau_mem_inv, dt * tau_syn_inv) as fp32 products of 0-dim tensors, the way Norse and ops.make_params form them;
    ``constants`` (oracle.snn_oracle.NeuronConstants) defaults to the reference's dt = 1 ms, 100 / s, 200 / s"""
    if constants is None:
        return float(torch.tensor(0.001) * torch.tensor(100.0)), float(torch.tensor(0.001) * torch.tensor(200.0))
    return (float(torch.tensor(constants.dt) * torch.tensor(constants.tau_mem_inv)),
            float(torch.tensor(constants.dt) * torch.tensor(constants.tau_syn_inv)))


# ---- layouts ------------------------------------------------------------------------------------------------------------------------
def rows_from_split(raw, T: int, P: int, Cw: int, split):
    """the shared LIF's planes as rows [T, P, Cw]: from blocks of four words [T][Cw / 4][P][4] if `split`, else they are rows already"""
    if split:
        return raw.reshape(T, Cw // 4, P, 4).transpose(1, 2).reshape(T, P, Cw)
    return raw.reshape(T, P, Cw)


def rows_from_word_major(raw, T: int, R: int, Hw: int, word_major):
    """lif6's planes as rows [T, R, Hw]: from word-major [T][Hw][R] if `word_major`"""
    if word_major:
        return raw.reshape(T, Hw, R).transpose(1, 2)
    return raw.reshape(T, R, Hw)


def rpn_planes(dev, T, Cw):
    """(raw bytes of the last RPN forward's shared-LIF planes, 1 if they lie in blocks of four words)"""
    from snn_automotive_object_detection_amd import _lib, ops
    off3 = (C.c_uint64 * 3)()
    _lib.load().snn_debug_last_rpn_planes(off3)
    P = int(off3[2])
    return ops._WS.get(dev, 1)[int(off3[0]): int(off3[0]) + T * P * Cw * 4].clone(), int(off3[1])


def det_planes(dev, T, Hd, R):
    """(raw bytes of lif6's planes, of lif7's, 1 if lif6's are word-major) of the last detector forward"""
    from snn_automotive_object_detection_amd import _lib, ops
    off3 = (C.c_uint64 * 3)()
    _lib.load().snn_debug_last_det_planes(off3)
    n = T * ((Hd + 31) // 32) * R * 4
    ws = ops._WS.get(dev, 1)
    return ws[int(off3[0]): int(off3[0]) + n].clone(), ws[int(off3[1]): int(off3[1]) + n].clone(), int(off3[2])


def head_rpn_planes(dev, T, C_):
    """the shared LIF's spike planes the last RPN forward left in the workspace, as rows [T, P, C / 32] (all levels, position-major)"""
    from snn_automotive_object_detection_amd import _lib, ops
    off3 = (C.c_uint64 * 3)()
    _lib.load().snn_debug_last_rpn_planes(off3)
    P, Cw = int(off3[2]), (C_ + 31) // 32
    raw = ops._WS.get(dev, 1)[int(off3[0]): int(off3[0]) + T * P * Cw * 4].view(torch.int32)
    return rows_from_split(raw, T, P, Cw, off3[1]).contiguous().clone()


def head_det_planes(dev, T, Hd, R):
    """lif6 / lif7 spike planes of the last detector forward as rows [T, R, Hd / 32]"""
    p6, p7, wm = det_planes(dev, T, Hd, R)
    Hw = (Hd + 31) // 32
    return rows_from_word_major(p6.view(torch.int32), T, R, Hw, wm).contiguous(), p7.view(torch.int32).view(T, R, Hw)


# ---- what a readout is, from the planes --------------------------------------------------------------------------------------------------
def li_fp64(spk_dense, w, a: float, b: float, li_order: str = "jump_first"):
    """The LI recursion in float64 with the value after EVERY step: spikes {0, 1} [T, M, K], weights [N, K] ->
    (last [T, M, N], running_sum [T, M, N]); row T' - 1 of each is the output / time sum of a T'-step head."""
    spk = np.asarray(spk_dense, dtype=np.float64)
    w = np.asarray(w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else w, dtype=np.float64)
    T, M, K = spk.shape
    cur = (spk.reshape(T * M, K) @ w.T).reshape(T, M, w.shape[0])
    v = np.zeros((M, w.shape[0]))
    i = np.zeros_like(v)
    vsum = np.zeros_like(v)
    last, run = np.empty_like(cur), np.empty_like(cur)
    for t in range(T):
        if li_order == "jump_first":
            i = i + cur[t]; v = v + a * (i - v); i = i - b * i
        elif li_order == "voltage_first":
            v = v + a * (i - v); i = i - b * i + cur[t]
        else:
            raise ValueError(li_order)
        vsum = vsum + v
        last[t], run[t] = v, vsum
    return last, run


def popcounts(planes_rows) -> np.ndarray:
    """spike planes as rows [T, M, W] (int32 words) -> int64 [T, M]: set bits per step and row"""
    a = np.ascontiguousarray(planes_rows.detach().cpu().numpy() if isinstance(planes_rows, torch.Tensor) else planes_rows)
    T, M, W = a.shape
    return np.unpackbits(a.view(np.uint8).reshape(T, M, W * 4), axis=2).sum(axis=2, dtype=np.int64)


def cumulative_popcounts(planes_rows) -> np.ndarray:
    """int64 [T, M]: row T' - 1 = spikes of steps < T' - what a T'-step forward counts"""
    return np.cumsum(popcounts(planes_rows), axis=0)
