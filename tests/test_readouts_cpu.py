"""Any-time readouts (one head pass, a readout per T' of a time-step sweep) - what needs no GPU: the C ABI exists and refuses
bad step lists before any device work, and the Python methods refuse them before touching a device."""
import ctypes as C

import pytest
import torch

import snn_automotive_object_detection_amd as S
from snn_automotive_object_detection_amd import _lib, ops
from snn_automotive_object_detection_amd.sweep import timestep_sweep

READOUT_SYMBOLS = ("snn_li_heads_readouts", "snn_rpn_head_forward_readouts", "snn_det_head_forward_readouts",
                   "snn_det_head_forward_roialign_readouts")
BAD_STEPS = [[], [5, 4], [4, 4], [0, 3], [3, 33], [33], list(range(1, 34))]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_symbols_exist(lib):
    for name in READOUT_SYMBOLS:
        assert name in _lib.SYMBOLS
        assert hasattr(lib, name)


def _steps(v):
    return (C.c_int * max(1, len(v)))(*v), len(v)


@pytest.mark.parametrize("bad", BAD_STEPS, ids=lambda v: "steps=%s" % (v if len(v) < 5 else "1..%d" % len(v)))
def test_bad_step_lists_return_minus_one(lib, bad):
    st, n = _steps(bad)
    p = _lib.snn_params(0.1, -0.2, 0.0, 0.0, 0.25, 0.1, 0, 1)
    dummy = C.c_void_p(16)                     # never dereferenced: the step list is checked first
    lv = (_lib.snn_rpn_level * 1)(_lib.snn_rpn_level(16, 1, 4, 4, 0))
    rlv = (_lib.snn_roi_level * 1)(_lib.snn_roi_level(16, 4, 4, 0.25, 0))
    calls = {
        "snn_li_heads_readouts": lambda: lib.snn_li_heads_readouts(dummy, 16, st, n, 16, 64, dummy, 3, 12, C.byref(p), dummy, dummy,
                                                                   None, None, None),
        "snn_rpn_head_forward_readouts": lambda: lib.snn_rpn_head_forward_readouts(lv, 1, 64, 3, st, n, C.byref(p), dummy, dummy, dummy,
                                                                                   dummy, None, None, None, dummy, 1 << 30, None),
        "snn_det_head_forward_readouts": lambda: lib.snn_det_head_forward_readouts(dummy, 16, 64, 64, 9, 36, st, n, C.byref(p), dummy, 0,
                                                                                   dummy, dummy, dummy, dummy, None, None, None, None,
                                                                                   dummy, 1 << 30, None),
        "snn_det_head_forward_roialign_readouts": lambda: lib.snn_det_head_forward_roialign_readouts(
            rlv, 1, 64, dummy, dummy, dummy, 16, 64, 9, 36, st, n, C.byref(p), dummy, 0, dummy, dummy, dummy, dummy, None, None, None,
            None, dummy, 1 << 30, None),
    }
    for name, call in calls.items():
        assert call() == -1, name
        msg = lib.snn_last_error().decode()
        assert name in msg and "step" in msg.lower(), (name, msg)


@pytest.mark.parametrize("bad", BAD_STEPS + [[1.0, 2.0], [True, 2], "12", 12], ids=repr)
def test_check_steps_raises_value_error(bad):
    with pytest.raises(ValueError):
        ops.check_steps(bad)


def test_check_steps_accepts_a_sweep():
    assert ops.check_steps(range(4, 13)) == tuple(range(4, 13))
    assert ops.check_steps([1]) == (1,)
    assert ops.check_steps(list(range(1, 33))) == tuple(range(1, 33))


@pytest.mark.parametrize("bad", [[], [8, 4], [0, 4], [4, 40]], ids=repr)
def test_module_methods_refuse_bad_steps_before_the_device(bad):
    # CPU weights and inputs: any device work would raise SnnHipError, so a ValueError shows the check came first
    rpn = S.RPNHeadSNN(64, 3, 8)
    det = S.FastRCNNPredictorSNNFull(64 * 49, 64, 5, 8)
    feats = [torch.zeros(1, 64, 4, 4)]
    with pytest.raises(ValueError):
        rpn.forward_readouts(feats, bad)
    with pytest.raises(ValueError):
        det.forward_readouts(torch.zeros(3, 64 * 49), bad)
    with pytest.raises(ValueError):
        det.forward_roialign_readouts(feats, [0.25], torch.zeros(3, 5), torch.zeros(3, dtype=torch.int32), bad)
    assert rpn.num_steps == 8 and det.num_steps == 8


def test_sweep_refuses_bad_steps_before_the_device():
    model = S.create_model("cityscapes", 9).eval()
    with pytest.raises(ValueError):
        timestep_sweep(model, [torch.zeros(3, 32, 32)], [4, 40], [8])
    with pytest.raises(ValueError):
        timestep_sweep(model, [torch.zeros(3, 32, 32)], [4], [])


# ---- the references of tests/test_gpu_readouts_planes.py (tests/_planes.py) ------------------------------------------------------------
CUR_TOL = 1e-5                                   # tests/test_gpu_stages.py


@pytest.mark.parametrize("li_order", ["jump_first", "voltage_first"])
@pytest.mark.parametrize("name", ["rpn_c64_A5_T8", "det_K9_T12"])
def test_li_fp64_equals_the_oracle_at_every_step(name, li_order):
    """li_fp64's row T' - 1 is the oracle's LI head (li_last_from_spikes: Norse's cell, fp32) on the first T' steps of the oracle's own
    hidden trace - last membrane and time sum, every T' = 1 .. T: the GPU tests' reference does not rest on an unchecked helper"""
    import numpy as np
    from oracle import fixtures as FX
    from oracle import snn_oracle as OR
    from tests import _planes as PL
    from tests._util import nchw_to_rows
    a, b = PL.li_constants()
    assert PL.CUR_TOL == CUR_TOL
    if name.startswith("rpn"):
        spec = FX.RPN_SPECS[name]
        feats, w_s, w_c, w_b = FX.rpn_inputs(spec)
        with torch.no_grad():
            tr = OR.rpn_head_forward(feats, w_s, w_c, w_b, spec["T"], trace=True)[2]
        cases = [(t["spk"], nchw_to_rows(t["spk"]), True) for t in tr]
        w_heads = (w_c, w_b)
    else:
        spec = FX.DET_SPECS[name]
        x, w6, w7, w_c, w_b = FX.det_inputs(spec)
        with torch.no_grad():
            tr = OR.det_head_forward(x, w6, w7, w_c, w_b, spec["T"], trace=True)[2]
        cases = [(tr["spk7"], tr["spk7"].numpy(), False)]
        w_heads = (w_c, w_b)
    T = spec["T"]
    assert all(cases[0][1][t].any() for t in range(T // 2, T))                            # a live trace
    for spk, rows, conv in cases:
        assert rows.shape[0] == T
        for w in w_heads:
            last, run = PL.li_fp64(rows, w.flatten(1), a, b, li_order)
            assert last.shape == run.shape == (T, rows.shape[1], w.shape[0])
            for Tp in range(1, T + 1):
                with torch.no_grad():
                    mem, acc = OR.li_last_from_spikes(spk[:Tp], w, li_order, conv=conv)
                if conv:
                    mem, acc = (nchw_to_rows(m[None])[0] for m in (mem, acc))
                else:
                    mem, acc = mem.numpy(), acc.numpy()
                assert np.abs(last[Tp - 1] - mem).max() <= CUR_TOL, (Tp, float(np.abs(last[Tp - 1] - mem).max()))
                assert np.abs(run[Tp - 1] - acc).max() <= Tp * CUR_TOL, (Tp, float(np.abs(run[Tp - 1] - acc).max()))
    other = PL.li_fp64(cases[0][1], w_heads[0].flatten(1), a, b, "voltage_first" if li_order == "jump_first" else "jump_first")[0]
    mine = PL.li_fp64(cases[0][1], w_heads[0].flatten(1), a, b, li_order)[0]
    assert np.abs(other - mine).max() > 100 * CUR_TOL                                     # the two orders are told apart


def test_plane_layout_helpers_invert_synthetic_buffers():
    """rows_from_split / rows_from_word_major against buffers laid out in numpy word by word as include/snn_hip_debug.h words them
    ([T][C/128][P][4] / [T][Hd/32][R]), popcounts against a bit loop, and the dense round trip of tests/_util.py"""
    import numpy as np
    from tests import _planes as PL
    from tests._util import dense_to_planes, planes_to_dense
    rng = np.random.default_rng(5)
    T, P, Cw = 3, 7, 8
    rows = rng.integers(-2 ** 31, 2 ** 31, (T, P, Cw), dtype=np.int64).astype(np.int32)
    split = np.zeros((T, Cw // 4, P, 4), dtype=np.int32)
    for t in range(T):
        for p in range(P):
            for w in range(Cw):
                split[t, w // 4, p, w % 4] = rows[t, p, w]
    assert np.array_equal(PL.rows_from_split(torch.from_numpy(split.reshape(-1)), T, P, Cw, 1).numpy(), rows)
    assert np.array_equal(PL.rows_from_split(torch.from_numpy(rows.reshape(-1)), T, P, Cw, 0).numpy(), rows)
    assert not np.array_equal(split.reshape(T, P, Cw), rows)                               # (the layouts do differ)
    R, Hw = 11, 4
    rows = rng.integers(-2 ** 31, 2 ** 31, (T, R, Hw), dtype=np.int64).astype(np.int32)
    wm = np.zeros((T, Hw, R), dtype=np.int32)
    for t in range(T):
        for r in range(R):
            for w in range(Hw):
                wm[t, w, r] = rows[t, r, w]
    assert np.array_equal(PL.rows_from_word_major(torch.from_numpy(wm.reshape(-1)), T, R, Hw, 1).numpy(), rows)
    assert np.array_equal(PL.rows_from_word_major(torch.from_numpy(rows.reshape(-1)), T, R, Hw, 0).numpy(), rows)
    assert not np.array_equal(wm.reshape(T, R, Hw), rows)
    exp = np.array([[sum(bin(int(v) & 0xFFFFFFFF).count("1") for v in rows[t, r]) for r in range(R)] for t in range(T)], dtype=np.int64)
    got = PL.popcounts(torch.from_numpy(rows))
    assert got.dtype == np.int64 and np.array_equal(got, exp)
    assert np.array_equal(PL.cumulative_popcounts(torch.from_numpy(rows)), np.cumsum(exp, axis=0))
    dense = planes_to_dense(torch.from_numpy(rows), Hw * 32)
    assert np.array_equal(dense.sum(axis=2).astype(np.int64), exp) and np.array_equal(dense_to_planes(dense).numpy(), rows)
