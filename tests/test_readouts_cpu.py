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
