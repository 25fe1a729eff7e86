"""The seven training entries stay inside their buffers at every tile edge (include/snn_hip.h: snn_li_heads_wgrad, snn_match_targets,
snn_rpn_loss_grad, snn_det_loss_grad, snn_planes_to_rows, snn_lif_surrogate_bwd, snn_spike_linear_wgrad).

Every call here runs through tests/_train_entries.run: each operand lies in an allocation of its own, [guard | payload | guard] to the byte
(tests/_ws_state.Guarded), outputs pre-filled with NaN / 0x5a, and the scratch comes from a _ws_state.GuardedWorkspace installed at
readout._WS_WGRAD, hidden._WS_WGRAD and losses._WS_LOSS.  After every call: no guard byte of any operand changed, no input changed, no output
element left unwritten, and the fp64 / integer expectation of the case's own builder is met.

  1. guarded operands   every edge shape and loss case under input guards of zeros and of 0xff bytes (NaN as floats, every spike bit set,
                        label -1): the two snapshots are bit-equal.  The edge shapes: snn_spike_linear_wgrad at K, N in {1, 31, 33, 63, 65,
                        127, 129, 255, 257, 288} (28 pairs) over reduction lengths on every branch of the batch / slab split, ldd = N + 5,
                        padding bits set, both accumulate values; snn_li_heads_wgrad at n_cols in {1, 33, 127, 129, 130} on the three layouts
                        with 1, 17, 32 and 17 outputs over 63, 64 and 65 rows; snn_lif_surrogate_bwd at N in {1, 31, 33}, R in {1, 9},
                        Tc in {1, 31}; snn_planes_to_rows on the three layouts; snn_match_targets at 64 images of one box and at 257 / 0 / 256
                        boxes with 256 / 3 / 1 ground-truth boxes
  2. the scratch seam   per fill 0x00 / 0x5a / 0xff: guards and tail intact, the handed-out size equal to the size query (max(16, need): the
                        wrappers never ask for less than 16 bytes), snapshots bit-equal
  3. one byte short     SnnHipError naming the scratch, nothing enqueued: outputs still poisoned, the armed buffer untouched
  4. sequences          per seam, on a buffer armed once with 0x5a: large, small, large (losses: match, rpn loss, det loss, match - the three
                        entries share the buffer); each step bit-equal to the same call alone on armed zeros
profiles/train_entry_bounds.txt lists the shapes and the boundary each one sits on."""
import importlib

import pytest
import torch

from tests import _train_entries as TE
from tests import _ws_state as W

pytestmark = pytest.mark.gpu


def _module(name):
    return importlib.import_module("snn_automotive_object_detection_amd." + name)


@pytest.fixture(scope="module")
def buffers(gpu_device):
    return {seam: W.GuardedWorkspace(gpu_device, TE.SEAM_INTERIOR) for seam in TE.SEAMS}


@pytest.fixture
def seams(buffers, monkeypatch):
    for (module, attr), b in buffers.items():
        monkeypatch.setattr(_module(module), attr, b)
        b.short_by = 0
        b.arm(0x00)
    yield buffers
    for b in buffers.values():
        b.short_by = 0


def _assert_size(s, b):
    """the library was told the size query's bytes, to the byte (the wrappers ask for max(16, need))"""
    from snn_automotive_object_detection_amd import _lib
    need = TE.queried_bytes(_lib.load(), s)
    assert need == TE.restated_bytes(s) > 0
    assert b.sizes and b.sizes[-1] == max(16, need) == b.size, "%s: handed out %s, max(16, need) = max(16, %d)" % (TE.spec_id(s), b.sizes, need)


# ---- 1. guarded operands, edge shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", TE.OPERAND_SPECS, ids=[TE.spec_id(s) for s in TE.OPERAND_SPECS])
def test_operands_are_respected_to_the_byte(gpu_device, seams, s):
    """zeros, then 0xff bytes, before and behind every input: guards, inputs and outputs verified and the expectation met both times (TE.run),
    the two snapshots bit-equal; the scratch (where the entry takes one) stays inside the queried size on armed 0x5a"""
    seam = TE.seam_of(s)
    for b in seams.values():
        b.arm(0x5a)
    W.run_input_guards(lambda guard: TE.run(s, gpu_device, guard))
    for b in seams.values():
        b.check()
    if seam is not None:
        _assert_size(s, seams[seam])
    assert all(b.untouched() for k, b in seams.items() if k != seam), "a seam of another module was used"


# ---- 2. the scratch seam: contents and exact size --------------------------------------------------------------------------------------------
_ZERO_SNAPS = {}


@pytest.mark.parametrize("s,fill", [(s, f) for s in TE.FILL_SPECS for f in W.FILLS], ids=["%s-fill%02x" % (TE.spec_id(s), f) for s in TE.FILL_SPECS for f in W.FILLS])
def test_scratch_contents_and_exact_size(gpu_device, seams, s, fill):
    """armed with `fill`, told exactly the queried size: guards and tail intact, the expectation met, the snapshot bit-equal to the 0x00 one"""
    b = seams[TE.seam_of(s)]
    k = TE.key(s)
    if k not in _ZERO_SNAPS:
        _ZERO_SNAPS[k] = W.armed_call([b], 0x00, TE.call(s, gpu_device))
        _assert_size(s, b)
    if fill != 0x00:
        snap = W.armed_call([b], fill, TE.call(s, gpu_device))
        assert W.same_bits(snap, _ZERO_SNAPS[k]), "fill 0x%02x against 0x00: %s" % (fill, W.first_difference(snap, _ZERO_SNAPS[k]))
        _assert_size(s, b)
    assert b.high == b.sizes[-1]


# ---- 3. one byte short ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", TE.SHORT_SPECS, ids=[TE.spec_id(s) for s in TE.SHORT_SPECS])
def test_scratch_one_byte_short_is_refused_with_nothing_enqueued(gpu_device, seams, s):
    from snn_automotive_object_detection_amd import _lib
    b = seams[TE.seam_of(s)]
    need = TE.queried_bytes(_lib.load(), s)
    assert need >= 16, "max(16, need) would hide the missing byte"
    host, gc = TE.prepare(s), TE.stage(s, gpu_device)
    b.arm(0x5a)
    b.short_by = 1
    with pytest.raises(_lib.SnnHipError, match=r"%s failed \(rc=-1\): %s: scratch %d < %d bytes" % (s["entry"], s["entry"], need - 1, need)):
        TE.CALLS[s["entry"]](s, host, gc.ins, gc.outs)
    torch.cuda.synchronize()
    assert b.sizes == [need] and b.size == need - 1
    assert b.untouched(), "the refused call wrote to its scratch"
    assert gc.outputs_untouched(), "the refused call wrote to an output"
    gc.check_guards()


# ---- 4. sequences on one buffer --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam", list(TE.SEQUENCES), ids=["%s.%s" % k for k in TE.SEQUENCES])
def test_sequence_on_one_buffer(gpu_device, seams, seam):
    """each step returns the bits of the same call alone on freshly armed zeros (and meets its expectation both times); the buffer is armed
    once, with 0x5a, before the first step"""
    specs = TE.SEQUENCES[seam]
    assert all(TE.seam_of(s) == seam for s in specs)
    b = seams[seam]
    W.run_sequence([b], [TE.call(s, gpu_device) for s in specs], start_fill=0x5a)
    from snn_automotive_object_detection_amd import _lib
    assert b.sizes == [max(16, TE.queried_bytes(_lib.load(), s)) for s in specs], "every step is told its own max(16, need)"
    assert all(o.untouched() for k, o in seams.items() if k != seam)
