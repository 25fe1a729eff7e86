"""Heads and post-processing must not depend on what their workspace held before, and must stay inside the size they asked for.

Every call here reaches the library through the seam of tests/_ws_state.py: ops._WS / ops._WS_RATES are GuardedWorkspaces, so the library is
told EXACTLY the size its own query returned, the bytes around that region are guarded, and the region's prior contents are chosen.  Outputs
are allocated by ops inside W.poisoned_outputs(): NaN / 0x5a before the call.  The cases are the smallest of the suite's own exact builders
(tests/_exact_grid.py, tests/_conv_route.py, tests/_fc6_route.py, tests/_post_grid.py), so the expectation is the oracle with zero flips and
not only self-agreement; each case asserts the launch plan it is meant to reach (snn_debug_last_conv_path / snn_debug_last_fc6_path).

  (b) sequences on one buffer (they come first in the file: they run before the fills): each step returns the bits of the same call alone
      on freshly armed zeros - large then small, the product's order, route flips, counter sharing, plane forms, precisions, T;
  (a) per entry of _ws_state.ENTRIES and per fill 0x00 / 0x5a / 0xff: guards and tail intact, the snapshot bit-equal to the 0x00 one, and the
      0x00 one equal to the oracle (hidden planes and counts with zero flips, outputs within CUR_TOL of fp64 on those planes and 1e-4 of the
      oracle, post-processing with the zero-tolerance asserts of tests/test_gpu_post_grid.py);
  (c) a workspace one byte too small: an error, nothing enqueued - poisoned outputs stay poisoned, the armed buffer stays armed.
A snapshot = outputs, time sums, spike counts, rate rows, route_stat and the hidden planes (through the debug accessors).
The spec constructors and the runners (run_rpn, run_det, run_roi, run_nms, run_rpn_proposals, run_det_postprocess) live in tests/_entry_cases.py,
split into prepare / call / oracle: tests/test_gpu_graph_capture.py replays the same cases from a captured graph."""
import pytest
import torch

from tests import _ws_state as W
from tests._entry_cases import BUILDERS, Record, call, det, post, roi, rpn, run, spec_id   # noqa: F401  (the runners, split into prepare / call / oracle, live there: graph capture shares them)

pytestmark = pytest.mark.gpu


# ---- the seam ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def buffers(gpu_device):
    return W.GuardedWorkspace(gpu_device), W.GuardedWorkspace(gpu_device, 1 << 20)


@pytest.fixture
def seam(buffers, monkeypatch):
    from snn_automotive_object_detection_amd import ops
    monkeypatch.setattr(ops, "_WS", buffers[0])
    monkeypatch.setattr(ops, "_WS_RATES", buffers[1])
    for b in buffers:
        b.short_by = 0
    yield buffers
    for b in buffers:
        b.short_by = 0


# ---- (b) sequences on one buffer ---------------------------------------------------------------------------------------------------------
RO = dict(entry="rpn_head_forward_readouts")
DRO = dict(entry="det_head_forward_readouts")
SEQUENCES = {
    "large_then_small_rpn": [rpn(128, 16, "full"), rpn(64, 5, "silent", in_shapes=W.ONE_BY_ONE)],
    "large_then_small_det": [det(65, 64, 24), det(1, 64, 6)],
    "product_order": [rpn(64, 8), post("rpn_proposals", spec=W.RPN_POST_SPEC), roi(), post("det_postprocess", spec=W.DET_POST_SPEC),
                      rpn(64, 8, "mixed"), post("rpn_proposals", spec=W.RPN_POST_SPEC)],
    "route_flips_rpn": [rpn(128, 8, "full", "auto"), rpn(128, 8, "silent", "auto"), rpn(128, 8, "mixed", "sparse"), rpn(128, 8, "mixed", "dense"),
                        rpn(128, 8, "mixed", "auto")],
    "route_flips_det": [det(29, 64, 12, "full", "auto"), det(29, 64, 12, "silent", "auto"), det(29, 64, 12, "case", "sparse"),
                        det(29, 64, 12, "case", "dense"), det(29, 64, 12, "case", "auto")],
    "counter_sharing_rpn": [rpn(64, 8, "full", "rates"), rpn(64, 8, "mixed", "auto"), rpn(64, 8, "full", "rates")],
    "counter_sharing_det": [det(29, 64, 12, "full", "rates"), det(29, 64, 12, "mixed", "auto"), det(29, 64, 12, "full", "rates")],
    "plane_form_rpn": [rpn(64, 12, "mixed"), rpn(64, 12, "mixed", "auto"), rpn(64, 12, "mixed", **RO), rpn(64, 12, "mixed")],
    "plane_form_det": [det(29, 64, 12), det(29, 64, 12, "case", "auto"), det(29, 64, 12, **DRO), det(29, 64, 12)],
    "precisions": [rpn(128, 8, "mixed"), rpn(128, 8, "mixed", precision="f32"), rpn(128, 8, "mixed", precision="mxfp6"),
                   rpn(128, 8, "mixed", precision="bf16"), rpn(128, 8, "mixed")],
    "T_rpn": [rpn(64, 16, "mixed"), rpn(64, 5, "mixed"), rpn(64, 8, "mixed"), rpn(64, 4, "mixed")],
    "T_det": [det(29, 64, 24), det(29, 64, 6), det(29, 64, 12)],
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_sequence_on_one_buffer(gpu_device, seam, name):
    """each step returns the bits of the same call alone on freshly armed zeros (and meets its oracle both times); the buffer is armed once,
    with 0x5a, before the first step"""
    specs = SEQUENCES[name]
    W.run_sequence(seam, [call(s, gpu_device) for s in specs], start_fill=0x5a)
    assert seam[0].sizes and len(seam[0].sizes) >= len(specs)


def test_route_flips_take_the_side_the_input_names(gpu_device, seam):
    """the first two steps of the route sequences: `auto` at the header's crossover takes the dense side on full-nibble input and the sparse
    side on silent input (route_stat[2]; run_rpn / run_det compare the whole array with the restated count)"""
    for s, route in [(SEQUENCES["route_flips_rpn"][0], 1), (SEQUENCES["route_flips_rpn"][1], 0), (SEQUENCES["route_flips_det"][0], 1),
                     (SEQUENCES["route_flips_det"][1], 0)]:
        for b in seam:
            b.arm(0x00)
        r = run(s, gpu_device)
        r["oracle"]()
        assert r["path"] == 2 and r["stat"][2] == route and r["stat"][1] > 0 and (r["stat"][0] > 0) == bool(route), (spec_id(s), r["stat"])


# ---- (a) contents and exact size, per entry and fill --------------------------------------------------------------------------------------
def _fill_specs():
    out = []
    # the RPN head: the sparse window's edges, both FAT shapes and the 8-wave shape, on every input
    out += [rpn(C, T, inp) for C in (64, 128) for T in (5, 8, 16) for inp in ("silent", "mixed", "full")]
    out += [rpn(C, T, inp, v) for C, T, inp in ((64, 8, "mixed"), (128, 16, "full")) for v in W.HEAD_VARIANTS[1:]]
    out += [rpn(64, 8, "mixed", "rates", ws="_WS_RATES")]
    out += [rpn(256, 8, inp, v, shapes=W.SPLIT_PYRAMID) for inp, v in (("mixed", "plain"), ("full", "auto_never"), ("case", "rates"))]
    out += [rpn(64, 4, "mixed", v) for v in ("plain", "rates", "auto_always")]                     # the dense plan
    out += [rpn(64, 8, "mixed", precision="f32"), rpn(64, 8, "mixed", precision="bf16"), rpn(128, 8, "mixed", precision="mxfp6")]
    out += [rpn(64, 8, "case", feat="fp16", nhwc=True)]
    out += [rpn(64, 12, "mixed", v, **RO) for v in ("plain", "rates")] + [rpn(64, 12, "mixed", "rates", ws="_WS_RATES", **RO)]
    # the detector head
    out += [det(29, 64, T) for T in (6, 12, 16, 24)]
    out += [det(R, C, 12) for R in (1, 17, 65) for C in (32, 64)]                                    # R = 17: a partly filled RoI group
    out += [det(R, 64, 12, inp, v) for R, inp in ((29, "case"), (17, "case"), (29, "full")) for v in W.HEAD_VARIANTS[1:]]
    out += [det(29, 64, 12, "silent")]
    out += [det(29, 64, 12, precision="f32"), det(29, 64, 12, precision="bf16"), det(37, 128, 12, precision="mxfp6")]
    out += [det(29, 64, 12, feat="fp16")]
    out += [det(29, 64, 12, "case", v, **DRO) for v in ("plain", "rates")]
    out += [roi(v) for v in W.ENTRIES[("det_head_forward_roialign", "_WS")]] + [roi("rates"), roi("plain", feat="fp16", nhwc=True)]
    out += [roi(v, entry="det_head_forward_roialign_readouts") for v in ("plain", "rates")]
    # post-processing
    out += [post(e, n=n, ncat=3, layout=lay) for e in ("batched_nms", "nms_keep_mask") for n, lay in ((65, 3), (129, 5))]
    out += [post("rpn_proposals", spec=W.RPN_POST_SPEC), post("det_postprocess", spec=W.DET_POST_SPEC), post("det_postprocess_padded", spec=W.DET_POST_SPEC)]
    return out


FILL_SPECS = _fill_specs()
_ZERO_SNAPS = {}


def _buffers_of(seam, s):
    return list(seam) if s["kind"] == "rpn" else [seam[0]]


@pytest.mark.parametrize("s,fill", [(s, f) for s in FILL_SPECS for f in W.FILLS], ids=["%s-fill%02x" % (spec_id(s), f) for s in FILL_SPECS for f in W.FILLS])
def test_contents_and_exact_size(gpu_device, seam, s, fill):
    """armed with `fill`, told exactly the queried size: guards and tail intact, the oracle met, the snapshot bit-equal to the 0x00 one"""
    key = spec_id(s)
    if key not in _ZERO_SNAPS:
        _ZERO_SNAPS[key] = W.armed_call(_buffers_of(seam, s), 0x00, call(s, gpu_device))
    if fill != 0x00:
        snap = W.armed_call(_buffers_of(seam, s), fill, call(s, gpu_device))
        assert W.same_bits(snap, _ZERO_SNAPS[key]), "fill 0x%02x against 0x00: %s" % (fill, W.first_difference(snap, _ZERO_SNAPS[key]))
    assert seam[0].sizes and seam[0].high == seam[0].sizes[-1]           # (the region was the query's size, to the byte)


# ---- (c) too small by one byte -----------------------------------------------------------------------------------------------------------
SHORT_SPECS = ([rpn(64, 8, "mixed", v) for v in W.HEAD_VARIANTS] + [rpn(64, 8, "mixed", "rates", ws="_WS_RATES")]
               + [rpn(64, 12, "mixed", v, **RO) for v in ("plain", "rates")] + [rpn(64, 12, "mixed", "rates", ws="_WS_RATES", **RO)]
               + [det(29, 64, 12, "case", v) for v in W.HEAD_VARIANTS] + [det(29, 64, 12, "case", v, **DRO) for v in ("plain", "rates")]
               + [roi(v) for v in W.ENTRIES[("det_head_forward_roialign", "_WS")]]
               + [roi(v, entry="det_head_forward_roialign_readouts") for v in ("plain", "rates")]
               + [post(e, n=65, ncat=3, layout=3) for e in ("batched_nms", "nms_keep_mask")]
               + [post("rpn_proposals", spec=W.RPN_POST_SPEC), post("det_postprocess", spec=W.DET_POST_SPEC),
                  post("det_postprocess_padded", spec=W.DET_POST_SPEC)])


@pytest.mark.parametrize("s", SHORT_SPECS, ids=[spec_id(s) for s in SHORT_SPECS])
def test_one_byte_too_small_is_refused_with_nothing_enqueued(gpu_device, seam, s):
    """the seam hands out need - 1 bytes: the call returns its error (snn_last_error names the workspace) before any device work - every output
    ops allocated for it is still NaN / 0x5a, route_stat still -7, the armed buffer untouched.  (The rates call sits behind a head call that
    runs: there the claim is about the rates buffer and the rate rows.)"""
    from snn_automotive_object_detection_amd import _lib
    main, rates = seam
    target = rates if s["ws"] == "_WS_RATES" else main
    for b in seam:
        b.arm(0x5a)
    target.short_by = 1
    record = Record()
    with pytest.raises(_lib.SnnHipError, match=r"rc=-[12]\b.*workspace"):
        run(s, gpu_device, record)
    torch.cuda.synchronize()
    assert record.stat is None or s["ws"] == "_WS_RATES" or record.stat.tolist() == [-7] * 4
    assert target.sizes and target.size == target.sizes[-1] - 1
    assert target.untouched(), "the refused call wrote to its workspace"
    outs = [t for t in record if t.is_cuda]
    assert outs or s["entry"] == "nms_keep_mask"                      # (its buffers are torch.full / torch.zeros: nothing of it is left unwritten)
    if s["ws"] == "_WS_RATES":
        outs = outs[-1:]                                                # the rate rows (allocated right before the refused call)
    assert all(W.still_poisoned(t) for t in outs), "the refused call wrote to an output"
    for b in seam:
        b.check()


def all_specs():
    """every spec this file runs (tests/test_ws_state_cpu.py asks the size queries about their shapes)"""
    return [s for seq in SEQUENCES.values() for s in seq] + FILL_SPECS + SHORT_SPECS
