"""Host-side checks of the fc6 route: the numpy restatement of the density statistic against hand-made period planes,
the default crossover against the inputs the GPU tests decide on, the module's switches and the argument checks that come before any
device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _exact_grid as G
from tests import _fc6_route as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_float(name):
    txt = open(os.path.join(ROOT, "include", "snn_hip.h")).read()
    m = re.search(r"#define\s+%s\s+([-+0-9.eE]+)f?\b" % name, txt)
    assert m, name
    return float(m.group(1))


def test_bin_major_order_puts_the_channels_of_a_bin_side_by_side():
    per = np.arange(2 * 3 * 49).reshape(2, 3 * 49)                    # R = 2, C = 3: k = c * 49 + bin
    bm = R.bin_major(per, 3)
    assert bm.shape == per.shape
    assert bm[0, :3].tolist() == [0, 49, 98] and bm[0, 3:6].tolist() == [1, 50, 99]          # bin 0: channels 0, 1, 2; then bin 1
    assert bm[1, 48 * 3 + 2] == per[1, 2 * 49 + 48]


def test_a_hit_needs_three_of_one_period_in_one_nibble():
    per = np.zeros((4, 128), dtype=np.int64)
    per[0, 8:12] = 3                 # a full nibble of period 3 in word pair 0
    per[1, 4:6] = 3                  # two ones in a nibble: the primary plane only
    per[2, 64:67] = 4                # three ones of period 4 in the first nibble of word pair 1
    per[3, 2:5] = 3                  # three of period 3 across two nibbles: 2 + 1
    assert R.secondary_rows(per, 3).tolist() == [[True, False], [False, False], [False, False], [False, False]]
    assert R.secondary_rows(per, 4).tolist() == [[False, False], [False, False], [False, True], [False, False]]
    assert not R.secondary_rows(per, 5).any()
    assert R.count_blocks(per, 8) == (2, 1 * 2 * 4)                   # T = 8: planes e_3 .. e_6
    assert R.count_blocks(per[1:2], 8) == (0, 8) and R.count_blocks(per[3:4], 8) == (0, 8)


def test_blocks_are_sixteen_rois_by_word_pair_by_plane_and_the_last_one_is_short():
    per = np.zeros((37, 64), dtype=np.int64)                           # 37 RoIs: blocks 0 .. 15, 16 .. 31, 32 .. 36 (short)
    assert R.count_blocks(per, 8) == (0, 3 * 1 * 4)
    assert R.count_blocks(per, 6) == (0, 3 * 1 * 2) and R.count_blocks(per, 5) == (0, 3) and R.count_blocks(per, 4) == (0, 0)
    assert list(R.fc6_planes(12)) == list(range(3, 11))
    per[15, 0:4] = 3
    per[16, 0:4] = 3                                                   # neighbours in two blocks
    per[17, 8:11] = 3                                                  # a second entry of block 1, plane e_3: still one hit
    per[36, 60:64] = 6                                                 # the short block, plane e_6
    assert R.count_blocks(per, 8) == (3, 12)
    assert R.count_blocks(per, 7) == (2, 9)                            # T = 7 has no plane e_6
    per[0, 0:4] = [1, 1, 1, 2]                                         # periods 1 and 2 stay on the dense instruction: never counted
    per[1, 0:4] = 7                                                    # period 7 = T - 1 lies outside fc6's window of T - 2 planes
    assert R.count_blocks(per, 8) == (3, 12)
    wide = np.zeros((37, 192), dtype=np.int64)
    wide[:, :64] = per
    wide[3, 188:192] = 4                                               # word pair 2 of plane e_4, block 0: counts once
    wide[5, 128:132] = 4                                               # the same block again
    assert R.count_blocks(wide, 8) == (4, 36)


@pytest.mark.parametrize("Rn,T", [(17, 6), (29, 12), (33, 16)])
def test_full_nibble_features_hit_every_block_and_silent_ones_none(Rn, T):
    g = torch.Generator().manual_seed(Rn + T)
    x = G.full_nibble_values((Rn, 64, 7, 7), T, g)
    hits, blocks = R.route_counts(x, T)
    planes = len(R.fc6_planes(T))
    assert blocks == (Rn + 15) // 16 * 49 * planes
    # every (RoI, nibble) sits on one of the periods 3 .. min(T - 1, 7) with four ones: every block of a plane that some nibble picked is hit;
    # planes beyond period 7 (and period T - 1, outside the window) stay empty
    # (a block of 16 RoIs holds 256 nibbles, each on one of at most five periods: it misses a period with probability 0.8^256; the short last
    # block - one row at R = 17 and 33 - may)
    live = len([n for n in R.fc6_planes(T) if n <= min(T - 1, 7)])
    assert Rn // 16 * 49 * live <= hits <= (Rn + 15) // 16 * 49 * live
    assert R.route_counts(R.silent_like(x), T) == (0, blocks)
    mh, mb = R.route_counts(R.mixed_like(x), T)
    assert mb == blocks and 0 < mh <= min(2, (Rn + 15) // 16) * 49 * live


def test_the_full_nibble_detector_case_hits_every_live_block():
    case = G.det_full_nibble_case()
    hits, blocks = R.route_counts(case["x"], case["T"])
    assert blocks == 2 * 49 * 8 and hits == 2 * 49 * 5               # R = 29, T = 12: planes e_3 .. e_10, periods 3 .. 7 in use


def test_default_crossover_is_the_headers_and_the_rule_has_its_two_ends():
    from snn_automotive_object_detection_amd import _lib
    d = _header_float("SNN_FC6_ROUTE_DEFAULT_CROSSOVER")
    assert np.float32(_lib.FC6_ROUTE_DEFAULT_CROSSOVER) == np.float32(d)
    assert _header_float("SNN_ROUTE_DEFAULT_CROSSOVER") == pytest.approx(_lib.ROUTE_DEFAULT_CROSSOVER)      # (the conv's constant keeps its own line)
    # the committed measurement names the same value
    txt = open(os.path.join(ROOT, "profiles", "fc6_route_crossover.txt")).read()
    m = re.search(r"^# Result: SNN_FC6_ROUTE_DEFAULT_CROSSOVER = ([0-9.]+)", txt, re.M)
    assert m and float(m.group(1)) == pytest.approx(d)
    # the rule itself: a crossover <= -1 always takes the dense side, one >= 1 never does
    assert R.route_of(0, 392, -1.0) == 1 and R.route_of(392, 392, 1.0) == 0 and R.route_of(392, 392, 2.0) == 0


def test_default_crossover_lies_in_the_expected_range_and_leaves_the_gpu_test_inputs_decisive():
    """the constant in (0.05, 0.95), or exactly 1.0 if measurement finds no crossover; the restated hit rates of the inputs the GPU tests
    decide on (tests/_fc6_route.decided_inputs) at least 0.05 away from it, on the expected side"""
    d = _header_float("SNN_FC6_ROUTE_DEFAULT_CROSSOVER")
    assert 0.05 < d < 0.95 or d == 1.0
    for name, x, route in R.decided_inputs():
        hits, blocks = R.route_counts(x, 8)
        print("%s: %d / %d = %.4f, crossover %g" % (name, hits, blocks, hits / blocks, d))
        assert blocks == 2 * 49 * 4
        if route and d < 1.0:
            assert hits / blocks >= d + 0.05 and R.route_of(hits, blocks, d) == 1, name
        elif not route:
            assert hits / blocks <= min(d, 1.0) - 0.05 and R.route_of(hits, blocks, d) == 0, name
    assert [R.route_counts(x, 8)[0] > 0 for _, x, _ in R.decided_inputs()] == [True, True, False, True]


def test_module_switches():
    import snn_automotive_object_detection_amd as S
    h = S.FastRCNNPredictorSNNFull(64 * 49, 128, 9, 12)
    assert h.fc6_route is None and h.fc6_crossover is None and h.route_stat is None and h.only_one_bbox is False
    h2 = S.FastRCNNPredictorSNNFull(64 * 49, 128, 9, 12, False, "auto", 0.25)
    assert h2.fc6_route == "auto" and h2.fc6_crossover == 0.25
    h3 = S.FastRCNNPredictorSNNFull(64 * 49, 128, 9, 12, fc6_route="dense")
    assert h3.fc6_route == "dense" and h3.fc6_crossover is None
    assert sorted(h2.state_dict()) == sorted(h.state_dict()) == ["bbox_pred.weight", "cls_score.weight", "fc6.weight", "fc7.weight"]


def test_bad_route_arguments_are_refused_before_any_device_work():
    from snn_automotive_object_detection_amd import _lib
    lib = _lib.load()
    p = _lib.snn_params(0.1, -0.2, 0, 0, 0.25, 0.1, 0, 1)
    shape = (29, 64 * 49, 128, 9, 36, 12)
    base = lib.snn_det_head_workspace_bytes(*shape, 1)
    for route in (0, 1, 2):
        assert lib.snn_det_head_workspace_bytes_routed(*shape, 1, route) >= base > 0
    assert lib.snn_det_head_workspace_bytes_routed(*shape, 1, 3) == 0
    nine = [None] * 9

    def rows(ws_bytes, route, stat=None):
        return lib.snn_det_head_forward_routed(None, 0, *shape, C.byref(p), None, 49, *nine, ws_bytes, route, 0.5, stat, None)

    def roialign(ws_bytes, route, stat=None):
        return lib.snn_det_head_forward_roialign_routed(None, 0, 2, 64, None, None, None, 29, 128, 9, 36, 12, C.byref(p), None, 49, *nine,
                                                        ws_bytes, route, 0.5, stat, None)

    for call in (rows, roialign):
        assert call(base, 3) == -1 and b"route" in lib.snn_last_error()
        assert call(base, 2) == -1 and b"route_stat" in lib.snn_last_error()
        assert call(base - 1, 1) == -1 and b"workspace" in lib.snn_last_error()
        assert call(base - 1, 0) == -1 and b"workspace" in lib.snn_last_error()
