"""Host-side checks of the conv route: the numpy restatement of the density statistic against hand-made period planes,
the default crossover, the module's switches and the argument checks that come before any device work."""
import ctypes as C
import os
import re

import numpy as np

from tests import _conv_route as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_float(name):
    txt = open(os.path.join(ROOT, "include", "snn_hip.h")).read()
    m = re.search(r"#define\s+%s\s+([-+0-9.eE]+)f?\b" % name, txt)
    assert m, name
    return float(m.group(1))


def _header_int(name):
    txt = open(os.path.join(ROOT, "include", "snn_hip.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)\b" % name, txt).group(1))


def test_periods_come_from_the_first_spike():
    z = np.zeros((5, 4), dtype=np.float32)
    z[0, 0] = z[2, 0] = 1            # period 1
    z[2, 1] = 1                      # period 3
    z[4, 2] = 1                      # period 5
    assert R.periods_from_trains(z).tolist() == [1, 3, 5, 0]


def test_padded_rows_put_every_position_behind_its_halo():
    a = np.arange(1, 1 + 2 * 1 * 2 * 3).reshape(2, 1, 2, 3)           # N = 2, C = 1, H = 2, W = 3
    b = np.full((1, 1, 1, 1), 99)
    rows = R.padded_rows([a, b])[:, 0]
    assert rows.shape == (2 * 4 * 5 + 9,)
    img0 = rows[:20].reshape(4, 5)
    assert img0[1:3, 1:4].tolist() == [[1, 2, 3], [4, 5, 6]] and img0.sum() == 21
    assert rows[20:40].reshape(4, 5)[1:3, 1:4].tolist() == [[7, 8, 9], [10, 11, 12]]
    assert rows[40:].reshape(3, 3).tolist() == [[0, 0, 0], [0, 99, 0], [0, 0, 0]]


def test_a_secondary_entry_needs_three_of_one_period_in_one_nibble():
    per = np.zeros((3, 128), dtype=np.int64)
    per[0, 4:7] = 3                  # three of period 3 in nibble 1 of word pair 0
    per[1, 2:5] = 3                  # three of period 3 across two nibbles: 2 + 1
    per[2, 64:68] = [4, 4, 4, 3]     # three of period 4 (and one of period 3) in the first nibble of word pair 1
    assert R.secondary_rows(per, 3).tolist() == [[True, False], [False, False], [False, False]]
    assert R.secondary_rows(per, 4).tolist() == [[False, False], [False, False], [False, True]]
    assert not R.secondary_rows(per, 5).any()
    assert R.secondary_rows(per[:, :100], 3).shape == (3, 2)           # 100 channels: two word pairs, the tail silent


def test_blocks_are_sixteen_padded_rows_by_word_pair_by_plane():
    per = np.zeros((40, 64), dtype=np.int64)                           # 40 rows: blocks 0 .. 15, 16 .. 31, 32 .. 39 (short)
    assert R.count_blocks(per, 8) == (0, 3 * 1 * 5)
    assert R.count_blocks(per, 5) == (0, 3 * 1 * 2) and R.count_blocks(per, 3) == (0, 0)
    per[15, 0:4] = 3
    per[16, 0:4] = 3                                                   # neighbours in two blocks
    per[17, 8:11] = 3                                                  # a second entry of block 1, plane e_3: still one hit
    per[39, 60:64] = 7                                                 # the short block, plane e_7
    assert R.count_blocks(per, 8) == (3, 15)
    assert R.count_blocks(per, 7) == (2, 12)                           # T = 7 has no plane e_7
    per[0, 0:2] = 5                                                    # two of a period: primary plane only
    per[1, 0:4] = [1, 1, 1, 2]                                         # periods 1 and 2 stay on the dense instruction: never counted
    assert R.count_blocks(per, 8) == (3, 15)
    wide = np.zeros((40, 128), dtype=np.int64)
    wide[:, :64] = per
    wide[3, 124:128] = 4
    assert R.count_blocks(wide, 8) == (4, 30)


def test_the_full_nibble_maps_hit_every_block_that_holds_a_position():
    from tests._exact_grid import PYRAMID
    feats = R.full_nibble_maps(64, 8, PYRAMID, 2, 5)
    hits, blocks = R.route_counts(feats, 8)
    Pe = sum(2 * (h + 2) * (w + 2) for h, w in PYRAMID)
    assert blocks == (Pe + 15) // 16 * 5 and 0.3 * blocks < hits <= blocks
    assert R.route_counts(R.silent_maps(64, PYRAMID, 2), 8) == (0, blocks)
    mh, mb = R.route_counts(R.mixed_maps(64, 8, PYRAMID, 2, 5), 8)
    assert mb == blocks and 0 < mh < hits


def test_default_crossover_is_the_headers_and_leaves_both_test_cases_decisive():
    from snn_automotive_object_detection_amd import _lib
    d = _header_float("SNN_ROUTE_DEFAULT_CROSSOVER")
    assert 0.05 < d < 0.95
    assert np.float32(_lib.ROUTE_DEFAULT_CROSSOVER) == np.float32(d)
    assert _lib.CONV_ROUTES == {"sparse": _header_int("SNN_ROUTE_SPARSE"), "dense": _header_int("SNN_ROUTE_DENSE"),
                                "auto": _header_int("SNN_ROUTE_AUTO")}


def test_module_switches():
    import snn_automotive_object_detection_amd as S
    h = S.RPNHeadSNN(64, 3, 8)
    assert h.conv_route is None and h.conv_crossover is None and h.route_stat is None
    h2 = S.RPNHeadSNN(64, 3, 8, conv_route="auto", conv_crossover=0.25)
    assert h2.conv_route == "auto" and h2.conv_crossover == 0.25
    assert sorted(h2.state_dict()) == sorted(h.state_dict())


def test_bad_route_arguments_are_refused_before_any_device_work():
    from snn_automotive_object_detection_amd import _lib
    lib = _lib.load()
    lv = (_lib.snn_rpn_level * 1)(_lib.snn_rpn_level(None, 2, 16, 16, 0))
    p = _lib.snn_params(0.1, -0.2, 0, 0, 0.25, 0.1, 0, 1)
    base = lib.snn_rpn_head_workspace_bytes(lv, 1, 64, 3, 8, 1)
    for route in (0, 1, 2):
        assert lib.snn_rpn_head_workspace_bytes_routed(lv, 1, 64, 3, 8, 1, route) >= base > 0
    assert lib.snn_rpn_head_workspace_bytes_routed(lv, 1, 64, 3, 8, 1, 3) == 0
    tail = [None] * 8
    rc = lib.snn_rpn_head_forward_routed(lv, 0, 1, 64, 3, 8, C.byref(p), *tail, 0, 3, 0.5, None, None)
    assert rc == -1 and b"route" in lib.snn_last_error()
    rc = lib.snn_rpn_head_forward_routed(lv, 0, 1, 64, 3, 8, C.byref(p), *tail, 0, 2, 0.5, None, None)
    assert rc == -1 and b"route_stat" in lib.snn_last_error()
    rc = lib.snn_rpn_head_forward_routed(lv, 0, 1, 64, 3, 8, C.byref(p), *tail, base - 1, 1, 0.5, None, None)
    assert rc == -1 and b"workspace" in lib.snn_last_error()
