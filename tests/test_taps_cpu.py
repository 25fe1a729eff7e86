"""Spike taps without a GPU: the host-only plane-view queries over the shape grids of tests/_ws_state.py, the taps' argument checks, and
the numpy restatement of the three plane layouts (tests/_taps.py) against the layout helpers of tests/_planes.py."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

from tests import _taps as TP
from tests import _ws_state as WS
from tests._planes import rows_from_split, rows_from_word_major

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from snn_automotive_object_detection_amd import _lib
    return _lib


def _params(precision: str):
    L = _lib()
    return L.snn_params(0.1, -0.2, 0.0, 0.0, 0.25, 0.1, 0, L.PRECISIONS[precision])


def _levels(shapes, N):
    L = _lib()
    return (L.snn_rpn_level * len(shapes))(*[L.snn_rpn_level(None, N, h, w, 0) for h, w in shapes])


def _check_view(v, T, need, spike_rates, what):
    f = TP.view_fields(v)
    assert f["layout"] in TP.LAYOUTS, what
    assert f["offset"] % 4 == 0 and f["rows"] > 0 and f["words"] > 0 and f["stride"] >= f["rows"] * f["words"], (what, f)
    assert f["offset"] + T * f["stride"] * 4 <= need, "%s: the view ends at byte %d of a %d-byte workspace" % (what, f["offset"] + T * f["stride"] * 4, need)
    assert 1 <= f["steps_formed"] <= T, (what, f)
    if spike_rates:
        assert f["steps_formed"] == T, (what, f)
    if f["layout"] == TP.SPLIT4:
        assert f["words"] % 4 == 0, what
    return f


def test_header_layout_enumerators_match_the_binding():
    txt = open(os.path.join(ROOT, "include", "snn_hip.h")).read()
    got = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"SNN_PLANES_([A-Z0-9_]+) = (\d+)", txt)}
    assert got == _lib().PLANE_LAYOUTS == {"rows": TP.ROWS, "split4": TP.SPLIT4, "word_major": TP.WORD_MAJOR}
    assert C.sizeof(_lib().snn_planes_view) == 40


def test_rpn_view_lies_inside_the_workspace_for_every_shape_precision_and_route():
    L = _lib()
    lib = L.load()
    seen = set()
    shapes = sorted({(Cc, T, sh, N) for Cc, T, sh, N, _ in WS.RPN_SHAPES})
    for (Cc, T, sh, N), prec, (route_name, route), rates in itertools.product(shapes, sorted(L.PRECISIONS), sorted(L.CONV_ROUTES.items()), (0, 1)):
        p, lv, v = _params(prec), _levels(sh, N), L.snn_planes_view()
        what = "C=%d T=%d %s N=%d %s %s rates=%d" % (Cc, T, sh, N, prec, route_name, rates)
        assert lib.snn_rpn_head_planes_view(lv, len(sh), Cc, 3, T, C.byref(p), route, rates, C.byref(v)) == 0, (what, lib.snn_last_error())
        need = lib.snn_rpn_head_workspace_bytes_routed(lv, len(sh), Cc, 3, T, p.precision, route)
        assert need == lib.snn_rpn_head_workspace_bytes(lv, len(sh), Cc, 3, T, p.precision) > 0
        f = _check_view(v, T, need, rates, what)
        assert f["rows"] == N * sum(h * w for h, w in sh) and f["words"] == (Cc + 31) // 32
        assert f["steps_formed"] == T                               # (the LI heads read the shared LIF's spikes of every step)
        assert f["layout"] in (TP.ROWS, TP.SPLIT4)
        seen.add((prec, f["layout"]))
    assert ("bf16x3", TP.SPLIT4) in seen and ("bf16x3", TP.ROWS) in seen and ("f32", TP.SPLIT4) not in seen


def test_det_views_lie_inside_the_workspace_for_every_shape_precision_and_route():
    L = _lib()
    lib = L.load()
    seen = set()
    shapes = sorted({(R, Cc, Hd, K, T) for R, Cc, Hd, K, T, _ in WS.DET_SHAPES})
    for (R, Cc, Hd, K, T), prec, (route_name, route), rates, inner in itertools.product(shapes, sorted(L.PRECISIONS), sorted(L.CONV_ROUTES.items()),
                                                                                      (0, 1), (0, 49)):
        p, v6, v7 = _params(prec), L.snn_planes_view(), L.snn_planes_view()
        D = 49 * Cc
        what = "R=%d C=%d Hd=%d T=%d %s %s rates=%d inner=%d" % (R, Cc, Hd, T, prec, route_name, rates, inner)
        assert lib.snn_det_head_planes_view(R, D, Hd, K, 4 * K, T, C.byref(p), inner, route, rates, C.byref(v6), C.byref(v7)) == 0, (what, lib.snn_last_error())
        need = lib.snn_det_head_workspace_bytes_routed(R, D, Hd, K, 4 * K, T, p.precision, route)
        assert need == lib.snn_det_head_workspace_bytes(R, D, Hd, K, 4 * K, T, p.precision) > 0
        f6, f7 = _check_view(v6, T, need, rates, what + " lif6"), _check_view(v7, T, need, rates, what + " lif7")
        for f in (f6, f7):
            assert f["rows"] == R and f["words"] == (Hd + 31) // 32
        assert f7["layout"] == TP.ROWS and f7["steps_formed"] == T
        assert f6["layout"] in (TP.ROWS, TP.WORD_MAJOR)
        assert f6["offset"] + T * f6["stride"] * 4 <= f7["offset"]    # (two plane sets, not one)
        if not rates and T >= 3:
            assert f6["steps_formed"] == T - 1, what                 # lif6's last plane reaches nothing and is not formed
        seen.add((prec, f6["layout"]))
    assert ("bf16x3", TP.WORD_MAJOR) in seen and ("f32", TP.ROWS) in seen and ("f32", TP.WORD_MAJOR) not in seen


def test_view_queries_refuse_bad_arguments():
    L = _lib()
    lib = L.load()
    p, lv, v = _params("bf16x3"), _levels(((3, 4),), 1), L.snn_planes_view()
    assert lib.snn_rpn_head_planes_view(lv, 1, 64, 3, 8, C.byref(p), 0, 1, None) == -1 and b"snn_rpn_head_planes_view" in lib.snn_last_error()
    assert lib.snn_rpn_head_planes_view(lv, 1, 64, 3, 40, C.byref(p), 0, 1, C.byref(v)) == -1
    assert lib.snn_rpn_head_planes_view(lv, 1, 64, 3, 8, C.byref(p), 7, 1, C.byref(v)) == -1 and b"route" in lib.snn_last_error()
    assert lib.snn_det_head_planes_view(4, 49 * 64, 128, 9, 36, 12, C.byref(p), 49, 0, 1, None, None) == -1
    assert lib.snn_det_head_planes_view(0, 49 * 64, 128, 9, 36, 12, C.byref(p), 49, 0, 1, C.byref(v), None) == -1
    assert lib.snn_det_head_planes_view(4, 49 * 64, 128, 9, 36, 12, C.byref(p), 49, 0, 1, C.byref(v), None) == 0      # (either view may be left out)


def test_taps_refuse_bad_arguments_before_any_device_work():
    """null view, T' above steps_formed, a group table that is not increasing: -1 with a message, on a machine without a GPU"""
    L = _lib()
    lib = L.load()
    p, v6 = _params("bf16x3"), L.snn_planes_view()
    assert lib.snn_det_head_planes_view(10, 49 * 64, 128, 9, 36, 12, C.byref(p), 49, 0, 0, C.byref(v6), None) == 0
    assert v6.steps_formed == 11
    fake = (C.c_uint8 * 64)()                                        # never dereferenced: every call below is refused on the host
    ws = C.c_void_p(C.addressof(fake))
    starts = (C.c_int64 * 3)(0, 4, 10)

    def refused(rc, word):
        msg = lib.snn_last_error()
        assert rc == -1 and word in msg, (rc, msg)

    refused(lib.snn_planes_counts(ws, None, starts, 2, 128, 4, None, None, None, None), b"snn_planes_counts")
    refused(lib.snn_planes_counts(None, C.byref(v6), starts, 2, 128, 4, None, None, None, None), b"null")
    refused(lib.snn_planes_counts(ws, C.byref(v6), starts, 2, 128, 12, None, None, None, None), b"forms 11")
    refused(lib.snn_planes_counts(ws, C.byref(v6), starts, 2, 128, 0, None, None, None, None), b"forms 11")
    refused(lib.snn_planes_counts(ws, C.byref(v6), (C.c_int64 * 3)(0, 6, 4), 2, 128, 4, None, None, None, None), b"group_row_start[2]")
    refused(lib.snn_planes_counts(ws, C.byref(v6), (C.c_int64 * 3)(0, 4, 11), 2, 128, 4, None, None, None, None), b"group_row_start[2]")
    refused(lib.snn_planes_counts(ws, C.byref(v6), None, 2, 128, 4, None, None, None, None), b"groups")
    refused(lib.snn_planes_counts(ws, C.byref(v6), starts, 2, 129, 4, None, None, None, None), b"n_cols")
    refused(lib.snn_planes_raster_rows(ws, None, 128, 4, None, None), b"snn_planes_raster_rows")
    refused(lib.snn_planes_raster_rows(ws, C.byref(v6), 128, 12, None, None), b"forms 11")
    refused(lib.snn_planes_raster_rows(ws, C.byref(v6), 0, 4, None, None), b"n_cols")
    refused(lib.snn_planes_raster_nchw(ws, None, 0, 1, 128, 2, 5, 4, None, None), b"snn_planes_raster_nchw")
    refused(lib.snn_planes_raster_nchw(ws, C.byref(v6), 0, 1, 128, 2, 5, 12, None, None), b"forms 11")
    refused(lib.snn_planes_raster_nchw(ws, C.byref(v6), 1, 1, 128, 2, 5, 4, None, None), b"outside the view")
    refused(lib.snn_planes_raster_nchw(ws, C.byref(v6), 0, 1, 129, 2, 5, 4, None, None), b"bad shape")
    bad = L.snn_planes_view(0, 10 * 4, 10, 4, 5, 8, 0)
    refused(lib.snn_planes_raster_rows(ws, C.byref(bad), 128, 4, None, None), b"layout")
    bad = L.snn_planes_view(0, 10 * 6, 10, 6, TP.SPLIT4, 8, 0)       # blocks of four words need words % 4 == 0
    refused(lib.snn_planes_raster_rows(ws, C.byref(bad), 128, 4, None, None), b"bad view")
    bad = L.snn_planes_view(0, 10 * 4 - 1, 10, 4, TP.ROWS, 8, 0)     # steps would overlap
    refused(lib.snn_planes_raster_rows(ws, C.byref(bad), 128, 4, None, None), b"bad view")


@pytest.mark.parametrize("T,rows,words", [(3, 5, 8), (2, 94, 4), (1, 1, 8), (4, 17, 3)])
def test_layout_restatement_matches_the_plane_helpers(T, rows, words):
    rng = np.random.default_rng(T * 1000 + rows * 10 + words)
    raw = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, size=T * rows * words, dtype=np.int64).astype(np.int32))
    flat = raw.numpy().view(np.uint32)
    assert np.array_equal(TP.rows_from_layout(flat, T, rows, words, TP.ROWS), rows_from_split(raw, T, rows, words, 0).numpy().view(np.uint32))
    assert np.array_equal(TP.rows_from_layout(flat, T, rows, words, TP.WORD_MAJOR),
                          rows_from_word_major(raw, T, rows, words, 1).contiguous().numpy().view(np.uint32))
    assert np.array_equal(TP.rows_from_layout(flat, T, rows, words, TP.ROWS), rows_from_word_major(raw, T, rows, words, 0).numpy().view(np.uint32))
    if words % 4 == 0:
        assert np.array_equal(TP.rows_from_layout(flat, T, rows, words, TP.SPLIT4),
                              rows_from_split(raw, T, rows, words, 1).contiguous().numpy().view(np.uint32))
    # a step stride beyond rows x words: the steps are read where the view says they start
    pad = np.concatenate([np.concatenate([flat[t * rows * words:(t + 1) * rows * words], np.full(7, 0xdeadbeef, np.uint32)]) for t in range(T)])
    assert np.array_equal(TP.rows_from_layout(pad, T, rows, words, TP.ROWS, rows * words + 7), TP.rows_from_layout(flat, T, rows, words, TP.ROWS))


def test_expected_counts_and_dense_on_a_hand_made_plane_set():
    rows = np.zeros((2, 3, 2), dtype=np.uint32)
    rows[0, 0, 0] = 0b101                  # step 0, row 0: columns 0 and 2
    rows[1, 2, 1] = 1 << 7 | 1 << 8        # step 1, row 2: column 39; bit 40 is padding at n_cols = 40
    spk = TP.dense(rows, 40)
    assert spk.shape == (2, 3, 40) and spk.sum() == 3 and spk[0, 0, 0] and spk[0, 0, 2] and spk[1, 2, 39]
    per_step, per_col, per_row = TP.expected_counts(spk, [1, 2])
    assert per_step.tolist() == [[2, 0], [0, 1]] and per_row.tolist() == [2, 0, 1]
    assert per_col[0].nonzero()[0].tolist() == [0, 2] and per_col[1].nonzero()[0].tolist() == [39]


def test_tapped_methods_exist_and_taps_stay_out_of_ops():
    """the bindings live in taps.py: tests/_graph_capture.py and tests/_ws_state.py pin every stream-taking function and workspace call
    site of ops.py"""
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import energy, ops, taps
    for cls, names in ((S.RPNHeadSNN, ("forward_tapped",)), (S.FastRCNNPredictorSNNFull, ("forward_tapped", "forward_roialign_tapped"))):
        for n in names:
            assert callable(getattr(cls, n))
    from snn_automotive_object_detection_amd.generalized_rcnn import GeneralizedRCNN
    from snn_automotive_object_detection_amd.roi_heads import RoIHeadsSNN
    assert callable(GeneralizedRCNN.forward_tapped) and callable(RoIHeadsSNN.forward_tapped) and callable(energy.rates_from_taps)
    assert callable(taps.planes_counts) and not [n for n in dir(ops) if "planes_counts" in n or "raster" in n or "tapped" in n]
    h = S.RPNHeadSNN(64, 3, 8)
    assert h.spike_rates is False
    with pytest.raises(Exception):                                   # CPU tensors: loud, as every product path
        h.forward_tapped([torch.randn(1, 64, 4, 4)])
    assert h.spike_rates is False
