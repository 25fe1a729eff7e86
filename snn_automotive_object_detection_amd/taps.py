"""Spike taps: the hidden LIF layers of a head pass - the RPN's shared LIF, the detector's lif6 and lif7 - as rasters (one byte per
spike) and activity statistics (spike counts per time step, per channel, per position / RoI), read on the GPU from the bit-planes the
pass left in its workspace (include/snn_hip.h: snn_*_planes_view, snn_planes_counts, snn_planes_raster_*).

A tapped pass IS the spike-rate-mode pass of the head (the existing entry, handed the spike-rate side outputs): it returns that pass's
outputs, counts and time sums bit for bit, whatever the module's ``spike_rates`` attribute says, and the attribute is not touched.  That
is the launch plan of spike-rate mode - every spike plane formed - and no promise about the launches of a plain forward.  Everything is
enqueued on the current stream without a host synchronisation; the planes are read before anything else is handed the workspace."""
import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib, ops
from ._lib import snn_planes_view, snn_params, snn_rpn_level


# ---- where the planes are (host-only) ------------------------------------------------------------------------------------------------
def rpn_planes_view(level_shapes: Sequence[Sequence[int]], C_: int, A: int, T: int, p: snn_params, route: str = "sparse",
                    spike_rates: bool = True) -> snn_planes_view:
    """the shared LIF's planes of an RPN head pass over levels of (N, H, W); nothing touches a device"""
    lv = (snn_rpn_level * len(level_shapes))(*[snn_rpn_level(None, int(n), int(h), int(w), 0) for n, h, w in level_shapes])
    v = snn_planes_view()
    _lib.check(_lib.load().snn_rpn_head_planes_view(lv, len(level_shapes), C_, A, T, C.byref(p), _lib.CONV_ROUTES[route], int(bool(spike_rates)),
                                                    C.byref(v)), "snn_rpn_head_planes_view")
    return v


def det_planes_views(R: int, D: int, Hd: int, K: int, K4: int, T: int, p: snn_params, w6_inner: int = 0, route: str = "sparse",
                     spike_rates: bool = True):
    """(lif6's view, lif7's view) of a detector head pass; nothing touches a device"""
    v6, v7 = snn_planes_view(), snn_planes_view()
    _lib.check(_lib.load().snn_det_head_planes_view(R, D, Hd, K, K4, T, C.byref(p), int(w6_inner), _lib.CONV_ROUTES[route],
                                                    int(bool(spike_rates)), C.byref(v6), C.byref(v7)), "snn_det_head_planes_view")
    return v6, v7


def _starts(rows_per_group: Sequence[int]):
    s = [0]
    for n in rows_per_group:
        s.append(s[-1] + int(n))
    return (C.c_int64 * len(s))(*s)


# ---- the three taps ------------------------------------------------------------------------------------------------------------------
def planes_counts(ws: torch.Tensor, view: snn_planes_view, rows_per_group: Sequence[int], n_cols: int, T: int):
    """spike counts of the steps t < T: (per_step int64 [T, groups], per_col int32 [groups, n_cols], per_row int32 [rows]); the groups are
    consecutive row ranges of the given lengths, from row 0.  The counters are unsigned 32-bit in the library; every plane set a head
    takes keeps them below 2^31"""
    ops._need_gpu(ws, "workspace")
    G = len(rows_per_group)
    per_step = torch.empty((T, G), dtype=torch.int64, device=ws.device)
    per_col = torch.empty((G, n_cols), dtype=torch.int32, device=ws.device)
    per_row = torch.empty((int(view.rows),), dtype=torch.int32, device=ws.device)
    _lib.check(_lib.load().snn_planes_counts(ops._ptr(ws), C.byref(view), _starts(rows_per_group), G, n_cols, T, ops._ptr(per_step),
                                             ops._ptr(per_col), ops._ptr(per_row), ops._stream()), "snn_planes_counts")
    return per_step, per_col, per_row


def planes_raster_nchw(ws: torch.Tensor, view: snn_planes_view, row0: int, N: int, C_: int, H: int, W: int, T: int) -> torch.Tensor:
    """one RPN level's spike train as torch.bool [T, N, C, H, W] (rows row0 .. row0 + N H W - 1 of the view)"""
    ops._need_gpu(ws, "workspace")
    out = torch.empty((T, N, C_, H, W), dtype=torch.uint8, device=ws.device)
    _lib.check(_lib.load().snn_planes_raster_nchw(ops._ptr(ws), C.byref(view), int(row0), N, C_, H, W, T, ops._ptr(out), ops._stream()),
               "snn_planes_raster_nchw")
    return out.view(torch.bool)


def planes_raster_rows(ws: torch.Tensor, view: snn_planes_view, n_cols: int, T: int) -> torch.Tensor:
    """a plane set's spike train as torch.bool [T, rows, n_cols]"""
    ops._need_gpu(ws, "workspace")
    out = torch.empty((T, int(view.rows), n_cols), dtype=torch.uint8, device=ws.device)
    _lib.check(_lib.load().snn_planes_raster_rows(ops._ptr(ws), C.byref(view), n_cols, T, ops._ptr(out), ops._stream()), "snn_planes_raster_rows")
    return out.view(torch.bool)


# ---- tapped head passes ----------------------------------------------------------------------------------------------------------------
def _current_ws(dev) -> torch.Tensor:
    """the workspace the head pass just ran in: ops hands out one buffer per (device, stream), grow-only"""
    return ops._WS.get(dev, 1)


@ops._on_tensor_device
def rpn_head_tapped(feats, C_: int, A: int, T: int, p: snn_params, w_shared_packed, w_heads_packed, raster: bool = False,
                    levels: Optional[Sequence[int]] = None):
    """ops.rpn_head_forward in spike-rate mode, then the taps of its shared LIF: (out_logits [P, A], out_bbox [P, 4A], level_rows, taps).
    taps["shared_lif"][l] = {"per_step" [N, T] int64, "per_channel" [N, C] int32, "per_position" [N, H, W] int32} and, with ``raster``
    for the levels of ``levels`` (None: all of them), "raster" [T, N, C, H, W] torch.bool; taps["pass"] = the pass's own counts and
    time sums with the shapes snn_rpn_rates needs (energy.rates_from_taps)."""
    shapes = [(int(f.shape[0]), int(f.shape[2]), int(f.shape[3])) for f in feats]
    out_l, out_b, rows, (counts, sum_l, sum_b, _) = ops.rpn_head_forward(list(feats), C_, A, T, p, w_shared_packed, w_heads_packed, spike_rates=True)
    view = rpn_planes_view(shapes, C_, A, T, p)
    ws = _current_ws(out_l.device)
    groups = [h * w for n, h, w in shapes for _ in range(n)]
    per_step, per_col, per_row = planes_counts(ws, view, groups, C_, T)
    want = range(len(shapes)) if levels is None else [int(l) for l in levels]
    per_level, g0, r0 = [], 0, 0
    for l, (n, h, w) in enumerate(shapes):
        d = {"per_step": per_step[:, g0:g0 + n].t(), "per_channel": per_col[g0:g0 + n], "per_position": per_row[r0:r0 + n * h * w].view(n, h, w)}
        if raster and l in want:
            d["raster"] = planes_raster_nchw(ws, view, r0, n, C_, h, w, T)
        per_level.append(d)
        g0, r0 = g0 + n, r0 + n * h * w
    taps = {"shared_lif": per_level,
            "pass": {"levels": shapes, "C": C_, "A": A, "T": T, "spike_counts": counts, "sum_logits": sum_l, "sum_bbox": sum_b}}
    return out_l, out_b, rows, taps


def _det_taps(dev, R: int, D: int, Hd: int, K: int, K4: int, T: int, p: snn_params, w6_inner: int, extras, raster: bool,
              rois_per_image: Optional[Sequence[int]], only_one_bbox: bool) -> Dict:
    groups = [R] if rois_per_image is None else [int(n) for n in rois_per_image]
    if sum(groups) != R or min(groups) < 0:
        raise ValueError("rois_per_image %r does not add up to the %d RoIs of the call" % (groups, R))
    taps = {"pass": {"D": D, "Hd": Hd, "K": K, "K4": K4, "T": T, "only_one_bbox": bool(only_one_bbox), "spk6_count": extras[0],
                     "spk7_count": extras[1], "sum_cls": extras[2], "sum_bbox": extras[3]}}
    if R == 0:                                                     # (no RoIs: no launch ran, nothing spiked)
        for name in ("lif6", "lif7"):
            taps[name] = {"per_step": torch.zeros((len(groups), T), dtype=torch.int64, device=dev),
                          "per_channel": torch.zeros((len(groups), Hd), dtype=torch.int32, device=dev),
                          "per_roi": torch.zeros((0,), dtype=torch.int32, device=dev)}
            if raster:
                taps[name]["raster"] = torch.zeros((T, 0, Hd), dtype=torch.bool, device=dev)
        return taps
    ws = _current_ws(dev)
    for name, view in zip(("lif6", "lif7"), det_planes_views(R, D, Hd, K, K4, T, p, w6_inner)):
        per_step, per_col, per_row = planes_counts(ws, view, groups, Hd, T)
        taps[name] = {"per_step": per_step.t(), "per_channel": per_col, "per_roi": per_row}
        if raster:
            taps[name]["raster"] = planes_raster_rows(ws, view, Hd, T)
    return taps


@ops._on_tensor_device
def det_head_tapped(x, Hd: int, K: int, K4: int, T: int, p: snn_params, w6_packed, w7_packed, w_heads_packed, w6_inner: int = 0,
                    raster: bool = False, rois_per_image: Optional[Sequence[int]] = None, only_one_bbox: bool = False, **_):
    """ops.det_head_forward in spike-rate mode, then the taps of lif6 and lif7: (out_cls [R, K], out_bbox [R, K4], taps).
    taps["lif6"] / taps["lif7"] = {"per_step" [n_images, T] int64, "per_channel" [n_images, Hd] int32, "per_roi" [R] int32} and, with
    ``raster``, "raster" [T, R, Hd] torch.bool; ``rois_per_image``: consecutive RoIs per image (None: one image); taps["pass"] = the
    pass's own counts and time sums with the shapes snn_det_rates needs."""
    x = x.flatten(1)
    out_cls, out_bbox, extras = ops.det_head_forward(x, Hd, K, K4, T, p, w6_packed, w7_packed, w_heads_packed, spike_rates=True, w6_inner=w6_inner)
    R, D = int(x.shape[0]), int(x.shape[1])
    return out_cls, out_bbox, _det_taps(out_cls.device, R, D, Hd, K, K4, T, p, w6_inner, extras, raster, rois_per_image, only_one_bbox)


@ops._on_tensor_device
def det_head_roialign_tapped(feats, scales, rois, roi_batch, roi_level, Hd: int, K: int, K4: int, T: int, p: snn_params, w6_packed,
                             w7_packed, w_heads_packed, w6_inner: int = 0, raster: bool = False,
                             rois_per_image: Optional[Sequence[int]] = None, only_one_bbox: bool = False, **_):
    """det_head_tapped for the head fed by the fused RoIAlign encoder (ops.det_head_forward_roialign in spike-rate mode)"""
    out_cls, out_bbox, extras = ops.det_head_forward_roialign(feats, scales, rois, roi_batch, roi_level, Hd, K, K4, T, p, w6_packed, w7_packed,
                                                              w_heads_packed, spike_rates=True, w6_inner=w6_inner)
    D = int(feats[0].shape[1]) * 49
    return out_cls, out_bbox, _det_taps(out_cls.device, out_cls.shape[0], D, Hd, K, K4, T, p, w6_inner, extras, raster, rois_per_image,
                                        only_one_bbox)


# ---- the rate rows of spike-rate mode from a tapped pass ------------------------------------------------------------------------------
def rpn_rate_list(taps: Dict) -> List[torch.Tensor]:
    """what RPNHeadSNN.forward returns as its third value in spike-rate mode (three [N, 2] = (rate, FLOPs) tensors per level), from the
    counts and time sums of a tapped pass through snn_rpn_rates"""
    ps = taps["pass"]
    shapes = ps["levels"]
    lv = (snn_rpn_level * len(shapes))(*[snn_rpn_level(None, n, h, w, 0) for n, h, w in shapes])
    max_n = max(n for n, _, _ in shapes)
    counts = ps["spike_counts"]
    with torch.cuda.device(counts.device):
        rows = ops._rpn_rates(_lib.load(), lv, len(shapes), ps["C"], ps["A"], ps["T"], max_n, counts, ps["sum_logits"], ps["sum_bbox"], counts.device)
    return [rows[l, j, :n] for l, (n, _, _) in enumerate(shapes) for j in range(3)]


def det_rate_list(taps: Dict) -> List[torch.Tensor]:
    """what FastRCNNPredictorSNNFull.forward returns in spike-rate mode (four [R, 2] tensors), through snn_det_rates"""
    ps = taps["pass"]
    rates = ops.det_rates((ps["spk6_count"], ps["spk7_count"], ps["sum_cls"], ps["sum_bbox"]), ps["D"], ps["Hd"], ps["K"], ps["K4"], ps["T"],
                          ps["only_one_bbox"])
    return [rates[0], rates[1], rates[2], rates[3]]
