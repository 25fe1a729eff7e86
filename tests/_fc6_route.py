"""The fc6 route of the detector head (include/snn_hip.h: snn_det_head_forward_routed): the density statistic restated in
numpy, and the plumbing the GPU tests share.

Rows are the R RoIs.  fc6 reads its period planes in the bin-major reduction order k' = bin * C + c (bin = 0 .. 48 of the 7 x 7 RoI window; the
flattened features run k = c * 49 + bin).  BLOCK = 16 consecutive RoIs, cut every 16 rows from row 0 (the last one may be short) x one 64-k
word pair of that order (D / 64 of them) x one compressed period plane e_n, n = 3 .. T - 2 (fc6's window of a plain forward: it forms the
currents of steps 0 .. T - 3).  HIT = a block in which some row holds, in some nibble (four consecutive k') of that word pair, three or four
neurons of period n - the rows whose secondary-occupancy dword is non-zero.  The restatement starts from the oracle's encoder spike TRAINS (a
neuron's period is the step of its first spike + 1), not from any plane the library wrote."""
import ctypes as Ct
import hashlib
from typing import Tuple

import numpy as np
import torch

from tests._conv_route import periods_from_trains


# ---- the restatement (host only) -------------------------------------------------------------------------------------------------------
def bin_major(per: np.ndarray, C: int) -> np.ndarray:
    """[R, C * 49] in the flattened order k = c * 49 + bin -> the same values in fc6's order k' = bin * C + c"""
    R = per.shape[0]
    return np.ascontiguousarray(per.reshape(R, C, 49).transpose(0, 2, 1)).reshape(R, 49 * C)


def fc6_planes(T: int) -> range:
    """the compressed planes of a plain forward at T steps: e_3 .. e_(T - 2)"""
    return range(3, T - 1)


def secondary_rows(period_rows: np.ndarray, n: int) -> np.ndarray:
    """int [R, D] periods in bin-major order (D a multiple of 64) -> bool [R, D / 64]: row r has a secondary entry in word pair w of plane
    e_n, i.e. a nibble of k' = 64 w .. 64 w + 63 holding >= 3 neurons of period n"""
    R, D = period_rows.shape
    assert D % 64 == 0
    nib = (period_rows == n).reshape(R, D // 4, 4).sum(axis=2) >= 3
    return nib.reshape(R, D // 64, 16).any(axis=2)


def count_blocks(period_rows: np.ndarray, T: int) -> Tuple[int, int]:
    """(hits, blocks) over the planes e_3 .. e_(T - 2)"""
    R, D = period_rows.shape
    nblk = (R + 15) // 16
    pairs = D // 64
    hits = 0
    for n in fc6_planes(T):
        pad = np.zeros((nblk * 16, pairs), dtype=bool)
        pad[:R] = secondary_rows(period_rows, n)
        hits += int(pad.reshape(nblk, 16, pairs).any(axis=1).sum())
    return hits, nblk * pairs * len(fc6_planes(T))


def route_counts(x: torch.Tensor, T: int) -> Tuple[int, int]:
    """(hits, blocks) of RoI features [R, C, 7, 7] at T steps, periods from the oracle's encoder trains"""
    from oracle import snn_oracle as OR
    R, C = x.shape[0], x.shape[1]
    z = OR.encoder_spikes(x.float().flatten(1), T).numpy()
    return count_blocks(bin_major(periods_from_trains(z), C), T)


def route_of(hits: int, blocks: int, crossover: float) -> int:
    """the device's decision, in fp32 as stated in snn_hip.h"""
    return int(np.float32(hits) > np.float32(crossover) * np.float32(blocks))


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def silent_like(x: torch.Tensor) -> torch.Tensor:
    return torch.zeros_like(x)


def mixed_like(full: torch.Tensor) -> torch.Tensor:
    """full-nibble values on rows 15 .. 17 only (the last row of block 0, the first two of block 1), silence everywhere else"""
    out = torch.zeros_like(full)
    out[15:18] = full[15:18]
    return out


def decided_inputs():
    """the inputs the tests decide on at the header's crossover, (name, features [29, 64, 7, 7] for T = 8, expected route): full-nibble
    features (every plane of fc6's window live: hit rate 1) and N(0, 1) features (0.17) take the dense side, silent and N(0, 4) features (0.010:
    most neurons fire at once, on the dense planes e_1, e_2) the sparse side.  tests/test_fc6_route_cpu.py checks that each lies at least 0.05 from
    the header's crossover"""
    from tests._exact_grid import full_nibble_values
    full = full_nibble_values((29, 64, 7, 7), 8, torch.Generator().manual_seed(29 + 8))
    randn = torch.randn(29, 64, 7, 7, generator=torch.Generator().manual_seed(208))
    return [("full", full, 1), ("randn_1", randn, 1), ("silent", silent_like(full), 0), ("randn_4", randn * 4.0, 0)]


# ---- GPU plumbing ----------------------------------------------------------------------------------------------------------------------
def head_for(case: dict, dev, precision: str):
    import snn_automotive_object_detection_amd as pkg
    d = pkg.FastRCNNPredictorSNNFull(case["C"] * 49, case["Hd"], case["K"], case["T"]).to(dev)
    d.precision, d.li_order = precision, case["li_order"]
    d.load_state_dict({"fc6.weight": case["w6"], "fc7.weight": case["w7"], "cls_score.weight": case["w_cls"], "bbox_pred.weight": case["w_bbox"]})
    return d


def forward(d, x, route, crossover=None, roi=None) -> dict:
    """one forward of the head module on `route` (None: the plain entry) -> outputs, lif6 / lif7 planes as rows [T, R, Hd / 32] (lif6's last
    step is never formed by a plain forward and is left out), route_stat as a list (None on the plain entry) and the launch fc6 reported.
    ``roi`` = (flist, scales, rois, lvl): the RoIAlign-fed forward (x is ignored)"""
    from snn_automotive_object_detection_amd import _lib
    from tests._planes import head_det_planes
    d.fc6_route, d.fc6_crossover = route, crossover
    try:
        out = d.forward_roialign(*roi) if roi is not None else d(x)
    finally:
        d.fc6_route, d.fc6_crossover = None, None
    R = int(roi[2].shape[0]) if roi is not None else int(x.shape[0])
    T = int(d.num_steps)
    tensors = [t.contiguous().clone() for t in out]
    path = _lib.load().snn_debug_last_fc6_path()
    p6, p7 = head_det_planes(x.device if roi is None else roi[2].device, T, d.representation_size, R)
    n6 = T if d.spike_rates else T - 1
    stat = None if d.route_stat is None else d.route_stat.cpu().tolist()
    res = dict(out=tensors, p6=p6[:n6].clone(), p7=p7.clone(), stat=stat, path=path)
    if route == "sparse":
        # the module's "sparse" IS the plain entry (no route_stat); the routed entry with SNN_ROUTE_SPARSE must give the same bits: run it as well
        from snn_automotive_object_detection_amd import ops
        dev = x.device if roi is None else roi[2].device
        st = torch.full((4,), -7, dtype=torch.int32, device=dev)
        kw = dict(T=T, fc6_route="sparse", route_stat=st)
        if roi is not None:
            flist, scales, rois, lvl = roi
            cls, bbox, extras = ops.det_head_forward_roialign(flist, scales, rois[:, 1:5], rois[:, 0], lvl, **kw,
                                                              **d._pass_args(flist[0].shape[1] * 49, "maps"))
        else:
            xr = x.flatten(1)
            cls, bbox, extras = ops.det_head_forward(xr, **kw, **d._pass_args(xr.shape[1], "rows"))
        assert _lib.load().snn_debug_last_fc6_path() == path
        q6, q7 = head_det_planes(dev, T, d.representation_size, R)
        assert torch.equal(q6[:n6], res["p6"]) and torch.equal(q7, res["p7"])
        if d.spike_rates:
            assert all(torch.equal(a, b) for a, b in zip(extras[:2], d.last_spike_counts))
        else:
            assert torch.equal(cls, tensors[0]) and torch.equal(bbox, tensors[1])
        res["stat"] = st.cpu().tolist()
    return res


def same_bits(a: dict, b: dict) -> bool:
    return (len(a["out"]) == len(b["out"]) and all(torch.equal(x, y) for x, y in zip(a["out"], b["out"])) and torch.equal(a["p6"], b["p6"])
            and torch.equal(a["p7"], b["p7"]))


def digest(r: dict) -> str:
    h = hashlib.sha256()
    for t in r["out"] + [r["p6"], r["p7"]]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def raw_call(lib, d, x, route, crossover, stat, ws, ws_bytes=None):
    """snn_det_head_forward_routed on fp32 rows with every argument spelled out -> (return code, out_cls, out_bbox)"""
    from snn_automotive_object_detection_amd import ops
    x = x.flatten(1).contiguous()
    R, D = x.shape
    a = d._pass_args(D, "%d" % D)
    out_c = torch.zeros((R, a["K"]), dtype=torch.float32, device=x.device)
    out_b = torch.zeros((R, a["K4"]), dtype=torch.float32, device=x.device)
    rc = lib.snn_det_head_forward_routed(ops._ptr(x), 0, R, D, a["Hd"], a["K"], a["K4"], int(d.num_steps), Ct.byref(a["p"]), ops._ptr(a["w6_packed"]),
                                         a["w6_inner"], ops._ptr(a["w7_packed"]), ops._ptr(a["w_heads_packed"]), ops._ptr(out_c), ops._ptr(out_b),
                                         None, None, None, None, ops._ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, route, crossover,
                                         ops._ptr(stat), ops._stream())
    return rc, out_c, out_b


# ---- the RoIAlign feed of the GPU tests: a two-level pyramid, 2 images ------------------------------------------------------------------
ROI_LEVELS = ((48, 80), (24, 40))
ROI_IMAGE = (192, 320)


def roi_setup(C: int, R: int, seed: int, scale: float = 2.0):
    """(pooler, {name: [2, C, H, W]} fp32 CPU maps, boxes per image, image shapes): boxes of 4 .. 300 px, both levels in use"""
    from snn_automotive_object_detection_amd.stock.roi_align import MultiScaleRoIAlign
    g = torch.Generator().manual_seed(seed)
    feats = {str(i): torch.randn((2, C, h, w), generator=g) * scale for i, (h, w) in enumerate(ROI_LEVELS)}
    boxes = []
    for n, k in enumerate((R - R // 2, R // 2)):
        xy = torch.rand((k, 2), generator=g) * torch.tensor([240.0, 140.0])
        wh = torch.exp(torch.rand((k, 2), generator=g) * 4.3 + 1.4)
        boxes.append(torch.cat([xy, torch.minimum(xy + wh, torch.tensor([319.0, 191.0]))], dim=1))
    return MultiScaleRoIAlign(["0", "1"], 7, 2), feats, boxes, [ROI_IMAGE] * 2


def roi_pooled(feats, boxes, shapes) -> torch.Tensor:
    """the RoI features [R, C, 7, 7] the fused kernel pools, from the CPU restatement of torchvision's roi_align (bit-identical:
    tests/test_gpu_roialign.py)"""
    from oracle import roi_align_oracle as RA
    return RA.multiscale_roi_align({k: v.float() for k, v in feats.items()}, boxes, shapes, featmap_names=("0", "1"))


# ---- child process of tests/test_gpu_fc6_route.py -----------------------------------------------------------------------------------------
def _child(mode, cases):
    """the plain detector forward (fc6_route None) on exact-grid cases under the environment the parent set before the library read its
    knobs (SNN_SPARSE=0, or SNN_FC6_ROUTE=auto).  Prints one JSON line: per case the launch fc6 reported, route_stat and a digest of outputs
    and hidden planes."""
    import json
    from tests import _exact_grid as G
    dev = torch.device("cuda:0")
    out = {}
    for name, R, T, precision in cases:
        case = G.det_case(R, 64, 128, 9, T, 600 + R + T, "narrow" if precision == "bf16" else "wide", full_nibble=name.startswith("full"))
        d = head_for(case, dev, precision)
        r = forward(d, case["x"].to(dev), None)
        out[name] = dict(path=r["path"], stat=r["stat"], digest=digest(r), mode=mode)
    print(json.dumps(out))


if __name__ == "__main__":
    import json
    import sys
    _child(sys.argv[1], json.loads(sys.argv[2]))
