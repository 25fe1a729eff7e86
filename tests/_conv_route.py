"""The conv route of the RPN head (include/snn_hip.h: snn_rpn_head_forward_routed): the density statistic restated in numpy,
and the plumbing the GPU tests share.

BLOCK = 16 consecutive rows of the encoder's padded row space (aligned to 16 within the Pe rows of a word plane) x one 64-channel word pair
x one compressed period plane e_n, n = 3 .. T - 1.  HIT = a block in which some row holds, in some nibble (four consecutive channels) of
that word pair, three or four neurons of period n - the rows whose secondary-occupancy dword is non-zero.  The restatement starts from
the oracle's encoder spike TRAINS (a neuron's period is the step of its first spike + 1), not from any plane the library wrote.

Padded row order: levels back to back; inside a level image by image; an image is (H + 2) x (W + 2) rows, row (n, y, x) at
(n (H + 2) + y + 1)(W + 2) + x + 1; halo rows are silent.  Blocks are cut from the concatenation, so they run across image and level
boundaries, and the last one may be short."""
import ctypes as Ct
import hashlib
from typing import List, Sequence, Tuple

import numpy as np
import torch


# ---- the restatement (host only) -------------------------------------------------------------------------------------------------------
def periods_from_trains(z: np.ndarray) -> np.ndarray:
    """z {0, 1} [T, ...] encoder spike trains -> int [...]: the neuron's period n (first spike at step n - 1), 0 if it never fires"""
    fired = z > 0
    return np.where(fired.any(axis=0), fired.argmax(axis=0) + 1, 0)


def padded_rows(per_level: Sequence[np.ndarray]) -> np.ndarray:
    """per level an int array [N, C, H, W] -> [Pe, C]: the padded row space, halo rows zero"""
    out = []
    for a in per_level:
        N, C, H, W = a.shape
        p = np.zeros((N, H + 2, W + 2, C), dtype=a.dtype)
        p[:, 1:H + 1, 1:W + 1] = a.transpose(0, 2, 3, 1)
        out.append(p.reshape(N * (H + 2) * (W + 2), C))
    return np.concatenate(out, axis=0)


def secondary_rows(period_rows: np.ndarray, n: int) -> np.ndarray:
    """int [Pe, C] periods -> bool [Pe, ceil(C / 64)]: row r has a secondary entry in word pair w of plane e_n, i.e. a nibble of channels
    64 w .. 64 w + 63 holding >= 3 neurons of period n (channels past C are silent)"""
    Pe, C = period_rows.shape
    Cp = (C + 63) // 64 * 64
    e = np.zeros((Pe, Cp), dtype=np.int64)
    e[:, :C] = period_rows == n
    nib = e.reshape(Pe, Cp // 4, 4).sum(axis=2) >= 3
    return nib.reshape(Pe, Cp // 64, 16).any(axis=2)


def count_blocks(period_rows: np.ndarray, T: int) -> Tuple[int, int]:
    """(hits, blocks) over the planes e_3 .. e_(T-1)"""
    Pe, C = period_rows.shape
    nblk = (Pe + 15) // 16
    pairs = (C + 63) // 64
    hits = 0
    for n in range(3, T):
        sec = secondary_rows(period_rows, n)
        pad = np.zeros((nblk * 16, pairs), dtype=bool)
        pad[:Pe] = sec
        hits += int(pad.reshape(nblk, 16, pairs).any(axis=1).sum())
    return hits, nblk * pairs * max(T - 3, 0)


def route_counts(feats: Sequence[torch.Tensor], T: int) -> Tuple[int, int]:
    """(hits, blocks) of a pyramid of feature maps [N, C, H, W] at T steps, periods from the oracle's encoder trains"""
    from oracle import snn_oracle as OR
    per = [periods_from_trains(OR.encoder_spikes(f.float(), T).numpy()) for f in feats]
    return count_blocks(padded_rows(per), T)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def silent_maps(C: int, shapes, N: int) -> List[torch.Tensor]:
    return [torch.zeros(N, C, h, w) for h, w in shapes]


def full_nibble_maps(C: int, T: int, shapes, N: int, seed: int) -> List[torch.Tensor]:
    from tests._exact_grid import full_nibble_values
    g = torch.Generator().manual_seed(seed)
    return [full_nibble_values((N, C, h, w), T, g) for h, w in shapes]


def mixed_maps(C: int, T: int, shapes, N: int, seed: int) -> List[torch.Tensor]:
    """silent maps with full-nibble values on a few patches: the second and third row of image 0 of level 0 (runs of 17 positions that
    straddle 16-row blocks and leave the halo rows above them empty), one position of image 1, all of the last level; everywhere else -
    whole halo-only blocks included - nothing fires"""
    full = full_nibble_maps(C, T, shapes, N, seed)
    out = silent_maps(C, shapes, N)
    out[0][0, :, 1:3, :] = full[0][0, :, 1:3, :]
    out[0][N - 1, :, shapes[0][0] - 1, 3] = full[0][N - 1, :, shapes[0][0] - 1, 3]
    out[-1][:] = full[-1]
    return out


# ---- GPU plumbing ----------------------------------------------------------------------------------------------------------------------
def head_for(case: dict, dev, precision: str):
    import snn_automotive_object_detection_amd as pkg
    m = pkg.RPNHeadSNN(case["C"], case["A"], case["T"]).to(dev)
    m.precision, m.li_order = precision, case["li_order"]
    m.load_state_dict({"shared_conv.weight": case["w_shared"], "conv_cls.weight": case["w_cls"], "conv_bbox.weight": case["w_bbox"]})
    return m


def forward(m, feats, route, crossover=None) -> dict:
    """one forward of the head module on `route` (None: the plain entry) -> outputs (per level logits then box deltas), the hidden planes
    as rows [T, P, C / 32], route_stat as a list (None on the plain entry) and the launch the conv reported.  "sparse" runs twice: through
    the module (the plain entry) and through the routed entry, which must agree bit for bit; route_stat is the routed entry's"""
    from snn_automotive_object_detection_amd import _lib
    from tests._planes import head_rpn_planes
    m.conv_route, m.conv_crossover = route, crossover
    out = m(feats)
    planes = head_rpn_planes(feats[0].device, int(m.num_steps), m.in_channels)
    path = _lib.load().snn_debug_last_conv_path()
    stat = None if m.route_stat is None else m.route_stat.cpu().tolist()
    tensors = [t.contiguous().clone() for t in list(out[0]) + list(out[1])]
    if len(out) == 3:
        tensors += [t.contiguous().clone() for t in out[2]]
    if route == "sparse":
        # the module's "sparse" IS the plain entry (no route_stat); the routed entry with SNN_ROUTE_SPARSE must give the same bits: run it as well
        from snn_automotive_object_detection_amd import ops
        C_, A, p, w_shared, w_heads = m._pass_args()
        st = torch.full((4,), -7, dtype=torch.int32, device=feats[0].device)
        out_l, out_b, rows, _ = ops.rpn_head_forward(list(feats), C_, A, int(m.num_steps), p, w_shared, w_heads, spike_rates=m.spike_rates,
                                                     conv_route="sparse", route_stat=st)
        assert _lib.load().snn_debug_last_conv_path() == path
        assert torch.equal(head_rpn_planes(feats[0].device, int(m.num_steps), m.in_channels), planes)
        L, pos = len(feats), 0
        for l, f in enumerate(feats):
            N, H, W = f.shape[0], f.shape[2], f.shape[3]
            assert torch.equal(out_l[pos:pos + rows[l]].view(N, H, W, A).permute(0, 3, 1, 2), tensors[l])
            assert torch.equal(out_b[pos:pos + rows[l]].view(N, H, W, 4 * A).permute(0, 3, 1, 2), tensors[L + l])
            pos += rows[l]
        stat = st.cpu().tolist()
    return dict(out=tensors, planes=planes, stat=stat, path=path)


def same_bits(a: dict, b: dict) -> bool:
    return len(a["out"]) == len(b["out"]) and all(torch.equal(x, y) for x, y in zip(a["out"], b["out"])) and torch.equal(a["planes"], b["planes"])


def digest(r: dict) -> str:
    h = hashlib.sha256()
    for t in r["out"] + [r["planes"]]:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def raw_call(lib, feats, C_, A, T, p, w_shared, w_heads, route, crossover, stat, ws, ws_bytes=None):
    """snn_rpn_head_forward_routed on fp32 NCHW maps with every argument spelled out -> its return code"""
    from snn_automotive_object_detection_amd import ops
    lv = ops._rpn_table(feats)
    P = sum(f.shape[0] * f.shape[2] * f.shape[3] for f in feats)
    out_l = torch.zeros((P, A), dtype=torch.float32, device=feats[0].device)
    out_b = torch.zeros((P, 4 * A), dtype=torch.float32, device=feats[0].device)
    rc = lib.snn_rpn_head_forward_routed(lv, 0, len(feats), C_, A, T, Ct.byref(p), ops._ptr(w_shared), ops._ptr(w_heads), ops._ptr(out_l),
                                         ops._ptr(out_b), None, None, None, ops._ptr(ws), ws.numel() if ws_bytes is None else ws_bytes,
                                         route, crossover, ops._ptr(stat), ops._stream())
    return rc, out_l, out_b
