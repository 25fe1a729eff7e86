"""The seven stream-only training entries under the memory-extent contract of tests/_ws_state.py (test infrastructure).

  snn_li_heads_wgrad (readout.py)   snn_match_targets, snn_rpn_loss_grad, snn_det_loss_grad (losses.py)
  snn_planes_to_rows, snn_lif_surrogate_bwd, snn_spike_linear_wgrad (hidden.py)

A spec is a plain dict (li / sw / lif / p2r / match / rpnl / detl below; nothing is built at collection time).  Each entry has three parts:
  prepare(spec) -> host case   the smallest of the suite's exact builders: tests/_readout_grad.exact_case, tests/_hidden_grad.exact_wgrad_case,
                               the fp64 / fp32 adjoint of tests/_hidden_grad.py, the restated matcher and losses of tests/_head_losses.py, the index
                               arithmetic of tests/_taps.word_index - with the padding the value tests use left on (NaN in the ldc / ldd padding
                               columns, plane padding bits set, view offsets and step strides with slack).  host["inputs"] / host["outputs"]
                               name every operand; the plane buffers end on the last word of the last step that is read;
  CALLS[entry](spec, host, ins, outs)   ONE wrapper call on device operands (snn_planes_to_rows has no `out=`: the C entry through ctypes);
  EXPECT[entry](spec, host, outs)       the fp64 or integer expectation on what came back.
run(spec, dev, in_guard) stages every operand in a _ws_state.Guarded allocation of its own ([guard | payload | guard], outputs poisoned, inputs
between guards of `in_guard` bytes), calls, verifies guards / inputs / unwritten elements, checks the expectation and returns the snapshot:
every output tensor, as bits.  The scratch of a call is whatever readout._WS_WGRAD / hidden._WS_WGRAD / losses._WS_LOSS hand out: the GPU file
installs _ws_state.GuardedWorkspace objects there.

TRAIN_ENTRIES maps each entry to (module, seam attribute, size query); tests/test_train_entries_cpu.py pins it to the `.get(` call sites of
the three modules and asks the size queries about every shape listed here."""
import ctypes as C
import functools

import numpy as np
import torch

from tests import _head_losses as HL
from tests import _hidden_grad as HG
from tests import _li_grid as L
from tests import _neuron_constants as NC
from tests import _readout_grad as RG
from tests import _taps as TP
from tests import _ws_state as W

#                 entry                      module     seam attribute  size query
TRAIN_ENTRIES = {
    "snn_li_heads_wgrad": ("readout", "_WS_WGRAD", "snn_li_heads_wgrad_workspace_bytes"),
    "snn_match_targets": ("losses", "_WS_LOSS", "snn_match_targets_workspace_bytes"),
    "snn_rpn_loss_grad": ("losses", "_WS_LOSS", "snn_rpn_loss_grad_workspace_bytes"),
    "snn_det_loss_grad": ("losses", "_WS_LOSS", "snn_det_loss_grad_workspace_bytes"),
    "snn_planes_to_rows": ("hidden", None, None),
    "snn_lif_surrogate_bwd": ("hidden", None, None),
    "snn_spike_linear_wgrad": ("hidden", "_WS_WGRAD", "snn_spike_linear_wgrad_workspace_bytes"),
}
SEAMS = (("readout", "_WS_WGRAD"), ("hidden", "_WS_WGRAD"), ("losses", "_WS_LOSS"))
SEAM_INTERIOR = 4 << 20                  # bytes of a GuardedWorkspace at a seam: the largest scratch below is under 1 MiB

RPN_T, DET_T = (0.7, 0.3), (0.5, 0.5)
RPN_W, DET_W = (1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)


def cdiv(a, b):
    return (a + b - 1) // b


# ---- specs ---------------------------------------------------------------------------------------------------------------------------------
def li(rows, n_cols, layout, NA, NB, acc=0, slack=0, name="a2_b2", T=8, order="jump_first"):
    """snn_li_heads_wgrad at T' = T (the last plane that is read is the last one of the buffer)"""
    return dict(entry="snn_li_heads_wgrad", rows=rows, n_cols=n_cols, layout=layout, NA=NA, NB=NB, acc=acc, slack=slack, name=name, T=T, order=order)


def sw(K, N, rows, Tp, acc=0, density=0.3):
    return dict(entry="snn_spike_linear_wgrad", K=K, N=N, rows=rows, Tp=Tp, acc=acc, density=density)


def lif(R, N, Tc, order="jump_first", mode="both", alpha=100.0, cname="reference", rate=0.5):
    return dict(entry="snn_lif_surrogate_bwd", R=R, N=N, Tc=Tc, order=order, mode=mode, alpha=alpha, cname=cname, rate=rate)


def p2r(layout, rows, words, Tp=3):
    return dict(entry="snn_planes_to_rows", layout=layout, rows=rows, words=words, Tp=Tp)


def match(images, mode="rpn", lq=1):
    """images: ((boxes, ground-truth boxes), ..) per image"""
    return dict(entry="snn_match_targets", images=tuple(tuple(i) for i in images), mode=mode, lq=lq)


def rpnl(shapes, N, A):
    return dict(entry="snn_rpn_loss_grad", shapes=tuple(tuple(s) for s in shapes), N=N, A=A)


def detl(R, K, ignore=0):
    return dict(entry="snn_det_loss_grad", R=R, K=K, ignore=ignore)


def _short(v):
    if isinstance(v, tuple):
        return "x".join(_short(x) for x in v) if len(v) <= 6 else "%dof_%s" % (len(v), _short(v[:2]))
    return ("%g" % v) if isinstance(v, float) else str(v)


def spec_id(s) -> str:
    return s["entry"][4:] + "-" + "-".join("%s%s" % (k, _short(v)) for k, v in s.items() if k != "entry")


def key(s):
    return tuple(sorted(s.items()))


# ---- the size queries, restated (tests/test_train_entries_cpu.py holds the library to them) ------------------------------------------------
WG_ROWS, WG_MAX_SLABS = 64, 512
SW_SLAB_ROWS, SW_MAX_SLABS, SW_BATCH = 512, 16, 8
LS_BLOCK, LS_MAX_GT, LS_HEADER, DL_ROWS = 256, 256, 64, 16


def sw_slabs(M: int):
    """spike_wgrad_slabs restated: (slabs, rows of every slab but the last) - a function of M = T' x rows alone"""
    want = min(cdiv(M, SW_SLAB_ROWS), SW_MAX_SLABS)
    per = cdiv(cdiv(M, want), SW_BATCH) * SW_BATCH
    return cdiv(M, per), per


def sw_classes(rows: int, Tp: int):
    """the classes of a reduction length the edge list must cover"""
    M = rows * Tp
    slabs, per = sw_slabs(M)
    out = set()
    if M < SW_BATCH:
        out.add("tail_only")
    if M in (8, 9, 16, 17):
        out.add("M%d" % M)
    if M == SW_SLAB_ROWS:
        out.add("one_slab")
    if M == SW_SLAB_ROWS + 1:
        out.add("two_slabs")
    if SW_MAX_SLABS * SW_SLAB_ROWS < M <= SW_MAX_SLABS * SW_SLAB_ROWS + 64:
        out.add("slab_cap")
    if Tp > 1 and min(per, M) > rows:
        out.add("slab_spans_a_step")
    return out


SW_CLASSES = {"tail_only", "M8", "M9", "M16", "M17", "one_slab", "two_slabs", "slab_cap", "slab_spans_a_step"}


def _shapes_of(s):
    return [(s["N"], h, w) for h, w in s["shapes"]]


def _anchors(s):
    return sum(n * h * w for n, h, w in _shapes_of(s)) * s["A"]


def restated_bytes(s) -> int:
    """what the size query of the spec's entry must return (0: the entry takes no scratch)"""
    e = s["entry"]
    if e == "snn_li_heads_wgrad":
        return min(cdiv(s["rows"], WG_ROWS), WG_MAX_SLABS) * (s["NA"] + s["NB"]) * s["n_cols"] * 4
    if e == "snn_spike_linear_wgrad":
        return sw_slabs(s["rows"] * s["Tp"])[0] * s["N"] * s["K"] * 4
    if e == "snn_match_targets":
        total = sum(b for b, _ in s["images"])
        return (total // LS_BLOCK + 2 * len(s["images"])) * LS_MAX_GT * 4
    if e == "snn_rpn_loss_grad":
        return LS_HEADER + cdiv(_anchors(s), LS_BLOCK) * 24
    if e == "snn_det_loss_grad":
        return LS_HEADER + cdiv(s["R"], DL_ROWS) * 24
    return 0


def queried_bytes(lib, s) -> int:
    e = s["entry"]
    if e == "snn_li_heads_wgrad":
        return lib.snn_li_heads_wgrad_workspace_bytes(s["rows"], s["n_cols"], s["NA"], s["NB"])
    if e == "snn_spike_linear_wgrad":
        return lib.snn_spike_linear_wgrad_workspace_bytes(s["rows"], s["K"], s["N"], s["Tp"])
    if e == "snn_match_targets":
        return lib.snn_match_targets_workspace_bytes(sum(b for b, _ in s["images"]), len(s["images"]))
    if e == "snn_rpn_loss_grad":
        return lib.snn_rpn_loss_grad_workspace_bytes(_anchors(s))
    if e == "snn_det_loss_grad":
        return lib.snn_det_loss_grad_workspace_bytes(s["R"], s["K"])
    return 0


# ---- snn_li_heads_wgrad ----------------------------------------------------------------------------------------------------------------------
def _prep_li(s):
    c = RG.exact_case(rows=s["rows"], n_cols=s["n_cols"], layout=s["layout"], NA=s["NA"], NB=s["NB"], name=s["name"], T=s["T"], Tp=s["T"],
                      li_order=s["order"], extra_words=1 if s["slack"] & 1 else 0, pad_stride=7 if s["slack"] & 2 else 0,
                      offset_bytes=132 if s["slack"] & 4 else 0)
    v, NA, NB, acc = c["view"], s["NA"], s["NB"], s["acc"]
    end = v["offset"] // 4 + (s["T"] - 1) * v["stride"] + v["rows"] * v["words"]      # the last word of the last plane: flush against the guard
    planes = torch.from_numpy(c["flat"][:end].view(np.uint8).copy())
    S = RG.fold_units(c["spk"], c["ku"])
    assert RG.demand_units(c["g"], S).max(initial=0) + RG.PRIOR < RG.BUDGET
    shift = c["fb"] + RG.G_SHIFT
    want = RG.units_to_fp32(RG.expect_units(c["g"], S) + (c["prior"] if acc else 0), shift)
    g = torch.from_numpy((c["g"].astype(np.float64) * 2.0 ** -RG.G_SHIFT).astype(np.float32))
    prior = torch.from_numpy(RG.units_to_fp32(c["prior"], shift))

    def out(lo, n):
        return None if not n else (prior[lo:lo + n].clone() if acc else ((n, s["n_cols"]), torch.float32))
    return dict(inputs=dict(planes=planes, grad_a=g[:, :NA].contiguous() if NA else None, grad_b=g[:, NA:].contiguous() if NB else None),
                outputs=dict(gw_a=out(0, NA), gw_b=out(NA, NB)), view=v, want=want, p=NC.abi_params(L.SETS[s["name"]], s["order"]))


def _call_li(s, host, ins, outs):
    from snn_automotive_object_detection_amd import _lib, readout
    v = host["view"]
    view = _lib.snn_planes_view(v["offset"], v["stride"], v["rows"], v["words"], v["layout"], v["steps_formed"], 0)
    readout.li_heads_wgrad(ins["planes"], view, s["n_cols"], s["T"], host["p"], ins["grad_a"], ins["grad_b"], out=(outs["gw_a"], outs["gw_b"]),
                           accumulate=bool(s["acc"]))


def _expect_li(s, host, outs):
    got = torch.cat([t for t in (outs["gw_a"], outs["gw_b"]) if t is not None]).cpu().numpy()
    want = host["want"]
    assert got.shape == want.shape == (s["NA"] + s["NB"], s["n_cols"])
    bad = got.view(np.uint32) != want.view(np.uint32)
    bad &= ~((got == 0) & (want == 0))                                # (a zero is a zero)
    assert not bad.any(), "%s: %d of %d elements differ from the integer expectation, the first at %s: %r against %r" % (
        spec_id(s), bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


# ---- snn_spike_linear_wgrad -------------------------------------------------------------------------------------------------------------------
def _prep_sw(s):
    K, N, rows, Tp, acc = s["K"], s["N"], s["rows"], s["Tp"], s["acc"]
    c = HG.exact_wgrad_case(rows, K, N, Tp, s["density"], acc, [rows, Tp, K, N, acc])
    return dict(inputs=dict(a_rows=c["a_rows"], d_cur=HG.padded(c["d"], N + 5)), outputs=dict(gw=c["prior"] if acc else ((N, K), torch.float32)),
                want32=c["want32"])


def _call_sw(s, host, ins, outs):
    from snn_automotive_object_detection_amd import hidden
    hidden.spike_linear_wgrad(ins["a_rows"], ins["d_cur"], s["K"], s["N"], out=outs["gw"], accumulate=bool(s["acc"]))


def _expect_sw(s, host, outs):
    got, want32 = outs["gw"].cpu().numpy(), host["want32"]
    bad = got != want32
    assert not bad.any(), "%s: %d of %d elements differ from the integer expectation, the first at %s: %r against %r" % (
        spec_id(s), bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want32[bad][0])


# ---- snn_lif_surrogate_bwd -------------------------------------------------------------------------------------------------------------------
def _prep_lif(s):
    R, N, Tc, order, mode = s["R"], s["N"], s["Tc"], s["order"], s["mode"]
    c = HG.REFERENCE if s["cname"] == "reference" else HG.OTHER
    ldc = N + 32 - N % 32 if N % 32 else N + 32                     # ldc > N, padding columns hold NaN
    cur = HG.draw_currents(Tc, R, N, ldc, s["rate"], c, [R, N, Tc, int(s["rate"] * 10)])
    z = HG.lif_forward(cur[:, :, :N].double(), c)                    # the planes come from an fp64 forward of those currents
    g = torch.Generator().manual_seed(R * 1000 + N * 10 + Tc)
    gz = torch.randn((Tc + 1, R, N), generator=g) if mode in ("gz", "both") else None
    gu = torch.randn((R, N), generator=g) if mode in ("gu", "both") else None
    ref = {dt: HG.adjoint(cur[:, :, :N], z, c, s["alpha"], gz=gz, gu=gu, kappa=HG.kappa(c, Tc + 1, order, dt), dtype=dt)
           for dt in (torch.float64, torch.float32)}
    return dict(inputs=dict(cur=cur, z_rows=HG.pack_bits(z, set_padding=True), gz=gz, gu=gu), outputs=dict(d_cur=((Tc, R, N), torch.float32)),
                ref64=ref[torch.float64], ref32=ref[torch.float32], c=c)


def _call_lif(s, host, ins, outs):
    from snn_automotive_object_detection_amd import _lib, hidden
    c = host["c"]
    p = _lib.snn_params(c.a, c.b, c.v_leak, c.v_reset, 0.25, c.th, {"jump_first": 0, "voltage_first": 1}[s["order"]], _lib.PRECISIONS["bf16x3"])
    hidden.lif_surrogate_bwd(ins["cur"], ins["z_rows"], s["N"], p, s["alpha"], gz=ins["gz"], gu=ins["gu"], out=outs["d_cur"])


def _expect_lif(s, host, outs):
    """the rule of tests/test_gpu_hidden_grad.py: the error against fp64 at most 4 x that of the op-for-op fp32 CPU evaluation, largest and rms"""
    got = outs["d_cur"].cpu()
    assert got.shape == host["ref64"].shape and bool(torch.isfinite(got).all())
    (gmax, grms), (cmax, crms) = HG.errors(got, host["ref64"]), HG.errors(host["ref32"], host["ref64"])
    print("%s: |err| max %.3g rms %.3g; fp32 CPU %.3g / %.3g" % (spec_id(s), gmax, grms, cmax, crms))
    assert gmax <= 4 * cmax and grms <= 4 * crms, "%s: |err| max %.3g rms %.3g against 4 x (%.3g, %.3g)" % (spec_id(s), gmax, grms, cmax, crms)


# ---- snn_planes_to_rows ------------------------------------------------------------------------------------------------------------------------
def _prep_p2r(s):
    layout, rows, words, Tp = s["layout"], s["rows"], s["words"], s["Tp"]
    rng = np.random.default_rng([layout, rows, words, Tp])
    offset, stride = 132, rows * words + 7
    want = rng.integers(0, 2 ** 32, size=(Tp, rows, words), dtype=np.uint64).astype(np.uint32)
    flat = np.full(offset // 4 + (Tp - 1) * stride + rows * words, 0xa5a5a5a5, dtype=np.uint32)     # ends on the last word of step T' - 1
    idx = TP.word_index(layout, rows, words)
    for t in range(Tp):
        flat[offset // 4 + t * stride + idx] = want[t]
    assert np.array_equal(TP.rows_from_layout(flat[offset // 4:], Tp, rows, words, layout, stride), want)
    return dict(inputs=dict(ws=torch.from_numpy(flat.view(np.uint8).copy())), outputs=dict(rows=((Tp, rows, words), torch.int32)),
                view=(offset, stride, rows, words, layout, Tp, 0), want=want)


def _call_p2r(s, host, ins, outs):
    from snn_automotive_object_detection_amd import _lib
    view = _lib.snn_planes_view(*host["view"])
    _lib.check(_lib.load().snn_planes_to_rows(C.c_void_p(ins["ws"].data_ptr()), C.byref(view), s["Tp"], C.c_void_p(outs["rows"].data_ptr()),
                                              torch.cuda.current_stream().cuda_stream), "snn_planes_to_rows")


def _expect_p2r(s, host, outs):
    got = outs["rows"].cpu().numpy().view(np.uint32)
    assert np.array_equal(got, host["want"]), "%s: %d words differ from the index arithmetic" % (spec_id(s), int((got != host["want"]).sum()))


# ---- snn_match_targets -------------------------------------------------------------------------------------------------------------------------
def _image(B, G, seed):
    if B == 0:                                                        # (an image without boxes between others: its ground truth is still staged)
        _, gt, labels = HL.random_image(1, G, seed)
        return torch.zeros((0, 4)), gt, labels
    return HL.random_image(B, G, seed)


def _prep_match(s):
    imgs = [_image(B, G, 1000 * n + 100 * B + G) for n, (B, G) in enumerate(s["images"])]
    rpn = s["mode"] == "rpn"
    (high, low), weights = (RPN_T, RPN_W) if rpn else (DET_T, DET_W)
    total = sum(b for b, _ in s["images"])
    want = []
    for b, g, l in imgs:
        if not b.shape[0]:                                            # (no boxes: nothing of this image is written)
            want.append((torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), torch.zeros((0, 4), dtype=torch.float64), 0.0))
            continue
        idx, lab = HL.match(b, g, None if rpn else l, high, low, bool(s["lq"]))
        ref = HL.matched_gt(g, idx)
        t32, t64 = HL.encode(ref, b, weights), HL.encode(ref.double(), b.double(), weights)
        want.append((idx, lab, t64, HL.tolerance(HL.target_bound(ref, b, weights), t32, t64)))
    return dict(inputs=dict(boxes=torch.cat([i[0] for i in imgs]), gt_boxes=torch.cat([i[1] for i in imgs]),
                            gt_labels=None if rpn else torch.cat([i[2] for i in imgs])),
                outputs=dict(idx=((total,), torch.int32), label=((total,), torch.int32), tgt=((total, 4), torch.float32)),
                want=want, thresholds=(high, low), weights=weights)


def _call_match(s, host, ins, outs):
    from snn_automotive_object_detection_amd import losses
    high, low = host["thresholds"]
    losses.match_targets_raw(ins["boxes"], [b for b, _ in s["images"]], ins["gt_boxes"], ins["gt_labels"], [g for _, g in s["images"]], high, low,
                             bool(s["lq"]), host["weights"], out=(outs["idx"], outs["label"], outs["tgt"]))


def _expect_match(s, host, outs):
    bc = [b for b, _ in s["images"]]
    idx, lab, tgt = (outs[k].cpu().split(bc) for k in ("idx", "label", "tgt"))
    for n, (want_idx, want_lab, t64, tol) in enumerate(host["want"]):
        assert torch.equal(idx[n].to(torch.int64), want_idx), "%s image %d: matched_idx differs at %s" % (
            spec_id(s), n, torch.where(idx[n].to(torch.int64) != want_idx)[0][:8].tolist())
        assert torch.equal(lab[n].to(torch.int64), want_lab), "%s image %d: labels differ" % (spec_id(s), n)
        HL.assert_close(tgt[n], t64, tol, "%s image %d targets" % (spec_id(s), n))


# ---- snn_rpn_loss_grad / snn_det_loss_grad -----------------------------------------------------------------------------------------------------
def _rpn_ref(shapes, N, A, case, dt):
    logits, deltas, label, sampled, targets = case
    o = HL.head_rows_to_ref(logits.to(dt), shapes, N, 1).reshape(-1)
    d = HL.head_rows_to_ref(deltas.to(dt), shapes, N, 4)
    (l0, l1), (g_o, g_d), _ = HL.with_grads(HL.rpn_loss, o, d, label.to(dt), targets.to(dt), sampled.bool())
    return torch.stack((l0, l1)), HL.ref_to_head_rows(g_o.reshape(-1, 1), shapes, N, A, 1), HL.ref_to_head_rows(g_d, shapes, N, A, 4)


def _prep_rpnl(s):
    shapes, N, A = s["shapes"], s["N"], s["A"]
    case = list(HL.rpn_loss_case(shapes, N, A, 7 + A))
    if case[0].numel() < 8:                                           # (a handful of anchors: all of them sampled positives, so that n > 0)
        case[3][:] = 1
        case[2][:] = 1
    assert int(case[3].sum()) > 0                                     # (n = 0 is the NaN loss: not a case here)
    names = ("logits", "deltas", "label", "sampled", "reg_target")
    return dict(inputs=dict(zip(names, case)),
                outputs=dict(loss=((2,), torch.float32), g_logits=(tuple(case[0].shape), torch.float32), g_deltas=(tuple(case[1].shape), torch.float32)),
                ref32=_rpn_ref(shapes, N, A, case, torch.float32), ref64=_rpn_ref(shapes, N, A, case, torch.float64), n=int(case[3].sum()))


def _call_rpnl(s, host, ins, outs):
    from snn_automotive_object_detection_amd import losses
    losses.rpn_loss_grad(_shapes_of(s), s["A"], ins["logits"], ins["deltas"], ins["label"], ins["sampled"], ins["reg_target"],
                         out=(outs["loss"], outs["g_logits"], outs["g_deltas"]))


def _expect_losses(s, host, outs, names):
    (l32, a32, b32), (l64, a64, b64), n = host["ref32"], host["ref64"], host["n"]
    HL.assert_close(outs["loss"], l64, HL.tolerance(HL.LOSS_UNITS * HL.U * l64.abs(), l32, l64), spec_id(s) + " losses")
    HL.assert_close(outs[names[0]], a64, HL.tolerance(HL.GRAD_UNITS * HL.U / n, a32, a64), spec_id(s) + " " + names[0])
    HL.assert_close(outs[names[1]], b64, HL.tolerance(HL.GRAD_UNITS * HL.U / n, b32, b64), spec_id(s) + " " + names[1])
    assert not bool(outs[names[1]].cpu()[b64 == 0].any()), "an element the loss does not read is not an exact zero"


def _det_ref(case, dt):
    logits, box, label, targets = case
    (l0, l1), (g_l, g_b), _ = HL.with_grads(HL.det_loss, logits.to(dt), box.to(dt), label.to(torch.int64), targets.to(dt))
    return torch.stack((l0, l1)), g_l, g_b


def _prep_detl(s):
    R, K = s["R"], s["K"]
    case = list(HL.det_loss_case(R, K, R + K, ignore=bool(s["ignore"]) and R > 1))
    if R == 1:
        case[2][:] = 1
    names = ("logits", "box", "label", "reg_target")
    return dict(inputs=dict(zip(names, case)), outputs=dict(loss=((2,), torch.float32), g_logits=((R, K), torch.float32), g_box=((R, 4 * K), torch.float32)),
                ref32=_det_ref(case, torch.float32), ref64=_det_ref(case, torch.float64), n=int((case[2] >= 0).sum()))


def _call_detl(s, host, ins, outs):
    from snn_automotive_object_detection_amd import losses
    losses.det_loss_grad(ins["logits"], ins["box"], ins["label"], ins["reg_target"], out=(outs["loss"], outs["g_logits"], outs["g_box"]))


PREPARE = {"snn_li_heads_wgrad": _prep_li, "snn_spike_linear_wgrad": _prep_sw, "snn_lif_surrogate_bwd": _prep_lif, "snn_planes_to_rows": _prep_p2r,
           "snn_match_targets": _prep_match, "snn_rpn_loss_grad": _prep_rpnl, "snn_det_loss_grad": _prep_detl}
CALLS = {"snn_li_heads_wgrad": _call_li, "snn_spike_linear_wgrad": _call_sw, "snn_lif_surrogate_bwd": _call_lif, "snn_planes_to_rows": _call_p2r,
         "snn_match_targets": _call_match, "snn_rpn_loss_grad": _call_rpnl, "snn_det_loss_grad": _call_detl}
EXPECT = {"snn_li_heads_wgrad": _expect_li, "snn_spike_linear_wgrad": _expect_sw, "snn_lif_surrogate_bwd": _expect_lif, "snn_planes_to_rows": _expect_p2r,
          "snn_match_targets": _expect_match,
          "snn_rpn_loss_grad": lambda s, h, o: _expect_losses(s, h, o, ("g_logits", "g_deltas")),
          "snn_det_loss_grad": lambda s, h, o: _expect_losses(s, h, o, ("g_logits", "g_box"))}


@functools.lru_cache(maxsize=8)
def _prepared(k):
    s = dict(k)
    return PREPARE[s["entry"]](s)


def prepare(s) -> dict:
    """the host case of a spec (built once for the runs that follow each other: the two input guards, the three fills)"""
    return _prepared(key(s))


def stage(s, dev, in_guard: int = 0x00) -> W.GuardedCall:
    host = prepare(s)
    return W.GuardedCall(dev, host["inputs"], host["outputs"], in_guard)


def run(s, dev, in_guard: int = 0x00):
    """stage, call, verify (guards, inputs, unwritten elements), expectation -> the snapshot of the outputs"""
    host = prepare(s)
    gc = stage(s, dev, in_guard)
    CALLS[s["entry"]](s, host, gc.ins, gc.outs)
    snap = gc.verify()
    EXPECT[s["entry"]](s, host, gc.outs)
    return snap


def call(s, dev, in_guard: int = 0x00):
    return lambda: run(s, dev, in_guard)


# ---- the shapes tests/test_gpu_train_entries.py runs -------------------------------------------------------------------------------------------
SW_DIMS = (1, 31, 33, 63, 65, 127, 129, 255, 257, 288)          # 288 = 9 x 32 is the whole-block value; the others leave a partial block


def sw_pairs():
    """(K, N): every value but 288 meets a partial-block partner (the anti-diagonal) and the whole-block one, as K and as N; 288 meets all"""
    part = SW_DIMS[:-1]
    return ([(part[i], part[len(part) - 1 - i]) for i in range(len(part))] + [(k, 288) for k in SW_DIMS] + [(288, n) for n in part])


#        (rows, T'): M = 1, 5, 7 (tail only), 8 = 4 x 2 (one batch, over a step boundary), 9, 16, 17, 15 = 3 x 5, 512, 513, 600 = 100 x 6 (two slabs of 304)
SW_M = ((1, 1), (5, 1), (7, 1), (4, 2), (9, 1), (16, 1), (17, 1), (3, 5), (512, 1), (513, 1), (100, 6))
SW_CAP = (1025, 8)                                                # M = 8200 > 16 x 512: 16 slabs of 520 rows (the last of 400)
SW_DENSITIES = (0.02, 0.3, 1.0)


def _sw_edges():
    out = [sw(K, N, *SW_M[i % len(SW_M)], acc=i % 2, density=SW_DENSITIES[i % 3]) for i, (K, N) in enumerate(sw_pairs())]
    return out + [sw(33, 65, *SW_CAP, acc=0), sw(65, 33, *SW_CAP, acc=1)]


LI_NCOLS, LI_OUTS, LI_ROWS = (1, 33, 127, 129, 130), ((1, 0), (15, 2), (16, 16), (17, 0)), (63, 64, 65)
LI_SETS = (("a2_b2", 8), ("a2_b1", 12))


def _li_edges():
    """every n_cols on every layout; the outputs, the rows, the set, the order, accumulate and the view's slack dealt round-robin (15 cases: every
    (NA, NB) meets every rows)"""
    out, i = [], 0
    for n_cols in LI_NCOLS:
        for layout in TP.LAYOUTS:
            (NA, NB), (name, T) = LI_OUTS[i % 4], LI_SETS[(i // 4) % 2]
            out.append(li(LI_ROWS[i % 3], n_cols, layout, NA, NB, acc=(i // 2) % 2, slack=i % 8, name=name, T=T, order=L.ORDERS[(i // 3) % 2]))
            i += 1
    return out


def _lif_edges():
    out, i = [], 0
    for N in (1, 31, 33):
        for R in (1, 9):
            for Tc in (1, 31):
                out.append(lif(R, N, Tc, L.ORDERS[i % 2], ("gz", "gu", "both")[(i // 2) % 3], (100.0, 1.0, 0.0)[i % 3], ("reference", "other")[(i // 3) % 2],
                               (0.1, 0.5)[(i // 5) % 2]))
                i += 1
    return out


def _p2r_cases():
    return [p2r(layout, rows, words) for layout in TP.LAYOUTS for rows in (1, 65) for words in (1, 4, 8) if layout != TP.SPLIT4 or words % 4 == 0]


SW_EDGES, LI_EDGES, LIF_EDGES, P2R_CASES = _sw_edges(), _li_edges(), _lif_edges(), _p2r_cases()

M_SMALL, M_RAGGED = match(((63, 2),), "rpn"), match(((257, 2), (63, 0), (300, 65)), "det")
M_64 = match(tuple((1, n % 3) for n in range(64)), "rpn")        # LS_MAX_IMAGES images of one box each: 64 work-groups, 0 .. 2 ground-truth boxes
M_GROUPS = match(((257, 256), (0, 3), (256, 1)), "det")           # 2 + 0 + 1 work-groups; LS_MAX_GT ground-truth boxes in the first image
M_STRICT = match(((65, 64), (1, 1)), "det", lq=0)                 # one launch, no scratch read or written
MATCH_CASES = (M_SMALL, M_RAGGED, M_64, M_GROUPS, M_STRICT)
R_LARGE, R_SMALL, R_ONE = rpnl(HL.PYRAMID, 2, 3), rpnl(((3, 4), (1, 2)), 3, 5), rpnl(((1, 1),), 1, 1)      # 294 anchors (two work-groups), 210, 1
RPNL_CASES = (R_LARGE, R_SMALL, R_ONE)
D_LARGE, D_SMALL = detl(65, 11, 1), detl(1, 2)
DETL_CASES = (D_LARGE, D_SMALL, detl(63, 9), detl(17, 256, 1))    # 16-row work-groups: 4 + 1 rows, 1, 3 x 16 + 15, 16 + 1 at LS_MAX_K

# guarded operands (tests 1 and 2 of the GPU file): the edge shapes and every loss case
OPERAND_SPECS = SW_EDGES + LI_EDGES + LIF_EDGES + P2R_CASES + list(MATCH_CASES) + list(RPNL_CASES) + list(DETL_CASES)

# the scratch seam: fills, one byte short, sequences
LI_LARGE, LI_SMALL = li(65, 130, TP.SPLIT4, 16, 16, slack=6), li(63, 1, TP.ROWS, 1, 0)            # 2 slabs x 32 x 130 floats; 4 bytes (max(16, need) applies)
SW_LARGE, SW_SMALL = sw(288, 257, 100, 6), sw(1, 1, 1, 1)                                       # 2 slabs x 257 x 288 floats; 4 bytes
FILL_SPECS = [LI_LARGE, LI_SMALL, li(64, 33, TP.WORD_MAJOR, 15, 2, acc=1, slack=3), SW_LARGE, SW_SMALL, sw(129, 65, 513, 1, acc=1),
              M_SMALL, M_RAGGED, M_64, M_GROUPS, R_LARGE, R_SMALL, D_LARGE, D_SMALL]
SHORT_SPECS = [LI_LARGE, SW_LARGE, M_RAGGED, M_64, M_GROUPS, R_LARGE, D_LARGE]
SEQUENCES = {
    ("readout", "_WS_WGRAD"): [LI_LARGE, LI_SMALL, LI_LARGE],
    ("hidden", "_WS_WGRAD"): [SW_LARGE, SW_SMALL, SW_LARGE],
    ("losses", "_WS_LOSS"): [M_RAGGED, R_LARGE, D_LARGE, M_RAGGED],
}


def all_specs():
    """every spec the GPU file runs (tests/test_train_entries_cpu.py asks the size queries about each)"""
    return OPERAND_SPECS + FILL_SPECS + SHORT_SPECS + [s for seq in SEQUENCES.values() for s in seq]


def seam_of(s):
    module, attr, _ = TRAIN_ENTRIES[s["entry"]]
    return (module, attr) if attr else None
