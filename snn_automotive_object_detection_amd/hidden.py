"""Detector fine-tuning below the readout: SuperSpike gradients through lif7 into ``fc7.weight``, computed on the GPU from the spike planes
a head pass left in its workspace (include/snn_hip.h: snn_planes_to_rows, snn_lif_surrogate_bwd, snn_spike_linear_wgrad).

The reference's hidden cells are Norse LIFCells with the default ``method="super"``: Heaviside forward, ``grad / (alpha |x| + 1)^2`` backward
(``p_lif.alpha`` = 100).  ``Fc7Grad`` is ``readout.ReadoutGrad``'s twin one layer further down: its forward returns the pass's own outputs, its
backward hands gradients to ``cls_score.weight``, ``bbox_pred.weight`` (the exact ones of readout.py, bit for bit) and ``fc7.weight``.  The
backward is teacher-forced: currents are recomputed from the saved lif6 rows with the un-fused GEMM of the pass's precision, membranes by
re-running the recurrence on them, and every reset decision is the bit the pass itself stored.  fc6, the RPN's conv and the features get no
gradient.  Everything is enqueued on the current stream without a host synchronisation."""
import ctypes as C
from typing import Optional

import torch

from . import _lib, ops, readout
from ._lib import snn_planes_view, snn_params

_WS_WGRAD = ops._Workspace()                  # slab partial tiles of snn_spike_linear_wgrad


def rows_view(rows: int, words: int, steps: int) -> snn_planes_view:
    """the view of a [steps, rows, words] tensor in rows layout, as its own workspace"""
    return snn_planes_view(0, rows * words, rows, words, _lib.PLANE_LAYOUTS["rows"], steps, 0)


@ops._on_tensor_device
def planes_to_rows(ws: torch.Tensor, view: snn_planes_view, T_prime: int) -> torch.Tensor:
    """the first ``T_prime`` steps of the planes ``view`` names inside ``ws``, in any layout -> int32 [T_prime, rows, words] in rows layout, bit
    for bit: what stays valid when the next pass overwrites the workspace, and the operand of the un-fused spike GEMMs"""
    ops._need_gpu(ws, "workspace")
    out = torch.empty((int(T_prime), int(view.rows), int(view.words)), dtype=torch.int32, device=ws.device)
    _lib.check(_lib.load().snn_planes_to_rows(ops._ptr(ws), C.byref(view), int(T_prime), ops._ptr(out), ops._stream()), "snn_planes_to_rows")
    return out


@ops._on_tensor_device
def lif_surrogate_bwd(cur: torch.Tensor, z_rows: torch.Tensor, N: int, p: snn_params, alpha: float, gz: Optional[torch.Tensor] = None,
                      gu: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """d_cur fp32 [Tc, R, N] = dL/dcur of one LIF layer with a SuperSpike threshold.  cur fp32 [Tc, R, ldc] (ldc >= N), z_rows int32
    [Tc + 1, R, ceil(N / 32)]: the layer's own spikes; the upstream gradient is gz [Tc + 1, R, N] + kappa_t gu [R, N] (either may be None)."""
    ops._need_gpu(cur, "currents")
    ops._need_gpu(z_rows, "spike rows")
    if cur.dtype != torch.float32 or not cur.is_contiguous() or cur.dim() != 3:
        raise _lib.SnnHipError("cur must be a contiguous fp32 [Tc, R, ldc] tensor")
    Tc, R, ldc = (int(x) for x in cur.shape)
    Nw = ops.cdiv(N, 32)
    if z_rows.dtype != torch.int32 or not z_rows.is_contiguous() or tuple(z_rows.shape) != (Tc + 1, R, Nw):
        raise _lib.SnnHipError("z_rows must be a contiguous int32 [%d, %d, %d] tensor, got %s" % (Tc + 1, R, Nw, tuple(z_rows.shape)))
    if gz is not None:
        gz = ops._f32c(gz)
        if tuple(gz.shape) != (Tc + 1, R, N):
            raise _lib.SnnHipError("gz must be [%d, %d, %d], got %s" % (Tc + 1, R, N, tuple(gz.shape)))
    if gu is not None:
        gu = ops._f32c(gu)
        if tuple(gu.shape) != (R, N):
            raise _lib.SnnHipError("gu must be [%d, %d], got %s" % (R, N, tuple(gu.shape)))
    if out is None:
        out = torch.empty((Tc, R, N), dtype=torch.float32, device=cur.device)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or tuple(out.shape) != (Tc, R, N):
        raise _lib.SnnHipError("out must be a contiguous fp32 GPU tensor [%d, %d, %d]" % (Tc, R, N))
    _lib.check(_lib.load().snn_lif_surrogate_bwd(ops._ptr(cur), ldc, ops._ptr(z_rows), Tc, R, int(N), C.byref(p), float(alpha), ops._ptr(gz),
                                                 ops._ptr(gu), ops._ptr(out), ops._stream()), "snn_lif_surrogate_bwd")
    return out


@ops._on_tensor_device
def spike_linear_wgrad(a_rows: torch.Tensor, d_cur: torch.Tensor, K: int, N: int, out: Optional[torch.Tensor] = None,
                       accumulate: bool = False) -> torch.Tensor:
    """gw fp32 [N, K] with gw[n][k] = sum_t sum_r d_cur[t][r][n] * bit_t(r, k): the weight gradient of a bias-free linear layer fed by the
    spikes a_rows int32 [T', rows, ceil(K / 32)]; d_cur fp32 [T', rows, ldd], ldd >= N.  ``out``: write into this tensor - or, with
    ``accumulate``, add to it.  Deterministic: two calls on the same data are bit-equal."""
    ops._need_gpu(a_rows, "spike rows")
    ops._need_gpu(d_cur, "d_cur")
    lib = _lib.load()
    if d_cur.dtype != torch.float32 or not d_cur.is_contiguous() or d_cur.dim() != 3:
        raise _lib.SnnHipError("d_cur must be a contiguous fp32 [T', rows, ldd] tensor")
    Tp, rows, ldd = (int(x) for x in d_cur.shape)
    if a_rows.dtype != torch.int32 or not a_rows.is_contiguous() or tuple(a_rows.shape) != (Tp, rows, ops.cdiv(K, 32)):
        raise _lib.SnnHipError("a_rows must be a contiguous int32 [%d, %d, %d] tensor, got %s" % (Tp, rows, ops.cdiv(K, 32), tuple(a_rows.shape)))
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs `out`: the tensor to add to")
        out = torch.empty((N, K), dtype=torch.float32, device=d_cur.device)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != N * K:
        raise _lib.SnnHipError("out must be a contiguous fp32 GPU tensor of %d x %d elements" % (N, K))
    scratch = _WS_WGRAD.get(d_cur.device, max(16, lib.snn_spike_linear_wgrad_workspace_bytes(rows, int(K), int(N), Tp)))
    _lib.check(lib.snn_spike_linear_wgrad(ops._ptr(a_rows), ops._ptr(d_cur), ldd, Tp, rows, int(K), int(N), ops._ptr(out), int(bool(accumulate)),
                                          ops._ptr(scratch), scratch.numel(), ops._stream()), "snn_spike_linear_wgrad")
    return out


class _Saved:
    """what backward needs of one detector-head pass (held by the graph, not by the module): lif6's first T - 1 steps and lif7's T steps as
    rows, the parameters, the surrogate's alpha, and fc7 as the pass multiplied it (packed, with the un-fused GEMM that takes it)"""
    def __init__(self, outs, z6, z7, Hd, T, p, alpha, w7_packed, gemm):
        self.outs, self.z6, self.z7, self.Hd, self.T, self.p, self.alpha, self.w7_packed, self.gemm = tuple(outs), z6, z7, Hd, T, p, alpha, w7_packed, gemm


class Fc7Grad(torch.autograd.Function):
    """outputs of a finished detector-head pass as a function of cls_score.weight, bbox_pred.weight and fc7.weight: forward returns the pass's
    own tensors; backward is (i) snn_li_heads_wgrad on the saved lif7 rows, (ii) gu = g_cls W_cls + g_box W_box, (iii) fc7's currents by the
    un-fused GEMM on the saved lif6 rows, (iv) snn_lif_surrogate_bwd, (v) snn_spike_linear_wgrad."""

    @staticmethod
    def forward(ctx, w_cls, w_box, w7, saved: _Saved):
        outs, saved.outs = saved.outs, None                            # (the outputs hold the graph: it must not hold them)
        ctx.saved = saved
        ctx.save_for_backward(w_cls, w_box)
        ctx.shapes = (w_cls.shape, w_box.shape, w7.shape)
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        s = ctx.saved
        need_c, need_b, need_7 = ctx.needs_input_grad[:3]
        if all(g is None for g in grads):
            return None, None, None, None
        dev = next(g.device for g in grads if g is not None)

        def zeros(k, need):
            return torch.zeros(ctx.shapes[k], dtype=torch.float32, device=dev) if need else None
        if s.z7 is None:                                              # (a pass over no rows: nothing ran, nothing arrives)
            return zeros(0, need_c), zeros(1, need_b), zeros(2, need_7), None
        g_cls, g_box = (None if g is None else ops._f32c(g) for g in grads)
        T, R, Hd = s.T, int(s.z7.shape[1]), s.Hd
        gw_c = gw_b = gw_7 = None
        if need_c or need_b:
            gw_c, gw_b = readout.li_heads_wgrad(s.z7, rows_view(R, int(s.z7.shape[2]), T), Hd, T, s.p, g_cls if need_c else None,
                                                g_box if need_b else None)
        if need_7:
            w_cls, w_box = ctx.saved_tensors
            with torch.no_grad():
                gu = None
                for g, w in ((g_cls, w_cls), (g_box, w_box)):
                    if g is not None:
                        part = torch.matmul(g, w.detach().to(torch.float32))
                        gu = part if gu is None else gu + part
                cur = s.gemm(s.z6.view((T - 1) * R, -1), Hd, Hd, s.w7_packed)
                d_cur = lif_surrogate_bwd(cur.view(T - 1, R, -1), s.z7, Hd, s.p, s.alpha, gu=gu)
                gw_7 = spike_linear_wgrad(s.z6, d_cur, Hd, Hd)

        def shaped(gw, k, need):
            if not need:
                return None
            return zeros(k, True) if gw is None else gw.view(ctx.shapes[k])
        return shaped(gw_c, 0, need_c), shaped(gw_b, 1, need_b), shaped(gw_7, 2, need_7), None


def wanted(module) -> bool:
    """does this forward of the detector head build the fc7 graph: ``train_fc7`` set, grad mode on, ``fc7.weight`` requiring grad"""
    if not getattr(module, "train_fc7", False):
        return False
    if getattr(module, "spike_rates", False):
        raise NotImplementedError("train_fc7 with spike_rates: spike-rate mode returns rates, not outputs to put a loss on")
    if module.precision in ("bf16", "mxfp6"):
        raise NotImplementedError("train_fc7 under precision %r: the weight that pass multiplies is not the fp32 parameter, and a hidden layer's "
                                  "straight-through rule is not decided here (use \"bf16x3\" or \"f32\")" % module.precision)
    return torch.is_grad_enabled() and module.fc7.weight.requires_grad


def attach(module, outs, ws: Optional[torch.Tensor], view6: Optional[snn_planes_view], view7: Optional[snn_planes_view], T: int, p: snn_params,
           prec: str):
    """the tensors ``outs`` of a detector-head pass that just ran in ``ws`` -> the same tensors with a grad_fn to the readout weights and
    fc7.weight (ws None: the pass ran nothing).  lif6's first T - 1 steps and lif7's T steps leave the workspace as rows here."""
    if T < 3:
        raise ValueError("train_fc7 needs num_steps >= 3 (lif6's plane of step 0 first moves an output at step 2), got %d" % T)
    z6 = z7 = w7 = gemm = None
    if ws is not None:
        if int(view6.steps_formed) < T - 1:
            raise _lib.SnnHipError("train_fc7: the pass formed %d lif6 planes, the gradient needs %d" % (int(view6.steps_formed), T - 1))
        z6, z7 = planes_to_rows(ws, view6, T - 1), planes_to_rows(ws, view7, T)
        w7 = module._packed(prec)[1]
        gemm = ops.spike_gemm_bf16x3 if prec == "bf16x3" else ops.spike_gemm
    outs = [o.detach() for o in outs]
    saved = _Saved(outs, z6, z7, int(module.representation_size), T, p, float(module.p_lif.alpha), w7, gemm)
    return Fc7Grad.apply(module.cls_score.weight, module.bbox_pred.weight, module.fc7.weight, saved)


FC7_WEIGHTS = ("fc7", "cls_score", "bbox_pred")


def freeze_below_fc7(module_or_model) -> list:
    """``readout.freeze_hidden``'s twin one layer further down: ``requires_grad = False`` on every parameter under ``module_or_model`` but the
    readout weights of the spiking heads in it and the detector head's ``fc7.weight``; returns those parameters - what an optimiser is given.
    The detector head's fc7 comes first, then the readout weights in ``freeze_hidden``'s order."""
    keep = [m.fc7.weight for m in module_or_model.modules() if type(m).__name__ == "FastRCNNPredictorSNNFull"]
    for m in module_or_model.modules():
        for name in readout.READOUT_WEIGHTS.get(type(m).__name__, ()):
            keep.append(getattr(m, name).weight)
    ids = {id(w) for w in keep}
    for q in module_or_model.parameters():
        q.requires_grad_(id(q) in ids and q.requires_grad)
    return keep
