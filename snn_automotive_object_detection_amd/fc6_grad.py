"""Detector fine-tuning one layer below hidden.py: SuperSpike gradients through lif7 AND lif6 into ``fc6.weight``, with fc6's weight gradient
on the bf16 matrix cores (include/snn_hip.h: snn_spike_wgrad_bf16x3).

``Fc6Grad`` is ``hidden.Fc7Grad``'s twin one layer further down: its forward returns the pass's own outputs, its backward hands gradients to
``cls_score.weight``, ``bbox_pred.weight``, ``fc7.weight`` (the calls of Fc7Grad, bit for bit) and ``fc6.weight``:
    gz6_t = d_cur7_t W7 (t <= T - 2; one fp32 matmul)     d_cur6 = snn_lif_surrogate_bwd(cur6, z6, gz = gz6)  (Tc = T - 2)
    dL/dW6[n][k] = sum_{t <= T - 3} sum_r d_cur6_t[r][n] enc_t(r, k)          (k = channel * 49 + bin: fc6.weight's own layout)
The backward is teacher-forced as hidden.py's: fc6's currents are recomputed with the un-fused GEMM of the pass's precision from the encoder's
spikes, membranes by re-running the recurrence, every reset decision is the saved lif6 bit.  The encoder's spikes are NOT read from the pass's
workspace (the product path keeps them permuted and compressed): at attach time the features are still alive, and the stand-alone encoder
- pinned bit-identical to the fused ones - is re-run for T - 2 steps into natural-order rows.  The RPN's conv, the encoders and the features get
no gradient.  Everything is enqueued on the current stream without a host synchronisation."""
from typing import Callable, Optional

import torch

from . import _lib, hidden, ops, readout
from ._lib import snn_planes_view, snn_params

_WS_WGRAD3 = ops._Workspace()                 # slab partial tiles of snn_spike_wgrad_bf16x3


@ops._on_tensor_device
def spike_wgrad_bf16x3(a_rows: torch.Tensor, d_cur: torch.Tensor, K: int, N: int, out: Optional[torch.Tensor] = None,
                       accumulate: bool = False) -> torch.Tensor:
    """``hidden.spike_linear_wgrad`` on the bf16 matrix cores: gw fp32 [N, K] with gw[n][k] = sum_t sum_r d_cur[t][r][n] * bit_t(r, k), every
    d_cur element split on the fly into three bf16 values (exact for values below 2^128 - 2^119 in magnitude with no bit below 2^-133).
    a_rows int32 [T', rows, ceil(K / 32)]; d_cur fp32 [T', rows, ldd], ldd >= N, finite and below bf16's largest value; K <= 16384,
    N <= 8192.  ``out``: write into this tensor - or, with ``accumulate``, add to it.  Deterministic: two calls on the same data are bit-equal.
    The scratch is sized by the monotone size query and kept: with one slab (fc6's shape: 85 MB) the call never touches it."""
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
    scratch = _WS_WGRAD3.get(d_cur.device, max(16, lib.snn_spike_wgrad_bf16x3_workspace_bytes(rows, int(K), int(N), Tp)))
    _lib.check(lib.snn_spike_wgrad_bf16x3(ops._ptr(a_rows), ops._ptr(d_cur), ldd, Tp, rows, int(K), int(N), ops._ptr(out), int(bool(accumulate)),
                                          ops._ptr(scratch), scratch.numel(), ops._stream()), "snn_spike_wgrad_bf16x3")
    return out


class _Saved:
    """what backward needs of one detector-head pass (held by the graph, not by the module): the encoder's first T - 2 steps, lif6's first
    T - 1 steps and lif7's T steps as rows, the parameters, the surrogate's alpha, fc6 (natural order) and fc7 as the pass multiplied them
    (packed, with the un-fused GEMM that takes them)"""
    def __init__(self, outs, enc, z6, z7, D, Hd, T, p, alpha, w6_packed, w7_packed, gemm):
        self.outs, self.enc, self.z6, self.z7, self.D, self.Hd, self.T, self.p, self.alpha = tuple(outs), enc, z6, z7, D, Hd, T, p, alpha
        self.w6_packed, self.w7_packed, self.gemm = w6_packed, w7_packed, gemm


class Fc6Grad(torch.autograd.Function):
    """outputs of a finished detector-head pass as a function of cls_score.weight, bbox_pred.weight, fc7.weight and fc6.weight: forward returns
    the pass's own tensors; backward is Fc7Grad's five calls, then (vi) gz6 = d_cur7 W7, (vii) fc6's currents by the un-fused GEMM on the
    re-encoded rows, (viii) snn_lif_surrogate_bwd with gz, (ix) snn_spike_wgrad_bf16x3."""

    @staticmethod
    def forward(ctx, w_cls, w_box, w7, w6, saved: _Saved):
        outs, saved.outs = saved.outs, None                            # (the outputs hold the graph: it must not hold them)
        ctx.saved = saved
        ctx.save_for_backward(w_cls, w_box, w7)
        ctx.shapes = (w_cls.shape, w_box.shape, w7.shape, w6.shape)
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        s = ctx.saved
        need_c, need_b, need_7, need_6 = ctx.needs_input_grad[:4]
        if all(g is None for g in grads):
            return None, None, None, None, None
        dev = next(g.device for g in grads if g is not None)

        def zeros(k, need):
            return torch.zeros(ctx.shapes[k], dtype=torch.float32, device=dev) if need else None
        if s.z7 is None:                                              # (a pass over no rows: nothing ran, nothing arrives)
            return zeros(0, need_c), zeros(1, need_b), zeros(2, need_7), zeros(3, need_6), None
        g_cls, g_box = (None if g is None else ops._f32c(g) for g in grads)
        T, R, Hd, D = s.T, int(s.z7.shape[1]), s.Hd, s.D
        gw_c = gw_b = gw_7 = gw_6 = None
        if need_c or need_b:
            gw_c, gw_b = readout.li_heads_wgrad(s.z7, hidden.rows_view(R, int(s.z7.shape[2]), T), Hd, T, s.p, g_cls if need_c else None,
                                                g_box if need_b else None)
        if need_7 or need_6:
            w_cls, w_box, w7 = ctx.saved_tensors
            with torch.no_grad():
                gu = None
                for g, w in ((g_cls, w_cls), (g_box, w_box)):
                    if g is not None:
                        part = torch.matmul(g, w.detach().to(torch.float32))
                        gu = part if gu is None else gu + part
                cur7 = s.gemm(s.z6.view((T - 1) * R, -1), Hd, Hd, s.w7_packed)
                d_cur7 = hidden.lif_surrogate_bwd(cur7.view(T - 1, R, -1), s.z7, Hd, s.p, s.alpha, gu=gu)
                if need_7:
                    gw_7 = hidden.spike_linear_wgrad(s.z6, d_cur7, Hd, Hd)
                if need_6:
                    gz6 = torch.matmul(d_cur7.view((T - 1) * R, Hd), w7.detach().to(torch.float32)).view(T - 1, R, Hd)
                    cur6 = s.gemm(s.enc.view((T - 2) * R, -1), D, Hd, s.w6_packed)
                    d_cur6 = hidden.lif_surrogate_bwd(cur6.view(T - 2, R, -1), s.z6, Hd, s.p, s.alpha, gz=gz6)
                    gw_6 = spike_wgrad_bf16x3(s.enc, d_cur6, D, Hd)

        def shaped(gw, k, need):
            if not need:
                return None
            return zeros(k, True) if gw is None else gw.view(ctx.shapes[k])
        return shaped(gw_c, 0, need_c), shaped(gw_b, 1, need_b), shaped(gw_7, 2, need_7), shaped(gw_6, 3, need_6), None


def wanted(module) -> bool:
    """does this forward of the detector head build the fc6 graph: ``train_fc6`` set, grad mode on, ``fc6.weight`` requiring grad"""
    if not getattr(module, "train_fc6", False):
        return False
    if getattr(module, "spike_rates", False):
        raise NotImplementedError("train_fc6 with spike_rates: spike-rate mode returns rates, not outputs to put a loss on")
    if module.precision in ("bf16", "mxfp6"):
        raise NotImplementedError("train_fc6 under precision %r: the weight that pass multiplies is not the fp32 parameter, and a hidden layer's "
                                  "straight-through rule is not decided here (use \"bf16x3\" or \"f32\")" % module.precision)
    return torch.is_grad_enabled() and module.fc6.weight.requires_grad


def attach(module, outs, ws: Optional[torch.Tensor], view6: Optional[snn_planes_view], view7: Optional[snn_planes_view], T: int, p: snn_params,
           prec: str, encode: Optional[Callable[[int], torch.Tensor]] = None):
    """the tensors ``outs`` of a detector-head pass that just ran in ``ws`` -> the same tensors with a grad_fn to the readout weights,
    fc7.weight and fc6.weight (ws None: the pass ran nothing).  lif6's first T - 1 steps and lif7's T steps leave the workspace as rows here;
    ``encode(T - 2)`` re-runs the stand-alone encoder on the pass's own feed: int32 [T - 2, R, ceil(D / 32)] in the reference's order."""
    if T < 3:
        raise ValueError("train_fc6 needs num_steps >= 3 (the encoder's plane of step 0 first moves an output at step 2), got %d" % T)
    enc = z6 = z7 = w6 = w7 = gemm = None
    D, Hd = int(module.in_channels), int(module.representation_size)
    if ws is not None:
        if int(view6.steps_formed) < T - 1:
            raise _lib.SnnHipError("train_fc6: the pass formed %d lif6 planes, the gradient needs %d" % (int(view6.steps_formed), T - 1))
        z6, z7 = hidden.planes_to_rows(ws, view6, T - 1), hidden.planes_to_rows(ws, view7, T)
        enc = encode(T - 2)
        if tuple(enc.shape) != (T - 2, int(z7.shape[1]), ops.cdiv(D, 32)):
            raise _lib.SnnHipError("train_fc6: the re-encoded rows are %s, expected %s" % (tuple(enc.shape), (T - 2, int(z7.shape[1]), ops.cdiv(D, 32))))
        w6, w7 = module._packed(prec, inner=0)[:2]                     # fc6 in the NATURAL order: a second packed copy beside the pass's permuted one
        gemm = ops.spike_gemm_bf16x3 if prec == "bf16x3" else ops.spike_gemm
    outs = [o.detach() for o in outs]
    saved = _Saved(outs, enc, z6, z7, D, Hd, T, p, float(module.p_lif.alpha), w6, w7, gemm)
    return Fc6Grad.apply(module.cls_score.weight, module.bbox_pred.weight, module.fc7.weight, module.fc6.weight, saved)


FC6_WEIGHTS = ("fc6",) + hidden.FC7_WEIGHTS


def freeze_below_fc6(module_or_model) -> list:
    """``hidden.freeze_below_fc7``'s twin one layer further down: ``requires_grad = False`` on every parameter under ``module_or_model`` but the
    readout weights of the spiking heads in it and the detector head's ``fc6.weight`` and ``fc7.weight``; returns those parameters - what an
    optimiser is given.  The detector head's fc6 comes first, then its fc7, then the readout weights in ``freeze_hidden``'s order."""
    heads = [m for m in module_or_model.modules() if type(m).__name__ == "FastRCNNPredictorSNNFull"]
    keep = [m.fc6.weight for m in heads] + [m.fc7.weight for m in heads]
    for m in module_or_model.modules():
        for name in readout.READOUT_WEIGHTS.get(type(m).__name__, ()):
            keep.append(getattr(m, name).weight)
    ids = {id(w) for w in keep}
    for q in module_or_model.parameters():
        q.requires_grad_(id(q) in ids and q.requires_grad)
    return keep
