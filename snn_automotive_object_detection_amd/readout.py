"""Readout fine-tuning: the exact gradients of the LI heads' weights - ``cls_logits`` / ``bbox_pred`` of the RPN head, ``cls_score`` /
``bbox_pred`` of the detector head - computed on the GPU from the spike planes a head pass left in its workspace
(include/snn_hip.h: snn_li_heads_wgrad).

The LI cell is linear and so is the bias-free 1x1 conv / linear in front of it, and the hidden spike trains do not depend on the readout
weights: out = W S with S[r][k] = sum_t kappa_t spk_t[r][k], so dL/dW[j][k] = sum_r g[r][j] S[r][k] - exact, no surrogate gradient, no
threshold ties.  That is ALL that is differentiated: features and the hidden weights (shared conv, fc6, fc7) get no gradient, there is no
loss, no sampler and no ``model.train()``.  Under ``precision = "bf16"`` / ``"mxfp6"`` the hidden spike train is the one the
rounded hidden weights produce, and at "bf16" the readout product itself ran on w.to(torch.bfloat16): the gradient is the one with respect to
the weight the pass multiplied, handed to the fp32 parameter unchanged (straight-through).

A head with ``train_readout = True`` returns, in grad mode and with a readout weight that requires grad, the outputs of its plain forward -
the same launches, bit for bit - with a ``grad_fn``.  The pass's planes of the last hidden layer are cloned out of the workspace first (the
next pass on that workspace overwrites them); backward is one snn_li_heads_wgrad call on the clone.  Everything is enqueued on the current
stream without a host synchronisation."""
import ctypes as C
from typing import Optional, Sequence, Tuple

import torch

from . import _lib, ops
from ._lib import snn_planes_view, snn_params

_WS_WGRAD = ops._Workspace()                  # slab partial sums of snn_li_heads_wgrad (must not alias the heads' workspace: the planes may lie there)


def _grad_rows(g, rows: int, what: str):
    if g is None:
        return None, 0
    g = ops._f32c(g)
    if g.dim() != 2 or g.shape[0] != rows:
        raise _lib.SnnHipError("%s must be [%d, n], got %s" % (what, rows, tuple(g.shape)))
    ops._need_gpu(g, what)
    return (g, int(g.shape[1])) if g.shape[1] else (None, 0)


def _result(t, n: int, n_cols: int, what: str):
    if t is None or n == 0:
        return None
    if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n * n_cols:
        raise _lib.SnnHipError("%s must be a contiguous fp32 GPU tensor of %d x %d elements" % (what, n, n_cols))
    return t


@ops._on_tensor_device
def li_heads_wgrad(planes: torch.Tensor, view: snn_planes_view, n_cols: int, T_prime: int, p: snn_params, grad_a: Optional[torch.Tensor],
                   grad_b: Optional[torch.Tensor], out: Optional[Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]] = None,
                   accumulate: bool = False):
    """(gw_a [NA, n_cols], gw_b [NB, n_cols]) with gw_x[j][k] = sum_r grad_x[r][j] * S[r][k], S the kappa fold of the first ``T_prime`` steps
    of the planes ``view`` describes inside ``planes`` (a workspace, or a copy of its plane region with offset_bytes = 0).  grad_a [rows, NA] /
    grad_b [rows, NB]; either may be None (its result is None).  ``out`` = (gw_a, gw_b): write into these tensors - or, with ``accumulate``,
    add to them.  Deterministic: two calls on the same data are bit-equal."""
    ops._need_gpu(planes, "spike planes")
    lib = _lib.load()
    rows = int(view.rows)
    grad_a, NA = _grad_rows(grad_a, rows, "grad_a")
    grad_b, NB = _grad_rows(grad_b, rows, "grad_b")
    dev = planes.device
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs `out`: the tensors to add to")
        gw_a = torch.empty((NA, n_cols), dtype=torch.float32, device=dev) if NA else None
        gw_b = torch.empty((NB, n_cols), dtype=torch.float32, device=dev) if NB else None
    else:
        gw_a, gw_b = _result(out[0], NA, n_cols, "out[0]"), _result(out[1], NB, n_cols, "out[1]")
        if (NA and gw_a is None) or (NB and gw_b is None):
            raise _lib.SnnHipError("out: a result tensor per gradient given")
    scratch = _WS_WGRAD.get(dev, max(16, lib.snn_li_heads_wgrad_workspace_bytes(rows, n_cols, NA, NB)))
    _lib.check(lib.snn_li_heads_wgrad(ops._ptr(planes), C.byref(view), int(n_cols), int(T_prime), C.byref(p), ops._ptr(grad_a), ops._ptr(grad_b),
                                      NA, NB, ops._ptr(gw_a), ops._ptr(gw_b), int(bool(accumulate)), ops._ptr(scratch), scratch.numel(),
                                      ops._stream()), "snn_li_heads_wgrad")
    return gw_a, gw_b


def readout_grads(planes: torch.Tensor, view: snn_planes_view, n_cols: int, p: snn_params, steps, grad_a, grad_b) -> dict:
    """{T': (gw_a, gw_b)} for every any-time readout T' of ``steps`` from ONE saved pass: the gradient of the readout at T' (the outputs of
    ``forward_readouts``) with respect to the readout weights.  grad_a / grad_b: one tensor for every T' (or None), or a sequence with one
    entry per step - the gradient of the loss on that readout's outputs."""
    steps = ops.check_steps(steps)
    if steps[-1] > int(view.steps_formed):
        raise ValueError("steps %r reach past the %d steps the pass formed" % (steps, int(view.steps_formed)))

    def per_step(g, what):
        if g is None or isinstance(g, torch.Tensor):
            return [g] * len(steps)
        g = list(g)
        if len(g) != len(steps):
            raise ValueError("%s: %d gradients for %d steps" % (what, len(g), len(steps)))
        return g
    ga, gb = per_step(grad_a, "grad_a"), per_step(grad_b, "grad_b")
    return {T: li_heads_wgrad(planes, view, n_cols, T, p, ga[j], gb[j]) for j, T in enumerate(steps)}


def save_planes(ws: torch.Tensor, view: snn_planes_view):
    """(a clone of the plane region ``view`` describes inside the workspace ``ws``, the view of that clone): what stays valid when the next
    pass overwrites the workspace"""
    off = int(view.offset_bytes)
    n = min(int(view.steps_formed) * int(view.step_stride_words) * 4, ws.numel() - off)
    own = snn_planes_view(0, view.step_stride_words, view.rows, view.words, view.layout, view.steps_formed, 0)
    return ws[off:off + n].clone(), own


def rpn_grad_rows(grads: Sequence[Optional[torch.Tensor]], shapes: Sequence[Sequence[int]], width: int, device=None) -> torch.Tensor:
    """per-level NCHW gradients [N, width, H, W] (None: zeros) -> the row order of the ABI, [P, width]: level-major, then n, y, x - the order of
    the head's position-major outputs.  shapes: (N, H, W) per level"""
    rows = []
    for g, (n, h, w) in zip(grads, shapes):
        if g is None:
            dev = device if device is not None else next(x.device for x in grads if x is not None)
            rows.append(torch.zeros((n * h * w, width), dtype=torch.float32, device=dev))
        else:
            if tuple(g.shape) != (n, width, h, w):
                raise ValueError("gradient of a level must be %s, got %s" % ((n, width, h, w), tuple(g.shape)))
            rows.append(g.to(torch.float32).permute(0, 2, 3, 1).reshape(n * h * w, width))
    return torch.cat(rows, 0)


class _Saved:
    """what backward needs of one pass (held by the graph, not by the module): the cloned planes and their view, the parameters, and how
    the gradients of the returned tensors become the rows of the ABI"""
    def __init__(self, outs, planes, view, n_cols, T, p, to_rows):
        self.outs, self.planes, self.view, self.n_cols, self.T, self.p, self.to_rows = tuple(outs), planes, view, n_cols, T, p, to_rows


class ReadoutGrad(torch.autograd.Function):
    """outputs of a finished head pass as a function of the two readout weights: forward returns the pass's own tensors, backward is one
    snn_li_heads_wgrad at T' = T on the saved planes.  Gradients go to the two weights alone."""

    @staticmethod
    def forward(ctx, w_a, w_b, saved: _Saved):
        outs, saved.outs = saved.outs, None                            # (the outputs hold the graph: it must not hold them)
        ctx.saved = saved
        ctx.shapes = (w_a.shape, w_b.shape)
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def backward(ctx, *grads):
        s = ctx.saved
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if all(g is None for g in grads):
            return None, None, None
        dev = next(g.device for g in grads if g is not None)
        if s.planes is None:                                          # (a pass over no rows: nothing ran, nothing arrives)
            return (torch.zeros(ctx.shapes[0], device=dev) if need_a else None, torch.zeros(ctx.shapes[1], device=dev) if need_b else None, None)
        g_a, g_b = s.to_rows(grads)
        gw_a, gw_b = li_heads_wgrad(s.planes, s.view, s.n_cols, s.T, s.p, g_a if need_a else None, g_b if need_b else None)

        def shaped(gw, shape, need):
            if not need:
                return None
            return torch.zeros(shape, dtype=torch.float32, device=dev) if gw is None else gw.view(shape)
        return shaped(gw_a, ctx.shapes[0], need_a), shaped(gw_b, ctx.shapes[1], need_b), None


def wanted(module, w_a, w_b) -> bool:
    """does this forward of ``module`` build the readout graph: ``train_readout`` set, grad mode on, a readout weight that requires grad"""
    if not getattr(module, "train_readout", False):
        return False
    if getattr(module, "spike_rates", False):
        raise NotImplementedError("train_readout with spike_rates: spike-rate mode returns rates, not outputs to put a loss on")
    return torch.is_grad_enabled() and (w_a.requires_grad or w_b.requires_grad)


def attach(w_a, w_b, outs, ws: Optional[torch.Tensor], view: Optional[snn_planes_view], n_cols: int, T: int, p: snn_params, to_rows):
    """the tensors ``outs`` of a pass that just ran in ``ws`` -> the same tensors with a grad_fn (ws None: the pass ran nothing)"""
    planes, own = save_planes(ws, view) if ws is not None else (None, None)
    outs = [o.detach() for o in outs]                                  # (the same storage; no view history of the pass's own tensors travels along)
    return ReadoutGrad.apply(w_a, w_b, _Saved(outs, planes, own, n_cols, T, p, to_rows))


READOUT_WEIGHTS = {"RPNHeadSNN": ("conv_cls", "conv_bbox"), "FastRCNNPredictorSNNFull": ("cls_score", "bbox_pred")}


def freeze_hidden(module_or_model) -> list:
    """``requires_grad = False`` on every parameter under ``module_or_model`` but the readout weights of the spiking heads in it (a head, or a
    whole model); returns those readout parameters - what an optimiser is given.  Why: the readout gradient is the only one this package
    computes.  Backbone, FPN, shared conv, fc6 and fc7 never receive one (a loss on the heads' outputs reaches them through nothing), so
    leaving them trainable would hand an optimiser parameters whose ``grad`` stays None, and weight decay or momentum would still move them
    while the spike planes the gradient was taken on assume them fixed."""
    keep = []
    for m in module_or_model.modules():
        for name in READOUT_WEIGHTS.get(type(m).__name__, ()):
            keep.append(getattr(m, name).weight)
    ids = {id(w) for w in keep}
    for q in module_or_model.parameters():
        if id(q) not in ids:
            q.requires_grad_(False)
    return keep
