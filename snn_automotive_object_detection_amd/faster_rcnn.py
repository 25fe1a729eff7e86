"""Drop-in for the reference's ``FastRCNNPredictorSNNFull`` (/root/reference/faster_rcnn.py:414-516)
on the MI355X kernels: same constructor, ``forward`` signature, return values and ``state_dict``
keys (``fc6.weight``, ``fc7.weight``, ``cls_score.weight``, ``bbox_pred.weight``; default
``nn.Linear`` init).  ``RoIHeadsSNN.forward`` (roi_heads.py:1230) can call it unchanged.
``spike_rates = True`` gives the faster_rcnn.py:520-618 variant (returns ONLY the rate list)."""
import torch
import os

from torch import nn

from . import fc6_grad, hidden, ops, readout
from .rpn import _SpikingHead, _WeightCache, _pack_heads_unchecked, _per_precision


class FastRCNNPredictorSNNFull(_SpikingHead):
    """
    Spiking box head + predictor: ``num_steps`` x { encoder -> fc6 -> LIF -> fc7 -> LIF ->
    {cls_score -> LI, bbox_pred -> LI} } on the flattened RoI features.

    Args (faster_rcnn.py:427-429):
        in_channels (int): number of input features (C*7*7)
        representation_size (int): size of the intermediate representation
        num_classes (int): number of output classes (including background)
        num_steps (int): simulation time steps (T_det)
        only_one_bbox (bool): 4 box outputs instead of 4 per class
        fc6_route, fc6_crossover: launch plan of fc6 + LIF per call (not in the reference; see __init__)
    """

    def __init__(self, in_channels, representation_size, num_classes, num_steps, only_one_bbox=False, fc6_route=None, fc6_crossover=None):
        super().__init__()
        self.num_steps = num_steps                                     # faster_rcnn.py:433
        # launch plan of fc6 + LIF, per call (include/snn_hip.h: snn_det_head_forward_routed): "sparse" (the default plan),
        # "dense", or "auto" (decided on the device from the density of the RoI features' period planes); None reads SNN_FC6_ROUTE at each
        # forward (default "sparse").  fc6_crossover: the hit rate above which "auto" takes the dense side (None:
        # SNN_FC6_ROUTE_DEFAULT_CROSSOVER).  route_stat: the last forward's device int32[4] = {hits, blocks, route taken, 0} (None on the
        # plain "sparse" path); never read here.  The readout methods keep the plain plan.
        self.fc6_route = fc6_route
        self.fc6_crossover = fc6_crossover
        self.route_stat = None
        self.dt = 0.001                                                # :436
        self.in_channels = in_channels
        self.representation_size = representation_size
        self.num_classes = num_classes
        self.p_enc = ops.LIFParameters(v_th=torch.tensor(0.25))        # :444
        self.p_lif = ops.LIFParameters(alpha=100, v_th=torch.tensor(0.1))   # :449,452
        self.li_order = "jump_first"
        self.spike_rates = False
        self.train_readout = False         # True: in grad mode, with cls_score.weight or bbox_pred.weight requiring grad, the outputs of forward /
                                           # forward_roialign carry a grad_fn to those two weights alone (readout.py); False: as ever
        self.train_fc7 = False             # True: in grad mode, with fc7.weight requiring grad, that grad_fn also reaches fc7.weight through a SuperSpike
                                           # lif7 (hidden.py; "bf16x3" / "f32" only, num_steps >= 3); False: as ever
        self.train_fc6 = False             # True: in grad mode, with fc6.weight requiring grad, the grad_fn reaches fc6.weight as well, through SuperSpike
                                           # lif7 and lif6 (fc6_grad.py; same limits); checked before train_fc7; False: as ever
        self.precision = "bf16x3"          # or "f32" (fp32 matrix cores) / "mxfp6" (fp4 x fp6 digit planes) / "bf16" (ONE bf16 weight plane: fc6, fc7
                                           # and the LI heads on w.to(torch.bfloat16) - outside the 1e-4-to-fp32 contract, as "mxfp6"); see RPNHeadSNN
        self.fc6 = nn.Linear(in_channels, representation_size, bias=False)          # :448
        self.fc7 = nn.Linear(representation_size, representation_size, bias=False)  # :451
        self.cls_score = nn.Linear(representation_size, num_classes, bias=False)    # :455
        self.only_one_bbox = only_one_bbox                                           # :460-467
        self.bbox_pred = nn.Linear(representation_size, 4 if only_one_bbox else num_classes * 4, bias=False)
        self._c6 = _per_precision()
        self._c7 = _per_precision()
        self._ch = _WeightCache()
        self._c6p = _WeightCache()              # fc6 in the permuted reduction order (fc6_inner)
        self._ch_bf16 = _WeightCache()          # "bf16": the LI heads' operand packed from the rounded values
        self._c6p_bf16 = _WeightCache()         # "bf16": fc6's single plane in the permuted order

    def _caches(self):
        return list(self._c6.values()) + list(self._c7.values()) + [self._ch, self._c6p, self._ch_bf16, self._c6p_bf16]

    def _split_weights(self, prec):
        if prec == "bf16":
            return ()
        return (self.cls_score.weight, self.bbox_pred.weight) + ((self.fc6.weight, self.fc7.weight) if prec == "bf16x3" else ())

    def _eff_precision(self) -> str:
        if self.precision == "mxfp6" and (self.in_channels % 128 or self.representation_size % 128):
            return "bf16x3"
        return self.precision

    def fc6_inner(self, prec=None) -> int:
        """49 when fc6's weights are packed in the permuted reduction order k' = bin * C + channel (include/snn_hip.h:
        snn_det_head_forward_k): bf16x3 on [C, 7, 7] inputs with C % 32 == 0 - what lets fc6's sparse period planes run on the
        structured-sparse matrix-core instruction.  0: the reference's order (SNN_FC6_PERM=0 forces it: A/B, tests)."""
        prec = prec or self._resolve_precision()
        # (mirrors the C side's gates: the permuted order needs the word-major fused bf16x3 layers - SNN_PLANES=rm, an A/B knob, switches
        # them off; any channel count that is a multiple of 32 is fine since round 5: k_permute_planes works in passes of 8 channel blocks)
        if prec not in ("bf16x3", "bf16") or os.environ.get("SNN_FC6_PERM") == "0" or os.environ.get("SNN_PLANES") == "rm":
            return 0
        return 49 if (self.in_channels % 49 == 0 and (self.in_channels // 49) % 32 == 0) else 0

    def _packed(self, prec=None, inner=None):
        """packed fc6, fc7, LI heads for `prec` (default: the precision this forward resolves to); ``inner`` = 0: fc6 in the
        reference's reduction order whatever fc6_inner() says (the stage-level ops read un-permuted planes)"""
        prec = prec or self._resolve_precision()
        pack = {"f32": ops.pack_linear, "f32_strict": ops.pack_linear, "bf16x3": lambda w: ops.pack_linear_bf16x3(w, check_split=False),
                "mxfp6": ops.pack_linear_mx, "bf16": ops.pack_linear_bf16}[prec]
        slot = "f32" if prec == "f32_strict" else prec
        inner = self.fc6_inner(prec) if inner is None else inner
        if inner and prec == "bf16":
            w6 = self._c6p_bf16.get((self.fc6.weight,), lambda w: ops.pack_linear_bf16(w, inner=inner))
        elif inner:
            w6 = self._c6p.get((self.fc6.weight,), lambda w: ops.pack_linear_bf16x3(w, check_split=False, inner=inner))
        else:
            w6 = self._c6[slot].get((self.fc6.weight,), pack)
        w7 = self._c7[slot].get((self.fc7.weight,), pack)
        if prec == "bf16":
            wh = self._ch_bf16.get((self.cls_score.weight, self.bbox_pred.weight), ops.pack_heads_bf16)
        else:
            wh = self._ch.get((self.cls_score.weight, self.bbox_pred.weight), _pack_heads_unchecked)
        return w6, w7, wh

    def _pass_args(self, width: int, got: str) -> dict:
        """the shapes, parameters and packed weights every forward variant hands to ops (ValueError on a wrong input width)"""
        prec = self._resolve_precision()
        w6, w7, wh = self._packed(prec)
        if width != self.in_channels:
            raise ValueError("expected %d input features, got %s" % (self.in_channels, got))
        return dict(Hd=self.representation_size, K=self.num_classes, K4=self.bbox_pred.weight.shape[0], p=self._params(prec),
                    w6_packed=w6, w7_packed=w7, w_heads_packed=wh, spike_rates=self.spike_rates, w6_inner=self.fc6_inner(prec))

    def _route_args(self, dev) -> dict:
        """the fc6 route of this forward: nothing on "sparse" (the plain entry: the launches of every earlier version), else the keywords
        of the routed entry with a fresh route_stat"""
        route = self.fc6_route if self.fc6_route is not None else os.environ.get("SNN_FC6_ROUTE", "sparse")
        if route == "sparse":
            self.route_stat = None
            return {}
        self.route_stat = torch.empty(4, dtype=torch.int32, device=dev)
        return dict(fc6_route=route, fc6_crossover=self.fc6_crossover, route_stat=self.route_stat)

    def forward(self, x):
        if self.train_fc6 and fc6_grad.wanted(self):
            cls, bbox = self._forward(x)
            R = int(cls.shape[0])
            return self._attach_fc6(cls, bbox, R, int(x[0].numel()) if R else self.in_channels,
                                    lambda steps, p: ops.encode_rows(x.flatten(start_dim=1), steps, p))
        if self.train_fc7 and hidden.wanted(self):
            cls, bbox = self._forward(x)
            R = int(cls.shape[0])
            return self._attach_fc7(cls, bbox, R, int(x[0].numel()) if R else self.in_channels)
        if self.train_readout and readout.wanted(self, self.cls_score.weight, self.bbox_pred.weight):
            cls, bbox = self._forward(x)
            R = int(cls.shape[0])
            return self._attach_readout(cls, bbox, R, int(x[0].numel()) if R else self.in_channels)
        return self._forward(x)

    def forward_roialign(self, feats, scales, rois, roi_level, roi_batch=None):
        """Same head fed straight from the FPN maps: MultiScaleRoIAlign(7x7, sampling 2) is fused with the encoder
        (the [R,C,7,7] RoI features of roi_heads.py:1217 are never materialised).  rois [R,5] = (image, x1,y1,x2,y2) - or, with
        ``roi_batch`` (int32 [R], the image of every row: the table ops.roi_assign writes), rois [R,4]."""
        if self.train_fc6 and fc6_grad.wanted(self):
            cls, bbox = self._forward_roialign(feats, scales, rois, roi_level, roi_batch)
            boxes, batch = (rois[:, 1:5], rois[:, 0]) if roi_batch is None else (rois, roi_batch)
            return self._attach_fc6(cls, bbox, int(cls.shape[0]), int(feats[0].shape[1]) * 49,
                                    lambda steps, p: ops.roi_align_encode(feats, scales, boxes, batch, roi_level, steps, p))
        if self.train_fc7 and hidden.wanted(self):
            cls, bbox = self._forward_roialign(feats, scales, rois, roi_level, roi_batch)
            return self._attach_fc7(cls, bbox, int(cls.shape[0]), int(feats[0].shape[1]) * 49)
        if self.train_readout and readout.wanted(self, self.cls_score.weight, self.bbox_pred.weight):
            cls, bbox = self._forward_roialign(feats, scales, rois, roi_level, roi_batch)
            return self._attach_readout(cls, bbox, int(cls.shape[0]), int(feats[0].shape[1]) * 49)
        return self._forward_roialign(feats, scales, rois, roi_level, roi_batch)

    def _attach_readout(self, cls, bbox, R: int, D: int):
        """the outputs of the pass that just ran, with a grad_fn that leads to cls_score.weight and bbox_pred.weight alone (readout.py;
        DESIGN.md 4.13): lif7's planes are cloned out of the workspace, backward is snn_li_heads_wgrad at T' = T on the clone"""
        from . import taps
        ws = view = p = None
        T = int(self.num_steps)
        with torch.no_grad():
            prec = self._resolve_precision()
            p = self._params(prec)
            if R:
                route = self.fc6_route if self.fc6_route is not None else os.environ.get("SNN_FC6_ROUTE", "sparse")
                _, view = taps.det_planes_views(R, D, self.representation_size, self.num_classes, int(self.bbox_pred.weight.shape[0]), T, p,
                                                w6_inner=self.fc6_inner(prec), route=route, spike_rates=False)
                ws = taps._current_ws(cls.device)
        return readout.attach(self.cls_score.weight, self.bbox_pred.weight, (cls, bbox), ws, view, self.representation_size, T, p, lambda g: g)

    def _attach_fc7(self, cls, bbox, R: int, D: int):
        """the outputs of the pass that just ran, with a grad_fn that leads to cls_score.weight, bbox_pred.weight and fc7.weight (hidden.py;
        DESIGN.md 4.15): lif6's first T - 1 steps and lif7's T steps leave the workspace as rows (snn_planes_to_rows), through the views of the
        pass - the same route and arguments as _attach_readout"""
        from . import taps
        ws = v6 = v7 = None
        T = int(self.num_steps)
        with torch.no_grad():
            prec = self._resolve_precision()
            p = self._params(prec)
            if R:
                route = self.fc6_route if self.fc6_route is not None else os.environ.get("SNN_FC6_ROUTE", "sparse")
                v6, v7 = taps.det_planes_views(R, D, self.representation_size, self.num_classes, int(self.bbox_pred.weight.shape[0]), T, p,
                                               w6_inner=self.fc6_inner(prec), route=route, spike_rates=False)
                ws = taps._current_ws(cls.device)
        return hidden.attach(self, (cls, bbox), ws, v6, v7, T, p, prec)

    def _attach_fc6(self, cls, bbox, R: int, D: int, encode):
        """_attach_fc7 one layer further down (fc6_grad.py): the grad_fn also leads to fc6.weight.  ``encode(steps, p)`` re-runs
        the stand-alone encoder on the feed of the pass that just ran - the features are still alive here - for its first T - 2 steps"""
        from . import taps
        ws = v6 = v7 = None
        T = int(self.num_steps)
        with torch.no_grad():
            prec = self._resolve_precision()
            p = self._params(prec)
            if R:
                route = self.fc6_route if self.fc6_route is not None else os.environ.get("SNN_FC6_ROUTE", "sparse")
                v6, v7 = taps.det_planes_views(R, D, self.representation_size, self.num_classes, int(self.bbox_pred.weight.shape[0]), T, p,
                                               w6_inner=self.fc6_inner(prec), route=route, spike_rates=False)
                ws = taps._current_ws(cls.device)
        return fc6_grad.attach(self, (cls, bbox), ws, v6, v7, T, p, prec, lambda steps: encode(steps, p))

    @torch.no_grad()
    def _forward(self, x):
        x = x.flatten(start_dim=1)                                     # :473
        out = ops.det_head_forward(x, T=int(self.num_steps), **self._pass_args(x.shape[1], "%d" % x.shape[1]), **self._route_args(x.device))
        return self._finish(out)

    @torch.no_grad()
    def _forward_roialign(self, feats, scales, rois, roi_level, roi_batch=None):
        if roi_batch is None:
            rois, roi_batch = rois[:, 1:5], rois[:, 0]
        out = ops.det_head_forward_roialign(feats, scales, rois, roi_batch, roi_level, T=int(self.num_steps),
                                            **self._pass_args(feats[0].shape[1] * 49, "%d x 49" % feats[0].shape[1]),
                                            **self._route_args(rois.device))
        return self._finish(out)

    @torch.no_grad()
    def forward_readouts(self, x, steps) -> dict:
        """Every T' of ``steps`` from ONE head pass at T = steps[-1]: {T': (class_logits, box_regression)}, or {T': rates} with
        ``spike_rates`` - each what ``forward`` returns for num_steps = T'.  ``num_steps`` is not touched."""
        steps = ops.check_steps(steps)
        x = x.flatten(start_dim=1)
        out = ops.det_head_forward_readouts(x, steps=steps, **self._pass_args(x.shape[1], "%d" % x.shape[1]))
        return self._finish_readouts(out, steps)

    @torch.no_grad()
    def forward_roialign_readouts(self, feats, scales, rois, roi_level, steps) -> dict:
        """forward_roialign with a readout per T' of ``steps`` (see forward_readouts)"""
        steps = ops.check_steps(steps)
        out = ops.det_head_forward_roialign_readouts(feats, scales, rois[:, 1:5], rois[:, 0], roi_level, steps=steps,
                                                     **self._pass_args(feats[0].shape[1] * 49, "%d x 49" % feats[0].shape[1]))
        return self._finish_readouts(out, steps)

    @torch.no_grad()
    def forward_tapped(self, x, raster: bool = False, rois_per_image=None):
        """``(class_logits, box_regression, taps)``: the head's outputs together with the spike taps of lif6 and lif7, from ONE pass.
        ``taps["lif6"]`` / ``taps["lif7"]``: ``per_step`` [n_images, T] int64, ``per_channel`` [n_images, representation_size] and
        ``per_roi`` [R] (int32, summed over the T steps) and, with ``raster``, ``raster`` [T, R, representation_size] torch.bool.
        ``rois_per_image``: how many consecutive RoIs belong to each image (None: one image).  ``taps["pass"]``: the pass's own per-RoI
        counts and time sums (energy.rates_from_taps).
        The pass is the one spike-rate mode runs, bit for bit (outputs, counts, sums) - the plan of spike-rate mode, whose fc6 window is
        one step longer so that every lif6 plane is formed, not a promise about the launches of a plain ``forward``.  ``spike_rates``,
        ``num_steps`` and ``route_stat`` are not touched (spike-rate mode runs the plain fc6 plan on every route)."""
        from . import taps as _taps
        x = x.flatten(start_dim=1)
        args = self._pass_args(x.shape[1], "%d" % x.shape[1])
        return _taps.det_head_tapped(x, T=int(self.num_steps), raster=raster, rois_per_image=rois_per_image, only_one_bbox=self.only_one_bbox, **args)

    @torch.no_grad()
    def forward_roialign_tapped(self, feats, scales, rois, roi_level, roi_batch=None, raster: bool = False, rois_per_image=None):
        """``forward_tapped`` for the head fed straight from the FPN maps (see ``forward_roialign`` for the RoI arguments)"""
        from . import taps as _taps
        if roi_batch is None:
            rois, roi_batch = rois[:, 1:5], rois[:, 0]
        args = self._pass_args(feats[0].shape[1] * 49, "%d x 49" % feats[0].shape[1])
        return _taps.det_head_roialign_tapped(feats, scales, rois, roi_batch, roi_level, T=int(self.num_steps), raster=raster,
                                              rois_per_image=rois_per_image, only_one_bbox=self.only_one_bbox, **args)

    def _rates(self, extras, T):
        """faster_rcnn.py:568-618: four [R, 2] = (rate, "FLOPs") tensors - lif6, lif7, cls_score, bbox_pred - finished by
        snn_det_rates from the integer spike counts of the LIF epilogues and the time-summed LI membranes (one launch)"""
        rates = ops.det_rates(extras, self.in_channels, self.representation_size, self.num_classes,
                              self.bbox_pred.weight.shape[0], T, self.only_one_bbox)
        return [rates[0], rates[1], rates[2], rates[3]]

    def _finish_readouts(self, out, steps):
        cls, bbox, extras = out
        return {T: self._rates(tuple(e[j] for e in extras), T) if self.spike_rates else (cls[j], bbox[j]) for j, T in enumerate(steps)}

    def _finish(self, out):
        cls, bbox, extras = out
        if not self.spike_rates:
            return cls, bbox                                           # :513-516
        self.last_spike_counts = (extras[0], extras[1])
        return self._rates(extras, int(self.num_steps))
