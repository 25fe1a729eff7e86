"""static.CapturedHeads on the GPU: the captured static path, its exchange rows, its slots, its refusals and what close() releases.

The model, the 128 x 256 pyramid (N = 2, C = 256, Hd = 1024, T = 8 / 12) and the three feature sets are those of tests/test_gpu_static.py and
tests/test_gpu_graph_capture.py (saturating, a fifth of the amplitude, silent).  Per configuration the eager static.heads_padded of every set is
computed once and kept on the host; a runner is then made ONCE per test (one warm-up, one capture per slot) and called six times over the sets
0 1 2 0 1 2, under torch's sync debug mode "error":

  - every key of runner(features) equals the eager call on the same features bit for bit; payload / payload_counts equal
    dp.pack_detections(static.unpad(eager), max_det); dp.unpack_detections of them gives unpad's boxes / scores / labels;
  - cap = 40 (saturated: roi_counts [40, 40] on set 0) and cap = 1000 at rpn.score_thresh = 0.5 (unsaturated, the images differ), slots 1 and 2;
    with two slots the tensors the previous call returned are unchanged after the next call;
  - bf16 channels-last features at precision "bf16" once;
  - a changed shape, dtype, layout or key raises ValueError, a changed num_steps / threshold / repacked weights RuntimeError, before any device work;
  - close() takes the runner's workspaces, and only those, out of ops._WS.captured / ops._WS_RATES.captured;
  - dp.all_gather_padded in a one-rank group equals all_gather_detections(unpad(out)).

Each test captures once and replays each graph a few times; nothing is retried."""
from collections import OrderedDict

import pytest
import torch

from tests.test_gpu_graph_capture import _static_sets, detector          # noqa: F401  (the fixture of the graph-capture tests: same model, same seed)
from tests.test_gpu_static import _images, _set_post_nms

pytestmark = pytest.mark.gpu

CONFIGS = {"cap40": dict(cap=40, max_det=140), "cap1000_thresh": dict(cap=1000, thresh=0.5, max_det=1100)}


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _to_device(s, dev, dtype=torch.float32, channels_last=False):
    out = OrderedDict((k, v.to(dev).to(dtype)) for k, v in s.items())
    return OrderedDict((k, v.contiguous(memory_format=torch.channels_last)) for k, v in out.items()) if channels_last else out


@pytest.fixture
def own_workspaces(monkeypatch):
    """fresh ops._Workspace objects for the test: what a runner's capture leaves in `captured` is then the test's to look at, not the process's"""
    from snn_automotive_object_detection_amd import ops
    ws, ws_rates = ops._Workspace(), ops._Workspace()
    monkeypatch.setattr(ops, "_WS", ws)
    monkeypatch.setattr(ops, "_WS_RATES", ws_rates)
    return ws, ws_rates


class _Configured:
    """the detector under a configuration, restored on exit"""
    def __init__(self, model, cfg):
        self.model, self.cfg = model, cfg
        self.heads = (model.rpn.head, model.roi_heads.box_head_and_predictor)

    def __enter__(self):
        _set_post_nms(self.model, self.cfg["cap"])
        self.model.rpn.score_thresh = self.cfg.get("thresh", 0.0)
        for h in self.heads:
            h.precision = "bf16" if self.cfg.get("bf16") else "bf16x3"
        return self.model

    def __exit__(self, *exc):
        self.model.rpn.score_thresh = 0.0
        for h in self.heads:
            h.precision = "bf16x3"
        return False


_EAGER = {}


def _eager(model, name, cfg, dev, sets):
    """the eager padded outputs of every feature set under cfg (model already configured): host copies, computed once per configuration"""
    from snn_automotive_object_detection_amd import static
    if name not in _EAGER:
        dtype = torch.bfloat16 if cfg.get("bf16") else torch.float32
        twins = []
        for s in sets:
            out = static.heads_padded(model, _to_device(s, dev, dtype, bool(cfg.get("bf16"))), _images())
            twins.append({k: v.cpu() for k, v in out.items()})
        _EAGER[name] = twins
    return _EAGER[name]


def _check_call(out, eager, max_det, dev):
    from snn_automotive_object_detection_amd import dp, static
    assert set(out) == set(eager) | {"payload", "payload_counts"}
    for k in eager:
        assert _same(out[k], eager[k]), "key %r of the replay differs from the eager call" % k
    lists = static.unpad(eager)
    ref_p, ref_c = dp.pack_detections(lists, max_det, torch.device("cpu"))
    assert _same(out["payload"], ref_p) and _same(out["payload_counts"], ref_c)
    back = dp.unpack_detections(out["payload"].cpu(), out["payload_counts"].cpu())
    assert len(back) == len(lists)
    for got, want in zip(back, lists):
        for k in ("boxes", "scores", "labels"):
            assert _same(got[k], want[k][:max_det]), k


def _six_calls(runner, model, name, cfg, dev, slots):
    sets = _static_sets()
    dtype = torch.bfloat16 if cfg.get("bf16") else torch.float32
    eager = _eager(model, name, cfg, dev, sets)
    feats = [_to_device(s, dev, dtype, bool(cfg.get("bf16"))) for s in sets]
    torch.cuda.synchronize()
    prev = prev_snap = None
    roi_counts = []
    for i in (0, 1, 2, 0, 1, 2):
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = runner(feats[i])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        _check_call(out, eager[i], cfg["max_det"], dev)
        roi_counts.append(out["roi_counts"].tolist())
        if slots == 2 and prev is not None:
            assert all(prev[k] is not out[k] for k in out), "two slots must not share output tensors"
            for k in prev:
                assert _same(prev[k], prev_snap[k]), "key %r of the previous call changed when the other slot replayed" % k
        prev, prev_snap = out, {k: v.clone() for k, v in out.items()}
    if slots == 1:
        again = runner(feats[0])
        assert all(prev[k] is again[k] for k in prev)                             # one slot: the same static tensors every call
    return roi_counts


@pytest.mark.parametrize("slots", [1, 2])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_runner_equals_eager_on_every_call(gpu_device, own_workspaces, detector, name, slots):            # noqa: F811
    from snn_automotive_object_detection_amd import static
    cfg = CONFIGS[name]
    with _Configured(detector, cfg) as model:
        example = _to_device(_static_sets()[2], gpu_device)
        runner = static.CapturedHeads(model, example, _images(), max_det=cfg["max_det"], slots=slots)
        try:
            counts = _six_calls(runner, model, name, cfg, gpu_device, slots)
        finally:
            runner.close()
    print("roi_counts per call", counts)
    assert counts[:3] == counts[3:]
    if cfg["cap"] == 40:
        assert counts[0] == [40, 40]
    else:
        assert max(counts[0]) < 1000 and any(c[0] != c[1] for c in counts[:3]), counts


def test_runner_on_bf16_channels_last_features(gpu_device, own_workspaces, detector):                      # noqa: F811
    from snn_automotive_object_detection_amd import ops, static
    cfg = dict(cap=40, max_det=140, bf16=True)
    with _Configured(detector, cfg) as model:
        sets = _static_sets()
        feats = [_to_device(s, gpu_device, torch.bfloat16, True) for s in sets]
        assert ops.levels_nhwc(list(feats[0].values()))
        eager = _eager(model, "cap40_bf16_nhwc", cfg, gpu_device, sets)
        nhwc_before = ops.feature_calls["nhwc"]
        runner = static.CapturedHeads(model, feats[0], _images(), max_det=140)
        assert ops.feature_calls["nhwc"] > nhwc_before                            # the typed channels-last entries took the maps as they are
        try:
            for i in (0, 1, 2):
                _check_call(runner(feats[i]), eager[i], 140, gpu_device)
            with pytest.raises(ValueError, match="layout"):                       # the same values in the default format are other features
                runner(OrderedDict((k, v.contiguous()) for k, v in feats[0].items()))
        finally:
            runner.close()


def test_refusals_after_capture_and_what_close_releases(gpu_device, own_workspaces, detector):            # noqa: F811
    from snn_automotive_object_detection_amd import dp, static
    ws, ws_rates = own_workspaces
    foreign = [torch.empty(64, dtype=torch.uint8, device=gpu_device), torch.empty(32, dtype=torch.uint8, device=gpu_device)]
    ws.captured.append(foreign[0])                                                # what somebody else's graph made the workspaces keep
    ws_rates.captured.append(foreign[1])
    cfg = CONFIGS["cap40"]
    with _Configured(detector, cfg) as model:
        feats = _to_device(_static_sets()[0], gpu_device)
        runner = static.CapturedHeads(model, feats, _images(), max_det=50, slots=2)
        try:
            mine = [b for b in ws.captured if b is not foreign[0]]
            assert mine and ws.captured[0] is foreign[0] and ws_rates.captured == [foreign[1]]
            out = runner(feats)
            eager = static.heads_padded(model, feats, _images())
            assert all(_same(out[k], eager[k]) for k in eager)
            ref_p, ref_c = dp.pack_detections(static.unpad(eager), 50, gpu_device)           # (where fg + bg > 50: the first 50 rows)
            assert _same(out["payload"], ref_p) and _same(out["payload_counts"], ref_c)
            print("fg + bg", eager["counts"].sum(1).tolist(), "rows", ref_c.tolist())
            torch.cuda.synchronize()
            # features that are not the captured ones: ValueError, nothing enqueued (the sync debug mode would not notice, the spec check is first)
            bad = [OrderedDict((k, v[:1]) for k, v in feats.items()), OrderedDict((k, v.half()) for k, v in feats.items()),
                   OrderedDict((k, v.contiguous(memory_format=torch.channels_last)) for k, v in feats.items()),
                   OrderedDict(list(feats.items())[:-1]), OrderedDict((k, v.cpu()) for k, v in feats.items())]
            for f in bad:
                with pytest.raises(ValueError, match="differ from the captured"):
                    runner(f)
            # settings the graph has baked in: RuntimeError naming them, and the runner works again once they are back
            head = model.rpn.head
            for obj, attr, value, word in ((head, "num_steps", 6, "num_steps"), (model.roi_heads.box_head_and_predictor, "precision", "bf16", "precision"),
                                           (model.roi_heads, "score_thresh", 0.3, "score_thresh"), (model.rpn, "nms_thresh", 0.6, "nms_thresh"),
                                           (head, "conv_route", "auto", "route")):
                old = getattr(obj, attr)
                setattr(obj, attr, value)
                try:
                    with pytest.raises(RuntimeError, match=word):
                        runner(feats)
                finally:
                    setattr(obj, attr, old)
            _set_post_nms(model, 41)
            with pytest.raises(RuntimeError, match="post_nms_top_n"):
                runner(feats)
            _set_post_nms(model, 40)
            assert all(_same(runner(feats)[k], eager[k]) for k in eager)
            head.invalidate_packed_weights()
            with pytest.raises(RuntimeError, match="packed weights"):
                runner(feats)
        finally:
            runner.close()
        assert ws.captured == [foreign[0]] and ws_rates.captured == [foreign[1]]  # the runner's are gone, the others are still there
        assert not any(b is m for b in ws.buf.values() for m in mine)
        with pytest.raises(RuntimeError, match="close"):
            runner(feats)
        runner.close()                                                            # (idempotent)


def test_all_gather_padded_in_a_one_rank_group(gpu_device, own_workspaces, detector):          # noqa: F811
    import torch.distributed as dist
    from snn_automotive_object_detection_amd import dp, static
    with _Configured(detector, CONFIGS["cap40"]) as model:
        out = static.heads_padded(model, _to_device(_static_sets()[1], gpu_device), _images())
    want_plain = dp.all_gather_detections(static.unpad(out), 60)                  # no process group at all
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % dp._free_port(), rank=0, world_size=1)
    try:
        want = dp.all_gather_detections(static.unpad(out), 60)
        rows = static.pack_padded_detections(out, 60)
        for got in (dp.all_gather_padded(out, 60), dp.all_gather_padded(rows, 60), dp.all_gather_padded(dict(out, payload=rows[0], payload_counts=rows[1]), 60),
                    dp.all_gather_padded(out, 60, images_per_rank=2)):
            assert len(got) == len(want) == len(want_plain) == 2
            for g, w, p in zip(got, want, want_plain):
                assert set(g) == {"boxes", "scores", "labels"}
                assert all(_same(g[k], w[k]) and _same(g[k], p[k]) for k in g)
        assert max(int(d["boxes"].shape[0]) for d in want) > 0
    finally:
        dist.destroy_process_group()
