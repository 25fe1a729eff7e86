"""snn_pack_padded_detections (k_pack_padded_detections) on the GPU: padded detections -> the exchange rows of dp.py.

Every case runs the kernel, through the C ABI, into buffers the TEST owns and pre-fills with 0xff, against (1) the contract restated in plain torch
on the host (tests/test_static_runner_cpu.rows_expected) and (2) dp.pack_detections(static.unpad(out), max_det), bit for bit.  Input rows at or
past an image's count hold NaN, labels included as a bit pattern no label has, so anything read from them shows; the calls of one case go into
the SAME buffers one after the other, so what a call leaves unwritten shows as the residue of the one before.

Shapes: N 1 / 3; out_cap 5 / 17 / 140 (no multiples of a 16-byte vector's rows); max_det below, equal to and above out_cap - odd (8-byte stores)
and even (16-byte stores) - and, beyond what one tile of 256 rows holds: 530 / 531 rows (three tiles, the last one ragged) and 16642 / 16641 rows
(66 tiles on a grid of 64: two blocks per image take a second tile).
Counts: (0, 0); foreground only; background only; fg + bg == out_cap; fg + bg > max_det (the first max_det rows are kept); garbage (-7, 2^30),
clamped to out_cap on the device."""
import ctypes as C

import pytest
import torch

from tests.test_static_runner_cpu import rows_expected

pytestmark = pytest.mark.gpu

GARBAGE = (-7, 1 << 30)
SHAPES = [(n, cap, md) for n in (1, 3) for cap in (5, 17, 140) for md in (cap - 2, cap, cap + 3)] + \
         [(3, 600, 530), (3, 600, 531), (1, 140, 16642), (2, 140, 16641)]


def _patterns(cap, max_det):
    """(fg, bg) per image, six kinds"""
    over = (min(cap, max_det + 1) - 1, 1) if max_det < cap else (cap - 1, 1)           # fg + bg > max_det where out_cap allows it
    return [(0, 0), (min(3, cap), 0), (0, min(4, cap)), (cap - 2, 2), over, GARBAGE]


def _draw(N, cap, counts, seed):
    """valid rows: random boxes / scores, labels 1 .. 95 on foreground rows and 0 on background rows; the other rows NaN / 0x7fc00000"""
    g = torch.Generator().manual_seed(seed)
    boxes = torch.rand((N, cap, 4), generator=g) * 512
    scores = torch.rand((N, cap), generator=g)
    labels = torch.randint(1, 96, (N, cap), generator=g, dtype=torch.int32)
    labels[:, 0], labels[:, -1] = 95, 1
    for i, (fg, bg) in enumerate(counts):
        k = min(max(fg + bg, 0), cap)
        if (fg, bg) != GARBAGE:
            labels[i, fg:k] = 0
        boxes[i, k:], scores[i, k:], labels[i, k:] = float("nan"), float("nan"), 0x7fc00000
    return boxes, scores, labels, torch.tensor(counts, dtype=torch.int32).reshape(N, 2)


def _bits(t):
    return t.cpu().contiguous().view(torch.int32)


def _run_into(lib, dev_in, N, cap, max_det, payload, counts):
    from snn_automotive_object_detection_amd import _lib
    b, s, l, c = dev_in
    rc = lib.snn_pack_padded_detections(C.c_void_p(b.data_ptr()), C.c_void_p(s.data_ptr()), C.c_void_p(l.data_ptr()), C.c_void_p(c.data_ptr()), N, cap,
                                        max_det, C.c_void_p(payload.data_ptr()), C.c_void_p(counts.data_ptr()), torch.cuda.current_stream().cuda_stream)
    _lib.check(rc, "snn_pack_padded_detections")


def _as_out(dev_in):
    """the dict static.unpad reads, with the fields this call does not look at empty"""
    b, s, l, c = dev_in
    N = b.shape[0]
    return {"boxes": b, "scores": s, "labels": l, "counts": c, "roi_counts": torch.zeros(N, dtype=torch.int32, device=b.device),
            "all_scores": torch.zeros((N, 1, 2), device=b.device), "all_boxes": torch.zeros((N, 1, 2, 4), device=b.device)}


@pytest.mark.parametrize("N,cap,max_det", SHAPES, ids=["N%d_cap%d_max%d" % s for s in SHAPES])
def test_rows_equal_the_contract_and_pack_detections(gpu_device, N, cap, max_det):
    from snn_automotive_object_detection_amd import _lib, dp, ops, static
    lib = _lib.load()
    pats = _patterns(cap, max_det)
    payload = torch.empty((N, max_det, 6), dtype=torch.float32, device=gpu_device)
    counts = torch.empty((N,), dtype=torch.int32, device=gpu_device)
    payload.view(torch.uint8).fill_(0xff)
    counts.view(torch.uint8).fill_(0xff)
    n_calls = 4 if N == 3 else 6
    seen = set()
    for call in range(n_calls):
        shift = 1 if N == 3 and call >= 2 else 0                                              # N = 3: kinds 012 345 123 450
        per_image = [pats[(call * N + i + shift) % len(pats)] for i in range(N)]
        seen.update(per_image)
        host = _draw(N, cap, per_image, 100 * call + N)
        dev_in = [t.to(gpu_device) for t in host]
        _run_into(lib, dev_in, N, cap, max_det, payload, counts)
        exp_p, exp_c = rows_expected(*host, max_det)
        assert not torch.isnan(exp_p).any()                                                   # (the expectation itself never reaches a NaN row)
        assert torch.equal(counts.cpu(), exp_c), (call, per_image, counts.tolist(), exp_c.tolist())
        assert torch.equal(_bits(payload), _bits(exp_p)), (call, per_image)
        ref_p, ref_c = dp.pack_detections(static.unpad(_as_out(dev_in)), max_det, gpu_device)
        assert torch.equal(_bits(ref_p), _bits(payload)) and torch.equal(ref_c, counts), (call, per_image)
        for i, (fg, bg) in enumerate(per_image):                                              # truncation and the garbage clamp, spelled out
            assert exp_c[i] == (min(cap, max_det) if (fg, bg) == GARBAGE else min(fg + bg, max_det))
    assert seen == set(pats)
    # the wrapper: the same rows in tensors of its own, and dp.unpack_detections reads them back as unpad's boxes / scores / labels
    w_p, w_c = ops.pack_padded_detections(_as_out(dev_in), max_det)
    assert w_p.shape == (N, max_det, 6) and w_c.dtype == torch.int32 and torch.equal(_bits(w_p), _bits(payload)) and torch.equal(w_c, counts)
    for got, want in zip(dp.unpack_detections(w_p, w_c), static.unpad(_as_out(dev_in))):
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(got[k], want[k][:max_det]), k


def test_wrapper_refuses_bad_shapes(gpu_device):
    from snn_automotive_object_detection_amd import ops
    from snn_automotive_object_detection_amd._lib import SnnHipError
    out = _as_out([t.to(gpu_device) for t in _draw(2, 5, [(1, 1), (0, 0)], 1)])
    with pytest.raises(SnnHipError, match="max_det"):
        ops.pack_padded_detections(out, 0)
    with pytest.raises(SnnHipError, match="expected"):
        ops.pack_padded_detections(dict(out, scores=out["scores"][:, :4]), 5)
