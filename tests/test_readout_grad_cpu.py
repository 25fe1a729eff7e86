"""Readout weight gradients without a GPU: header <-> library <-> binding signatures of the two entries, the argument checks of
snn_li_heads_wgrad (every refusal comes back as -1 with a message before any device work: this machine has no device), the monotone scratch
query, and the NCHW -> row-order mapping the RPN head's backward uses, against a plain torch permutation."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("snn_li_heads_wgrad_workspace_bytes", "snn_li_heads_wgrad")


def _L():
    from snn_automotive_object_detection_amd import _lib
    return _lib


def _params(order=0):
    L = _L()
    return L.snn_params(0.1, -0.2, 0.0, 0.0, 0.25, 0.1, order, L.PRECISIONS["bf16x3"])


def _view(rows=100, words=8, layout=0, steps=8, stride=None, offset=0):
    return _L().snn_planes_view(offset, rows * words if stride is None else stride, rows, words, layout, steps, 0)


def test_header_library_and_binding_agree_on_the_two_entries():
    L = _L()
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snn_hip.h")).read(), flags=re.S)
    m = re.search(r"size_t snn_li_heads_wgrad_workspace_bytes\(([^)]*)\);", hdr)
    assert m and [a.strip().rsplit(" ", 1)[0] for a in m.group(1).split(",")] == ["int64_t", "int", "int", "int"]
    m = re.search(r"\bint snn_li_heads_wgrad\(([^)]*)\);", hdr)
    assert m
    types = [re.sub(r"\s+", " ", a).strip().rsplit(" ", 1)[0] for a in m.group(1).split(",")]
    assert types == ["const void*", "const snn_planes_view*", "int", "int", "const snn_params*", "const float*", "const float*", "int", "int",
                     "float*", "float*", "int", "void*", "size_t", "snn_stream_t"]
    for name in ENTRIES:
        assert name in L.SYMBOLS and hasattr(lib, name), name
    res, args = L.SYMBOLS["snn_li_heads_wgrad_workspace_bytes"]
    assert res is C.c_size_t and args == [C.c_int64, C.c_int, C.c_int, C.c_int]
    res, args = L.SYMBOLS["snn_li_heads_wgrad"]
    ptr, view, par = C.c_void_p, C.POINTER(L.snn_planes_view), C.POINTER(L.snn_params)
    assert res is C.c_int and args == [ptr, view, C.c_int, C.c_int, par, ptr, ptr, C.c_int, C.c_int, ptr, ptr, C.c_int, ptr, C.c_size_t, L.c_stream]
    # the kernels are in their own file, included by the one translation unit
    csrc = os.path.join(ROOT, "snn_automotive_object_detection_amd", "csrc")
    assert '#include "snn_wgrad.h"' in open(os.path.join(csrc, "snn_kernels.hip")).read() and os.path.exists(os.path.join(csrc, "snn_wgrad.h"))
    assert "atomic" not in re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "snn_wgrad.h")).read())


def test_the_ops_name_forwards_to_the_readout_module():
    from snn_automotive_object_detection_amd import ops, readout
    import inspect
    assert "readout.li_heads_wgrad(" in inspect.getsource(ops.li_heads_wgrad)
    with pytest.raises(Exception, match="GPU"):
        ops.li_heads_wgrad(torch.zeros(64, dtype=torch.uint8), _view(2, 1, 0, 1), 32, 1, _params(), torch.zeros(2, 3), None)
    assert callable(readout.readout_grads) and callable(readout.freeze_hidden)


BAD = [
    # what,                         overrides of the good call
    ("null view",                   dict(view=None)),
    ("null planes",                 dict(planes=None)),
    ("unknown layout",              dict(view=_view(layout=3))),
    ("split4 with words % 4",       dict(view=_view(words=6, layout=1))),
    ("T' = 0",                      dict(T=0)),
    ("T' = steps_formed + 1",       dict(T=9)),
    ("n_cols > 32 words",           dict(n_cols=257)),
    ("n_cols = 0",                  dict(n_cols=0)),
    ("NA + NB = 0",                 dict(NA=0, NB=0)),
    ("NA + NB > 480",               dict(NA=96, NB=385)),
    ("negative NA",                 dict(NA=-1, NB=5)),
    ("short scratch",               dict(short=4)),
    ("null scratch",                dict(scratch=None)),
    ("null parameters",             dict(p=None)),
    ("null grad_a with NA",         dict(ga=None)),
    ("null gw_b with NB",           dict(wb=None)),
    ("accumulate = 2",              dict(acc=2)),
    ("a step stride below a plane", dict(view=_view(stride=799))),
]


@pytest.mark.parametrize("what,over", BAD, ids=[b[0] for b in BAD])
def test_bad_arguments_return_minus_one_with_a_message_and_no_device_work(what, over):
    L = _L()
    lib = L.load()
    fake = (C.c_uint8 * 64)()                                        # never dereferenced: every call is refused on the host
    ptr = C.c_void_p(C.addressof(fake))
    a = dict(planes=ptr, view=_view(), n_cols=256, T=8, p=_params(), ga=ptr, gb=ptr, NA=3, NB=12, wa=ptr, wb=ptr, acc=0, scratch=ptr, short=0)
    a.update(over)
    v, p = a["view"], a["p"]
    need = lib.snn_li_heads_wgrad_workspace_bytes(100, 256, 3, 12)
    assert need > 0
    rc = lib.snn_li_heads_wgrad(a["planes"], C.byref(v) if v is not None else None, a["n_cols"], a["T"], C.byref(p) if p is not None else None,
                                a["ga"], a["gb"], a["NA"], a["NB"], a["wa"], a["wb"], a["acc"], a["scratch"], need - a["short"], None)
    assert rc == -1, (what, rc)
    msg = lib.snn_last_error()
    assert msg and b"snn_li_heads_wgrad" in msg, (what, msg)


def test_a_head_without_outputs_may_leave_its_pointers_null_up_to_the_checks():
    """NA = 0 with null (grad_a, gw_a) passes every check but the one that is made wrong here on purpose (the scratch): the refusal names the
    scratch, not the null pair"""
    L = _L()
    lib = L.load()
    fake = (C.c_uint8 * 64)()
    ptr = C.c_void_p(C.addressof(fake))
    v, p = _view(), _params(1)
    rc = lib.snn_li_heads_wgrad(ptr, C.byref(v), 256, 8, C.byref(p), None, ptr, 0, 7, None, ptr, 0, ptr, 0, None)
    assert rc == -1 and b"scratch" in lib.snn_last_error()
    rc = lib.snn_li_heads_wgrad(ptr, C.byref(v), 256, 8, C.byref(p), ptr, None, 5, 0, ptr, None, 1, ptr, 0, None)
    assert rc == -1 and b"scratch" in lib.snn_last_error()


def test_workspace_bytes_is_monotone_and_zero_outside_the_limits():
    lib = _L().load()
    q = lib.snn_li_heads_wgrad_workspace_bytes
    rows = (1, 63, 64, 65, 257, 1031, 2000, 32768, 32769, 196416, 2 ** 31 - 1)
    cols = (1, 20, 96, 256, 1024, 8192)
    outs = ((1, 0), (0, 1), (1, 4), (3, 12), (9, 36), (91, 364), (96, 384))
    for c in cols:
        for na, nb in outs:
            sizes = [q(r, c, na, nb) for r in rows]
            assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (c, na, nb, sizes)
    for r in rows:
        for na, nb in outs:
            sizes = [q(r, c, na, nb) for c in cols]
            assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes), (r, na, nb, sizes)
        for c in cols:
            sizes = [q(r, c, na, nb) for na, nb in outs]
            assert sizes == sorted(sizes), (r, c, sizes)
            assert q(r, c, 3, 12) == q(r, c, 12, 3) == q(r, c, 15, 0)             # (a function of NA + NB)
    # at least one float per (slab, output, column), at most 512 slabs; headline shapes
    assert q(1, 20, 1, 4) == 5 * 20 * 4 and q(65, 256, 3, 12) == 2 * 15 * 256 * 4
    assert q(196416, 256, 3, 12) == 512 * 15 * 256 * 4 and q(2000, 1024, 9, 36) == 32 * 45 * 1024 * 4
    for bad in ((0, 256, 3, 12), (2 ** 31, 256, 3, 12), (10, 0, 3, 12), (10, 8193, 3, 12), (10, 256, 0, 0), (10, 256, -1, 3), (10, 256, 96, 385)):
        assert q(*bad) == 0, bad


def test_rpn_gradient_rows_are_the_plain_permutation():
    """per-level NCHW gradients -> [P, width] in the order of the head's position-major outputs (level-major, then n, y, x), None as zeros"""
    from snn_automotive_object_detection_amd import readout
    g = torch.Generator().manual_seed(5)
    shapes = ((2, 5, 7), (2, 3, 1), (2, 1, 1))
    for width in (3, 12, 5):
        grads = [torch.randn((n, width, h, w), generator=g) for n, h, w in shapes]
        want = torch.cat([x.permute(0, 2, 3, 1).reshape(-1, width) for x in grads])
        got = readout.rpn_grad_rows(grads, shapes, width)
        assert got.shape == (sum(n * h * w for n, h, w in shapes), width) and torch.equal(got, want)
        # element by element: row of (level, n, y, x), column a
        row0 = 0
        for x, (n, h, w) in zip(grads, shapes):
            for (i, y, xx, a) in ((0, 0, 0, 0), (n - 1, h - 1, w - 1, width - 1), (1, h // 2, w // 2, 1)):
                assert got[row0 + (i * h + y) * w + xx, a] == x[i, a, y, xx]
            row0 += n * h * w
        # what the head's own views do to position-major outputs is undone by it
        rows = torch.randn((want.shape[0], width), generator=g)
        views, pos = [], 0
        for n, h, w in shapes:
            views.append(rows[pos:pos + n * h * w].view(n, h, w, width).permute(0, 3, 1, 2))
            pos += n * h * w
        assert torch.equal(readout.rpn_grad_rows(views, shapes, width), rows)
        holes = [grads[0], None, grads[2]]
        got = readout.rpn_grad_rows(holes, shapes, width)
        assert torch.equal(got[:70], want[:70]) and not got[70:76].any() and torch.equal(got[76:], want[76:])
    with pytest.raises(ValueError):
        readout.rpn_grad_rows([torch.zeros(2, 3, 7, 5)], ((2, 5, 7),), 3)


def test_train_readout_defaults_off_and_refuses_spike_rates():
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import readout
    h, d = S.RPNHeadSNN(32, 3, 4), S.FastRCNNPredictorSNNFull(49 * 8, 32, 3, 4)
    assert h.train_readout is False and d.train_readout is False
    for m, x in ((h, [torch.randn(1, 32, 4, 4)]), (d, torch.randn(2, 8, 7, 7))):
        m.train_readout = m.spike_rates = True
        with pytest.raises(NotImplementedError, match="train_readout"):
            m(x)
    # freeze_hidden: everything but the readout weights stops requiring grad; they are returned
    for m, names in ((h, ("conv_cls", "conv_bbox")), (d, ("cls_score", "bbox_pred"))):
        keep = readout.freeze_hidden(m)
        assert [id(w) for w in keep] == [id(getattr(m, n).weight) for n in names]
        assert sorted(n for n, q in m.named_parameters() if q.requires_grad) == sorted(n + ".weight" for n in names)
    from snn_automotive_object_detection_amd.roi_heads import RoIHeadsSNN
    assert callable(RoIHeadsSNN.head_outputs)
