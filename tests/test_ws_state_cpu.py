"""The workspace seam of tests/_ws_state.py proves itself on the host, and nothing bypasses it (CPU).

  1. four fake "library calls" written in torch run through a GuardedWorkspace on the CPU: one reads a byte it did not write, one writes
     one byte past `nbytes`, one leaves a flag behind that changes its next result - the harness flags each, by the check that is meant to -
     and a well-behaved one passes every fill and every sequence;
  2. coverage: every _WS.get( / _WS_RATES.get( call site of ops.py, mapped to the public function it serves, is an entry of
     _ws_state.ENTRIES, and tests/test_gpu_ws_state.py has a builder for every entry: a new workspace-taking function without a state
     test fails here;
  3. the size queries of every shape the GPU file uses: positive, the _routed ones at least the plain ones, monotone in T, R, N and the
     level shapes (the library loads without a GPU)."""
import ctypes as C

import pytest
import torch

from tests import _ws_state as W

CPU = torch.device("cpu")


# ---- 1. the harness on fake calls ------------------------------------------------------------------------------------------------------
class FakeLib:
    """y = 2 x + 1 through n data bytes and one counter byte of scratch, the way ops reaches the library: size query, _WS.get, the call"""

    def __init__(self, kind: str):
        self.kind = kind
        self._WS = W.GuardedWorkspace(CPU, 1 << 16)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        n = x.numel()
        ws = self._WS.get(CPU, n + 1)
        if self.kind == "reads_unwritten":
            ws[:n - 1] = (2 * x)[:n - 1]                   # (the last data byte is read below and was never written)
        else:
            ws[:n] = 2 * x
        if self.kind == "writes_past":
            torch.as_strided(ws, (n + 2,), (1,))[n + 1] = 7    # one byte past the region it was told about
        if self.kind == "leaves_flag":                     # a counter that is read before anybody cleared it, and left set
            seen = int(ws[n] == 0x77)
        else:
            ws[n] = 0
            seen = int(ws[n])
        ws[n] = 0x77 if self.kind == "leaves_flag" else 0
        return ws[:n].clone() + 1 + seen


def _call(lib, x):
    return lambda: W.snapshot(lib(x))


X = torch.arange(40, dtype=torch.uint8)


def test_a_well_behaved_call_passes_every_fill_and_sequence():
    lib = FakeLib("good")
    snap = W.run_fills([lib._WS], _call(lib, X))
    assert torch.equal(snap[1], 2 * X + 1)
    small, large = X[:7], torch.cat([X, X])
    W.run_sequence([lib._WS], [_call(lib, large), _call(lib, small), _call(lib, X), _call(lib, large)], start_fill=0xff)
    assert lib._WS.sizes == [81, 8, 41, 81]                # (each step was told exactly its own size)


def test_a_read_before_a_write_is_flagged_by_the_fills():
    lib = FakeLib("reads_unwritten")
    with pytest.raises(AssertionError, match="fill 0x5a against 0x00"):
        W.run_fills([lib._WS], _call(lib, X))
    W.armed_call([lib._WS], 0x00, _call(lib, X))           # (on zeros alone nothing shows: the suite's usual state)


def test_a_write_past_the_end_is_flagged_by_the_tail_at_its_offset():
    lib = FakeLib("writes_past")
    with pytest.raises(AssertionError, match=r"interior written at region end \+ 0:"):
        W.armed_call([lib._WS], 0x00, _call(lib, X))
    lib._WS.arm(0x00)
    lib._WS.back[5] = 1
    with pytest.raises(AssertionError, match=r"back guard touched at region end \+ %d" % ((1 << 16) + 5)):
        lib._WS.check()
    lib._WS.arm(0x00)
    lib._WS.front[-1] = 1
    with pytest.raises(AssertionError, match=r"front guard touched at region end - 1 "):
        lib._WS.check()


def test_a_flag_left_behind_is_flagged_by_the_sequence():
    lib = FakeLib("leaves_flag")
    W.run_fills([lib._WS], _call(lib, X))                  # (no fill is the flag's value: each call alone is right)
    with pytest.raises(AssertionError, match="step 1 of the sequence differs from the same call alone"):
        W.run_sequence([lib._WS], [_call(lib, X), _call(lib, X)])


def test_get_hands_out_exactly_the_size_and_keeps_the_view_for_smaller_requests():
    ws = W.GuardedWorkspace(CPU, 1 << 16)
    assert ws.interior.data_ptr() % 4096 == 0 and ws.front.numel() == ws.back.numel() == 1 << 20
    assert ws.front.data_ptr() + (1 << 20) == ws.interior.data_ptr() and ws.interior.data_ptr() + (1 << 16) == ws.back.data_ptr()
    ws.arm(0x5a)
    v = ws.get(CPU, 1000)
    assert v.numel() == 1000 and v.data_ptr() == ws.interior.data_ptr() and ws.sizes == [1000]
    assert ws.get(CPU, 1).data_ptr() == v.data_ptr() and ws.get(CPU, 1).numel() == 1000 and ws.sizes == [1000]       # the plane readers
    assert bool((ws.interior == 0x5a).all()) and ws.untouched()                                                          # get never writes
    assert ws.get(CPU, 1001).numel() == 1001
    ws.forget()
    assert ws.get(CPU, 10).numel() == 10 and ws.high == 1001
    ws.short_by = 1
    ws.forget()
    assert ws.get(CPU, 500).numel() == 499 and ws.get(CPU, 1).numel() == 499
    with pytest.raises(AssertionError, match="the interior holds"):
        ws.get(CPU, (1 << 16) + 1)


def test_snapshots_compare_bits_and_poisoned_outputs_are_told_apart():
    nan = torch.full((3,), float("nan"))
    assert W.same_bits(W.snapshot(nan, None, [1, (2, torch.zeros(2, dtype=torch.int32))]), W.snapshot(nan.clone(), None, [1, (2, torch.zeros(2, dtype=torch.int32))]))
    assert not W.same_bits(W.snapshot(torch.tensor([0.0])), W.snapshot(torch.tensor([-0.0])))
    assert not W.same_bits(W.snapshot(torch.zeros(2)), W.snapshot(torch.zeros(3)))
    assert "part 1: 2 of 8 bytes differ, the first at byte 6" in W.first_difference(W.snapshot(torch.zeros(2)), W.snapshot(torch.tensor([0.0, 1.5])))
    rec = []
    with W.poisoned_outputs(rec):
        a, b, c = torch.empty((2, 3)), torch.empty((4,), dtype=torch.int32), torch.empty_like(torch.zeros(5))
    assert len(rec) == 3 and all(W.still_poisoned(t) for t in rec) and torch.empty is not None
    a[1, 2] = 0.0
    b[0] = 0
    assert not W.still_poisoned(a) and not W.still_poisoned(b) and W.still_poisoned(c)
    assert torch.empty.__module__ != __name__ and not torch.isnan(torch.empty_like(torch.zeros(4)).fill_(1.0)).any()  # (both restored)


# ---- 2. coverage -----------------------------------------------------------------------------------------------------------------------
def test_every_workspace_call_site_of_ops_is_an_entry():
    import inspect
    import re

    from snn_automotive_object_detection_amd import ops
    sites = W.workspace_call_sites(ops)
    assert set(sites) == set(W.ENTRIES), "ops.py and _ws_state.ENTRIES disagree: %s" % sorted(set(sites) ^ set(W.ENTRIES))
    src = inspect.getsource(ops)
    n_text = len(re.findall(r"\b_WS(?:_RATES)?\.get\(", src))
    n_mapped = sum(len(v) for v in W.direct_sites(ops).values())
    assert n_text == n_mapped >= 11, "%d workspace call sites in ops.py, %d of them inside a top-level function" % (n_text, n_mapped)
    # the helpers are private and every public caller of them is listed: _det_ws serves four entries, _rpn_rates two
    assert {f for f, w in sites if w == "_WS_RATES"} == {"rpn_head_forward", "rpn_head_forward_readouts"}
    assert sites[("det_head_forward", "_WS")] == 2 and sites[("det_head_forward_roialign", "_WS")] == 2
    assert all(hasattr(ops, f) for f, _ in W.ENTRIES)
    # nothing else in the package obtains a workspace of its own
    assert isinstance(ops._WS, ops._Workspace) and isinstance(ops._WS_RATES, ops._Workspace)


def test_the_map_sees_a_new_entry_and_a_new_helper():
    import types
    fake = types.ModuleType("fake_ops")
    src = ("_WS = None\n_WS_RATES = None\n"
           "def _inner(dev):\n    return _WS.get(dev, 4)\n"
           "def _outer(dev):\n    return _inner(dev)\n"
           "def new_entry(dev):\n    return _outer(dev), _WS_RATES.get(dev, 8)\n"
           "def no_workspace(dev):\n    return dev\n")
    import linecache
    linecache.cache["fake_ops.py"] = (len(src), None, src.splitlines(True), "fake_ops.py")
    exec(compile(src, "fake_ops.py", "exec"), fake.__dict__)
    fake.__file__ = "fake_ops.py"
    import sys
    sys.modules["fake_ops"] = fake
    try:
        assert W.workspace_call_sites(fake) == {("new_entry", "_WS"): 1, ("new_entry", "_WS_RATES"): 1}
    finally:
        del sys.modules["fake_ops"]
        linecache.cache.pop("fake_ops.py", None)


def test_the_gpu_file_builds_every_entry_and_variant():
    from tests import test_gpu_ws_state as GPU
    assert set(GPU.BUILDERS) == set(W.ENTRIES)
    listed = {(s["entry"], s["ws"], s["variant"]) for s in GPU.FILL_SPECS}
    want = {(f, w, v) for (f, w), vs in W.ENTRIES.items() for v in vs}
    assert want <= listed, "entries without a contents test: %s" % sorted(want - listed)
    short = {(s["entry"], s["ws"], s["variant"]) for s in GPU.SHORT_SPECS}
    assert want <= short, "entries without a too-small test: %s" % sorted(want - short)
    # every shape the GPU file runs is a shape the size queries below are asked about
    for s in GPU.all_specs():
        if s["kind"] == "rpn":
            assert (s["C"], s["T"], s["in_shapes"], s["N"], s["precision"]) in W.RPN_SHAPES, s
        elif s["kind"] in ("det", "roi"):
            assert (s["R"], s["C"], 128 if s["C"] != 128 else 256, 9, s["T"], s["precision"]) in W.DET_SHAPES, s
        elif s["kind"] == "nms":
            assert s["n"] in W.NMS_SIZES


# ---- 3. size queries -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from snn_automotive_object_detection_amd import _lib
    return _lib.load()


def _levels(shapes, N):
    from snn_automotive_object_detection_amd._lib import snn_rpn_level
    return (snn_rpn_level * len(shapes))(*[snn_rpn_level(None, N, h, w, 0) for h, w in shapes])


def _rpn_bytes(lib, C_, T, shapes, N, precision, route=None):
    from snn_automotive_object_detection_amd import _lib
    pr = _lib.PRECISIONS[precision]
    if route is None:
        return lib.snn_rpn_head_workspace_bytes(_levels(shapes, N), len(shapes), C_, 3, T, pr)
    return lib.snn_rpn_head_workspace_bytes_routed(_levels(shapes, N), len(shapes), C_, 3, T, pr, route)


@pytest.mark.parametrize("C_,T,shapes,N,precision", W.RPN_SHAPES, ids=lambda v: str(v).replace(" ", "") if not isinstance(v, tuple) else "x".join("%d_%d" % hw for hw in v))
def test_rpn_size_query(lib, C_, T, shapes, N, precision):
    need = _rpn_bytes(lib, C_, T, shapes, N, precision)
    assert need > 0 and need % 256 == 0
    for route in (0, 1, 2):
        assert _rpn_bytes(lib, C_, T, shapes, N, precision, route) >= need
    assert _rpn_bytes(lib, C_, T, shapes, N, precision, 3) == 0
    assert _rpn_bytes(lib, C_, T + 1, shapes, N, precision) >= need
    assert _rpn_bytes(lib, C_, T, shapes, N + 1, precision) >= need
    for l in range(len(shapes)):
        for dh, dw in ((1, 0), (0, 1)):
            grown = tuple((h + dh, w + dw) if i == l else (h, w) for i, (h, w) in enumerate(shapes))
            assert _rpn_bytes(lib, C_, T, grown, N, precision) >= need
    assert _rpn_bytes(lib, C_, T, shapes + ((1, 1),), N, precision) >= need
    # the steps of the T sequences on this shape never ask for more than the largest T
    assert all(_rpn_bytes(lib, C_, t, shapes, N, precision) <= _rpn_bytes(lib, C_, 16, shapes, N, precision) for t in (4, 5, 8, 12, 16))


def _det_bytes(lib, R, C_, Hd, K, T, precision, route=None):
    from snn_automotive_object_detection_amd import _lib
    pr = _lib.PRECISIONS[precision]
    if route is None:
        return lib.snn_det_head_workspace_bytes(R, C_ * 49, Hd, K, 4 * K, T, pr)
    return lib.snn_det_head_workspace_bytes_routed(R, C_ * 49, Hd, K, 4 * K, T, pr, route)


@pytest.mark.parametrize("R,C_,Hd,K,T,precision", W.DET_SHAPES)
def test_det_size_query(lib, R, C_, Hd, K, T, precision):
    need = _det_bytes(lib, R, C_, Hd, K, T, precision)
    assert need > 0 and need % 256 == 0
    for route in (0, 1, 2):
        assert _det_bytes(lib, R, C_, Hd, K, T, precision, route) >= need
    assert _det_bytes(lib, R, C_, Hd, K, T, precision, -1) == 0
    assert _det_bytes(lib, R, C_, Hd, K, T + 1, precision) >= need
    assert _det_bytes(lib, R + 1, C_, Hd, K, T, precision) >= need
    assert _det_bytes(lib, R, C_ + 32, Hd, K, T, precision) >= need
    assert _det_bytes(lib, R, C_, Hd + 32, K, T, precision) >= need
    assert all(_det_bytes(lib, R, C_, Hd, K, t, precision) <= _det_bytes(lib, R, C_, Hd, K, 24, precision) for t in (6, 12, 16, 24))


def test_post_processing_and_rates_size_queries(lib):
    from tests import _post_grid as PG
    for n in W.NMS_SIZES:
        need = lib.snn_nms_workspace_bytes(n)
        assert need == n * ((n + 63) // 64) * 8 and lib.snn_nms_workspace_bytes(n + 1) >= need     # the whole bit matrix: n rows of ceil(n / 64) words
    for N in (1, 2, 3):
        for K in (1, 63, 64, 65, 300, 1000):
            need = lib.snn_rpn_proposals_workspace_bytes(N, K)
            assert need > 0 and need % 256 == 0
            assert lib.snn_rpn_proposals_workspace_bytes(N + 1, K) >= need and lib.snn_rpn_proposals_workspace_bytes(N, K + 1) >= need
    assert lib.snn_rpn_proposals_workspace_bytes(0, 10) == 0 and lib.snn_rpn_proposals_workspace_bytes(2, 0) == 0
    spec = PG.DET_SPECS[W.DET_POST_SPEC]
    N, rmax, K = len(spec["rois"]), max(spec["rois"]), spec["K"]
    need = lib.snn_det_postprocess_workspace_bytes(N, rmax, K)
    assert need > 0 and need % 256 == 0
    assert lib.snn_det_postprocess_workspace_bytes(N + 1, rmax, K) >= need and lib.snn_det_postprocess_workspace_bytes(N, rmax + 1, K) >= need
    assert lib.snn_det_postprocess_workspace_bytes(N, rmax, K + 1) >= need and lib.snn_det_postprocess_workspace_bytes(N, 0, K) == 0
    for levels, max_n in ((1, 2), (2, 2), (3, 2)):
        need = lib.snn_rpn_rates_workspace_bytes(levels, max_n)
        assert need > 0 and lib.snn_rpn_rates_workspace_bytes(levels + 1, max_n) >= need and lib.snn_rpn_rates_workspace_bytes(levels, max_n + 1) >= need
    assert lib.snn_rpn_rates_workspace_bytes(0, 2) == 0


def test_rpn_proposals_holds_the_caller_to_its_size_query(lib):
    """the query bounds every level split (it is not told the levels), so the layout of one call may need less: a buffer below the QUERY is refused
    all the same, before any device work (fake device pointers: nothing may be dereferenced or enqueued)"""
    from snn_automotive_object_detection_amd import _lib
    fake = 0x1000
    lv = (_lib.snn_rpn_post_level * 3)()
    for l, (h, w) in enumerate(((8, 8), (4, 4), (2, 2))):
        lv[l].logits, lv[l].deltas, lv[l].H, lv[l].W, lv[l].stride_h, lv[l].stride_w = fake, fake, h, w, 4.0 * 2 ** l, 4.0 * 2 ** l
    N, A, pre = 2, 3, 100
    K = lib.snn_rpn_proposals_candidates(lv, 3, A, pre)
    assert K == 100 + 48 + 12
    need = lib.snn_rpn_proposals_workspace_bytes(N, K)
    hw = (C.c_float * 4)(64.0, 64.0, 64.0, 64.0)
    rc = lib.snn_rpn_proposals(lv, 3, N, A, hw, pre, 50, 0.7, 0.0, 1e-3, fake, fake, fake, None, None, fake, need - 1, None)
    assert rc == -2 and b"workspace too small" in lib.snn_last_error()
