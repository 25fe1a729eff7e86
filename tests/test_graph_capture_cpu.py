"""The graph-capture protocol of tests/_graph_capture.py proves itself on the host, and the classification it rests on is pinned to the code (CPU).

  1. fake graphs over CPU tensors run through the protocol: one whose replay returns the capture-time result whatever the operands hold, one
     whose replay adds to the previous outputs, a call whose result depends on the workspace fill, one whose replay leaves a row unwritten that
     the eager call writes - the protocol flags each, by the check that is meant to - an honest one passes, and a case whose two input sets give
     equal snapshots is refused;
  2. every public function of ops.py that reaches a library call taking _stream() is in CAPTURABLE or in SYNCHRONISING, never both; the ones that
     reach a host read are exactly SYNCHRONISING; ops._Workspace keeps every buffer it handed out while its stream was capturing;
  3. the only function body of csrc/ that waits for the stream, allocates, frees or copies to / from the host is pack_bf16_launch, reached from
     the bf16 packers alone."""
import glob
import os
import types

import pytest
import torch

from tests import _graph_capture as GC
from tests import _ws_state as W

CPU = torch.device("cpu")


# ---- 1. the protocol on fake graphs -----------------------------------------------------------------------------------------------------
class FakeGraph:
    """a tape of (compute, out) pairs the case's "kernels" append while the capture runs; a replay poisons the outputs allocated during the
    capture again (in a real graph those fills are nodes) and runs the tape on the same tensors.  `kind` is the defect of the REPLAY"""

    def __init__(self, kind="honest"):
        self.kind, self.tape = kind, []

    def capture(self, call, outputs):
        FakeCase.tape = self.tape
        try:
            source = call()
        finally:
            FakeCase.tape = None
        baked = [t.clone() for t in outputs]

        def replay():
            if self.kind == "baked":                          # the graph holds the answer of the capture, not the computation
                for t, b in zip(outputs, baked):
                    t.copy_(b)
                return
            if self.kind != "accumulating":
                for t in outputs:
                    t.fill_(float("nan"))
            for compute, out in self.tape:
                v = compute()
                if self.kind == "accumulating":               # a buffer nobody clears inside the graph
                    out.add_(v)
                elif self.kind == "unwritten_row":
                    out[:-1].copy_(v[:-1])
                else:
                    out.copy_(v)
        return replay, source


class FakeCase(GC.Case):
    """y = 2 x + 1 through n floats of scratch, the way ops reaches the library: _WS.get, the call, outputs from torch.empty"""
    tape = None

    def __init__(self, kernel="good", same_sets=False):
        self.kernel = kernel
        self.ws = W.GuardedWorkspace(CPU, 1 << 12)
        self.sets = [torch.arange(12, dtype=torch.float32), torch.arange(12, dtype=torch.float32) * (1.0 if same_sets else 3.0)]

    def prepare(self):
        self.x = self.sets[0].clone()

    def load(self, i):
        self.x.copy_(self.sets[i])

    def call(self):
        ws = self.ws.get(CPU, self.x.numel() * 4).view(torch.float32)
        out = torch.empty(self.x.numel())
        self.out = out

        def compute():
            if self.kernel == "reads_scratch":                # adds whatever the scratch held before it writes it
                stale = ws.clone()
                stale = torch.where(torch.isfinite(stale), stale, torch.ones_like(stale))
                ws.copy_(2 * self.x)
                return ws + 1 + (stale != 0).float()
            ws.copy_(2 * self.x)
            return ws + 1
        if FakeCase.tape is not None:
            FakeCase.tape.append((compute, out))
        out.copy_(compute())
        return lambda: W.snapshot(out)


def test_an_honest_graph_passes_and_is_replayed_four_times_over_two_sets():
    case = FakeCase()
    cap = GC.run_protocol(case, FakeGraph(), [case.ws])
    assert cap.n_replays == 4 and sorted(cap.seen) == [0, 1]
    assert torch.equal(case.out, 2 * case.sets[1] + 1)
    assert case.ws.fill == 0xff and case.ws.sizes == [48]         # (the last replay ran on the last of REPLAY_FILLS, the region stayed the capture's)


def test_a_baked_result_is_flagged_at_the_first_replay_of_the_other_set():
    case = FakeCase()                                             # (the capture runs on the set the last eager twin left loaded: set 1)
    with pytest.raises(AssertionError, match=r"replay 0 \(input set 0, workspace fill 0xff\) differs from the eager call"):
        GC.run_protocol(case, FakeGraph("baked"), [case.ws])


def test_an_accumulating_output_is_flagged():
    case = FakeCase()
    with pytest.raises(AssertionError, match=r"replay 0 .* differs from the eager call on that set: part 1: "):
        GC.run_protocol(case, FakeGraph("accumulating"), [case.ws])


def test_stale_scratch_is_flagged_by_the_fills():
    case = FakeCase("reads_scratch")
    with pytest.raises(AssertionError, match=r"replay 0 \(input set 0, workspace fill 0xff\) differs from the eager call"):
        GC.run_protocol(case, FakeGraph(), [case.ws])
    # (armed with zeros every time, as the eager tests of the suite mostly run, the same case passes)
    again = FakeCase("reads_scratch")
    cap = GC.capture_case(again, FakeGraph(), [again.ws])
    for i in (0, 1, 0, 1):
        cap.replay(i, 0x00)


def test_a_row_left_poisoned_by_the_replay_is_flagged():
    case = FakeCase()
    with pytest.raises(AssertionError, match=r"replay 0 .* differs from the eager call on that set: part 1: \d of 48 bytes differ, the first at byte 4[4-7]"):
        GC.run_protocol(case, FakeGraph("unwritten_row"), [case.ws])


def test_a_case_whose_input_sets_give_equal_results_is_refused():
    case = FakeCase(same_sets=True)
    with pytest.raises(GC.CaseProvesNothing, match="input sets 0 and 1 give equal snapshots"):
        GC.run_protocol(case, FakeGraph(), [case.ws])


def test_a_write_past_the_region_during_a_replay_is_flagged_by_the_tail():
    case = FakeCase()
    cap = GC.capture_case(case, FakeGraph(), [case.ws])
    cap.replay(0, 0xff)
    tape = cap.strategy.tape
    tape.append((lambda: torch.zeros(()), case.ws.interior[48 + 5:48 + 6]))
    with pytest.raises(AssertionError, match=r"interior written at region end \+ 5:"):
        cap.replay(1, 0x5a)


def test_a_synchronising_entry_is_refused_before_anything_is_captured_or_called():
    case = FakeCase()
    case.entries = ("rpn_head_forward", "batched_nms")
    with pytest.raises(AssertionError, match=r"never run inside a capture: \['batched_nms'\]"):
        GC.capture_case(case, FakeGraph(), [case.ws])
    fake_ops = types.SimpleNamespace(batched_nms=lambda *a: "ran", nms_keep_mask=lambda *a: "ran")
    with GC.synchronising_entries_raise(fake_ops):
        assert fake_ops.nms_keep_mask() == "ran"
        with pytest.raises(AssertionError, match="batched_nms is a synchronising entry"):
            fake_ops.batched_nms()
    assert fake_ops.batched_nms() == "ran"


# ---- 2. the classification, pinned to ops.py ---------------------------------------------------------------------------------------------
def test_every_stream_taking_function_of_ops_is_classified_once():
    from snn_automotive_object_detection_amd import ops
    taking = GC.stream_functions(ops)
    assert len(taking) >= 40 and {"rpn_head_forward", "roi_assign", "pack_heads_bf16", "split_problem"} <= taking
    assert not set(GC.CAPTURABLE) & set(GC.SYNCHRONISING)
    listed = set(GC.CAPTURABLE) | set(GC.SYNCHRONISING)
    assert taking == listed, "ops.py and the classification disagree: %s" % sorted(taking ^ listed)
    assert all(v.strip() for v in list(GC.CAPTURABLE.values()) + list(GC.SYNCHRONISING.values()))


def test_the_synchronising_list_is_what_reaches_a_host_read():
    """read from the code: .item() / .tolist() / .cpu() / int(sum) in a function's own text, or a call of a library entry that reaches
    pack_bf16_launch, followed through every caller; _anchors_host reads the host on a cache miss only (WARM_ONLY)"""
    from snn_automotive_object_detection_amd import ops
    entries = [e for es in GC.LIBRARY_SYNCHRONISING.values() for e in es]
    assert GC.host_reading_functions(ops, entries) == set(GC.SYNCHRONISING)
    funcs = W._functions(ops)
    assert set(GC.WARM_ONLY) <= set(funcs) and all(GC.HOST_READ.search(funcs[f]) for f in GC.WARM_ONLY)
    assert "_ANCHORS_HOST.get(key)" in funcs["_anchors_host"] and "_anchors_host(" in funcs["rpn_proposals"]
    # without the exception rpn_proposals would count as synchronising: the rule sees the helper
    direct = {n for n, body in funcs.items() if GC.HOST_READ.search(body)}
    assert "rpn_proposals" in GC._reaching(funcs, direct)


def test_the_map_sees_a_new_stream_function_and_a_new_host_read():
    import linecache
    import sys
    fake = types.ModuleType("fake_stream_ops")
    src = ("def _stream():\n    return 0\n"
           "def _launch(lib, x):\n    return lib.snn_thing(x, _stream())\n"
           "def new_entry(lib, x):\n    return _launch(lib, x)\n"
           "def new_reader(lib, x):\n    return new_entry(lib, x).item()\n"
           "def host_only(x):\n    return x.tolist()\n")
    linecache.cache["fake_stream_ops.py"] = (len(src), None, src.splitlines(True), "fake_stream_ops.py")
    exec(compile(src, "fake_stream_ops.py", "exec"), fake.__dict__)
    fake.__file__ = "fake_stream_ops.py"
    sys.modules["fake_stream_ops"] = fake
    try:
        assert GC.stream_functions(fake) == {"new_entry", "new_reader"}
        assert GC.host_reading_functions(fake) == {"new_reader"}
    finally:
        del sys.modules["fake_stream_ops"]
        linecache.cache.pop("fake_stream_ops.py", None)


def test_the_gpu_file_replays_every_capturable_entry():
    from tests import test_gpu_graph_capture as GPU
    reached = GPU.entries_reached()
    assert set(GC.CAPTURABLE) <= reached, "capturable entries no graph test replays: %s" % sorted(set(GC.CAPTURABLE) - reached)
    assert not reached & set(GC.SYNCHRONISING)
    for name in GC.CAPTURABLE:
        assert name in GPU.__doc__, "%s is not in the table of tests/test_gpu_graph_capture.py" % name


def test_workspace_keeps_what_it_handed_out_while_capturing(monkeypatch):
    """ops._Workspace is grow-only: a larger request replaces the buffer of its (device, stream).  A graph captured in between still writes into
    the smaller one, so a buffer handed out while the stream was capturing is never dropped"""
    from snn_automotive_object_detection_amd import ops
    capturing = [False]
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=7))
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing[0])
    ws = ops._Workspace()
    a = ws.get(CPU, 100)
    assert ws.get(CPU, 50) is a and not ws.captured
    b = ws.get(CPU, 200)                                          # eager growth: the old buffer is dropped, as before
    assert b is not a and not ws.captured
    capturing[0] = True
    assert ws.get(CPU, 150) is b and ws.captured == [b]           # handed out to a graph
    assert ws.get(CPU, 10) is b and ws.captured == [b]            # (once)
    c = ws.get(CPU, 300)
    assert c is not b and [t.data_ptr() for t in ws.captured] == [b.data_ptr(), c.data_ptr()]
    capturing[0] = False
    d = ws.get(CPU, 400)                                          # a later, larger eager call on the same key
    assert d is not c and [t.data_ptr() for t in ws.captured] == [b.data_ptr(), c.data_ptr()]
    assert ws.captured[0].numel() == 200 and ws.captured[1].numel() == 300


# ---- 3. the library side ---------------------------------------------------------------------------------------------------------------
def _csrc():
    from snn_automotive_object_detection_amd import ops
    root = os.path.join(os.path.dirname(os.path.abspath(ops.__file__)), "csrc")
    files = sorted(glob.glob(os.path.join(root, "*")))
    assert len(files) >= 10
    return {os.path.basename(f): open(f).read() for f in files}


def test_only_the_bf16_packers_synchronise_in_the_library():
    src = _csrc()
    found = GC.library_offenders(src)
    assert set(found) == set(GC.LIBRARY_SYNCHRONISING), "function bodies of csrc/ that wait, allocate, free or copy to / from the host: %s" % {k: sorted(v) for k, v in found.items()}
    assert {"hipMalloc", "hipMemcpyAsync", "hipStreamSynchronize", "hipFree"} <= found["pack_bf16_launch"]
    # who reaches it: the exported entries named in LIBRARY_SYNCHRONISING and nobody else
    import re
    text = re.sub(r"//[^\n]*", "", src["snn_kernels.hip"])
    for helper, entries in GC.LIBRARY_SYNCHRONISING.items():
        callers = set()
        for m in re.finditer(r"\b%s\(" % helper, text):
            lines = text[:m.start()].split("\n")
            if re.match(r"[A-Za-z_]", lines[-1]):              # (the helper's own definition)
                continue
            head = [l for l in lines[:-1] if re.match(r"[A-Za-z_]", l) and "(" in l][-1]
            callers.add(re.search(r"(\w+)\s*\(", head).group(1))
        assert callers == set(entries), callers
    # and ops.py reaches those entries from the synchronising packers alone
    from snn_automotive_object_detection_amd import ops
    for name, body in W._functions(ops).items():
        if any(re.search(r"\blib\.%s\(" % e, body) for es in GC.LIBRARY_SYNCHRONISING.values() for e in es):
            assert name in GC.SYNCHRONISING, name


def test_the_library_check_sees_a_new_offender():
    fake = {"x.hip": "static int helper(int a) {\n    return a;\n}\n\nint snn_new_entry(void* p, snn_stream_t s) {\n    if (p) {\n"
                     "        hipMemcpyAsync(p, p, 4, hipMemcpyDeviceToDevice, s);\n        hipMemcpyAsync(&h, p, 4,\n            hipMemcpyDeviceToHost, s);\n"
                     "        // hipFree(p) in a comment does not count\n        hipStreamSynchronize(s);\n    }\n    return 0;\n}\n"}
    assert GC.library_offenders(fake) == {"snn_new_entry": {"hipMemcpyAsync", "hipStreamSynchronize"}}
