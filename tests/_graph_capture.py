"""Graph capture of the stream-only entries: one protocol for every test, and the classification it rests on (test infrastructure).

include/snn_hip.h promises that a call enqueues its work on the caller's stream and nothing else, so it can be captured into a hipGraph and
replayed on new data.  A replayed graph can be wrong where an eager call cannot: every replay skips the call's HOST half.  So a decision the host
made from data is baked in, a counter cleared by something that is not a node of the graph accumulates, a result may depend on what the replay
before left behind, and a buffer the graph holds may be gone.  The protocol (run_protocol) is built to show each of those:

  case.prepare()    the static device operands
  case.load(i)      input set i into those operands (copy_; nothing is reallocated)
  case.call()       ONE call of the entry on the static operands -> a snapshot SOURCE: a callable that reads back, when asked, everything a caller
                    can observe from that call (tests/_ws_state.snapshot)
  case.eager(i)     the same call outside any graph on input set i -> snapshot (default: load(i), call()())
  case.oracle()     optional: asserts on what eager(0) read back (the zero-flip comparison with the oracle, tests/_entry_cases.py)
  case.after_replay(k, i)  optional: further asserts after replay k on input set i (route_stat against its documented value)

  1. warm-up        load(0), call() once eagerly: packed-weight, anchor and ratio caches fill here (a cache filled during a capture would record its
                    event inside the graph; the cold case is not tested)
  2. eager twins    eager(i) for every input set, inside poisoned_outputs(), the pinned workspaces armed with 0x00; oracle() after eager(0).  Two input
                    sets with equal snapshots prove nothing: CaseProvesNothing
  3. capture        call() under the strategy's capture, inside poisoned_outputs(): the NaN / 0x5a fills of the outputs become nodes of the graph, so
                    every replay starts from poisoned outputs
  4. replays        input sets 0, 1, .., 0, 1, .. (at least four, every set at least twice); before each one the workspaces are re-armed with the next of
                    REPLAY_FILLS, after it guards and tail are checked; the snapshot is bit-equal to eager(i), and to the earlier replay of the set.

The capture mechanism is a STRATEGY (capture(call, outputs) -> (replay, source)), so that tests/test_graph_capture_cpu.py can prove on fake graphs
over CPU tensors that the protocol flags each defect.  HipGraph is the real one.  Rules it keeps, for the sake of shared machines: one stream (no
other stream is made current inside a capture, so the graph has no parallel branches); every tensor the graph references stays alive as long
as the graph (the case object holds operands and results, the Capture holds the case); a synchronising entry (SYNCHRONISING below) raises a
Python error BEFORE it reaches the runtime when it is called inside a capture; a Python exception during a capture ends the capture, waits
for the device and is raised again - nothing is retried."""
import contextlib
import re
from typing import Callable, Dict, List, Sequence, Set, Tuple

import torch

from tests import _ws_state as W

REPLAY_FILLS = (0xff, 0x5a, 0x00, 0xff)


class CaseProvesNothing(AssertionError):
    """two input sets of a case give equal snapshots"""


# ---- the classification: every public function of ops.py that reaches a library call taking _stream() ---------------------------------------
CAPTURABLE: Dict[str, str] = {
    # name: where tests/test_gpu_graph_capture.py replays it
    "rpn_head_forward": "(a) heads, (b) routes, (c) typed, (f) static",
    "rpn_head_forward_readouts": "(a) heads",
    "det_head_forward": "(a) heads, (b) routes, (c) typed",
    "det_head_forward_readouts": "(a) heads",
    "det_head_forward_roialign": "(a) heads, (c) typed, (f) static",
    "det_head_forward_roialign_readouts": "(a) heads",
    "nms_keep_mask": "(e) post-processing",
    "rpn_proposals": "(e) post-processing, (f) static; its anchors come from the host copy _anchors_host cached at warm-up",
    "det_postprocess": "(e) post-processing",
    "det_postprocess_padded": "(e) post-processing, (f) static",
    "roi_assign": "(d) stages, (f) static",
    "encode_nchw": "(d) stages", "encode_rows": "(d) stages",
    "conv3x3_lif_bf16x3": "(d) stages", "spike_conv3x3_bf16x3": "(d) stages", "spike_gemm_lif_bf16x3": "(d) stages", "spike_gemm_bf16x3": "(d) stages",
    "conv3x3_lif_mx": "(d) stages", "spike_conv3x3_mx": "(d) stages", "spike_gemm_lif_mx": "(d) stages", "spike_gemm_mx": "(d) stages",
    "conv3x3_lif": "(d) stages", "spike_gemm": "(d) stages", "lif_scan": "(d) stages", "li_heads": "(d) stages", "li_heads_readouts": "(d) stages",
    "roi_align_encode": "(d) stages", "det_exchange_payload": "(d) stages", "det_rates": "(d) stages", "affine_act_nchw": "(d) stages",
    # weight packers without a verdict: one launch on the stream.  Weights are packed when they change, before any capture (warm caches)
    "pack_conv3x3": "(d) stages", "pack_linear": "(d) stages", "pack_linear_mx": "(d) stages", "pack_conv3x3_mx": "(d) stages",
}
SYNCHRONISING: Dict[str, str] = {
    # name: why it cannot sit in a capture (read from the code, never tried)
    "batched_nms": "n_keep.item(): the number of kept boxes comes to the host to size the result",
    "bf16x3_split_status": "status.tolist(): the verdict of snn_check_bf16x3_split comes to the host",
    "check_bf16x3_split": "raises from bf16x3_split_status's verdict",
    "split_problem": "check_bf16x3_split per weight",
    "pack_heads": "check_split (default on): check_bf16x3_split of both weights",
    "pack_conv3x3_bf16x3": "check_split (default on): check_bf16x3_split",
    "pack_linear_bf16x3": "check_split (default on): check_bf16x3_split",
    "pack_heads_bf16": "counts non-finite rounded weights on the host (int(...sum()))",
    "pack_conv3x3_bf16": "snn_pack_conv3x3_weight_bf16 -> pack_bf16_launch: hipMalloc, copy of the verdict to the host, hipStreamSynchronize, hipFree",
    "pack_linear_bf16": "snn_pack_linear_weight_bf16(_perm) -> pack_bf16_launch",
}
# private helpers that read the host only on a cache miss: capturable once warm (the protocol's warm-up), synchronising on first sight
WARM_ONLY: Dict[str, str] = {"_anchors_host": "base.detach().cpu() on its first sight of an anchor tensor; cached per tensor and version after that"}
# the only function bodies of csrc/ that may wait for the stream, allocate, free or copy to / from the host, and the exported entries that reach them
LIBRARY_SYNCHRONISING: Dict[str, Tuple[str, ...]] = {
    "pack_bf16_launch": ("snn_pack_conv3x3_weight_bf16", "snn_pack_linear_weight_bf16", "snn_pack_linear_weight_bf16_perm"),
}
HOST_READ = re.compile(r"\.item\(\)|\.tolist\(\)|\.cpu\(\)|\.numpy\(\)|\bint\(\([^\n]*\.sum\(\)\)|torch\.cuda\.synchronize|\.synchronize\(\)")
LIBRARY_FORBIDDEN = re.compile(r"\b(hipStreamSynchronize|hipDeviceSynchronize|hipEventSynchronize|hipStreamWaitEvent|hipEventRecord|hipMalloc\w*|hipHostMalloc|"
                               r"hipFree\w*|hipHostFree|hipMemcpy(?!Async)\w*|hipMemcpyAsync)\s*\(")


def _calls(funcs: Dict[str, str]) -> Dict[str, Set[str]]:
    return {name: {g for g in funcs if g != name and re.search(r"\b%s\(" % re.escape(g), body)} for name, body in funcs.items()}


def _reaching(funcs: Dict[str, str], direct: Set[str], skip: Sequence[str] = ()) -> Set[str]:
    """the functions that are in `direct` or call, through any number of functions of the module (those in `skip` excepted), one that is"""
    calls = _calls(funcs)
    out = set(direct)
    grew = True
    while grew:
        grew = False
        for name, cs in calls.items():
            if name not in out and name not in skip and any(c in out and c not in skip for c in cs):
                out.add(name)
                grew = True
    return out


def stream_functions(module) -> Set[str]:
    """the public top-level functions of `module` that reach a `lib.snn_*(... _stream())` call"""
    funcs = W._functions(module)
    direct = {n for n, body in funcs.items() if re.search(r"\blib\.snn_\w+\(", body) and "_stream()" in body}
    return {n for n in _reaching(funcs, direct) if not n.startswith("_")}


def host_reading_functions(module, library_entries: Sequence[str] = ()) -> Set[str]:
    """the public stream functions that reach a host read (HOST_READ in a function's own text, WARM_ONLY helpers excepted) or a call of one of
    `library_entries`"""
    funcs = W._functions(module)
    lib_re = re.compile(r"\blib\.(%s)\(" % "|".join(map(re.escape, library_entries))) if library_entries else None
    direct = {n for n, body in funcs.items() if n not in WARM_ONLY and (HOST_READ.search(body) or (lib_re is not None and lib_re.search(body)))}
    return _reaching(funcs, direct, skip=tuple(WARM_ONLY)) & stream_functions(module)


def library_offenders(sources: Dict[str, str]) -> Dict[str, Set[str]]:
    """{enclosing function: the forbidden calls in its body} over C / HIP sources {file name: text}.  The enclosing function is the nearest line
    above that starts in column 0 with a declaration and an opening parenthesis (the style of csrc/).  A hipMemcpyAsync counts unless its
    statement names hipMemcpyDeviceToDevice"""
    out: Dict[str, Set[str]] = {}
    for fname, text in sources.items():
        text = re.sub(r"//[^\n]*", "", text)
        for m in LIBRARY_FORBIDDEN.finditer(text):
            if m.group(1) == "hipMemcpyAsync" and "hipMemcpyDeviceToDevice" in text[m.start():text.find(";", m.start())]:
                continue
            head = None
            for line in reversed(text[:m.start()].split("\n")[:-1]):
                if line and re.match(r"[A-Za-z_]", line) and "(" in line and not line.startswith(("return", "if", "for", "while", "else", "case")):
                    head = line
                    break
            name = re.search(r"(\w+)\s*\(", head).group(1) if head else "%s:?" % fname
            out.setdefault(name, set()).add(m.group(1))
    return out


@contextlib.contextmanager
def synchronising_entries_raise(ops):
    """inside this block (a capture) a call of a SYNCHRONISING function of ops raises before anything reaches the runtime"""
    saved = {}

    def refuser(name):
        def refuse(*a, **k):
            raise AssertionError("%s is a synchronising entry (%s): it must not be called while a stream is capturing" % (name, SYNCHRONISING[name]))
        return refuse
    for name in SYNCHRONISING:
        if hasattr(ops, name):
            saved[name] = getattr(ops, name)
            setattr(ops, name, refuser(name))
    try:
        yield
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)


# ---- strategies -------------------------------------------------------------------------------------------------------------------------
class HipGraph:
    """the real thing: torch.cuda.graph on its one capture stream"""

    def __init__(self):
        self.graph = None

    def capture(self, call: Callable, outputs: list):
        from snn_automotive_object_detection_amd import ops
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        failure = None
        with synchronising_entries_raise(ops):
            try:
                with torch.cuda.graph(self.graph):
                    stream = torch.cuda.current_stream()
                    try:
                        source = call()
                        assert torch.cuda.current_stream() == stream, "the call left another stream current inside the capture"
                    except BaseException as e:               # leave the capture first (the context ends it), then wait, then raise: no retry
                        failure = e
            except BaseException as e:
                failure = failure or e
        if failure is not None:
            self.graph = None
            torch.cuda.synchronize()
            raise failure

        def replay():
            self.graph.replay()
            torch.cuda.synchronize()
        return replay, source

    def release(self):
        self.graph = None


# ---- the protocol -----------------------------------------------------------------------------------------------------------------------
class Case:
    """what run_protocol needs; subclasses hold every tensor they make (operands, results, route_stat, counts) on themselves"""
    n_sets = 2
    entries: Tuple[str, ...] = ()             # the ops functions call() reaches (checked against SYNCHRONISING before anything is captured)

    def prepare(self) -> None:
        raise NotImplementedError

    def load(self, i: int) -> None:
        raise NotImplementedError

    def call(self) -> Callable:
        raise NotImplementedError

    def eager(self, i: int):
        self.load(i)
        return self.call()()

    def oracle(self) -> None:
        pass

    def after_replay(self, k: int, i: int) -> None:
        pass


class Capture:
    """a captured case: keeps the case (and with it every tensor the graph references), the strategy and the eager twins"""

    def __init__(self, case, strategy, buffers, eager, replay, source, outputs):
        self.case, self.strategy, self.buffers, self.eager, self._replay, self.source, self.outputs = case, strategy, list(buffers), eager, replay, source, outputs
        self.seen: Dict[int, tuple] = {}
        self.n_replays = 0

    def replay(self, i: int, fill: int = 0x00):
        """input set i, workspaces re-armed with `fill`, one replay -> its snapshot, checked against the eager twin and the earlier replays of set i"""
        self.case.load(i)
        for b in self.buffers:
            b.rearm(fill)
        self._replay()
        for b in self.buffers:
            b.check()
        snap = self.source()
        k, self.n_replays = self.n_replays, self.n_replays + 1
        assert W.same_bits(snap, self.eager[i]), "replay %d (input set %d, workspace fill 0x%02x) differs from the eager call on that set: %s" % (
            k, i, fill, W.first_difference(snap, self.eager[i]))
        if i in self.seen:
            assert W.same_bits(snap, self.seen[i]), "replay %d differs from the earlier replay of input set %d: %s" % (k, i, W.first_difference(snap, self.seen[i]))
        self.seen.setdefault(i, snap)
        self.case.after_replay(k, i)
        return snap


def capture_case(case, strategy, buffers=()) -> Capture:
    """steps 1 - 3 of the protocol -> Capture"""
    bad = [e for e in case.entries if e in SYNCHRONISING]
    assert not bad, "a synchronising entry is never run inside a capture: %s" % bad
    case.prepare()
    case.load(0)
    case.call()()                                                # warm-up: caches fill here
    eager = []
    for i in range(case.n_sets):
        for b in buffers:
            b.arm(0x00)
        with W.poisoned_outputs():
            eager.append(case.eager(i))
        for b in buffers:
            b.check()
        if i == 0:
            case.oracle()
    for i in range(case.n_sets):
        for j in range(i):
            if W.same_bits(eager[i], eager[j]):
                raise CaseProvesNothing("input sets %d and %d give equal snapshots: replaying one for the other would go unnoticed" % (j, i))
    for b in buffers:
        b.arm(0x00)
    outputs: list = []
    with W.poisoned_outputs(outputs):
        replay, source = strategy.capture(case.call, outputs)
    return Capture(case, strategy, buffers, eager, replay, source, outputs)


def run_protocol(case, strategy, buffers=(), rounds: int = 2) -> Capture:
    """the whole protocol: every input set `rounds` (>= 2) times in the order 0, 1, .., 0, 1, .., at least four replays"""
    cap = capture_case(case, strategy, buffers)
    order = list(range(case.n_sets)) * max(rounds, 2)
    assert len(order) >= 4
    for k, i in enumerate(order):
        cap.replay(i, REPLAY_FILLS[k % len(REPLAY_FILLS)])
    return cap


# ---- cases over tests/_entry_cases.py -------------------------------------------------------------------------------------------------------
class EntryCase(Case):
    """a spec of tests/_entry_cases.py with the names of its input sets.  `oracle_sets`: the sets the builders have an oracle for (default: all
    of them; the derived sets of the post-processing cases have none).  For those the zero-flip comparison with the oracle - hidden planes,
    counts, outputs and route_stat against its documented value for THAT input - runs on the eager snapshot of set 0 and again after every replay"""

    def __init__(self, s: dict, dev, inputs: Sequence[str], oracle_sets=None):
        self.s, self.dev, self.inputs = s, dev, tuple(inputs)
        self.oracle_sets = set(self.inputs if oracle_sets is None else oracle_sets)
        self.n_sets = len(self.inputs)
        self.entries = (s["entry"],)
        self.ctx = self.last = None
        self.results: List[dict] = []                            # every call's tensors stay alive with the case

    def prepare(self):
        from tests import _entry_cases as E
        self.ctx = E.prepare(self.s, self.dev, self.inputs)

    def load(self, i):
        from tests import _entry_cases as E
        E.load(self.ctx, self.inputs[i])

    def call(self):
        from tests import _entry_cases as E
        res = E.call_entry(self.s, self.ctx)
        self.results.append(res)
        self.last = res
        return res["source"]

    def oracle(self):
        if self.inputs[0] in self.oracle_sets:
            self.last["oracle"](self.inputs[0])

    def after_replay(self, k, i):
        if self.inputs[i] in self.oracle_sets:                   # (self.last is the captured call: no eager call follows the capture)
            self.last["oracle"](self.inputs[i])


class FnCase(Case):
    """a call given as a function of static operands: sets[i] is a tuple of host tensors, fn(*operands) -> the tensors a caller observes"""

    def __init__(self, entries, dev, sets, fn, to_device=None):
        self.entries, self.dev, self.sets, self.fn = tuple(entries), dev, [tuple(s) for s in sets], fn
        self.n_sets = len(self.sets)
        self.to_device = to_device or (lambda t: t.to(dev))
        self.operands = None
        self.results = []

    def prepare(self):
        self.operands = [self.to_device(t) for t in self.sets[0]]

    def load(self, i):
        for dst, src in zip(self.operands, self.sets[i]):
            dst.copy_(src)

    def call(self):
        out = self.fn(*self.operands)
        self.results.append(out)
        return lambda: W.snapshot(out)
