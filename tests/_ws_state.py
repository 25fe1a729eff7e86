"""The workspace seam: what a head or post-processing call may assume about the scratch buffer it is handed (test infrastructure).

The contract (include/snn_hip.h): the caller owns the workspace, sizes it with snn_*_workspace_bytes, hands it over
with whatever bytes the allocator left in it, and the library keeps no state between calls.  So a call
  * may write `nbytes` bytes behind the pointer it was given and not one more;
  * must return the same bits whatever the buffer held before - zeros, the planes of a larger and denser call, all ones;
  * must refuse a buffer one byte too small before it enqueues anything.
ops._WS and ops._WS_RATES (ops._Workspace.get(device, nbytes)) are the only places the Python layer obtains a workspace.  A
GuardedWorkspace has the same `get` and is installed in their place (monkeypatch.setattr(ops, "_WS", ...)): one uint8 tensor laid out
[1 MiB guard | interior | 1 MiB guard], the interior 4096-byte aligned; `get` hands out interior[:nbytes] - the library is told EXACTLY
the queried size - and never writes a byte itself.  `arm(fill)` fills the interior and writes GUARD_BYTE over both guards; `check()`
asserts that the guards still hold GUARD_BYTE and that the interior behind the largest region handed out since arm() still holds the fill
(written zeros cannot be told from the fill 0x00: the other two fills show an overhang of any value).

tests/test_ws_state_cpu.py proves on fake calls that the harness flags a read before a write, a write past the end and a flag left
behind, and pins ENTRIES to the call sites of ops.py; tests/test_gpu_ws_state.py runs every entry of ENTRIES.

The same contract for the OPERANDS of a call: `guarded` / `GuardedCall` / `run_input_guards` below put every input and output of one call into an
allocation of its own, [guard | payload | guard] to the byte.  tests/_train_entries.py runs the seven training entries that way, with
GuardedWorkspaces at readout._WS_WGRAD, hidden._WS_WGRAD and losses._WS_LOSS (tests/test_train_entries_cpu.py, tests/test_gpu_train_entries.py)."""
import ast
import contextlib
import inspect
import re
from typing import Dict, List, Optional, Tuple

import torch

GUARD = 1 << 20
GUARD_BYTE = 0xa5
ALIGN = 4096
# 0x00: what a fresh allocation usually holds; 0x5a: the precedent of tests/test_gpu_nhwc_features.py; 0xff: every spike of a plane word
# set, -1 in a counter, NaN in a float - the most sensitive fill for a halo row or a counter nobody wrote
FILLS = (0x00, 0x5a, 0xff)
OUT_POISON = 0x5a                      # the byte integer outputs are pre-filled with (floating ones: NaN)


class GuardedWorkspace:
    """drop-in for ops._Workspace: one buffer for every stream of one device (the tests run on one stream)"""

    def __init__(self, device, interior_bytes: int = 32 << 20):
        self.device = torch.device(device)
        raw = torch.empty(GUARD + int(interior_bytes) + GUARD + ALIGN, dtype=torch.uint8, device=self.device)
        lead = (-(raw.data_ptr() + GUARD)) % ALIGN               # the interior starts on a multiple of ALIGN
        self.front = raw[lead:lead + GUARD]
        self.interior = raw[lead + GUARD:lead + GUARD + int(interior_bytes)]
        self.back = raw[lead + GUARD + int(interior_bytes):lead + 2 * GUARD + int(interior_bytes)]
        assert self.interior.data_ptr() % ALIGN == 0
        self.fill: Optional[int] = None
        self.short_by = 0                 # > 0: hand out that many bytes LESS than asked for (the too-small-by-one-byte tests)
        self.size = 0                     # bytes handed out by the last sizing `get`
        self.view: Optional[torch.Tensor] = None
        self.sizes: List[int] = []        # every size asked for since the last arm()
        self.high = 0                     # the largest region handed out since the last arm()

    def get(self, device, nbytes: int) -> torch.Tensor:
        nbytes = int(nbytes)
        if self.view is not None and nbytes <= self.size + self.short_by:
            return self.view              # (the plane readers of tests/_planes.py ask for 1 byte: the view of the call before, untouched)
        if nbytes > self.interior.numel():
            raise AssertionError("GuardedWorkspace: %d bytes asked for, the interior holds %d" % (nbytes, self.interior.numel()))
        if torch.device(device).type != self.device.type:
            raise AssertionError("GuardedWorkspace on %s asked for a buffer on %s" % (self.device, device))
        self.size = nbytes - self.short_by
        self.sizes.append(nbytes)
        self.high = max(self.high, self.size)
        self.view = self.interior[:self.size]
        return self.view

    def forget(self) -> None:
        """the next `get` sizes its view anew whatever it asks for (between the steps of a sequence); no byte is touched"""
        self.size, self.view = 0, None

    def arm(self, fill: int) -> None:
        self.fill = int(fill)
        self.interior.fill_(self.fill)
        self.front.fill_(GUARD_BYTE)
        self.back.fill_(GUARD_BYTE)
        self.sizes, self.high = [], 0
        self.forget()

    def rearm(self, fill: int) -> None:
        """arm() for a region that is still in use: a captured graph holds the view handed out during its capture and no `get` runs when it is
        replayed, so the fill and the guards are renewed while the view, its size and the largest region so far stay as they are"""
        size, view, sizes, high = self.size, self.view, self.sizes, self.high
        self.arm(fill)
        self.size, self.view, self.sizes, self.high = size, view, sizes, high

    @staticmethod
    def _first_bad(t: torch.Tensor, byte: int) -> Optional[int]:
        bad = (t != byte).nonzero()
        return int(bad[0]) if bad.numel() else None

    def check(self) -> None:
        """both guards intact, and the interior behind the largest region handed out since arm() still armed (after one call: behind the
        region of that call).  Offsets in the message count from the END of that region (>= 0: written past the end)"""
        assert self.fill is not None, "check() before arm()"
        n = self.high
        b = self._first_bad(self.back, GUARD_BYTE)
        assert b is None, "back guard touched at region end + %d (region %d bytes)" % (self.interior.numel() - n + b, n)
        f = self._first_bad(self.front, GUARD_BYTE)
        assert f is None, "front guard touched at region end - %d (region %d bytes)" % (n + GUARD - f, n)
        t = self._first_bad(self.interior[n:], self.fill)
        assert t is None, "interior written at region end + %d: the %d bytes the size query names do not hold what the call writes" % (t, n)

    def untouched(self) -> bool:
        """nothing was written anywhere since arm()"""
        return (self._first_bad(self.interior, self.fill) is None and self._first_bad(self.front, GUARD_BYTE) is None
                and self._first_bad(self.back, GUARD_BYTE) is None)


def armed_call(buffers, fill: int, call):
    """arm every buffer with `fill`, run call() -> snapshot, check every buffer"""
    for b in buffers:
        b.arm(fill)
    snap = call()
    for b in buffers:
        b.check()
    return snap


def run_fills(buffers, call, fills=FILLS):
    """the call under every fill: guards and tail intact each time, the snapshots bit-equal; -> the snapshot"""
    snaps = [armed_call(buffers, f, call) for f in fills]
    for f, s in zip(fills[1:], snaps[1:]):
        assert same_bits(s, snaps[0]), "fill 0x%02x against 0x%02x: %s" % (f, fills[0], first_difference(s, snaps[0]))
    return snaps[0]


def run_sequence(buffers, calls, start_fill: int = 0x00):
    """every call alone on freshly armed zeros, then all of them in order on ONE buffer that is armed once: each step is told exactly its own
    size, must leave the guards and the bytes behind the largest region so far alone, and must return the bits it returned alone"""
    alone = [armed_call(buffers, 0x00, c) for c in calls]
    for b in buffers:
        b.arm(start_fill)
    for i, c in enumerate(calls):
        for b in buffers:
            b.forget()
        got = c()
        for b in buffers:
            b.check()
        assert same_bits(got, alone[i]), "step %d of the sequence differs from the same call alone: %s" % (i, first_difference(got, alone[i]))
    return alone


# ---- what a caller can observe --------------------------------------------------------------------------------------------------------
def _flatten(x, out):
    if x is None:
        out.append(torch.zeros(0, dtype=torch.uint8))
    elif isinstance(x, torch.Tensor):
        t = x.detach().contiguous().cpu()
        out.append(t.reshape(-1).view(torch.uint8) if t.numel() else torch.zeros(0, dtype=torch.uint8))
    elif isinstance(x, (list, tuple)):
        out.append(torch.tensor([len(x)], dtype=torch.int64).view(torch.uint8))
        for y in x:
            _flatten(y, out)
    elif isinstance(x, (bool, int)):
        out.append(torch.tensor([int(x)], dtype=torch.int64).view(torch.uint8))
    else:
        raise TypeError("snapshot: %r" % type(x))


def snapshot(*parts) -> Tuple[torch.Tensor, ...]:
    """everything a caller can observe from one call - outputs, time sums, spike counts, route_stat, the hidden planes read through the
    debug accessors - as host copies of the BYTES (a NaN a call left in place compares equal to itself)"""
    out: List[torch.Tensor] = []
    _flatten(list(parts), out)
    return tuple(out)


def same_bits(a, b) -> bool:
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, b))


def first_difference(a, b) -> str:
    if len(a) != len(b):
        return "%d parts against %d" % (len(a), len(b))
    for i, (x, y) in enumerate(zip(a, b)):
        if x.shape != y.shape:
            return "part %d: %s bytes against %s" % (i, tuple(x.shape), tuple(y.shape))
        d = (x.reshape(-1) != y.reshape(-1)).nonzero()
        if d.numel():
            return "part %d: %d of %d bytes differ, the first at byte %d" % (i, d.numel(), x.numel(), int(d[0]))
    return "equal"


@contextlib.contextmanager
def poisoned_outputs(record: Optional[list] = None):
    """ops allocates its outputs with torch.empty / torch.empty_like - the allocator's leftovers, often the right answer of the call before.
    Inside this block each of them comes back filled with NaN (floating) or OUT_POISON bytes (integers), so that a row a kernel does not
    write is the same in every run and an output nobody wrote is visible; `record` collects the tensors"""
    real = {"empty": torch.empty, "empty_like": torch.empty_like}

    def poisoning(fn):
        def alloc(*a, **k):
            t = fn(*a, **k)
            if t.numel():
                if t.is_floating_point():
                    t.fill_(float("nan"))
                else:
                    t.reshape(-1).view(torch.uint8).fill_(OUT_POISON)
            if record is not None:
                record.append(t)
            return t
        return alloc
    for name, fn in real.items():
        setattr(torch, name, poisoning(fn))
    try:
        yield record
    finally:
        for name, fn in real.items():
            setattr(torch, name, fn)


def still_poisoned(t: torch.Tensor) -> bool:
    if not t.numel():
        return True
    return bool(torch.isnan(t).all()) if t.is_floating_point() else bool((t.contiguous().reshape(-1).view(torch.uint8) == OUT_POISON).all())


# ---- guarded operands: the same contract for the inputs and outputs of a call (tests/_train_entries.py) ----------------------------------
OPERAND_GUARD = 64 << 10                # bytes of each guard around an operand: more than a work-group's stride at any shape the tests run
OPERAND_ALIGN = 256                     # the payload starts on a multiple of this: no entry sees a base pointer it would refuse


class Guarded:
    """one allocation laid out [front guard | payload | back guard]: the payload is a contiguous view of exactly `shape`, starts 256-byte
    aligned and touches both guards to the byte, so an element before the first or behind the last is a guard byte.  The wrappers take such
    a view as it is (a contiguous tensor is never copied).  An OUTPUT is poison()ed: payload NaN / OUT_POISON, guards GUARD_BYTE.  An INPUT
    is load()ed: payload = the source, guards a byte of the caller's choosing - 0x00 and 0xff (NaN as a float, every spike bit of a plane
    word set, label -1) give different results to a kernel that reads one element too far."""

    def __init__(self, shape, dtype, device):
        self.shape, self.dtype = tuple(int(x) for x in shape), dtype
        self.item = torch.empty((), dtype=dtype).element_size()
        n = self.item
        for x in self.shape:
            n *= x
        raw = torch.empty(2 * OPERAND_GUARD + n + OPERAND_ALIGN, dtype=torch.uint8, device=device)
        lead = (-(raw.data_ptr() + OPERAND_GUARD)) % OPERAND_ALIGN
        self.front = raw[lead:lead + OPERAND_GUARD]
        self.bytes = raw[lead + OPERAND_GUARD:lead + OPERAND_GUARD + n]
        self.back = raw[lead + OPERAND_GUARD + n:lead + 2 * OPERAND_GUARD + n]
        self.payload = self.bytes.view(dtype).view(self.shape)
        assert self.payload.is_contiguous() and (self.front.data_ptr() + OPERAND_GUARD) % OPERAND_ALIGN == 0
        assert self.front.data_ptr() + OPERAND_GUARD + n == self.back.data_ptr()
        assert not n or self.payload.data_ptr() == self.front.data_ptr() + OPERAND_GUARD       # (an empty tensor has no address)
        self.guard_byte: Optional[int] = None
        self.source: Optional[torch.Tensor] = None         # host bytes of what load() put into the payload

    def set_guards(self, byte: int) -> None:
        self.guard_byte = int(byte)
        self.front.fill_(self.guard_byte)
        self.back.fill_(self.guard_byte)

    def poison(self) -> "Guarded":
        if self.bytes.numel():
            if self.payload.is_floating_point():
                self.payload.fill_(float("nan"))
            else:
                self.bytes.fill_(OUT_POISON)
        self.set_guards(GUARD_BYTE)
        return self

    def load(self, src: torch.Tensor, guard_byte: int) -> "Guarded":
        src = src.detach().contiguous()
        assert tuple(src.shape) == self.shape and src.dtype == self.dtype, (tuple(src.shape), src.dtype, self.shape, self.dtype)
        self.payload.copy_(src)
        self.source = src.cpu().reshape(-1).view(torch.uint8).clone() if src.numel() else torch.zeros(0, dtype=torch.uint8)
        self.set_guards(guard_byte)
        return self

    def check_guards(self, what: str) -> None:
        assert self.guard_byte is not None, "check_guards() before poison() / load()"
        b = GuardedWorkspace._first_bad(self.back, self.guard_byte)
        assert b is None, "%s: back guard touched at payload end + %d (payload %s, %d bytes)" % (what, b, self.shape, self.bytes.numel())
        f = GuardedWorkspace._first_bad(self.front, self.guard_byte)
        assert f is None, "%s: front guard touched at payload start - %d (payload %s)" % (what, OPERAND_GUARD - f, self.shape)

    def check_unchanged(self, what: str) -> None:
        """an input still holds what load() put there"""
        now = self.bytes.cpu()
        d = (now != self.source).nonzero()
        assert not d.numel(), "%s: the call wrote into its input, first at byte %d of %d" % (what, int(d[0]), now.numel())

    def unwritten(self) -> int:
        """how many payload elements still hold the poison (NaN; every byte OUT_POISON)"""
        if not self.bytes.numel():
            return 0
        if self.payload.is_floating_point():
            return int(torch.isnan(self.payload).sum())
        return int((self.bytes.view(-1, self.item) == OUT_POISON).all(dim=1).sum())


def guarded(shape, dtype, device) -> Guarded:
    """[front guard | payload | back guard] for one operand; `.payload` is the tensor a call is given"""
    return Guarded(shape, dtype, device)


class GuardedCall:
    """the operands of ONE call, each in an allocation of its own.
    inputs  {name: host tensor | None}: loaded flush between guards of `in_guard` bytes;
    outputs {name: (shape, dtype) | host tensor | None}: a (shape, dtype) is poisoned and must come back wholly written; a host tensor is
            what the call adds to (accumulate = 1: every element counts as written before the call).
    verify() -> the snapshot of every output, after: no guard byte of any operand changed, no input changed, no output element left unwritten."""

    def __init__(self, device, inputs: dict, outputs: dict, in_guard: int = 0x00):
        self.g_in: Dict[str, Guarded] = {}
        self.g_out: Dict[str, Guarded] = {}
        self.prior = set()
        for k, v in inputs.items():
            if v is not None:
                self.g_in[k] = guarded(v.shape, v.dtype, device).load(v, in_guard)
        for k, v in outputs.items():
            if v is None:
                continue
            if isinstance(v, torch.Tensor):
                self.g_out[k] = guarded(v.shape, v.dtype, device).load(v, GUARD_BYTE)
                self.prior.add(k)
            else:
                self.g_out[k] = guarded(v[0], v[1], device).poison()
        self.ins = {k: (self.g_in[k].payload if k in self.g_in else None) for k in inputs}
        self.outs = {k: (self.g_out[k].payload if k in self.g_out else None) for k in outputs}

    def check_guards(self) -> None:
        for k, g in self.g_out.items():
            g.check_guards("output %s" % k)
        for k, g in self.g_in.items():
            g.check_guards("input %s" % k)
            g.check_unchanged("input %s" % k)

    def verify(self):
        self.check_guards()
        for k, g in self.g_out.items():
            if k not in self.prior:
                n = g.unwritten()
                assert n == 0, "output %s: %d of %d elements were never written" % (k, n, g.payload.numel())
        return snapshot(*[g.payload for g in self.g_out.values()])

    def outputs_untouched(self) -> bool:
        """after a refused call: every poisoned output is still poison, every prior still the prior"""
        for k, g in self.g_out.items():
            if k in self.prior:
                if not torch.equal(g.bytes.cpu(), g.source):
                    return False
            elif not still_poisoned(g.payload):
                return False
        return True


def run_input_guards(call):
    """call(in_guard) -> snapshot, under input guards of zeros and of 0xff bytes: what lies behind (or before) an input must not reach a
    result; -> the snapshot"""
    a, b = call(0x00), call(0xff)
    assert same_bits(a, b), "input guards 0xff against 0x00: %s" % first_difference(a, b)
    return a


# ---- the entries: every public ops function that takes a workspace, with the variants tests/test_gpu_ws_state.py runs ---------------------
HEAD_VARIANTS = ("plain", "rates", "sparse", "dense", "auto_never", "auto_always")        # auto at crossover 2 (never dense) and -1 (always)
ENTRIES: Dict[Tuple[str, str], Tuple[str, ...]] = {
    ("rpn_head_forward", "_WS"): HEAD_VARIANTS,
    ("rpn_head_forward", "_WS_RATES"): ("rates",),
    ("rpn_head_forward_readouts", "_WS"): ("plain", "rates"),
    ("rpn_head_forward_readouts", "_WS_RATES"): ("rates",),
    ("det_head_forward", "_WS"): HEAD_VARIANTS,
    ("det_head_forward_roialign", "_WS"): ("plain", "dense", "auto_never", "auto_always"),
    ("det_head_forward_readouts", "_WS"): ("plain", "rates"),
    ("det_head_forward_roialign_readouts", "_WS"): ("plain", "rates"),
    ("batched_nms", "_WS"): ("plain",),
    ("nms_keep_mask", "_WS"): ("plain",),
    ("rpn_proposals", "_WS"): ("plain",),
    ("det_postprocess", "_WS"): ("plain",),
    ("det_postprocess_padded", "_WS"): ("plain",),
}


def _functions(module) -> Dict[str, str]:
    """{name: source} of the top-level functions of a module"""
    src = inspect.getsource(module)
    return {n.name: ast.get_source_segment(src, n) for n in ast.parse(src).body if isinstance(n, ast.FunctionDef)}


def direct_sites(module) -> Dict[str, List[str]]:
    """{top-level function: the workspaces ("_WS" / "_WS_RATES") whose .get( it calls itself, one item per call site}"""
    return {name: re.findall(r"\b(_WS(?:_RATES)?)\.get\(", body) for name, body in _functions(module).items()}


def workspace_call_sites(module) -> Dict[Tuple[str, str], int]:
    """{(public function of `module`, "_WS" | "_WS_RATES"): number of .get( call sites it reaches}: the sites are found in the source
    of every top-level function; a site in a private helper (_det_ws, _rpn_rates) counts for every public function that calls the helper,
    through any number of private helpers"""
    funcs = _functions(module)
    direct = direct_sites(module)
    calls = {name: {g for g in funcs if g != name and re.search(r"\b%s\(" % re.escape(g), body)} for name, body in funcs.items()}

    def reach(name, seen):
        sites = list(direct[name])
        for g in calls[name]:
            if g.startswith("_") and g not in seen:
                sites += reach(g, seen | {g})
        return sites
    out: Dict[Tuple[str, str], int] = {}
    for name in funcs:
        if name.startswith("_"):
            continue
        for which in reach(name, {name}):
            out[(name, which)] = out.get((name, which), 0) + 1
    return out


# ---- the shapes of tests/test_gpu_ws_state.py (tests/test_ws_state_cpu.py asks the size queries about each of them) ------------------------
PYRAMID = ((13, 17), (6, 7), (2, 1))
SPLIT_PYRAMID = ((7, 9), (1, 3))           # C = 256: spike planes in blocks of four words behind the FAT conv
ONE_BY_ONE = ((1, 1),)
# (C, T, level shapes, N, precision)
RPN_SHAPES = tuple((C, T, PYRAMID, 2, "bf16x3") for C in (64, 128) for T in (5, 8, 16)) + (
    (256, 8, SPLIT_PYRAMID, 2, "bf16x3"), (64, 4, PYRAMID, 2, "bf16x3"), (64, 12, PYRAMID, 2, "bf16x3"), (64, 5, ONE_BY_ONE, 2, "bf16x3"),
    (64, 8, PYRAMID, 2, "f32"), (64, 8, PYRAMID, 2, "bf16"), (128, 8, PYRAMID, 2, "mxfp6"), (128, 8, PYRAMID, 2, "f32"), (128, 8, PYRAMID, 2, "bf16"),
    (128, 4, PYRAMID, 2, "bf16x3"))
# (R, C, Hd, K, T, precision): D = 49 C, K4 = 4 K
DET_SHAPES = tuple((29, 64, 128, 9, T, "bf16x3") for T in (6, 12, 16, 24)) + tuple((R, C, 128, 9, 12, "bf16x3") for R in (1, 17, 65) for C in (32, 64)) + (
    (65, 64, 128, 9, 24, "bf16x3"), (1, 64, 128, 9, 6, "bf16x3"), (38, 64, 128, 9, 12, "bf16x3"),
    (29, 64, 128, 9, 12, "f32"), (29, 64, 128, 9, 12, "bf16"), (37, 128, 256, 9, 12, "mxfp6"))
NMS_SIZES = (65, 129)
RPN_POST_SPEC = "r_t3_cut"
DET_POST_SPEC = "d_k5_small"
READOUT_STEPS = (4, 8, 12)
