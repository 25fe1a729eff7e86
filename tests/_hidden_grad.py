"""The SuperSpike LIF adjoint restated in torch (test infrastructure, host only): the oracle of tests/test_gpu_hidden_grad.py, tied to
torch.autograd through oracle.norse_restated.lif_feed_forward_step by tests/test_hidden_grad_cpu.py.

``adjoint`` is the recurrence of include/snn_hip.h (snn_lif_surrogate_bwd) operation for operation; evaluated in float64 it is the yardstick,
evaluated in float32 it is the "op-for-op fp32 CPU evaluation" the GPU's error is measured against (torch's CPU element-wise kernels do not
contract, and neither does the library's build)."""
from typing import NamedTuple, Optional

import numpy as np
import torch

from oracle import norse_restated as NR
from tests import _readout_grad as RG


class Consts(NamedTuple):
    a: float                 # dt_tau_mem
    b: float                 # neg_dt_tau_syn
    v_leak: float
    v_reset: float
    th: float                # v_th_lif


def f32(x: float) -> float:
    return float(np.float32(x))


REFERENCE = Consts(f32(float(torch.tensor(0.001) * torch.tensor(100.0))), f32(float(-torch.tensor(0.001) * torch.tensor(200.0))), 0.0, 0.0, f32(0.1))
OTHER = Consts(f32(0.07), f32(-0.15), f32(-0.05), f32(-0.2), f32(0.3))          # non-zero v_leak / v_reset, other time constants


class SuperSpike(torch.autograd.Function):
    """norse/torch/functional/superspike.py: heaviside forward, grad / (alpha |x| + 1)^2 backward"""

    @staticmethod
    def forward(ctx, x, alpha, forced=None):
        ctx.save_for_backward(x)
        ctx.alpha = alpha
        return torch.gt(x, 0).to(x.dtype) if forced is None else forced.to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        return g / (ctx.alpha * torch.abs(x) + 1.0).pow(2), None, None


def lif_forward_autograd(cur: torch.Tensor, c: Consts, alpha: float, forced: Optional[torch.Tensor] = None):
    """z [Tc + 1, ...] of a SuperSpike LIF layer through lif_feed_forward_step, differentiable with respect to cur [Tc, ...]; the step
    function is the oracle's, with its threshold swapped for one that carries the surrogate (the forward values are the same).  ``forced``
    [Tc + 1, ...]: teacher forcing - step t's threshold returns forced[t] whatever it compares (the surrogate still sees this run's x)"""
    dt = cur.dtype
    p = NR.LIFParameters(tau_syn_inv=torch.tensor(-c.b, dtype=dt), tau_mem_inv=torch.tensor(c.a, dtype=dt), v_leak=torch.tensor(c.v_leak, dtype=dt),
                         v_th=torch.tensor(c.th, dtype=dt), v_reset=torch.tensor(c.v_reset, dtype=dt), alpha=alpha)
    keep = NR.threshold
    step = [0]

    def surrogate(x, method, al):
        t, step[0] = step[0], step[0] + 1
        return SuperSpike.apply(x, al, None if forced is None else forced[t])
    NR.threshold = surrogate
    try:
        state = NR.LIFFeedForwardState(v=torch.full(cur.shape[1:], c.v_leak, dtype=dt), i=torch.zeros(cur.shape[1:], dtype=dt))
        zs = []
        for t in range(cur.shape[0] + 1):
            x = cur[t] if t < cur.shape[0] else torch.zeros(cur.shape[1:], dtype=dt)
            z, state = NR.lif_feed_forward_step(x, state, p, dt=1.0)            # (dt = 1: a and -b ARE the products dt * tau_inv)
            zs.append(z)
    finally:
        NR.threshold = keep
    return torch.stack(zs)


def lif_forward(cur: torch.Tensor, c: Consts) -> torch.Tensor:
    """spikes bool [Tc + 1, ...] of the plain forward on cur [Tc, ...] in cur's dtype"""
    dt = cur.dtype
    v = torch.full(cur.shape[1:], c.v_leak, dtype=dt)
    i = torch.zeros(cur.shape[1:], dtype=dt)
    zs = []
    for t in range(cur.shape[0] + 1):
        vd = v + c.a * ((c.v_leak - v) + i)
        z = vd - c.th > 0
        v = torch.where(z, torch.full_like(vd, c.v_reset), vd)
        i = (i + c.b * i) + (cur[t] if t < cur.shape[0] else 0.0)
        zs.append(z)
    return torch.stack(zs)


def adjoint(cur: torch.Tensor, z: torch.Tensor, c: Consts, alpha: float, gz: Optional[torch.Tensor] = None, gu: Optional[torch.Tensor] = None,
            kappa=None, dtype=torch.float64) -> torch.Tensor:
    """d_cur [Tc, ...] in ``dtype``.  cur [Tc, ...], z bool [Tc + 1, ...] (the SAVED spikes: teacher forcing), upstream gradient gz [Tc + 1, ...]
    + kappa[t] gu [...]; the constants are the fp32 values of ``c`` taken into ``dtype``"""
    Tc = cur.shape[0]
    cur = cur.to(dtype)
    zf = z.to(dtype)
    a, b, vl, vr, th = (torch.tensor(x, dtype=dtype) for x in c)
    al = torch.tensor(alpha, dtype=dtype)
    one = torch.tensor(1.0, dtype=dtype)
    v = torch.full(cur.shape[1:], float(vl), dtype=dtype)
    i = torch.zeros(cur.shape[1:], dtype=dtype)
    vds = []
    for t in range(Tc + 1):
        vd = v + a * ((vl - v) + i) if t else v.clone()
        vds.append(vd)
        v = torch.where(z[t], vr.expand_as(vd), vd)
        if t < Tc:
            i = (i + b * i) + cur[t]
    Gv = torch.zeros_like(v)
    Gi = torch.zeros_like(v)
    one_b, one_a = one + b, one - a
    out = [None] * Tc
    for t in range(Tc, -1, -1):
        if t < Tc:
            out[t] = Gi
        up = gz[t].to(dtype) if gz is not None else torch.zeros_like(v)
        if gu is not None:
            up = up + torch.tensor(kappa[t], dtype=dtype) * gu.to(dtype)
        d = al * torch.abs(vds[t] - th) + one
        s = one / (d * d)
        dz = up + Gv * (vr - vds[t])
        dvd = Gv * (one - zf[t]) + dz * s
        Gi = dvd * a + Gi * one_b
        Gv = dvd * one_a
    return torch.stack(out)


def kappa(c: Consts, T: int, li_order: str, dtype) -> np.ndarray:
    """the LI impulse responses the library forms on the host: its double recursion (tests/_readout_grad.kappa64), rounded to fp32 for the
    fp32 evaluation as the library rounds them for the kernel"""
    k = RG.kappa64(c.a, -c.b, T, li_order)                               # (kappa64 takes dt * tau_syn_inv, the positive product)
    return k.astype(np.float32).astype(np.float64) if dtype == torch.float32 else k


def pack_bits(z: torch.Tensor, set_padding: bool = False) -> torch.Tensor:
    """bool [T, R, N] -> int32 [T, R, ceil(N / 32)], bit n & 31 of word n >> 5; ``set_padding``: the bits at or above N are set"""
    zn = z.numpy().astype(bool)
    T, R, N = zn.shape
    W = (N + 31) // 32
    full = np.full((T, R, W * 32), bool(set_padding))
    full[:, :, :N] = zn
    words = np.ascontiguousarray(np.packbits(full, axis=2, bitorder="little")).view(np.uint32).reshape(T, R, W)
    return torch.from_numpy(words.view(np.int32).copy())


def unpack_bits(rows: torch.Tensor, N: int) -> torch.Tensor:
    """int32 [T, R, W] -> bool [T, R, N]"""
    a = np.ascontiguousarray(rows.cpu().numpy()).view(np.uint8)
    T, R, W4 = a.shape
    return torch.from_numpy(np.unpackbits(a, axis=2, bitorder="little")[:, :, :N].astype(bool))


def draw_currents(Tc: int, R: int, N: int, ldc: int, rate: float, c: Consts, seed) -> torch.Tensor:
    """fp32 currents [Tc, R, ldc] whose fp64 forward spikes at about ``rate`` per neuron and step over the steps 1 .. Tc (step 0 never
    spikes: the membrane starts at rest); the padding columns hold NaN.  The draw is uniform noise on (-0.6, 1.4) times a scale found by
    bisection on the forward itself (the rate grows with the scale)"""
    g = torch.Generator().manual_seed(int(np.random.default_rng(seed).integers(2 ** 31)))
    noise = torch.rand((Tc, R, N), generator=g) * 2.0 - 0.6
    lo, hi = 0.0, 64.0 * max(c.th - c.v_leak, 0.05) / c.a
    for _ in range(24):
        mid = 0.5 * (lo + hi)
        seen = float(lif_forward((noise * mid).float().double(), c)[1:].float().mean())
        lo, hi = (mid, hi) if seen < rate else (lo, mid)
    cur = torch.full((Tc, R, ldc), float("nan"), dtype=torch.float32)
    cur[:, :, :N] = (noise * hi).float()
    return cur


def spike_rows(Tp, rows, K, density, rng):
    """(int32 [T', rows, ceil(K / 32)] with the padding bits SET, float64 [T' rows, K])"""
    z = torch.from_numpy(rng.random((Tp, rows, K)) < density)
    return pack_bits(z, set_padding=True), z.reshape(Tp * rows, K).double().numpy()


def padded(d: torch.Tensor, ldd: int) -> torch.Tensor:
    """fp32 [T', rows, N] -> [T', rows, ldd] with NaN in the padding columns"""
    out = torch.full(d.shape[:2] + (ldd,), float("nan"), dtype=torch.float32)
    out[:, :, :d.shape[2]] = d
    return out


def exact_wgrad_case(rows, K, N, Tp, density, acc, seed) -> dict:
    """the integer grid of snn_spike_linear_wgrad: gradients are integer numbers of units 2^-10 with |units| <= 128, so every sum over the
    M = T' rows reduction rows, in any order, stays below 2^24 units and the float64 expectation must come back bit for bit.
    a_rows int32 [T', rows, ceil(K / 32)] (padding bits set), d fp32 [T', rows, N], prior fp32 [N, K] (what accumulate = 1 adds to; drawn
    either way), want32 fp32 [N, K]"""
    rng = np.random.default_rng(seed)
    a_rows, bits = spike_rows(Tp, rows, K, density, rng)
    units = rng.integers(-128, 129, size=(Tp, rows, N))
    assert Tp * rows * 128 + 64 < 2 ** 24                            # every sum, in any order, stays below 2^24 units of 2^-10
    d = torch.from_numpy((units * 2.0 ** -10).astype(np.float32))
    want = units.reshape(Tp * rows, N).astype(np.float64).T @ bits    # exact in float64
    prior = rng.integers(-64, 65, size=(N, K)).astype(np.float64)
    if acc:
        want = want + prior
    want32 = (want * 2.0 ** -10).astype(np.float32)
    assert np.array_equal(want32.astype(np.float64), want * 2.0 ** -10)
    return dict(a_rows=a_rows, d=d, prior=torch.from_numpy((prior * 2.0 ** -10).astype(np.float32)), want32=want32)


def errors(got: torch.Tensor, ref64: torch.Tensor):
    """(largest absolute error, rms error) against the fp64 yardstick"""
    d = got.to(torch.float64) - ref64
    return float(d.abs().max()), float(d.pow(2).mean().sqrt())
