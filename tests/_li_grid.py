"""Dyadic neuron constants and head weights on a grid: LI-head outputs that are the same fp32 number in EVERY summation order (test
infrastructure, host only; the builders of tests/test_li_grid_cpu.py and tests/test_gpu_li_grid.py, next to tests/_exact_grid.py).

The launcher folds the LI cell into impulse responses kappa (li_kappa in csrc/snn_post.h: computed in double, cast to fp32); an output is
sum_t kappa_t * (spk_t . W).  If a = dt * tau_mem_inv and b = dt * tau_syn_inv are powers of two, every kappa_t is a dyadic rational with
`fb` fractional bits; if every head weight is an integer number of units 2^-s, every term is an integer number of units 2^-(fb + s), and if

    sum_t |kappa_t| * sum_k (|hi| + |mid| + |lo|)(w_k) * spk[t, k]  <=  2^24 units      for every (row, column)

(hi, mid, lo the three bf16 planes of a weight, which the matrix-core kernels add separately) then every partial sum of every subset of the
terms is exact in fp32: the t-ascending fma chain over per-step products of the matrix-core epilogues, the k-ascending sum of the
kappa-folded S[k] = sum_t kappa_t * bit[t, k] of the fp32 VALU kernel (S[k] itself is bounded by the same sum for every k that carries a
weight; a weight of 0 multiplies whatever S[k] is), the four k-quarters of the reduction-split kernel, and the fold of a readout at T' < T.
The expectation is evaluated in INTEGERS here (kappa from fractions.Fraction) and converts to fp32 without loss; tests/_planes.li_fp64
and the fp32 oracle must both equal it bit for bit (tests/test_li_grid_cpu.py), and so must every kernel form (tests/test_gpu_li_grid.py).

The builders never skip: a (set, T) the kappa table does not admit, or a draw that misses the bit budget on every rung of the ladder below,
raises BudgetError, and the CPU file builds every case of the grid."""
import fractions
import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from oracle import snn_oracle as OR
from tests import _exact_grid as G
from tests._planes import li_constants
from tests._sentinels import _bf16_rn, split3

Fr = fractions.Fraction
BUDGET = 2 ** 24
ORDERS = ("jump_first", "voltage_first")

_K = OR.NeuronConstants
# a = dt * tau_mem_inv, b = dt * tau_syn_inv as the fp32 0-dim products of tests/_planes.li_constants: (1/2, 1/2), (1/2, 1), (1/2, 1/4)
# and the existing edge set dt = 10 ms, whose products round to (1, 2) exactly (tests/_exact_grid.NEURON_SETS)
SETS: Dict[str, OR.NeuronConstants] = {
    "a2_b2": _K(dt=2.0 ** -10, tau_mem_inv=512.0, tau_syn_inv=512.0),
    "a2_b1": _K(dt=2.0 ** -10, tau_mem_inv=512.0, tau_syn_inv=1024.0),
    "a2_b4": _K(dt=2.0 ** -10, tau_mem_inv=512.0, tau_syn_inv=256.0),
    "pm1": G.NEURON_SETS["dt_10ms"][0],
}
SET_AB = {"a2_b2": (Fr(1, 2), Fr(1, 2)), "a2_b1": (Fr(1, 2), Fr(1)), "a2_b4": (Fr(1, 2), Fr(1, 4)), "pm1": (Fr(1), Fr(2))}
ROUTE = "abi"                                    # ops.make_params refuses other time constants: hand-made snn_params (tests/_neuron_constants.py)

# The kappa table (jump-first order), as the computation below must reproduce it: per set the T at which every kappa converts to fp32
# without loss and the first listed T at which one does not (None: exact up to SNN_MAX_STEPS = 32), for the last membrane and for the sums.
KAPPA_TABLE = {
    #          last: exact at      refused at   sums: exact at          refused at
    "a2_b2": ((1, 8, 16, 24, 32), None,         (1, 8, 12, 16, 24),     25),
    "a2_b1": ((1, 8, 16, 24, 32), None,         (1, 8, 12, 16, 24),     26),
    "a2_b4": ((1, 8, 10, 12),     16,           (1, 8, 10),             12),
    "pm1":   ((1, 8, 16, 24, 32), None,         (1, 8, 16, 24, 32),     None),
}
# significant bits of the widest kappa (jump-first) where the table states them
KAPPA_SIG = {("a2_b4", "last"): {8: 13, 10: 16, 12: 20, 16: 26}, ("a2_b4", "sum"): {8: 17, 10: 21, 12: 25},
             ("a2_b2", "sum"): {8: 8, 16: 16, 24: 24}, ("a2_b1", "sum"): {8: 8, 16: 16, 24: 24}}
# what the grid USES (a subset of what the table admits: the table's own limits, not the wider ones of single T in between)
T_MAX_LAST = {"a2_b2": 16, "a2_b1": 16, "a2_b4": 12, "pm1": 32}          # a = 1/2 leaves too few weight units beyond T = 16 (fb ~ T)
T_MAX_SUMS = {"a2_b2": 16, "a2_b1": 16, "a2_b4": 10, "pm1": 32}


class BudgetError(AssertionError):
    """a combination the kappa table does not admit, or a case that misses the bit budget: never skipped"""


# ---- kappa, exactly ------------------------------------------------------------------------------------------------------------------------
def _sig_bits(f: Fr) -> int:
    n = abs(f.numerator)
    if n == 0:
        return 0
    return (n // (n & -n)).bit_length()


def _frac_bits(f: Fr) -> int:
    d = f.denominator
    assert d & (d - 1) == 0, "not a dyadic rational"
    return d.bit_length() - 1


def fp32_exact(f: Fr) -> bool:
    """f is a normal fp32 number (or 0): at most 24 significant bits, exponent in range"""
    if f == 0:
        return True
    return _sig_bits(f) <= 24 and Fr(2) ** -126 <= abs(f) < Fr(2) ** 128 and Fr(float(np.float32(float(f)))) == f


@functools.lru_cache(maxsize=None)
def kappa_exact(a: Fr, b: Fr, T: int, li_order: str) -> dict:
    """The impulse responses of the LI cell, restated from include/snn_hip.h (LI update orders) and tests/_planes.li_fp64 in rationals:
    kappa_last[s] = the membrane after step T - 1 of a unit current at step s, kappa_sum[s] = the sum of the membranes of steps s .. T - 1.
      jump-first:     i += x;  v += a (i - v);  i -= b i            voltage-first:  v += a (i - v);  i = i - b i + x
    Returns last, sum (tuples of Fraction), fb_last, fb_sum (fractional bits of the finest), sig_last, sig_sum (significant bits of the widest)."""
    if li_order not in ORDERS:
        raise ValueError(li_order)
    last, tot = [], []
    for s in range(T):
        v = i = acc = Fr(0)
        for t in range(s, T):
            x = Fr(1 if t == s else 0)
            if li_order == "jump_first":
                i = i + x
                v = v + a * (i - v)
                i = i - b * i
            else:
                v = v + a * (i - v)
                i = i - b * i + x
            acc += v
        last.append(v)
        tot.append(acc)
    return dict(last=tuple(last), sum=tuple(tot), fb_last=max(map(_frac_bits, last)), fb_sum=max(map(_frac_bits, tot)),
                sig_last=max(map(_sig_bits, last)), sig_sum=max(map(_sig_bits, tot)))


def set_ab(name: str) -> Tuple[Fr, Fr]:
    """(a, b) of a set from its constants, through the fp32 0-dim tensor products; they must be the dyadic values the set is named after"""
    a, b = li_constants(SETS[name])
    assert (Fr(a), Fr(b)) == SET_AB[name], (name, a, b)
    return Fr(a), Fr(b)


def kappa_of(name: str, T: int, li_order: str) -> dict:
    return kappa_exact(*set_ab(name), T, li_order)


def kappa_admits(name: str, T: int, li_order: str, sums: bool) -> bool:
    """every kappa of the combination converts to fp32 without loss"""
    k = kappa_of(name, T, li_order)
    return all(map(fp32_exact, k["last"])) and (not sums or all(map(fp32_exact, k["sum"])))


def fold_fits(name: str, T: int, li_order: str, sums: bool) -> bool:
    """sum_t |kappa_t| <= 2^24 units of 2^-fb: the VALU kernel's S[k] = sum_t kappa_t * bit[t, k] is exact for EVERY spike train"""
    k = kappa_of(name, T, li_order)
    return all(sum(abs(f) for f in k[q]) * 2 ** k["fb_" + q] <= BUDGET for q in (("last", "sum") if sums else ("last",)))


def admitted(name: str, T: int, li_order: str, sums: bool) -> bool:
    """what the grid may use: the kappa table's verdict and the bound on the kappa fold, inside the limits the table and the budget set (T_MAX_*)"""
    return kappa_admits(name, T, li_order, sums) and fold_fits(name, T, li_order, sums) and T <= (T_MAX_SUMS if sums else T_MAX_LAST)[name]


# admitted by the kappa table and inside T_MAX_*, but refused by the bound on the kappa fold: (1/2, 1/4) at T = 12 in jump-first order has
# fb = 23 and sum_t |kappa_t| = 3.81 > 2.  Listed, not dropped: tests/test_li_grid_cpu.py asserts that exactly these are refused.
FOLD_REFUSED = (("a2_b4", 12, "jump_first", False),)


def _kappa_units(name: str, Tp: int, li_order: str, which: str) -> Tuple[np.ndarray, int]:
    """kappa^(T') of one quantity as integers: (int64 [T'] in units of 2^-fb, fb)"""
    k = kappa_of(name, Tp, li_order)
    fb = k["fb_" + which]
    return np.array([int(f * 2 ** fb) for f in k[which]], dtype=np.int64), fb


# ---- head weights --------------------------------------------------------------------------------------------------------------------------
# the ladder: (non-zero entries per output column, largest |n| in units, spike density of the stage-level draw, most spikes per neuron).
# A case takes the first rung on which it meets the budget; a = 1/2 halves the room with every step, b = 1/4 quarters it.
LADDER = ((12, 3, 0.15, None), (6, 2, 0.12, None), (3, 1, 0.10, None), (1, 1, 0.10, 4), (1, 1, 0.08, 3))
S_UNIT = 6                                        # unit 2^-6 (the issue's feasibility check: integers in [-3, 3] / 64)
WIDE_S = 20                                       # wide variant: unit 2^-20, planted +-(2^17 + odd) units ~ +-0.125
WIDE_PER_COL = 2


def _positions(N: int, K: int, nnz: int, rng: np.random.Generator) -> np.ndarray:
    """int64 [N, nnz]: entry j of column n at a seeded bit of a 32-channel word that advances with n and strides through the Kw words with j
    (the next word where the bit is taken): the entries of a column spread over the reduction, neighbouring columns start in different words"""
    Kw = (K + 31) // 32
    nnz = min(nnz, K)
    out = np.zeros((N, nnz), dtype=np.int64)
    for n in range(N):
        used = set()
        for j in range(nnz):
            wd = (n + j * max(1, Kw // nnz) + (j * Kw) // nnz) % Kw if Kw >= nnz else j % Kw
            while True:
                k = 32 * wd + int(rng.integers(min(32, K - 32 * wd)))
                if k not in used:
                    break
                wd = (wd + 1) % Kw
            used.add(k)
            out[n, j] = k
    return out


def head_weights(N: int, K: int, nnz: int, amp: int, seed: int, variant: str = "plain") -> Tuple[torch.Tensor, int, dict]:
    """[N, K] fp32 head weights (NA + NB output columns as rows), sparse per column: `nnz` entries of +-1 .. +-amp units 2^-s, the rest 0.
      "plain"   s = S_UNIT
      "narrow"  the same (|n| <= 127 units: one bf16 plane carries it; ops.pack_heads_bf16's rounding must leave it unchanged)
      "wide"    s = WIDE_S, and WIDE_PER_COL further entries per column of +-(2^17 + odd) units whose mid AND lo planes are non-zero"""
    rng = np.random.default_rng([seed, N, K, nnz, amp])
    s = WIDE_S if variant == "wide" else S_UNIT
    pos = _positions(N, K, nnz + (WIDE_PER_COL if variant == "wide" else 0), rng)
    n = np.zeros((N, K), dtype=np.float64)
    small = rng.integers(1, amp + 1, size=(N, pos.shape[1])) * rng.choice([-1.0, 1.0], size=(N, pos.shape[1]))
    np.put_along_axis(n, pos, small, axis=1)
    info = dict(s=s, nnz=int(pos.shape[1]), wide_idx=np.zeros((N, 0), dtype=np.int64))
    if variant == "wide":
        wp = pos[:, :WIDE_PER_COL]
        np.put_along_axis(n, wp, G.wide_units(wp.size, rng).reshape(wp.shape), axis=1)
        info["wide_idx"] = wp
    q = (n * 2.0 ** -s).astype(np.float32)
    G.check_grid(q, s, 24, info["wide_idx"])                          # on the grid, hi + mid + lo == q, planted entries with mid, lo != 0
    if variant == "narrow":
        assert np.abs(n).max() <= 127 and np.array_equal(_bf16_rn(q).view(np.uint32), q.view(np.uint32))
    return torch.from_numpy(q), s, info


def plane_units(w: torch.Tensor, s: int) -> np.ndarray:
    """int64 [N, K]: (|hi| + |mid| + |lo|) of every weight in units of 2^-s"""
    hi, mid, lo = split3(w.numpy())
    u = (np.abs(hi).astype(np.float64) + np.abs(mid).astype(np.float64) + np.abs(lo).astype(np.float64)) * 2.0 ** s
    assert np.array_equal(u, np.rint(u))
    return u.astype(np.int64)


def weight_units(w: torch.Tensor, s: int) -> np.ndarray:
    u = w.numpy().astype(np.float64) * 2.0 ** s
    assert np.array_equal(u, np.rint(u))
    return u.astype(np.int64)


# ---- the expectation, in integers ----------------------------------------------------------------------------------------------------------
def _currents(spk: np.ndarray, wu: np.ndarray) -> np.ndarray:
    """spikes {0, 1} [T, M, K], weights int64 [N, K] -> int64 [T, M, N] (through float64: exact below 2^53)"""
    T, M, K = spk.shape
    c = spk.reshape(T * M, K).astype(np.float64) @ wu.T.astype(np.float64)
    assert np.abs(c).max(initial=0) < 2.0 ** 52
    return c.reshape(T, M, -1).astype(np.int64)


def _fold(cur: np.ndarray, ku: np.ndarray) -> np.ndarray:
    """sum_t ku[t] * cur[t] in int64 (|.| checked against overflow in float64 first)"""
    Tp = ku.shape[0]
    bound = (np.abs(ku).astype(np.float64)[:, None, None] * np.abs(cur[:Tp]).astype(np.float64)).sum(axis=0)
    assert bound.max(initial=0) < 2.0 ** 62
    return (ku[:, None, None] * cur[:Tp]).sum(axis=0)


def _to_fp32(units: np.ndarray, shift: int) -> np.ndarray:
    """integer units of 2^-shift -> fp32, asserting that nothing is lost"""
    assert np.abs(units).max(initial=0) <= BUDGET, "an expectation beyond 2^24 units"
    x = units.astype(np.float64) * 2.0 ** -shift
    y = x.astype(np.float32)
    assert np.array_equal(y.astype(np.float64), x), "the expectation does not convert to fp32 without loss"
    return y


def expect(spk: np.ndarray, w: torch.Tensor, s: int, name: str, li_order: str, steps: Sequence[int], sums: bool) -> dict:
    """Expectations of the readouts T' in `steps` on the first T' planes, with the budget checked on the planes actually used:
    last [n, M, N] fp32 (and sum if `sums`), `room` = the smallest budget / demand over everything asserted.  Raises BudgetError."""
    T = spk.shape[0]
    cur = _currents(spk, weight_units(w, s))
    use = _currents(spk, plane_units(w, s))                           # U[t, row, column] = sum_k (|hi| + |mid| + |lo|)(w_k) spk[t, k]
    if use.max(initial=0) > BUDGET:
        raise BudgetError("a per-step product beyond 2^24 units")
    out: Dict[str, List[np.ndarray]] = {"last": [], "sum": []}
    room = np.inf
    for Tp in steps:
        assert 1 <= Tp <= T
        for which in ("last", "sum") if sums else ("last",):
            if not admitted(name, Tp, li_order, which == "sum"):
                raise BudgetError("kappa_%s of %s at T' = %d (%s) is not admitted" % (which, name, Tp, li_order))
            ku, fb = _kappa_units(name, Tp, li_order, which)
            demand = _fold(use, np.abs(ku))                           # in units of 2^-(fb + s): bounds every partial sum in every order
            if np.abs(ku).sum() > BUDGET:
                raise BudgetError("sum_t |kappa_t| beyond 2^24 units of 2^-%d" % fb)
            if demand.max(initial=0) > BUDGET:
                raise BudgetError("kappa_%s at T' = %d: %.3g units asked of 2^24" % (which, Tp, float(demand.max())))
            room = min(room, BUDGET / max(1.0, float(demand.max(initial=0))))
            out[which].append(_to_fp32(_fold(cur, ku), fb + s))
    res = dict(last=np.stack(out["last"]), room=room, cur=cur, use=use)
    if sums:
        res["sum"] = np.stack(out["sum"])
    return res


def check_alive(case: dict) -> None:
    """every step with a non-zero kappa carries a non-zero current into some output; every readout has a non-zero output and at least half of
    all asserted outputs are non-zero - but where nothing can arrive: voltage-first order does not see the last step, so its T' = 1 readout is exact zeros, asserted as such"""
    cur, T = case["cur"], case["T"]
    k = kappa_of(case["set"], T, case["li_order"])
    dead = case.get("dead_steps", 0)                                 # whole heads: a LIF layer cannot fire before its input arrives (shared LIF, lif6: step 0; lif7: 0 and 1)
    assert not np.any(cur[:dead] != 0)
    for t in range(dead, T):
        if k["last"][t] != 0:
            assert np.any(cur[t] != 0), "step %d carries no current" % t
    live = [j for j, Tp in enumerate(case["steps"]) if Tp - (case["li_order"] == "voltage_first") > dead]
    for q in ("last", "sum") if case["sums"] else ("last",):
        for j in range(len(case["steps"])):
            assert np.any(case[q][j] != 0) == (j in live), "readout T' = %d: %s" % (case["steps"][j], "dead" if j in live else "not identically zero")
        if live:
            nz = float((case[q][live] != 0).mean())
            assert nz >= 0.5, "%.2f of the asserted outputs (%s) are non-zero" % (nz, q)


# ---- stage-level cases ---------------------------------------------------------------------------------------------------------------------
def _spikes(T: int, M: int, K: int, density: float, cap: Optional[int], rng: np.random.Generator) -> np.ndarray:
    z = rng.random((T, M, K)) < density
    if cap is not None:                                               # at most `cap` spikes per neuron: the earliest are kept
        z &= np.cumsum(z, axis=0) <= cap
    return z.astype(np.float32)


@functools.lru_cache(maxsize=8)
def stage_case(M: int, K: int, NA: int, NB: int, T: int, name: str, li_order: str = "jump_first", variant: str = "plain",
               steps: Optional[Tuple[int, ...]] = None, sums: bool = True) -> dict:
    """spike planes [T, M, K] and head weights [NA + NB, K] for ops.li_heads / ops.li_heads_readouts with the expectation of every readout
    in `steps` (None: the single readout at T).  `sums`: the time sums are asserted too (kappa_sum must be admitted).  The first rung of
    LADDER that meets the budget is taken; BudgetError if none does."""
    readouts = steps is not None                                      # (a list, even of one, goes through the several-readout entry)
    steps = (T,) if steps is None else tuple(steps)
    assert steps[-1] == T
    seed = [M, K, NA, NB, T, sorted(SETS).index(name), ORDERS.index(li_order), len(steps)]
    err = None
    for rung, (nnz, amp, density, cap) in enumerate(LADDER):
        rng = np.random.default_rng(seed + [rung])
        spk = _spikes(T, M, K, density, cap, rng)
        w, s, info = head_weights(NA + NB, K, nnz, amp, K + NA + rung, variant)
        try:
            e = expect(spk, w, s, name, li_order, steps, sums)
        except BudgetError as ex:
            if "not admitted" in str(ex):
                raise
            err = ex
            continue
        case = dict(kind="stage", M=M, K=K, NA=NA, NB=NB, T=T, set=name, constants=SETS[name], li_order=li_order, variant=variant, steps=steps,
                    readouts=readouts, sums=sums, spk=spk, w=w, s=s, info=info, rung=rung, **e)
        check_alive(case)
        return case
    raise BudgetError("no rung of the ladder meets the budget for %s: %s" % ((M, K, NA, NB, T, name, li_order, variant, steps, sums), err))


# ---- whole-head cases ----------------------------------------------------------------------------------------------------------------------
def _head_case(base: dict, spk: np.ndarray, K: int, NA: int, NB: int, name: str, variant: str, steps, sums: bool, seed: int) -> dict:
    T, li_order = base["T"], base["li_order"]
    steps = (T,) if steps is None else tuple(steps)
    err = None
    for rung, (nnz, amp, _, _) in enumerate(LADDER):
        w, s, info = head_weights(NA + NB, K, nnz, amp, seed + rung, variant)
        try:
            e = expect(spk, w, s, name, li_order, steps, sums)
        except BudgetError as ex:
            if "not admitted" in str(ex):
                raise
            err = ex
            continue
        base = {k: v for k, v in base.items() if k not in ("logits", "bbox", "cls", "w_cls", "w_bbox")}      # (the outputs of the weights that are replaced)
        case = dict(base, spk=spk, w=w, s=s, info=info, rung=rung, set=name, dead_steps=1 if base["kind"] == "rpn" else 2, NA=NA, NB=NB, K_in=K, steps=steps, sums=sums, variant=variant, **e)
        check_alive(case)
        return case
    raise BudgetError("no rung of the ladder meets the budget for the %s head at T = %d on %s: %s" % (base["kind"], T, name, err))


@functools.lru_cache(maxsize=4)
def rpn_case(C: int, A: int, T: int, shapes: Tuple[Tuple[int, int], ...], N: int, seed: int, name: str, li_order: str = "jump_first",
             variant: str = "plain", steps: Optional[Tuple[int, ...]] = None, sums: bool = True) -> dict:
    """tests/_exact_grid.rpn_case (shared conv on the dyadic weight grid, the oracle's planes at the set's constants) with conv_cls / conv_bbox from
    this grid, and the oracle's outputs recomputed with them"""
    grid = "narrow" if variant == "narrow" else "wide"
    base = dict(G.rpn_case(C, A, T, shapes, N, seed, grid, li_order, constants=SETS[name]))
    case = _head_case(base, base["spk"], C, A, 4 * A, name, variant, steps, sums, seed)
    case["w_cls"], case["w_bbox"] = case["w"][:A].reshape(A, C, 1, 1).clone(), case["w"][A:].reshape(4 * A, C, 1, 1).clone()
    return case


@functools.lru_cache(maxsize=4)
def det_case(R: int, C: int, Hd: int, K: int, T: int, seed: int, name: str, li_order: str = "jump_first", variant: str = "plain",
             steps: Optional[Tuple[int, ...]] = None, sums: bool = True) -> dict:
    grid = "narrow" if variant == "narrow" else "wide"
    base = dict(G.det_case(R, C, Hd, K, T, seed, grid, li_order, constants=SETS[name]))
    case = _head_case(base, base["trace"]["spk7"].numpy(), Hd, K, 4 * K, name, variant, steps, sums, seed)
    case["w_cls"], case["w_bbox"] = case["w"][:K].clone(), case["w"][K:].clone()
    return case


def hidden_rates(case: dict) -> Tuple[float, ...]:
    """firing rates of the hidden layers of a whole-head case"""
    return (case["rate"],) if case["kind"] == "rpn" else (case["rate6"], case["rate7"])


def oracle_outputs(case: dict) -> Tuple[np.ndarray, np.ndarray]:
    """(last [M, NA + NB]) of the fp32 oracle's whole-head forward with the case's head weights, rows in the kernels' order"""
    k = case["constants"]
    with torch.no_grad():
        if case["kind"] == "rpn":
            lo, bb = OR.rpn_head_forward(case["feats"], case["w_shared"], case["w_cls"], case["w_bbox"], case["T"], li_order=case["li_order"], constants=k)
            rows = [torch.cat([a, b], dim=1).permute(0, 2, 3, 1).reshape(-1, 5 * case["A"]) for a, b in zip(lo, bb)]
            return torch.cat(rows).numpy()
        c, b = OR.det_head_forward(case["x"], case["w6"], case["w7"], case["w_cls"], case["w_bbox"], case["T"], li_order=case["li_order"], constants=k)
        return torch.cat([c, b], dim=1).numpy()


# ---- the grid (shared by the CPU file, which builds every case, and the GPU file) -----------------------------------------------------------
M_EDGES = (1, 15, 17, 65, 83)
#           K     NA  NB
K_EDGES = ((32, 3, 12), (100, 3, 12), (128, 5, 20), (256, 3, 12), (1024, 2, 8), (1024, 9, 36), (2048, 3, 12))
N_EDGES = ((1, 4), (3, 12), (5, 20), (9, 36), (11, 44), (24, 96), (91, 364))
T_DYADIC = (1, 2, 4, 5, 8, 9, 10, 12, 16)
T_PM1 = (17, 18, 24, 26, 32)
# the three matrix shapes the T edges run on: Kw = 8 resident (the C = 256 RPN path), ksplit by default with NT = 3 (groups of 12) and
# NT = 1 where it is forced (groups of 16)
T_SHAPES = ((83, 256, 3, 12), (17, 1024, 9, 36), (17, 1024, 2, 8))


def t_cases() -> List[tuple]:
    """(M, K, NA, NB, T, set, sums) of the T edges: every dyadic set at every T it is admitted at (sums where kappa_sum is), the +-1 set beyond"""
    out = []
    for (M, K, NA, NB) in T_SHAPES:
        for name in ("a2_b2", "a2_b1", "a2_b4"):
            out += [(M, K, NA, NB, T, name, T <= T_MAX_SUMS[name]) for T in T_DYADIC if T <= T_MAX_LAST[name]]
        out += [(M, K, NA, NB, T, "pm1", True) for T in T_PM1]
    return out


# the default run takes these (set, T) of t_cases on every shape; the rest is marked `sweep`
T_DEFAULT = {"a2_b2": (1, 2, 4, 5, 8, 9, 10, 12, 16), "a2_b1": (2, 5, 10, 16), "a2_b4": (4, 8, 10, 12), "pm1": T_PM1}

READOUT_SHAPES = ((83, 256, 3, 12), (17, 1024, 9, 36), (17, 128, 5, 20), (33, 256, 24, 96))
#                set      T   steps                              (sums follow from T_MAX_SUMS)
READOUT_LISTS = (("a2_b2", 12, tuple(range(1, 13))), ("a2_b1", 11, tuple(range(1, 12))), ("a2_b2", 12, (2, 5, 8, 12)), ("a2_b4", 8, (8,)),
                 ("a2_b4", 10, (1, 4, 9, 10)), ("pm1", 26, tuple(range(1, 27))), ("a2_b1", 16, (16,)))

WIDE_CASES = [(83, 256, 3, 12, T, "pm1") for T in T_PM1] + [(17, 1024, 9, 36, T, "pm1") for T in (12, 26)] + \
             [(83, 256, 3, 12, T, "a2_b1") for T in (2, 4)] + [(17, 1024, 9, 36, 4, "a2_b1"), (17, 128, 24, 96, 8, "pm1")]


def stage_grid() -> List[Tuple[str, dict]]:
    """every stage-level case of the GPU file as (id, keyword arguments of stage_case), both LI orders where the GPU file runs both"""
    out = []
    for M in M_EDGES:
        out.append(("M%d" % M, dict(M=M, K=128, NA=5, NB=20, T=8, name="a2_b1")))
    for K, NA, NB in K_EDGES:
        for order in ORDERS:
            out.append(("K%d_N%d_%s" % (K, NA + NB, order), dict(M=17, K=K, NA=NA, NB=NB, T=9, name="a2_b2", li_order=order)))
    for NA, NB in N_EDGES:
        out.append(("N%d_%d" % (NA, NB), dict(M=17, K=256, NA=NA, NB=NB, T=8, name="a2_b1")))
    for M, K, NA, NB, T, name, sums in t_cases():
        for order in ORDERS:
            if admitted(name, T, order, sums):
                out.append(("T%d_%s_%dx%dx%d_%s" % (T, name, M, K, NA + NB, order), dict(M=M, K=K, NA=NA, NB=NB, T=T, name=name, li_order=order, sums=sums)))
    for (M, K, NA, NB) in READOUT_SHAPES:
        for name, T, steps in READOUT_LISTS:
            out.append(("ro_%s_T%d_n%d_%dx%dx%d" % (name, T, len(steps), M, K, NA + NB),
                        dict(M=M, K=K, NA=NA, NB=NB, T=T, name=name, steps=steps, sums=T <= T_MAX_SUMS[name])))
    for M, K, NA, NB, T, name in WIDE_CASES:
        out.append(("wide_%s_T%d_%dx%dx%d" % (name, T, M, K, NA + NB), dict(M=M, K=K, NA=NA, NB=NB, T=T, name=name, variant="wide")))
    out.append(("narrow", dict(M=83, K=256, NA=3, NB=12, T=12, name="a2_b2", variant="narrow")))
    return out


# whole heads: (id, builder).  RPN: C = 64; C = 256 on the structured-sparse conv (T = 8, 12, 16: half_split planes into the resident heads
# kernel) and the dense conv (T = 4); a two-level pyramid with a ragged last tile.  Detector: Hd = 128, 256, 1024 (K = 9: ksplit), R = 17, 65.
RPN_PYRAMID = G.PYRAMID
RPN_TWO_LEVELS = ((6, 7), (2, 1))


def head_grid() -> List[Tuple[str, object]]:
    P = functools.partial
    out = [("rpn_C64_T8_%s" % n, P(rpn_case, 64, 3, 8, RPN_PYRAMID, 2, 72, n)) for n in ("a2_b2", "a2_b1", "a2_b4")]
    out += [("rpn_C256_T%d_%s" % (T, n), P(rpn_case, 256, 3, T, RPN_PYRAMID, 2, 256 + T, n)) for T, n in RPN_C256]
    out += [("rpn_two_levels", P(rpn_case, 32, 3, 8, RPN_TWO_LEVELS, 2, 3, "a2_b2")),
            ("rpn_voltage_first", P(rpn_case, 64, 3, 12, RPN_PYRAMID, 2, 76, "a2_b2", "voltage_first")),
            ("rpn_wide", P(rpn_case, 64, 3, 4, RPN_PYRAMID, 2, 68, "a2_b1", "jump_first", "wide")),       # (under the +-1 set the shared LIF fires every other step only: the detector carries it)
            ("rpn_narrow", P(rpn_case, 64, 3, 8, RPN_PYRAMID, 2, 72, "a2_b2", "jump_first", "narrow")),
            ("rpn_mx", P(rpn_case, 128, 3, 8, RPN_PYRAMID, 2, 136, "a2_b2")),
            ("rpn_readouts", P(rpn_case, 256, 3, 12, RPN_PYRAMID, 2, 268, "a2_b2", "jump_first", "plain", READOUT_STEPS))]
    out += [("det_Hd%d_R%d_T%d_%s" % (Hd, R, T, n), P(det_case, R, 8, Hd, 9, T, 500 + Hd + R, n)) for (R, Hd, T, n) in DET_SHAPES]
    out += [("det_voltage_first", P(det_case, 17, 8, 128, 9, 12, 645, "a2_b1", "voltage_first")),
            ("det_pm1_wide", P(det_case, 17, 8, 128, 9, 24, 669, "pm1", "jump_first", "wide")),
            ("det_narrow", P(det_case, 17, 8, 128, 9, 12, 645, "a2_b2", "jump_first", "narrow")),
            ("det_readouts", P(det_case, 17, 8, 128, 9, 12, 645, "a2_b1", "jump_first", "plain", READOUT_STEPS))]
    return out


RPN_C256 = ((8, "a2_b4"), (12, "a2_b2"), (16, "a2_b1"), (4, "a2_b2"))
DET_SHAPES = ((17, 128, 12, "a2_b2"), (65, 256, 12, "a2_b1"), (17, 1024, 12, "a2_b2"), (65, 128, 8, "a2_b4"))
READOUT_STEPS = (4, 8, 12)
HEAD_CASES = dict(head_grid())


# ---- the launcher's kappa, three fp32 summation orders, and mutants (tests/test_li_grid_cpu.py) ----------------------------------------------
def kappa_fp32(a: float, b: float, T: int, li_order: str) -> Tuple[np.ndarray, np.ndarray]:
    """li_kappa as the launcher states it: the recursion in double on (double)fp32(a) and (double)fp32(-b), cast to fp32 at the end"""
    a, cb = float(np.float32(a)), float(np.float32(-b))
    last, tot = np.zeros(T, dtype=np.float32), np.zeros(T, dtype=np.float32)
    for s in range(T):
        v = i = acc = 0.0
        for t in range(s, T):
            x = 1.0 if t == s else 0.0
            if li_order == "jump_first":
                i_in = i + x
                v = v + a * (i_in - v)
                i = i_in + cb * i_in
            else:
                v = v + a * (i - v)
                i = i + cb * i + x
            acc += v
        last[s], tot[s] = v, acc
    return last, tot


def emulate_orders(case: dict, j: int, which: str) -> Dict[str, np.ndarray]:
    """readout j of a case in numpy float32, every operation rounded separately (no fma: with the budget met each product is exact), in the
    three orders of the kernels: "t_chain" kappa_t * (spk_t . W) added for t ascending (matrix-core epilogue), "k_chain" S[k] * w_k added for
    k ascending with S[k] = sum_t kappa_t * bit[t, k] (VALU kernel), "k_quarters" four t-chains over quarters of the 32-channel words, added
    in wave order (reduction-split kernel)"""
    Tp, s = case["steps"][j], case["s"]
    a, b = li_constants(case["constants"])
    k32 = kappa_fp32(a, b, Tp, case["li_order"])[0 if which == "last" else 1]
    spk, w = case["spk"][:Tp], case["w"].numpy()
    wu = weight_units(case["w"], s)
    f32 = np.float32

    def t_chain(cols: slice) -> np.ndarray:
        cur = _currents(spk[:, :, cols], wu[:, cols])
        o = np.zeros(cur.shape[1:], dtype=f32)
        for t in range(Tp):
            o = o + k32[t] * (cur[t].astype(np.float64) * 2.0 ** -s).astype(f32)
        return o
    out = {"t_chain": t_chain(slice(None))}
    S = np.zeros(spk.shape[1:], dtype=f32)
    for t in range(Tp):
        S = S + k32[t] * spk[t].astype(f32)
    o = np.zeros((spk.shape[1], w.shape[0]), dtype=f32)
    for k in np.flatnonzero(np.any(w != 0, axis=0)):
        o = o + S[:, k:k + 1] * w[None, :, k]
    out["k_chain"] = o
    Kw = (spk.shape[2] + 31) // 32
    o = None
    for q in range(4):
        part = t_chain(slice(32 * (q * Kw // 4), min(spk.shape[2], 32 * ((q + 1) * Kw // 4))))
        o = part if o is None else o + part
    out["k_quarters"] = o
    assert all(v.dtype == f32 for v in out.values())
    return out


def _value(cur: np.ndarray, ku: np.ndarray, shift: int) -> np.ndarray:
    """sum_t ku[t] cur[t] 2^-shift rounded to fp32 (a mutant's value need not be representable)"""
    return (_fold(cur, ku).astype(np.float64) * 2.0 ** -shift).astype(np.float32)


def mutants(case: dict) -> List[Tuple[str, int, str, bool]]:
    """(mutant, T', quantity, expectation bits changed) for every mutant that applies to a readout of the case: each restates the expectation
    with ONE term wrong, as a kernel or the launcher could have it"""
    s, name, order, T = case["s"], case["set"], case["li_order"], case["T"]
    other = ORDERS[1 - ORDERS.index(order)]
    spk, w = case["spk"], case["w"]
    wu, cur = weight_units(w, s), case["cur"]
    dead = case.get("dead_steps", 0)
    alt: Dict[str, np.ndarray] = {}
    if case["variant"] == "wide":                                     # the lo plane of the planted weights removed
        alt["lo_plane_dropped"] = _currents(spk, wu - weight_units(G.lo_of_planted(w, case["info"]["wide_idx"]), s))
    load = (spk.sum(axis=(0, 1)) * np.abs(wu).sum(axis=0)).reshape(-1)
    wd = int(np.argmax(np.add.reduceat(load, np.arange(0, load.size, 32))))
    z = spk.copy()
    z[:, :, 32 * wd: 32 * wd + 32] = 0                                # one 32-channel word dropped (the most loaded one)
    alt["word_dropped"] = _currents(z, wu)
    if wu.shape[0] > 64:                                              # the second 64-column block reads the first block's weights
        w2 = wu.copy()
        n = min(64, wu.shape[0] - 64)
        w2[64:64 + n] = wu[:n]
        alt["previous_block"] = _currents(spk, w2)
    out = []
    for j, Tp in enumerate(case["steps"]):
        for q in ("last", "sum") if case["sums"] else ("last",):
            exp = case[q][j]
            ku, fb = _kappa_units(name, Tp, order, q)

            def add(mutant, value):
                out.append((mutant, Tp, q, bool(np.any(value.view(np.uint32) != exp.view(np.uint32)))))

            def same(k_alt, fb_alt):                                  # a restatement with the SAME kappa is no mutant (equal neighbours, +-1 at equal parity)
                return [Fr(int(x), 2 ** fb_alt) for x in k_alt] == [Fr(int(x), 2 ** fb) for x in ku]
            if Tp - (order == "voltage_first") <= dead:                # nothing arrives in this readout: only the other order can tell
                if Tp > dead:
                    k2, fb2 = _kappa_units(name, Tp, other, q)
                    add("other_order", _value(cur, k2, fb2 + s))
                continue
            if not same(np.roll(ku, -1), fb):
                add("kappa_shifted", _value(cur, np.roll(ku, -1), fb + s))
            k2, fb2 = _kappa_units(name, Tp, other, q)
            add("other_order", _value(cur, k2, fb2 + s))
            k3, fb3 = _kappa_units(name, Tp, order, "sum" if q == "last" else "last")
            if not same(k3, fb3):
                add("last_sum_swapped", _value(cur, k3, fb3 + s))
            if Tp < T:
                k4, fb4 = _kappa_units(name, T, order, q)
                if not same(k4[:Tp], fb4):
                    add("kappa_of_T", _value(cur, k4[:Tp], fb4 + s))
            t_last = Tp - 1 - (order == "voltage_first")              # the last step that contributes
            if t_last >= dead:
                k5 = ku.copy()
                k5[t_last] = 0
                add("last_step_dropped", _value(cur, k5, fb + s))
            for mutant, c in alt.items():
                add(mutant, _value(c, ku, fb + s))
    return out


MUTANTS = ("kappa_shifted", "other_order", "last_sum_swapped", "kappa_of_T", "lo_plane_dropped", "word_dropped", "previous_block", "last_step_dropped")


# ---- which kernel a call takes: the launcher's plan, restated (csrc/snn_kernels.hip: li_heads_call / li_heads_kind / li_heads_cols) -----------
FORMS = (None, "valu", "ksplit", "mfma")                             # SNN_LI_HEADS as the GPU file sets it (None: by shape)


def li_plan(K: int, NA: int, NB: int, form: Optional[str] = None, strict: bool = False, want_sums: bool = False, readouts: int = 0) -> List[tuple]:
    """the launches behind one snn_li_heads / snn_li_heads_readouts call, one tuple per block of columns:
    ("valu", RB) | ("mfma", NT, "resident" | "streamed", Kw == 8) | ("ksplit", NT), with ("ro", RB_readouts, remainder block?) appended for the
    several-readout matrix-core kernels.  Documentation of what the grid reaches (tests/test_li_grid_cpu.py asserts the coverage table of
    tests/test_gpu_li_grid.py with it); nothing on the GPU is decided by it."""
    Kw, ldw = (K + 31) // 32, (NA + NB + 15) // 16 * 16
    force = 1 if strict else {None: 0, "valu": 1, "mfma": 2, "ksplit": 3}[form]
    step = 256 if force == 1 else 64
    out = []
    for col0 in range(0, ldw, step):
        NOp = min(step, ldw - col0)
        fits = Kw * 3 * NOp * 64 <= 96 * 1024
        if NOp <= 64 and Kw >= 4 and (force == 3 if force else not fits):
            plan = ("ksplit", NOp // 16)
        elif NOp <= 64 and (force == 2 if force else fits):
            plan = ("mfma", NOp // 16, "resident" if fits else "streamed", Kw == 8)
        else:
            jg = NOp // 4
            plan = ("valu", next(rb for rb in (64, 32, 16, 8, 4) if 256 // jg >= rb or rb == 4))
        if readouts and plan[0] != "valu":
            rb = (8 if plan[1] <= 2 else 4) // (2 if want_sums else 1)
            plan += ("ro", rb, readouts % rb != 0)
        out.append(plan)
    return out
