"""Synthetic spike planes behind hand-filled views, and what snn_li_heads_wgrad must return for them (test infrastructure, host only; the
builders of tests/test_gpu_readout_grad.py).

A plane set is drawn as dense bits, packed into 32-bit words and laid out as one of the three layouts of include/snn_hip.h through
tests/_taps.word_index.  The bits at or above n_cols - the padding of the last word, and whole words a view carries beyond the counted
columns - are SET: a kernel that reads them as spikes is off by a whole kappa fold.  Steps may lie further apart than a plane is long and the
planes may start behind an offset; the words in between are 0xa5a5a5a5.

The exact grid: dyadic neuron constants (tests/_li_grid.SETS) make every kappa an integer number of units 2^-fb; gradients are integer
numbers of units 2^-3 with |g| <= 1.  If sum_r |g| S stays under 2^24 units of 2^-(fb + 3) for every output, every partial sum in every order
is exact in fp32 and the expectation, evaluated in integers, must come back bit for bit.  A draw takes the first rung of LADDER that meets
the budget (BudgetError if none does: never skipped)."""
import functools
from typing import Optional, Tuple

import numpy as np

from tests import _li_grid as L
from tests import _taps as TP

G_SHIFT = 3                                       # gradients in units of 2^-3, |g| <= 1
BUDGET = 2 ** 24
PRIOR = 64                                        # |units| of what accumulate = 1 adds to
#          spike density, largest |g| in units, share of non-zero g
LADDER = ((0.12, 8, 1.0), (0.08, 8, 0.5), (0.05, 4, 0.5), (0.03, 2, 0.25), (0.02, 1, 0.1), (0.01, 1, 0.03))

ROWS = (1, 63, 65, 257, 1031)
N_COLS = (20, 96, 256, 1024)
OUTS = ((1, 4), (3, 12), (9, 36), (91, 364), (5, 0), (0, 7))
SET_T = (("a2_b2", 8), ("a2_b1", 12), ("a2_b4", 8), ("pm1", 24))
TILE_STRIDE_ROWS = 512 * 64 + 64 + 5              # more tiles than slabs: a slab walks tiles slab, slab + 512


def words_of(n_cols: int, layout: int, extra_words: int = 0) -> int:
    w = (n_cols + 31) // 32 + extra_words
    return (w + 3) // 4 * 4 if layout == TP.SPLIT4 else w


def make_planes(T: int, rows: int, n_cols: int, layout: int, density: float, seed, extra_words: int = 0, pad_stride: int = 0,
                offset_bytes: int = 0) -> Tuple[np.ndarray, dict, np.ndarray]:
    """(flat uint32 buffer, view fields, spikes bool [T, rows, n_cols])"""
    rng = np.random.default_rng(seed)
    words = words_of(n_cols, layout, extra_words)
    bits = rng.random((T, rows, words * 32)) < density
    bits[:, :, n_cols:] = True
    packed = np.packbits(bits, axis=2, bitorder="little").reshape(T, rows, words, 4)
    rows_u32 = np.ascontiguousarray(packed).view(np.uint32).reshape(T, rows, words)
    stride = rows * words + pad_stride
    assert offset_bytes % 4 == 0
    flat = np.full(offset_bytes // 4 + T * stride, 0xa5a5a5a5, dtype=np.uint32)
    idx = TP.word_index(layout, rows, words)
    for t in range(T):
        flat[offset_bytes // 4 + t * stride + idx] = rows_u32[t]
    view = dict(offset=offset_bytes, stride=stride, rows=rows, words=words, layout=layout, steps_formed=T)
    return flat, view, np.ascontiguousarray(bits[:, :, :n_cols])


def fold_units(spk: np.ndarray, ku: np.ndarray) -> np.ndarray:
    """S in kappa units: int64 [rows, n_cols] = sum_{t < T'} ku[t] * spk[t]"""
    Tp = ku.shape[0]
    return np.tensordot(ku.astype(np.int64), spk[:Tp].astype(np.int64), axes=(0, 0))


def demand_units(g_units: np.ndarray, s_units: np.ndarray) -> np.ndarray:
    """sum_r |g| |S| per (output, column), in units of 2^-(fb + G_SHIFT) (through float64: exact below 2^53)"""
    d = np.abs(g_units).astype(np.float64).T @ np.abs(s_units).astype(np.float64)
    assert d.max(initial=0) < 2.0 ** 52
    return d


def expect_units(g_units: np.ndarray, s_units: np.ndarray) -> np.ndarray:
    e = g_units.astype(np.float64).T @ s_units.astype(np.float64)
    return e.astype(np.int64)


def units_to_fp32(units: np.ndarray, shift: int) -> np.ndarray:
    assert np.abs(units).max(initial=0) <= BUDGET
    x = units.astype(np.float64) * 2.0 ** -shift
    y = x.astype(np.float32)
    assert np.array_equal(y.astype(np.float64), x)
    return y


def draw_grads(rows: int, n: int, amp: int, share: float, rng) -> np.ndarray:
    """int64 [rows, n]: gradients in units of 2^-G_SHIFT"""
    g = rng.integers(1, amp + 1, size=(rows, n)) * rng.choice([-1, 1], size=(rows, n))
    return (g * (rng.random((rows, n)) < share)).astype(np.int64)


@functools.lru_cache(maxsize=4)
def exact_case(rows: int, n_cols: int, layout: int, NA: int, NB: int, name: str, T: int, Tp: int, li_order: str, extra_words: int = 0,
               pad_stride: int = 0, offset_bytes: int = 0) -> dict:
    """planes, gradients and the kappa of the readout at T' for one case of the exact grid; the first rung of LADDER that meets the budget"""
    if not L.admitted(name, Tp, li_order, False):
        raise L.BudgetError("kappa_last of %s at T' = %d (%s) is not admitted" % (name, Tp, li_order))
    ku, fb = L._kappa_units(name, Tp, li_order, "last")
    seed = [rows, n_cols, layout, NA, NB, sorted(L.SETS).index(name), T, Tp, L.ORDERS.index(li_order)]
    worst = None
    for rung, (density, amp, share) in enumerate(LADDER):
        flat, view, spk = make_planes(T, rows, n_cols, layout, density, seed + [rung], extra_words, pad_stride, offset_bytes)
        rng = np.random.default_rng(seed + [rung, 1])
        g = draw_grads(rows, NA + NB, amp, share, rng)
        if rows * (NA + NB) > 8 and not g.any():
            g[0, 0] = 1
        worst = float(demand_units(g, fold_units(spk, ku)).max(initial=0))
        if worst + PRIOR < BUDGET:
            prior = rng.integers(-PRIOR, PRIOR + 1, size=(NA + NB, n_cols)).astype(np.int64)
            return dict(flat=flat, view=view, spk=spk, g=g, ku=ku, fb=fb, prior=prior, rung=rung, name=name, T=T, Tp=Tp, li_order=li_order,
                        NA=NA, NB=NB, n_cols=n_cols)
    raise L.BudgetError("no rung meets the budget for %s: %.3g units asked of 2^24" % ((rows, n_cols, layout, NA, NB, name, T, Tp, li_order), worst))


def exact_grid():
    """(id, keyword arguments of exact_case, accumulate): every layout x n_cols x rows, with the outputs, the set, T', the order, accumulate and
    the view's slack (words beyond n_cols, a step stride beyond a plane, an offset) dealt round-robin on strides that do not divide each other;
    then every (NA, NB) on every layout; then T' in {1, 2, T} x both orders x accumulate on one multi-slab shape"""
    out, i = [], 0

    def add(rows, n_cols, layout, NA, NB, name, T, tsel, order, acc, slack):
        Tp = (1, 2, T)[tsel]
        kw = dict(rows=rows, n_cols=n_cols, layout=layout, NA=NA, NB=NB, name=name, T=T, Tp=Tp, li_order=order,
                  extra_words=1 if slack & 1 else 0, pad_stride=7 if slack & 2 else 0, offset_bytes=132 if slack & 4 else 0)
        out.append(("r%d_c%d_l%d_o%dx%d_%s_T%dof%d_%s_acc%d_s%d" % (rows, n_cols, layout, NA, NB, name, Tp, T, order[0], acc, slack), kw, acc))
    for layout in TP.LAYOUTS:
        for n_cols in N_COLS:
            for rows in ROWS:
                NA, NB = OUTS[i % 6]
                name, T = SET_T[(i // 2) % 4]
                add(rows, n_cols, layout, NA, NB, name, T, (i // 3) % 3, L.ORDERS[(i // 5) % 2], (i // 4) % 2, i % 8)
                i += 1
    for layout in TP.LAYOUTS:
        for j, (NA, NB) in enumerate(OUTS):
            name, T = SET_T[j % 4]
            add(65, 96, layout, NA, NB, name, T, 2, L.ORDERS[j % 2], (j + layout) % 2, (j + 3) % 8)
    for tsel in range(3):
        for order in L.ORDERS:
            for acc in (0, 1):
                add(257, 256, TP.SPLIT4, 3, 12, "a2_b2", 8, tsel, order, acc, 0)
    return out


# ---- default constants: the fp64 yardstick ------------------------------------------------------------------------------------------------
def kappa64(a: float, b: float, T: int, li_order: str) -> np.ndarray:
    """li_kappa's recursion in double on (double)fp32(a), (double)fp32(-b), BEFORE its cast to fp32: the last membrane of a unit current at step s"""
    a, cb = float(np.float32(a)), float(np.float32(-b))
    last = np.zeros(T)
    for s in range(T):
        v = i = 0.0
        for t in range(s, T):
            x = 1.0 if t == s else 0.0
            if li_order == "jump_first":
                i_in = i + x
                v = v + a * (i_in - v)
                i = i_in + cb * i_in
            else:
                v = v + a * (i - v)
                i = i + cb * i + x
        last[s] = v
    return last


def fold64(spk: np.ndarray, k64: np.ndarray) -> np.ndarray:
    """S64 [rows, n_cols] = sum_t k64[t] * spk[t], one step at a time (no [T, rows, n_cols] of doubles)"""
    S = np.zeros(spk.shape[1:], dtype=np.float64)
    for t in range(k64.shape[0]):
        S += k64[t] * spk[t]
    return S


def bound(rows: int, Tp: int, g: np.ndarray, S64: np.ndarray) -> np.ndarray:
    """|G - G64| <= (rows + 2 T' + 4) 2^-24 sum_r |g| S64, element-wise: the standard bound for any summation order of rows products whose
    factor S carries T' - 1 additions, plus kappa's single rounding and the product's.  Derived, not measured."""
    return (rows + 2 * Tp + 4) * 2.0 ** -24 * (np.abs(g).astype(np.float64).T @ np.abs(S64))


#                 rows, n_cols, layout,        NA, NB, T,  T', order,           slack
YARDSTICK = ((1, 20, TP.ROWS, 1, 4, 8, 8, "jump_first", 0), (63, 96, TP.WORD_MAJOR, 3, 12, 8, 5, "voltage_first", 3),
             (65, 256, TP.SPLIT4, 3, 12, 8, 8, "jump_first", 4), (257, 1024, TP.ROWS, 9, 36, 12, 12, "jump_first", 2),
             (1031, 1024, TP.ROWS, 91, 364, 12, 12, "voltage_first", 1), (1031, 256, TP.SPLIT4, 0, 7, 16, 2, "jump_first", 6),
             (257, 96, TP.SPLIT4, 5, 0, 32, 32, "jump_first", 7), (1031, 20, TP.WORD_MAJOR, 9, 36, 8, 1, "jump_first", 5),
             (TILE_STRIDE_ROWS, 96, TP.SPLIT4, 3, 12, 4, 4, "jump_first", 0), (TILE_STRIDE_ROWS, 20, TP.WORD_MAJOR, 1, 4, 4, 3, "voltage_first", 3))


@functools.lru_cache(maxsize=2)
def float_case(rows, n_cols, layout, NA, NB, T, Tp, li_order, slack, seed: int = 0) -> dict:
    flat, view, spk = make_planes(T, rows, n_cols, layout, 0.15, [rows, n_cols, layout, NA, NB, T, seed], 1 if slack & 1 else 0, 7 if slack & 2 else 0,
                                  132 if slack & 4 else 0)
    rng = np.random.default_rng([rows, n_cols, NA, NB, seed, 9])
    g = rng.standard_normal((rows, NA + NB)).astype(np.float32)
    return dict(flat=flat, view=view, spk=spk, g=g, T=T, Tp=Tp, li_order=li_order, NA=NA, NB=NB, n_cols=n_cols)
