"""Dyadic weight grids: dense conv / fc weights whose currents are the same fp32 number in EVERY summation order (test infrastructure,
host only; the builder next to tests/_sentinels.py).

Spikes are 0 / 1.  If every weight of a layer is an integer multiple of one unit 2^-s and the largest row sum of |w| stays below 2^24
units, every partial sum of every subset of a row's terms - in any order, fused or not - is an integer below 2^24 units and therefore
exact in fp32.  For the bf16x3 kernels the terms are the three bf16 planes hi, mid, lo of a weight (each a multiple of the unit as
well), so the bound is taken over sum(|hi| + |mid| + |lo|).  The oracle's oneDNN currents and the GPU's currents are then the SAME
number, and since the fused LIF epilogues repeat the oracle's fp32 operations in the same order (tests/_sentinels.py pins that for
single-term currents) the hidden spike planes must equal the oracle's with ZERO flips: tests/test_gpu_exact_grid.py has no flip budget.
tests/test_exact_grid_cpu.py proves the precondition on the oracle (fp32 currents bit-equal to an fp64 evaluation) and that removing
one contribution from a current changes the planes.

Two grids:
  "wide"    the modules' own initial weights rounded to the finest unit that keeps every row inside 2^23 units, plus `wide_per_row`
            planted entries per output row that need all THREE planes ((2^17 + odd) units: 18 significant bits, lo != 0) at seeded
            positions spread over the taps and 32-channel k-blocks - the random grid alone is 13 - 17 bits wide and leaves lo empty;
  "narrow"  |n| <= 127 units: 8 significant bits, bf16(q) == q - the single weight plane of precision "bf16" carries it exactly.
The LI-head weights stay as initialised (rounded to bf16 on the narrow grid, so that one oracle run serves "bf16x3" and "bf16"): head sums
multiply by kappa_t and are not exact; they keep the tolerance of tests/_planes.py.
"""
import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import snn_oracle as OR
from tests._sentinels import _bf16_rn, period_input, split3
from tests._util import nchw_to_rows

BUDGET_LOG2 = 23
WIDE_PER_ROW = 8


# ---- the grids -----------------------------------------------------------------------------------------------------------------------
def _rows(w: np.ndarray) -> np.ndarray:
    return w.reshape(w.shape[0], -1)


def plane_units(q: np.ndarray, s: int) -> np.ndarray:
    """sum over a row of (|hi| + |mid| + |lo|) in units of 2^-s (float64, exact: every term is an integer below 2^24)"""
    hi, mid, lo = split3(q)
    tot = np.abs(hi).astype(np.float64) + np.abs(mid).astype(np.float64) + np.abs(lo).astype(np.float64)
    return _rows(tot).sum(axis=1) * 2.0 ** s


def wide_positions(shape: Sequence[int], per_row: int, rng: np.random.Generator) -> np.ndarray:
    """int64 [rows, per_row]: flat reduction indices (k = ci * 9 + tap for OIHW 3x3 weights, the column for linear ones) of the planted
    entries of every row - entry j of row r in 32-channel k-block (j * blocks / per_row + r) mod blocks and, for a conv, on tap (j + r) mod 9;
    distinct within a row"""
    rows = shape[0]
    conv = len(shape) == 4
    chans = shape[1]
    blocks = (chans + 31) // 32
    out = np.zeros((rows, per_row), dtype=np.int64)
    for r in range(rows):
        used = set()
        for j in range(per_row):
            blk = (j * blocks // per_row + r) % blocks
            width = min(32, chans - 32 * blk)
            while True:
                c = 32 * blk + int(rng.integers(width))
                k = c * 9 + (j + r) % 9 if conv else c
                if k not in used:
                    break
                blk = (blk + 1) % blocks                             # (a block narrower than the entries it was dealt: the next one)
                width = min(32, chans - 32 * blk)
            used.add(k)
            out[r, j] = k
    return out


def wide_units(count: int, rng: np.random.Generator) -> np.ndarray:
    """`count` signed integers +-(2^17 + odd), odd < 2^17, whose three-plane split has lo != 0 (float64).  (17 significant bits always
    fit two planes: round-to-nearest residuals are signed, so hi + mid carry 8 + 9 bits; 18 bits leave a residual for lo about every
    second time.)"""
    out = np.zeros(0)
    while out.size < count:
        n = (2.0 ** 17 + 2.0 * rng.integers(0, 1 << 16, size=2 * count + 16) + 1.0) * rng.choice([-1.0, 1.0], size=2 * count + 16)
        _, _, lo = split3(n.astype(np.float32))
        out = np.concatenate([out, n[lo != 0]])
    return out[:count]


def n_wide_for(shape: Sequence[int], wide_per_row: int) -> int:
    """planted entries per row: `wide_per_row`, fewer in rows shorter than four times that (at most a quarter of a row, at least one)"""
    k = int(np.prod(shape[1:]))
    return min(wide_per_row, max(1, k // 4))


def dyadic(w: torch.Tensor, budget_log2: int = BUDGET_LOG2, wide_per_row: int = WIDE_PER_ROW, seed: int = 0,
           info: Optional[dict] = None) -> Tuple[torch.Tensor, int]:
    """w (fp32, [N, ...]: one output row per leading index) -> (q, s): w rounded to multiples of 2^-s with `wide_per_row` planted
    three-plane entries per row, s the largest exponent for which every row has sum(|hi| + |mid| + |lo|) <= 2^budget_log2 units and every
    entry stays below 2^24 units.  ``info`` receives s, the planted positions (`wide_idx` [rows, n]) and the largest row sum in units."""
    w64 = w.detach().cpu().numpy().astype(np.float64)
    shape = w64.shape
    rng = np.random.default_rng([seed, int(np.prod(shape)), 7])
    n_wide = n_wide_for(shape, wide_per_row) if wide_per_row > 0 else 0
    idx = wide_positions(shape, n_wide, rng) if n_wide else np.zeros((shape[0], 0), dtype=np.int64)
    planted = wide_units(idx.size, rng).reshape(idx.shape) if n_wide else np.zeros(idx.shape)
    rsum = float(np.abs(_rows(w64)).sum(axis=1).max())
    amax = float(np.abs(w64).max())
    assert amax > 0
    s = min(int(np.ceil(np.log2(2.0 ** budget_log2 / rsum))) + 1, int(np.floor(np.log2((2.0 ** 24 - 1) / amax))))
    while True:
        n = np.rint(w64 * 2.0 ** s)
        if n_wide:
            np.put_along_axis(_rows(n), idx, planted, axis=1)
        q = (n * 2.0 ** -s).astype(np.float32)
        units = plane_units(q, s)
        if np.abs(n).max() < 2.0 ** 24 and units.max() <= 2.0 ** budget_log2:
            break
        s -= 1
    check_grid(q, s, budget_log2, idx)
    if info is not None:
        info.update(s=s, wide_idx=idx, n_wide=n_wide, max_row_units=float(units.max()),
                    bits=int(np.ceil(np.log2(np.abs(n).max() + 1))))
    return torch.from_numpy(q.reshape(shape)), s


def narrow(w: torch.Tensor, info: Optional[dict] = None) -> Tuple[torch.Tensor, int]:
    """w -> (q, s): multiples of 2^-s with |n| <= 127 (8 significant bits), s the largest such exponent: bf16(q) == q"""
    w64 = w.detach().cpu().numpy().astype(np.float64)
    s = int(np.floor(np.log2(127.5 / float(np.abs(w64).max()))))
    while np.abs(np.rint(w64 * 2.0 ** s)).max() > 127:
        s -= 1
    q = (np.rint(w64 * 2.0 ** s) * 2.0 ** -s).astype(np.float32)
    check_grid(q, s, BUDGET_LOG2, np.zeros((q.shape[0], 0), dtype=np.int64))
    assert np.array_equal(_bf16_rn(q).view(np.uint32), q.view(np.uint32)), "the narrow grid is not bf16-representable"
    if info is not None:
        info.update(s=s, wide_idx=np.zeros((q.shape[0], 0), dtype=np.int64), n_wide=0, max_row_units=float(plane_units(q, s).max()), bits=7)
    return torch.from_numpy(q), s


def check_grid(q: np.ndarray, s: int, budget_log2: int, wide_idx: np.ndarray) -> None:
    """the builder's assertions: every entry an integer number of units that round-trips through fp64, hi + mid + lo == q bitwise, each
    plane on the grid as well, every row inside the budget, lo != 0 at the planted entries"""
    q = np.ascontiguousarray(q, dtype=np.float32)
    n = q.astype(np.float64) * 2.0 ** s
    assert np.array_equal(n, np.rint(n)) and np.abs(n).max() < 2.0 ** 24, "not on the grid"
    assert np.array_equal((n * 2.0 ** -s).astype(np.float32).view(np.uint32) & 0x7fffffff, q.view(np.uint32) & 0x7fffffff), "no fp64 round trip"
    hi, mid, lo = split3(q)
    back = ((hi + mid) + lo).astype(np.float32)
    nz = q != 0
    assert np.array_equal(back.view(np.uint32)[nz], q.view(np.uint32)[nz]) and np.all(back[~nz] == 0), "hi + mid + lo != q"
    for p in (hi, mid, lo):
        u = p.astype(np.float64) * 2.0 ** s
        assert np.array_equal(u, np.rint(u)), "a plane is off the grid"
    assert plane_units(q, s).max() <= 2.0 ** budget_log2, "a row leaves the budget"
    if wide_idx.size:
        assert np.all(np.take_along_axis(_rows(lo), wide_idx, axis=1) != 0), "a planted entry has an empty lo plane"
        assert np.all(np.take_along_axis(_rows(mid), wide_idx, axis=1) != 0)


def lo_of_planted(q: torch.Tensor, wide_idx: np.ndarray) -> torch.Tensor:
    """a tensor like q holding the lo plane of the planted entries and zero elsewhere (what a kernel that drops lo would lose)"""
    _, _, lo = split3(q.numpy())
    out = np.zeros_like(_rows(lo))
    np.put_along_axis(out, wide_idx, np.take_along_axis(_rows(lo), wide_idx, axis=1), axis=1)
    return torch.from_numpy(out.reshape(q.shape))


def _grid(w: torch.Tensor, grid: str, seed: int, info: dict) -> torch.Tensor:
    if grid == "wide":
        return dyadic(w, seed=seed, info=info)[0]
    if grid == "narrow":
        return narrow(w, info=info)[0]
    raise ValueError(grid)


def _round_bf16(w: torch.Tensor) -> torch.Tensor:
    return w.detach().to(torch.bfloat16).to(torch.float32)


# ---- features ------------------------------------------------------------------------------------------------------------------------
def _half_grid(x: torch.Tensor, feat: Optional[str]) -> torch.Tensor:
    """features on the grid of a half-precision type (as fp32): what both the oracle and, cast back, the kernels see"""
    if feat == "fp16":
        return x.to(torch.float16).float()
    if feat == "bf16":
        return x.to(torch.bfloat16).float()
    return x


def full_nibble_values(shape: Sequence[int], T: int, g: torch.Generator) -> torch.Tensor:
    """[N, C, ...] features constant over aligned groups of FOUR channels, each group (per image and position) on one encoder period
    n in 3 .. min(T - 1, 7), the value in the middle of that period's fp32 interval (tests/_sentinels.period_input: found by bisection
    on the oracle's encoder step, no literal boundaries).  A nibble of the period planes e_3 .. that holds a spike then holds four: every
    16-row tile of the structured-sparse launches takes the secondary pass (cf. bench.worst_case_tensor)."""
    periods = list(range(3, max(3, min(T - 1, 7)) + 1))
    vals = torch.tensor([period_input(p) for p in periods], dtype=torch.float32)
    N, C = shape[0], shape[1]
    pick = torch.randint(0, len(periods), (N, (C + 3) // 4, *shape[2:]), generator=g)
    return vals[pick].repeat_interleave(4, dim=1)[:, :C].contiguous()


def nibble_hit_fraction(z: np.ndarray) -> Tuple[float, int]:
    """z {0, 1} [T, M, K] encoder spikes in the kernels' reduction order (K a multiple of 4) -> (fraction of 16-row tiles in which some
    nibble of a period plane e_n, 3 <= n <= T - 1, holds >= 3 ones; number of occupied nibbles that are not full)"""
    T, M, K = z.shape
    before = np.zeros((M, K), dtype=bool)
    hit = np.zeros((M + 15) // 16, dtype=bool)
    partial = 0
    for n in range(1, T):                                            # e_n: first spike at step n - 1; the sparse pass reads e_3 .. e_(T-1) (bench.planes_hit_stats)
        e = (z[n - 1] > 0) & ~before
        before |= z[n - 1] > 0
        if n < 3:
            continue
        c = e.reshape(M, K // 4, 4).sum(axis=2)
        partial += int(((c > 0) & (c < 4)).sum())
        rows = (c >= 3).any(axis=1)
        hit |= np.add.reduceat(rows, np.arange(0, M, 16)) > 0
    return float(hit.mean()), partial


def mx_block_span_bits(q: torch.Tensor, s: int) -> int:
    """the pack definition of the block-scaled fp6 digit planes (restated by tests/test_gpu_mx.py: six base-32 digits under the biased
    exponent Eb of a block of 32 consecutive reduction indices, exact for every weight whose lowest bit is >= 2^(Eb - 155)): the largest
    number of bits, over all blocks, from the top bit of the block maximum down to the unit 2^-s - the grid is carried exactly while this
    is <= 27 (Eb may sit one above the maximum's exponent).  Blocks are taken along each row's flat reduction index and, for a conv,
    along the channels of each tap: a bound over whole rows covers every blocking."""
    n = np.abs(q.numpy().astype(np.float64).reshape(q.shape[0], -1)) * 2.0 ** s
    assert np.array_equal(n, np.rint(n))
    return int(np.ceil(np.log2(n.max(axis=1) + 1)).max())


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=6)
def rpn_case(C: int, A: int, T: int, shapes: Tuple[Tuple[int, int], ...], N: int, seed: int, grid: str = "wide",
             li_order: str = "jump_first", feat: Optional[str] = None, full_nibble: bool = False,
             constants: Optional[OR.NeuronConstants] = None) -> dict:
    """tests/test_gpu_shape_sweeps._rpn_case with shared_conv.weight on a dyadic grid: same feature scale (N(0, 1.7)), module
    construction (RPNHeadSNN(C, A, T) after torch.manual_seed(seed), shared conv x 4) and seeding.  Returns the module weights, the
    features, the oracle's outputs, trace and integer spike counts, and the grid's figures.  ``constants``: the neuron constants the oracle
    runs at (None: the reference's); features and weights do not depend on them."""
    import snn_automotive_object_detection_amd as S
    g = torch.Generator().manual_seed(seed)
    if full_nibble:
        feats = [full_nibble_values((N, C, h, w), T, g) for h, w in shapes]
    else:
        feats = [_half_grid(torch.randn(N, C, h, w, generator=g) * 1.7, feat) for h, w in shapes]
    torch.manual_seed(seed)
    m = S.RPNHeadSNN(C, A, T)
    info: Dict = {}
    w_shared = _grid(m.shared_conv.weight.detach() * 4.0, grid, seed, info)
    w_cls, w_bbox = m.conv_cls.weight.detach().clone(), m.conv_bbox.weight.detach().clone()
    if grid == "narrow":
        w_cls, w_bbox = _round_bf16(w_cls), _round_bf16(w_bbox)
    counts: List[torch.Tensor] = []
    with torch.no_grad():
        logits, bbox, traces = OR.rpn_head_forward(feats, w_shared, w_cls, w_bbox, T, li_order=li_order, trace=True, counts_out=counts,
                                                     constants=constants)
    spk = np.concatenate([nchw_to_rows(tr["spk"]) for tr in traces], axis=1)                     # [T, P, C], levels back to back
    return dict(kind="rpn", C=C, A=A, T=T, N=N, shapes=list(shapes), li_order=li_order, grid=grid, feat=feat, w_shared=w_shared,
                w_cls=w_cls, w_bbox=w_bbox, feats=feats, logits=logits, bbox=bbox, traces=traces, spk=spk,
                counts=torch.stack(counts).numpy(), info=info, rate=float(spk.mean()), constants=constants)


@functools.lru_cache(maxsize=6)
def det_case(R: int, C: int, Hd: int, K: int, T: int, seed: int, grid: str = "wide", li_order: str = "jump_first",
             feat: Optional[str] = None, full_nibble: bool = False, constants: Optional[OR.NeuronConstants] = None) -> dict:
    """tests/test_gpu_shape_sweeps._det_case with fc6.weight and fc7.weight (x 3) on a dyadic grid; features N(0, 2) as there"""
    import snn_automotive_object_detection_amd as S
    g = torch.Generator().manual_seed(seed)
    if full_nibble:                                                  # fc6's bin-major order k' = bin * C + c: a nibble is four channels of one bin
        x = full_nibble_values((R, C, 7, 7), T, g)
    else:
        x = _half_grid(torch.randn(R, C, 7, 7, generator=g) * 2, feat)
    torch.manual_seed(seed)
    d = S.FastRCNNPredictorSNNFull(C * 49, Hd, K, T)
    i6: Dict = {}
    i7: Dict = {}
    w6 = _grid(d.fc6.weight.detach().clone(), grid, seed, i6)
    w7 = _grid(d.fc7.weight.detach() * 3.0, grid, seed + 1, i7)
    w_cls, w_bbox = d.cls_score.weight.detach().clone(), d.bbox_pred.weight.detach().clone()
    if grid == "narrow":
        w_cls, w_bbox = _round_bf16(w_cls), _round_bf16(w_bbox)
    counts: List[torch.Tensor] = []
    with torch.no_grad():
        cls, bbox, tr = OR.det_head_forward(x, w6, w7, w_cls, w_bbox, T, li_order=li_order, trace=True, counts_out=counts, constants=constants)
    return dict(kind="det", R=R, C=C, Hd=Hd, K=K, T=T, li_order=li_order, grid=grid, feat=feat, w6=w6, w7=w7, w_cls=w_cls,
                w_bbox=w_bbox, x=x, cls=cls, bbox=bbox, trace=tr, counts=[c.numpy() for c in counts], info6=i6, info7=i7,
                rate6=float(tr["spk6"].mean()), rate7=float(tr["spk7"].mean()), constants=constants)


@functools.lru_cache(maxsize=6)
def gemm_case(M: int, K: int, N: int, seed: int, grid: str = "wide") -> dict:
    """a stage-level spike GEMM: the oracle's encoder spikes of N(0, 2) features at step 6 of 6 (periods 1, 2, 3 and 6 fire: about a third
    of the inputs) against dyadic N(0, 1 / sqrt(K)) weights; `cur` is the oracle's own F.linear"""
    g = torch.Generator().manual_seed(seed)
    z = OR.encoder_spikes(torch.randn(M, K, generator=g) * 2, 6)[5]
    info: Dict = {}
    w = _grid(torch.randn(N, K, generator=g) / K ** 0.5, grid, seed, info)
    with torch.no_grad():
        cur = F.linear(z, w)
    return dict(M=M, K=K, N=N, z=z, w=w, cur=cur, info=info)


# ---- the grid of cases (shared by tests/test_exact_grid_cpu.py, which checks every builder, and tests/test_gpu_exact_grid.py) ------------
PYRAMID = ((13, 17), (6, 7), (2, 1))
LEVEL_SHAPES = (PYRAMID, ((1, 1),), ((1, 63),), ((65, 1),), ((15, 17),), ((33, 31), (1, 1)))
CONV_CHANNELS = (3, 32, 64, 100, 192, 256, 320)
GEMM_SHAPES = ((1, 49, 8), (17, 64 * 49, 128), (65, 32 * 49, 100), (257, 64 * 49, 256), (130, 256, 1024))
RPN_T = (1, 2, 4, 5, 8, 12, 16, 17, 26)
RPN_C_AT_T8 = (3, 100, 192, 320, 512)
DET_T = (1, 2, 3, 6, 8, 12, 14, 16, 17, 24, 32)
DET_R = (1, 15, 16, 17, 33, 64, 65, 257)
DET_C_HD = ((1, 8), (8, 40), (32, 128), (64, 64), (64, 1024), (40, 100), (128, 256))


def rpn_t_case(C, T, grid="wide", li_order="jump_first", constants=None):
    return rpn_case(C, 3, T, PYRAMID, 2, C + T, grid, li_order, constants=constants)


def rpn_shape_case(shapes, N):
    return rpn_case(64, 3, 8, tuple(shapes), N, 70 + N + 10 * len(shapes) + shapes[0][0])


def det_t_case(T, grid="wide", li_order="jump_first", constants=None):
    return det_case(29, 64, 128, 9, T, 200 + T, grid, li_order, constants=constants)


def det_r_case(R, C=32, constants=None):
    return det_case(R, C, 128, 9, 12, 300 + R, constants=constants)


def det_mx_case(grid="wide", constants=None):
    """both widths multiples of 128: what precision "mxfp6" needs"""
    return det_case(37, 128, 256, 9, 12, 530, grid, constants=constants)


def det_width_case(C, Hd):
    return det_case(23, C, Hd, 5, 12, 400 + C + Hd)


def all_cases():
    """every (name, builder) the GPU file runs at default precision on the wide grid, and the narrow / order / full-nibble / feature legs"""
    out = []
    for C in (64, 256):
        out += [("rpn_C%d_T%d" % (C, T), functools.partial(rpn_t_case, C, T)) for T in RPN_T]
    out += [("rpn_C%d_T8" % C, functools.partial(rpn_t_case, C, 8)) for C in RPN_C_AT_T8]
    out += [("rpn_shapes%d_N%d" % (i, N), functools.partial(rpn_shape_case, sh, N)) for i, sh in enumerate(LEVEL_SHAPES) for N in (1, 3)]
    out += [("det_T%d" % T, functools.partial(det_t_case, T)) for T in DET_T]
    out += [("det_R%d_C%d" % (R, C), functools.partial(det_r_case, R, C)) for R in DET_R for C in (32, 64)]
    out += [("det_mx_%s" % g, functools.partial(det_mx_case, g)) for g in ("wide", "narrow")] + [("rpn_mx_narrow", functools.partial(rpn_t_case, 256, 8, "narrow"))]
    out += [("det_C%d_Hd%d" % ch, functools.partial(det_width_case, *ch)) for ch in DET_C_HD]
    out += [("rpn_narrow_T%d" % T, functools.partial(rpn_t_case, 64, T, "narrow")) for T in PRECISION_T_RPN]
    out += [("det_narrow_T%d" % T, functools.partial(det_t_case, T, "narrow")) for T in PRECISION_T_DET]
    out += [("rpn_voltage_first", functools.partial(rpn_t_case, 64, 12, "wide", "voltage_first")),
            ("det_voltage_first", functools.partial(det_t_case, 12, "wide", "voltage_first")),
            ("rpn_full_nibble", rpn_full_nibble_case), ("det_full_nibble", det_full_nibble_case)]
    out += [("rpn_feat_%s" % f, functools.partial(rpn_feat_case, f)) for f in ("fp16", "bf16")]
    out += [("det_feat_%s" % f, functools.partial(det_feat_case, f)) for f in ("fp16", "bf16")]
    return out


# one case per head and T class for the other precisions: RPN dead steps / dense tile (4), 8-wave sparse (5), FAT (8, 16), general
# epilogue on the dense tile (17); detector dense (3), sparse with the register LIF (8, 12), tile image (16), general epilogue (24)
PRECISION_T_RPN = (4, 5, 8, 16, 17)
PRECISION_T_DET = (3, 8, 12, 16, 24)


def rpn_full_nibble_case():
    return rpn_case(256, 3, 8, PYRAMID, 2, 511, full_nibble=True)


def det_full_nibble_case():
    return det_case(29, 64, 128, 9, 12, 512, full_nibble=True)


def rpn_feat_case(feat):
    return rpn_case(64, 3, 8, PYRAMID, 2, 520, feat=feat)


def det_feat_case(feat):
    return det_case(29, 64, 128, 9, 12, 521, feat=feat)


# ---- neuron constants other than the reference's (tests/test_neuron_constants_cpu.py, tests/test_gpu_neuron_constants.py) ----------------
# name -> (constants, route).  Routes: "module" = set p_enc / p_lif / dt on the modules (ops.make_params accepts them); "abi" = the modules
# refuse them (another rest potential or time constant), so the heads run through ops.* with hand-made snn_params.  Groups:
#   zero rest    v_leak = v_reset = 0: period planes and the structured-sparse launches stay in play, the threshold table is rebuilt for
#                the set's (ca, v_th_enc);
#   reset        a reset potential: the op-for-op encoder and the guarded general epilogues, no period planes;
#   abi          rest potentials (0.2 > v_th_lif and v_th_lif = -0.05 < v_leak = 0: every LIF neuron fires at step 0), other time constants;
#   edge         dt = 10 ms: ca = fl32(fl32(0.01) * 100) = 1.0 exactly (fl32(0.01) = 0.00999999977648..., the product 0.999999977648...
#                lies above the midpoint 1 - 2^-25 = 0.99999997019... of the two floats around it and rounds up), outside the threshold
#                table's (0, 1): the recurrence runs.  cb = -2.0: the LIF's synaptic current alternates in sign.
_K = OR.NeuronConstants
NEURON_SETS = {
    "vth_enc_1.0": (_K(v_th_enc=1.0), "module"),
    "vth_enc_0.05": (_K(v_th_enc=0.05), "module"),
    "vth_lif_0.3": (_K(v_th_lif=0.3), "module"),
    "vth_lif_0.02": (_K(v_th_lif=0.02), "module"),
    "dt_2ms": (_K(dt=0.002), "module"),
    "dt_0.5ms": (_K(dt=0.0005), "module"),
    "vreset_-0.05": (_K(v_reset=-0.05), "module"),
    "vreset_0.03": (_K(v_reset=0.03), "module"),
    "vleak_0.05": (_K(v_leak=0.05), "abi"),
    "vleak_-0.1": (_K(v_leak=-0.1), "abi"),
    "vleak_0.2": (_K(v_leak=0.2), "abi"),
    "vleak_0.04_vreset_-0.03": (_K(v_leak=0.04, v_reset=-0.03), "abi"),
    "taus_150_120": (_K(tau_mem_inv=150.0, tau_syn_inv=120.0), "abi"),
    "vth_lif_-0.05": (_K(v_th_lif=-0.05), "abi"),
    "dt_10ms": (_K(dt=0.01), "module"),
}
ZERO_REST_SETS = ("vth_enc_1.0", "vth_enc_0.05", "vth_lif_0.3", "vth_lif_0.02", "dt_2ms", "dt_0.5ms")
EDGE_SETS = ("dt_10ms",)
T_CLASS_SETS = ("vreset_-0.05", "vleak_0.2", "vth_enc_1.0")        # the sets that run every T class and every precision by default


def route_of(k) -> str:
    """the route a set of NEURON_SETS is listed with ("module" for constants that are in no set)"""
    return next((route for kk, route in NEURON_SETS.values() if kk == k), "module")


def is_zero_rest(k) -> bool:
    return k.v_leak == 0.0 and k.v_reset == 0.0


def fires_at_step_0(k) -> bool:
    """an LIF cell starts at v = v_leak, i = 0: v_dec = v_leak + ca * ((v_leak - v_leak) + 0) = v_leak, a spike iff fl32(v_leak - v_th) > 0"""
    return float(np.float32(k.v_leak) - np.float32(k.v_th_lif)) > 0
