"""Sentinel neurons: weights and inputs whose outputs are predictable on the host to the last bit (test infrastructure, host only).

Inputs of every LIF layer are spikes in {0, 1}.  A neuron whose weight row has exactly ONE nonzero entry w therefore receives the
current w or 0 - in any summation order, on any instruction, whatever the other inputs hold.  For bf16x3 this needs
hi + mid + lo == w with exact partial sums, which holds for every fp32 weight the modules do not send to "f32_strict".  Given identical
currents the fused LIF epilogues repeat the oracle's fp32 operations in the same order (csrc/snn_common.h: lif_step; the sparse kernels'
sp_lif_*), so such a neuron's spike train is predicted here BIT FOR BIT by the fp32 step functions below (copied op for op from
oracle/norse_restated.py).

Boundary pairs make the trains sensitive to the last bit of a weight: two adjacent floats a < b = nextafter(a) whose trains differ for
the input schedule the sentinel sees sit on two neighbouring output channels.  A current wrong by one ulp changes one of the two trains.
The trains are read through the LI heads: every head output is itself a sentinel (one-hot row on one hidden sentinel), whose value
mem_T = sum over the spikes t of kappa_t * u is compared with an fp64 evaluation of the LI recursion (head_tolerance below).

Builders return a dict with the module weights (fp32 CPU tensors), the inputs, the expected hidden trains and the expected outputs
(fp64) with their per-element tolerances.  Everything is deterministic in the builder's arguments.
"""
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

F32 = np.float32

# ---- fp32 constants exactly as the oracle forms them: (dt * tau_inv) is a 0-dim fp32 tensor product (oracle/norse_restated.py) -----
DT = 0.001
CA = F32((DT * torch.as_tensor(1.0 / 1e-2)).item())            # dt * tau_mem_inv
CB = F32((-DT * torch.as_tensor(1.0 / 5e-3)).item())           # -dt * tau_syn_inv
V_TH_ENC = F32(torch.tensor(0.25).item())
V_TH_LIF = F32(torch.tensor(0.1).item())
ZERO = F32(0.0)


def encoder_train(x: float, T: int) -> np.ndarray:
    """lif_current_encoder (norse_restated.py) on a constant input, fp32 op for op -> bool [T]"""
    x = F32(x)
    v = ZERO
    out = np.zeros(T, dtype=bool)
    for t in range(T):
        dv = F32(CA * F32(F32(ZERO - v) + x))
        v = F32(v + dv)
        z = F32(v - V_TH_ENC) > 0
        v = F32(v - F32(F32(z) * F32(v - ZERO)))
        out[t] = z
    return out


def lif_train(w: float, sched: np.ndarray) -> np.ndarray:
    """lif_feed_forward_step (norse_restated.py) with the current w at the steps where sched is set (0 elsewhere) -> bool [T]"""
    w = F32(w)
    v = i = ZERO
    out = np.zeros(len(sched), dtype=bool)
    for t, s in enumerate(sched):
        dv = F32(CA * F32(F32(ZERO - v) + i))
        v_dec = F32(v + dv)
        di = F32(CB * i)
        i_dec = F32(i + di)
        z = F32(v_dec - V_TH_LIF) > 0
        v = F32(F32(F32(1.0 - F32(z)) * v_dec) + F32(F32(z) * ZERO))
        i = F32(i_dec + (w if s else ZERO))
        out[t] = z
    return out


def li_last64(u: float, train: np.ndarray, li_order: str = "jump_first") -> Tuple[float, float]:
    """fp64 LI recursion (li_feed_forward_step semantics, the fp32 constants CA / CB) fed u at the spikes of `train`:
    (last membrane, sum of the membranes over t)"""
    a, cb, u = float(CA), float(CB), float(u)
    v = i = acc = 0.0
    for s in train:
        x = u if s else 0.0
        if li_order == "jump_first":
            i = i + x
            v = v + a * ((0.0 - v) + i)
            i = i + cb * i
        else:
            v = v + a * ((0.0 - v) + i)
            i = i + cb * i + x
        acc += v
    return v, acc


def kappa64(T: int, li_order: str = "jump_first") -> np.ndarray:
    """kappa_t: the last membrane of the fp64 LI after a unit current at step t alone"""
    return np.array([li_last64(1.0, np.arange(T) == t, li_order)[0] for t in range(T)])


# ---- head tolerance ---------------------------------------------------------------------------------------------------------------
# The LI heads compute mem_T = sum_t kappa32[t] * (spk_t . U) (csrc/snn_heads.h K5 / K5b / K5c), kappa32 = fp32(kappa64) (li_kappa,
# csrc/snn_post.h).  For a head sentinel spk_t . U is exactly u or 0, so with n spikes at steps t_1 .. t_n the kernels evaluate
#     fma / add chain of the n products kappa32[t_j] * u      (VALU form: an exact fma sum of the kappas, then one product)
# Each kappa32 carries a relative error <= 2^-24 and each of the <= n + 1 roundings an error <= 2^-24 of a partial result, and every
# partial is <= S = sum_j kappa64[t_j] |u| (all kappa > 0).  Hence |got - exact| <= (2 n + 2) 2^-24 S.  The fp32 oracle recursion
# (T rounded steps) is not bound by this - it is compared on the trains only; its outputs are checked against the same bound
# with the factor T + 2n + 2 (oracle_tolerance).  One ulp of x is >= 2^-24 |x|, so for one spike the bound is <= 4 ulps of the result.
# A dropped / doubled lo plane moves u by |lo| >= 2^-18 |u| (design_head_weight), i.e. the output by >= 64 x 2^-24 S: the bound stays
# <= a quarter of that for n <= 7 spikes (head sentinels fire once or twice; tests/test_sentinels_cpu.py asserts it per case).
U = 2.0 ** -24


def head_tolerance(n_spikes: int, s_abs: float) -> float:
    return (2 * n_spikes + 2) * U * s_abs


def oracle_tolerance(n_spikes: int, s_abs: float, T: int) -> float:
    return (T + 2 * n_spikes + 2) * U * s_abs


def ulps(err: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """|err| in units of ulp(ref) (fp32); 0 where both are zero"""
    ref = np.abs(np.asarray(ref, dtype=np.float64))
    e = np.floor(np.log2(np.where(ref > 0, ref, 1.0)))
    ulp = np.where(ref > 0, 2.0 ** (e - 23), 2.0 ** -149)
    return np.abs(err) / ulp


# ---- bf16x3 planes ----------------------------------------------------------------------------------------------------------------
def _bf16_rn(x: np.ndarray) -> np.ndarray:
    b = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b >> 16) & 1) + 0x7FFF
    return ((b + r) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def split3(w) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """w -> (hi, mid, lo) bf16 values (as fp32) with the kernels' f2bf_rn split: hi = rn(w), mid = rn(w - hi), lo = rn(w - hi - mid)"""
    w = np.asarray(w, dtype=np.float32)
    hi = _bf16_rn(w)
    r1 = (w - hi).astype(np.float32)
    mid = _bf16_rn(r1)
    lo = _bf16_rn((r1 - mid).astype(np.float32))
    return hi, mid, lo


def next_up(a: float) -> float:
    return float(np.nextafter(F32(a), F32(np.inf)))


def _fbits(x: float) -> int:
    return int(np.array(x, dtype=np.float32).view(np.uint32))


def _bitsf(b: int) -> float:
    return float(np.array(b, dtype=np.uint32).view(np.float32))


def boundaries(sched: np.ndarray, w_lo: float = 0.02, w_hi: float = 1.5, probes: int = 96) -> List[float]:
    """fp32 weights a in (w_lo, w_hi) with lif_train(a) != lif_train(nextafter(a)): bisection over the fp32 bit patterns between
    `probes` log-spaced probes (boundaries closer together than the probe spacing can be missed; the builders need only some)"""
    pts = sorted({_fbits(float(x)) for x in np.geomspace(w_lo, w_hi, probes)})
    trains = {b: lif_train(_bitsf(b), sched) for b in pts}
    out = []

    def rec(lo, hi):
        if np.array_equal(trains[lo], trains[hi]):
            return
        if hi - lo == 1:
            out.append(_bitsf(lo))
            return
        mid = (lo + hi) // 2
        trains[mid] = lif_train(_bitsf(mid), sched)
        rec(lo, mid)
        rec(mid, hi)
    for lo, hi in zip(pts[:-1], pts[1:]):
        rec(lo, hi)
    return out


def sensitive_pairs(sched: np.ndarray, **kw) -> List[float]:
    key = (np.asarray(sched, dtype=bool).tobytes(), tuple(sorted(kw.items())))
    if key not in _PAIRS:
        _PAIRS[key] = _sensitive_pairs(np.asarray(sched, dtype=bool), **kw)
    return _PAIRS[key]


_PAIRS: Dict[tuple, List[float]] = {}


def _sensitive_pairs(sched: np.ndarray, **kw) -> List[float]:
    """boundaries a whose pair (a, b = nextafter(a)) catches every weight mutant of MUTANTS: for each, the train of the mutated a or
    of the mutated b differs from the true one"""
    keep = []
    for a in boundaries(sched, **kw):
        ab = np.array([a, next_up(a)], dtype=np.float32)
        true = [lif_train(x, sched) for x in ab]
        if all(any(not np.array_equal(lif_train(x, sched), t) for x, t in zip(mutate_np(ab, how), true)) for how in MUTANTS):
            keep.append(a)
    return keep


def robust_weight(sched: np.ndarray, n_spikes: Sequence[int] = (1, 2)) -> float:
    """a weight in the middle of a train interval whose train has 1 (else 2) spikes: far from every boundary"""
    bs = boundaries(sched, 0.005, 4.0, 160)
    edges = [0.005] + bs + [4.0]
    for n in n_spikes:
        for lo, hi in zip(edges[:-1], edges[1:]):
            w = float(F32(0.5 * (lo + hi)))
            if int(lif_train(w, sched).sum()) == n and (hi - lo) > 1e-3 * w:
                return w
    raise ValueError("no weight gives %s spikes for this schedule" % (n_spikes,))


def design_head_weight(rng: np.random.Generator, scale: float = 0.05) -> float:
    """a weight with large mid and lo planes: |mid| >= 2^-10 |u|, |lo| >= 2^-18 |u| (then dropping lo moves the output by >= 64
    units of 2^-24 |output|)"""
    while True:
        u = F32(rng.normal() * scale)
        _, m, l = split3(np.array([u]))
        if abs(m[0]) >= 2.0 ** -10 * abs(u) and abs(l[0]) >= 2.0 ** -18 * abs(u) and abs(u) > 1e-3:
            return float(u)


# ---- encoder periods ----------------------------------------------------------------------------------------------------------------
def _first_spike(x: float, T: int = 40) -> int:
    tr = encoder_train(x, T)
    return int(np.argmax(tr)) if tr.any() else T


_PERIOD_X: Dict[int, float] = {}


def period_input(p: int) -> float:
    """a constant input in the middle of the fp32 interval whose encoder fires every p steps (first spike at step p - 1)"""
    if p in _PERIOD_X:
        return _PERIOD_X[p]

    def lowest(q):            # smallest float with first spike at or before step q - 1
        lo, hi = _fbits(0.25), _fbits(64.0)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if _first_spike(_bitsf(mid)) <= q - 1:
                hi = mid
            else:
                lo = mid
        return _bitsf(hi)
    top = 2.0 * lowest(1) if p == 1 else lowest(p - 1)
    x = float(F32(0.5 * (lowest(p) + top)))
    tr = encoder_train(x, 3 * p + 2)
    assert tr[p - 1] and tr.sum() == (3 * p + 2) // p and not tr[:p - 1].any(), p
    _PERIOD_X[p] = x
    return x


def period_sched(p: int, T: int) -> np.ndarray:
    return encoder_train(period_input(p), T)


# ---- placement ----------------------------------------------------------------------------------------------------------------------
def _spread(n: int, size: int, pairs: int) -> List[int]:
    """n channel indices (the first 2 * pairs as neighbouring pairs) over the first, middle and last 16-wide tile and every lane
    residue mod 16 (as far as n and size allow), all distinct"""
    tiles = max(1, size // 16)
    tile_order = [0, tiles // 2, tiles - 1]
    out, used = [], set()
    for k in range(n):
        pair_k, second = (k // 2, k % 2) if k < 2 * pairs else (k - pairs, 0)
        if second:
            c = out[-1] + 1
        else:
            c = (tile_order[pair_k % 3] * 16 + (2 * pair_k + (k >= 2 * pairs)) % 16) % size
            while c in used or (k < 2 * pairs and (c + 1 in used or c + 1 >= size)):
                c = (c + 3) % size
        out.append(c)
        used.add(c)
    return out


def _input_channels(n: int, C: int) -> List[int]:
    """n input channels covering every bit of a nibble and both word parities of a 64-channel step; distinct while n <= C"""
    out, used = [], set()
    for k in range(n):
        c = (32 * (k % max(1, C // 32)) + 5 * (k // 4) * 4 + k % 4) % C
        while c in used and len(used) < C:
            c = (c + 1) % C
        out.append(c)
        used.add(c)
    return out


def _pair_period(k: int, T: int) -> int:
    """the k-th period of PERIODS (cyclic) for a boundary pair, or the next shorter one whose schedule has sensitive pairs at T"""
    i = k % len(PERIODS)
    while not sensitive_pairs(period_sched(PERIODS[i], T)):
        i -= 1
    return PERIODS[i]


# ---- RPN --------------------------------------------------------------------------------------------------------------------------
PERIODS = (1, 2, 3, 4, 5, 7)


def rpn_case(C: int, A: int, T: int, shapes: Sequence[Tuple[int, int]], N: int = 2, seed: int = 0, li_order: str = "jump_first",
             all_sentinel: bool = False) -> dict:
    """RPNHeadSNN(C, A, T) weights + feature pyramid.  Every head output (A cls + 4A bbox) is a sentinel reading one hidden sentinel
    channel; hidden sentinels sit among random dense channels (or, all_sentinel=True, every hidden row is one-hot too and every input
    channel constant: the whole output and the spike counts are predictable).

    Returns dict(w_shared, w_cls, w_bbox, feats [list of N,C,H,W], hidden [list of (channel, input channel, tap, weight, train)],
    heads [list of (output, hidden index, u)], exp (list per level of [N, 5A, H, W] fp64: cls then bbox), tol (same shapes),
    counts (all_sentinel: int64 [levels, N]), pairs (hidden indices of boundary pairs))"""
    rng = np.random.default_rng([seed, C, A, T, int(all_sentinel), 1])
    n_out = 5 * A
    n_head_only = max(1, n_out % 2 + 2)                 # outputs reading a 1-2-spike hidden sentinel; the rest read boundary pairs
    n_pairs = (n_out - n_head_only) // 2
    n_head_only = n_out - 2 * n_pairs
    hid = _spread(n_out, C, n_pairs)
    cin = _input_channels(n_pairs + n_head_only, C)
    w_shared = (rng.normal(size=(C, C, 3, 3)) * 0.04).astype(np.float32)
    hidden = []
    for k in range(n_pairs + n_head_only):
        period = _pair_period(k, T) if k < n_pairs else PERIODS[(k + 1) % 4]
        sched = period_sched(period, T)
        tap = k % 9
        if k < n_pairs:
            cands = sensitive_pairs(sched)
            a = cands[int(rng.integers(len(cands)))]
            ws = [(hid[2 * k], a), (hid[2 * k + 1], next_up(a))]
        else:
            ws = [(hid[2 * n_pairs + (k - n_pairs)], robust_weight(sched))]
        for h, w in ws:
            hidden.append(dict(channel=h, cin=cin[k], tap=tap, weight=w, period=period, train=lif_train(w, sched), pair=k < n_pairs))
    in_val = {}
    for hd in hidden:
        in_val[hd["cin"]] = period_input(hd["period"])
    if all_sentinel:
        used = {hd["channel"] for hd in hidden}
        free_in = [c for c in range(C) if c not in in_val]
        for c in free_in:
            in_val[c] = period_input(int(rng.integers(1, T + 2)))
        for h in range(C):
            if h in used:
                continue
            c = int(rng.integers(C))
            p = _first_spike(in_val[c]) + 1
            sched = encoder_train(in_val[c], T)
            w = float(F32(rng.uniform(0.03, 1.2)))
            hidden.append(dict(channel=h, cin=c, tap=int(rng.integers(9)), weight=w, period=p, train=lif_train(w, sched), pair=False))
    for hd in hidden:
        w_shared[hd["channel"]] = 0.0
        w_shared[hd["channel"], hd["cin"], hd["tap"] // 3, hd["tap"] % 3] = hd["weight"]
    w_head = np.zeros((n_out, C), dtype=np.float32) if all_sentinel else (rng.normal(size=(n_out, C)) * 0.01).astype(np.float32)
    heads = []
    for o in range(n_out):
        u = design_head_weight(rng)
        w_head[o] = 0.0
        w_head[o, hidden[o]["channel"]] = u
        heads.append(dict(output=o, hidden=o, u=u))
    # features: N(0, 1.7) with the sentinel input channels constant
    g = torch.Generator().manual_seed(int(rng.integers(1 << 31)))
    feats = []
    for (H, W) in shapes:
        f = torch.randn(N, C, H, W, generator=g) * 1.7
        for c, x in in_val.items():
            f[:, c] = x
        feats.append(f)
    kap_last = kappa64(T, li_order)
    exp, tol, otol = [], [], []
    counts = np.zeros((len(shapes), N), dtype=np.int64)
    for l, (H, W) in enumerate(shapes):
        e = np.zeros((N, n_out, H, W))
        t_ = np.zeros((N, n_out, H, W))
        ot = np.zeros((N, n_out, H, W))
        for o, hd in enumerate(heads):
            hs = hidden[hd["hidden"]]
            m = _tap_inside(H, W, hs["tap"])
            val = li_last64(hd["u"], hs["train"], li_order)[0]
            n = int(hs["train"].sum())
            s_abs = float(np.sum(kap_last[hs["train"]])) * abs(hd["u"])
            e[:, o] = np.where(m, val, 0.0)
            t_[:, o] = np.where(m, head_tolerance(n, s_abs), 0.0)
            ot[:, o] = np.where(m, oracle_tolerance(n, s_abs, T), 0.0)
        if all_sentinel:
            counts[l, :] = sum(int(_tap_inside(H, W, hs["tap"]).sum()) * int(hs["train"].sum()) for hs in hidden)
        exp.append(e); tol.append(t_); otol.append(ot)
    w_cls = torch.from_numpy(w_head[:A].copy()).view(A, C, 1, 1)
    w_bbox = torch.from_numpy(w_head[A:].copy()).view(4 * A, C, 1, 1)
    return dict(kind="rpn", C=C, A=A, T=T, N=N, shapes=list(shapes), li_order=li_order, w_shared=torch.from_numpy(w_shared),
                w_cls=w_cls, w_bbox=w_bbox, feats=feats, hidden=hidden, heads=heads, exp=exp, tol=tol, oracle_tol=otol,
                counts=counts if all_sentinel else None)


def _tap_inside(H: int, W: int, tap: int) -> np.ndarray:
    """[H, W]: positions whose 3x3 tap (row-major index) reads inside the map (padding 1)"""
    dy, dx = tap // 3 - 1, tap % 3 - 1
    ys, xs = np.arange(H)[:, None] + dy, np.arange(W)[None, :] + dx
    return (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)


def rpn_outputs(logits, bbox) -> List[np.ndarray]:
    """module / oracle outputs -> per level [N, 5A, H, W] fp64 (cls channels, then bbox)"""
    return [np.concatenate([np.asarray(a.detach().cpu(), dtype=np.float64), np.asarray(b.detach().cpu(), dtype=np.float64)], axis=1)
            for a, b in zip(logits, bbox)]


# ---- detector ------------------------------------------------------------------------------------------------------------------------
def det_case(C: int, Hd: int, K: int, T: int, R: int, seed: int = 0, li_order: str = "jump_first") -> dict:
    """FastRCNNPredictorSNNFull(C * 49, Hd, K, T) weights + RoI features [R, C, 7, 7].  Chains of sentinels: a constant input feature
    -> an fc6 sentinel -> an fc7 sentinel -> one cls / bbox output each.  Boundary pairs sit in fc6 (read by fc7 followers, weight
    FOLLOW_W) and in fc7 (reading a robust fc6 sentinel); the remaining outputs read 1-2-spike fc7 sentinels.  All other fc6 / fc7 rows
    are random and dense.  Returns dict(w6, w7, w_cls, w_bbox, x, chains, exp [R, 5K], tol, oracle_tol, feature_values {d: x})"""
    rng = np.random.default_rng([seed, C, Hd, K, T, R, 2])
    D = C * 49
    n_out = 5 * K
    n6_pairs = max(1, n_out // 6)
    n7_pairs = max(1, n_out // 6)
    n_single = n_out - 2 * n6_pairs - 2 * n7_pairs
    assert n_single >= 1
    w6 = (rng.normal(size=(Hd, D)) * 0.02).astype(np.float32)
    w7 = (rng.normal(size=(Hd, Hd)) * 0.06).astype(np.float32)
    n6 = 2 * n6_pairs + n7_pairs + n_single
    h6 = _spread(n6, Hd, n6_pairs)
    h7 = _spread(n_out, Hd, n6_pairs + n7_pairs)
    feat_ch = _input_channels(n6_pairs + n7_pairs + n_single, C)
    fvals, chains, u6 = {}, [], []
    k6 = 0
    # fc6 units: n6_pairs boundary pairs, then robust units (for the fc7 pairs and the 1-2-spike chains)
    units6 = []
    for k in range(n6_pairs + n7_pairs + n_single):
        period = _pair_period(k, T) if k < n6_pairs else PERIODS[k % 4]
        d = feat_ch[k] * 49 + (7 * k) % 49
        fvals[d] = period_input(period)
        sched = period_sched(period, T)
        if k < n6_pairs:
            a = sensitive_pairs(sched)
            a = a[int(rng.integers(len(a)))]
            for w in (a, next_up(a)):
                units6.append(dict(unit=h6[len(units6)], d=d, weight=w, train=lif_train(w, sched), pair=True))
        else:
            w = float(F32(rng.uniform(0.3, 1.0)))
            units6.append(dict(unit=h6[len(units6)], d=d, weight=w, train=lif_train(w, sched), pair=False))
    for u in units6:
        w6[u["unit"]] = 0.0
        w6[u["unit"], u["d"]] = u["weight"]
    units7 = []
    for u in units6[:2 * n6_pairs]:                     # followers of the fc6 pairs
        units7.append(dict(src=u, weight=FOLLOW_W, kind="follow6"))
    rest = units6[2 * n6_pairs:]
    rest = sorted(rest, key=lambda u: -len(sensitive_pairs(u["train"])))     # (fc7 pairs on the fc6 trains that give most choice)
    for j in range(n7_pairs):
        src = rest[j]
        cands = sensitive_pairs(src["train"])
        if not cands:
            raise ValueError("fc6 train without a sensitive fc7 boundary")
        a = cands[int(rng.integers(len(cands)))]
        units7 += [dict(src=src, weight=a, kind="pair7"), dict(src=src, weight=next_up(a), kind="pair7")]
    srcs = [u for u in rest[n7_pairs:] if u["train"][:-3].any()] or [u for u in units6 if u["train"][:-3].any()]
    for j in range(n_single):
        src = srcs[j % len(srcs)]                         # (an fc6 train with a spike early enough for one in fc7)
        units7.append(dict(src=src, weight=robust_weight(src["train"]), kind="single"))
    for o, u in enumerate(units7):
        u["unit"] = h7[o]
        u["train"] = lif_train(u["weight"], u["src"]["train"])
        w7[u["unit"]] = 0.0
        w7[u["unit"], u["src"]["unit"]] = u["weight"]
    w_head = np.zeros((n_out, Hd), dtype=np.float32)
    heads = []
    for o, u in enumerate(units7):
        uu = design_head_weight(rng)
        w_head[o, u["unit"]] = uu
        heads.append(dict(output=o, u=uu, src=u))
    g = torch.Generator().manual_seed(int(rng.integers(1 << 31)))
    x = torch.randn(R, D, generator=g) * 1.7
    for d, v in fvals.items():
        x[:, d] = v
    kap = kappa64(T, li_order)
    exp, tol, otol = np.zeros(n_out), np.zeros(n_out), np.zeros(n_out)
    for o, hd in enumerate(heads):
        tr = hd["src"]["train"]
        n = int(tr.sum())
        s_abs = float(np.sum(kap[tr])) * abs(hd["u"])
        exp[o] = li_last64(hd["u"], tr, li_order)[0]
        tol[o] = head_tolerance(n, s_abs)
        otol[o] = oracle_tolerance(n, s_abs, T)
    return dict(kind="det", C=C, Hd=Hd, K=K, T=T, R=R, li_order=li_order, w6=torch.from_numpy(w6), w7=torch.from_numpy(w7),
                w_cls=torch.from_numpy(w_head[:K].copy()), w_bbox=torch.from_numpy(w_head[K:].copy()),
                x=x.view(R, C, 7, 7), units6=units6, units7=units7, heads=heads, feature_values=fvals,
                exp=np.broadcast_to(exp, (R, n_out)), tol=np.broadcast_to(tol, (R, n_out)),
                oracle_tol=np.broadcast_to(otol, (R, n_out)))


FOLLOW_W = 0.7      # an fc7 follower of an fc6 pair: large enough that every fc6 spike moves the fc7 train


def det_outputs(cls, bbox) -> np.ndarray:
    return np.concatenate([np.asarray(cls.detach().cpu(), dtype=np.float64), np.asarray(bbox.detach().cpu(), dtype=np.float64)], axis=1)


# ---- the assertion (shared by the GPU tests and the CPU sensitivity test) ---------------------------------------------------------
def check(got: np.ndarray, exp: np.ndarray, tol: np.ndarray) -> Tuple[int, float]:
    """(number of elements outside their bound, largest error in ulps of the expected value).  Where the expected value is 0 (no
    spike reached the head) the output must be exactly 0."""
    got, exp, tol = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64), np.asarray(tol, dtype=np.float64)
    err = np.abs(got - exp)
    bad = int(np.sum(err > tol)) + int(np.sum(~np.isfinite(got)))
    return bad, float(np.max(ulps(err, exp), initial=0.0))


def check_levels(got: List[np.ndarray], case: dict, key: str = "tol") -> Tuple[int, float]:
    bad, mx = 0, 0.0
    for g, e, t in zip(got, case["exp"], case[key]):
        b, m = check(g, e, t)
        bad, mx = bad + b, max(mx, m)
    return bad, mx


# ---- host-only weight mutants (what a kernel that mishandles a plane would compute) -----------------------------------------------
def mutate_np(a: np.ndarray, how: str) -> np.ndarray:
    a = np.asarray(a, dtype=np.float32)
    hi, mid, lo = split3(a)
    f = {"hi_only": lambda: hi,
         "hi_mid": lambda: hi + mid,
         "no_mid": lambda: hi + lo,
         "lo_doubled": lambda: (hi + mid) + 2 * lo,
         "bf16": lambda: _bf16_rn(a),
         "ulp_up": lambda: np.where(a != 0, np.nextafter(a, np.float32(np.inf)), a),
         "ulp_down": lambda: np.where(a != 0, np.nextafter(a, np.float32(-np.inf)), a)}[how]
    return np.ascontiguousarray(f(), dtype=np.float32)


def mutate(w: torch.Tensor, how: str) -> torch.Tensor:
    return torch.from_numpy(mutate_np(w.detach().cpu().numpy(), how))


MUTANTS = ("hi_only", "hi_mid", "no_mid", "lo_doubled", "bf16", "ulp_up", "ulp_down")
