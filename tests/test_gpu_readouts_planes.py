"""Any-time readouts against the spike planes of their own pass (include/snn_hip.h: Equality contract).

A readout at T' is a pure function of the hidden spike planes the pass at T = steps[-1] left in the caller's workspace: its outputs and
time sums are the LI recursion on planes[:T'], its counts their popcounts, its rate rows quotients of those.  So everything a readout
pass returns is recomputed on the CPU from the planes read back after that pass - float64 (tests/_planes.py: li_fp64, tied to the oracle
by tests/test_readouts_cpu.py) and integers; no threshold is involved, so there is no flip budget and NO exception is tolerated:

* outputs within CUR_TOL, time sums within T' * CUR_TOL (the bounds of tests/test_gpu_stages.py for one LI head);
* spike counts equal as integers; spike-rate rows equal float32(count / (T' * neurons)) formed in float64;
* LI rate rows within CUR_TOL (a mean of sums divided by T' errs no more than one value); the FLOPs column equals a standalone forward's;
* the prefix property where the header promises it (structured-sparse launches): the planes of a standalone forward at T' ARE the first
  planes of the pass at T, hence its outputs, rates and counts are the readout's, bit for bit.

Dead planes: a LIF layer starts from zero state and sees a current one step after it arrives, so the shared LIF / lif6 cannot fire at
step 0 and lif7 not at steps 0 and 1.  Non-vacuity is therefore asked of every plane with t >= 2 (at least one spike), of every readout
that contains such a plane (T' >= 3: outputs not all zero) and of every pair of readouts the later of which adds such a plane (counts
grow strictly for some image / RoI); the inputs are scaled so that this holds (detector features reach the encoder's first-step
threshold 2.5, fc7 is drawn at 0.12).  Readouts at T' = 1, 2 are checked like all others - against li_fp64 on their (silent) planes."""
import numpy as np
import pytest
import torch

from tests import _planes as PL
from tests._planes import CUR_TOL
from tests._util import planes_to_dense, record_parity

pytestmark = pytest.mark.gpu

RPN_PYRAMID = [(32, 33), (19, 27), (7, 9), (1, 3)]      # 1056 positions: k_count_spikes_ro's gridDim.y = 2 on split planes, 4 on plain rows at C = 256
X_DET = 4.0                                             # detector features rand * 4: some cross 2.5, where the encoder fires at step 0
W7_STD = 0.12                                           # fc7's draw: lif7 fires from step 2 on


def _rnd(w):
    return w.detach().to(torch.bfloat16).to(torch.float32)


def _step_lists(Tmax):
    return (tuple(range(1, Tmax + 1)), (1, Tmax - 1, Tmax))                 # several readout blocks of RB / a sparse list


def _recorded(ops, name, call):
    """run call() with ops.<name> wrapped: (what call() returned, what ops.<name> returned - the raw side outputs of that very pass)"""
    seen = []
    orig = getattr(ops, name)

    def wrapper(*a, **k):
        seen.append(orig(*a, **k))
        return seen[-1]
    setattr(ops, name, wrapper)
    try:
        out = call()
    finally:
        setattr(ops, name, orig)
    assert len(seen) == 1
    return out, seen[0]


def _alive(planes, t0=2):
    """every plane with t >= t0 holds a spike"""
    return all(bool(planes[t].ne(0).any()) for t in range(t0, planes.shape[0]))


def _grows(counts_by_step, steps):
    """counts [n, units]: some unit's count grows strictly over every pair of readouts whose later one adds a plane with t >= 2"""
    pairs = [j for j in range(1, len(steps)) if steps[j] >= 3]
    c = np.asarray(counts_by_step).reshape(len(steps), -1)
    return bool(np.all(c[pairs] > c[[j - 1 for j in pairs]], axis=0).any()) if pairs else True


# ---- RPN -------------------------------------------------------------------------------------------------------------------------------
def rpn_inputs(C_, A, Tmax, N):
    """features randn * 1.7 and weights at the scales of tests/test_gpu_bf16.py; with N = 2 the third level holds ONE image (count and
    rate entries beyond a level's N)"""
    g = torch.Generator().manual_seed(1000 + C_ + 7 * Tmax + N)
    ws = torch.randn(C_, C_, 3, 3, generator=g) * 0.02
    wc = torch.randn(A, C_, 1, 1, generator=g) * 0.05
    wb = torch.randn(4 * A, C_, 1, 1, generator=g) * 0.05
    feats = [torch.randn(1 if (l == 2 and N > 1) else N, C_, h, w, generator=g) * 1.7 for l, (h, w) in enumerate(RPN_PYRAMID)]
    return feats, (ws, wc, wb)


def _rpn_module(pkg, dev, C_, A, T, prec, weights):
    m = pkg.RPNHeadSNN(C_, A, T).to(dev)
    m.precision = prec
    m.load_state_dict({"shared_conv.weight": weights[0], "conv_cls.weight": weights[1], "conv_bbox.weight": weights[2]})
    assert m._resolve_precision() == prec                                    # no fallback to another precision
    return m


def _rows(per_level):
    """what forward returns per level ([N, c, H, W] views) -> position-major rows [P, c] in float64"""
    return np.concatenate([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).double().cpu().numpy() for t in per_level])


def _rpn_flops(m, x, Tp):
    """the "FLOPs" columns of a standalone spike-rate forward at T'"""
    keep = m.num_steps, m.spike_rates
    m.num_steps, m.spike_rates = Tp, True
    cols = [r[:, 1].clone() for r in m(x)[2]]
    m.num_steps, m.spike_rates = keep
    return cols


#             C    A  Tmax precision     N  conv path  split planes   (None: not named by the case)
RPN_GRID = [(256, 3, 12, "bf16x3",     2, 1,    1),          # structured-sparse conv, split planes, resident heads kernel
            (256, 3, 16, "bf16",       2, 1,    None),       # FAT 2 x 2, rounded weights
            (256, 3, 20, "bf16x3",     2, 0,    None),       # dense tile, general epilogue
            (256, 3, 4,  "bf16x3",     2, 0,    None),       # dense tile, T <= 4
            (96,  5, 8,  "bf16x3",     2, 0,    0),          # C % 64 != 0, plain rows, NT = 2
            (64,  3, 12, "f32",        2, None, 0),
            (64,  3, 8,  "f32_strict", 2, None, 0),          # VALU heads, one launch per readout
            (128, 3, 8,  "mxfp6",      2, None, None),
            (256, 3, 12, "bf16x3",     1, 1,    1)]


@pytest.mark.parametrize("C_,A,Tmax,prec,N,want_path,want_split", RPN_GRID, ids=lambda v: str(v))
def test_rpn_readouts_are_functions_of_the_pass_own_planes(gpu_device, C_, A, Tmax, prec, N, want_path, want_split):
    import snn_automotive_object_detection_amd as pkg
    from snn_automotive_object_detection_amd import _lib, ops
    lib = _lib.load()
    feats, weights = rpn_inputs(C_, A, Tmax, N)
    m = _rpn_module(pkg, gpu_device, C_, A, Tmax, prec, weights)
    x = [f.to(gpu_device) for f in feats]
    w_heads = torch.cat([weights[1].flatten(1), weights[2].flatten(1)])
    if prec == "bf16":
        w_heads = _rnd(w_heads)
    a, b = PL.li_constants()
    Cw = (C_ + 31) // 32
    level = []                                                               # (first row, images, H * W) per level
    for f in feats:
        level.append((sum(n * hw for _, n, hw in level), f.shape[0], f.shape[2] * f.shape[3]))
    max_n = max(n for _, n, _ in level)
    flops = {}
    worst_out = worst_sum = 0.0
    for steps in _step_lists(Tmax):
        # 1. outputs, spike rates off
        m.spike_rates = False
        out = m.forward_readouts(x, steps)
        path, split = lib.snn_debug_last_conv_path(), PL.rpn_planes(gpu_device, Tmax, Cw)[1]
        assert want_path is None or path == want_path, (path, want_path)     # a case that runs another launch fails
        assert want_split is None or split == want_split, (split, want_split)
        planes = PL.head_rpn_planes(gpu_device, Tmax, C_)
        assert _alive(planes), "a plane with t >= 2 without a spike"
        last, _ = PL.li_fp64(planes_to_dense(planes, C_), w_heads, a, b, m.li_order)
        assert sorted(out) == list(steps)
        for Tp in steps:
            got = np.concatenate([_rows(out[Tp][0]), _rows(out[Tp][1])], axis=1)
            err = float(np.abs(got - last[Tp - 1]).max())
            print("rpn", C_, prec, Tmax, "T'", Tp, "output error / CUR_TOL %.4f" % (err / CUR_TOL))
            worst_out = max(worst_out, err)
            assert err <= CUR_TOL, (Tp, err)
            assert Tp < 3 or np.abs(got).max() > 1e-3, Tp
        # 2. sums, counts and rate rows of ONE spike-rate pass: the module's finished rows and the raw side outputs behind them
        m.spike_rates = True
        outr, (o_l, o_b, _, (counts, sum_l, sum_b, _)) = _recorded(ops, "rpn_head_forward_readouts", lambda: m.forward_readouts(x, steps))
        assert want_path is None or lib.snn_debug_last_conv_path() == want_path
        planes = PL.head_rpn_planes(gpu_device, Tmax, C_)
        assert _alive(planes)
        last, run = PL.li_fp64(planes_to_dense(planes, C_), w_heads, a, b, m.li_order)
        cum = PL.cumulative_popcounts(planes)                                 # [T, P]
        counts = counts.cpu().numpy()
        assert counts.dtype == np.int64 and counts.shape == (len(steps), len(level), max_n)
        exp_counts = np.zeros_like(counts)
        for l, (r0, n, hw) in enumerate(level):
            exp_counts[:, l, :n] = cum[[t - 1 for t in steps], r0: r0 + n * hw].reshape(len(steps), n, hw).sum(axis=2)
        assert np.array_equal(counts, exp_counts), np.argwhere(counts != exp_counts)[:8]      # (entries beyond a level's N: 0)
        assert _grows(counts, steps)
        for j, Tp in enumerate(steps):
            got = torch.cat([o_l[j], o_b[j]], dim=1).double().cpu().numpy()
            gsum = torch.cat([sum_l[j], sum_b[j]], dim=1).double().cpu().numpy()
            err, serr = float(np.abs(got - last[Tp - 1]).max()), float(np.abs(gsum - run[Tp - 1]).max())
            print("rpn", C_, prec, Tmax, "T'", Tp, "spike-rate pass: output error / CUR_TOL %.4f, sum error / (T' CUR_TOL) %.4f" % (err / CUR_TOL, serr / (Tp * CUR_TOL)))
            worst_out, worst_sum = max(worst_out, err), max(worst_sum, serr / Tp)
            assert err <= CUR_TOL and serr <= Tp * CUR_TOL, (Tp, err, serr)
            if Tp not in flops:
                flops[Tp] = _rpn_flops(m, x, Tp)
            rates = outr[Tp][2]
            assert len(rates) == 3 * len(level)
            for l, (r0, n, hw) in enumerate(level):
                r_spk, r_obj, r_box = (rates[3 * l + k].cpu() for k in range(3))
                assert r_spk.shape == r_obj.shape == r_box.shape == (n, 2) and r_spk.dtype == torch.float32
                exp = (counts[j, l, :n].astype(np.float64) / (Tp * C_ * hw)).astype(np.float32)
                assert np.array_equal(r_spk[:, 0].numpy(), exp), (Tp, l)
                mean = run[Tp - 1, r0: r0 + n * hw].reshape(n, hw, 5 * A) / Tp
                assert np.abs(r_obj[:, 0].double().numpy() - mean[:, :, :A].mean(axis=(1, 2))).max() <= CUR_TOL, (Tp, l)
                assert np.abs(r_box[:, 0].double().numpy() - mean[:, :, A:].mean(axis=(1, 2))).max() <= CUR_TOL, (Tp, l)
                for k, r in enumerate((r_spk, r_obj, r_box)):
                    assert torch.equal(r[:, 1], flops[Tp][3 * l + k].cpu()), (Tp, l, k)
    record_parity("readouts_own_planes", head="rpn", C=C_, A=A, T=Tmax, precision=prec, N=N, max_output_error_in_cur_tol=round(worst_out / CUR_TOL, 4),
                  max_sum_error_in_cur_tol_per_step=round(worst_sum / CUR_TOL, 4))


# ---- detector --------------------------------------------------------------------------------------------------------------------------
def det_inputs(R, K, Tmax, Cc, Hd, feed):
    """weights at the scales of tests/test_gpu_bf16.py but fc7 (W7_STD); rows: x = rand * X_DET; roialign: that file's three-level setup
    (two images, maps rand * X_DET)"""
    g = torch.Generator().manual_seed(2000 + R + 3 * K + 5 * Tmax + (1 if feed == "roialign" else 0))
    w = {"fc6.weight": torch.randn(Hd, Cc * 49, generator=g) * 0.02, "fc7.weight": torch.randn(Hd, Hd, generator=g) * W7_STD,
         "cls_score.weight": torch.randn(K, Hd, generator=g) * 0.05, "bbox_pred.weight": torch.randn(4 * K, Hd, generator=g) * 0.05}
    if feed == "rows":
        return w, (torch.rand(R, Cc, 7, 7, generator=g) * X_DET,)
    feats = [torch.rand(2, Cc, 48 >> l, 64 >> l, generator=g) * X_DET for l in range(3)]
    xy = torch.rand(R, 2, generator=g) * torch.tensor([150.0, 100.0])
    wh = torch.rand(R, 2, generator=g) * 80 + 8
    rois = torch.cat([torch.randint(0, 2, (R, 1), generator=g).float(), xy, xy + wh], dim=1)
    lvl = torch.randint(0, 3, (R,), generator=g).to(torch.int32)
    return w, (feats, [0.25, 0.125, 0.0625], rois, lvl)


def _det_module(pkg, dev, Cc, Hd, K, T, prec, w):
    d = pkg.FastRCNNPredictorSNNFull(Cc * 49, Hd, K, T).to(dev)
    d.precision = prec
    d.load_state_dict(w)
    assert d._resolve_precision() == prec
    return d


def _to_dev(args, dev):
    return tuple([f.to(dev) for f in a] if isinstance(a, list) and isinstance(a[0], torch.Tensor) else (a.to(dev) if isinstance(a, torch.Tensor) else a)
                 for a in args)


def _det_calls(d, feed, args):
    """(forward, forward_readouts, name of the ops entry point behind the readouts) of this feed"""
    if feed == "rows":
        return (lambda: d(*args)), (lambda steps: d.forward_readouts(*args, steps)), "det_head_forward_readouts"
    return (lambda: d.forward_roialign(*args)), (lambda steps: d.forward_roialign_readouts(*args, steps)), "det_head_forward_roialign_readouts"


def _det_flops(d, fwd, Tp):
    keep = d.num_steps, d.spike_rates
    d.num_steps, d.spike_rates = Tp, True
    cols = [r[:, 1].clone() for r in fwd()]
    d.num_steps, d.spike_rates = keep
    return cols


def _check_det(dev, R, K, Tmax, prec, feed, Cc, Hd, want_fc6_path=None):
    """every readout of both step lists from the planes of its own pass; returns the lif6 layout flags (out3[2]) the passes reported"""
    import snn_automotive_object_detection_amd as pkg
    from snn_automotive_object_detection_amd import _lib, ops
    lib = _lib.load()
    w, args = det_inputs(R, K, Tmax, Cc, Hd, feed)
    d = _det_module(pkg, dev, Cc, Hd, K, Tmax, prec, w)
    args = _to_dev(args, dev)
    fwd, readouts, entry = _det_calls(d, feed, args)
    w_heads = torch.cat([w["cls_score.weight"], w["bbox_pred.weight"]])
    if prec == "bf16":
        w_heads = _rnd(w_heads)
    a, b = PL.li_constants()
    flops, layouts = {}, set()
    worst_out = worst_sum = 0.0
    for steps in _step_lists(Tmax):
        d.spike_rates = False
        out = readouts(steps)
        assert want_fc6_path is None or lib.snn_debug_last_fc6_path() == want_fc6_path
        _, p7 = PL.head_det_planes(dev, Tmax, Hd, R)                        # (lif6's last plane is not formed without spike rates)
        assert _alive(p7), "a lif7 plane with t >= 2 without a spike"
        last, _ = PL.li_fp64(planes_to_dense(p7, Hd), w_heads, a, b, d.li_order)
        assert sorted(out) == list(steps)
        for Tp in steps:
            got = torch.cat(list(out[Tp]), dim=1).double().cpu().numpy()
            err = float(np.abs(got - last[Tp - 1]).max())
            print("det", feed, R, K, prec, Tmax, "T'", Tp, "output error / CUR_TOL %.4f" % (err / CUR_TOL))
            worst_out = max(worst_out, err)
            assert got.shape == (R, 5 * K) and err <= CUR_TOL, (Tp, err)
            assert Tp < 3 or np.abs(got).max() > 1e-3, Tp
        d.spike_rates = True
        outr, (o_c, o_b, (c6, c7, s_c, s_b)) = _recorded(ops, entry, lambda: readouts(steps))
        assert want_fc6_path is None or lib.snn_debug_last_fc6_path() == want_fc6_path
        layouts.add(PL.det_planes(dev, Tmax, Hd, R)[2])
        p6, p7 = PL.head_det_planes(dev, Tmax, Hd, R)
        assert _alive(p6) and _alive(p7)
        last, run = PL.li_fp64(planes_to_dense(p7, Hd), w_heads, a, b, d.li_order)
        idx = [t - 1 for t in steps]
        c6, c7 = c6.cpu().numpy(), c7.cpu().numpy()
        assert c6.shape == c7.shape == (len(steps), R) and c6.dtype.kind == "i"
        e6, e7 = PL.cumulative_popcounts(p6)[idx], PL.cumulative_popcounts(p7)[idx]
        assert np.array_equal(c6.astype(np.int64), e6), np.argwhere(c6 != e6)[:8]
        assert np.array_equal(c7.astype(np.int64), e7), np.argwhere(c7 != e7)[:8]
        assert _grows(c6, steps) and _grows(c7, steps)
        for j, Tp in enumerate(steps):
            got = torch.cat([o_c[j], o_b[j]], dim=1).double().cpu().numpy()
            gsum = torch.cat([s_c[j], s_b[j]], dim=1).double().cpu().numpy()
            err, serr = float(np.abs(got - last[Tp - 1]).max()), float(np.abs(gsum - run[Tp - 1]).max())
            print("det", feed, R, K, prec, Tmax, "T'", Tp, "spike-rate pass: output error / CUR_TOL %.4f, sum error / (T' CUR_TOL) %.4f" % (err / CUR_TOL, serr / (Tp * CUR_TOL)))
            worst_out, worst_sum = max(worst_out, err), max(worst_sum, serr / Tp)
            assert err <= CUR_TOL and serr <= Tp * CUR_TOL, (Tp, err, serr)
            if Tp not in flops:
                flops[Tp] = _det_flops(d, fwd, Tp)
            rates = [r.cpu() for r in outr[Tp]]
            assert len(rates) == 4 and all(r.shape == (R, 2) and r.dtype == torch.float32 for r in rates)
            for r, c in ((rates[0], c6[j]), (rates[1], c7[j])):
                assert np.array_equal(r[:, 0].numpy(), (c.astype(np.float64) / (Tp * Hd)).astype(np.float32)), Tp
            mean = run[Tp - 1] / Tp
            assert np.abs(rates[2][:, 0].double().numpy() - mean[:, :K].mean(axis=1)).max() <= CUR_TOL, Tp
            assert np.abs(rates[3][:, 0].double().numpy() - mean[:, K:].mean(axis=1)).max() <= CUR_TOL, Tp
            for k in range(4):
                assert torch.equal(rates[k][:, 1], flops[Tp][k].cpu()), (Tp, k)
    record_parity("readouts_own_planes", head="det", feed=feed, R=R, K=K, T=Tmax, precision=prec, lif6_word_major=sorted(layouts),
                  max_output_error_in_cur_tol=round(worst_out / CUR_TOL, 4), max_sum_error_in_cur_tol_per_step=round(worst_sum / CUR_TOL, 4))
    return layouts


#             R   K  Tmax precision     feed        Cc   Hd   fc6 path
DET_GRID = [(300, 9,  12, "bf16x3",     "rows",     64,  256, 1),       # crosses k_count_rows_ro's 256-thread block, partial tile
            (300, 9,  12, "bf16x3",     "roialign", 64,  256, 1),       # folded encoder
            (17,  9,  16, "bf16",       "roialign", 64,  256, None),
            (1,   9,  24, "bf16x3",     "rows",     64,  256, None),    # two time groups
            (130, 91, 12, "bf16x3",     "rows",     64,  256, None),    # column blocks of 64
            (45,  9,  6,  "f32",        "rows",     64,  256, None),
            (45,  9,  8,  "f32_strict", "rows",     64,  256, None),
            (40,  9,  12, "mxfp6",      "rows",     128, 128, None)]


@pytest.mark.parametrize("R,K,Tmax,prec,feed,Cc,Hd,want_path", DET_GRID, ids=lambda v: str(v))
def test_det_readouts_are_functions_of_the_pass_own_planes(gpu_device, R, K, Tmax, prec, feed, Cc, Hd, want_path):
    _check_det(gpu_device, R, K, Tmax, prec, feed, Cc, Hd, want_path)


def test_det_readouts_on_both_lif6_layouts(gpu_device, monkeypatch):
    """the bf16x3 case again with lif6's planes forced row-major (SNN_PLANES=rm) and word-major (wm): k_count_rows_ro's two layouts"""
    seen = set()
    for planes in ("rm", "wm"):
        monkeypatch.setenv("SNN_PLANES", planes)
        got = _check_det(gpu_device, 300, 9, 12, "bf16x3", "rows", 64, 256)
        assert got == {0 if planes == "rm" else 1}, (planes, got)
        seen |= got
    monkeypatch.delenv("SNN_PLANES")
    seen |= _check_det(gpu_device, 45, 9, 6, "f32", "rows", 64, 256)
    assert seen == {0, 1}


# ---- the prefix property ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
def test_rpn_standalone_forward_is_a_prefix_of_the_pass(gpu_device, prec):
    """C = 256, pass at T = 16 against standalone forwards at T' = 5 .. 15 (all on the structured-sparse conv): same planes, hence the
    same outputs (rates off), rate tensors and spike counts (rates on), bit for bit"""
    import snn_automotive_object_detection_amd as pkg
    from snn_automotive_object_detection_amd import _lib, ops
    lib = _lib.load()
    T, C_, A = 16, 256, 3
    feats, weights = rpn_inputs(C_, A, T, 2)
    m = _rpn_module(pkg, gpu_device, C_, A, T, prec, weights)
    x = [f.to(gpu_device) for f in feats]
    steps = tuple(range(5, T + 1))
    compared = 0
    for rates_on in (False, True):
        m.spike_rates, m.num_steps = rates_on, T
        out, raw = _recorded(ops, "rpn_head_forward_readouts", lambda: m.forward_readouts(x, steps))
        path = lib.snn_debug_last_conv_path()
        planes = PL.head_rpn_planes(gpu_device, T, C_)
        assert path == 1 and _alive(planes)
        for j, Tp in enumerate(steps[:-1]):
            m.num_steps = Tp
            alone = m(x)
            if lib.snn_debug_last_conv_path() != path:
                continue                                                     # another launch family: equal up to threshold ties only
            compared += 1
            mine = PL.head_rpn_planes(gpu_device, Tp, C_)
            if not torch.equal(mine, planes[:Tp]):
                t, p, w = (int(v) for v in (mine != planes[:Tp]).nonzero()[0])
                raise AssertionError("T' = %d: planes differ first at step %d, position %d, word %d (%d words in all)" % (Tp, t, p, w, int((mine != planes[:Tp]).sum())))
            for part_a, part_b in zip(out[Tp], alone):
                assert len(part_a) == len(part_b)
                for u, v in zip(part_a, part_b):
                    assert torch.equal(u, v), (Tp, rates_on)
            if rates_on:
                assert torch.equal(raw[3][0][j], m.last_spike_counts), Tp
    assert compared >= 0.8 * 2 * (len(steps) - 1), compared


@pytest.mark.parametrize("feed", ["rows", "roialign"])
def test_det_standalone_forward_is_a_prefix_of_the_pass(gpu_device, feed):
    """pass at T = 16 against standalone forwards at T' in {6, 8, 12, 14}, fc6 on the structured-sparse launch in both: lif7's planes
    and the lif6 planes the standalone run forms (its last step only in spike-rate mode: the dead time steps of tests/test_gpu_bf16.py)
    are the pass's, hence outputs, rate tensors and counts are the readout's"""
    import snn_automotive_object_detection_amd as pkg
    from snn_automotive_object_detection_amd import _lib, ops
    lib = _lib.load()
    T, R, K, Cc, Hd = 16, 300, 9, 64, 256
    w, args = det_inputs(R, K, T, Cc, Hd, feed)
    d = _det_module(pkg, gpu_device, Cc, Hd, K, T, "bf16x3", w)
    args = _to_dev(args, gpu_device)
    fwd, readouts, entry = _det_calls(d, feed, args)
    steps = (6, 8, 12, 14, 16)
    compared = 0
    for rates_on in (False, True):
        d.spike_rates, d.num_steps = rates_on, T
        out, raw = _recorded(ops, entry, lambda: readouts(steps))
        path = lib.snn_debug_last_fc6_path()
        p6, p7 = PL.head_det_planes(gpu_device, T, Hd, R)
        assert path == 1 and _alive(p7)
        for j, Tp in enumerate(steps[:-1]):
            d.num_steps = Tp
            alone = fwd()
            if lib.snn_debug_last_fc6_path() != path:
                continue
            compared += 1
            q6, q7 = PL.head_det_planes(gpu_device, Tp, Hd, R)
            n6 = Tp if rates_on else Tp - 1
            for name, mine, ref in (("lif6", q6[:n6], p6[:n6]), ("lif7", q7, p7[:Tp])):
                if not torch.equal(mine, ref):
                    t, r, wd = (int(v) for v in (mine != ref).nonzero()[0])
                    raise AssertionError("T' = %d: %s planes differ first at step %d, RoI %d, word %d (%d words in all)" % (Tp, name, t, r, wd, int((mine != ref).sum())))
            assert len(out[Tp]) == len(alone)
            for u, v in zip(out[Tp], alone):
                assert torch.equal(u, v), (Tp, rates_on)
            if rates_on:
                assert torch.equal(raw[2][0][j], d.last_spike_counts[0]) and torch.equal(raw[2][1][j], d.last_spike_counts[1]), Tp
    assert compared >= 0.8 * 2 * (len(steps) - 1), compared
