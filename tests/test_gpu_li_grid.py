"""The LI heads on dyadic neuron constants and gridded head weights (tests/_li_grid.py): the zero-tolerance gate for the kernel family of
csrc/snn_heads.h and its launcher.

On these cases every partial sum of sum_t kappa_t * (spk_t . W) is exact in fp32 in every order (tests/test_li_grid_cpu.py proves the
expectation side and that the bit budget is not vacuous), so every output and every time sum of every kernel form is compared with
torch.equal against the integer expectation - which is the fp64 recursion of tests/_planes.li_fp64 and the fp32 oracle, bit for bit.
Every output buffer is filled with NaN before the call.  A difference is a wrong term (a kappa from the wrong step, order or readout, a
dropped plane or word, a column block reading its neighbour's weights), not a rounding: there is none.  No tolerance appears below; the
finished rate rows, which divide by T, are left to tests/test_gpu_readouts_planes.py.

What reaches what (the launcher's plan as restated by tests/_li_grid.li_plan; ids are those of tests/_li_grid.stage_grid / head_grid):

  k_li_heads<RB> (fp32 VALU)        RB = 64 K32_N15 / 32 M* / 16 K1024_N45 / 8 N24_96 / 4 N91_364 (256 + 208 columns), all under SNN_LI_HEADS=valu;
                                    whole heads at precision "f32_strict"
  k_li_heads_mfma<NT>, W resident   NT = 1 K256_N15 (Kw = 8 line loads) and K32_N15 / 2 M*, N5_20 / 3 N9_36 / 4 N11_44, wide_pm1_T8_17x128x120
  k_li_heads_mfma<NT>, W streamed   NT = 1 K2048_N15 / 3 K1024_N45, both under SNN_LI_HEADS=mfma
  k_li_heads_ksplit<NT>             NT = 3 K1024_N45 and every T*_17x1024x45 by default (W does not fit); NT = 1, 2, 4 under SNN_LI_HEADS=ksplit
                                    (T*_17x1024x10, M*, N11_44); whole detector head at Hd = 1024, K = 9 by default
  64-column blocks (col0 > 0)       N24_96 (two blocks), N91_364 (seven blocks + a 16-column remainder)
  time groups                       T*_83x256x15 and T*_17x1024x*: groups of 8 / 16 / 12 with last groups of 1, 2, 4, 8 (T = 1 .. 16 dyadic, 17 .. 32 on +-1)
  k_li_heads_mfma_ro / _ksplit_ro   ro_*: every T' of 1 .. 12 and 1 .. 11 (a remainder block for RB = 8, 4 and 2), a sparse list, single readouts,
                                    1 .. 26 on +-1; resident (83x256x15, 17x128x25, 33x256x120), streamed and ksplit (17x1024x45)
  half_split planes                 rpn_C256_T8 / T12 / T16 (structured-sparse conv) and T4 (dense conv) at C = 256 -> resident heads kernel; rpn_readouts
  both LI orders                    K*_jump_first / K*_voltage_first, T*_voltage_first, rpn_voltage_first, det_voltage_first
  sums on and off                   every stage case runs both; whole heads with and without spike rates
  lo / mid planes of lih_split3     wide_* (planted 18-bit weights), rpn_wide, det_pm1_wide
  plane stride                      test_plane_stride_beyond_the_planes_is_honoured"""
import ctypes as Ct

import numpy as np
import pytest
import torch

from tests import _li_grid as L
from tests import _neuron_constants as NC
from tests import _planes as PL
from tests._util import dense_to_planes, planes_to_dense

pytestmark = pytest.mark.gpu

STAGE = dict(L.stage_grid())


@pytest.fixture(scope="module")
def ops():
    from snn_automotive_object_detection_amd import ops
    return ops


def _lib():
    from snn_automotive_object_detection_amd import _lib
    return _lib.load()


def _set_form(monkeypatch, form):
    if form is None:
        monkeypatch.delenv("SNN_LI_HEADS", raising=False)
    else:
        monkeypatch.setenv("SNN_LI_HEADS", form)      # a form that does not apply to the shape falls through to the VALU kernel


# ---- stage level -------------------------------------------------------------------------------------------------------------------------
def _call(planes, K, wh, NA, NB, p, steps=None, want_sums=False, stride=None):
    """snn_li_heads / snn_li_heads_readouts as ops.li_heads / ops.li_heads_readouts call them, argument for argument, but into buffers
    filled with NaN: (out_a, out_b, sum_a, sum_b), each with a leading readout axis if `steps`"""
    from snn_automotive_object_detection_amd import _lib
    from snn_automotive_object_detection_amd.ops import _ptr, _stream
    T, M, Kw = planes.shape[0], planes.shape[1], (K + 31) // 32
    lead = () if steps is None else (len(steps),)

    def buf(c):
        return torch.full(lead + (M, c), float("nan"), dtype=torch.float32, device=planes.device)
    out_a, out_b = buf(NA), buf(NB)
    sum_a, sum_b = (buf(NA), buf(NB)) if want_sums else (None, None)
    stride = M * Kw if stride is None else stride
    tail = (M, K, _ptr(wh), NA, NB, Ct.byref(p), _ptr(out_a), _ptr(out_b), _ptr(sum_a), _ptr(sum_b), _stream())
    if steps is None:
        _lib.check(_lib.load().snn_li_heads(_ptr(planes), stride, T, *tail), "snn_li_heads")
    else:
        st = (Ct.c_int * len(steps))(*steps)
        _lib.check(_lib.load().snn_li_heads_readouts(_ptr(planes), stride, st, len(steps), *tail), "snn_li_heads_readouts")
    return out_a, out_b, sum_a, sum_b


def _expected(case, dev):
    """(last, sum or None) as [n, M, NA + NB] fp32 on the device"""
    return torch.from_numpy(case["last"]).to(dev), (torch.from_numpy(case["sum"]).to(dev) if case["sums"] else None)


def _same(got_a, got_b, exp, what):
    got = torch.cat([got_a, got_b], dim=-1)
    if not torch.equal(got, exp):
        bad = (got != exp) | torch.isnan(got)
        raise AssertionError("%s: %d of %d outputs differ (first at %s: got %r, expected %r)" % (
            what, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), float(got[bad][0]), float(exp[bad][0])))


def _packed(ops, case, dev):
    wa, wb = case["w"][:case["NA"]].to(dev), case["w"][case["NA"]:].to(dev)
    packs = [("pack_heads", ops.pack_heads(wa, wb))]
    if case["variant"] == "narrow":                                  # precision "bf16": the rounding must leave the narrow grid unchanged
        packs.append(("pack_heads_bf16", ops.pack_heads_bf16(wa, wb)))
        assert torch.equal(packs[0][1], packs[1][1])
    return packs


def _run_stage(ops, dev, monkeypatch, case):
    K, NA, NB, T = case["K"], case["NA"], case["NB"], case["T"]
    planes = dense_to_planes(case["spk"]).to(dev)
    p = NC.abi_params(case["constants"], case["li_order"])
    exp_last, exp_sum = _expected(case, dev)
    steps = case["steps"] if case["readouts"] else None
    firsts = {}
    for name, wh in _packed(ops, case, dev):
        for form in L.FORMS:
            _set_form(monkeypatch, form)
            for want_sums in (False, True):
                what = "%s, SNN_LI_HEADS=%s, sums %s" % (name, form, want_sums)
                o_a, o_b, s_a, s_b = _call(planes, K, wh, NA, NB, p, steps, want_sums)
                if steps is None:
                    o_a, o_b = o_a[None], o_b[None]
                    s_a, s_b = (s_a[None], s_b[None]) if want_sums else (None, None)
                _same(o_a, o_b, exp_last, what)
                if want_sums and exp_sum is not None:
                    _same(s_a, s_b, exp_sum, what + " (time sums)")
                    for key, t in (("sum_a", s_a), ("sum_b", s_b)):
                        assert torch.equal(firsts.setdefault(key, t), t), what
                for key, t in (("a", o_a), ("b", o_b)):              # all forms agree - a consequence of the above, asserted anyway
                    assert torch.equal(firsts.setdefault(key, t), t), what
    # the public entries are the same calls
    monkeypatch.delenv("SNN_LI_HEADS", raising=False)
    wh = _packed(ops, case, dev)[0][1]
    if steps is None:
        out = ops.li_heads(planes, K, wh, NA, NB, p, want_sums=True)
        out = [t[None] for t in out]
    else:
        out = ops.li_heads_readouts(planes, K, wh, NA, NB, p, steps, want_sums=True)
    _same(out[0], out[1], exp_last, "ops entry")
    if exp_sum is not None:
        _same(out[2], out[3], exp_sum, "ops entry (time sums)")


def _default_run(cid, kw):
    """the edges run by default; the T edges in between, and the second LI order on the two K = 1024 shapes, are marked `sweep`"""
    if not cid.startswith("T"):
        return True
    return kw["T"] in L.T_DEFAULT[kw["name"]] and (kw.get("li_order", "jump_first") == "jump_first" or kw["K"] == 256)


@pytest.mark.parametrize("cid", [c if _default_run(c, kw) else pytest.param(c, marks=pytest.mark.sweep) for c, kw in L.stage_grid()])
def test_li_heads_equal_the_expectation_bit_for_bit(ops, gpu_device, monkeypatch, cid):
    _run_stage(ops, gpu_device, monkeypatch, L.stage_case(**STAGE[cid]))


def test_voltage_first_does_not_see_the_last_step(ops, gpu_device, monkeypatch):
    """kappa_last[T - 1] = kappa_sum[T - 1] = 0 in voltage-first order: a T = 1 call writes exact zeros over the NaN, and the last plane of
    a longer call may hold anything"""
    case = L.stage_case(M=83, K=256, NA=3, NB=12, T=1, name="a2_b2", li_order="voltage_first")
    assert not case["last"].any() and not case["sum"].any() and case["spk"].any()
    _run_stage(ops, gpu_device, monkeypatch, case)
    case = L.stage_case(M=83, K=256, NA=3, NB=12, T=9, name="a2_b2", li_order="voltage_first")
    spk = case["spk"].copy()
    spk[-1] = 1.0 - spk[-1]                                           # every bit of the last plane flipped
    _run_stage(ops, gpu_device, monkeypatch, dict(case, spk=spk))


@pytest.mark.parametrize("cid", ["T12_a2_b2_83x256x15_jump_first", "T12_a2_b2_17x1024x45_jump_first", "ro_a2_b1_T11_n11_17x128x25", "N91_364"])
def test_plane_stride_beyond_the_planes_is_honoured(ops, gpu_device, monkeypatch, cid):
    """a plane stride larger than M * Kw words with all-ones filler between the planes: nothing but the planes is read"""
    case = L.stage_case(**STAGE[cid])
    K, NA, NB, T, M = case["K"], case["NA"], case["NB"], case["T"], case["M"]
    Kw = (K + 31) // 32
    stride = M * Kw + 4 * 37                                          # (a multiple of four words: the resident kernel loads 16-byte lines)
    buf = torch.full((T, stride), -1, dtype=torch.int32, device=gpu_device)
    buf[:, :M * Kw] = dense_to_planes(case["spk"]).to(gpu_device).view(T, M * Kw)
    view = buf[:, :M * Kw].view(T, M, Kw)                             # shape only: _call passes the base address and the stride
    assert view.data_ptr() == buf.data_ptr()
    p = NC.abi_params(case["constants"], case["li_order"])
    exp_last, exp_sum = _expected(case, gpu_device)
    wh = _packed(ops, case, gpu_device)[0][1]
    steps = case["steps"] if case["readouts"] else None
    for form in L.FORMS:
        _set_form(monkeypatch, form)
        o_a, o_b, s_a, s_b = _call(view, K, wh, NA, NB, p, steps, True, stride=stride)
        if steps is None:
            o_a, o_b, s_a, s_b = o_a[None], o_b[None], s_a[None], s_b[None]
        _same(o_a, o_b, exp_last, "stride, SNN_LI_HEADS=%s" % form)
        _same(s_a, s_b, exp_sum, "stride, SNN_LI_HEADS=%s (time sums)" % form)


# ---- head level --------------------------------------------------------------------------------------------------------------------------
def _recorded(ops, name, call):
    """run call() with ops.<name> wrapped: (what call() returned, what ops.<name> returned - the raw outputs of that very pass)"""
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


def _rpn_module(case, dev, precision):
    import snn_automotive_object_detection_amd as pkg
    m = pkg.RPNHeadSNN(case["C"], case["A"], case["T"]).to(dev)
    m.precision, m.li_order = precision, case["li_order"]
    m.load_state_dict({"shared_conv.weight": case["w_shared"], "conv_cls.weight": case["w_cls"], "conv_bbox.weight": case["w_bbox"]})
    NC.set_on_module(m, case["constants"], L.ROUTE)
    assert m._resolve_precision() == precision                       # no fallback to another precision
    return m


def _rpn_hidden(case, dev, m, rates, sparse, split):
    """the pass that just ran took the launch the case is about and left the oracle's planes (zero flips) and counts"""
    C, T, N = case["C"], case["T"], case["N"]
    if sparse is not None:
        assert _lib().snn_debug_last_conv_path() == int(sparse), "not the launch this test is about"
    if split is not None:
        assert PL.rpn_planes(dev, T, (C + 31) // 32)[1] == int(split), "not the plane layout this test is about"
    got = planes_to_dense(PL.head_rpn_planes(dev, T, C), C)
    diff = got != case["spk"]
    assert not diff.any(), "hidden planes differ from the oracle's at (step, position, channel) %s ... (%d in all)" % (np.argwhere(diff)[:4].tolist(), int(diff.sum()))
    if rates and m.last_spike_counts is not None:
        assert np.array_equal(m.last_spike_counts[:, :N].cpu().numpy(), case["counts"])


def _level_rows(per_level):
    return torch.cat([t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) for t in per_level])


def run_rpn(case, dev, precision="bf16x3", sparse=None, split=None):
    """both modes of RPNHeadSNN: hidden planes and counts == the oracle's, logits and box deltas == the expectation at every position, the raw
    time sums of the spike-rate pass as well"""
    from snn_automotive_object_detection_amd import ops
    m = _rpn_module(case, dev, precision)
    feats = [f.to(dev) for f in case["feats"]]
    exp_last, exp_sum = _expected(case, dev)
    for rates in (False, True):
        m.spike_rates = rates
        out, (o_l, o_b, _, (_, sum_l, sum_b, _)) = _recorded(ops, "rpn_head_forward", lambda: m(feats))
        _rpn_hidden(case, dev, m, rates, sparse, split)
        _same(o_l, o_b, exp_last[-1], "rpn %s rates %s" % (precision, rates))
        _same(_level_rows(out[0]), _level_rows(out[1]), exp_last[-1], "rpn %s rates %s (what forward returns)" % (precision, rates))
        if rates and exp_sum is not None:
            _same(sum_l, sum_b, exp_sum[-1], "rpn %s (time sums)" % precision)
    return m


def run_rpn_readouts(case, dev, precision="bf16x3", sparse=None, split=None):
    from snn_automotive_object_detection_amd import ops
    m = _rpn_module(case, dev, precision)
    feats = [f.to(dev) for f in case["feats"]]
    exp_last, exp_sum = _expected(case, dev)
    steps = case["steps"]
    for rates in (False, True):
        m.spike_rates = rates
        out, (o_l, o_b, _, (_, sum_l, sum_b, _)) = _recorded(ops, "rpn_head_forward_readouts", lambda: m.forward_readouts(feats, steps))
        _rpn_hidden(case, dev, m, False, sparse, split)
        assert sorted(out) == list(steps)
        for j, Tp in enumerate(steps):
            _same(o_l[j], o_b[j], exp_last[j], "rpn readout T' = %d, rates %s" % (Tp, rates))
            _same(_level_rows(out[Tp][0]), _level_rows(out[Tp][1]), exp_last[j], "rpn readout T' = %d (what forward_readouts returns)" % Tp)
            if rates and exp_sum is not None:
                _same(sum_l[j], sum_b[j], exp_sum[j], "rpn readout T' = %d (time sums)" % Tp)


def _det_module(case, dev, precision):
    import snn_automotive_object_detection_amd as pkg
    d = pkg.FastRCNNPredictorSNNFull(case["C"] * 49, case["Hd"], case["K"], case["T"]).to(dev)
    d.precision, d.li_order = precision, case["li_order"]
    d.load_state_dict({"fc6.weight": case["w6"], "fc7.weight": case["w7"], "cls_score.weight": case["w_cls"], "bbox_pred.weight": case["w_bbox"]})
    NC.set_on_module(d, case["constants"], L.ROUTE)
    assert d._resolve_precision() == precision
    return d


def _det_hidden(case, dev, d, rates, extras):
    R, Hd, T = case["R"], case["Hd"], case["T"]
    e6, e7 = case["trace"]["spk6"].numpy(), case["trace"]["spk7"].numpy()
    p6, p7 = PL.head_det_planes(dev, T, Hd, R)
    n6 = T if rates else T - 1                                       # (without the rates lif6's spikes of the last step are never read and not formed)
    d6, d7 = planes_to_dense(p6, Hd)[:n6] != e6[:n6], planes_to_dense(p7, Hd) != e7
    assert not d6.any(), "lif6 planes differ at (step, RoI, unit) %s ... (%d in all)" % (np.argwhere(d6)[:4].tolist(), int(d6.sum()))
    assert not d7.any(), "lif7 planes differ at (step, RoI, unit) %s ... (%d in all)" % (np.argwhere(d7)[:4].tolist(), int(d7.sum()))
    if rates and extras is not None:
        c6, c7 = (c.cpu().numpy().astype(np.int64) for c in extras[:2])
        assert np.array_equal(c6, case["counts"][0]) and np.array_equal(c7, case["counts"][1])


def run_det(case, dev, precision="bf16x3"):
    from snn_automotive_object_detection_amd import ops
    d = _det_module(case, dev, precision)
    x = case["x"].to(dev)
    exp_last, exp_sum = _expected(case, dev)
    for rates in (False, True):
        d.spike_rates = rates
        out, (o_c, o_b, extras) = _recorded(ops, "det_head_forward", lambda: d(x))
        _det_hidden(case, dev, d, rates, extras)
        _same(o_c, o_b, exp_last[-1], "det %s rates %s" % (precision, rates))
        if not rates:
            _same(out[0], out[1], exp_last[-1], "det %s (what forward returns)" % precision)
        elif exp_sum is not None:
            _same(extras[2], extras[3], exp_sum[-1], "det %s (time sums)" % precision)
    return d


def run_det_readouts(case, dev, precision="bf16x3"):
    from snn_automotive_object_detection_amd import ops
    d = _det_module(case, dev, precision)
    x = case["x"].to(dev)
    exp_last, exp_sum = _expected(case, dev)
    steps = case["steps"]
    for rates in (False, True):
        d.spike_rates = rates
        out, (o_c, o_b, extras) = _recorded(ops, "det_head_forward_readouts", lambda: d.forward_readouts(x, steps))
        _det_hidden(case, dev, d, rates, None)
        for j, Tp in enumerate(steps):
            _same(o_c[j], o_b[j], exp_last[j], "det readout T' = %d, rates %s" % (Tp, rates))
            if not rates:
                _same(out[Tp][0], out[Tp][1], exp_last[j], "det readout T' = %d (what forward_readouts returns)" % Tp)
            elif exp_sum is not None:
                _same(extras[2][j], extras[3][j], exp_sum[j], "det readout T' = %d (time sums)" % Tp)


@pytest.mark.parametrize("name", ["a2_b2", "a2_b1", "a2_b4"])
def test_rpn_head_C64_on_every_dyadic_set(gpu_device, name):
    run_rpn(L.HEAD_CASES["rpn_C64_T8_%s" % name](), gpu_device, sparse=True, split=False)


@pytest.mark.parametrize("T,name", L.RPN_C256)
def test_rpn_head_C256_split_planes_and_dense_conv(gpu_device, T, name):
    """the RPN conv at C = 256 - structured-sparse at T = 8, 12, 16, dense at T = 4 - leaves its planes in blocks of four words, which the
    resident matrix-core heads kernel reads (half_split)"""
    run_rpn(L.HEAD_CASES["rpn_C256_T%d_%s" % (T, name)](), gpu_device, sparse=T >= 5, split=True)


def test_rpn_head_two_levels_with_a_ragged_last_tile(gpu_device):
    case = L.HEAD_CASES["rpn_two_levels"]()
    assert sum(case["N"] * h * w for h, w in case["shapes"]) % 16
    run_rpn(case, gpu_device)


def test_heads_voltage_first(gpu_device):
    run_rpn(L.HEAD_CASES["rpn_voltage_first"](), gpu_device, sparse=True)
    run_det(L.HEAD_CASES["det_voltage_first"](), gpu_device)


def test_heads_with_three_plane_head_weights(gpu_device):
    """planted 18-bit head weights: the mid and lo planes of lih_split3 carry bits the expectation needs"""
    run_rpn(L.HEAD_CASES["rpn_wide"](), gpu_device, sparse=False)
    run_det(L.HEAD_CASES["det_pm1_wide"](), gpu_device)


@pytest.mark.parametrize("R,Hd,T,name", L.DET_SHAPES)
def test_det_head_widths_and_row_counts(gpu_device, R, Hd, T, name):
    """Hd = 1024 with K = 9 (45 outputs): W does not fit in LDS, the reduction-split kernel runs by default"""
    run_det(L.HEAD_CASES["det_Hd%d_R%d_T%d_%s" % (Hd, R, T, name)](), gpu_device)


@pytest.mark.parametrize("precision", ["f32", "f32_strict"])
def test_heads_at_the_fp32_precisions(gpu_device, precision):
    """"f32_strict" takes the fp32 VALU heads kernel"""
    run_rpn(L.HEAD_CASES["rpn_C64_T8_a2_b1"](), gpu_device, precision)
    run_det(L.HEAD_CASES["det_Hd128_R17_T12_a2_b2"](), gpu_device, precision)
    run_det(L.HEAD_CASES["det_Hd1024_R17_T12_a2_b2"](), gpu_device, precision)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3"])
def test_heads_on_the_narrow_grid(gpu_device, precision):
    run_rpn(L.HEAD_CASES["rpn_narrow"](), gpu_device, precision)
    run_det(L.HEAD_CASES["det_narrow"](), gpu_device, precision)


def test_rpn_head_at_mxfp6(gpu_device):
    run_rpn(L.HEAD_CASES["rpn_mx"](), gpu_device, "mxfp6")


@pytest.mark.parametrize("form", ["valu", "ksplit", "mfma"])
def test_whole_heads_under_every_forced_kernel_form(gpu_device, monkeypatch, form):
    """SNN_LI_HEADS inside the whole-head entries.  (C = 256 on the sparse conv hands over split planes, which only the resident kernel
    reads: the knob is for the other shapes.)"""
    monkeypatch.setenv("SNN_LI_HEADS", form)
    run_rpn(L.HEAD_CASES["rpn_C64_T8_a2_b4"](), gpu_device)
    run_det(L.HEAD_CASES["det_Hd256_R65_T12_a2_b1"](), gpu_device)


def test_whole_head_readouts_equal_the_expectation_rows(gpu_device):
    """steps (4, 8, 12) of one pass at T = 12: with zero flips the hidden planes of the pass are the oracle's, so readout T' is row T' - 1 of
    the recursion on them, exactly"""
    assert L.READOUT_STEPS == (4, 8, 12)
    run_rpn_readouts(L.HEAD_CASES["rpn_readouts"](), gpu_device, sparse=True, split=True)
    run_det_readouts(L.HEAD_CASES["det_readouts"](), gpu_device)
    run_det_readouts(L.HEAD_CASES["det_readouts"](), gpu_device, "f32_strict")
