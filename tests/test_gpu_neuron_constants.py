"""Neuron constants other than the reference's, on the GPU, against the parametrised oracle (oracle/snn_oracle.NeuronConstants).

snn_params carries dt * tau_mem_inv, -dt * tau_syn_inv, the rest and reset potentials and both thresholds across the C ABI, and the launchers
choose kernel text and launch plans from them (csrc/snn_kernels.hip): the encoder's three forms (enc_mode: the threshold table, built per
(ca, v_th_enc), the zero-rest recurrence, the op-for-op form), period planes and the structured-sparse launches (zero rest and reset
potentials only), the windows of time steps that are formed (a rest potential above the threshold fires at step 0), the straight-line and
the guarded general LIF epilogues, the LI heads' impulse responses.  Every other parity test runs at the reference's constants; here the
sets of tests/_exact_grid.NEURON_SETS (tests/test_neuron_constants_cpu.py shows what they are sensitive to) go through

  * the stage entries, bit for bit - this is element-wise arithmetic, no grid needed: encoders on the fixtures' features plus both floats
    either side of every first-spike boundary of the set and the reset sentinels (tests/_neuron_constants.planted_inputs), as spike
    planes and as period planes; the LIF scan on random currents; the fused conv / linear + LIF launches on the oracle's own planes;
  * both heads on the dyadic grids (tests/_exact_grid.py: the currents are the same fp32 number on both sides), with ZERO flips: hidden
    planes and integer spike counts equal to the oracle's, outputs within CUR_TOL of the fp64 LI recursion at the set's (a, b) and within
    1e-4 of the oracle - at the T classes of both heads, the other precisions, both LI orders;
  * the equalities that hold at the reference's constants: half-precision and channels-last features, the RoIAlign-fed head, any-time
    readouts, the padded static path.
Each case asserts the launch it is about (snn_debug_last_conv_path / _fc6_path) and the encoder form that ran (snn_debug_last_enc_mode); the
expectations are derived from the launchers: period planes and the sparse side need v_leak == v_reset == 0 and no spike at step 0
(periods_possible, gemm3_lif_sparse), the table needs 0 < ca < 1 (enc_thresholds).  Routes: sets the modules accept are set on their public
attributes (p_enc, p_lif, dt); rest potentials and other time constants go in as hand-made snn_params (tests/_neuron_constants.set_on_module).
The default run takes every set at T = 8 / 12 and three sets at every T class and precision; the rest is marked `sweep`."""
import ctypes as Ct

import numpy as np
import pytest
import torch

from oracle import fixtures as FX
from oracle import snn_oracle as OR
from tests import _exact_grid as G
from tests import _neuron_constants as NC
from tests._util import dense_to_planes, nchw_to_rows, planes_to_dense
from tests.test_gpu_exact_grid import TOL, run_det, run_rpn

pytestmark = pytest.mark.gpu
SETS = sorted(G.NEURON_SETS)
ENC_GENERIC, ENC_ZR, ENC_QUANT = 0, 1, 2


def _k(name):
    return G.NEURON_SETS[name][0]


def _sets_with_sweep(default):
    return [n if n in default else pytest.param(n, marks=pytest.mark.sweep) for n in SETS]


@pytest.fixture(scope="module")
def ops():
    from snn_automotive_object_detection_amd import ops
    return ops


def _lib():
    from snn_automotive_object_detection_amd import _lib
    return _lib.load()


def _table_ok(k) -> bool:
    """the library's own verdict on its threshold table for these constants (host code)"""
    th = (Ct.c_float * 32)()
    p = NC.abi_params(k)
    rc = _lib().snn_debug_encoder_thresholds(Ct.byref(p), th)
    assert rc in (0, 1)
    return rc == 1


def _expected_table_ok(k) -> bool:
    """csrc/snn_kernels.hip: enc_thresholds builds a table for 0 < ca < 1 and v_th > 0; snn_debug_encoder_thresholds adds zero rest"""
    return 0.0 < k.ca < 1.0 and k.v_th_enc > 0 and G.is_zero_rest(k)


def _head_enc_mode(k, precision="bf16x3"):
    """the encoder form a head forward runs (enc_mode): op for op unless rest and reset potentials are zero; then the threshold table where
    the head multiplies period planes (the bf16x3 family) and the table verified, else the zero-rest recurrence"""
    if not G.is_zero_rest(k):
        return ENC_GENERIC
    if precision in ("bf16x3", "bf16") and _expected_table_ok(k):
        return ENC_QUANT
    return ENC_ZR


def _sparse(k, default: bool) -> bool:
    """gemm3_lif_sparse: the structured-sparse side needs period planes (periods_possible: v_leak == v_reset == 0) and no spike at step 0"""
    return bool(default) and G.is_zero_rest(k) and not G.fires_at_step_0(k)


# ---- stage level: encoders ---------------------------------------------------------------------------------------------------------------
def _first_spike_planes(z: np.ndarray) -> np.ndarray:
    """spikes {0, 1} [T, ...] -> the period planes e_t = (first spike at step t)"""
    zb = z > 0
    before = np.zeros_like(zb[0])
    out = np.zeros_like(zb)
    for t in range(zb.shape[0]):
        out[t] = zb[t] & ~before
        before |= zb[t]
    return out.astype(np.float32)


def _plant(x: torch.Tensor, vals: np.ndarray, count=None) -> torch.Tensor:
    """the planted values over the head of the flattened tensor and once more over its tail (first and last work-group, ragged last word);
    ``count`` > len(vals): the vector repeated to that many elements at either end"""
    flat = x.clone().reshape(-1)
    n = min(int(count or len(vals)), flat.numel())
    v = torch.from_numpy(np.resize(vals, n).copy())
    flat[:n] = v
    flat[flat.numel() - n:] = v
    return flat.reshape(x.shape)


@pytest.mark.parametrize("name", SETS)
def test_encoders_equal_the_oracle(ops, gpu_device, monkeypatch, name):
    """snn_encode_nchw / snn_encode_rows at the set's constants: spike planes (the zero-rest recurrence or the op-for-op form) and, for
    zero rest / reset potentials, period planes (SNN_STAGE_PERIODS=1: the threshold table rebuilt for the set's (ca, v_th_enc) - or the
    recurrence where the table cannot be built) against the oracle's encoder, bit for bit, on the features of tests/test_gpu_stages.py's
    encoder tests with the set's boundary inputs planted"""
    k = _k(name)
    p = NC.abi_params(k)
    assert _table_ok(k) == _expected_table_ok(k)
    zero_rest = G.is_zero_rest(k)
    plain = ENC_ZR if zero_rest else ENC_GENERIC
    period = ENC_QUANT if _expected_table_ok(k) else ENC_ZR
    for spec_name in ("rpn_c16_T8", "rpn_c256_T24"):
        spec = FX.RPN_SPECS[spec_name]
        T = spec["T"]
        planted = NC.planted_inputs(k, T)
        for f in FX.rpn_inputs(spec)[0]:
            f = _plant(f, planted)
            z = nchw_to_rows(OR.encoder_spikes(f, T, k))
            planes = ops.encode_nchw(f.to(gpu_device), T, p)
            assert _lib().snn_debug_last_enc_mode() == plain
            full = planes_to_dense(planes, planes.shape[2] * 32)
            assert np.array_equal(full[:, :, :f.shape[1]], z) and not full[:, :, f.shape[1]:].any()
            if zero_rest:
                monkeypatch.setenv("SNN_STAGE_PERIODS", "1")
                e = ops.encode_nchw(f.to(gpu_device), T, p)
                assert _lib().snn_debug_last_enc_mode() == period
                monkeypatch.delenv("SNN_STAGE_PERIODS")
                assert np.array_equal(planes_to_dense(e, f.shape[1]), _first_spike_planes(z))
    for spec_name in ("det_small_T16", "det_K11_T8_R37"):             # D = 392 (ragged last word, the element-per-lane kernel) and 12544 (word per lane)
        spec = FX.DET_SPECS[spec_name]
        T = spec["T"]
        x = _plant(FX.det_inputs(spec)[0].flatten(1), NC.planted_inputs(k, T))
        z = OR.encoder_spikes(x, T, k).numpy()
        planes = ops.encode_rows(x.to(gpu_device), T, p)
        assert _lib().snn_debug_last_enc_mode() == plain
        full = planes_to_dense(planes, planes.shape[2] * 32)
        assert np.array_equal(full[:, :, :x.shape[1]], z) and not full[:, :, x.shape[1]:].any()
        if zero_rest:
            monkeypatch.setenv("SNN_STAGE_PERIODS", "1")
            e = ops.encode_rows(x.to(gpu_device), T, p)
            assert _lib().snn_debug_last_enc_mode() == period
            monkeypatch.delenv("SNN_STAGE_PERIODS")
            assert np.array_equal(planes_to_dense(e, x.shape[1]), _first_spike_planes(z))
        assert z.any() and not z.all()


# ---- stage level: the LIF scan and the fused launches --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SETS)
def test_lif_scan_equals_the_oracle(ops, gpu_device, name):
    k = _k(name)
    p = NC.abi_params(k)
    for T in (1, 2, 8, 17):
        g = torch.Generator().manual_seed(100 + T)
        cur = torch.randn(T, 33, 100, generator=g) * 0.5
        want, _, _ = OR.lif_scan_from_currents(cur, constants=k)
        spk, counts = ops.lif_scan(cur.to(gpu_device), 100, p, want_counts=True)
        full = planes_to_dense(spk, spk.shape[2] * 32)
        assert np.array_equal(full[:, :, :100], want.numpy()) and not full[:, :, 100:].any(), T
        assert np.array_equal(counts.cpu().numpy(), want.sum(dim=(0, 2)).numpy().astype(np.int32))
        assert bool(want[0].all()) == G.fires_at_step_0(k) and (T < 8 or 0.02 < float(want.mean()) < 0.9)


@pytest.mark.parametrize("name", SETS)
def test_fused_conv_and_linear_lif_equal_the_oracle_on_its_own_encoder_planes(ops, gpu_device, name):
    """snn_conv3x3_lif_bf16x3 and snn_spike_gemm_lif_bf16x3 fed the ORACLE's encoder spike planes of the grid cases: the currents are exact,
    so the LIF planes equal the oracle's spk / spk6 at every step"""
    k = _k(name)
    p = NC.abi_params(k)
    case = G.rpn_t_case(64, 8, constants=k)
    C, T = case["C"], case["T"]
    shapes3 = [(case["N"], h, w) for h, w in case["shapes"]]
    enc = torch.cat([dense_to_planes(nchw_to_rows(tr["z"])) for tr in case["traces"]], dim=1).to(gpu_device)
    spk = ops.conv3x3_lif_bf16x3(enc, shapes3, C, C, p, ops.pack_conv3x3_bf16x3(case["w_shared"].to(gpu_device)))
    diff = planes_to_dense(spk, C) != case["spk"]
    assert not diff.any(), "conv + LIF planes differ at (step, position, channel) %s ... (%d in all)" % (np.argwhere(diff)[:4].tolist(), int(diff.sum()))
    case = G.det_t_case(12, constants=k)
    tr = case["trace"]
    a = dense_to_planes(tr["z"].numpy()).to(gpu_device)
    s6 = ops.spike_gemm_lif_bf16x3(a, case["C"] * 49, case["Hd"], p, ops.pack_linear_bf16x3(case["w6"].to(gpu_device)))
    diff = planes_to_dense(s6, case["Hd"]) != tr["spk6"].numpy()
    assert not diff.any(), "fc6 + LIF planes differ at (step, RoI, unit) %s ... (%d in all)" % (np.argwhere(diff)[:4].tolist(), int(diff.sum()))
    a = dense_to_planes(tr["spk6"].numpy()).to(gpu_device)
    s7 = ops.spike_gemm_lif_bf16x3(a, case["Hd"], case["Hd"], p, ops.pack_linear_bf16x3(case["w7"].to(gpu_device)))
    assert np.array_equal(planes_to_dense(s7, case["Hd"]), tr["spk7"].numpy())


# ---- head level: zero flips on the wide grid ------------------------------------------------------------------------------------------------
def _rpn(dev, name, T, C=64, precision="bf16x3", grid="wide", li_order="jump_first", **kw):
    k = _k(name)
    # (the T classes of tests/test_gpu_exact_grid.py: the dense tile below 5 and above 16 steps, the sparse / FAT launch in between)
    sparse = _sparse(k, 5 <= T <= 16) if precision in ("bf16x3", "bf16") else False
    exact_T = T in (8, 12)
    em = _head_enc_mode(k, precision)
    if not exact_T and em == ENC_QUANT:
        em = (ENC_QUANT, ENC_ZR)                                     # (period planes only where a tile holds the window: g3_some_tile_ok)
    return run_rpn(G.rpn_t_case(C, T, grid, li_order, constants=k), dev, precision, sparse=sparse if precision == "bf16x3" else None, enc_mode=em, **kw)


def _det(dev, name, T, C=64, precision="bf16x3", grid="wide", li_order="jump_first", **kw):
    k = _k(name)
    if C == 64:
        case = G.det_t_case(T, grid, li_order, constants=k)
    else:
        assert T == 12 and grid == "wide" and li_order == "jump_first"
        case = G.det_r_case(29, C, constants=k)
    # fc6 takes the sparse launch once it forms four live steps, T - 2 of them, T - 1 in spike-rate mode; C = 32: 49 C / 32 is odd - the dense tile
    sparse = (_sparse(k, C == 64 and T >= 6), _sparse(k, C == 64 and T >= 5))
    em = _head_enc_mode(k, precision)
    if T != 12 and em == ENC_QUANT:
        em = (ENC_QUANT, ENC_ZR)
    return run_det(case, dev, precision, fc6_sparse=sparse if precision == "bf16x3" else None, enc_mode=em, **kw)


@pytest.mark.parametrize("name", SETS)
def test_rpn_head_every_set(gpu_device, name):
    _rpn(gpu_device, name, 8)


@pytest.mark.parametrize("name", SETS)
def test_det_head_every_set(gpu_device, name):
    _det(gpu_device, name, 12)


@pytest.mark.parametrize("T", [4, 17])
@pytest.mark.parametrize("name", _sets_with_sweep(G.T_CLASS_SETS))
def test_rpn_head_T_classes(gpu_device, name, T):
    """T = 4: the dense tile; T = 17: the guarded general epilogue (T = 8, the sparse / FAT launch where the set allows it, runs above)"""
    _rpn(gpu_device, name, T)


@pytest.mark.parametrize("T", [3, 24])
@pytest.mark.parametrize("name", _sets_with_sweep(G.T_CLASS_SETS))
def test_det_head_T_classes(gpu_device, name, T):
    _det(gpu_device, name, T)


@pytest.mark.parametrize("name", _sets_with_sweep(G.T_CLASS_SETS))
def test_det_head_dense_fc6_tile(gpu_device, name):
    _det(gpu_device, name, 12, C=32)


def _planted_rpn_case(k, T):
    """rpn_t_case(64, T) with the set's boundary inputs and reset sentinels planted at the head and the tail of every level, the oracle run again"""
    base = G.rpn_t_case(64, T, constants=k)
    # (eight whole channel maps of the first and of the last image: a wrong first or second spike of a planted value then moves the currents of
    # every position of the level by several weights, far more than a threshold - the hidden planes are all the head lets one see)
    feats = [_plant(f, NC.planted_inputs(k, T), min(f[0].numel() // 2, 8 * f.shape[2] * f.shape[3])) for f in base["feats"]]
    counts = []
    with torch.no_grad():
        logits, bbox, traces = OR.rpn_head_forward(feats, base["w_shared"], base["w_cls"], base["w_bbox"], T, trace=True, counts_out=counts, constants=k)
    spk = np.concatenate([nchw_to_rows(tr["spk"]) for tr in traces], axis=1)
    return dict(base, feats=feats, logits=logits, bbox=bbox, traces=traces, spk=spk, counts=torch.stack(counts).numpy())


def _planted_det_case(k, T):
    base = G.det_t_case(T, constants=k)
    x = _plant(base["x"], NC.planted_inputs(k, T), base["x"][0].numel())     # the first and the last RoI whole
    counts = []
    with torch.no_grad():
        cls, bbox, tr = OR.det_head_forward(x, base["w6"], base["w7"], base["w_cls"], base["w_bbox"], T, trace=True, counts_out=counts, constants=k)
    return dict(base, x=x, cls=cls, bbox=bbox, trace=tr, counts=[c.numpy() for c in counts])


@pytest.mark.parametrize("name", SETS)
def test_heads_on_planted_boundary_inputs(gpu_device, name):
    """the heads' own encoder launches (all levels in one launch; word-major rows, folded with fc6's permutation and the plane compression
    where the sparse launch runs) are other kernel text than the stage entries': the grid cases again with both floats either side of every
    first-spike boundary and the reset sentinels among the features - an encoder that resets to exactly v_reset fails here too"""
    k = _k(name)
    run_rpn(_planted_rpn_case(k, 8), gpu_device, sparse=_sparse(k, True), enc_mode=_head_enc_mode(k))
    run_det(_planted_det_case(k, 12), gpu_device, fc6_sparse=_sparse(k, True), enc_mode=_head_enc_mode(k))


# ---- the other precisions, both LI orders --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,grid", [("f32", "wide"), ("f32_strict", "wide"), ("bf16", "narrow")])
@pytest.mark.parametrize("name", G.T_CLASS_SETS)
def test_heads_other_precisions(gpu_device, name, precision, grid):
    _rpn(gpu_device, name, 8, precision=precision, grid=grid)
    _det(gpu_device, name, 12, precision=precision, grid=grid)


@pytest.mark.parametrize("name", G.T_CLASS_SETS)
def test_heads_at_mxfp6(gpu_device, name):
    k = _k(name)
    _rpn(gpu_device, name, 8, C=256, precision="mxfp6", grid="narrow")
    run_det(G.det_mx_case("wide", constants=k), gpu_device, "mxfp6", enc_mode=_head_enc_mode(k, "mxfp6"))


def test_voltage_first_with_a_reset_potential(gpu_device):
    _rpn(gpu_device, "vreset_-0.05", 8, li_order="voltage_first")
    _det(gpu_device, "vreset_-0.05", 12, li_order="voltage_first")


# ---- equalities that must survive the general forms ------------------------------------------------------------------------------------------
EQ_SETS = ("vreset_-0.05", "vth_enc_1.0")


def _flat(out):
    return [t.clone() for t in (list(out[0]) + list(out[1]) if isinstance(out[0], (list, tuple)) else list(out))]


@pytest.mark.parametrize("name", EQ_SETS)
def test_feature_types_and_layouts_equal_fp32_nchw(gpu_device, name):
    """fp16 / bf16 / channels-last features give the bits of the fp32 NCHW call on the same values"""
    k = _k(name)
    rc, dc = G.rpn_t_case(64, 8, constants=k), G.det_t_case(12, constants=k)
    for feat in ("fp16", "bf16"):
        half = {"fp16": torch.float16, "bf16": torch.bfloat16}[feat]
        feats = [f.to(half) for f in rc["feats"]]
        x = dc["x"].to(half)
        import snn_automotive_object_detection_amd as pkg
        m = pkg.RPNHeadSNN(64, 3, 8).to(gpu_device)
        m.load_state_dict({"shared_conv.weight": rc["w_shared"], "conv_cls.weight": rc["w_cls"], "conv_bbox.weight": rc["w_bbox"]})
        d = pkg.FastRCNNPredictorSNNFull(64 * 49, 128, 9, 12).to(gpu_device)
        d.load_state_dict({"fc6.weight": dc["w6"], "fc7.weight": dc["w7"], "cls_score.weight": dc["w_cls"], "bbox_pred.weight": dc["w_bbox"]})
        for mod in (m, d):
            NC.set_on_module(mod, k, G.route_of(k))
        want_r = _flat(m([f.float().to(gpu_device) for f in feats]))
        want_d = _flat(d(x.float().to(gpu_device)))
        got_r = _flat(m([f.to(gpu_device) for f in feats]))
        got_d = _flat(d(x.to(gpu_device)))
        assert all(torch.equal(a, b) for a, b in zip(got_r + got_d, want_r + want_d)), feat
        nh_r = _flat(m([f.float().to(gpu_device).contiguous(memory_format=torch.channels_last) for f in feats]))
        nh_d = _flat(d(x.float().to(gpu_device).contiguous(memory_format=torch.channels_last)))
        assert all(torch.equal(a, b) for a, b in zip(nh_r + nh_d, want_r + want_d)), feat
        assert any(bool(t.any()) for t in want_r) and any(bool(t.any()) for t in want_d)
    # ... and against the oracle, on the grid, with the planes checked
    run_rpn(rc, gpu_device, nhwc=True, sparse=_sparse(k, True))
    run_det(dc, gpu_device, nhwc=True, fc6_sparse=_sparse(k, True))


@pytest.mark.parametrize("name", EQ_SETS)
def test_roialign_fed_head_equals_the_row_fed_head_on_its_own_pooled_rows(gpu_device, name):
    """the pattern of tests/test_gpu_roialign.py: the fused RoIAlign + encoder feed against the row-fed head on the GPU's own pooled_dbg rows,
    bit for bit - and both against the oracle on those rows (weights on the grid: zero flips)"""
    import snn_automotive_object_detection_amd as pkg
    from snn_automotive_object_detection_amd import ops
    from tests.test_gpu_roialign import _setup
    k = _k(name)
    dc = G.det_t_case(12, constants=k)
    pool, fm, boxes, shapes = _setup(gpu_device, R=60, C=64, seed=11)
    fm = {n: 2.0 * f for n, f in fm.items()}
    flist, scales, rois, lvl = pool.assign(fm, boxes, shapes)
    d = pkg.FastRCNNPredictorSNNFull(64 * 49, 128, 9, 12).to(gpu_device)
    d.load_state_dict({"fc6.weight": dc["w6"], "fc7.weight": dc["w7"], "cls_score.weight": dc["w_cls"], "bbox_pred.weight": dc["w_bbox"]})
    NC.set_on_module(d, k, G.route_of(k))
    planes, pooled = ops.roi_align_encode(flist, scales, rois[:, 1:5], rois[:, 0], lvl, 12, d._params(), want_pooled=True)
    z = OR.encoder_spikes(pooled.cpu(), 12, k)
    assert np.array_equal(planes_to_dense(planes, pooled.shape[1]), z.numpy())
    fused = _flat(d.forward_roialign(flist, scales, rois, lvl))
    assert _lib().snn_debug_last_fc6_path() == int(_sparse(k, True))
    rows = _flat(d(pooled.view(-1, 64, 7, 7)))
    assert torch.equal(fused[0], rows[0]) and torch.equal(fused[1], rows[1])
    with torch.no_grad():
        o_c, o_b = OR.det_head_forward(pooled.cpu().view(-1, 64, 7, 7), dc["w6"], dc["w7"], dc["w_cls"], dc["w_bbox"], 12, constants=k)
    assert float((fused[0].cpu() - o_c).abs().max()) <= TOL and float((fused[1].cpu() - o_b).abs().max()) <= TOL
    assert float(o_c.abs().max()) > 0


@pytest.mark.parametrize("name", EQ_SETS)
def test_readouts_equal_the_plain_forwards(gpu_device, name):
    """include/snn_hip.h, any-time readouts: the readout at T' = T is the plain forward at T bit for bit; a readout at T' < T is
    snn_li_heads at T' on the first T' planes of the pass, and equals the standalone forward at T' up to threshold ties where the two take
    different launches - on the grid there are no ties (the currents are exact), so the planes are the standalone forward's and every
    readout equals it bit for bit"""
    import snn_automotive_object_detection_amd as pkg
    k = _k(name)
    steps = (3, 8, 12)
    rc, dc = G.rpn_t_case(64, 12, constants=k), G.det_t_case(12, constants=k)
    m = pkg.RPNHeadSNN(64, 3, 12).to(gpu_device)
    m.load_state_dict({"shared_conv.weight": rc["w_shared"], "conv_cls.weight": rc["w_cls"], "conv_bbox.weight": rc["w_bbox"]})
    d = pkg.FastRCNNPredictorSNNFull(64 * 49, 128, 9, 12).to(gpu_device)
    d.load_state_dict({"fc6.weight": dc["w6"], "fc7.weight": dc["w7"], "cls_score.weight": dc["w_cls"], "bbox_pred.weight": dc["w_bbox"]})
    for mod in (m, d):
        NC.set_on_module(mod, k, G.route_of(k))
    feats = [f.to(gpu_device) for f in rc["feats"]]
    x = dc["x"].to(gpu_device)
    ro_r = {T: _flat(v) for T, v in m.forward_readouts(feats, steps).items()}
    ro_d = {T: _flat(v) for T, v in d.forward_readouts(x, steps).items()}
    for T in steps:
        m.num_steps = d.num_steps = T
        plain = _flat(m(feats)) + _flat(d(x))
        got = ro_r[T] + ro_d[T]
        worst = max(float((a - b).abs().max()) for a, b in zip(got, plain))
        print("readout at T' = %d against the standalone forward: %.3g" % (T, worst))
        assert all(torch.equal(a, b) for a, b in zip(got, plain)), T
        assert T < steps[-1] or all(bool(t.any()) for t in plain[-2:])         # (at v_th_enc = 1 nothing reaches the detector's outputs within 3 steps)
    # the readouts against the oracle at T' (its planes are a prefix of the T = 12 run's: one trace serves)
    with torch.no_grad():
        for T in steps:
            o_c, o_b = OR.det_head_forward(dc["x"], dc["w6"], dc["w7"], dc["w_cls"], dc["w_bbox"], T, constants=k)
            assert float((ro_d[T][0].cpu() - o_c).abs().max()) <= TOL and float((ro_d[T][1].cpu() - o_b).abs().max()) <= TOL


@pytest.mark.parametrize("name", EQ_SETS)
def test_padded_static_path_takes_the_constants_from_the_modules(gpu_device, name):
    """forward_padded against the list path (tests/test_gpu_static.py's saturated check) with the set on both heads: the static path builds
    its parameters through the modules' own _params(), so it must follow them - and the detections must differ from the default constants'"""
    import snn_automotive_object_detection_amd as S
    from tests.test_gpu_static import _check_saturated, _features as static_features
    k = _k(name)
    torch.manual_seed(1234)
    model = S.create_model("cityscapes", 9, True, True, 0, False, False, num_steps_rpn=8, num_steps_detector=12).eval()
    model.rpn.to(gpu_device)
    model.roi_heads.to(gpu_device)
    with torch.no_grad():
        model.rpn.head.shared_conv.weight.mul_(5.0)
    model.roi_heads.score_thresh = 0.05
    feats = static_features(gpu_device, 21)
    base = _check_saturated(model, feats)
    base = {n: t.clone() for n, t in base.items()}
    for mod in (model.rpn.head, model.roi_heads.box_head_and_predictor):
        NC.set_on_module(mod, k, G.route_of(k))
    out = _check_saturated(model, feats)
    assert not torch.equal(out["class_logits"], base["class_logits"])
