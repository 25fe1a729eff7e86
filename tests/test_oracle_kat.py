"""Known-answer tests pinning the oracle's neuron arithmetic.

The reference has no tests and does not ship Norse 0.0.7; these sequences are the pins:
the LIF membrane sequence is the one of upstream Norse's test_lif_feed_forward_step."""
import numpy as np
import torch

from oracle import norse_restated as NR


def test_lif_feed_forward_step_upstream_sequence():
    # v_th = 1 (default), constant input 1.0
    cell = NR.LIFCell()
    state = None
    x = torch.ones(1)
    vs = []
    for _ in range(10):
        z, state = cell(x, state)
        vs.append(float(state.v))
    expect = [0.0, 0.1, 0.27, 0.487, 0.7335, 0.9963, 0.0, 0.3951, 0.7717, 0.0]
    np.testing.assert_allclose(vs, expect, atol=1e-4)


def test_lif_theta_0p1_const_input():
    cell = NR.LIFCell(p=NR.LIFParameters(alpha=100, v_th=torch.tensor(0.1)), dt=0.001)
    state = None
    out = []
    for _ in range(4):
        z, state = cell(torch.ones(1), state)
        out.append((float(z), float(state.v), float(state.i)))
    expect = [(0, 0, 1), (0, 0.1, 1.8), (1, 0, 2.44), (1, 0, 2.952)]
    np.testing.assert_allclose(np.array(out), np.array(expect, dtype=np.float64), atol=1e-6)


def test_encoder_x1_pattern_and_subthreshold():
    p = NR.LIFParameters(v_th=torch.tensor(0.25))
    v = torch.zeros(1)
    zs, vs = [], []
    for _ in range(9):
        z, v = NR.lif_current_encoder(torch.ones(1), v, p, 0.001)
        zs.append(int(z)); vs.append(float(v))
    assert zs == [0, 0, 1, 0, 0, 1, 0, 0, 1]
    np.testing.assert_allclose(vs[:3], [0.1, 0.19, 0.0], atol=1e-7)
    for x in (0.25, 0.26, 0.3):
        v = torch.zeros(1)
        for _ in range(16):
            z, v = NR.lif_current_encoder(torch.full((1,), x), v, p, 0.001)
            assert float(z) == 0.0


def test_encoder_first_spike_thresholds():
    # closed form between resets: v_t = x (1 - 0.9^t); spike within T steps iff x(1-0.9^T) > 0.25
    p = NR.LIFParameters(v_th=torch.tensor(0.25))
    for T, xmin in ((8, 0.25 / (1 - 0.9 ** 8)), (12, 0.25 / (1 - 0.9 ** 12))):
        for x, should in ((xmin * 1.001, True), (xmin * 0.999, False)):
            v = torch.zeros(1); fired = False
            for _ in range(T):
                z, v = NR.lif_current_encoder(torch.full((1,), x), v, p, 0.001)
                fired |= bool(z)
            assert fired == should


def test_li_both_orders():
    for order, expect in (("jump_first", [0.1, 0.27, 0.487, 0.7335, 0.99631]),
                          ("voltage_first", [0.0, 0.1, 0.27, 0.487, 0.7335])):
        state = NR.LIState(torch.zeros(1), torch.zeros(1))
        vs = []
        for _ in range(5):
            v, state = NR.li_feed_forward_step(torch.ones(1), state, li_order=order)
            vs.append(float(v))
        np.testing.assert_allclose(vs, expect, atol=1e-5)


def test_constants_are_fp32_products():
    # dt * tau_mem_inv and dt * tau_syn_inv as the 0-dim fp32 products the oracle evaluates
    p = NR.LIFParameters()
    a = 0.001 * p.tau_mem_inv
    b = 0.001 * p.tau_syn_inv
    assert a.dtype == torch.float32 and b.dtype == torch.float32
    assert float(a) == float(np.float32(0.1)) and float(b) == float(np.float32(0.2))


def _dead(windows):
    """cur_hook that zeroes the input current of the steps OUTSIDE each layer's window [t0, t0+n)"""
    def hook(name, step, cur):
        t0, n = windows[name]
        return cur if t0 <= step < t0 + n else torch.zeros_like(cur)
    return hook


def test_dead_time_steps_cannot_reach_an_output():
    """What the HIP launchers skip (csrc/snn_kernels.hip: lif_windows), stated on the oracle: zeroing the 3x3 conv of the last
    RPN step, fc6 of the last two detector steps (the last one in spike-rate mode) and fc7 of the first and last step leaves
    every output, spike plane and rate tensor of the golden fixtures bit-identical (rpn.py:98-119, faster_rcnn.py:492-516:
    lif_feed_forward_step adds the input of step t after that step's membrane update)."""
    from oracle import fixtures as FX
    from oracle import snn_oracle as OR
    for name in ("rpn_c16_T8", "rpn_c256_T8_odd"):
        if name not in FX.RPN_SPECS:
            continue
        spec = FX.RPN_SPECS[name]
        feats, w_s, w_c, w_b = FX.rpn_inputs(spec)
        T = spec["T"]
        full = OR.rpn_head_forward(feats, w_s, w_c, w_b, T, trace=True, spike_rates=True)
        cut = OR.rpn_head_forward(feats, w_s, w_c, w_b, T, trace=True, spike_rates=True, cur_hook=_dead({"shared": (0, T - 1)}))
        for a, b in zip(full[0] + full[1] + full[2], cut[0] + cut[1] + cut[2]):
            assert torch.equal(a, b)
        for ta, tb in zip(full[3], cut[3]):
            assert torch.equal(ta["spk"], tb["spk"]) and bool(ta["spk"].any())
    for name in sorted(FX.DET_SPECS)[:2]:
        spec = FX.DET_SPECS[name]
        x, w6, w7, wc, wb = FX.det_inputs(spec)
        T = spec["T"]
        full = OR.det_head_forward(x, w6, w7, wc, wb, T, trace=True)
        cut = OR.det_head_forward(x, w6, w7, wc, wb, T, trace=True, cur_hook=_dead({"fc6": (0, T - 2), "fc7": (1, T - 2)}))
        assert torch.equal(full[0], cut[0]) and torch.equal(full[1], cut[1])
        assert torch.equal(full[2]["spk7"], cut[2]["spk7"]) and bool(full[2]["spk7"].any())
        r_full = OR.det_head_forward(x, w6, w7, wc, wb, T, spike_rates=True)
        r_cut = OR.det_head_forward(x, w6, w7, wc, wb, T, spike_rates=True, cur_hook=_dead({"fc6": (0, T - 1), "fc7": (1, T - 2)}))
        for a, b in zip(r_full, r_cut):
            assert torch.equal(a, b)
        # ... and one step more IS visible: the windows are tight
        one_less = OR.det_head_forward(x, w6, w7, wc, wb, T, trace=True, cur_hook=_dead({"fc6": (0, T - 3), "fc7": (1, T - 2)}))
        assert not torch.equal(full[2]["spk7"], one_less[2]["spk7"]) or not torch.equal(full[0], one_less[0])


def test_encoder_spike_trains_are_exactly_periodic():
    """What the HIP heads' period planes rest on (csrc/snn_common.h), stated on the oracle: the constant-current encoder starts from
    and resets to +0 (rpn.py:58,93,101; faster_rcnn.py:444,484,494), so a neuron's train is z_t = 1 iff n | t + 1 with n = (step of its
    first spike) + 1 - for every input, threshold neighbours included"""
    from oracle import snn_oracle as OR
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(20000, generator=g) * 4.0, torch.tensor([2.5, 2.4999998, 2.5000002, 0.25, 0.26, 0.3, 1.0, 1e6, -3.0, 0.0]),
                   torch.linspace(0.2, 3.0, 5000)])
    T = 32
    z = OR.encoder_spikes(x, T).bool()                                       # [T, n]
    fired = z.any(dim=0)
    n = torch.where(fired, z.float().argmax(dim=0) + 1, torch.zeros_like(z[0], dtype=torch.int64))
    t1 = torch.arange(1, T + 1)[:, None]
    expect = fired[None, :] & ((t1 % n.clamp(min=1)[None, :]) == 0)
    assert torch.equal(z, expect)
    assert int(n.max()) >= 20 and int((n == 1).sum()) > 0 and int((~fired).sum()) > 0   # long periods, every-step neurons and silent ones all present


def test_encoder_threshold_table_against_the_oracle_encoder():
    """The HIP encoders emit period planes by comparing the input with a table of thresholds (csrc/snn_common.h: THRESHOLD FORM):
    first spike at or before step t  <=>  x >= th[t].  The table comes from the library (host code: no GPU needed); here every
    float within 300 ulps of each of the 32 thresholds - and a coarse sweep in between - goes through the ORACLE's encoder."""
    import ctypes as C
    from snn_automotive_object_detection_amd import _lib, ops
    from oracle import snn_oracle as OR
    lib = _lib.load()
    p = ops.make_params(ops.LIFParameters(v_th=torch.tensor(0.25)), ops.LIFParameters(alpha=100, v_th=torch.tensor(0.1)))
    th = (C.c_float * 32)()
    assert lib.snn_debug_encoder_thresholds(C.byref(p), th) == 1
    th = np.array(list(th), dtype=np.float32)
    assert (np.diff(th) < 0).all() and th[0] == np.float32(2.5000002) and th[-1] > 0.25        # strictly decreasing towards v_th = 0.25
    bits = th.view(np.uint32)
    xs = np.concatenate([(b + np.arange(-300, 301)).astype(np.uint32).view(np.float32) for b in bits] +
                        [np.linspace(0.2, 3.0, 4001, dtype=np.float32), np.array([0.0, -1.0, 1e30, np.inf], dtype=np.float32)])
    z = OR.encoder_spikes(torch.from_numpy(xs.copy()), 32).bool().numpy()                       # [32, n]
    fired_by = np.logical_or.accumulate(z, axis=0)                                              # first spike at or before step t
    expect = xs[None, :] >= th[:, None]
    assert np.array_equal(fired_by, expect)


def test_encoder_on_non_finite_and_extreme_inputs_kat():
    """Norse's encoder resets ARITHMETICALLY, v - z * (v - v_reset) (lif_current_encoder; /root/reference/rpn.py:101,
    faster_rcnn.py:494): a +inf feature spikes ONCE and is NaN ever after; -inf and NaN never spike; huge finite values and FLT_MAX
    spike every step; -0.0 never.  The HIP encoders reset by selection: they agree on all of these EXCEPT +inf, which they turn into a
    period-1 neuron (documented in INTEGRATION.md; tests/test_gpu_exactness.py asserts the documented behaviour and that
    SNN_ENC_GENERIC=1 reproduces this table)."""
    from oracle import snn_oracle as OR
    x = torch.tensor([float("inf"), float("-inf"), float("nan"), 3e38, -0.0, 3.4028235e38])
    z = OR.encoder_spikes(x, 8)
    assert z[:, 0].tolist() == [1.0, 0, 0, 0, 0, 0, 0, 0]
    assert float(z[:, 1].sum()) == 0 and float(z[:, 2].sum()) == 0 and float(z[:, 4].sum()) == 0
    assert z[:, 3].tolist() == [1.0] * 8 and z[:, 5].tolist() == [1.0] * 8
    # the library's threshold table classifies them the same way except +inf (first spike at step 0 -> period 1)
    import ctypes as C
    from snn_automotive_object_detection_amd import _lib, ops
    p = ops.make_params(ops.LIFParameters(v_th=torch.tensor(0.25)), ops.LIFParameters(alpha=100, v_th=torch.tensor(0.1)))
    th = (C.c_float * 32)()
    assert _lib.load().snn_debug_encoder_thresholds(C.byref(p), th) == 1
    with np.errstate(invalid="ignore"):
        first_by_0 = x.numpy() >= np.float32(th[0])
    assert first_by_0.tolist() == [True, False, False, True, False, True]


# ---- neuron constants other than the reference's: answers worked out by hand (decimal arithmetic; none produced by the restatement) ---------
def _K(**kw):
    from oracle import snn_oracle as OR
    return OR.NeuronConstants(**kw)


def test_default_neuron_constants_are_the_reference_values():
    from oracle import snn_oracle as OR
    k = OR.NeuronConstants()
    assert tuple(k) == (0.25, 0.1, 0.0, 0.0, 0.001, 100.0, 200.0) and k == OR.DEFAULT_CONSTANTS and hash(k) == hash(OR.NeuronConstants())
    assert 1.0 / 1e-2 == 100.0 and 1.0 / 5e-3 == 200.0
    assert k.ca == float(np.float32(0.1)) and k.cb == float(np.float32(-0.2))
    # the parameter tuples the cells get are the ones the fixed call sites used to build, value for value
    p = k.lif_parameters(k.v_th_lif)
    q = NR.LIFParameters(alpha=100, v_th=torch.tensor(0.1))
    for name in ("tau_syn_inv", "tau_mem_inv", "v_leak", "v_th", "v_reset"):
        a, b = getattr(p, name), getattr(q, name)
        assert a.dtype == b.dtype == torch.float32 and a.dim() == 0 and torch.equal(a, b), name
    li = k.li_parameters()
    for name in ("tau_syn_inv", "tau_mem_inv", "v_leak"):
        assert torch.equal(getattr(li, name), getattr(NR.LIParameters(), name))


def test_encoder_with_a_reset_potential_kat():
    """v_reset = -0.05, v_th = 0.25, dt * tau_mem_inv = 0.1, constant input 1: v = 0.1, 0.19, 0.271 -> spike, v - (v + 0.05) = -0.05;
    then -0.05 + 0.1 * 1.05 = 0.055, 0.1495, 0.23455, 0.311095 -> spike: the first spike after 3 steps, then every 4 (every 3 at
    v_reset = 0).  The membrane after a spike is the fp32 value of v - (v - v_reset), which is NOT the float -0.05 for every v."""
    from oracle import snn_oracle as OR
    k = _K(v_reset=-0.05)
    z = OR.encoder_spikes(torch.ones(1), 11, k)[:, 0]
    assert z.tolist() == [0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1]
    assert OR.encoder_spikes(torch.ones(1), 11)[:, 0].tolist() == [0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0]
    p, v, vs = k.lif_parameters(k.v_th_enc), torch.zeros(1), []
    for _ in range(7):
        _, v = NR.lif_current_encoder(torch.ones(1), v, p, k.dt)
        vs.append(float(v))
    np.testing.assert_allclose(vs, [0.1, 0.19, -0.05, 0.055, 0.1495, 0.23455, -0.05], atol=1e-6)
    # the arithmetic reset, in numpy's fp32: v = 0.9 crosses at once; 0.9f + 0.05f rounds, and 0.9f minus that is one ulp off -0.05f
    f = np.float32
    v1 = f(f(0.0) + f(f(0.1) * f(f(f(0.0) - f(0.0)) + f(9.0))))
    want = f(v1 - f(v1 - f(-0.05)))
    z, v = NR.lif_current_encoder(torch.full((1,), 9.0), torch.zeros(1), p, k.dt)
    assert float(z) == 1.0 and np.float32(float(v)).view(np.uint32) == want.view(np.uint32)
    assert want != f(-0.05)                                           # (so "reset to exactly v_reset" is a different encoder)


def test_encoder_starts_at_zero_not_at_the_rest_potential_kat():
    """v_leak = 0.05, input 2.4: from v = 0 (rpn.py:93) the membrane is 0.1 * 2.45 = 0.245 < 0.25, then 0.245 + 0.1 * 2.205 = 0.4655 ->
    spike, reset to v - (v - 0) = 0: spikes at steps 1, 3, 5.  From v = v_leak it would be 0.05 + 0.1 * 2.4 = 0.29: a spike at step 0."""
    from oracle import snn_oracle as OR
    assert OR.encoder_spikes(torch.full((1,), 2.4), 6, _K(v_leak=0.05))[:, 0].tolist() == [0, 1, 0, 1, 0, 1]
    assert OR.encoder_spikes(torch.full((1,), 2.4), 6)[:, 0].tolist() == [0, 1, 0, 1, 0, 1]          # (0.24, 0.456: the same train at v_leak = 0)
    assert OR.encoder_spikes(torch.full((1,), 2.46), 3, _K(v_leak=0.05))[:, 0].tolist() == [1, 1, 1]  # 0.1 * 2.51 = 0.251
    assert OR.encoder_spikes(torch.full((1,), 2.46), 3)[:, 0].tolist() == [0, 1, 0]                   # 0.246; 0.246 + 0.2214


def test_lif_rest_potential_above_threshold_fires_at_step_0_kat():
    """v_leak = 0.2 > v_th = 0.1: the cell starts at v = v_leak, so v_dec = 0.2 at step 0 -> spike, v = v_reset = 0.  Without input the
    membrane then climbs back towards the rest potential, 0.2 (1 - 0.9^n) = 0.02, 0.038, 0.0542, 0.06878, 0.081902, 0.0937118,
    0.10434062 -> the next spike at step 7.  With input 1: i = 1, 1.8, 2.44, 2.952 and v_dec = 0.12, 0.2, 0.264: a spike every step."""
    from oracle import snn_oracle as OR
    k = _K(v_leak=0.2)
    z, state, vdec = OR.lif_scan_from_currents(torch.zeros(9, 1), constants=k)
    assert z[:, 0].tolist() == [1, 0, 0, 0, 0, 0, 0, 1, 0]
    np.testing.assert_allclose(vdec[:8, 0].numpy(), [0.2, 0.02, 0.038, 0.0542, 0.06878, 0.081902, 0.0937118, 0.10434062], atol=1e-6)
    z, state, vdec = OR.lif_scan_from_currents(torch.ones(4, 1), constants=k)
    assert z[:, 0].tolist() == [1, 1, 1, 1]
    np.testing.assert_allclose(vdec[:, 0].numpy(), [0.2, 0.12, 0.2, 0.264], atol=1e-6)
    np.testing.assert_allclose([float(state.v), float(state.i)], [0.0, 2.952], atol=1e-6)
    # a threshold below the rest potential 0 does the same: v_dec = 0 > -0.05 at step 0
    assert OR.lif_scan_from_currents(torch.zeros(2, 1), constants=_K(v_th_lif=-0.05))[0][:, 0].tolist() == [1, 1]
    assert OR.lif_scan_from_currents(torch.zeros(2, 1))[0][:, 0].tolist() == [0, 0]


def test_lif_rest_and_reset_potentials_kat():
    """v_leak = 0.04, v_reset = -0.03, v_th = 0.1, input 0.2 every step, (z, v, i) after each step:
    v_dec = 0.04;  0.04 + 0.1 (0 + 0.2) = 0.06;  0.06 + 0.1 (-0.02 + 0.36) = 0.094;  0.094 + 0.1 (-0.054 + 0.488) = 0.1374 -> spike, v = -0.03;
    -0.03 + 0.1 (0.07 + 0.5904) = 0.03604;  i = 0.2, 0.36, 0.488, 0.5904, 0.67232"""
    k = _K(v_leak=0.04, v_reset=-0.03)
    cell = NR.LIFCell(p=k.lif_parameters(k.v_th_lif), dt=k.dt)
    state, out = None, []
    for _ in range(5):
        z, state = cell(torch.full((1,), 0.2), state)
        out.append((float(z), float(state.v), float(state.i)))
    expect = [(0, 0.04, 0.2), (0, 0.06, 0.36), (0, 0.094, 0.488), (1, -0.03, 0.5904), (0, 0.03604, 0.67232)]
    np.testing.assert_allclose(np.array(out), np.array(expect), atol=1e-6)


def test_time_step_and_time_constants_kat():
    """dt = 2 ms: ca = 0.2, cb = -0.4; LIF at v_th = 0.1 on input 1: v_dec = 0, 0.2 -> spike, 0.2 * 1.6 = 0.32 -> spike; i = 1, 1.6, 1.96.
    tau_mem_inv = 150, tau_syn_inv = 120 on the LI cell (jump first), input 1: i = 1, v = 0.15, i = 0.88; i = 1.88, v = 0.15 + 0.15 * 1.73 =
    0.4095, i = 1.6544; i = 2.6544, v = 0.4095 + 0.15 * 2.2449 = 0.746235: last 0.746235, sum over t 1.305735."""
    from oracle import snn_oracle as OR
    k = _K(dt=0.002)
    assert k.ca == float(np.float32(0.002) * np.float32(100.0)) and k.cb == float(-np.float32(0.002) * np.float32(200.0))
    z, state, vdec = OR.lif_scan_from_currents(torch.ones(3, 1), constants=k)
    assert z[:, 0].tolist() == [0, 1, 1]
    np.testing.assert_allclose(vdec[:, 0].numpy(), [0.0, 0.2, 0.32], atol=1e-6)
    np.testing.assert_allclose(float(state.i), 1.96, atol=1e-6)
    k = _K(tau_mem_inv=150.0, tau_syn_inv=120.0)
    assert k.ca == float(np.float32(0.001) * np.float32(150.0)) and k.cb == float(-np.float32(0.001) * np.float32(120.0))
    last, acc = OR.li_last_from_spikes(torch.ones(3, 1, 1), torch.ones(1, 1), constants=k)
    np.testing.assert_allclose([float(last), float(acc)], [0.746235, 1.305735], atol=1e-6)
    last, _ = OR.li_last_from_spikes(torch.ones(3, 1, 1), torch.ones(1, 1), "voltage_first", constants=k)
    np.testing.assert_allclose(float(last), 0.4095, atol=1e-6)      # (the input of step t reaches the membrane one step later)
    # the LI cells ignore the rest and reset potentials: v_leak = 0 there
    a, _ = OR.li_last_from_spikes(torch.ones(3, 1, 1), torch.ones(1, 1), constants=_K(v_leak=0.2, v_reset=-0.05))
    b, _ = OR.li_last_from_spikes(torch.ones(3, 1, 1), torch.ones(1, 1))
    assert torch.equal(a, b)
