"""Channels-last (NHWC) feature maps straight into both spiking heads (include/snn_hip.h: SNN_FEAT_NHWC on the *_typed entry points).

Layout does not change a value, so the yardstick of every check is the EXISTING path on x.contiguous() with the same dtype - which the rest
of the suite pins to the oracle - and the comparison is torch.equal: outputs, sums, spike counts and rates, hidden spike planes, and the
encoder's raw and compressed planes in the workspace.  The channels-last path is never its own yardstick."""
import ctypes as C

import pytest
import torch

from tests._planes import head_det_planes, head_rpn_planes
from tests.test_gpu_roialign import _setup

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
IDS = ["f32", "f16", "bf16"]
CL = torch.channels_last


def _params():
    from snn_automotive_object_detection_amd import ops
    return ops.make_params(ops.LIFParameters(v_th=torch.tensor(0.25)), ops.LIFParameters(alpha=100, v_th=torch.tensor(0.1)))


def _calls():
    from snn_automotive_object_detection_amd import ops
    return dict(ops.feature_calls)


def _nhwc_ran(before, n=1, no_typed=0):
    """n calls ran on the channels-last path since `before`, and `no_typed` answered "no kernel for this plan\""""
    now = _calls()
    assert now["nhwc"] - before["nhwc"] == n and now["no_typed_kernel"] - before["no_typed_kernel"] == no_typed, (before, now)


def _same(a, b):
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), float((a.float() - b.float()).abs().max())
    else:
        assert a == b


def _cl(x):
    """the same values, dense in channels_last"""
    from snn_automotive_object_detection_amd import ops
    y = x.contiguous(memory_format=CL)
    assert ops.feat_layout(y) in ("nhwc", "either") and torch.equal(x, y)
    return y


# ---- 1. encoder planes, stage level ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("T", [4, 8, 16])
@pytest.mark.parametrize("shape", [(2, 64, 13, 19), (2, 256, 5, 3), (1, 32, 1, 70), (1, 48, 7, 10)])   # odd H W; H W < 64; one row; C % 32 != 0
def test_encode_on_channels_last_map_equals_the_contiguous_call(gpu_device, dtype, T, shape):
    from snn_automotive_object_detection_amd import ops
    x = (torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape) + T)) * 1.5).to(gpu_device).to(dtype)
    ref = ops.encode_nchw(x.contiguous(), T, _params())
    assert int((ref != 0).sum()) > 0
    before = _calls()
    got = ops.encode_nchw(x.to(memory_format=CL), T, _params())
    if shape[1] % 32:
        _nhwc_ran(before, 0, 1)                              # no channels-last kernel: converted, and still the same planes
    else:
        _nhwc_ran(before, 1, 0)
    _same(got, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("knob", ["SNN_STAGE_PERIODS=1", "SNN_ENC_GENERIC=1", "SNN_ENC_QUANT=0"])
def test_other_encoder_modes_of_the_channels_last_kernels(gpu_device, monkeypatch, dtype, knob):
    """the threshold (period-plane) and op-for-op instantiations of k_encode_nhwc, and the recurrence / op-for-op ones of k_encode_levels_nhwc"""
    from snn_automotive_object_detection_amd import ops
    monkeypatch.setenv(*knob.split("="))
    x = (torch.randn((2, 96, 7, 10), generator=torch.Generator().manual_seed(3)) * 1.5).to(gpu_device).to(dtype)       # 3 words: a partly filled word block
    ref = ops.encode_nchw(x, 8, _params())
    before = _calls()
    got = ops.encode_nchw(_cl(x), 8, _params())
    _nhwc_ran(before)
    assert int((ref != 0).sum()) > 0
    _same(got, ref)
    if knob != "SNN_STAGE_PERIODS=1":
        m, feats = _rpn(gpu_device, 64, 8, dtype)
        ref = m(feats)
        ref_planes = head_rpn_planes(gpu_device, 8, 64)
        before = _calls()
        got = m([_cl(f) for f in feats])
        _nhwc_ran(before)
        _same(got, ref)
        _same(head_rpn_planes(gpu_device, 8, 64), ref_planes)


# ---- 2. RPN head -----------------------------------------------------------------------------------------------------------------------
def _rpn(dev, C_, T, dtype, seed=0, sizes=((13, 19), (7, 10))):
    import snn_automotive_object_detection_amd as S
    torch.manual_seed(seed)
    m = S.RPNHeadSNN(C_, 3, T).to(dev)
    with torch.no_grad():
        m.shared_conv.weight.mul_(4.0)                       # (so that the shared LIF fires)
    g = torch.Generator().manual_seed(seed + 1)
    feats = [(torch.randn((2, C_, h, w), generator=g) * 1.5).to(dev).to(dtype) for h, w in sizes]
    return m, feats


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C_,T", [(256, 8), (256, 4), (64, 12)])      # fold + compressed planes + FAT conv; dense conv, no fold; narrow head
def test_rpn_head_on_channels_last_maps_equals_the_contiguous_path(gpu_device, dtype, C_, T):
    m, feats = _rpn(gpu_device, C_, T, dtype)
    cl = [_cl(f) for f in feats]
    for rates in (False, True):
        m.spike_rates = rates
        ref = m(feats)
        ref_planes = head_rpn_planes(gpu_device, T, C_)
        ref_counts = m.last_spike_counts.clone() if rates else None
        before = _calls()
        got = m(cl)
        _nhwc_ran(before)
        _same(got, ref)
        _same(head_rpn_planes(gpu_device, T, C_), ref_planes)
        assert int((ref_planes != 0).sum()) > 0
        if rates:
            _same(m.last_spike_counts, ref_counts)
        # (rates on: {T': (logits, bbox, rate rows)} through the count buffers of snn_rpn_head_forward_readouts_typed)
        ref = m.forward_readouts(feats, (3, 5, 8))
        before = _calls()
        got = m.forward_readouts(cl, (3, 5, 8))
        _nhwc_ran(before)
        assert set(got) == set(ref) == {3, 5, 8}
        for t in (3, 5, 8):
            assert len(ref[t]) == (3 if rates else 2)
            _same(got[t], ref[t])
    m.spike_rates = False


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("precision,C_", [("f32", 64), ("mxfp6", 128)])      # row-major planes without a halo; a halo without word-major planes
def test_rpn_head_other_precisions_on_channels_last_maps(gpu_device, dtype, precision, C_):
    T = 8
    m, feats = _rpn(gpu_device, C_, T, dtype)
    m.precision = precision
    cl = [_cl(f) for f in feats]
    for rates in (False, True):
        m.spike_rates = rates
        ref = m(feats)
        ref_planes = head_rpn_planes(gpu_device, T, C_)
        ref_counts = m.last_spike_counts.clone() if rates else None
        before = _calls()
        got = m(cl)
        _nhwc_ran(before)
        _same(got, ref)
        _same(head_rpn_planes(gpu_device, T, C_), ref_planes)
        assert int((ref_planes != 0).sum()) > 0
        if rates:
            _same(m.last_spike_counts, ref_counts)
    m.spike_rates = False


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_rpn_levels_share_a_layout(gpu_device, dtype):
    from snn_automotive_object_detection_amd import ops
    m, feats = _rpn(gpu_device, 64, 8, dtype, sizes=((13, 19), (7, 10), (1, 1)))
    ref = m(feats)
    # a 1 x 1 level has the same bytes in both layouts: beside two channels-last levels the call still takes the channels-last path
    assert ops.feat_layout(feats[2]) == "either"
    before = _calls()
    _same(m([_cl(feats[0]), _cl(feats[1]), feats[2]]), ref)
    _nhwc_ran(before)
    # one contiguous level beside one channels-last level of the same H W > 1: all levels take the conversion, without an error
    m2, f2 = _rpn(gpu_device, 64, 8, dtype, sizes=((7, 10), (7, 10)))
    ref = m2(f2)
    before = _calls()
    _same(m2([f2[0], _cl(f2[1])]), ref)
    _nhwc_ran(before, 0, 0)


# ---- 3. RoIAlign-fed detector head --------------------------------------------------------------------------------------------------------
def _det(dev, C_, Hd, K, T, seed):
    import snn_automotive_object_detection_amd as S
    torch.manual_seed(seed)
    head = S.FastRCNNPredictorSNNFull(C_ * 49, Hd, K, T).to(dev)
    with torch.no_grad():
        head.fc6.weight.mul_(4.0)
        head.fc7.weight.mul_(4.0)
    assert head.fc6_inner() == 49
    return head


def _det_run(dev, head, flist, scales, rois, lvl, C_, Hd, T, nhwc):
    """one plain and one spike-rate pass: (outputs, lif6 / lif7 planes, every raw encoder plane, the compressed planes, counts).  The
    encoder's planes lie where tests/test_gpu_roialign.py::test_roialign_encoder_fold_writes_the_same_planes locates them (det_ws_layout: the
    planes fc6 reads at the front, then the side buffers); the workspace is poisoned first, so bytes nobody wrote compare equal"""
    from snn_automotive_object_detection_amd import ops
    Rn = int(rois.shape[0])
    al = lambda v: (v + 255) // 256 * 256
    Dw, Tc = C_ * 49 // 32, T - 2
    o_cur = al(T * Rn * Dw * 4)
    raw_bytes, cmp_bytes = Tc * Dw * Rn * 4, (Tc - 2) * (Dw // 2) * 4 * Rn * 4
    head.spike_rates = False
    head.forward_roialign(flist, scales, rois, lvl)             # (sizes the workspace)
    ops._WS.get(dev, 1)[: o_cur + cmp_bytes].fill_(0x5a)
    before = _calls()
    out = head.forward_roialign(flist, scales, rois, lvl)
    if nhwc:
        _nhwc_ran(before)
    ws = ops._WS.get(dev, 1)
    res = [tuple(o.clone() for o in out), head_det_planes(dev, T, Hd, Rn), ws[:raw_bytes].clone(), ws[o_cur: o_cur + cmp_bytes].clone()]
    head.spike_rates = True
    before = _calls()
    out = head.forward_roialign(flist, scales, rois, lvl)
    if nhwc:
        _nhwc_ran(before)
    res += [tuple(o.clone() for o in out), [c.clone() for c in head.last_spike_counts], head_det_planes(dev, T, Hd, Rn)]
    head.spike_rates = False
    return res


# (R = 37 / 38: a partly filled RoI group; T = 14: the spike-rate pass has a 13-plane window; T = 16: every window is beyond 12 planes - all raw, then
# k_compress_planes)
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("R,C_,Hd,K,T", [(38, 64, 64, 3, 6), (130, 128, 64, 3, 14), (60, 192, 64, 3, 8), (300, 256, 128, 9, 12), (37, 64, 64, 3, 16)])
def test_det_head_on_channels_last_maps_equals_the_contiguous_path(gpu_device, dtype, R, C_, Hd, K, T):
    from snn_automotive_object_detection_amd import ops
    pool, feats, boxes, shapes = _setup(gpu_device, R=R, C=C_, seed=R)
    feats = {k: (v * 1.5).to(dtype) for k, v in feats.items()}
    head = _det(gpu_device, C_, Hd, K, T, R + T)
    flist, scales, rois, lvl = pool.assign(feats, boxes, shapes)
    flist_cl, scales_cl, rois_cl, lvl_cl = pool.assign({k: _cl(v) for k, v in feats.items()}, boxes, shapes)
    assert all(ops.feat_layout(f) == "nhwc" for f in flist_cl) and all(ops.feat_layout(f) == "nchw" for f in flist)    # assign re-lays nothing
    ref = _det_run(gpu_device, head, flist, scales, rois, lvl, C_, Hd, T, False)
    got = _det_run(gpu_device, head, flist_cl, scales_cl, rois_cl, lvl_cl, C_, Hd, T, True)
    _same(got, ref)
    assert int((ref[2] != 0x5a).sum()) > 0 and int((ref[1][0] != 0).sum()) > 0 and any(int(c.sum()) > 0 for c in ref[5])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("C_,knob,precision", [(96, None, "bf16x3"), (64, "SNN_ROI_TAB=0", "bf16x3"), (64, None, "f32")],
                         ids=["C96", "roi_tab0", "f32_planes"])      # C % 64 != 0; the per-element kernels; row-major detector planes
def test_det_head_plan_without_a_channels_last_kernel_converts(gpu_device, monkeypatch, dtype, C_, knob, precision):
    """a launch plan with no channels-last RoIAlign kernel answers SNN_STATUS_NO_TYPED_KERNEL with nothing enqueued: the maps are converted to
    NCHW, the call runs again and gives what contiguous maps give - counted once under "no_typed_kernel", never under the key "nhwc".  """
    if knob:
        monkeypatch.setenv(*knob.split("="))
    pool, feats, boxes, shapes = _setup(gpu_device, R=38, C=C_, seed=C_)
    feats = {k: (v * 1.5).to(dtype) for k, v in feats.items()}
    head = _det(gpu_device, C_, 64, 3, 8, 9)
    head.precision = precision
    flist, scales, rois, lvl = pool.assign(feats, boxes, shapes)
    flist_cl = pool.assign({k: _cl(v) for k, v in feats.items()}, boxes, shapes)[0]
    for rates in (False, True):
        head.spike_rates = rates
        ref = head.forward_roialign(flist, scales, rois, lvl)
        ref_planes = head_det_planes(gpu_device, 8, 64, int(rois.shape[0]))
        ref_counts = [c.clone() for c in head.last_spike_counts] if rates else []
        before = _calls()
        got = head.forward_roialign(flist_cl, scales, rois, lvl)
        _nhwc_ran(before, 0, 1)
        _same(got, ref)
        _same(head_det_planes(gpu_device, 8, 64, int(rois.shape[0])), ref_planes)
        if rates:
            _same([c.clone() for c in head.last_spike_counts], ref_counts)
            assert any(int(c.sum()) > 0 for c in ref_counts)
    head.spike_rates = False
    ref = head.forward_roialign_readouts(flist, scales, rois, lvl, (3, 6, 8))
    before = _calls()
    got = head.forward_roialign_readouts(flist_cl, scales, rois, lvl, (3, 6, 8))
    _nhwc_ran(before, 0, 1)
    for t in (3, 6, 8):
        _same(got[t], ref[t])


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_det_head_on_borders_and_tiny_channels_last_maps(gpu_device, dtype):
    """the inputs of tests/test_gpu_roialign.py::test_table_driven_kernel_on_borders_and_tiny_maps: clamped columns / rows, samples outside the
    map, a 2-pixel-wide level"""
    from snn_automotive_object_detection_amd.stock.roi_align import MultiScaleRoIAlign
    g = torch.Generator().manual_seed(9)
    sizes = [(16, 16), (8, 8), (4, 4), (2, 2)]
    feats = {str(i): (torch.randn((1, 64, h, w), generator=g) * 1.5).to(gpu_device).to(dtype) for i, (h, w) in enumerate(sizes)}
    b = torch.tensor([[0.0, 0.0, 64.0, 64.0], [60.0, 60.0, 64.0, 64.0], [63.5, 0.0, 64.0, 64.0], [-30.0, -30.0, 10.0, 10.0],
                      [0.0, 62.0, 64.0, 66.0], [10.0, 10.0, 500.0, 500.0], [63.9, 63.9, 64.0, 64.0], [0.0, 0.0, 3.0, 3.0]])
    boxes = [torch.cat([b, torch.rand((40, 4), generator=g) * 32 + torch.tensor([0.0, 0.0, 32.0, 32.0])]).to(gpu_device)]
    pool = MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2)
    head = _det(gpu_device, 64, 128, 5, 8, 2)
    flist, scales, rois, lvl = pool.assign(feats, boxes, [(64, 64)])
    ref = _det_run(gpu_device, head, flist, scales, rois, lvl, 64, 128, 8, False)
    flist_cl = pool.assign({k: _cl(v) for k, v in feats.items()}, boxes, [(64, 64)])[0]
    got = _det_run(gpu_device, head, flist_cl, scales, rois, lvl, 64, 128, 8, True)
    _same(got, ref)
    assert any(int(c.sum()) > 0 for c in ref[5])


@pytest.mark.parametrize("dtype", DTYPES[1:], ids=IDS[1:])
def test_det_head_keeps_half_subnormals_of_channels_last_maps(gpu_device, dtype):
    """half-precision SUBNORMALS beside ordinary values: the widening of the channels-last loads keeps them as the contiguous path's does"""
    pool, feats, boxes, shapes = _setup(gpu_device, R=38, C=64, seed=38)
    g = torch.Generator().manual_seed(11)
    top = 0x3FF if dtype == torch.float16 else 0x7F                            # mantissa bits only: exponent field 0
    half = {}
    for k, v in feats.items():
        sub = (torch.randint(1, top + 1, v.shape, generator=g, dtype=torch.int16) | (torch.randint(0, 2, v.shape, generator=g, dtype=torch.int16) << 15)).view(dtype)
        assert float(sub.float().abs().max()) < float(torch.finfo(dtype).tiny)
        pick = torch.rand(v.shape, generator=g) < 0.5
        half[k] = torch.where(pick.to(gpu_device), sub.to(gpu_device), (v * 1.5).to(dtype))
    head = _det(gpu_device, 64, 64, 3, 8, 5)
    flist, scales, rois, lvl = pool.assign(half, boxes, shapes)
    ref = _det_run(gpu_device, head, flist, scales, rois, lvl, 64, 64, 8, False)
    flist_cl = pool.assign({k: _cl(v) for k, v in half.items()}, boxes, shapes)[0]
    got = _det_run(gpu_device, head, flist_cl, scales, rois, lvl, 64, 64, 8, True)
    _same(got, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_det_head_readouts_on_channels_last_maps(gpu_device, dtype):
    pool, feats, boxes, shapes = _setup(gpu_device, R=38, C=64, seed=4)
    feats = {k: (v * 1.5).to(dtype) for k, v in feats.items()}
    head = _det(gpu_device, 64, 64, 3, 12, 7)
    flist, scales, rois, lvl = pool.assign(feats, boxes, shapes)
    flist_cl = pool.assign({k: _cl(v) for k, v in feats.items()}, boxes, shapes)[0]
    for rates in (False, True):
        head.spike_rates = rates
        ref = head.forward_roialign_readouts(flist, scales, rois, lvl, (6, 9, 12))
        before = _calls()
        got = head.forward_roialign_readouts(flist_cl, scales, rois, lvl, (6, 9, 12))
        _nhwc_ran(before)
        for t in (6, 9, 12):
            _same(got[t], ref[t])


# ---- 4. the C ABI ---------------------------------------------------------------------------------------------------------------------------
def test_layout_bit_at_the_c_abi(gpu_device):
    from snn_automotive_object_detection_amd import _lib, ops
    from snn_automotive_object_detection_amd._lib import snn_roi_level
    lib, p, dev = _lib.load(), _params(), gpu_device
    NHWC, s = _lib.FEAT_NHWC, torch.cuda.current_stream().cuda_stream
    vp = lambda t: C.c_void_p(t.data_ptr())
    # the bit on a row-fed entry: -1 (pooled rows have no layout)
    R, D, Hd, K, T = 8, 64 * 49, 64, 3, 6
    x = torch.randn((R, D), device=dev)
    w6, w7, wh = (torch.zeros(1 << 20, device=dev) for _ in range(3))
    out_c, out_b = torch.empty((R, K), device=dev), torch.empty((R, 4 * K), device=dev)
    ws = torch.empty(lib.snn_det_head_workspace_bytes(R, D, Hd, K, 4 * K, T, p.precision), dtype=torch.uint8, device=dev)
    tail = (C.byref(p), vp(w6), 0, vp(w7), vp(wh), vp(out_c), vp(out_b), None, None, None, None, vp(ws), ws.numel(), s)
    assert lib.snn_det_head_forward_k_typed(vp(x), NHWC, R, D, Hd, K, 4 * K, T, *tail) == -1
    assert b"row-fed" in lib.snn_last_error()
    steps = (C.c_int * 2)(3, 6)
    assert lib.snn_det_head_forward_readouts_typed(vp(x), NHWC | 1, R, D, Hd, K, 4 * K, steps, 2, *tail) == -1
    # a misaligned channels-last fp32 base: -1; an unknown bit: -1
    planes = torch.full((4, 2 * 15, 1), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    buf = torch.randn(2 * 32 * 15 + 4, device=dev)
    assert buf.data_ptr() % 16 == 0
    enc = lambda ptr, fdt: lib.snn_encode_nchw_typed(C.c_void_p(ptr), fdt, 2, 32, 3, 5, 4, C.byref(p), vp(planes), 2 * 15, s)
    assert enc(buf.data_ptr() + 4, NHWC) == -1 and b"16-byte aligned" in lib.snn_last_error()
    assert enc(buf.data_ptr(), 32) == -1 and b"unknown feat_dtype" in lib.snn_last_error()
    assert enc(buf.data_ptr(), NHWC | 32) == -1 and enc(buf.data_ptr(), NHWC | 3) == -1
    torch.cuda.synchronize()
    assert bool((planes == 0x5a5a5a5a).all())                  # (a refused call enqueues nothing)
    assert enc(buf.data_ptr(), NHWC) == 0
    want = ops.encode_nchw(buf[: 2 * 32 * 15].view(2, 3, 5, 32).permute(0, 3, 1, 2).contiguous(), 4, p)
    assert torch.equal(planes, want) and int((want != 0).sum()) > 0
    # the bit on snn_roi_align_encode_typed: "no typed kernel", and a poisoned output buffer stays as it was
    fmap = torch.randn((1, 64, 8, 8), device=dev)
    table = (snn_roi_level * 1)(snn_roi_level(fmap.data_ptr(), 8, 8, 0.25, 0))
    rois = torch.tensor([[2.0, 2.0, 20.0, 20.0]], device=dev)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.full((4, 1, 98), 0x5a5a5a5a, dtype=torch.int32, device=dev)
    call = lambda fdt: lib.snn_roi_align_encode_typed(table, fdt, 1, 64, vp(rois), vp(zero), vp(zero), 1, 4, C.byref(p), vp(out), 98, None, s)
    assert call(NHWC) == _lib.NO_TYPED_KERNEL and call(NHWC | 2) == _lib.NO_TYPED_KERNEL
    assert call(NHWC | 32) == -1
    torch.cuda.synchronize()
    assert bool((out == 0x5a5a5a5a).all())
    assert call(0) == 0
    torch.cuda.synchronize()
    assert not bool((out == 0x5a5a5a5a).all())


# ---- 5. module level --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector(gpu_device):
    import snn_automotive_object_detection_amd as S
    torch.manual_seed(0)
    m = S.create_model("cityscapes", 9, True, True, 0, False, False, num_steps_rpn=4, num_steps_detector=6)
    m.transform.min_size, m.transform.max_size = 256, 512
    m = m.to(gpu_device).eval()
    img = [torch.rand((3, 256, 512), generator=torch.Generator().manual_seed(1)).to(gpu_device)]
    with torch.no_grad():
        il, _ = m.transform(img)
        fm = m.backbone(il.tensors)
    return m, il, fm


def test_heads_on_channels_last_fpn_maps(gpu_device, detector):
    from snn_automotive_object_detection_amd import ops, static
    m, il, fm = detector
    fm_cl = type(fm)((k, v.contiguous(memory_format=CL)) for k, v in fm.items())
    assert all(ops.feat_layout(v) == "nhwc" for v in fm_cl.values())
    with torch.no_grad():
        props, _ = m.rpn(il, fm)
        dets, _ = m.roi_heads(fm, props, il.image_sizes)
        before = _calls()
        props_cl, _ = m.rpn(il, fm_cl)
        mid = _calls()
        dets_cl, _ = m.roi_heads(fm_cl, props_cl, il.image_sizes)
        after = _calls()
        assert mid["nhwc"] - before["nhwc"] >= 1 and after["nhwc"] - mid["nhwc"] >= 1 and after["no_typed_kernel"] == before["no_typed_kernel"], (before, mid, after)
        _same(props_cl, props)
        _same(dets_cl, dets)
        assert props[0].shape[0] > 0
        ref = static.heads_padded(m, fm, il)
        before = _calls()
        got = static.heads_padded(m, fm_cl, il)
        after = _calls()
        assert after["nhwc"] - before["nhwc"] >= 2 and after["no_typed_kernel"] == before["no_typed_kernel"], (before, after)
        _same(got, ref)
        assert int(ref["roi_counts"].sum()) > 0


def test_padded_path_on_channels_last_maps_never_synchronises(gpu_device, detector):
    from snn_automotive_object_detection_amd import static
    m, il, fm = detector
    fm_cl = type(fm)((k, v.contiguous(memory_format=CL)) for k, v in fm.items())
    with torch.no_grad():
        ref = static.heads_padded(m, fm_cl, il)                 # packs the weights, sizes the workspaces (host synchronisations)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = static.heads_padded(m, fm_cl, il)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    _same(out, ref)
