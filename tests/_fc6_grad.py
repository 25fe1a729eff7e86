"""fc6's gradient: what tests/test_fc6_grad_cpu.py and tests/test_gpu_fc6_grad.py share (test infrastructure, host only but for
``module_case``).  The tile constants and the slab function of csrc/snn_spike_wgrad_x3.h are RESTATED here; the CPU file compares the
restatement with the library's size query, the GPU file draws its shapes from it."""
import numpy as np
import torch

from tests import _hidden_grad as HG

# csrc/snn_spike_wgrad_x3.h, restated
TN, TK, MB = 128, 256, 32              # outputs / inputs of a work-group's tile; reduction rows per stage
WAVE_N, WAVE_K, MMA_ROWS = 64, 128, 16  # a wave's tile; reduction rows of one matrix instruction
SLAB_ROWS, MAX_SLABS, FILL = 256, 32, 256
MAX_K, MAX_N, MAX_STEPS = 16384, 8192, 32
LDS_BYTES = 2 * (3 * TN * (2 * MB + 16) + (TK // 32) * (MB + 4) * 4)      # two buffers: three bf16 planes with 16 bytes of padding per row + the word image
WORK_GROUPS_PER_CU = 2                 # what DESIGN.md 4.16 states


def cdiv(a, b):
    return (a + b - 1) // b


def slabs(M: int, K: int, N: int):
    """(slab count, rows per slab): one slab when the output tiles alone fill the device, otherwise as many as it takes to fill it"""
    tiles = cdiv(N, TN) * cdiv(K, TK)
    want = 1 if tiles >= FILL else min(cdiv(FILL, tiles), cdiv(M, SLAB_ROWS), MAX_SLABS)
    per = cdiv(cdiv(M, want), MB) * MB
    return cdiv(M, per), per


def query_bytes(rows: int, K: int, N: int, Tp: int) -> int:
    if not (1 <= rows < 2 ** 31 and 1 <= K <= MAX_K and 1 <= N <= MAX_N and 1 <= Tp <= MAX_STEPS):
        return 0
    return 4 * min(min(cdiv(rows * Tp, SLAB_ROWS), MAX_SLABS) * N * K, FILL * TN * TK + N * K)


def li_torch(z, w, c: HG.Consts, order, dtype):
    """the LI readout of tests/_planes.li_fp64 in torch (differentiable): spikes [T, R, Hd], weights [n, Hd] -> last membrane [R, n]"""
    a, b = torch.tensor(c.a, dtype=dtype), torch.tensor(-c.b, dtype=dtype)
    v = torch.zeros((z.shape[1], w.shape[0]), dtype=dtype)
    i = torch.zeros_like(v)
    for t in range(z.shape[0]):
        cur = z[t] @ w.t()
        if order == "jump_first":
            i = i + cur; v = v + a * (i - v); i = i - b * i
        else:
            v = v + a * (i - v); i = i - b * i + cur
    return v


def loss_of(kind, labels, targets):
    from tests import _head_losses as HL
    if kind == "quadratic":
        return lambda cls, box: 0.5 * (cls * cls).sum() + 0.25 * (box * box).sum()
    return lambda cls, box: sum(HL.det_loss(cls, box, labels, targets.to(box.dtype)))


def two_layer_restated(cur6, z6, cur7, z7, w7, w_out, g_out, c: HG.Consts, alpha, order, dtype=torch.float64):
    """d_cur6 [T - 2, R, Hd] by the restatement the GPU chain follows: gu = g_out W_out; d_cur7 = adjoint over the window T - 1;
    gz6 = d_cur7 W7; d_cur6 = adjoint over the window T - 2.  cur6, cur7 [T, ...] and z6, z7 [T, ...] of a T-step pass"""
    T = cur7.shape[0]
    gu = g_out.to(dtype) @ w_out.to(dtype)
    d_cur7 = HG.adjoint(cur7[:T - 1], z7, c, alpha, gu=gu, kappa=HG.kappa(c, T, order, dtype), dtype=dtype)
    gz6 = d_cur7 @ w7.to(dtype)
    return HG.adjoint(cur6[:T - 2], z6[:T - 1], c, alpha, gz=gz6, dtype=dtype), d_cur7


def cpu_fc6_grad(enc, spk6, spk7, w6, w7, w_cls, w_box, T, order, loss, dtype, n_cls):
    """autograd on the CPU in `dtype`: the oracle's encoder raster through fc6, a SuperSpike lif6, fc7, a SuperSpike lif7 (both teacher-forced
    with the oracle's rasters, as the backward under test is), the LI readout and the loss -> (d loss / d fc6, d loss / d fc7)"""
    a = w6.to(dtype).clone().requires_grad_()
    b = w7.to(dtype).clone().requires_grad_()
    cur6 = enc[:T - 2].to(dtype) @ a.t()
    z6 = HG.lif_forward_autograd(cur6, HG.REFERENCE, 100.0, forced=spk6[:T - 1])          # [T - 1]
    cur7 = z6 @ b.t()
    z7 = HG.lif_forward_autograd(cur7, HG.REFERENCE, 100.0, forced=spk7)                  # [T]
    out = li_torch(z7, torch.cat([w_cls, w_box]).to(dtype), HG.REFERENCE, order, dtype)
    loss(out[:, :n_cls], out[:, n_cls:]).backward()
    return a.grad, b.grad


def roi_inputs(dev, R, seed, C_in):
    from snn_automotive_object_detection_amd.stock.roi_align import MultiScaleRoIAlign
    g = torch.Generator().manual_seed(seed)
    feats = {str(i): (torch.randn((2, C_in, h, w), generator=g) * 2.0).to(dev) for i, (h, w) in enumerate([(24, 40), (12, 20), (6, 10), (3, 5)])}
    boxes = []
    for k in (R - R // 2, R // 2):
        xy = torch.rand((k, 2), generator=g) * torch.tensor([120.0, 70.0])
        wh = torch.exp(torch.rand((k, 2), generator=g) * 3.0 + 1.0)
        boxes.append(torch.cat([xy, torch.minimum(xy + wh, torch.tensor([159.0, 95.0]))], dim=1).to(dev))
    return MultiScaleRoIAlign(["0", "1", "2", "3"], 7, 2).assign(feats, boxes, [(96, 160)] * 2)


def module_case(dev, feed, R, T, precision, C_in, Hd, n_cls):
    """the head, its call, and the oracle's trace on the same inputs; fc6 and fc7 on the "wide" dyadic grid of tests/_exact_grid.py"""
    import snn_automotive_object_detection_amd as S
    from oracle import snn_oracle as OR
    from snn_automotive_object_detection_amd import ops
    from tests import _exact_grid as G
    seed = 300 + R + T
    if feed == "rows":
        case = G.det_case(R, C_in, Hd, n_cls, T, seed)
        w6, w7, w_cls, w_box, tr, x = case["w6"], case["w7"], case["w_cls"], case["w_bbox"], case["trace"], case["x"].to(dev)
        call = lambda mod: mod(x)
    else:
        torch.manual_seed(seed)
        d0 = S.FastRCNNPredictorSNNFull(C_in * 49, Hd, n_cls, T)
        w6, w7 = G._grid(d0.fc6.weight.detach().clone(), "wide", seed, {}), G._grid(d0.fc7.weight.detach() * 3.0, "wide", seed + 1, {})
        w_cls, w_box = d0.cls_score.weight.detach().clone(), d0.bbox_pred.weight.detach().clone()
        flist, scales, rois, lvl = roi_inputs(dev, R, seed, C_in)
        p = ops.make_params(d0.p_enc, d0.p_lif)
        _, pooled = ops.roi_align_encode(flist, scales, rois[:, 1:5], rois[:, 0], lvl, T, p, want_pooled=True)
        with torch.no_grad():
            _, _, tr = OR.det_head_forward(pooled.cpu().view(R, C_in, 7, 7), w6, w7, w_cls, w_box, T, trace=True)
        call = lambda mod: mod.forward_roialign(flist, scales, rois, lvl)
    d = S.FastRCNNPredictorSNNFull(C_in * 49, Hd, n_cls, T).to(dev)
    d.precision = precision
    d.load_state_dict({"fc6.weight": w6, "fc7.weight": w7, "cls_score.weight": w_cls, "bbox_pred.weight": w_box})
    return d, call, tr, (w6, w7, w_cls, w_box)


def one_hot_case(rows, Tp, K, N, seed):
    """every column k has exactly one spike over all M = T' rows reduction rows, at row m(k); d_cur drawn from full 24-bit mantissas at scales
    2^0, 2^-20 and 2^-100, exact powers of two, and values whose lo part is a bf16 SUBNORMAL -> (a_rows int32, d fp32 [T', rows, N], m int [K])"""
    rng = np.random.default_rng(seed)
    M = Tp * rows
    m = rng.integers(0, M, size=K)
    bits = np.zeros((M, K), dtype=bool)
    bits[m, np.arange(K)] = True
    a_rows = HG.pack_bits(torch.from_numpy(bits.reshape(Tp, rows, K)), set_padding=True)
    mant = (rng.integers(2 ** 23, 2 ** 24, size=(M, N)) | 1).astype(np.float64) * np.where(rng.random((M, N)) < 0.5, -1.0, 1.0)     # 24 significant bits
    kind = rng.integers(0, 5, size=(M, N))
    d = np.zeros((M, N), dtype=np.float64)
    for k, e in ((0, -23), (1, -43), (2, -123)):                      # |d| about 2^0, 2^-20, 2^-100
        d = np.where(kind == k, mant * 2.0 ** e, d)
    d = np.where(kind == 3, np.ldexp(1.0, rng.integers(-120, 100, size=(M, N))), d)
    # lo = bits 2^-128 .. 2^-133 under hi at 2^-112 .. 2^-119 and mid at 2^-120 .. 2^-127: a bf16 subnormal (below 2^-126), exact in fp32
    d = np.where(kind == 4, mant * 2.0 ** -133, d)
    d32 = d.astype(np.float32)
    assert np.array_equal(d32.astype(np.float64), d)
    return a_rows, torch.from_numpy(d32.reshape(Tp, rows, N)), m


def split3(x: np.ndarray):
    """the three bf16 planes of fp32 values, as fp32 arrays: hi = rn(x), mid = rn(x - hi), lo = rn(x - hi - mid)"""
    def rn(v):
        u = v.astype(np.float32).view(np.uint32).astype(np.uint64)
        u = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
        return u.astype(np.uint32).view(np.float32)
    hi = rn(x)
    r1 = (x - hi).astype(np.float32)
    mid = rn(r1)
    r2 = (r1 - mid).astype(np.float32)
    return hi, mid, rn(r2)
