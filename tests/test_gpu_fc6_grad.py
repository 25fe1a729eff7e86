"""fc6's gradient on the GPU: the spike-fed weight gradient on the bf16 matrix cores and SuperSpike through lif7 and lif6 into fc6
(include/snn_hip.h: snn_spike_wgrad_bf16x3; fc6_grad.py).

  1. integer grid       sums that are exact in every order -> bit equality with the float64 expectation, at every tile edge of the kernel, past the
                        fp32 entry's K limit and at fc6's width; ldd > N with NaN padding, padding bits set, accumulate, poisoned scratch, run to run
  2. one-hot            a column with one spike returns d_cur bit for bit: the three-plane split, its order, bf16 subnormals
  3. N(0, 1)            inside the header's bound
  4. guard bands        every operand between guard bands, the scratch told exactly its queried size
  5. the module         train_fc6 on dyadic fc6 / fc7 (zero flips by construction): outputs unchanged, the three upper gradients bit-equal to the
                        train_fc7 path, fc6.weight.grad against fp64 autograd within 4 x the error of fp32 CPU autograd
  6. graph capture      the whole backward chain captured once, replayed on a second data set
  7. end to end         one fine-tuning step of the small model through readout_losses"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _fc6_grad as F6
from tests import _graph_capture as GC
from tests import _hidden_grad as HG
from tests import _taps as TP
from tests import _ws_state as W

pytestmark = pytest.mark.gpu
RATIOS = {}                       # what the file logs: the largest observed error / tolerance ratios


def _L():
    from snn_automotive_object_detection_amd import _lib
    return _lib


def _params(c: HG.Consts, li_order="jump_first"):
    L = _L()
    return L.snn_params(c.a, c.b, c.v_leak, c.v_reset, 0.25, c.th, {"jump_first": 0, "voltage_first": 1}[li_order], L.PRECISIONS["bf16x3"])


def _note(key, value):
    RATIOS[key] = max(RATIOS.get(key, 0.0), float(value))


# ---- 1. the integer grid ----------------------------------------------------------------------------------------------------------------------
W_ROWS, W_DIMS, W_T = (1, 15, 16, 17, 63, 65, 1031), (32, 96, 160), (1, 3, 10)
DENSITIES = (0.02, 0.3, 1.0)


def _poison_scratch(dev, rows, K, N, Tp, pattern):
    from snn_automotive_object_detection_amd import fc6_grad
    need = _L().load().snn_spike_wgrad_bf16x3_workspace_bytes(rows, K, N, Tp)
    assert need == F6.query_bytes(rows, K, N, Tp) > 0
    buf = fc6_grad._WS_WGRAD3.get(dev, max(16, need))
    if pattern == "ff":
        buf.fill_(0xff)
    else:
        buf.view(torch.float32).fill_(float("nan"))                    # the quiet NaN 0x7fc00000
    per = C.c_int64(-1)
    n = _L().load().snn_spike_wgrad_bf16x3_slabs(rows, K, N, Tp, C.byref(per))
    assert (n, per.value) == F6.slabs(rows * Tp, K, N), "the library's launch plan differs from its restatement"
    return n


def _scratch_floats_written(dev) -> int:
    """how many floats of the scratch no longer hold the poison (both patterns are NaNs; every partial sum the tests produce is finite)"""
    from snn_automotive_object_detection_amd import fc6_grad
    buf = fc6_grad._WS_WGRAD3.get(dev, 16)
    return int((~torch.isnan(buf[:buf.numel() // 4 * 4].view(torch.float32))).sum())


def _check_scratch(dev, slabs, N, K):
    """the plan, observed: exactly slabs x N x K partial sums went through the scratch - and not one byte of it was touched with one slab"""
    got = _scratch_floats_written(dev)
    assert got == (slabs * N * K if slabs > 1 else 0), "%d floats of scratch written, the plan of %d slabs writes %d" % (got, slabs, slabs * N * K if slabs > 1 else 0)


def _exact(dev, rows, K, N, Tp, density, acc, pattern, seed):
    from snn_automotive_object_detection_amd import fc6_grad
    c = HG.exact_wgrad_case(rows, K, N, Tp, density, acc, seed)      # (the integer grid and its asserts: tests/_hidden_grad.py; padding bits set)
    a_rows, d, want32 = c["a_rows"], c["d"], c["want32"]
    out = c["prior"].to(dev) if acc else torch.full((N, K), float("nan"), device=dev)
    slabs = _poison_scratch(dev, rows, K, N, Tp, pattern)
    ar, dd = a_rows.to(dev), HG.padded(d, N + 5).to(dev)             # ldd > N, NaN in the padding columns
    got = fc6_grad.spike_wgrad_bf16x3(ar, dd, K, N, out=out, accumulate=bool(acc)).cpu().numpy()
    _check_scratch(dev, slabs, N, K)
    bad = got != want32
    assert not bad.any(), "rows %d K %d N %d T' %d: %d of %d elements differ, the first at %s: %r against %r" % (
        rows, K, N, Tp, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want32[bad][0])
    assert np.abs(want32).max() > 0
    if not acc:                                                      # a second call from the other scratch pattern: the same bits
        _poison_scratch(dev, rows, K, N, Tp, "nan" if pattern == "ff" else "ff")
        again = fc6_grad.spike_wgrad_bf16x3(ar, dd, K, N).cpu().numpy()
        assert np.array_equal(again.view(np.uint32), got.view(np.uint32)), "two calls on the same data differ"


@pytest.mark.parametrize("Tp", W_T)
@pytest.mark.parametrize("rows", W_ROWS)
def test_spike_wgrad_bf16x3_is_bit_equal_to_the_integer_expectation(gpu_device, rows, Tp):
    i = W_ROWS.index(rows) * 3 + W_T.index(Tp)
    for K in W_DIMS:
        for N in W_DIMS:
            _exact(gpu_device, rows, K, N, Tp, DENSITIES[i % 3], (i // 2) % 2, ("ff", "nan")[(i // 3) % 2], [rows, Tp, K, N])
            i += 1
    if rows <= 65:                                                   # K off a word, and K past the fp32 entry's limit of 8192
        _exact(gpu_device, rows, 392, 96, Tp, DENSITIES[i % 3], i % 2, "ff", [rows, Tp, 392])
        _exact(gpu_device, rows, 8224, 32, Tp, DENSITIES[(i + 1) % 3], (i + 1) % 2, "nan", [rows, Tp, 8224])


# d - 1, d, d + 1 for every tile dimension of the kernel (restated in tests/_fc6_grad.py): outputs and inputs of a wave and of a work-group,
# reduction rows of a matrix instruction, of a stage, and of the slab rule (256 rows per slab at least)
EDGE_N = sorted({d + e for d in (F6.WAVE_N, F6.TN, 2 * F6.TN) for e in (-1, 0, 1)})
EDGE_K = sorted({d + e for d in (F6.WAVE_K, F6.TK, 2 * F6.TK) for e in (-1, 0, 1)})
EDGE_M = sorted({d + e for d in (F6.MMA_ROWS, F6.MB, 2 * F6.MB, F6.SLAB_ROWS, 2 * F6.SLAB_ROWS) for e in (-1, 0, 1)})


@pytest.mark.parametrize("which", ("outputs", "inputs", "reduction_rows"))
def test_spike_wgrad_bf16x3_is_exact_at_every_tile_edge(gpu_device, which):
    i = 0
    if which == "outputs":
        for N in EDGE_N:
            _exact(gpu_device, 65, 96, N, 3, DENSITIES[i % 3], i % 2, ("ff", "nan")[i % 2], [N, 1]); i += 1
    elif which == "inputs":
        for K in EDGE_K:
            _exact(gpu_device, 65, K, 96, 3, DENSITIES[i % 3], i % 2, ("ff", "nan")[i % 2], [K, 2]); i += 1
    else:
        seen = set()
        for M in EDGE_M:
            seen.add(F6.slabs(M, 96, 160))
            _exact(gpu_device, M, 96, 160, 1, DENSITIES[i % 3], i % 2, ("ff", "nan")[i % 2], [M, 3]); i += 1
        assert {n for n, _ in seen} >= {1, 2, 3}, seen                # one slab, and the first rows at which there are two and three
    # more than one work-group in both output dimensions, partial in both, with several slabs
    assert F6.slabs(195, 513, 257)[0] == 1 and F6.slabs(1031 * 3, 513, 257)[0] > 1
    _exact(gpu_device, 65, 513, 257, 3, 0.3, 0, "nan", [513, 257])
    _exact(gpu_device, 1031, 513, 257, 3, 0.3, 1, "ff", [513, 257, 1])


@pytest.mark.parametrize("acc", (0, 1))
def test_spike_wgrad_bf16x3_exact_at_the_fc6_width(gpu_device, acc):
    assert F6.slabs(1290, 12544, 256)[0] == 3
    _exact(gpu_device, 129, 12544, 256, 10, 0.3, acc, "ff", [129, 12544, acc])


# ---- 2. one-hot: the split ------------------------------------------------------------------------------------------------------------------------
# (the third: 13 slabs, 3 x 3 work-groups with a partial tile in every dimension - the mid and lo planes through every LDS address and the second launch)
@pytest.mark.parametrize("rows,Tp,K,N", ((65, 3, 160, 96), (17, 1, 392, 32), (1031, 3, 513, 257)))
def test_a_one_hot_column_returns_d_cur_bit_for_bit(gpu_device, rows, Tp, K, N):
    """gw[:, k] == d_cur[m(k), :] for the one row m(k) that spikes in column k: hi + mid + lo in an order that is exact, and no bf16 subnormal
    flushed on the way (a wrong plane order, a truncating split or a flushed lo part fails here)"""
    from snn_automotive_object_detection_amd import fc6_grad
    a_rows, d, m = F6.one_hot_case(rows, Tp, K, N, [rows, Tp, K, N])
    slabs = _poison_scratch(gpu_device, rows, K, N, Tp, "nan")
    assert slabs == (13 if rows == 1031 else 1)
    got = fc6_grad.spike_wgrad_bf16x3(a_rows.to(gpu_device), HG.padded(d, N + 3).to(gpu_device), K, N).cpu().numpy()
    _check_scratch(gpu_device, slabs, N, K)
    want = d.reshape(Tp * rows, N).numpy()[m].T.copy()               # [N, K]
    bad = got.view(np.uint32) != want.view(np.uint32)
    bad &= ~((got == 0) & (want == 0))                                # (-0 may return +0)
    assert not bad.any(), "%d of %d elements differ, the first at %s: %r against %r" % (bad.sum(), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])
    hi, mid, lo = F6.split3(want.reshape(-1))
    assert ((np.abs(lo) > 0) & (np.abs(lo) < 2.0 ** -126)).sum() > 20, "no bf16-subnormal lo part in the draw"


# ---- 3. N(0, 1) inside the header's bound ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K,N,Tp", ((65, 96, 160, 3), (1031, 160, 96, 10), (257, 1568, 64, 10)))
def test_spike_wgrad_bf16x3_stays_inside_the_headers_bound(gpu_device, rows, K, N, Tp):
    from snn_automotive_object_detection_amd import fc6_grad
    rng = np.random.default_rng([rows, K, N, Tp, 7])
    a_rows, bits = HG.spike_rows(Tp, rows, K, 0.3, rng)
    d = torch.from_numpy(rng.standard_normal((Tp, rows, N)).astype(np.float32))
    d64 = d.reshape(Tp * rows, N).double().numpy()
    want = d64.T @ bits
    slabs = _poison_scratch(gpu_device, rows, K, N, Tp, "ff")
    tol = (3 * Tp * rows + slabs + 4) * 2.0 ** -24 * (np.abs(d64).T @ bits) + Tp * rows * 2.0 ** -133
    got = fc6_grad.spike_wgrad_bf16x3(a_rows.to(gpu_device), HG.padded(d, N + 32).to(gpu_device), K, N).cpu().numpy().astype(np.float64)
    err = np.abs(got - want)
    worst = float((err / np.maximum(tol, 1e-300)).max())
    _note("spike_wgrad_bf16x3 bound", worst)
    print("spike_wgrad_bf16x3 rows %d K %d N %d T' %d (%d slabs): largest error / bound = %.4f" % (rows, K, N, Tp, slabs, worst))
    assert np.isfinite(got).all() and (err <= tol).all() and np.abs(want).max() > 0


# ---- 4. guard bands ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,K,N,Tp,acc", ((65, 392, 160, 3, 0), (1031, 160, 96, 3, 1)))
def test_every_operand_stays_between_its_guard_bands(gpu_device, monkeypatch, rows, K, N, Tp, acc):
    """a partial tile in every dimension; one slab (the kernel writes gw itself) and thirteen (scratch and the second launch)"""
    from snn_automotive_object_detection_amd import fc6_grad
    dev = gpu_device
    seam = W.GuardedWorkspace(dev, 4 << 20)
    monkeypatch.setattr(fc6_grad, "_WS_WGRAD3", seam)
    c = HG.exact_wgrad_case(rows, K, N, Tp, 0.3, acc, [rows, K, N, Tp, acc, 4])
    n_slabs = F6.slabs(rows * Tp, K, N)[0]
    assert n_slabs == (1, 13)[acc]

    def call(in_guard):
        gc = W.GuardedCall(dev, dict(a_rows=c["a_rows"], d_cur=HG.padded(c["d"], N + 5)), dict(gw=c["prior"] if acc else ((N, K), torch.float32)), in_guard)
        seam.arm(0xff)
        fc6_grad.spike_wgrad_bf16x3(gc.ins["a_rows"], gc.ins["d_cur"], K, N, out=gc.outs["gw"], accumulate=bool(acc))
        torch.cuda.synchronize()
        snap = gc.verify()
        seam.check()
        assert seam.sizes == [max(16, F6.query_bytes(rows, K, N, Tp))], seam.sizes
        got = gc.outs["gw"].cpu().numpy()
        assert np.array_equal(got, c["want32"]), "differs from the integer expectation"
        return snap
    W.run_input_guards(call)


# ---- 5. the module ---------------------------------------------------------------------------------------------------------------------------------
C_IN, HD, KCLS = 32, 64, 5
D_IN = C_IN * 49
MODULE_CASES = ([(feed, R, T, "bf16x3") for T in (4, 12) for R in (37, 130) for feed in ("rows", "roialign")]
                + [("rows", 37, 12, "f32"), ("roialign", 130, 6, "f32"), ("rows", 130, 3, "bf16x3")])


@pytest.mark.parametrize("feed,R,T,precision", MODULE_CASES, ids=["%s_R%d_T%d_%s" % c for c in MODULE_CASES])
def test_train_fc6_on_a_dyadic_head_with_zero_flips(gpu_device, feed, R, T, precision):
    from snn_automotive_object_detection_amd import fc6_grad, losses, ops
    dev = gpu_device
    d, call, tr, (w6, w7, w_cls, w_box) = F6.module_case(dev, feed, R, T, precision, C_IN, HD, KCLS)
    enc_o, spk6, spk7 = tr["z"].reshape(T, R, D_IN), tr["spk6"], tr["spk7"]
    plain = call(d)
    assert all(t.grad_fn is None and not t.requires_grad for t in plain), "default off: the outputs carry no graph"
    plain = [t.clone() for t in plain]
    d.train_fc6 = True
    with torch.no_grad():
        assert all(not t.requires_grad for t in call(d)), "no grad mode: the plain forward"
    outs = call(d)
    assert type(outs[0].grad_fn).__name__.startswith("Fc6Grad") and fc6_grad.Fc6Grad is not None
    sv = outs[0].grad_fn.saved
    assert d._resolve_precision() == precision and sv.gemm is (ops.spike_gemm_bf16x3 if precision == "bf16x3" else ops.spike_gemm)
    # preconditions: the saved rows are the oracle's rasters (it fails otherwise: nothing below would mean anything)
    enc, z6, z7 = HG.unpack_bits(sv.enc, D_IN), HG.unpack_bits(sv.z6, HD), HG.unpack_bits(sv.z7, HD)
    assert enc.shape == (T - 2, R, D_IN) and z6.shape == (T - 1, R, HD) and z7.shape == (T, R, HD)
    assert torch.equal(enc, enc_o[:T - 2].bool()), "the re-encoded rows differ from the oracle's raster in %d places" % int((enc != enc_o[:T - 2].bool()).sum())
    assert torch.equal(z6, spk6[:T - 1].bool()), "lif6's saved rows differ from the oracle's raster in %d places" % int((z6 != spk6[:T - 1].bool()).sum())
    assert torch.equal(z7, spk7.bool()), "lif7's saved rows differ from the oracle's raster in %d places" % int((z7 != spk7.bool()).sum())
    assert bool(enc.any()) and bool(z6.any()) and bool(z7.any()), "a layer is silent: the case proves nothing"
    for got, want in zip(outs, plain):
        assert got.requires_grad and torch.equal(got.detach(), want), "train_fc6 changed an output"
    g = torch.Generator().manual_seed(R + T)
    labels = torch.randint(0, KCLS, (R,), generator=g)
    targets = torch.randn((R, 4), generator=g) * 0.5
    for kind in ("fastrcnn", "quadratic"):
        cpu_loss = F6.loss_of(kind, labels, targets)
        if kind == "fastrcnn":
            gpu_loss = lambda cls, box: sum(losses.fastrcnn_loss(cls, box, [labels.to(dev)], [targets.to(dev)]))
        else:
            gpu_loss = cpu_loss
        for q in d.parameters():
            q.grad = None
        d.train_fc6, d.train_fc7, d.train_readout = True, False, False
        gpu_loss(*call(d)).backward()
        g6, g7, g_cls, g_box = (q.grad.clone() for q in (d.fc6.weight, d.fc7.weight, d.cls_score.weight, d.bbox_pred.weight))
        # the three upper gradients: what train_fc7 returns, bit for bit
        for q in d.parameters():
            q.grad = None
        d.train_fc6, d.train_fc7 = False, True
        outs7 = call(d)
        assert "Fc7Grad" in type(outs7[0].grad_fn).__name__
        gpu_loss(*outs7).backward()
        assert d.fc6.weight.grad is None
        assert torch.equal(g7, d.fc7.weight.grad) and torch.equal(g_cls, d.cls_score.weight.grad) and torch.equal(g_box, d.bbox_pred.weight.grad), \
            "a gradient above fc6 differs from the train_fc7 path"
        # fc6.weight.grad against fp64 autograd, 4 x the error of fp32 CPU autograd
        ref64, _ = F6.cpu_fc6_grad(enc_o, spk6, spk7, w6, w7, w_cls, w_box, T, "jump_first", cpu_loss, torch.float64, KCLS)
        ref32, _ = F6.cpu_fc6_grad(enc_o, spk6, spk7, w6, w7, w_cls, w_box, T, "jump_first", cpu_loss, torch.float32, KCLS)
        assert g6.shape == (HD, D_IN) and bool(torch.isfinite(g6).all()) and float(ref64.abs().max()) > 0
        (gmax, grms), (cmax, crms) = HG.errors(g6.cpu(), ref64), HG.errors(ref32, ref64)
        _note("fc6.weight.grad", max(gmax / (4 * cmax), grms / (4 * crms)))
        print("%s R %d T %d %s %s: fc6 grad |err| max %.3g rms %.3g of |g| %.3g; fp32 CPU autograd %.3g / %.3g; error / tolerance %.3f (max) %.3f (rms)"
              % (feed, R, T, precision, kind, gmax, grms, float(ref64.abs().max()), cmax, crms, gmax / (4 * cmax), grms / (4 * crms)))
        assert gmax <= 4 * cmax and grms <= 4 * crms
    # fc6 frozen: today's logic, whatever train_fc6 says
    d.train_fc6, d.train_fc7, d.train_readout = True, True, False
    d.fc6.weight.requires_grad_(False)
    assert type(call(d)[0].grad_fn).__name__.startswith("Fc7Grad"), "fc6 frozen: the fc7 graph"
    d.train_fc7, d.train_readout = False, True
    assert "ReadoutGrad" in type(call(d)[0].grad_fn).__name__, "fc6 frozen, train_fc7 off: the readout graph alone"
    d.train_readout = False
    assert all(t.grad_fn is None for t in call(d)), "fc6 frozen, nothing else asked for: the plain forward"


def test_train_fc6_refusals_on_the_device(gpu_device):
    import snn_automotive_object_detection_amd as S
    d = S.FastRCNNPredictorSNNFull(8 * 49, 32, 3, 2).to(gpu_device)
    d.train_fc6 = True
    x = torch.randn(5, 8, 7, 7, device=gpu_device)
    with pytest.raises(ValueError, match="train_fc6 needs num_steps >= 3"):
        d(x)
    d.num_steps = 4
    outs = d(x)
    assert type(outs[0].grad_fn).__name__.startswith("Fc6Grad")
    empty = d(x[:0])                                                 # a pass over no rows: zero gradients of the right shapes
    (empty[0].sum() + empty[1].sum()).backward()
    assert d.fc6.weight.grad.shape == d.fc6.weight.shape and not d.fc6.weight.grad.any()


# ---- 6. graph capture ---------------------------------------------------------------------------------------------------------------------------
def test_the_backward_chain_replays_bit_equal_on_two_data_sets(gpu_device):
    """planes_to_rows x 2, both un-fused GEMMs, both adjoints, the matmul between them and both weight gradients: captured once, replayed on a
    second data set, bit-equal to the eager calls"""
    from snn_automotive_object_detection_amd import fc6_grad, hidden, ops
    L = _L()
    dev, R, D, Hd, T = gpu_device, 130, 392, 96, 8
    W6, Wd = (Hd + 31) // 32, (D + 31) // 32
    p = _params(HG.REFERENCE)
    g = torch.Generator().manual_seed(1)
    w7 = (torch.randn((Hd, Hd), generator=g) * 0.3).to(dev)
    w6 = (torch.randn((Hd, D), generator=g) * 0.1).to(dev)
    w7p, w6p = ops.pack_linear_bf16x3(w7), ops.pack_linear_bf16x3(w6)
    v6 = L.snn_planes_view(64, R * W6 + 3, R, W6, TP.WORD_MAJOR, T - 1, 0)
    v7 = L.snn_planes_view(0, R * W6, R, W6, TP.ROWS, T, 0)
    sets = []
    for seed in (0, 1):
        rng = np.random.default_rng(seed)
        z6 = HG.pack_bits(torch.from_numpy(rng.random((T - 1, R, Hd)) < 0.3)).numpy().view(np.uint32)
        flat = np.full(16 + (T - 1) * (R * W6 + 3), 0xa5a5a5a5, dtype=np.uint32)
        idx = TP.word_index(TP.WORD_MAJOR, R, W6)
        for t in range(T - 1):
            flat[16 + t * (R * W6 + 3) + idx] = z6[t]
        z7 = HG.pack_bits(torch.from_numpy(rng.random((T, R, Hd)) < 0.3))
        enc = HG.pack_bits(torch.from_numpy(rng.random((T - 2, R, D)) < 0.2), set_padding=True)
        sets.append((torch.from_numpy(flat.view(np.uint8).copy()), z7.reshape(-1).view(torch.uint8).clone(), enc,
                     torch.from_numpy(rng.standard_normal((R, Hd)).astype(np.float32))))

    def fn(ws6, ws7, enc, gu):
        a6 = hidden.planes_to_rows(ws6, v6, T - 1)
        z7 = hidden.planes_to_rows(ws7, v7, T)
        cur7 = ops.spike_gemm_bf16x3(a6.view((T - 1) * R, W6), Hd, Hd, w7p)
        d_cur7 = hidden.lif_surrogate_bwd(cur7.view(T - 1, R, -1), z7, Hd, p, 100.0, gu=gu)
        gw7 = hidden.spike_linear_wgrad(a6, d_cur7, Hd, Hd)
        gz6 = torch.matmul(d_cur7.view((T - 1) * R, Hd), w7).view(T - 1, R, Hd)
        cur6 = ops.spike_gemm_bf16x3(enc.view((T - 2) * R, Wd), D, Hd, w6p)
        d_cur6 = hidden.lif_surrogate_bwd(cur6.view(T - 2, R, -1), a6, Hd, p, 100.0, gz=gz6)
        return a6, z7, d_cur7, gw7, gz6, d_cur6, fc6_grad.spike_wgrad_bf16x3(enc, d_cur6, D, Hd)
    cap = GC.run_protocol(GC.FnCase(("spike_gemm_bf16x3",), dev, sets, fn), GC.HipGraph())
    assert cap.n_replays == 4
    gw6 = cap.case.results[-1][-1]
    assert gw6.shape == (Hd, D) and bool(torch.isfinite(gw6).all()) and float(gw6.abs().max()) > 0


# ---- 7. one fine-tuning step end to end -------------------------------------------------------------------------------------------------------------
def test_one_fine_tuning_step_moves_fc6_on_the_device(gpu_device):
    from snn_automotive_object_detection_amd import fc6_grad
    from tests._small_model import small_model, targets as _targets
    dev = gpu_device
    model = small_model(dev)
    det = model.roi_heads.box_head_and_predictor
    det.train_fc6 = True
    params = fc6_grad.freeze_below_fc6(model)
    assert len(params) == 6 and params[0] is det.fc6.weight and params[1] is det.fc7.weight
    images = [torch.rand((3, 64, 64), generator=torch.Generator().manual_seed(i)).to(dev) for i in range(2)]
    targets = _targets(dev)
    gen = lambda: torch.Generator(device=dev).manual_seed(5)
    with torch.no_grad():
        first = [t.clone() for t in model.roi_heads.box_head_and_predictor(torch.ones(3, 32, 7, 7, device=dev))]
    out = model.readout_losses(images, targets, generator=gen())
    sum(out.values()).backward()
    ids = {id(q) for q in params}
    assert all(q.grad is None for q in model.parameters() if id(q) not in ids), "a parameter below fc6 received a gradient"
    assert all(q.grad is not None and bool(torch.isfinite(q.grad).all()) for q in params)
    assert float(det.fc6.weight.grad.abs().max()) > 0, "fc6 received a zero gradient: the case proves nothing"
    before = det.fc6.weight.detach().clone()
    keep7 = det.fc7.weight.detach().clone()
    # fc6 ALONE, by a step normalised to 0.1 at its largest element (the gradient through two surrogate layers is small next to the weights, and
    # a step that flips no lif6 spike moves no output bit): what moves the outputs below is fc6's packed copies, rebuilt
    torch.optim.SGD([det.fc6.weight], lr=0.1 / float(det.fc6.weight.grad.abs().max())).step()
    assert not torch.equal(det.fc6.weight.detach(), before) and torch.equal(det.fc7.weight.detach(), keep7), "the optimiser step did not move fc6.weight"
    with torch.no_grad():                                            # the next forward repacks fc6 (the caches key on the version counter)
        second = model.roi_heads.box_head_and_predictor(torch.ones(3, 32, 7, 7, device=dev))
    assert not all(torch.equal(a, b) for a, b in zip(first, second)), "the outputs did not move after the step"
    for q in params:
        q.grad = None
    again = model.readout_losses(images, targets, generator=gen())
    assert all(bool(torch.isfinite(v)) for v in again.values())
    sum(again.values()).backward()                                   # the natural-order copy is rebuilt as well: the backward runs on the moved fc6
    assert bool(torch.isfinite(det.fc6.weight.grad).all()) and float(det.fc6.weight.grad.abs().max()) > 0


def test_log_the_largest_ratios():
    """runs last in the file: the figures profiles/fc6_grad.txt and DESIGN.md 4.16 record"""
    for k, v in sorted(RATIOS.items()):
        print("largest error / tolerance ratio, %s: %.4f" % (k, v))
