"""fc6's gradient without a GPU: that the two-layer restatement the GPU chain follows - gz6 = d_cur7 W7 between two
adjoints over the windows T - 1 and T - 2 - IS torch.autograd through both SuperSpike layers and the LI readout; header <-> library <-> binding
signatures of the two entries and of the host-only slab query; every refusal (-1 with a message before any device work: there is no device
here); the scratch query and the library's own slab plan against their restatement on a grid of (M, K, N); the code object's register and LDS figures; the module switches."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _fc6_grad as F6
from tests import _hidden_grad as HG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("snn_spike_wgrad_bf16x3_workspace_bytes", "snn_spike_wgrad_bf16x3_slabs", "snn_spike_wgrad_bf16x3")


def _L():
    from snn_automotive_object_detection_amd import _lib
    return _lib


def _params(order=0):
    L = _L()
    return L.snn_params(0.1, -0.2, 0.0, 0.0, 0.25, 0.1, order, L.PRECISIONS["bf16x3"])


# ---- 1. the identity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ("jump_first", "voltage_first"))
@pytest.mark.parametrize("name", ("reference", "other"))
@pytest.mark.parametrize("T", (3, 4, 12))
def test_the_two_layer_restatement_is_autograd_through_both_superspike_layers(T, name, order):
    c = HG.REFERENCE if name == "reference" else HG.OTHER
    R, N, n_out, alpha = 6, 24, 7, 100.0
    g = torch.Generator().manual_seed(T * 10 + (name == "other"))
    cur6 = HG.draw_currents(T, R, N, N, 0.5, c, [T, R, N, 6]).to(torch.float64).requires_grad_(True)
    w7 = (torch.rand((N, N), generator=g, dtype=torch.float64) - 0.3) * (8.0 * max(c.th - c.v_leak, 0.05) / (c.a * N * 0.35))
    w_out = torch.randn((n_out, N), generator=g, dtype=torch.float64)
    z6 = HG.lif_forward_autograd(cur6, c, alpha)[:T]                 # a pass of T steps: z6_t from cur6_0 .. cur6_{t-1}
    cur7 = z6 @ w7.t()
    z7 = HG.lif_forward_autograd(cur7, c, alpha)[:T]
    out = F6.li_torch(z7, w_out, c, order, torch.float64)
    loss = 0.5 * (out * out).sum() + out.sum()
    want, = torch.autograd.grad(loss, cur6)
    if T >= 4:
        assert 0.05 < float(z6.detach()[1:].mean()) < 0.95 and 0.02 < float(z7.detach()[2:].mean()) < 0.98, "a layer is silent or saturated"
    # a current first moves a spike one step later, and z6_{T-1} reaches nothing: exactly zero, not merely small
    assert want.shape == (T, R, N) and not want[T - 2:].any(), "cur6_{T-2} or cur6_{T-1} received a gradient"
    got, d_cur7 = F6.two_layer_restated(cur6.detach(), z6.detach().bool(), cur7.detach(), z7.detach().bool(), w7, w_out, (out + 1.0).detach(), c, alpha,
                                        order)
    assert got.shape == (T - 2, R, N) and d_cur7.shape == (T - 1, R, N)
    top = float(want.abs().max())
    # voltage-first at T = 3: cur6_0 reaches the outputs only through z6_1 -> cur7_1 -> z7_2, the LAST step's spike, and in that order a spike of
    # the last step reaches no output (kappa_{T-1} = 0).  The gradient is identically zero there, in autograd AND in the restatement, exactly
    if T == 3 and order == "voltage_first":
        assert top == 0.0 and not got.any() and not d_cur7[1:].any()
    else:
        assert top > 0
    assert float((got - want[:T - 2]).abs().max()) <= 1e-12 * max(top, 1e-300), float((got - want[:T - 2]).abs().max()) / max(top, 1e-300)


# ---- 2. header, library, binding -------------------------------------------------------------------------------------------------------------
def _types(hdr, decl):
    m = re.search(decl + r"\(([^)]*)\);", hdr)
    assert m, decl
    return [re.sub(r"\s+", " ", a).strip().rsplit(" ", 1)[0] for a in m.group(1).split(",")]


def test_header_library_and_binding_agree_on_the_two_entries():
    L = _L()
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snn_hip.h")).read(), flags=re.S)
    assert _types(hdr, r"size_t snn_spike_wgrad_bf16x3_workspace_bytes") == ["int64_t", "int", "int", "int"]
    assert _types(hdr, r"\bint snn_spike_wgrad_bf16x3") == ["const uint32_t*", "const float*", "int", "int", "int64_t", "int", "int", "float*", "int",
                                                             "void*", "size_t", "snn_stream_t"]
    assert _types(hdr, r"\bint snn_spike_wgrad_bf16x3") == _types(hdr, r"\bint snn_spike_linear_wgrad"), "the argument list of the fp32 pair"
    assert _types(hdr, r"\bint snn_spike_wgrad_bf16x3_slabs") == ["int64_t", "int", "int", "int", "int64_t*"]
    assert L.SYMBOLS["snn_spike_wgrad_bf16x3_slabs"] == (C.c_int, [C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)])
    for name in ENTRIES:
        assert name in L.SYMBOLS and hasattr(lib, name), name
    ptr = C.c_void_p
    assert L.SYMBOLS["snn_spike_wgrad_bf16x3_workspace_bytes"] == (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int])
    assert L.SYMBOLS["snn_spike_wgrad_bf16x3"] == (C.c_int, [ptr, ptr, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, ptr, C.c_int, ptr, C.c_size_t,
                                                             L.c_stream])
    csrc = os.path.join(ROOT, "snn_automotive_object_detection_amd", "csrc")
    assert '#include "snn_spike_wgrad_x3.h"' in open(os.path.join(csrc, "snn_kernels.hip")).read()
    src = open(os.path.join(csrc, "snn_spike_wgrad_x3.h")).read()
    assert "atomic" not in re.sub(r"//[^\n]*", "", src)
    # the constants tests/_fc6_grad.py restates
    for name, value in (("W3_TN", F6.TN), ("W3_TK", F6.TK), ("W3_MB", F6.MB), ("W3_SLAB_ROWS", F6.SLAB_ROWS), ("W3_MAX_SLABS", F6.MAX_SLABS),
                        ("W3_FILL", F6.FILL), ("W3_MAX_K", F6.MAX_K), ("W3_MAX_N", F6.MAX_N)):
        assert re.search(r"#define %s %d\b" % (name, value), src), name


# ---- 3. refusals, the size query, the slab function ------------------------------------------------------------------------------------------------
def _fake():
    fake = (C.c_uint8 * 64)()                                        # never dereferenced: every call is refused on the host
    return fake, C.c_void_p(C.addressof(fake))


BAD = [("null planes", dict(a=None)), ("null d_cur", dict(d=None)), ("null result", dict(gw=None)), ("T' = 0", dict(T=0)), ("T' = 33", dict(T=33)),
       ("rows = 0", dict(rows=0)), ("rows = 2^31", dict(rows=2 ** 31)), ("K = 0", dict(K=0)), ("K = 16385", dict(K=16385)), ("N = 0", dict(N=0)),
       ("N = 8193", dict(N=8193, ldd=8200)), ("ldd < N", dict(ldd=95)), ("ldd = 2^28", dict(ldd=2 ** 28)), ("accumulate = 2", dict(acc=2)),
       ("accumulate = -1", dict(acc=-1)), ("short scratch", dict(short=1)), ("null scratch", dict(scratch=None)), ("misaligned scratch", dict(off=2))]


@pytest.mark.parametrize("what,over", BAD, ids=[b[0] for b in BAD])
def test_spike_wgrad_bf16x3_refuses(what, over):
    lib = _L().load()
    keep, ptr = _fake()
    a = dict(a=ptr, d=ptr, ldd=96, T=11, rows=130, K=160, N=96, gw=ptr, acc=0, scratch=ptr, short=0, off=0)
    a.update(over)
    need = lib.snn_spike_wgrad_bf16x3_workspace_bytes(130, 160, 96, 11)
    assert need > 0
    scratch = a["scratch"] if not a["off"] else C.c_void_p(C.addressof(keep) + a["off"])
    rc = lib.snn_spike_wgrad_bf16x3(a["a"], a["d"], a["ldd"], a["T"], a["rows"], a["K"], a["N"], a["gw"], a["acc"], scratch, need - a["short"], None)
    assert rc == -1, (what, rc)
    msg = lib.snn_last_error()
    assert msg and b"snn_spike_wgrad_bf16x3" in msg, (what, msg)


def test_k_past_the_fp32_entrys_limit_is_taken():
    """K = 12544 (fc6 at C = 256) and K = 16384: the size query is non-zero where snn_spike_linear_wgrad's is 0"""
    lib = _L().load()
    for K in (8193, 12544, 16384):
        assert lib.snn_spike_wgrad_bf16x3_workspace_bytes(1024, K, 1024, 10) > 0 and lib.snn_spike_linear_wgrad_workspace_bytes(1024, K, 1024, 10) == 0


def test_workspace_bytes_is_monotone_zero_outside_the_limits_and_bounded_at_fc6():
    q = _L().load().snn_spike_wgrad_bf16x3_workspace_bytes
    rows = (1, 15, 16, 17, 63, 65, 255, 256, 257, 1024, 1031, 8191, 8193, 32769, 2 ** 31 - 1)
    ks = (1, 31, 32, 96, 160, 255, 256, 257, 392, 1024, 8192, 8224, 12544, 16384)
    ns = (1, 32, 96, 127, 128, 129, 160, 1024, 4096, 8192)
    steps = (1, 2, 3, 10, 11, 12, 31, 32)
    for K in ks:
        for N in ns:
            for T in steps:
                sizes = [q(r, K, N, T) for r in rows]
                assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (K, N, T, sizes)
                assert sizes == [F6.query_bytes(r, K, N, T) for r in rows], (K, N, T)
            for r in rows[:12]:
                sizes = [q(r, K, N, T) for T in steps]
                assert sizes == sorted(sizes), (r, K, N, sizes)
    for r in rows[:12]:
        for T in (1, 10):
            for N in ns:
                sizes = [q(r, K, N, T) for K in ks]
                assert sizes == sorted(sizes), (r, N, T, sizes)
            for K in ks:
                sizes = [q(r, K, N, T) for N in ns]
                assert sizes == sorted(sizes), (r, K, T, sizes)
    # the library's own launch plan (snn_spike_wgrad_bf16x3_slabs: host only) against the restatement, for M as rows x T' both ways round;
    # the query is never below what that plan writes: slabs x N x K floats (one slab writes gw itself)
    plan = _L().load().snn_spike_wgrad_bf16x3_slabs

    def lib_slabs(rows, K, N, T):
        per = C.c_int64(-1)
        n = plan(rows, K, N, T, C.byref(per))
        assert plan(rows, K, N, T, None) == n
        return n, per.value
    for M in (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 769, 2048, 3093, 8191, 8192, 8193, 10240, 11264, 10 ** 6, 2 ** 31 - 1):
        for K in ks:
            for N in ns:
                n, per = F6.slabs(M, K, N)
                assert lib_slabs(M, K, N, 1) == (n, per), (M, K, N, lib_slabs(M, K, N, 1), (n, per))
                for T in (2, 10, 32):
                    if M % T == 0:
                        assert lib_slabs(M // T, K, N, T) == (n, per), (M, K, N, T)
                assert 1 <= n <= F6.MAX_SLABS and per % F6.MB == 0 and (n - 1) * per < M <= n * per, (M, K, N, n, per)
                assert q(M, K, N, 1) >= (n * N * K * 4 if n > 1 else 1), (M, K, N, n)
                if F6.cdiv(N, F6.TN) * F6.cdiv(K, F6.TK) >= F6.FILL:
                    assert n == 1
    # the condition of fc6's shape: at most 2 N K floats (103 MB), and one slab - the 8 x 49 output tiles alone fill the device
    assert q(1024, 12544, 1024, 10) <= 2 * 1024 * 12544 * 4 and F6.slabs(10240, 12544, 1024) == (1, 10240)
    assert F6.slabs(11264, 1024, 1024) == (8, 1408) and F6.slabs(130 * 3, 160, 96) == (2, 224) and F6.slabs(17, 32, 32) == (1, 32)
    for bad in ((0, 32, 32, 1), (2 ** 31, 32, 32, 1), (10, 0, 32, 1), (10, 16385, 32, 1), (10, 32, 0, 1), (10, 32, 8193, 1), (10, 32, 32, 0), (10, 32, 32, 33),
                (-1, 32, 32, 1)):
        assert q(*bad) == 0, bad
        per = C.c_int64(-1)
        assert plan(*bad, C.byref(per)) == 0 and per.value == 0, bad


# ---- 4. the code object ---------------------------------------------------------------------------------------------------------------------------
def test_the_new_kernels_keep_the_register_and_lds_budget_the_design_states(tmp_path):
    """the code object's own metadata (llvm-readelf --notes; no GPU): k_wgrad3_partial and k_wgrad3_reduce neither spill nor use scratch memory,
    the partial kernel fits 256 registers per lane (vector + accumulator: one unified file on gfx950) and its LDS, times the two work-groups per
    CU DESIGN.md 4.16 argues from, fits the CU's 160 KB"""
    import subprocess
    from snn_automotive_object_detection_amd import build as B
    tools = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(tools, "llvm-readelf")):
        pytest.skip("no llvm-readelf")
    subprocess.run(["cp", B.build(force=False), str(tmp_path / "lib.so")], check=True)
    subprocess.run([os.path.join(tools, "llvm-objdump"), "--offloading", "lib.so"], cwd=str(tmp_path), check=True, stdout=subprocess.DEVNULL)
    objs = [f for f in os.listdir(str(tmp_path)) if "gfx950" in f]
    assert len(objs) == 1, os.listdir(str(tmp_path))
    notes = subprocess.run([os.path.join(tools, "llvm-readelf"), "--notes", objs[0]], cwd=str(tmp_path), check=True, stdout=subprocess.PIPE, text=True).stdout
    seen = {}
    for block in re.split(r"\n\s*- \.agpr_count:", "\n" + notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or not re.match(r"_Z\d+k_wgrad3_", name.group(1)):
            continue
        f = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1))
             for k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count", "group_segment_fixed_size")}
        f["agpr_count"] = int(re.match(r"\s*(\d+)", block).group(1))
        seen[re.match(r"_Z\d+(k_wgrad3_[a-z]+)", name.group(1)).group(1)] = f
    assert sorted(seen) == ["k_wgrad3_partial", "k_wgrad3_reduce"], sorted(seen)
    for k, f in seen.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (k, f)
        assert f["vgpr_count"] + f["agpr_count"] <= 256, (k, f)
    w = seen["k_wgrad3_partial"]
    assert w["group_segment_fixed_size"] == F6.LDS_BYTES == 63744, w
    assert w["group_segment_fixed_size"] * F6.WORK_GROUPS_PER_CU <= 160 * 1024, w
    assert seen["k_wgrad3_reduce"]["vgpr_count"] <= 64


# ---- 5. the module ---------------------------------------------------------------------------------------------------------------------------------
def test_train_fc6_defaults_off_and_refuses_what_it_cannot_differentiate():
    import snn_automotive_object_detection_amd as S
    d = S.FastRCNNPredictorSNNFull(49 * 8, 32, 3, 4)
    assert d.train_fc6 is False and d.train_fc7 is False
    x = torch.randn(2, 8, 7, 7)
    d.train_fc6 = d.spike_rates = True
    with pytest.raises(NotImplementedError, match="train_fc6"):
        d(x)
    d.spike_rates = False
    for prec in ("bf16", "mxfp6"):
        d.precision = prec
        with pytest.raises(NotImplementedError, match="train_fc6"):
            d(x)
        with pytest.raises(NotImplementedError, match="train_fc6"):
            d.forward_roialign([torch.randn(1, 8, 8, 8)], [1.0], torch.zeros(2, 5), torch.zeros(2, dtype=torch.int32))


def test_attach_refuses_short_passes_and_a_pass_that_formed_too_few_lif6_planes():
    """fc6_grad.attach checks T and lif6's view before anything touches a device"""
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import fc6_grad
    L = _L()
    d = S.FastRCNNPredictorSNNFull(49 * 8, 32, 3, 6)
    outs = (torch.zeros(4, 3), torch.zeros(4, 12))
    ws = torch.zeros(64, dtype=torch.uint8)                          # never read: the refusal comes first

    def view(steps):
        return L.snn_planes_view(0, 4, 4, 1, 0, steps, 0)

    def never(steps):
        raise AssertionError("the encoder ran before the refusal")
    with pytest.raises(L.SnnHipError, match="train_fc6: the pass formed 4 lif6 planes, the gradient needs 5"):
        fc6_grad.attach(d, outs, ws, view(4), view(6), 6, _params(), "bf16x3", never)
    for T in (1, 2):
        with pytest.raises(ValueError, match="train_fc6 needs num_steps >= 3"):
            fc6_grad.attach(d, outs, ws, view(6), view(6), T, _params(), "bf16x3", never)
    with pytest.raises(Exception, match="GPU"):                      # enough planes: the next thing is the copy out of the workspace, which needs a device
        fc6_grad.attach(d, outs, ws, view(5), view(6), 6, _params(), "bf16x3", never)


def test_freeze_below_fc6_leaves_four_trainable_parameters_on_a_detector_head():
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import fc6_grad
    d = S.FastRCNNPredictorSNNFull(49 * 8, 32, 3, 4)
    keep = fc6_grad.freeze_below_fc6(d)
    assert [id(w) for w in keep] == [id(d.fc6.weight), id(d.fc7.weight), id(d.cls_score.weight), id(d.bbox_pred.weight)]
    assert sorted(n for n, q in d.named_parameters() if q.requires_grad) == ["bbox_pred.weight", "cls_score.weight", "fc6.weight", "fc7.weight"]
    h = S.RPNHeadSNN(32, 3, 4)                                       # an RPN head keeps its readout weights, as freeze_hidden keeps them
    assert len(fc6_grad.freeze_below_fc6(h)) == 2 and sorted(n for n, q in h.named_parameters() if q.requires_grad) == ["conv_bbox.weight", "conv_cls.weight"]
    assert fc6_grad.FC6_WEIGHTS == ("fc6", "fc7", "cls_score", "bbox_pred")


def test_the_wrapper_refuses_cpu_tensors_and_the_scan_of_training_entries_stays_at_seven():
    from snn_automotive_object_detection_amd import fc6_grad
    with pytest.raises(Exception, match="GPU"):
        fc6_grad.spike_wgrad_bf16x3(torch.zeros(1, 2, 1, dtype=torch.int32), torch.zeros(1, 2, 32), 32, 32)
    # the scratch call site lives in fc6_grad.py alone
    pkg = os.path.join(ROOT, "snn_automotive_object_detection_amd")
    for name in ("hidden.py", "readout.py", "losses.py", "ops.py"):
        assert "wgrad_bf16x3" not in open(os.path.join(pkg, name)).read(), name
    assert open(os.path.join(pkg, "fc6_grad.py")).read().count("_WS_WGRAD3.get(") == 1


def test_the_split_restated_for_the_one_hot_test_is_exact_on_its_own_draws():
    """hi + mid + lo == d in the order (lo + mid) + hi for every value the one-hot GPU test draws, and a part of them has a bf16-subnormal lo"""
    a_rows, d, m = F6.one_hot_case(17, 1, 392, 32, [17, 1])
    x = d.numpy().reshape(-1)
    hi, mid, lo = F6.split3(x)
    assert np.array_equal(((lo + mid).astype(np.float32) + hi).astype(np.float32), x)
    sub = (np.abs(lo) > 0) & (np.abs(lo) < 2.0 ** -126)
    assert sub.sum() > 20 and (np.abs(mid) > 0).mean() > 0.5
    z = HG.unpack_bits(a_rows, 392).reshape(-1, 392)
    assert bool((z.sum(dim=0) == 1).all()) and np.array_equal(z.numpy().argmax(axis=0), m)
