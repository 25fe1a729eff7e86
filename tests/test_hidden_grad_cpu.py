"""Hidden-layer gradients (fc7 -> lif7) without a GPU: header <-> library <-> binding signatures of the four entries, every refusal (-1 with a
message before any device work: this machine has no device), the monotone scratch query, the module switches, and - the point of the file -
that the adjoint restated in tests/_hidden_grad.py, the oracle of the GPU tests, IS the reference's gradient: torch.autograd through
lif_feed_forward_step with a SuperSpike threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import _hidden_grad as HG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("snn_planes_to_rows", "snn_lif_surrogate_bwd", "snn_spike_linear_wgrad_workspace_bytes", "snn_spike_linear_wgrad")


def _L():
    from snn_automotive_object_detection_amd import _lib
    return _lib


def _params(order=0):
    L = _L()
    return L.snn_params(0.1, -0.2, 0.0, 0.0, 0.25, 0.1, order, L.PRECISIONS["bf16x3"])


def _view(rows=100, words=8, layout=0, steps=8, stride=None, offset=0):
    return _L().snn_planes_view(offset, rows * words if stride is None else stride, rows, words, layout, steps, 0)


def _types(hdr, decl):
    m = re.search(decl + r"\(([^)]*)\);", hdr)
    assert m, decl
    return [re.sub(r"\s+", " ", a).strip().rsplit(" ", 1)[0] for a in m.group(1).split(",")]


def test_header_library_and_binding_agree_on_the_four_entries():
    L = _L()
    lib = L.load()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "snn_hip.h")).read(), flags=re.S)
    assert _types(hdr, r"\bint snn_planes_to_rows") == ["const void*", "const snn_planes_view*", "int", "uint32_t*", "snn_stream_t"]
    assert _types(hdr, r"\bint snn_lif_surrogate_bwd") == ["const float*", "int", "const uint32_t*", "int", "int", "int", "const snn_params*", "float",
                                                            "const float*", "const float*", "float*", "snn_stream_t"]
    assert _types(hdr, r"size_t snn_spike_linear_wgrad_workspace_bytes") == ["int64_t", "int", "int", "int"]
    assert _types(hdr, r"\bint snn_spike_linear_wgrad") == ["const uint32_t*", "const float*", "int", "int", "int64_t", "int", "int", "float*", "int",
                                                             "void*", "size_t", "snn_stream_t"]
    for name in ENTRIES:
        assert name in L.SYMBOLS and hasattr(lib, name), name
    ptr, view, par = C.c_void_p, C.POINTER(L.snn_planes_view), C.POINTER(L.snn_params)
    assert L.SYMBOLS["snn_planes_to_rows"] == (C.c_int, [ptr, view, C.c_int, ptr, L.c_stream])
    assert L.SYMBOLS["snn_lif_surrogate_bwd"] == (C.c_int, [ptr, C.c_int, ptr, C.c_int, C.c_int, C.c_int, par, C.c_float, ptr, ptr, ptr, L.c_stream])
    assert L.SYMBOLS["snn_spike_linear_wgrad_workspace_bytes"] == (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int])
    assert L.SYMBOLS["snn_spike_linear_wgrad"] == (C.c_int, [ptr, ptr, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int, ptr, C.c_int, ptr, C.c_size_t,
                                                             L.c_stream])
    # the kernels are in their own file, included by the one translation unit, and use no atomic
    csrc = os.path.join(ROOT, "snn_automotive_object_detection_amd", "csrc")
    assert '#include "snn_hidden.h"' in open(os.path.join(csrc, "snn_kernels.hip")).read()
    assert "atomic" not in re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "snn_hidden.h")).read())


def _fake():
    fake = (C.c_uint8 * 64)()                                        # never dereferenced: every call is refused on the host
    return fake, C.c_void_p(C.addressof(fake))


def _refused(rc, entry, what):
    assert rc == -1, (what, rc)
    msg = _L().load().snn_last_error()
    assert msg and entry.encode() in msg, (what, msg)


BAD_ROWS = [("null view", dict(view=None)), ("null workspace", dict(ws=None)), ("null result", dict(out=None)), ("unknown layout", dict(view=_view(layout=3))),
            ("split4 with words % 4", dict(view=_view(words=6, layout=1))), ("T' = 0", dict(T=0)), ("T' = steps_formed + 1", dict(T=9)),
            ("a step stride below a plane", dict(view=_view(stride=799))), ("an offset off a word", dict(view=_view(offset=2)))]


@pytest.mark.parametrize("what,over", BAD_ROWS, ids=[b[0] for b in BAD_ROWS])
def test_planes_to_rows_refuses(what, over):
    lib = _L().load()
    keep, ptr = _fake()
    a = dict(ws=ptr, view=_view(), T=8, out=ptr)
    a.update(over)
    v = a["view"]
    _refused(lib.snn_planes_to_rows(a["ws"], C.byref(v) if v is not None else None, a["T"], a["out"], None), "snn_planes_to_rows", what)


BAD_LIF = [("null cur", dict(cur=None)), ("null planes", dict(z=None)), ("null result", dict(out=None)), ("null parameters", dict(p=None)),
           ("gz and gu both null", dict(gz=None, gu=None)), ("Tc = 0", dict(Tc=0)), ("Tc = SNN_MAX_STEPS", dict(Tc=32)), ("R = 0", dict(R=0)),
           ("N = 0", dict(N=0)), ("N > 8192", dict(N=8193, ldc=8200)), ("ldc < N", dict(ldc=39)), ("alpha < 0", dict(alpha=-1.0)),
           ("alpha = inf", dict(alpha=float("inf"))), ("alpha = nan", dict(alpha=float("nan"))), ("li_order = 2", dict(p=_params(2)))]


@pytest.mark.parametrize("what,over", BAD_LIF, ids=[b[0] for b in BAD_LIF])
def test_lif_surrogate_bwd_refuses(what, over):
    lib = _L().load()
    keep, ptr = _fake()
    a = dict(cur=ptr, ldc=64, z=ptr, Tc=11, R=7, N=40, p=_params(), alpha=100.0, gz=ptr, gu=ptr, out=ptr)
    a.update(over)
    p = a["p"]
    rc = lib.snn_lif_surrogate_bwd(a["cur"], a["ldc"], a["z"], a["Tc"], a["R"], a["N"], C.byref(p) if p is not None else None, a["alpha"], a["gz"],
                                   a["gu"], a["out"], None)
    _refused(rc, "snn_lif_surrogate_bwd", what)


BAD_WGRAD = [("null planes", dict(a=None)), ("null d_cur", dict(d=None)), ("null result", dict(gw=None)), ("T' = 0", dict(T=0)), ("T' = 33", dict(T=33)),
             ("rows = 0", dict(rows=0)), ("rows = 2^31", dict(rows=2 ** 31)), ("K = 0", dict(K=0)), ("K > 8192", dict(K=8193)), ("N = 0", dict(N=0)),
             ("N > 8192", dict(N=8193, ldd=8200)), ("ldd < N", dict(ldd=95)), ("ldd = 2^28", dict(ldd=2 ** 28)), ("accumulate = 2", dict(acc=2)), ("short scratch", dict(short=4)),
             ("null scratch", dict(scratch=None))]


@pytest.mark.parametrize("what,over", BAD_WGRAD, ids=[b[0] for b in BAD_WGRAD])
def test_spike_linear_wgrad_refuses(what, over):
    lib = _L().load()
    keep, ptr = _fake()
    a = dict(a=ptr, d=ptr, ldd=96, T=11, rows=130, K=160, N=96, gw=ptr, acc=0, scratch=ptr, short=0)
    a.update(over)
    need = lib.snn_spike_linear_wgrad_workspace_bytes(130, 160, 96, 11)
    assert need > 0
    rc = lib.snn_spike_linear_wgrad(a["a"], a["d"], a["ldd"], a["T"], a["rows"], a["K"], a["N"], a["gw"], a["acc"], a["scratch"], need - a["short"], None)
    _refused(rc, "snn_spike_linear_wgrad", what)


def test_workspace_bytes_is_monotone_and_zero_outside_the_limits():
    q = _L().load().snn_spike_linear_wgrad_workspace_bytes
    rows = (1, 63, 64, 65, 257, 511, 512, 513, 1024, 1031, 7680, 7681, 32769, 2 ** 31 - 1)
    dims = (1, 32, 96, 160, 1024, 8192)
    steps = (1, 2, 3, 11, 12, 31, 32)
    for K in dims:
        for N in dims:
            for T in steps:
                sizes = [q(r, K, N, T) for r in rows]
                assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (K, N, T, sizes)
            for r in rows:
                sizes = [q(r, K, N, T) for T in steps]
                assert sizes == sorted(sizes), (r, K, N, sizes)
    for r in rows:
        for T in (1, 11):
            for N in dims:
                sizes = [q(r, K, N, T) for K in dims]
                assert sizes == sorted(sizes) and len(set(sizes)) == len(sizes)
                assert sizes == [q(r, N, K, T) for K in dims]                  # (symmetric in K and N)
    # consecutive reduction lengths: the slab count never drops
    sizes = [q(m, 32, 32, 1) for m in range(1, 9000)]
    assert sizes == sorted(sizes) and sizes[0] == 32 * 32 * 4 and sizes[-1] == 16 * 32 * 32 * 4
    assert q(1024, 1024, 1024, 11) == 16 * 1024 * 1024 * 4 and q(130, 160, 96, 3) == 1 * 160 * 96 * 4 and q(513, 32, 32, 1) == 2 * 32 * 32 * 4
    for bad in ((0, 32, 32, 1), (2 ** 31, 32, 32, 1), (10, 0, 32, 1), (10, 8193, 32, 1), (10, 32, 0, 1), (10, 32, 8193, 1), (10, 32, 32, 0), (10, 32, 32, 33),
                (-1, 32, 32, 1)):
        assert q(*bad) == 0, bad


def test_the_new_kernels_keep_the_register_budget_the_design_states(tmp_path):
    """the code object's own metadata (llvm-readelf --notes; no GPU): no kernel of csrc/snn_hidden.h spills or uses scratch, and the weight-gradient
    kernel fits 256 registers per lane - vector + accumulator, one unified file on gfx950 - which is what lets two of its 256-thread work-groups
    share a CU, two waves per SIMD (DESIGN.md 4.15 argues from that occupancy)"""
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
        if not name or not re.match(r"_Z\d+k_(planes_to_rows|lif_surrogate_bwd|spike_wgrad_partial|spike_wgrad_reduce)", name.group(1)):
            continue
        f = {k: int(re.search(r"\.%s:\s+(\d+)" % k, block).group(1)) for k in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
        f["agpr_count"] = int(re.match(r"\s*(\d+)", block).group(1))
        seen[re.match(r"_Z\d+(k_[a-z_]+?)(\d|P)", name.group(1)).group(1)] = f
    assert sorted(seen) == ["k_lif_surrogate_bwd", "k_planes_to_rows", "k_spike_wgrad_partial", "k_spike_wgrad_reduce"], sorted(seen)
    for k, f in seen.items():
        assert f["private_segment_fixed_size"] == 0 and f["vgpr_spill_count"] == 0 and f["sgpr_spill_count"] == 0, (k, f)
    w = seen["k_spike_wgrad_partial"]
    assert w["vgpr_count"] + w["agpr_count"] <= 256, w
    assert seen["k_lif_surrogate_bwd"]["vgpr_count"] <= 64 and seen["k_planes_to_rows"]["vgpr_count"] <= 64       # 8 waves per SIMD


def test_wrappers_refuse_cpu_tensors():
    from snn_automotive_object_detection_amd import hidden
    with pytest.raises(Exception, match="GPU"):
        hidden.planes_to_rows(torch.zeros(64, dtype=torch.uint8), _view(2, 1, 0, 1), 1)
    with pytest.raises(Exception, match="GPU"):
        hidden.lif_surrogate_bwd(torch.zeros(1, 2, 32), torch.zeros(2, 2, 1, dtype=torch.int32), 32, _params(), 100.0, gu=torch.zeros(2, 32))
    with pytest.raises(Exception, match="GPU"):
        hidden.spike_linear_wgrad(torch.zeros(1, 2, 1, dtype=torch.int32), torch.zeros(1, 2, 32), 32, 32)


def test_train_fc7_defaults_off_and_refuses_what_it_cannot_differentiate():
    import snn_automotive_object_detection_amd as S
    d = S.FastRCNNPredictorSNNFull(49 * 8, 32, 3, 4)
    assert d.train_fc7 is False and float(d.p_lif.alpha) == 100.0
    x = torch.randn(2, 8, 7, 7)
    d.train_fc7 = d.spike_rates = True
    with pytest.raises(NotImplementedError, match="train_fc7"):
        d(x)
    d.spike_rates = False
    for prec in ("bf16", "mxfp6"):
        d.precision = prec
        with pytest.raises(NotImplementedError, match="train_fc7"):
            d(x)
        with pytest.raises(NotImplementedError, match="train_fc7"):
            d.forward_roialign([torch.randn(1, 8, 8, 8)], [1.0], torch.zeros(2, 5), torch.zeros(2, dtype=torch.int32))


def test_attach_refuses_a_pass_that_formed_too_few_lif6_planes_and_short_passes():
    """hidden.attach checks lif6's view before anything touches a device: a pass that formed fewer than T - 1 lif6 planes, and T < 3"""
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import hidden
    L = _L()
    d = S.FastRCNNPredictorSNNFull(49 * 8, 32, 3, 6)
    outs = (torch.zeros(4, 3), torch.zeros(4, 12))
    ws = torch.zeros(64, dtype=torch.uint8)                          # never read: the refusal comes first
    short, full = _view(rows=4, words=1, steps=4), _view(rows=4, words=1, steps=6)
    with pytest.raises(L.SnnHipError, match="formed 4 lif6 planes, the gradient needs 5"):
        hidden.attach(d, outs, ws, short, full, 6, _params(), "bf16x3")
    for T in (1, 2):
        with pytest.raises(ValueError, match="num_steps >= 3"):
            hidden.attach(d, outs, ws, full, full, T, _params(), "bf16x3")
    with pytest.raises(Exception, match="GPU"):                      # enough planes: the next thing is the copy out of the workspace, which needs a device
        hidden.attach(d, outs, ws, _view(rows=4, words=1, steps=5), full, 6, _params(), "bf16x3")


def test_freeze_below_fc7_leaves_three_trainable_parameters_on_a_detector_head():
    import snn_automotive_object_detection_amd as S
    from snn_automotive_object_detection_amd import hidden
    d = S.FastRCNNPredictorSNNFull(49 * 8, 32, 3, 4)
    keep = hidden.freeze_below_fc7(d)
    assert [id(w) for w in keep] == [id(d.fc7.weight), id(d.cls_score.weight), id(d.bbox_pred.weight)]
    assert sorted(n for n, q in d.named_parameters() if q.requires_grad) == ["bbox_pred.weight", "cls_score.weight", "fc7.weight"]
    assert not d.fc6.weight.requires_grad
    h = S.RPNHeadSNN(32, 3, 4)                                       # an RPN head keeps its readout weights, as freeze_hidden keeps them
    assert len(hidden.freeze_below_fc7(h)) == 2 and sorted(n for n, q in h.named_parameters() if q.requires_grad) == ["conv_bbox.weight", "conv_cls.weight"]


# ---- the recurrence is the reference's gradient ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Tc", (1, 2, 11))
@pytest.mark.parametrize("name", ("reference", "other"))
@pytest.mark.parametrize("alpha", (100.0, 1.0))
def test_the_adjoint_is_autograd_through_lif_feed_forward_step_with_superspike(Tc, name, alpha):
    c = HG.REFERENCE if name == "reference" else HG.OTHER
    R, N = 7, 40
    cur = HG.draw_currents(Tc, R, N, N, 0.5, c, [Tc, R, N, 1]).to(torch.float64).requires_grad_(True)
    z = HG.lif_forward_autograd(cur, c, alpha)                       # spikes taken from the forward itself
    assert torch.equal(z.detach().bool(), HG.lif_forward(cur.detach(), c))
    assert Tc < 2 or 0.05 < float(z.detach().mean()) < 0.95
    g = torch.Generator().manual_seed(Tc)
    gz = torch.randn(z.shape, generator=g, dtype=torch.float64)
    want, = torch.autograd.grad((z * gz).sum(), cur, retain_graph=True)
    got = HG.adjoint(cur.detach(), z.detach().bool(), c, alpha, gz=gz)
    assert float(want.abs().max()) > 0
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), float((got - want).abs().max()) / float(want.abs().max())
    # gz_t = kappa_t gu is the same thing as a readout gradient folded over time
    gu = torch.randn((R, N), generator=g, dtype=torch.float64)
    for order in ("jump_first", "voltage_first"):
        k = HG.kappa(c, Tc + 1, order, torch.float64)
        want, = torch.autograd.grad((z * (torch.from_numpy(k)[:, None, None] * gu)).sum(), cur, retain_graph=True)
        got = HG.adjoint(cur.detach(), z.detach().bool(), c, alpha, gu=gu, kappa=k)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_kappa_of_the_restatement_is_the_readouts_impulse_response():
    """out = W sum_t kappa_t z_t: the LI recursion of tests/_planes.py on a single spike at step s ends at kappa[s]"""
    from tests import _planes as PL
    c = HG.REFERENCE
    for order in ("jump_first", "voltage_first"):
        k = HG.kappa(c, 6, order, torch.float64)
        for s in range(6):
            spk = np.zeros((6, 1, 1))
            spk[s] = 1.0
            last, _ = PL.li_fp64(spk, np.ones((1, 1)), c.a, -c.b, order)
            assert abs(last[-1, 0, 0] - k[s]) <= 1e-15, (order, s)


def test_pack_and_unpack_bits_round_trip():
    z = torch.rand(3, 5, 40) < 0.3
    for pad in (False, True):
        w = HG.pack_bits(z, pad)
        assert w.shape == (3, 5, 2) and torch.equal(HG.unpack_bits(w, 40), z)
        assert bool(((w[:, :, 1].numpy().view(np.uint32) >> 8) == (0xffffff if pad else 0)).all())
