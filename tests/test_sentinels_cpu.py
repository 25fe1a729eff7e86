"""Sentinel neurons (tests/_sentinels.py) on the CPU: the host prediction equals the oracle (oracle/snn_oracle.py) on every configuration
the GPU tests use, in small instances, and the GPU tests' own assertion fails for every weight mutant a kernel bug could produce (a
lost or doubled weight plane, bf16 weights, one ulp on every weight) - the proof that tests/test_gpu_sentinels.py bites."""
import numpy as np
import pytest
import torch

from oracle import snn_oracle as OR
from tests import _sentinels as S

# (C, A, T, shapes, all_sentinel, li_order): small twins of the GPU configurations (T 5 / 8 / 12 / 16: the 8-wave, FAT 4x1 and
# FAT 2x2 conv instances; odd, 1x1 and 1x3 levels; both LI orders; the all-sentinel spike-rate configuration)
RPN_CASES = [(64, 3, 5, [(5, 7), (1, 1)], False, "jump_first"),
             (64, 3, 8, [(6, 5), (1, 3)], False, "jump_first"),
             (64, 3, 12, [(3, 4), (1, 1)], False, "voltage_first"),
             (64, 3, 16, [(5, 3), (1, 3)], False, "jump_first"),
             (64, 3, 8, [(4, 5), (1, 1), (1, 3)], True, "jump_first")]
DET_CASES = [(32, 64, 9, 8, 3, "jump_first"), (32, 64, 9, 12, 2, "voltage_first"), (32, 64, 9, 24, 2, "jump_first")]


def _rpn_oracle(case, w_shared=None, w_cls=None, w_bbox=None, counts=None, trace=False):
    return OR.rpn_head_forward(case["feats"], case["w_shared"] if w_shared is None else w_shared,
                               case["w_cls"] if w_cls is None else w_cls, case["w_bbox"] if w_bbox is None else w_bbox,
                               case["T"], li_order=case["li_order"], counts_out=counts, trace=trace)


def _det_oracle(case, w6=None, w7=None, wc=None, wb=None, trace=False):
    return OR.det_head_forward(case["x"], case["w6"] if w6 is None else w6, case["w7"] if w7 is None else w7,
                               case["w_cls"] if wc is None else wc, case["w_bbox"] if wb is None else wb, case["T"],
                               li_order=case["li_order"], trace=trace)


@pytest.fixture(scope="module", params=range(len(RPN_CASES)), ids=lambda i: "rpn%d" % i)
def rpn(request):
    C, A, T, shapes, alls, order = RPN_CASES[request.param]
    return S.rpn_case(C, A, T, shapes, N=2, seed=request.param, li_order=order, all_sentinel=alls)


@pytest.fixture(scope="module", params=range(len(DET_CASES)), ids=lambda i: "det%d" % i)
def det(request):
    C, Hd, K, T, R, order = DET_CASES[request.param]
    return S.det_case(C, Hd, K, T, R, seed=request.param, li_order=order)


def test_rpn_prediction_equals_oracle(rpn):
    counts = []
    out = _rpn_oracle(rpn, counts=counts, trace=True)
    traces = out[2]
    for l, (H, W) in enumerate(rpn["shapes"]):
        spk = traces[l]["spk"].numpy()                               # [T, N, C, H, W]
        for hs in rpn["hidden"]:                                     # hidden trains: bit for bit, inside the map; none in the padding
            m = S._tap_inside(H, W, hs["tap"])
            got = spk[:, :, hs["channel"]]
            assert np.array_equal(got[:, :, m], np.broadcast_to(hs["train"][:, None, None], got[:, :, m].shape)), (l, hs["channel"])
            assert not got[:, :, ~m].any()
    bad, mx = S.check_levels(S.rpn_outputs(out[0], out[1]), rpn, "oracle_tol")
    assert bad == 0, (bad, mx)
    if rpn["counts"] is not None:
        assert np.array_equal(torch.stack(counts).numpy(), rpn["counts"])
    # every sentinel weight splits into nonzero planes where the design says so, and the head bound is a quarter of a lo-plane shift
    for hd in rpn["heads"]:
        _, m, lo = S.split3(np.array([hd["u"]], dtype=np.float32))
        assert abs(lo[0]) >= 2.0 ** -18 * abs(hd["u"]) and m[0] != 0
    _tolerance_vs_shift(rpn["heads"], [rpn["hidden"][hd["hidden"]]["train"] for hd in rpn["heads"]], rpn["T"], rpn["li_order"])


def test_det_prediction_equals_oracle(det):
    cls, bbox, tr = _det_oracle(det, trace=True)
    s6, s7 = tr["spk6"].numpy(), tr["spk7"].numpy()
    for u in det["units6"]:
        assert np.array_equal(s6[:, :, u["unit"]], np.broadcast_to(u["train"][:, None], s6[:, :, u["unit"]].shape))
    for u in det["units7"]:
        assert np.array_equal(s7[:, :, u["unit"]], np.broadcast_to(u["train"][:, None], s7[:, :, u["unit"]].shape))
    bad, mx = S.check(S.det_outputs(cls, bbox), det["exp"], det["oracle_tol"])
    assert bad == 0, (bad, mx)
    _tolerance_vs_shift(det["heads"], [hd["src"]["train"] for hd in det["heads"]], det["T"], det["li_order"])


def _tolerance_vs_shift(heads, trains, T, order):
    """the bound of every head sentinel that fires at most twice is at most a quarter of the smallest output shift a lost / doubled
    plane of its weight causes"""
    kap = S.kappa64(T, order)
    n_checked = 0
    for hd, tr in zip(heads, trains):
        n = int(tr.sum())
        if n == 0 or n > 2:
            continue
        u = hd["u"]
        tol = S.head_tolerance(n, float(np.sum(kap[tr])) * abs(u))
        exp = S.li_last64(u, tr, order)[0]
        shifts = [abs(S.li_last64(float(S.mutate_np(np.array([u]), how)[0]), tr, order)[0] - exp)
                  for how in ("hi_only", "hi_mid", "no_mid", "lo_doubled", "bf16")]
        assert tol <= 0.25 * min(shifts), (u, tol, shifts)
        assert S.ulps(np.array([tol]), np.array([exp]))[0] <= 4.0 * n       # <= 4 ulps for a single spike
        n_checked += 1
    assert n_checked >= 1


@pytest.mark.parametrize("how", S.MUTANTS)
def test_rpn_sentinels_catch_every_mutant(rpn, how):
    ws, wc, wb = (S.mutate(w, how) for w in (rpn["w_shared"], rpn["w_cls"], rpn["w_bbox"]))
    # the shared conv alone (its boundary pairs), the heads alone (their plane shifts), and both
    for args in ((ws, None, None), (None, wc, wb), (ws, wc, wb)):
        if how.startswith("ulp") and args[0] is None:
            continue                                    # one ulp of a head weight is within the head's ulp bound by design
        counts = []
        out = _rpn_oracle(rpn, *args, counts=counts)
        bad, _ = S.check_levels(S.rpn_outputs(out[0], out[1]), rpn)
        if rpn["counts"] is not None and args[0] is not None:
            bad += int(not np.array_equal(torch.stack(counts).numpy(), rpn["counts"]))
        assert bad > 0, (how, [a is not None for a in args])


@pytest.mark.parametrize("how", S.MUTANTS)
def test_det_sentinels_catch_every_mutant(det, how):
    m6, m7, mc, mb = (S.mutate(w, how) for w in (det["w6"], det["w7"], det["w_cls"], det["w_bbox"]))
    cases = [(m6, None, None, None), (None, m7, None, None)]
    if not how.startswith("ulp"):
        cases.append((None, None, mc, mb))
    for args in cases:
        cls, bbox = _det_oracle(det, *args)
        bad, _ = S.check(S.det_outputs(cls, bbox), det["exp"], det["tol"])
        assert bad > 0, (how, [a is not None for a in args])


def test_builders_are_deterministic():
    a = S.rpn_case(64, 3, 8, [(3, 5), (1, 1)], seed=4)
    b = S.rpn_case(64, 3, 8, [(3, 5), (1, 1)], seed=4)
    for k in ("w_shared", "w_cls", "w_bbox"):
        assert a[k].numpy().tobytes() == b[k].numpy().tobytes()
    assert all(x.numpy().tobytes() == y.numpy().tobytes() for x, y in zip(a["feats"], b["feats"]))
    assert all(np.array_equal(x, y) for x, y in zip(a["exp"], b["exp"]))
    c = S.det_case(32, 64, 9, 12, 3, seed=1)
    d = S.det_case(32, 64, 9, 12, 3, seed=1)
    for k in ("w6", "w7", "w_cls", "w_bbox", "x"):
        assert c[k].numpy().tobytes() == d[k].numpy().tobytes()
    assert np.array_equal(c["exp"], d["exp"])


def test_step_functions_equal_the_oracle_cells():
    """the fp32 encoder / LIF of tests/_sentinels.py against the oracle's own on a grid of inputs and weights"""
    xs = torch.tensor([S.period_input(p) for p in (1, 2, 3, 4, 5, 7)] + [0.3, 0.26, 0.9, 2.5, 13.0])
    z = OR.encoder_spikes(xs, 20).numpy().astype(bool)
    for j, x in enumerate(xs.tolist()):
        assert np.array_equal(z[:, j], S.encoder_train(x, 20))
    sched = S.period_sched(3, 20)
    ws = np.geomspace(0.01, 2.0, 57).astype(np.float32)
    cur = torch.from_numpy(np.outer(sched.astype(np.float32), ws))
    spk, _, _ = OR.lif_scan_from_currents(cur)
    for j, w in enumerate(ws):
        assert np.array_equal(spk[:, j].numpy().astype(bool), S.lif_train(float(w), sched))
