"""Dyadic weight grids (tests/_exact_grid.py) on the CPU: what makes "zero flips" a fair demand of tests/test_gpu_exact_grid.py.

 * every case builder's assertions hold (units, fp64 round trip, hi + mid + lo == q, row budget, lo != 0 at the planted entries);
 * the oracle's fp32 currents (cur, cur6, cur7) are BIT-EQUAL to an fp64 evaluation of the same contraction - if they were not, the GPU
   test would blame a kernel for the oracle's rounding;
 * the cases are not vacuous: every LIF layer fires at a mean rate in [0.05, 0.5] (exempt: T <= 2 and lif7 at T = 3, which cannot; C = 3
   and the narrow lif6 at T = 3 must fire at all), and the
   full-nibble leg fills the nibbles of the period planes;
 * sensitivity: removing ONE contribution from a current through the oracle's cur_hook changes the hidden planes - one tap x one
   32-channel block at every position, one whole tap at the four corner positions of the smallest level, the lo plane of the planted
   wide weights.  With the hook a no-op the planes are the case's own and these tests fail."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import snn_oracle as OR
from tests import _exact_grid as G
from tests._sentinels import split3
from tests._util import nchw_to_rows

CASES = G.all_cases()


def _fp64_equal(cur32: torch.Tensor, cur64: torch.Tensor) -> bool:
    return torch.equal(cur32.double(), cur64)


@pytest.mark.parametrize("name,build", CASES, ids=[n for n, _ in CASES])
def test_case_is_exact_and_not_vacuous(name, build):
    case = build()
    T = case["T"]
    if case["kind"] == "rpn":
        q = case["w_shared"]
        G.check_grid(q.numpy(), case["info"]["s"], G.BUDGET_LOG2, case["info"]["wide_idx"])
        for tr in case["traces"]:
            z = tr["z"].double().flatten(0, 1)
            cur64 = F.conv2d(z, q.double(), padding=1).view(tr["cur"].shape)
            assert _fp64_equal(tr["cur"], cur64), float((tr["cur"].double() - cur64).abs().max())
        rates = {"shared": case["rate"]}
        if T <= 2:
            rates = {}                                               # the shared LIF cannot reach its threshold in two steps
        elif case["C"] < 32:                                         # 27 inputs of N(0, 0.04): the layer fires, below the floor (0.016 at C = 3)
            assert case["rate"] > 0
            rates = {}
    else:
        tr = case["trace"]
        for q, info, x, cur in ((case["w6"], case["info6"], tr["z"], tr["cur6"]), (case["w7"], case["info7"], tr["spk6"], tr["cur7"])):
            G.check_grid(q.numpy(), info["s"], G.BUDGET_LOG2, info["wide_idx"])
            assert _fp64_equal(cur, x.double() @ q.double().T)
        rates = {"lif6": case["rate6"], "lif7": case["rate7"]}
        if T <= 2:
            rates = {}                                               # lif6 fires from step 1 on at the earliest, lif7 from step 2
        elif T == 3:                                                 # lif7 has one step to fire in; on the narrow grid (no planted weights, fc6 as initialised)
            rates.pop("lif7")                                        # lif6 has barely started as well: it must fire, the floor comes with more steps
            if case["grid"] == "narrow":
                assert rates.pop("lif6") > 0
    if case["grid"] == "wide":
        infos = [case["info"]] if case["kind"] == "rpn" else [case["info6"], case["info7"]]
        assert all(i["n_wide"] >= 1 for i in infos)
    assert all(0.05 <= r <= 0.5 for r in rates.values()), rates


@pytest.mark.parametrize("M,K,N", G.GEMM_SHAPES)
@pytest.mark.parametrize("grid", ["wide", "narrow"])
def test_gemm_stage_case_is_exact(M, K, N, grid):
    """the stage-level GEMM cases: the oracle's F.linear is bit-equal to fp64, so torch.equal is a fair demand of the kernels"""
    c = G.gemm_case(M, K, N, M + N, grid)
    G.check_grid(c["w"].numpy(), c["info"]["s"], G.BUDGET_LOG2, c["info"]["wide_idx"])
    assert _fp64_equal(c["cur"], c["z"].double() @ c["w"].double().T)
    assert 0.1 <= float(c["z"].mean()) <= 0.6 and float(c["cur"].abs().max()) > 0


def test_mx_pack_definition_carries_the_grids():
    """mxfp6 is in scope only if its pack definition carries the grids exactly: every weight within 28 bits of its block's maximum.
    The wide grid spans at most 20 bits per row, the narrow one 7."""
    for build in (lambda: G.rpn_t_case(256, 8), lambda: G.rpn_t_case(256, 8, "narrow"), G.det_mx_case, lambda: G.det_mx_case("narrow")):
        case = build()
        pairs = [(case["w_shared"], case["info"])] if case["kind"] == "rpn" else [(case["w6"], case["info6"]), (case["w7"], case["info7"])]
        for q, info in pairs:
            assert G.mx_block_span_bits(q, info["s"]) <= 20


def test_full_nibble_leg_fills_the_nibbles():
    """at least half of the 16-row tiles hold a nibble with >= 3 ones in a period plane e_3 .. (here: every occupied nibble is full)"""
    c = G.rpn_full_nibble_case()
    z = np.concatenate([nchw_to_rows(tr["z"]) for tr in c["traces"]], axis=1)
    frac, partial = G.nibble_hit_fraction(z)
    assert frac >= 0.5 and partial == 0, (frac, partial)
    d = G.det_full_nibble_case()
    zr = d["trace"]["z"].numpy().reshape(d["T"], d["R"], d["C"], 49).transpose(0, 1, 3, 2).reshape(d["T"], d["R"], 49 * d["C"])   # k' = bin * C + c
    frac, partial = G.nibble_hit_fraction(zr)
    assert frac >= 0.5 and partial == 0, (frac, partial)
    g = torch.Generator().manual_seed(1)                             # and N(0, 1.7) features do not: the leg adds something
    assert G.nibble_hit_fraction(OR.encoder_spikes(torch.randn(64, 256, generator=g) * 1.7, 8).numpy())[1] > 0


# ---- sensitivity -------------------------------------------------------------------------------------------------------------------------
def _rpn_planes_with(case, hook, levels=None):
    feats = case["feats"] if levels is None else [case["feats"][l] for l in levels]
    with torch.no_grad():
        _, _, tr = OR.rpn_head_forward(feats, case["w_shared"], case["w_cls"], case["w_bbox"], case["T"], trace=True, cur_hook=hook)
    return [t["spk"] for t in tr]


def _one_level_hook(case, level, contribution):
    """cur_hook for an oracle run on ONE level: subtracts contribution(z of that step) from the shared conv's current (exact: both
    are integers of units)"""
    z_all = case["traces"][level]["z"]
    return lambda name, step, cur: cur - contribution(z_all[step])


@pytest.mark.parametrize("C,T", [(64, 8), (256, 8), (64, 16)])
def test_rpn_planes_feel_one_tap_of_one_channel_block(C, T):
    case = G.rpn_t_case(C, T)
    w = case["w_shared"]
    for tap, blk in [(0, 0), (4, C // 32 - 1), (8, C // 64)]:
        part = torch.zeros_like(w)
        part[:, 32 * blk: 32 * blk + 32, tap // 3, tap % 3] = w[:, 32 * blk: 32 * blk + 32, tap // 3, tap % 3]
        for l in range(len(case["shapes"])):
            if l == 2 and tap != 4:
                continue                                             # (the 2 x 1 level: taps of column 0 / 2 read padding only)
            spk = _rpn_planes_with(case, _one_level_hook(case, l, lambda z: F.conv2d(z, part, padding=1)), [l])[0]
            assert not torch.equal(spk, case["traces"][l]["spk"]), (tap, blk, l)


@pytest.mark.parametrize("C,T", [(64, 8), (256, 8)])
def test_rpn_planes_feel_one_tap_at_the_corners_of_the_smallest_level(C, T):
    case = G.rpn_case(C, 3, T, ((13, 17), (6, 7), (3, 2)), 2, C + T + 1)
    w = case["w_shared"]
    l = 2
    H, W = case["shapes"][l]
    corners = torch.zeros(1, 1, H, W)
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)):
        corners[0, 0, y, x] = 1.0
    for tap in (4, 8, 0):                                            # the centre, and the two diagonal taps (each inside the map at one corner)
        part = torch.zeros_like(w)
        part[:, :, tap // 3, tap % 3] = w[:, :, tap // 3, tap % 3]
        spk = _rpn_planes_with(case, _one_level_hook(case, l, lambda z: F.conv2d(z, part, padding=1) * corners), [l])[0]
        ref = case["traces"][l]["spk"]
        assert not torch.equal(spk, ref), tap
        assert torch.equal(spk * (1 - corners), ref * (1 - corners))           # ... and nowhere else


@pytest.mark.parametrize("C,T", [(256, 8), (64, 16)])
def test_rpn_planes_feel_the_lo_plane_of_the_planted_weights(C, T):
    case = G.rpn_t_case(C, T)
    lo = G.lo_of_planted(case["w_shared"], case["info"]["wide_idx"])
    assert int((lo != 0).sum()) == case["info"]["wide_idx"].size
    l = 0
    spk = _rpn_planes_with(case, _one_level_hook(case, l, lambda z: F.conv2d(z, lo, padding=1)), [l])[0]
    assert not torch.equal(spk, case["traces"][l]["spk"])


@pytest.mark.parametrize("what", ["block6", "lo6", "lo7"])
def test_det_planes_feel_one_block_and_the_lo_planes(what):
    # (lo7: one or two units of 2^-18 on a handful of fc7 inputs move a spike only in a neuron within ~1e-5 of its threshold - more RoIs, units and steps)
    case = G.det_case(513, 32, 256, 9, 16, 7) if what == "lo7" else G.det_case(257, 64, 128, 9, 12, 300 + 257)
    tr = case["trace"]
    if what == "block6":                                             # one 32-channel block of one bin, at every RoI
        part = torch.zeros_like(case["w6"]).view(128, 64, 49)
        part[:, 32:64, 24] = case["w6"].view(128, 64, 49)[:, 32:64, 24]
        part, layer, x = part.view(128, -1), "fc6", tr["z"]
    elif what == "lo6":
        part, layer, x = G.lo_of_planted(case["w6"], case["info6"]["wide_idx"]), "fc6", tr["z"]
    else:
        part, layer, x = G.lo_of_planted(case["w7"], case["info7"]["wide_idx"]), "fc7", tr["spk6"]
    state = {}

    def hook(name, step, cur):
        if name == "fc6":
            state["z"] = x[step] if layer == "fc6" else None
        if name != layer:
            return cur
        if layer == "fc7":                                           # teacher-forced on the case's own spk6 (fc6 is untouched, so it is the run's too)
            return cur - F.linear(x[step], part)
        return cur - F.linear(state["z"], part)
    with torch.no_grad():
        _, _, got = OR.det_head_forward(case["x"], case["w6"], case["w7"], case["w_cls"], case["w_bbox"], case["T"], trace=True, cur_hook=hook)
    key = "spk6" if layer == "fc6" else "spk7"
    assert not torch.equal(got[key], tr[key]), what


def test_builders_are_deterministic_and_grids_differ():
    a = G.rpn_case.__wrapped__(64, 3, 8, G.PYRAMID, 2, 9)
    b = G.rpn_case.__wrapped__(64, 3, 8, G.PYRAMID, 2, 9)
    assert a["w_shared"].numpy().tobytes() == b["w_shared"].numpy().tobytes() and np.array_equal(a["spk"], b["spk"])
    n = G.rpn_case.__wrapped__(64, 3, 8, G.PYRAMID, 2, 9, "narrow")
    hi, mid, lo = split3(n["w_shared"].numpy())
    assert not mid.any() and not lo.any()                            # one plane carries the narrow grid
    hi, mid, lo = split3(a["w_shared"].numpy())
    assert (mid != 0).mean() > 0.5 and int((lo != 0).sum()) >= a["info"]["wide_idx"].size
