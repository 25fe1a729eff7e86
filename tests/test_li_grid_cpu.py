"""Preconditions and sensitivity of the LI-head grid (tests/_li_grid.py), on the host: what tests/test_gpu_li_grid.py relies on when it
compares every kernel form of the LI heads with torch.equal.

  * the neuron constants give dyadic (a, b), and kappa in rationals reproduces the table the grid is built on; the launcher's kappa
    (double recursion, one cast to fp32) equals it wherever a combination is admitted;
  * for EVERY case of the grid the integer expectation converts to fp32 without loss, tests/_planes.li_fp64 and the fp32 oracle equal it bit
    for bit, and three fp32 summation orders emulated in numpy (t-ascending chain, k-ascending chain over kappa-folded spikes, four
    k-quarters) equal it - the budget is not vacuous;
  * each mutant (one wrong term of the kind a kernel or the launcher could have) changes the expectation's bits on every readout it applies to;
  * a combination outside the table or the budget RAISES (BudgetError); nothing is skipped."""
import collections

import numpy as np
import pytest
import torch

from oracle import snn_oracle as OR
from tests import _li_grid as L
from tests._planes import li_constants, li_fp64

Fr = L.Fr
STAGE = dict(L.stage_grid())
HEADS = L.HEAD_CASES


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ---- constants and kappa -------------------------------------------------------------------------------------------------------------------
def test_the_sets_are_dyadic_through_the_fp32_products():
    assert len(STAGE) == len(L.stage_grid()) and len(HEADS) == len(L.head_grid())                 # case ids are unique
    for name, (a, b) in L.SET_AB.items():
        k = L.SETS[name]
        assert L.set_ab(name) == (a, b)
        assert Fr(k.ca) == a and Fr(k.cb) == -b                      # what tests/_neuron_constants.abi_params hands the C ABI


@pytest.mark.parametrize("name", sorted(L.SETS))
def test_kappa_reproduces_the_table(name):
    last_ok, last_no, sums_ok, sums_no = L.KAPPA_TABLE[name]
    for T in last_ok:
        assert L.kappa_admits(name, T, "jump_first", False), T
    for T in sums_ok:
        assert L.kappa_admits(name, T, "jump_first", True), T
    if last_no is not None:
        assert not L.kappa_admits(name, last_no, "jump_first", False)
    if sums_no is not None:
        assert not L.kappa_admits(name, sums_no, "jump_first", True)
    for (n, q), sig in L.KAPPA_SIG.items():
        if n == name:
            for T, bits in sig.items():
                assert L.kappa_of(name, T, "jump_first")["sig_" + q] == bits, (q, T)
    for T in range(1, 33):
        for order in L.ORDERS:
            k = L.kappa_of(name, T, order)
            if order == "voltage_first":
                assert k["last"][T - 1] == 0 and k["sum"][T - 1] == 0    # the last step's spikes contribute exactly nothing
            if name == "a2_b2":
                assert k["sig_last"] <= 5 and k["fb_last"] <= T and k["sig_sum"] <= T + 1   # (the table's "sig = T" holds at its even T; odd T carry one bit more)
            if name == "a2_b1":                                      # one bit each, all distinct
                nz = [f for f in k["last"] if f != 0]
                assert all(L._sig_bits(f) == 1 for f in nz) and len(set(nz)) == len(nz) and k["sig_sum"] <= T + 1
            if name == "pm1":
                assert all(abs(f) == 1 for f in k["last"] if f != 0) and set(k["sum"]) <= {Fr(0), Fr(1)}
                assert all(k["last"][t] == -k["last"][t + 1] for t in range(T - 1) if k["last"][t + 1] != 0)


@pytest.mark.parametrize("name", sorted(L.SETS))
def test_the_launchers_kappa_is_the_rational_one_wherever_admitted(name):
    """li_kappa runs the recursion in double and casts once: on an admitted combination that is the exact value"""
    a, b = li_constants(L.SETS[name])
    n = 0
    for T in range(1, 33):
        for order in L.ORDERS:
            last, tot = L.kappa_fp32(a, b, T, order)
            k = L.kappa_of(name, T, order)
            if L.kappa_admits(name, T, order, False):
                assert [Fr(float(x)) for x in last] == list(k["last"]), (T, order)
                n += 1
            if L.kappa_admits(name, T, order, True):
                assert [Fr(float(x)) for x in tot] == list(k["sum"]), (T, order)
    assert n >= 2 * L.T_MAX_LAST[name]


def test_what_the_budget_refuses_is_listed_and_raises():
    """inside T_MAX_* the only combination the kappa table admits and the fold bound refuses is FOLD_REFUSED; the builders raise on it, on a
    T beyond the table, and on sums the table does not admit"""
    refused = [(n, T, o, s) for n in L.SETS for T in range(1, 33) for o in L.ORDERS for s in (False, True)
               if L.kappa_admits(n, T, o, s) and T <= (L.T_MAX_SUMS if s else L.T_MAX_LAST)[n] and not L.admitted(n, T, o, s)
               and T in L.T_DYADIC + L.T_PM1]
    assert tuple(refused) == L.FOLD_REFUSED
    for kw in (dict(T=12, name="a2_b4", sums=False), dict(T=16, name="a2_b4", sums=False), dict(T=12, name="a2_b4", li_order="voltage_first", sums=True),
               dict(T=17, name="a2_b2", sums=False), dict(T=17, name="a2_b1", sums=True)):
        with pytest.raises(L.BudgetError):
            L.stage_case(M=17, K=128, NA=3, NB=12, **kw)
    # every (set, T) of the issue's T edges is either in the grid or refused above: nothing dropped silently
    ids = set(STAGE)
    for M, K, NA, NB, T, name, sums in L.t_cases():
        for order in L.ORDERS:
            cid = "T%d_%s_%dx%dx%d_%s" % (T, name, M, K, NA + NB, order)
            assert (cid in ids) != ((name, T, order, sums) in L.FOLD_REFUSED), cid


def test_the_grid_reaches_every_edge():
    cases = [L.stage_case(**kw) for kw in STAGE.values()]
    assert {c["M"] for c in cases} >= set(L.M_EDGES)
    assert {(c["K"], c["NA"], c["NB"]) for c in cases} >= set(L.K_EDGES)
    assert {(c["NA"], c["NB"]) for c in cases} >= set(L.N_EDGES)
    assert any(c["NA"] % 4 for c in cases)                           # the A / B column boundary inside a group of four columns
    for name in ("a2_b2", "a2_b1"):
        assert {c["T"] for c in cases if c["set"] == name and len(c["steps"]) == 1} >= set(L.T_DYADIC)
    assert {c["T"] for c in cases if c["set"] == "a2_b4"} >= {1, 2, 4, 5, 8, 9, 10, 12}
    assert {c["T"] for c in cases if c["set"] == "pm1"} >= set(L.T_PM1)
    assert {c["variant"] for c in cases} == {"plain", "wide", "narrow"}
    print("rungs of the ladder taken:", sorted(collections.Counter(c["rung"] for c in cases).items()))


# ---- every case: exact reference side, a budget that is not vacuous, mutants told apart ------------------------------------------------------
def _check_case(c):
    a, b = li_constants(c["constants"])
    last, run = li_fp64(c["spk"], c["w"], a, b, c["li_order"])
    spk_t = torch.from_numpy(c["spk"])
    for j, Tp in enumerate(c["steps"]):
        for q, ref in (("last", last), ("sum", run)) if c["sums"] else (("last", last),):
            exp = c[q][j]
            assert exp.dtype == np.float32
            r32 = ref[Tp - 1].astype(np.float32)
            assert np.array_equal(r32.astype(np.float64), ref[Tp - 1]), "li_fp64 -> fp32 -> fp64 loses bits (%s, T' = %d)" % (q, Tp)
            assert np.array_equal(_bits(r32 + np.float32(0)), _bits(exp + np.float32(0))), (q, Tp)       # (+ 0: the recursion may leave -0 where the integers say 0)
            for order, v in L.emulate_orders(c, j, q).items():
                assert np.array_equal(_bits(v + np.float32(0)), _bits(exp + np.float32(0))), "fp32 order %s differs (%s, T' = %d)" % (order, q, Tp)
        o_last, o_sum = OR.li_last_from_spikes(spk_t[:Tp], c["w"], c["li_order"], constants=c["constants"])
        assert torch.equal(o_last, torch.from_numpy(c["last"][j]))
        if c["sums"]:
            assert torch.equal(o_sum, torch.from_numpy(c["sum"][j]))
    found = L.mutants(c)
    missed = [m for m in found if not m[3]]
    assert not missed, "mutants the expectation does not tell apart: %s" % missed[:6]
    return {m[0] for m in found}


@pytest.mark.parametrize("cid", sorted(STAGE))
def test_stage_case_is_exact_alive_and_tells_every_mutant_apart(cid):
    c = L.stage_case(**STAGE[cid])
    seen = _check_case(c)
    need = {"other_order", "word_dropped"}
    if c["variant"] == "wide":
        need.add("lo_plane_dropped")
    if c["NA"] + c["NB"] > 64:
        need.add("previous_block")
    if len(c["steps"]) > 1:
        need.add("kappa_of_T")
    if c["T"] > 2:
        need |= {"kappa_shifted", "last_sum_swapped", "last_step_dropped"}
    if c["T"] == 1 and c["li_order"] == "voltage_first":             # exact zeros: only the other order differs
        need = {"other_order"}
    assert seen >= need, need - seen
    assert seen <= set(L.MUTANTS)


@pytest.mark.parametrize("cid", sorted(HEADS))
def test_whole_head_case_is_exact_alive_and_tells_every_mutant_apart(cid):
    c = HEADS[cid]()
    for r in L.hidden_rates(c):
        assert 0.02 <= r <= 0.8, "a hidden layer fires at %.3f" % r
    seen = _check_case(c)
    assert seen >= {"kappa_shifted", "other_order", "last_sum_swapped", "word_dropped", "last_step_dropped"}
    # the fp32 oracle's whole-head forward with these head weights IS the expectation
    got = L.oracle_outputs(c)
    assert np.array_equal(_bits(got), _bits(c["last"][-1])), float(np.abs(got - c["last"][-1]).max())
    if c["variant"] == "narrow":
        assert torch.equal(c["w"].to(torch.bfloat16).float(), c["w"])                              # what ops.pack_heads_bf16's rounding leaves unchanged


def test_the_grid_reaches_every_kernel_form():
    """the coverage table in the docstring of tests/test_gpu_li_grid.py, from the launcher's plan as tests/_li_grid.li_plan restates it"""
    plans, by_default, blocks = set(), set(), set()
    for cid, kw in STAGE.items():
        for form in L.FORMS:
            for want_sums in (False, True):
                pl = L.li_plan(kw["K"], kw["NA"], kw["NB"], form, want_sums=want_sums, readouts=len(kw.get("steps", ())))
                plans |= set(pl)
                blocks.add(len(pl))
                if form is None:
                    by_default |= set(pl)
    assert {p[1] for p in plans if p[0] == "valu"} == {64, 32, 16, 8, 4}
    assert {p[1] for p in plans if p[:1] == ("mfma",) and p[2] == "resident"} == {1, 2, 3, 4}
    assert {p[1] for p in plans if p[:1] == ("mfma",) and p[2] == "streamed"} >= {1, 3}
    assert any(p[:1] == ("mfma",) and p[3] for p in by_default) and any(p[:1] == ("mfma",) and not p[3] for p in by_default)    # Kw = 8 line loads and the word loop
    assert {p[1] for p in plans if p[0] == "ksplit"} == {1, 2, 3, 4} and ("ksplit", 3) in by_default
    for kernel in ("mfma", "ksplit"):
        ro = {p[-2:] for p in plans if p[0] == kernel and "ro" in p}
        assert ro >= {(8, True), (4, True), (2, True), (4, False)}, (kernel, ro)                    # a remainder block for every launch-block size
    assert blocks >= {1, 2, 8}                                       # one launch, two 64-column blocks, seven + a 16-column remainder
    # whole heads: the detector at Hd = 1024, K = 9 takes the reduction-split kernel by default, the RPN at C = 256 the resident one on 8-word lines
    assert L.li_plan(1024, 9, 36) == [("ksplit", 3)] and L.li_plan(256, 3, 12) == [("mfma", 1, "resident", True)]
    assert L.li_plan(128, 9, 36, strict=True) == [("valu", 16)]
