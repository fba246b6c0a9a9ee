"""The window-table planner (ug_plan_window_tables, include/ultragroth_hip.h): host only, no device needed.

When full tables for every qualifying group fit the budget the plan is the one the provers always made (the cost-model
width, stride 1); below that each group gets strided tables or none, never more bytes than the budget, and the modelled
cost of the plan does not rise as the budget grows. The cost model is restated here from msm.hip (msm_cost) so that the
sweep can check the planner's optimisation, not only its bookkeeping."""
import math
import os

import pytest

import ultragroth_amd as ug
from ultragroth_amd import _lib

GiB = 1 << 30
G2_WEIGHT = 3.0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return ug.load()


def _windows(c):
    return (255 + c - 1) // c


def _segment_log(entries):
    log_seg = 5
    while log_seg < 7 and (entries >> (log_seg + 1)) >= (1 << 20):
        log_seg += 1
    return log_seg


def _msm_cost(n, c, tables, stride=1):
    w = _windows(c)
    entries, buckets = float(w * n), float(1 << (c - 1))
    sets = float(stride) if tables else float(w)
    over = entries / (sets * buckets) / float(1 << _segment_log(int(entries))) - 1.0
    return entries * (1.0 + (0.04 * over if over > 0 else 0.0)) + 4.0 * buckets * sets


def _classic_c(n):
    best, c = None, 0
    for k in range(6, 23):
        cost = _msm_cost(n, k, False)
        if best is None or cost < best:
            best, c = cost, k
    return c


def _plan_cost(groups, plan):
    total = 0.0
    for (n, g1, g2), (c, s, _) in zip(groups, plan):
        if not n:
            continue
        products = (g1 + G2_WEIGHT * g2) / n
        total += products * (_msm_cost(n, c, True, s) if c else _msm_cost(n, _classic_c(n), False))
    return total


def _full(lib, groups):
    out = []
    for n, g1, g2 in groups:
        if (1 << 14) <= n <= (1 << 26):
            c = lib.ug_msm_table_window(n)
            out.append((c, 1, ug.tables_bytes(g1, False, c) + ug.tables_bytes(g2, True, c)))
        else:
            out.append((0, 0, 0))
    return out


def _groth16(log):
    n = 1 << log
    return [(n, 3 * n, n), (n, n, 0)]                          # witness: A | B1 | C and B2; H


def _sparse_b(log):
    n = 1 << log
    return [(n, 2 * n, 0), (n, n, 0), (n // 2, n // 2, n // 2)]    # [A | C]; H; the compacted B1 / B2


def _ultra(log):
    n = 1 << log
    return [(n, 2 * n, n), (n // 4, n // 4, 0), (n // 8, n // 8, 0), (n, n, 0)]   # witness; round aux; final aux; H


SHAPES = [_groth16, _sparse_b, _ultra]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("log", [16, 20, 24])
def test_everything_fits_gives_todays_widths(lib, shape, log):
    groups = shape(log)
    full = _full(lib, groups)
    need = sum(b for _, _, b in full)
    for budget in (need, need + GiB, 1 << 62):
        assert ug.plan_window_tables(groups, budget) == full
    assert all(c == 0 or s == 1 for c, s, _ in full)


@pytest.mark.parametrize("shape", SHAPES)
def test_budget_zero_gives_no_tables(lib, shape):
    assert ug.plan_window_tables(shape(22), 0) == [(0, 0, 0)] * len(shape(22))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("log", [18, 22, 26])
def test_budget_sweep(lib, shape, log):
    """bytes never exceed the budget; the modelled cost does not rise with the budget; every choice is a legal table set"""
    groups = shape(log)
    need = sum(b for _, _, b in _full(lib, groups))
    prev = None
    for k in range(0, 41):
        budget = need * k // 32
        plan = ug.plan_window_tables(groups, budget)
        assert plan == ug.plan_window_tables(groups, budget)          # deterministic
        assert sum(b for _, _, b in plan) <= budget
        for (n, g1, g2), (c, s, b) in zip(groups, plan):
            if c == 0:
                assert (s, b) == (0, 0)
                continue
            w = _windows(c)
            assert 16 <= c <= 24 and 1 <= s <= w and math.ceil(w / s) >= 2
            assert n * w <= 1 << 30 and s << (c - 1) <= 1 << 24
            assert b == ug.tables_bytes(g1, False, c, s) + ug.tables_bytes(g2, True, c, s)
        cost = _plan_cost(groups, plan)
        if prev is not None:
            assert cost <= prev * (1 + 1e-12), (budget, plan)
        prev = cost
    assert ug.plan_window_tables(groups, need) == _full(lib, groups)


def test_small_groups_get_nothing(lib):
    groups = [((1 << 14) - 1, 3 << 14, 1 << 14), (1 << 10, 1 << 10, 0), (1 << 16, 1 << 16, 0), ((1 << 26) + 1, 1 << 26, 0)]
    for budget in (0, 4 * GiB, 1 << 62):
        plan = ug.plan_window_tables(groups, budget)
        assert plan[0] == plan[1] == plan[3] == (0, 0, 0)
    assert ug.plan_window_tables(groups, 1 << 62)[2][0] == lib.ug_msm_table_window(1 << 16)


@pytest.mark.parametrize("budget_gib", [140, 48])
def test_2_26_on_one_device_gets_a_plan(lib, budget_gib):
    """BASELINE configs[3] (2^26 on one GPU): full tables take far more than the budget, strided ones or H's alone fit"""
    groups = _groth16(26)
    need = sum(b for _, _, b in _full(lib, groups))
    assert need > budget_gib * GiB
    plan = ug.plan_window_tables(groups, budget_gib * GiB)
    assert any(c for c, _, _ in plan), plan
    assert sum(b for _, _, b in plan) <= budget_gib * GiB
    assert _plan_cost(groups, plan) < _plan_cost(groups, [(0, 0, 0)] * len(groups))


@pytest.mark.parametrize("c", [16, 17, 20, 22, 24])
def test_strided_bytes(lib, c):
    w = _windows(c)
    for n in (0, 1, 1000, 1 << 24):
        for g2 in (False, True):
            assert ug.tables_bytes(n, g2, c, 1) == lib.ug_bases_tables_bytes(n, 1 if g2 else 0, c)
            for s in range(1, w + 1):
                assert ug.tables_bytes(n, g2, c, s) == (math.ceil(w / s) - 1) * n * (128 if g2 else 64)
    assert ug.tables_bytes(1000, False, c, 0) == 0 and ug.tables_bytes(1000, False, c, w + 1) == 0
    assert ug.tables_bytes(1000, False, 15, 1) == 0
