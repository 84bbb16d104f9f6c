"""The block-order tuner's decision rule on made-up timing tables (hpcla_block_order_decide, csrc/spmv.hip): host code, no GPU.
ms[c][r] is candidate c in counted round r; candidate 0 is the natural order."""
import ctypes

import numpy as np


def decide(hp, table):
    ms = np.ascontiguousarray(table, dtype=np.float32)
    chosen = ctypes.c_int(-1)
    hp._capi.call("hpcla_block_order_decide", ms.ctypes.data, ms.shape[0], ms.shape[1], ctypes.byref(chosen))
    return int(chosen.value)


NATURAL = [1.400, 1.410, 1.395, 1.420, 1.405]


def scaled(f):
    return [t * f for t in NATURAL]


def test_half_a_percent_is_not_enough(hp):
    assert decide(hp, [NATURAL, scaled(1.01), scaled(0.995), scaled(1.0)]) == 0


def test_three_percent_in_every_round_wins(hp):
    assert decide(hp, [NATURAL, scaled(1.01), scaled(0.97), scaled(1.02)]) == 2
    assert decide(hp, [NATURAL, scaled(0.98), scaled(0.97), scaled(0.96)]) == 3           # the smallest median ratio


def test_faster_on_the_median_but_slower_in_one_round_gives_natural(hp):
    g = scaled(0.96)
    g[3] = NATURAL[3] * 1.002
    assert float(np.median(np.array(g) / np.array(NATURAL))) < 0.97
    assert decide(hp, [NATURAL, scaled(1.0), g, scaled(1.03)]) == 0


def test_rounds_are_compared_pair_by_pair(hp):
    """A drift between rounds larger than the gain: candidate 2 wins every round against the natural order OF THAT ROUND,
    although its slowest round is slower than the natural order's fastest."""
    nat = [1.40, 1.50, 1.60, 1.70, 1.80]
    assert decide(hp, [nat, [t * 1.01 for t in nat], [t * 0.97 for t in nat], [t * 1.0 for t in nat]]) == 2


def test_a_tie_between_two_grouped_orders_gives_the_first(hp):
    assert decide(hp, [NATURAL, scaled(0.97), scaled(0.97), scaled(1.0)]) == 1
    assert decide(hp, [NATURAL, scaled(1.0), scaled(0.97), scaled(0.97)]) == 2


def test_one_candidate_and_one_round(hp):
    assert decide(hp, [[1.0]]) == 0
    assert decide(hp, [[1.0], [0.5]]) == 1
    assert decide(hp, [[1.0, 1.0], [0.98, 0.99]]) == 1                                   # even count: mean of the middle pair, 0.985


def test_null_or_zero_sized_input_is_an_error(hp):
    lib = hp._capi.load()
    ms = np.ones((4, 5), dtype=np.float32)
    chosen = ctypes.c_int(7)
    assert lib.hpcla_block_order_decide(None, 4, 5, ctypes.byref(chosen)) != 0
    assert lib.hpcla_block_order_decide(ms.ctypes.data, 4, 5, None) != 0
    assert lib.hpcla_block_order_decide(ms.ctypes.data, 0, 5, ctypes.byref(chosen)) != 0
    assert lib.hpcla_block_order_decide(ms.ctypes.data, 4, 0, ctypes.byref(chosen)) != 0
    assert lib.hpcla_block_order_decide(ms.ctypes.data, 1, 65, ctypes.byref(chosen)) != 0
    bad = ms.copy()
    bad[2, 3] = 0.0
    assert lib.hpcla_block_order_decide(bad.ctypes.data, 4, 5, ctypes.byref(chosen)) != 0
    bad[2, 3] = np.nan
    assert lib.hpcla_block_order_decide(bad.ctypes.data, 4, 5, ctypes.byref(chosen)) != 0
    assert chosen.value == 7, "an error leaves the output alone"
    assert "block_order_decide" in hp._capi.last_error()
