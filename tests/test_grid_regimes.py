"""CPU test: the sizes at which the GPU tests run each kernel family on its own reach every regime of that family's launch grid
(tests/_grid_regimes.py states the regimes and reads the grids' constants from csrc/).  Removing a size that alone covers a
regime, or changing a grid constant so that a size no longer lands where it did, fails here."""
import pytest

from tests import _grid_regimes as gr


def test_constants_and_grid_functions_at_the_documented_sizes():
    """The figures the docstrings of the GPU tests quote.  A changed constant in csrc/ fails here first."""
    assert (gr.RT, gr.MAX_PARTIALS, gr.REDUCE_WIDTH, gr.REDUCE_PER_LANE) == (256, 2048, 2, 4)
    assert (gr.EW_T, gr.EW_CAP) == (256, 4096)
    assert (gr.F_RT, gr.F_MAX_PARTIALS, gr.F_WIDTH, gr.F_PER_LANE) == (256, 1024, 4, 4)
    assert (gr.SCAN_T, gr.SCAN_E, gr.SCAN_B) == (256, 4, 1024)
    assert (gr.DIGEST_T, gr.DIGEST_CAP, gr.PARTIALS_ONE_STAGE_TRIPS) == (256, 4096, 4)
    want = {2049: (1, "R1", 4, "E2"), 2051: (2, "R2", 5, "E2"), gr.R3_N: (301, "R3", 1201, "E2"),
            gr.R4_N: (2048, "R4", 4096, "E3")}
    for n, row in want.items():
        assert (gr.reduce_grid(n), gr.reduction_regime(n), gr.ew_grid(n // 2), gr.elementwise_regime(n)) == row, n
        assert gr.has_tail(n)
    assert [gr.reduce_grid(n) for n in (0, 1, 2048, 2050, 4_000_001, 1 << 40)] == [1, 1, 1, 2, 1954, 2048]
    assert gr.reduction_regime(2 * 1024 * 512) is None                    # 512 partials: no ragged trip, no regime of its own
    assert [gr.reduce_grid(2 * 1024 * 2047 + k) for k in (1, 2)] == [2047, 2048]     # the first size at the cap
    assert [gr.f32_reduce_grid(n) for n in (1_000_003, 1_228_807, gr.R4_N)] == [245, 301, 1024]
    assert [gr.ew_grid(i) for i in (0, 256, 257, 1 << 30)] == [1, 1, 2, 4096]


@pytest.mark.parametrize("family", sorted(gr.REDUCTION_FAMILIES))
def test_every_reduction_family_reaches_every_regime_with_a_tail(family):
    sizes = gr.REDUCTION_FAMILIES[family]
    seen = {}
    for n in sizes:
        seen.setdefault(gr.reduction_regime(n), []).append(n)
    for regime in gr.REDUCTION_REGIMES:
        assert regime in seen, f"{family}: no size in {regime} among {sizes}"
        assert any(gr.has_tail(n) for n in seen[regime]), f"{family}: no odd size (scalar tail) in {regime}: {seen[regime]}"


@pytest.mark.parametrize("family", sorted(gr.ELEMENTWISE_FAMILIES))
def test_every_elementwise_family_reaches_every_regime(family):
    sizes = gr.ELEMENTWISE_FAMILIES[family]
    regime = gr.elementwise_regime_of(family)
    seen = {regime(n) for n in sizes}
    assert set(gr.ELEMENTWISE_REGIMES) <= seen, (family, sorted(set(gr.ELEMENTWISE_REGIMES) - seen))
    assert any(regime(n) == "E3" and n & 1 for n in sizes), f"{family}: no odd size (scalar tail) on the capped grid"


def test_the_smoother_kernels_grid_at_the_documented_sizes():
    """amg_smooth_kernel's own grid, read from csrc/amg.hip: the figures tests/test_gpu_precond_kernels.py quotes."""
    assert (gr.AMG_SMOOTH_WIDTH, gr.AMG_SMOOTH_T, gr.AMG_SMOOTH_CAP) == (2, 256, 4096)
    assert [gr.amg_smooth_grid(n) for n in gr.AMG_SMOOTH_ALONE] == [1, 1, 1, 1, 5, 1201, 4096]
    assert [gr.amg_smooth_regime(n) for n in gr.AMG_SMOOTH_ALONE] == ["E1"] * 4 + ["E2"] * 2 + ["E3"]
    assert gr.elementwise_regime_of("amg_smooth") is gr.amg_smooth_regime and gr.elementwise_regime_of("pcg") is gr.elementwise_regime
    n2 = gr.R4_N // 2                                                       # 2 097 153 double2: two full trips and lane 0's third
    assert n2 == 2 * gr.AMG_SMOOTH_CAP * gr.AMG_SMOOTH_T + 1 and gr.R4_N & 1
    assert gr.amg_smooth_regime(2 * gr.AMG_SMOOTH_CAP * gr.AMG_SMOOTH_T) is None      # the cap reached, no further trip


def test_float32_reductions_reach_every_regime_with_a_tail():
    seen = {}
    for n in gr.F32_ALONE:
        seen.setdefault(gr.f32_reduction_regime(n), []).append(n)
    for regime in gr.REDUCTION_REGIMES:
        assert regime in seen and any(gr.has_tail(n, gr.F_WIDTH) for n in seen[regime]), (regime, seen.get(regime))


def test_nan_positions_at_the_capped_grid():
    """The NaNs of the largest case sit in the last workgroup's last trip, in the extra trip of lane 0 and at the scalar tail."""
    n = gr.R4_N
    stride = gr.reduce_grid(n) * gr.RT                                      # double2 per stage-1 trip
    n2 = n // 2
    last_full = (n2 // stride) * stride - 1                                 # the last lane of the last workgroup, last trip
    at = {where for size, where in gr.PLAIN_F64_NAN if size == n}
    assert 2 * last_full + 1 in at and 2 * (n2 - 1) + 1 in at and n - 1 in at
    assert last_full // gr.RT % gr.reduce_grid(n) == gr.reduce_grid(n) - 1 and (n2 - 1) % stride == 0 and n & 1
    assert all(0 <= where < size for size, where in gr.PLAIN_F64_NAN)


def test_scan_windows_partial_counts_and_digest_sizes():
    assert [(gr.scan_blocks(w), gr.scan_trips(w)) for w, _ in gr.SCAN_WINDOWS] == [(256, 1), (257, 2), (601, 3)]
    assert any(lo > 0 for _, lo in gr.SCAN_WINDOWS) and gr.SCAN_CARRY_AT == 262_144
    assert gr.scan_blocks(601 * 1024) % gr.SCAN_T != 0                      # the third trip is ragged
    assert [gr.partials_two_stage(b) for b in gr.PARTIAL_BLOCKS] == [False, True, True]
    assert gr.PARTIAL_BLOCKS[0] == gr.PARTIALS_ONE_STAGE_TRIPS * gr.RT and gr.PARTIAL_BLOCKS[1] == gr.PARTIAL_BLOCKS[0] + 1
    assert [gr.reduce_grid(b) for b in gr.PARTIAL_BLOCKS[1:]] == [1, 2] and all(b & 1 for b in gr.PARTIAL_BLOCKS[1:2])
    assert [(gr.digest_grid(n), gr.digest_trips(n)) for n in gr.DIGEST_SIZES] == [(1, 1), (1, 1), (2, 1), (4096, 1), (4096, 2),
                                                                                  (4096, 3)]
    assert gr.DIGEST_SIZES[4] - 1 == gr.DIGEST_CAP * gr.DIGEST_T            # element 1 048 576 opens the second trip


def test_ilu_kernels_sizes_land_on_both_sides_of_a_workgroup():
    from tests import _ilu_cases as ic
    assert gr.ILU_THREADS == 256
    assert [gr.ilu_grid(n) for n in ic.NNZ_EDGES] == [1, 1, 1, 2] and [gr.ilu_grid(n) for n in ic.PIVOT_SIZES] == [1, 1, 2, 3]
    assert [gr.ilu_grid(n) for n in ic.ROW_EDGES] == [1, 1, 1, 1, 2, 4, 4, 5, 9, 1025]
    items = sorted({n * lanes for n in ic.RAGGED_SIZES for lanes in ic.LANES})
    for lanes in ic.LANES[1:]:                                      # a row count whose lanes end on, before and behind a workgroup
        mod = {(n * lanes) % gr.ILU_THREADS for n in ic.RAGGED_SIZES if n * lanes >= gr.ILU_THREADS - lanes}
        assert {0, lanes, gr.ILU_THREADS - lanes} <= mod, (lanes, sorted(mod))
    assert {255, 256, 257} <= set(items) and max(gr.ilu_grid(v) for v in items) == 32
