"""CPU side of the fine-grained ILU(0) preconditioner: the public names, the C ABI tables, the argument rules that need no
device, and the numpy restatements of tests/_ilu_cases.py against each other and on the shared cases.  Every margin the GPU
tests rest on is re-measured here, printed, and held to the relation tests/_ilu_cases.py states for it."""
import os
import re

import numpy as np
import pytest

from tests import _bicgstab_cases as bc
from tests import _gmres_cases as gc
from tests import _ilu_cases as ic
from tests import _pcg_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["hpcla_ilu_work_bytes", "hpcla_ilu_count_f64_i32", "hpcla_ilu_count_f64_i64", "hpcla_ilu_fill_f64_i32",
               "hpcla_ilu_fill_f64_i64", "hpcla_ilu_gather_f64", "hpcla_ilu_init_f64", "hpcla_ilu_sweep_f64",
               "hpcla_ilu_pivots_f64", "hpcla_ilu_trisweep_f64", "hpcla_ilu_apply_f64"]


@pytest.fixture(scope="module")
def cases(orc):
    """Every factor case as its one-rank block, with the 3-sweep factors in both sum orders, computed once."""
    out = {}
    for name, (rowptr, colidx, vals, b) in ic.factor_cases(orc).items():
        bp, bcols, bv = ic.block_csr(rowptr, colidx, vals)
        out[name] = dict(rowptr=rowptr, colidx=colidx, vals=vals, b=b, bp=bp, bc=bcols, bv=bv,
                         f=ic.sweep_factors(bp, bcols, bv, 3), fd=ic.sweep_factors(bp, bcols, bv, 3, descending=True))
    return out


@pytest.fixture(scope="module")
def systems(orc):
    """The convection-diffusion case at the three sizes and LARGE_SIZE with Jacobi's GMRES(30) count, computed once."""
    out = {}
    for nx, ny in list(pc.SIZES) + [pc.LARGE_SIZE]:
        rowptr, colidx, vals, b = bc.convection_diffusion(orc, nx, ny)
        d = pc.host_diag(rowptr, colidx, vals)
        _, its, status, _ = gc.gmres(rowptr, colidx, vals, b, dinv=1.0 / d, rtol=1e-8)
        assert status == "converged"
        out[(nx, ny)] = dict(rowptr=rowptr, colidx=colidx, vals=vals, b=b, jacobi=its)
    return out


def test_public_names_exist(hp):
    assert callable(hp.ilu0) and hp.ILU0
    assert hp.ilu0.__module__.endswith("ilu")
    assert "ILU0" in hp.gmres.__doc__ and "ILU0" in hp.bicgstab.__doc__
    assert "ILU0" not in hp.cg.__doc__


def test_header_declares_the_new_entries_and_ctypes_binds_them(hp):
    with open(os.path.join(ROOT, "include", "hpcla_rocm.h"), encoding="utf-8") as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name in hp._capi.EXPORTED_SYMBOLS, name
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, f"{name} is not declared in include/hpcla_rocm.h"
        assert m.group(1).count(",") + 1 == len(hp._capi._SIGNATURES[name]), name
    lib = hp._capi.load()
    assert lib.hpcla_ilu_work_bytes(-1) == -1
    assert lib.hpcla_ilu_work_bytes(0) == 16 and lib.hpcla_ilu_work_bytes(1024) == 16 and lib.hpcla_ilu_work_bytes(1025) == 24


def test_c_entries_refuse_bad_arguments_without_a_gpu(hp):
    lib = hp._capi.load()
    INVALID = lib.hpcla_dot_f64(None, None, None, -1, None, None, None)
    assert INVALID != 0
    one = 8                                                              # any non-null address: refused before it is looked at
    assert lib.hpcla_ilu_count_f64_i32(None, None, -1, -1, 0, one, one, one, None) == INVALID                    # negative size
    assert lib.hpcla_ilu_count_f64_i64(None, None, 4, 5, 0, one, one, one, None) == INVALID                      # n_own != nrows
    assert lib.hpcla_ilu_count_f64_i32(None, None, 4, 4, 2, one, one, one, None) == INVALID                      # index_base
    assert lib.hpcla_ilu_count_f64_i32(None, None, 4, 4, 0, None, one, one, None) == INVALID                     # null rowptr out
    assert lib.hpcla_ilu_count_f64_i32(None, None, 4, 4, 0, one, one, one, None) == INVALID                      # null CSR
    assert lib.hpcla_ilu_fill_f64_i32(None, None, None, 4, 4, 0, one, one, one, one, one, one, None) == INVALID   # null CSR
    assert lib.hpcla_ilu_fill_f64_i64(one, one, one, 4, 3, 0, one, one, one, one, one, one, None) == INVALID
    assert lib.hpcla_ilu_gather_f64(None, one, 4, one, None) == INVALID
    assert lib.hpcla_ilu_init_f64(one, one, one, one, -1, one, None) == INVALID
    assert lib.hpcla_ilu_sweep_f64(one, one, one, one, one, one, one, 16, 16, 4, None) == INVALID                 # one buffer
    assert lib.hpcla_ilu_sweep_f64(one, one, one, one, one, one, one, 16, 24, 2 ** 31 + 1, None) == INVALID       # too many entries
    assert lib.hpcla_ilu_pivots_f64(one, one, 4, one, None, None) == INVALID                                      # null info
    assert lib.hpcla_ilu_trisweep_f64(one, one, one, one, one, one, None, 16, 4, 0, 3, None) == INVALID           # lanes
    assert lib.hpcla_ilu_trisweep_f64(one, one, one, one, one, 16, None, 16, 4, 0, 1, None) == INVALID            # in is out
    for sweeps in (0, 17):
        assert lib.hpcla_ilu_apply_f64(one, one, one, one, one, 16, 32, 48, 64, 4, sweeps, 1, None) == INVALID
    assert lib.hpcla_ilu_apply_f64(one, one, one, one, one, 16, 32, 32, 64, 4, 3, 1, None) == INVALID             # t0 is t1
    assert lib.hpcla_ilu_apply_f64(one, one, one, one, one, 16, 32, 48, 64, 4, 3, 5, None) == INVALID             # lanes
    # nothing to do: no launch, no error
    assert lib.hpcla_ilu_apply_f64(None, None, None, None, None, None, None, None, None, 0, 3, 1, None) == 0
    assert lib.hpcla_ilu_sweep_f64(None, None, None, None, None, None, None, None, None, 0, None) == 0


def test_argument_rules(hp):
    from hpcla_amd.ilu import check_arguments, error_message
    part = np.array([0, 5, 10])
    check_arguments(np.float64, (10, 10), part, part)
    check_arguments(np.float64, (10, 10), part, part, 64, 16)
    with pytest.raises(TypeError, match="Float64"):
        check_arguments(np.float32, (10, 10), part, part)
    with pytest.raises(ValueError, match="square"):
        check_arguments(np.float64, (10, 12), part, part)
    with pytest.raises(ValueError, match="partitioned alike"):
        check_arguments(np.float64, (10, 10), part, np.array([0, 4, 10]))
    for sweeps in (0, 65, -1):
        with pytest.raises(ValueError, match=r"^ilu0: sweeps must be in 1\.\.64"):
            check_arguments(np.float64, (10, 10), part, part, sweeps, 3)
    for solve_sweeps in (0, 17):
        with pytest.raises(ValueError, match=r"^ilu0: solve_sweeps must be in 1\.\.16"):
            check_arguments(np.float64, (10, 10), part, part, 3, solve_sweeps)
    assert error_message(1, 7, 3) == "ilu0: row 7 stores no diagonal"
    assert error_message(2, 7, 3) == "ilu0: the diagonal of row 7 is zero or NaN"
    assert error_message(3, 7, 3) == "ilu0: the pivot of row 7 is zero or not finite after 3 sweeps"


# ---- the restatements against each other ------------------------------------------------------------------------------------------
def test_cases_are_what_the_docstring_says(cases):
    for w in ic.BANDED_W:
        rowptr, colidx, vals = ic.banded(w)
        counts = np.diff(rowptr) - 1
        assert counts.min() == w and counts.max() == 2 * w
        dense = bc.dense_of(rowptr, colidx, vals)
        assert not np.allclose(dense, dense.T)
        off = np.abs(dense).sum(axis=1) - np.abs(np.diag(dense))
        assert np.all(np.diag(dense) > off)
    assert max(2 * w for w in ic.BANDED_W) >= 31 and min(ic.BANDED_W) == 1
    rowptr, colidx, vals = ic.asymmetric_pattern()
    dense = bc.dense_of(rowptr, colidx, vals)
    stored = dense != 0
    assert (stored & ~stored.T).sum() == stored.sum() - ic.ASYM_N          # no off-diagonal entry has its mirror
    assert np.all(np.diag(dense) > np.abs(dense).sum(axis=1) - np.abs(np.diag(dense)))
    lower_empty = [i for i in range(ic.ASYM_N) if not stored[i, :i].any()]
    upper_empty = [i for i in range(ic.ASYM_N) if not stored[i, i + 1:].any()]
    assert len(lower_empty) >= 3 and len(upper_empty) >= 3 and set(lower_empty) & set(upper_empty)


def test_forty_sweeps_reach_the_exact_factors(cases):
    worst = 0.0
    for name, c in cases.items():
        exact = ic.exact_ilu0(c["bp"], c["bc"], c["bv"])
        f40 = ic.sweep_factors(c["bp"], c["bc"], c["bv"], ic.EXACT_SWEEPS)
        dev = float(np.max(np.abs(f40 - exact) / np.abs(exact)))
        three = float(np.max(np.abs(c["f"] - exact) / np.abs(exact)))
        print(f"{name}: {ic.EXACT_SWEEPS} sweeps deviate by {dev:.2e} from the exact ILU(0), 3 sweeps by {three:.2e}")
        worst = max(worst, dev)
        # L U agrees with A on the pattern: the defining property of ILU(0), checked on the exact factors
        L, U, d = ic.split_factors(c["bp"], c["bc"], exact)
        n = len(c["bp"]) - 1
        Ld = bc.dense_of(*L) + np.eye(n) if n > 1 else np.eye(n)
        Ud = (bc.dense_of(*U) if n > 1 else np.zeros((n, n))) + np.diag(d)
        A = bc.dense_of(c["bp"], c["bc"], c["bv"])
        assert np.allclose((Ld @ Ud)[A != 0], A[A != 0], rtol=1e-12, atol=0), name
    print(f"largest deviation {worst:.2e}; EXACT_RTOL = {ic.EXACT_RTOL:.1e}")
    assert 0 < worst and 100 * worst <= ic.EXACT_RTOL <= 110 * worst


def test_the_two_sum_orders_give_the_margin(cases):
    worst = 0.0
    for name, c in cases.items():
        spread = float(np.max(np.abs(c["f"] - c["fd"]) / np.abs(c["f"])))
        print(f"{name}: ascending against descending sums at 3 sweeps: {spread:.2e}")
        worst = max(worst, spread)
    print(f"largest spread {worst:.2e}; ILU_RTOL = {ic.ILU_RTOL:.1e}")
    assert 0 < worst and 10 * worst <= ic.ILU_RTOL <= 11 * worst


def test_apply_is_the_truncated_series(cases):
    """``apply`` against the dense series sum_k (-L)^k and sum_k (-D^-1 U)^k D^-1; with enough terms it is the exact solve."""
    for name in ("convdiff16x16", "banded8", "asymmetric", "diagonal", "one"):
        c = cases[name]
        n = len(c["bp"]) - 1
        L, U, d = ic.split_factors(c["bp"], c["bc"], c["f"])
        Ld = bc.dense_of(*L) if len(L[1]) else np.zeros((n, n))
        Ud = bc.dense_of(*U) if len(U[1]) else np.zeros((n, n))
        r = c["b"]
        for s in (1, 2, 3, 16):
            NL = sum(np.linalg.matrix_power(-Ld, k) for k in range(s + 1))
            G = -Ud / d[:, None]
            NU = sum(np.linalg.matrix_power(G, k) for k in range(s + 1)) / d[None, :]
            want = NU @ (NL @ r)
            got = ic.apply(c["bp"], c["bc"], c["f"], r, s)
            assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max()), (name, s)
    c = cases["diagonal"]
    assert np.array_equal(ic.apply(c["bp"], c["bc"], c["f"], c["b"], 3), c["b"] / c["vals"])
    c = cases["one"]
    assert ic.apply(c["bp"], c["bc"], c["f"], c["b"], 3)[0] == 3.0 / 2.5


def test_blocks_ignore_what_other_ranks_own(cases):
    c = cases["convdiff24x20"]
    n = len(c["b"])
    part = ic.equal_blocks(n, 3)
    blocks = ic.ilu_blocks(c["rowptr"], c["colidx"], c["vals"], part)
    assert [b[3] for b in blocks] == part[:-1]
    for bp, bcols, f, lo in blocks:
        nloc = len(bp) - 1
        assert bcols.min() >= 0 and bcols.max() < nloc
        assert all(np.all(np.diff(bcols[bp[i]:bp[i + 1]]) > 0) for i in range(nloc))
    assert sum(len(b[1]) for b in blocks) < len(c["colidx"])            # the couplings across the cuts are gone
    one = ic.ilu_blocks(c["rowptr"], c["colidx"], c["vals"], [0, n])
    assert np.array_equal(pc.bits(one[0][2]), pc.bits(c["f"]))


def test_faults_are_named_in_row_order():
    for heal, (kind, row) in enumerate(zip((ic.BadDiagonal, ic.NoDiagonal, ic.BadDiagonal), ic.FAULT_ROWS)):
        bp, bcols, bv = ic.block_csr(*ic.three_faults(heal))
        with pytest.raises(kind) as e:
            ic.sweep_factors(bp, bcols, bv, 3)
        assert e.value.row == row
    bp, bcols, bv = ic.block_csr(*ic.three_faults(3))
    assert np.all(np.isfinite(ic.sweep_factors(bp, bcols, bv, 3)))
    # rank-local: the global row
    rowptr, colidx, vals = ic.three_faults(0)
    a, b = int(rowptr[30]), int(rowptr[90])
    with pytest.raises(ic.BadDiagonal) as e:
        ic.sweep_factors(*ic.block_csr(rowptr[30:91] - a, colidx[a:b], vals[a:b], 30), 3, row_start=30)
    assert e.value.row == 40


# ---- the solvers --------------------------------------------------------------------------------------------------------------------
def test_with_a_diagonal_K_the_solvers_are_the_existing_restatements(systems):
    s = systems[(16, 16)]
    dinv = 1.0 / pc.host_diag(s["rowptr"], s["colidx"], s["vals"])
    K = lambda u: dinv * u
    for restart in (30, 8):
        got = ic.gmres_op(s["rowptr"], s["colidx"], s["vals"], s["b"], K, restart=restart)
        want = gc.gmres(s["rowptr"], s["colidx"], s["vals"], s["b"], dinv=dinv, restart=restart)
        assert got[1:3] == want[1:3] and got[3] == want[3] and np.array_equal(pc.bits(got[0]), pc.bits(want[0]))
    got = ic.bicgstab_op(s["rowptr"], s["colidx"], s["vals"], s["b"], K)
    want = bc.bicgstab(s["rowptr"], s["colidx"], s["vals"], s["b"], dinv=dinv)
    assert got[1:3] == want[1:3] and got[3] == want[3] and np.array_equal(pc.bits(got[0]), pc.bits(want[0]))


@pytest.mark.parametrize("size", list(pc.SIZES) + [pc.LARGE_SIZE])
def test_gmres_takes_at_most_half_of_jacobis_iterations(systems, size):
    """The issue's condition, with defaults (3 factor sweeps, 3 + 3 solve sweeps, GMRES(30), rtol = 1e-8), for 1, 2, 3 and 8 equal
    row blocks."""
    s = systems[size]
    n = len(s["b"])
    for k in ic.BLOCKS:
        K = ic.operator(ic.ilu_blocks(s["rowptr"], s["colidx"], s["vals"], ic.equal_blocks(n, k)))
        x, its, status, hist = ic.gmres_op(s["rowptr"], s["colidx"], s["vals"], s["b"], K, rtol=1e-8)
        true = np.linalg.norm(s["b"] - pc.matvec(s["rowptr"], s["colidx"], s["vals"], x)) / np.linalg.norm(s["b"])
        xb, itb, statusb, _ = ic.bicgstab_op(s["rowptr"], s["colidx"], s["vals"], s["b"], K, rtol=1e-8)
        trueb = np.linalg.norm(s["b"] - pc.matvec(s["rowptr"], s["colidx"], s["vals"], xb)) / np.linalg.norm(s["b"])
        print(f"{size} in {k} blocks: gmres {its} against Jacobi's {s['jacobi']} ({its / s['jacobi']:.3f}), true residual "
              f"{true:.2e}; bicgstab {itb}, true residual {trueb:.2e}")
        assert status == statusb == "converged"
        assert its <= ic.JACOBI_FACTOR * s["jacobi"], (size, k, its, s["jacobi"])
        assert true <= pc.TRUE_RES_RTOL and trueb <= pc.TRUE_RES_RTOL
        assert all(b_ <= a_ * (1 + gc.RISE_RTOL) for a_, b_ in zip(hist, hist[1:]))


@pytest.mark.parametrize("size", list(pc.SIZES) + [pc.LARGE_SIZE])
def test_history_heads_spread_less_than_a_tenth_of_the_margin(systems, size):
    s = systems[size]
    K = ic.operator(ic.ilu_blocks(s["rowptr"], s["colidx"], s["vals"], [0, len(s["b"])]))
    hg, hb, counts = [], [], []
    for dot in bc.DOTS.values():
        _, it, _, h = ic.gmres_op(s["rowptr"], s["colidx"], s["vals"], s["b"], K, rtol=1e-8, restart=ic.HEAD_RESTART, maxiter=60, dot=dot)
        hg.append(h[:ic.HEAD_GMRES])
        _, itb, _, h = ic.bicgstab_op(s["rowptr"], s["colidx"], s["vals"], s["b"], K, rtol=1e-8, dot=dot)
        hb.append(h[:ic.HEAD_BICGSTAB])
        counts.append(itb)
    hg, hb = np.array(hg), np.array(hb)
    assert hg.shape[1] == ic.HEAD_GMRES and hb.shape[1] == ic.HEAD_BICGSTAB
    sg = float(np.max(np.abs(hg - hg[0]) / hg[0]))
    sb = float(np.max(np.abs(hb - hb[0]) / hb[0]))
    print(f"{size}: head spread over four summation orders: gmres {sg:.2e} ({ic.HEAD_GMRES} entries, restart {ic.HEAD_RESTART}), "
          f"bicgstab {sb:.2e} ({ic.HEAD_BICGSTAB} entries); bicgstab counts {counts}")
    assert sg < ic.HIST_RTOL / 10 and sb < ic.HIST_RTOL / 10
    assert max(counts) - min(counts) <= 2


# ---- the restatements of the single kernels (tests/test_gpu_ilu_kernels.py) -------------------------------------------------------
@pytest.fixture(scope="module")
def kernel_cases(orc):
    return ic.kernel_cases(orc)


def test_work_bytes_at_the_scan_block_edges(hp):
    from tests import _grid_regimes as gr
    lib = hp._capi.load()
    for n in (0, 1, 1024, 1025):
        assert lib.hpcla_ilu_work_bytes(n) == 8 * (1 + gr.scan_blocks(max(n, 1))), n
    assert ic.ROW_EDGES[-1] == gr.SCAN_T * gr.SCAN_B + 1 == gr.SCAN_CARRY_AT + 1
    assert [gr.scan_blocks(n) for n in ic.ROW_EDGES] == [1, 1, 1, 1, 1, 1, 1, 2, 3, 257]
    assert [gr.scan_trips(n) for n in ic.ROW_EDGES] == [1] * 9 + [2]
    assert gr.ILU_THREADS == 256
    large = pc.LARGE_SIZE[0] * pc.LARGE_SIZE[1]
    assert large == 4095 and gr.scan_blocks(large) == 4 and large == 4 * gr.SCAN_B - 1


def test_block_of_split_agrees_with_block_csr_on_every_block(kernel_cases):
    from tests import _amg_cases as ac
    chains = with_ghosts = 0
    for name, matrix in kernel_cases.items():
        rowptr, colidx, vals = matrix
        A = ic.to_scipy(*matrix)
        for k, j, part in ic.block_inputs(name, matrix):
            lo, hi = part[j], part[j + 1]
            a, b = int(rowptr[lo]), int(rowptr[hi])
            bp, bcols, bv = ic.block_csr(rowptr[lo:hi + 1] - a, colidx[a:b], vals[a:b], lo)
            first = None
            for base, Ti in ((0, np.int32), (1, np.int64)):
                r, split, v, n_own, ghosts = ac.split_block(A, part, j, base, Ti)
                got = ic.block_of_split(r, split, v, n_own, base)
                assert np.array_equal(got[0], bp) and np.array_equal(got[1], bcols), (name, k, j)
                assert np.array_equal(pc.bits(got[5]), pc.bits(bv)) and got[6] == ic.NO_FAILURE, (name, k, j)
                assert np.array_equal(got[2], np.repeat(np.arange(hi - lo), np.diff(bp)))
                assert np.array_equal(got[1][got[3]], np.arange(hi - lo)) and np.array_equal(v[got[4]], bv)
                first = first or got
                assert all(np.array_equal(x, y) for x, y in zip(got[:6], first[:6]))
            chains += 1
            with_ghosts += int(len(ghosts) > 0)
            if k > 1 and hi - lo > 1 and name != "diagonal":
                assert len(ghosts) > 0, (name, k, j)
    print(f"{chains} (case, blocks, block) inputs, {with_ghosts} of them with ghost columns")
    assert chains >= 150 and with_ghosts >= 100


def test_the_non_raising_chain_is_sweep_factors_on_healthy_input(kernel_cases):
    """init_values / sweep_once (the literal merge) against sweep_factors (the products by set intersection), bit for bit."""
    longest = 0
    for name in ("convdiff24x20", "banded3", "banded16", "asymmetric", "diagonal", "one", "arrow", "comb"):
        matrix = kernel_cases[name]
        n = len(matrix[0]) - 1
        for part, j in (([0, n], 0), (ic.equal_blocks(n, 3), 1)):
            if name in ("arrow", "comb", "one") and len(part) > 2:
                continue
            ref = ic.block_reference(matrix, part, j)
            for sweeps in (0, 1, 3):
                want = ic.sweep_factors(ref["bp"], ref["bc"], ref["a_vals"], sweeps, part[j])
                assert np.array_equal(pc.bits(ref["f"][sweeps]), pc.bits(want)), (name, len(part) - 1, sweeps)
            longest = max(longest, int(ref["products"][3][:, 0].max()))
    print(f"longest merged sum {longest} products")
    assert longest == ic.ARROW_N - 1


def test_arrow_and_comb_walk_the_merge_as_stated(kernel_cases):
    ref = ic.block_reference(kernel_cases["arrow"], [0, ic.ARROW_N], 0)
    n = ic.ARROW_N
    assert np.diff(ref["bp"]).max() == n and np.diff(ref["c_ptr"]).max() == n
    corner = int(ref["bp"][n]) - 1
    assert (ref["brows"][corner], ref["bc"][corner]) == (n - 1, n - 1) and ref["products"][3][corner].tolist() == [n - 1, 0, 0, 1]
    A = bc.dense_of(*kernel_cases["arrow"])
    assert not np.allclose(A, A.T) and np.all(np.diag(A) > np.abs(A).sum(axis=1) - np.diag(A))
    # the corner's sum depends on its order: the descending sum differs in bits
    up = ic.sweep_factors(ref["bp"], ref["bc"], ref["a_vals"], 1)[corner]
    down = ic.sweep_factors(ref["bp"], ref["bc"], ref["a_vals"], 1, descending=True)[corner]
    assert up != down
    ref = ic.block_reference(kernel_cases["comb"], [0, ic.COMB_N], 0)
    stats = ref["products"][3]
    every = np.flatnonzero((stats[:, 0] >= 5) & (stats[:, 1] >= 5) & (stats[:, 2] >= 5))
    print(f"comb: {len(stats)} entries, {len(every)} take every branch 5 times or more, {int(stats[:, 3].sum())} end at the break")
    assert 90 <= len(ref["bp"]) - 1 <= 100 and len(every) >= 1 and np.any(stats[every, 3] == 1)
    A = bc.dense_of(*kernel_cases["comb"])
    assert np.all(np.diag(A) > np.abs(A).sum(axis=1) - np.diag(A))
    # a walk that advanced the wrong pointer in a skip branch, or went on to k = m, would meet other products
    i, j = int(ref["brows"][every[0]]), int(ref["bc"][every[0]])
    ks = [k for k in range(min(i, j)) if A[i, k] != 0 and A[k, j] != 0]
    assert stats[every[0], 0] == len(ks) and A[i, min(i, j)] != 0


def test_counted_cases_have_the_counts_they_are_for(kernel_cases):
    for nnz in ic.NNZ_EDGES:
        rowptr, cols, vals = ic.nnz_edge(nnz)
        assert rowptr[-1] == len(cols) == len(vals) == nnz
        got = ic.block_of_split(rowptr, cols, vals, len(rowptr) - 1)
        assert got[6] == ic.NO_FAILURE and len(got[1]) == nnz
    # the duplicated columns: ties in stored order, the last stored diagonal
    rowptr, split, vals, n_own = ic.duplicated_block()
    bp, bcols, brows, bdiag, bmap, a_vals, word = ic.block_of_split(rowptr, split, vals, n_own)
    assert bp.tolist() == [0, 3, 7, 10, 11] and bcols.tolist() == [0, 0, 1, 0, 1, 1, 3, 2, 3, 3, 3]
    assert bmap.tolist() == [1, 2, 0, 6, 4, 7, 8, 11, 9, 10, 14] and bdiag.tolist() == [1, 5, 7, 10]
    assert a_vals.tolist() == [4.0, 5.0, -1.0, -2.0, 6.0, 0.0, 1.5, 7.0, -1.0, -2.0, 8.0] and word == (1 << 2) | ic.BAD_DIAG
    # generated rows: ghosts, unsorted rows, no duplicate, every diagonal
    for n in ic.ROW_EDGES[:-1]:
        rowptr, colval, vals = ic.generated_rows(n)
        assert len(rowptr) == n + 1 and np.all(np.diff(rowptr) >= 1) and np.all(np.diff(rowptr) <= 3)
        got = ic.block_of_split(rowptr, colval, vals, n)
        assert np.all(got[3] >= 0) and got[6] == ic.NO_FAILURE
        if n >= 255:
            assert np.any(colval >= n) and np.any(np.diff(colval)[np.diff(np.repeat(np.arange(n), np.diff(rowptr))) == 0] < 0)
            assert all(len(set(colval[rowptr[i]:rowptr[i + 1]])) == rowptr[i + 1] - rowptr[i] for i in range(0, n, 7))
            assert 0 < len(got[1]) < len(colval)
    # the word of the fill on the three faults
    for heal, want in enumerate([(40 << 2) | ic.BAD_DIAG, (300 << 2) | ic.NO_DIAG, (520 << 2) | ic.BAD_DIAG, ic.NO_FAILURE]):
        rowptr, cols, vals = ic.three_faults(heal)
        got = ic.block_of_split(rowptr, cols, vals, 600)
        assert got[6] == want and (got[3][300] == -1) == (heal < 2)
    # the shuffled rows leave the block where it was
    from tests import _amg_cases as ac
    for name in ic.SHUFFLED_ON:
        matrix = kernel_cases[name]
        part = ic.equal_blocks(len(matrix[0]) - 1, 3)
        between = 0
        for j in range(3):
            rowptr, split, vals, n_own, _ = ac.split_block(ic.to_scipy(*matrix), part, j)
            cols2, vals2, perm = ic.shuffled_rows(rowptr, split, vals, np.random.default_rng(5 + j))
            a, b = ic.block_of_split(rowptr, split, vals, n_own), ic.block_of_split(rowptr, cols2, vals2, n_own)
            assert not np.array_equal(cols2, split)
            assert all(np.array_equal(a[t], b[t]) for t in (0, 1, 2, 3, 5)) and np.array_equal(perm[b[4]], a[4])
            own = np.flatnonzero(cols2 < n_own)                 # a ghost stands between two owned entries of some row
            row_of = np.repeat(np.arange(n_own), np.diff(rowptr))
            between += int(np.sum((row_of[own][1:] == row_of[own][:-1]) & (np.diff(own) > 1)))
        assert between >= 1, name


def test_faults_spoil_only_the_rows_from_their_own_on(kernel_cases):
    clean = ic.block_reference(ic.fault_case(None), [0, ic.BANDED_N], 0)
    assert np.array_equal(pc.bits(clean["f"][3]), pc.bits(ic.sweep_factors(clean["bp"], clean["bc"], clean["a_vals"], 3)))
    r = ic.FAULT_ROW
    for kind in ic.FAULT_KINDS:
        ref = ic.block_reference(ic.fault_case(kind), [0, ic.BANDED_N], 0)
        head = int(ref["bp"][r])
        assert head == clean["bp"][r]
        for t in range(4):
            assert np.array_equal(pc.bits(ref["f"][t][:head]), pc.bits(clean["f"][t][:head])), (kind, t)
        changed = not np.array_equal(pc.bits(ref["f"][3][head:]), pc.bits(clean["f"][3][head:])) or len(ref["bc"]) != len(clean["bc"])
        assert changed, kind
        dinv, word = ic.pivots(ref["bdiag"], ref["f"][3], ref["word"])
        print(f"{kind}: {int(np.isnan(ref['f'][3]).sum())} NaN and {int(np.isinf(ref['f'][3]).sum())} Inf entries after 3 sweeps, "
              f"word of the fill {ref['word']}, after the pivots {word}")
        assert (ref["word"] == ic.NO_FAILURE) == (kind in ("inf_diagonal", "nan_off", "inf_off", "negative_zero_off"))


def test_pivots_restatement_at_its_special_values():
    for n in ic.PIVOT_SIZES:
        bdiag, f = ic.pivot_case(n)
        dinv, word = ic.pivots(bdiag, f)
        if n == 1:
            assert word == ic.NO_FAILURE and dinv[0] == 1.0 / f[0]
            continue
        assert np.isnan(dinv[1]) and np.isnan(dinv[n - 2]) and word >> 2 not in (1, n - 2)
        rows = np.linspace(3, n - 1, 8).astype(np.int64)
        u = f[bdiag[rows]]
        assert np.array_equal(pc.bits(u), pc.bits(np.array(ic.PIVOT_SPECIALS)))
        failing = rows[[1, 3, 5, 6, 7]]                          # +Inf, 0.0, NaN, -0.0, -Inf
        assert word == (int(failing[0]) << 2) | ic.BAD_PIVOT
        assert np.isinf(dinv[rows[0]]) and np.isinf(dinv[rows[2]]) and dinv[rows[4]] == 1e-308       # denormal pivots: no code
        assert np.signbit(dinv[rows[6]]) and np.isinf(dinv[rows[6]]) and dinv[rows[7]] == 0.0 and np.signbit(dinv[rows[7]])
        if n == 600:
            assert sorted(set((failing // 256).tolist())) == [0, 1, 2]
        # the word coming in: a smaller row stays, a larger one and all ones give way, the same row's structural code stays
        first = int(failing[0])
        assert ic.pivots(bdiag, f, (2 << 2) | ic.NO_DIAG)[1] == (2 << 2) | ic.NO_DIAG
        assert ic.pivots(bdiag, f, ((n + 5) << 2) | ic.BAD_DIAG)[1] == word
        for code in (ic.NO_DIAG, ic.BAD_DIAG):
            assert ic.pivots(bdiag, f, (first << 2) | code)[1] == (first << 2) | code


def test_trisweep_and_apply_chain_restatements(kernel_cases):
    differ = 0
    for n in ic.RAGGED_SIZES:
        rowptr, cols, vals = ic.ragged(n)
        lower = np.array([np.sum(cols[rowptr[i]:rowptr[i + 1]] < i) for i in range(n)])
        upper = np.array([np.sum(cols[rowptr[i]:rowptr[i + 1]] > i) for i in range(n)])
        assert np.array_equal(lower, np.minimum(np.arange(n), (7 * np.arange(n)) % 20))
        assert np.array_equal(upper, np.minimum(n - 1 - np.arange(n), (5 * np.arange(n)) % 19))
        if n >= 127:
            for lanes in ic.LANES[1:]:                           # part lengths below, at and above the lane count, and 2 lanes + 1
                assert {lanes - 1, lanes, lanes + 1, 2 * lanes + 1} <= set(lower.tolist()) & set(upper.tolist()), (n, lanes)
        bp, bcols, brows, bdiag, bmap, f, word = ic.block_of_split(rowptr, cols, vals, n)
        rng = np.random.default_rng(n)
        r, x = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
        dinv = 1.0 / f[bdiag]
        for up in (0, 1):
            outs = [ic.trisweep(bp, bcols, bdiag, f, r, x, dinv, up, lanes) for lanes in ic.LANES]
            L, U, d = ic.split_factors(bp, bcols, f)
            want = (r - pc.matvec(*(U if up else L), x)) / d if n > 1 else r / d
            for out in outs:
                assert np.allclose(out, want, rtol=1e-12, atol=1e-12 * np.abs(want).max()), (n, up)
            rows = [i for i in range(n) if len({int(pc.bits(out[i:i + 1])[0]) for out in outs}) == 4]
            differ += len(rows)
            assert np.array_equal(pc.bits(ic.trisweep(bp, bcols, bdiag, f, r, None, dinv, up, 4)), pc.bits(r * dinv))
            assert np.array_equal(pc.bits(ic.trisweep(bp, bcols, bdiag, f, r, None, None, up, 1)), pc.bits(r))
        for s in (1, 3):
            got = ic.apply_chain(bp, bcols, bdiag, f, dinv, r, s, 1)
            want = ic.apply(bp, bcols, f, r, s)
            assert np.allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max()), (n, s)
    print(f"{differ} (size, part, row) triples on which lanes 1, 2, 4 and 8 give four different bit patterns")
    assert differ >= 1
    for name in ("arrow", "banded16", "convdiff16x16", "asymmetric"):
        matrix = kernel_cases[name]
        n = len(matrix[0]) - 1
        ref = ic.block_reference(matrix, [0, n], 0)
        f = ref["f"][3]
        dinv, word = ic.pivots(ref["bdiag"], f)
        assert word == ic.NO_FAILURE
        r = np.random.default_rng(3).uniform(-1, 1, n)
        for s in (1, 2, 3, 16):
            want = ic.apply(ref["bp"], ref["bc"], f, r, s)
            for lanes in ic.LANES:
                got = ic.apply_chain(ref["bp"], ref["bc"], ref["bdiag"], f, dinv, r, s, lanes)
                assert lanes > 1 or np.allclose(got, want, rtol=1e-12, atol=1e-12 * np.abs(want).max()), (name, s)
                assert np.allclose(got, want, rtol=1e-10, atol=1e-10 * np.abs(want).max()), (name, s, lanes)
