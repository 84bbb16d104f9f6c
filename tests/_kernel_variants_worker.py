"""GPU worker of tests/test_gpu_kernel_variants.py: the kernel variants that only an environment switch selects
(HPCLA_CG_NT, HPCLA_SPMV_NT_Y / _XCD_GROUP, HPCLA_SPMM_CHUNK / _HALF64 / _CSTAGE / _LPR / _XCD_GROUP, HPCLA_COLMAJOR_KC / _UR).
Every switch is read once per process, so the parent starts this file once per setting; one process, one GPU, no communicator.

  (a) the existing checks against numpy and the oracle, unchanged: the test functions of the solver files,
      tests/test_gpu_parity.py and tests/test_gpu_colmajor.py, called as plain functions with the objects tests/conftest.py's
      fixtures return.  ``--families`` names the families whose checks run (the parent names those the child carries a setting
      of; the baseline runs all four).  A failing check ends the process with a line that names the family and its variables.
  (b) fingerprints (sha256 of the raw bytes) of results that the sources promise to be the same bits under every setting;
      always all of them.

Prints one JSON line {"env", "checks", "fingerprints", "seconds"} and then ``kernel variants OK``."""
import argparse
import hashlib
import json
import os
import sys
import time
import traceback

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the variables of each family (the parent's settings table is checked against the sources by tests/test_host_logic.py)
FAMILY_VARIABLES = {
    "cg": ("HPCLA_CG_NT",),
    "spmv": ("HPCLA_SPMV_NT_Y", "HPCLA_SPMV_XCD_GROUP"),
    "spmm": ("HPCLA_SPMM_CHUNK", "HPCLA_SPMM_HALF64", "HPCLA_SPMM_CSTAGE", "HPCLA_SPMM_LPR", "HPCLA_SPMM_XCD_GROUP"),
    "colmajor": ("HPCLA_COLMAJOR_KC", "HPCLA_COLMAJOR_UR"),
}
FAMILIES = tuple(FAMILY_VARIABLES)
LARGE_N = 4194307                  # caps the reduction grid and is odd: in the HPCLA_CG_NT=0 child only

I32, I64 = np.int32, np.int64


def family_env(family):
    return {v: os.environ[v] for v in FAMILY_VARIABLES[family] if v in os.environ}


def cg_pair_alone(hp, n):
    """hpcla_cg_residual_f64 / hpcla_cg_direction_f64 on their own: elements bit-equal to numpy's separately rounded
    expressions (the library is built with -ffp-contract=off), the sum to 1e-12 of math.fsum (the margin of the solver files)."""
    import math
    import torch
    from tests import _pcg_cases as pc
    lib = hp._capi.load()
    rng = np.random.default_rng(n)
    r_h, q_h, x_h, p_h = (rng.uniform(-1.0, 1.0, n) for _ in range(4))
    alpha, num, den, beta, bnum, bden = 1.25, 0.7310585786300049, 1.9, -0.5, 0.3, 0.7
    f64 = dict(dtype=torch.float64, device="cuda")
    scal = torch.tensor([num, den, bnum, bden], **f64)
    up = lambda a: torch.from_numpy(a).cuda()
    P = lambda t: t.data_ptr()
    r, q, x, p = up(r_h), up(q_h), up(x_h), up(p_h)
    rr = torch.zeros(1, **f64)
    work = torch.zeros(lib.hpcla_reduce_work_bytes() // 8, **f64)
    assert lib.hpcla_cg_residual_f64(None, alpha, P(scal[0:1]), P(scal[1:2]), P(q), P(r), n, P(rr), P(work), None) == 0
    assert lib.hpcla_cg_direction_f64(alpha, P(scal[0:1]), P(scal[1:2]), beta, P(scal[2:3]), P(scal[3:4]), P(r), P(x), P(p), n,
                                      None) == 0
    torch.cuda.synchronize()
    a = alpha * num / den
    b = beta * bnum / bden
    r_new = r_h - a * q_h
    bits_eq = lambda t, want: np.array_equal(pc.bits(t.cpu().numpy()), pc.bits(want))
    assert bits_eq(r, r_new), "r - a Ap"
    assert bits_eq(x, x_h + a * p_h), "x + a p"
    assert bits_eq(p, r_new + b * p_h), "r + b p"
    assert bits_eq(q, q_h), "Ap is read only"
    want = math.fsum((r_new * r_new).tolist())
    assert abs(rr.item() - want) <= 1e-12 * want, (rr.item(), want)


def checks_of(family, hp, orc, backend, large):
    """[(name, callable, arguments, families)] of part (a) for one family; `families`: those whose kernels the check launches
    (a failure names their variables)."""
    out = []

    def add(fn, *args, kernels_of=None):
        plain = [a.__name__ if a in (I32, I64) else repr(a) for a in args if a in (I32, I64) or isinstance(a, (bool, int, float, str))]
        out.append((f"{fn.__module__.split('.')[-1]}.{fn.__name__}({', '.join(plain)})", fn, args, kernels_of or (family,)))

    if family == "cg":
        from tests import test_gpu_bicgstab, test_gpu_gmres, test_gpu_lsqr, test_gpu_minres, test_gpu_parity, test_gpu_pcg
        for n in (1, 2, 515, 2051) + ((LARGE_N,) if large else ()):
            for mod in (test_gpu_pcg, test_gpu_bicgstab, test_gpu_lsqr):
                add(mod.test_gated_kernels_alone, hp, n)
        for n in (1, 3, 1023, 2046):
            for precond in (False, True):
                add(test_gpu_minres.test_gated_kernels_alone, hp, n, precond)
        for n, c in ((1, 1), (515, 9), (2051, 17), (2051, 31)):
            add(test_gpu_gmres.test_gated_kernels_alone, hp, n, c)
        add(test_gpu_parity.test_fused_spmv_dot_and_cg_update, hp, orc, backend, kernels_of=("cg", "spmv"))
        for n in (1, 2, 515, 2051):
            add(cg_pair_alone, hp, n)
    elif family == "spmv":
        from tests import test_gpu_colmajor, test_gpu_parity
        for n, p in ((1, 1.0), (257, 0.05), (10_000, 0.01)):
            for Ti in (I32, I64):
                add(test_gpu_parity.test_spmv_sprand_bit_exact, hp, orc, backend, n, p, Ti)
        for Ti in (I32, I64):
            add(test_gpu_parity.test_spmv_rowgather_wave_pass_boundaries, hp, orc, backend, Ti)
            add(test_gpu_parity.test_spmv_kernel_forms_give_the_reference_bits, hp, orc, backend, Ti)
            # (csrc/colmajor.hip's launch of the SpMV's row-gather kernel: it stores through the same nt_y flag)
            add(test_gpu_colmajor.test_spmm_colmajor_f64_long_and_empty_rows, hp, orc, 2, Ti, kernels_of=("spmv", "colmajor"))
    elif family == "spmm":
        from tests import test_gpu_parity
        for k in (2, 6, 8, 16, 32, 40):
            add(test_gpu_parity.test_spmm_bit_exact_raw_abi, hp, orc, backend, k, "row")
            # (column-major B and C: hpcla_spmm_csr_f64_* routes to csrc/colmajor.hip)
            add(test_gpu_parity.test_spmm_bit_exact_raw_abi, hp, orc, backend, k, "col", kernels_of=("colmajor",))
        for k in (3, 7, 15, 16, 17):
            for c_layout in ("row", "col"):
                for Ti in (I32, I64):
                    add(test_gpu_parity.test_spmm_bit_exact_padded_pitch, hp, orc, backend, k, c_layout, Ti)
        for k in (16, 6, 3):
            for Ti in (I32, I64):
                add(test_gpu_parity.test_spmm_panel_accumulate_is_one_running_sum, hp, orc, backend, k, Ti)
        # the pass, tile and lane-group edges of tests/test_gpu_spmm_edges.py under every HPCLA_SPMM_* setting: other kernel
        # instances on the same matrices.  Under HPCLA_SPMM_CHUNK the passes are the forced size, so only the matrix laid out
        # for that size has its straddling rows on the real boundaries; the other one still has multi-pass blocks and is
        # compared bit for bit, and both matrices run under both settings
        from tests import _spmm_edge_cases as sc, test_gpu_spmm_edges
        for CH in (sc.CHUNK_V_SMALL, sc.CHUNK_V_LARGE):
            for Ti, base in ((I32, 0), (I64, 1)):
                add(test_gpu_spmm_edges.test_vector_kernel_at_pass_edges, hp, orc, CH, Ti, base)
        for Ti, base in ((I32, 1), (I64, 0)):
            add(test_gpu_spmm_edges.test_generic_kernel_at_pass_edges, hp, orc, Ti, base)
        add(test_gpu_spmm_edges.test_switch_between_the_two_pass_sizes, hp, orc, I32)
    elif family == "colmajor":
        from tests import test_gpu_colmajor
        for k in (2, 8, 16, 17, 40):
            for Ti in (I32, I64):
                add(test_gpu_colmajor.test_spmm_colmajor_f64_long_and_empty_rows, hp, orc, k, Ti)
        for k in (1, 3, 16):
            add(test_gpu_colmajor.test_spmm_split_colmajor_ghost_segment_and_block_lists, hp, orc, "f64", k)
    else:
        raise ValueError(family)
    return out


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def fingerprints(hp, orc, backend):
    """{"family/name": sha256} of results that must carry the same bits under every setting; the family is the one whose
    kernels write the result (the solvers also run the SpMV)."""
    import torch
    from tests import _bicgstab_cases as bc, _lsqr_cases as lc, _minres_cases as mc, _pcg_cases as pc
    fp = {}
    s = torch.cuda.current_stream().cuda_stream
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fixed = dict(rtol=0.0, atol=0.0, maxiter=8, check_every=8)

    def solver(name, solve, rowptr, colidx, vals, ncols, bg, preconds):
        A = hp.HPCSparseMatrix_local(rowptr, colidx, vals, ncols, backend)
        b = hp.HPCVector.from_global(bg, backend)
        for M in preconds:
            x, info = solve(A, b, M)
            tag = f"{name}[M={M}]" if len(preconds) > 1 else name
            fp[f"cg/{tag}.end"] = f"{info.status} after {info.iterations}"
            fp[f"cg/{tag}.x"] = sha(x.local_values())
            fp[f"cg/{tag}.residual_norms"] = sha(np.asarray(info.residual_norms, dtype=np.float64))

    sym = pc.scaled_poisson(orc, 24, 20)
    saddle = mc.scaled_saddle(orc, 24, 20)
    nonsym = bc.convection_diffusion(orc, 24, 20)
    both = (None, "jacobi")
    solver("cg", lambda A, b, M: hp.cg(A, b, M=M, **fixed), *sym[:3], len(sym[3]), sym[3], both)
    solver("minres", lambda A, b, M: hp.minres(A, b, M=M, **fixed), *saddle[:3], len(saddle[3]), saddle[3], both)
    solver("bicgstab", lambda A, b, M: hp.bicgstab(A, b, M=M, **fixed), *nonsym[:3], len(nonsym[3]), nonsym[3], both)
    solver("gmres", lambda A, b, M: hp.gmres(A, b, M=M, restart=8, **fixed), *nonsym[:3], len(nonsym[3]), nonsym[3], both)
    tall = lc.tall(orc, *lc.SIZES[0])
    solver("lsqr", lambda A, b, M: hp.lsqr(A, b, ntol=0.0, **fixed), *tall[:4], tall[4], (None,))
    hp.clear_plan_cache()

    # y of one raw-ABI SpMV at (10 000, 0.01)
    n = 10_000
    rows = orc.sprand_rows(n, 0.01, 0, n)
    ci, cv = orc.compress_columns(rows)
    x = orc.fill_uniform(0, n, orc.SEED_X)[ci]
    d = (t(rows.rowptr.astype(I32)), t(cv.astype(I32)), t(rows.vals), t(x))
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_spmv_csr_f64_i32", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), y.data_ptr(), n,
                  rows.nnz, 0, s)
    torch.cuda.synchronize()
    fp["spmv/spmv(10000, 0.01).y"] = sha(y.cpu().numpy())

    # C of the raw-ABI SpMM (3000 x 2500, p = 0.01: ~ 1600 entries per 64-row block) at k = 6, 15, 16, 32, both layouts
    n, m = 3000, 2500
    rows = orc.sprand_rows(m, 0.01, 0, n)
    ci, cv = orc.compress_columns(rows)
    d = (t(rows.rowptr.astype(I32)), t(cv.astype(I32)), t(rows.vals))
    ROW, COL = hp._capi.LAYOUT_ROW, hp._capi.LAYOUT_COL
    for k in (6, 15, 16, 32):
        B = orc.fill_uniform(0, len(ci) * k, 9).reshape(len(ci), k) - 0.5
        kp = k + (k & 1)                                     # odd k: the even pitch the vector kernel needs
        Bp = np.zeros((len(ci), kp))
        Bp[:, :k] = B
        for layout in ("row", "col", "row B, col C"):        # the last: the row kernel's column-major store (one launch per tile)
            if layout == "row":
                dB, ldb, ldc = t(Bp), kp, kp
                dC = torch.full((n, kp), float("nan"), dtype=torch.float64, device="cuda")
            else:
                dB, ldb, ldc = (t(B.T), len(ci), n) if layout == "col" else (t(Bp), kp, n)
                dC = torch.full((k, n), float("nan"), dtype=torch.float64, device="cuda")
            hp._capi.call("hpcla_spmm_csr_f64_i32", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), dB.data_ptr(), ldb,
                          COL if layout == "col" else ROW, dC.data_ptr(), ldc, ROW if layout == "row" else COL, n, rows.nnz, k, 0, s)
            torch.cuda.synchronize()
            C = dC.cpu().numpy()
            # (column-major B and C: hpcla_spmm_csr_f64_* routes to csrc/colmajor.hip)
            fp[f"{'colmajor' if layout == 'col' else 'spmm'}/spmm(k={k}, {layout}).C"] = sha(C[:, :k] if layout == "row" else C)

    # C of the raw-ABI SpMM on the pass matrix of 512-record passes (tests/_spmm_edge_cases.py) at k = 16
    from tests import _spmm_edge_cases as sc
    M = sc.pass_matrix(sc.CHUNK_V_SMALL)
    n, k = M["nrows"], 16
    d = (t(M["rowptr"].astype(I32)), t(M["colval"].astype(I32)), t(M["vals"]))
    dB = t(sc.master_B()[:, :k])
    dC = torch.full((n, k), float("nan"), dtype=torch.float64, device="cuda")
    hp._capi.call("hpcla_spmm_csr_f64_i32", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), dB.data_ptr(), k, ROW, dC.data_ptr(), k,
                  ROW, n, len(M["vals"]), k, 0, s)
    torch.cuda.synchronize()
    fp[f"spmm/pass matrix(CH={sc.CHUNK_V_SMALL}, k={k}).C"] = sha(dC.cpu().numpy())

    # C of the column-major SpMM with long and empty rows at k = 3, 16, 17
    rng = np.random.default_rng(3)
    ncols = 6000
    lens = rng.integers(0, 12, 600)
    lens[[1, 7, 300, 599]] = [2500, 464, 465, 930]
    lens[100:130] = 0
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(I32)
    colval = np.concatenate([np.sort(rng.choice(ncols, int(l), replace=False)) for l in lens]).astype(I32)
    vals = rng.random(len(colval)) - 0.5
    n = len(lens)
    d = (t(rowptr), t(colval), t(vals))
    for k in (3, 16, 17):
        B = rng.random((k, ncols)) - 0.5
        dB = t(B)
        dC = torch.full((k, n), float("nan"), dtype=torch.float64, device="cuda")
        hp._capi.call("hpcla_spmm_csr_f64_i32", d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), dB.data_ptr(), ncols, COL,
                      dC.data_ptr(), n, COL, n, len(vals), k, 0, s)
        torch.cuda.synchronize()
        fp[f"colmajor/long and empty rows(k={k}).C"] = sha(dC.cpu().numpy())
    return fp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--families", default=",".join(FAMILIES))
    ap.add_argument("--large", action="store_true", help=f"the solver kernels at n = {LARGE_N} too")
    args = ap.parse_args()
    families = [f for f in args.families.split(",") if f]
    assert set(families) <= set(FAMILIES), families
    t0 = time.perf_counter()

    import torch
    import hpcla_amd as hp
    from oracle import oracle as orc
    orc.build()
    assert torch.cuda.is_available()
    backend = hp.backend_rocm_serial(np.float64, np.int32)

    ran = {}
    seconds = {}
    for family in families:
        t1 = time.perf_counter()
        ran[family] = []
        for label, fn, fargs, kernels_of in checks_of(family, hp, orc, backend, args.large):
            try:
                fn(*fargs)
            except BaseException:
                traceback.print_exc(file=sys.stdout)
                variables = {v: val for f in kernels_of for v, val in family_env(f).items()}
                print(f"kernel variants FAILED: family {' + '.join(kernels_of)}, variables {variables or 'defaults'}, check {label}",
                      flush=True)
                sys.exit(1)
            ran[family].append(label)
        torch.cuda.synchronize()
        seconds[family] = round(time.perf_counter() - t1, 1)
    t1 = time.perf_counter()
    try:
        fp = fingerprints(hp, orc, backend)
    except BaseException:
        traceback.print_exc(file=sys.stdout)
        print(f"kernel variants FAILED: fingerprints, variables {({v: os.environ[v] for f in FAMILIES for v in family_env(f)})}",
              flush=True)
        sys.exit(1)
    seconds["fingerprints"] = round(time.perf_counter() - t1, 1)
    seconds["total"] = round(time.perf_counter() - t0, 1)
    sys.stdout.flush()
    print(json.dumps({"env": {v: os.environ[v] for f in FAMILIES for v in family_env(f)}, "checks": ran, "fingerprints": fp,
                      "seconds": seconds}))
    print("kernel variants OK", flush=True)


if __name__ == "__main__":
    main()
