"""CPU tests of bench.py's host-side helpers (the benchmark itself needs an MI355X)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_cpu_baseline_leg_reports_the_contract_fields(orc):
    import bench
    rows = orc.poisson2d_rows(64, 64, 0, 64 * 64)
    ci, cv = orc.compress_columns(rows)
    x = orc.fill_uniform(0, 64 * 64, 1)
    out = bench.cpu_baseline_spmv(rows.rowptr.astype(np.int32), cv.astype(np.int32), rows.vals, x, 0.4)
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in out
    assert out["kind"] == "port" and out["unit"] == "GFLOP/s" and out["cores"] >= 1 and out["value"] > 0
    assert out["scipy_bits_equal_oracle"] is True
    json.dumps(out)                                             # serialisable as part of the JSON line


def test_cpu_baseline_rates_are_never_rounded_to_zero(orc, monkeypatch):
    """VERDICT r4 (weak 9): on a cold / oversubscribed host the 8-thread call over a tiny matrix is slow enough that a rate
    rounded to 3 decimals printed as 0.0.  The leg now keeps 6 SIGNIFICANT digits; made deterministic here by slowing the
    oracle's SpMV down by ~50 ms per call (a 200-entry matrix then runs at ~1e-5 GFLOP/s)."""
    import time
    import bench
    from oracle import oracle as orc_mod
    rows = orc.poisson2d_rows(8, 5, 0, 40)
    ci, cv = orc.compress_columns(rows)
    x = orc.fill_uniform(0, 40, 1)
    real = orc_mod.spmv

    def slow(*a, **k):
        time.sleep(0.05)
        return real(*a, **k)
    monkeypatch.setattr(orc_mod, "spmv", slow)
    out = bench.cpu_baseline_spmv(rows.rowptr.astype(np.int32), cv.astype(np.int32), rows.vals, x, 0.2)
    assert 0 < out["value"] < 1e-3 and 0 < out["value_1core"] < 1e-3 and out["scipy_1thread_gflops"] > 0
    assert out["ms_per_spmv"] >= 50.0


def test_configs_digest_carries_five_numbers_to_the_top_level():
    """the driver's parsed record keeps only key NAMES of the sub-records; the digest puts config 3's ms,
    CG ms/iter, config 5's row-major and column-major-caller ms and the Int64 ms at the top level (None where a record was
    skipped or failed)."""
    import bench
    line = {"strong_scaling": {"ms_per_step": 0.9},
            "other_configs": {"poisson3d_cg": {"ms_per_step": 0.48}, "int64": {"ms_per_step": 0.23},
                              "poisson2d_spmm": {"device_ms_per_step": 0.475, "odd_k": {"device_ms_per_step": 0.52}},
                              "sprand_spmm": {"ms_per_step": 1.47, "column_major_caller": {"via_b_conversion_and_colmajor_store_ms": 2.05}}}}
    d = bench.configs_digest(line)
    assert d == {"cfg3_poisson8192_spmv_ms": 0.9, "cfg4_cg_ms_per_iter": 0.48, "cfg5_spmm_rowmajor_ms": 1.47,
                 "cfg5_spmm_colmajor_caller_ms": 2.05, "headline_int64_ms": 0.23, "stencil_spmm_k16_ms": 0.475,
                 "stencil_spmm_k15_ms": 0.52}
    d = bench.configs_digest({"strong_scaling": {"skipped": "budget"}, "other_configs": {"sprand_spmm": {"error": "x"}}})
    assert set(d) == {"cfg3_poisson8192_spmv_ms", "cfg4_cg_ms_per_iter", "cfg5_spmm_rowmajor_ms", "cfg5_spmm_colmajor_caller_ms",
                      "headline_int64_ms", "stencil_spmm_k16_ms", "stencil_spmm_k15_ms"} and all(v is None for v in d.values())
    assert all(v is None for v in bench.configs_digest({}).values())


def test_roofline_fraction_and_value_share_one_clock():
    """`roofline.frac` must follow from `ms_per_step` (the clock of `value`), the HIP-event figure kept
    beside it as frac_device_events.  Static check of the expressions in bench.py (the line itself needs a GPU; the GPU test
    test_bench_line_roofline_follows_from_ms_per_step recomputes it from a real line)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "achieved = b_alg_loc / (ms_per_step * 1e-3) / 1e9" in src
    assert "achieved_events = b_alg_loc / (timed_region_launch_ms * 1e-3) / 1e9" in src
    assert '"frac_device_events": round(achieved_events / HBM_PEAK_GBS, 4)' in src


def test_stdout_guard_keeps_native_prints_off_stdout():
    """Whatever writes to file descriptor 1 while the guard is active (RCCL prints a banner there) must land
    on stderr; what bench.py prints afterwards must be the only stdout line."""
    code = (
        "import os, sys; sys.path.insert(0, %r); import bench\n"
        "with bench._StdoutToStderr():\n"
        "    os.write(1, b'native banner\\n'); print('python chatter')\n"
        "print('{\"the\": \"line\"}')\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert out.stdout == '{"the": "line"}\n'
    assert "native banner" in out.stderr and "python chatter" in out.stderr


def test_usable_cores_respects_override(monkeypatch):
    import bench
    monkeypatch.setenv("HPCLA_CPU_THREADS", "3")
    assert bench.usable_cores() == 3
    monkeypatch.delenv("HPCLA_CPU_THREADS")
    assert 1 <= bench.usable_cores() <= 64


def test_guarded_breakdown_watchdog_prints_the_result_and_exits():
    """The optional transport comparison runs under a watchdog: if it hangs, the finished result line is still
    printed (once, on the real stdout) and the process exits with the verification's code."""
    import subprocess
    code = ("import os, sys, time, json\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "import bench\n"
            "res = {'metric': 'm', 'value': 1.0}\n"
            "bench._guarded_breakdown(lambda: time.sleep(30), res, True, 1, 0.3)\n"
            "print('not reached')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-500:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and "not reached" not in out.stdout
    rec = json.loads(lines[0])
    assert rec["value"] == 1.0 and "error" in rec["step_breakdown_ms_max_over_ranks"]
    # and the ordinary case: the comparison's record comes back, nothing is printed by the guard
    code2 = ("import sys\n"
             f"sys.path.insert(0, {ROOT!r})\n"
             "import bench\n"
             "print(bench._guarded_breakdown(lambda: {'modes': {}}, {'value': 2.0}, True, 1, 30.0))\n")
    out2 = subprocess.run([sys.executable, "-c", code2], capture_output=True, text=True, timeout=60)
    assert out2.returncode == 0 and out2.stdout.strip() == "{'modes': {}}", (out2.stdout, out2.stderr[-300:])


# ---- the run's time budget (benchmarks/budget.py): every guard derives from ONE outer limit ------------------
class _Clock:
    def __init__(self, t=1000.0):
        self.t = t

    def __call__(self):
        return self.t


def _budget(outer=600.0, **kw):
    import io
    from benchmarks.budget import Budget
    clk = _Clock()
    return Budget(outer_s=outer, t0=clk.t, clock=clk, out=io.StringIO(), **kw), clk


def test_budget_guards_sum_to_less_than_the_outer_limit():
    """Round 2's guards (RCCL init 180 s + comparison 240 s, launcher 1500 s) could outlast the driver's 600 s.
    Now: RCCL init <= 60 s, comparison <= 90 s, launcher = outer - 30 s, for any outer limit."""
    for outer in (120.0, 300.0, 600.0, 1200.0):
        b, _ = _budget(outer)
        assert b.rccl_init_timeout() <= 60.0
        assert b.comparison_timeout() <= 90.0
        assert b.launcher_timeout() == max(outer - 30.0, 30.0) < outer
        assert b.rccl_init_timeout() + b.comparison_timeout() + b.spin_timeout() < outer - 30.0 or outer <= 120.0
    env = {}
    b, _ = _budget(600.0)
    b.export_guards(env)
    assert float(env["HPCLA_RCCL_INIT_TIMEOUT_S"]) <= 60 and float(env["HPCLA_PUSH_TIMEOUT_S"]) <= 20
    assert float(env["HPCLA_BENCH_T0"]) == b.t0
    env2 = {"HPCLA_RCCL_INIT_TIMEOUT_S": "7"}                   # an explicit setting wins
    b.export_guards(env2)
    assert env2["HPCLA_RCCL_INIT_TIMEOUT_S"] == "7"


def test_budget_skips_optional_stages_when_time_is_short():
    from benchmarks.budget import ESTIMATE_S, RESERVE_S
    b, clk = _budget(600.0)
    assert b.allows("strong_scaling") and b.allows("poisson3d_cg") and not b.skipped
    clk.t += 600.0 - RESERVE_S - ESTIMATE_S["strong_scaling_n1"] + 1.0      # one second short of the estimate
    assert not b.allows("strong_scaling_n1")
    assert b.allows("packed")                                               # a cheaper stage still fits
    clk.t += 100.0
    assert not b.allows("comparison") and b.comparison_timeout() == 0.0
    assert b.skipped == ["strong_scaling_n1", "comparison"]
    assert "SKIP strong_scaling_n1" in b.out.getvalue()


def test_budget_origin_travels_from_the_launching_parent(monkeypatch):
    """`python bench.py --gpus N` spawns its ranks: their clocks start at the PARENT's start (HPCLA_BENCH_T0), so
    the spawn, the imports and the rendezvous count against the same limit."""
    from benchmarks.budget import Budget
    clk = _Clock(5000.0)
    monkeypatch.setenv("HPCLA_BENCH_T0", "4900.0")
    monkeypatch.setenv("HPCLA_BENCH_OUTER_LIMIT_S", "200")
    b = Budget(clock=clk)
    assert b.outer == 200.0 and abs(b.elapsed() - 100.0) < 1e-9
    assert abs(b.remaining() - 70.0) < 1e-9 and b.launcher_timeout() == 170.0


def test_bench_main_derives_the_launcher_limit_from_the_outer_limit():
    """The self-launching parent must never outlive the driver's limit (round 2: 1500 s inside 600 s)."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert '"1500"' not in src and "budget.launcher_timeout()" in src
    assert "HPCLA_BENCH_BREAKDOWN_TIMEOUT_S\", \"240\"" not in src


def test_n_gt_1_records_carry_roofline_traffic_from_the_single_rank_passes():
    """no `"traffic": null` in an N > 1 line.  PMC counters cannot be read from inside the process,
    so every record takes the builder's stored single-rank rocprofv3 passes of the same per-GPU share and SAYS so."""
    import bench
    from benchmarks.extra_workloads import stored_traffic
    for world in (1, 2, 8):
        t, src = bench.headline_traffic(32, True)
        assert t and t > 1.3e9 and "NOT measured by this run" in src
    t1, s1 = bench.headline_traffic(1, True)               # the natural order has a pass of its own
    t32, s32 = bench.headline_traffic(32, True)
    assert t1 != t32 and "natural" in s1 and "groups of 32" in s32
    assert bench.headline_traffic(32, False) [0] is None
    for key in ("poisson3d_cg_iteration", "poisson2d_spmm", "sprand_spmm_b2e24"):
        t1, s1 = stored_traffic(key, True, 1)
        t8, s8 = stored_traffic(key, True, 8, "note about the share")
        assert t1 == t8 and t1 > 1e9
        assert "SINGLE-RANK" in s8 and "N = 8" in s8 and "note about the share" in s8 and "SINGLE-RANK" not in s1
    assert stored_traffic("no such workload", True, 8)[0] is None


def test_profiled_kernel_names_follow_the_kernel_templates():
    """a record named a kernel that no longer existed after a template refactor, and the PMC table script
    matched zero rows.  The names bench.py prints and benchmarks/collect_profiles.py matches must carry as many template
    arguments as the kernels have parameters in csrc/ (rocprofv3 prints every argument, defaults included)."""
    import re
    import types
    import bench
    csrc = os.path.join(ROOT, "linearalgebrampi.jl_amd", "csrc")

    def n_template_params(path, kernel):
        text = open(os.path.join(csrc, path)).read()
        m = re.search(r"template <([^>]*)>\s*\n__global__[^\n]*void %s\(" % kernel, text)
        assert m, (path, kernel)
        return len([p for p in m.group(1).split(",") if p.strip()])

    n_rg = n_template_params("spmv.hip", "spmv_rowgather_kernel")
    n_t = n_template_params("rowgather_t.h", "rowgather_kernel")
    inst = bench.spmv_kernel_instance(None, is_i64=True, split=True, wait=False)
    assert inst.startswith("hpcla::spmv_rowgather_kernel<long, true, false") and inst.count(",") == n_rg - 1, (inst, n_rg)
    assert "spmv_rowblock_quad_kernel" not in open(os.path.join(csrc, "spmv.hip")).read()      # retired in round 6
    assert bench.f32_kernel_name(16).count(",") == n_t - 1
    import importlib.util
    spec = importlib.util.spec_from_file_location("collect_profiles", os.path.join(ROOT, "benchmarks", "collect_profiles.py"))
    cp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cp)
    assert cp.KERNEL.startswith("spmv_rowgather_kernel<") and cp.KERNEL.count(",") == n_rg - 1
    table = open(os.path.join(ROOT, "benchmarks", "pmc_f32_table.py")).read()
    m = re.search(r'rg = lambda kc: "rowgather_kernel<([^"]*)>"', table)
    assert m and m.group(1).count(",") == n_t - 1


def test_bench_options_full_and_dump_outputs(monkeypatch, tmp_path):
    """--full is off by default (a plain run times the headline only); --dump-outputs takes a directory, made absolute so that
    spawned ranks write to the same place, and is refused for workloads it does not cover."""
    import pytest
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "3"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 3
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "rel_dir"])
    a = bench.parse()
    assert a.full is True and os.path.isabs(a.dump_outputs) and a.dump_outputs.endswith("rel_dir")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--workload", "poisson3d_cg", "--dump-outputs", str(tmp_path)])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_rows_are_fixed_bounded_and_cover_the_edges():
    """The sample --dump-outputs writes: the same rows in every run, sorted and distinct, within 64 MB with its row numbers
    (float64 values + float64 row numbers), the halo-adjacent first and last grid lines included; small outputs whole."""
    import bench
    n = 4096 * 4096
    for world in (1, 2, 8):
        r = bench.dump_rows(n, world)
        assert np.array_equal(r, bench.dump_rows(n, world))
        assert np.all(np.diff(r) > 0) and r[0] == 0 and r[-1] == n - 1 and r.max() < n
        assert world * r.size * 16 <= 64 * 2**20
        assert np.array_equal(r[:4096], np.arange(4096)) and np.array_equal(r[-4096:], np.arange(n - 4096, n))
    assert np.array_equal(bench.dump_rows(1000, 1), np.arange(1000))
