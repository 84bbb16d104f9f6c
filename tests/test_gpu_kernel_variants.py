"""The kernel variants that only an environment switch selects, each in a child process of its own.

The suite compares every kernel family with numpy and the oracle under the DEFAULT environment; the plain-load/store forms
of the solver kernels (HPCLA_CG_NT), the plain store and the forced block order of the SpMV, the pass sizes / lane mappings /
store paths of the vector SpMM and the column-group widths and unrolls of the column-major product are reached through
switches that the library reads once per process.  tests/_kernel_variants_worker.py runs the existing checks of a family
under such a setting and prints fingerprints of results that the sources promise to carry the same bits under every setting
("same operations on the same operands: same bits", csrc/vecops.hip; every block order is a bijection, csrc/spmv.hip,
csrc/spmm.hip; each C(r, c) is one running sum in stored order whatever the lane mapping, csrc/spmm.hip, csrc/rowgather_t.h).

The families launch disjoint kernels, so one child carries one setting of each family (SETTINGS); the baseline child runs
every family's checks with every variable of the table removed.  A child's test asserts its exit status, its OK line, that it
ran the checks the baseline ran for the families it carries (a child that skips one fails), and that every fingerprint
equals the baseline's.  The children run one after another; after a child that ends by a signal, an abort or at the time
limit no further child is started.

tests/test_host_logic.py checks the names of this table against the getenv calls of csrc/.

Wall time of the children on the MI355X, process start to exit (the cap is 180 s a child; about 3 s of each is the import
of torch and the first HIP call): baseline 4.6 s (checks: cg 0.7, spmv 0.1, spmm 1.5, colmajor 0.1, fingerprints 0.2);
HPCLA_CG_NT=0 ... 7.6 s (cg 3.9: the three solver files at n = 4 194 307, mostly math.fsum on the host); HPCLA_CG_NT=1 ... 4.2 s;
HPCLA_CG_NT=6 ... 4.3 s; the four children without a solver setting 3.9 - 4.0 s each; the module 37 s.
"""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_kernel_variants_worker.py")
CHILD_TIMEOUT_S = 180              # a cap against a hang, not an expectation

# family -> the settings to cover; child i carries the i-th setting of each family that has one
FAMILY_SETTINGS = {
    "cg": [{"HPCLA_CG_NT": "0"}, {"HPCLA_CG_NT": "1"}, {"HPCLA_CG_NT": "6"}],
    "spmv": [{"HPCLA_SPMV_NT_Y": "0"}, {"HPCLA_SPMV_XCD_GROUP": "4"}, {"HPCLA_SPMV_XCD_GROUP": "1024"}],
    "spmm": [{"HPCLA_SPMM_CHUNK": "512"}, {"HPCLA_SPMM_CHUNK": "1536"}, {"HPCLA_SPMM_HALF64": "0"}, {"HPCLA_SPMM_CSTAGE": "0"},
             {"HPCLA_SPMM_LPR": "4"}, {"HPCLA_SPMM_HALF64": "0", "HPCLA_SPMM_CSTAGE": "0", "HPCLA_SPMM_LPR": "4"},
             {"HPCLA_SPMM_XCD_GROUP": "4"}],
    "colmajor": [{"HPCLA_COLMAJOR_KC": "4"}, {"HPCLA_COLMAJOR_KC": "8"}, {"HPCLA_COLMAJOR_KC": "8", "HPCLA_COLMAJOR_UR": "2"},
                 {"HPCLA_COLMAJOR_KC": "16", "HPCLA_COLMAJOR_UR": "1"}, {"HPCLA_COLMAJOR_KC": "16", "HPCLA_COLMAJOR_UR": "3"},
                 {"HPCLA_COLMAJOR_KC": "16", "HPCLA_COLMAJOR_UR": "4"}],
}
TABLE_VARIABLES = sorted({v for settings in FAMILY_SETTINGS.values() for s in settings for v in s})
N_CHILDREN = max(len(s) for s in FAMILY_SETTINGS.values())
# SETTINGS[i] = {family: {variable: value}} of child i
SETTINGS = [{f: s[i] for f, s in FAMILY_SETTINGS.items() if i < len(s)} for i in range(N_CHILDREN)]
LARGE_IN = {"HPCLA_CG_NT": "0"}    # the child that also runs the solver kernels at n = 4 194 307


def _name(setting):
    return " ".join(f"{v}={val}" for fam in setting.values() for v, val in fam.items())


NAMES = [_name(s) for s in SETTINGS]


def _run_child(setting):
    """One child: ({family: {variable: value}}; {} = the baseline) -> dict(rc, abnormal, out, seconds, report)."""
    env = {k: v for k, v in os.environ.items() if k not in TABLE_VARIABLES}
    cmd = [sys.executable, WORKER]
    if setting:
        for fam in setting.values():
            env.update(fam)
        cmd += ["--families", ",".join(setting)]
        if setting.get("cg") == LARGE_IN:
            cmd.append("--large")
    t0 = time.perf_counter()
    try:
        done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT_S)
        rc, out, abnormal = done.returncode, done.stdout[-6000:] + done.stderr[-3000:], done.returncode < 0 or done.returncode in (134, 139)
        lines = done.stdout.strip().splitlines()
    except subprocess.TimeoutExpired as e:
        rc, out, abnormal, lines = None, f"time limit of {CHILD_TIMEOUT_S} s\n" + str(e.stdout or "")[-3000:], True, []
    seconds = time.perf_counter() - t0
    report = None
    if rc == 0 and len(lines) >= 2 and lines[-1] == "kernel variants OK":
        report = json.loads(lines[-2])
    print(f"kernel variants child [{_name(setting) or 'baseline'}]: {seconds:.1f} s, exit {rc}"
          + (f", {report['seconds']}" if report else ""))
    return dict(rc=rc, abnormal=abnormal, out=out, seconds=seconds, report=report)


@pytest.fixture(scope="module")
def children():
    """The baseline, then the settings, one after another; nothing more is started after an abnormal end."""
    results, stopped_after = {}, None
    for key, setting in [("baseline", {})] + list(zip(NAMES, SETTINGS)):
        if stopped_after is not None:
            results[key] = dict(not_started=f"not started after {stopped_after} ended abnormally")
            continue
        results[key] = _run_child(setting)
        if results[key]["abnormal"]:
            stopped_after = key
    return results


def _passed(child):
    assert "not_started" not in child, child.get("not_started")
    assert child["rc"] == 0, child["out"]
    assert child["report"] is not None, "no OK line:\n" + child["out"]
    return child["report"]


def test_baseline_runs_every_check_under_the_default_environment(children):
    report = _passed(children["baseline"])
    assert report["env"] == {}
    assert set(report["checks"]) == set(FAMILY_SETTINGS) and all(report["checks"].values())
    assert len(report["fingerprints"]) >= 41


@pytest.mark.parametrize("i", range(N_CHILDREN), ids=NAMES)
def test_variant_passes_its_checks_and_keeps_the_bits(children, i):
    setting = SETTINGS[i]
    base = _passed(children["baseline"])
    report = _passed(children[NAMES[i]])
    assert report["env"] == {v: val for fam in setting.values() for v, val in fam.items()}
    # the checks of every family the child carries a setting of: what the baseline ran (and the large size where asked for)
    assert set(report["checks"]) == set(setting)
    for family in setting:
        ran = report["checks"][family]
        if setting[family] == LARGE_IN:
            assert set(base["checks"][family]) < set(ran) and len(ran) == len(base["checks"][family]) + 3, (family, ran)
        else:
            assert ran == base["checks"][family], (family, setting[family])
    assert set(report["fingerprints"]) == set(base["fingerprints"])
    # "family/name": the family whose kernels write that result
    differ = sorted((k.split("/")[0], setting.get(k.split("/")[0], "defaults"), k) for k, v in report["fingerprints"].items()
                    if base["fingerprints"][k] != v)
    assert not differ, f"{NAMES[i]}: (family, its variables, result) whose bits differ from the default environment's: {differ}"
