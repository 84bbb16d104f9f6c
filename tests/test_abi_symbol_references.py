"""Every ``hpcla_*`` name that the scripts, the package, the tests and the Julia extension mention is a name the library
declares.  ctypes resolves symbols lazily, so a script that still calls an entry point the library has retired passes every
import and fails with AttributeError in the middle of a run (benchmarks/pmc_spmv_cases.py did: after measuring, before it
wrote its manifest)."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKEN = re.compile(r"\bhpcla_[a-z0-9_]+")           # whole words: libhpcla_rocm.so is a file name
# module, header, file and environment-prefix names that look like symbols and are none
NOT_SYMBOLS = {"hpcla_amd", "hpcla_rocm", "hpcla_budget", "hpcla_launch"}


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _without_comments(text):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def _declared():
    return set(TOKEN.findall(_without_comments(_read(os.path.join(ROOT, "include", "hpcla_rocm.h")))))


def _tuning_harness_symbols():
    """Functions the tuning harness's own sources DEFINE (name followed by a parameter list, comments stripped): a comment
    there that mentions a retired entry point must not put it on the list."""
    out = set()
    for path in glob.glob(os.path.join(ROOT, "benchmarks", "tune", "*.hip")):
        out |= set(re.findall(r"\b(hpcla_tune_[a-z0-9_]+)\s*\(", _without_comments(_read(path))))
    return out


def _sources():
    pats = [("benchmarks", "*.py"), ("linearalgebrampi.jl_amd", "*.py"), ("tests", "*.py"), ("tests", "cabi", "*.c"),
            ("integration", "HPCLinearAlgebraROCmExt.jl"), ("hpcla_amd.py",), ("bench.py",), ("__graft_entry__.py",)]
    files = sorted(p for pat in pats for p in glob.glob(os.path.join(ROOT, *pat)))
    assert len(files) > 60 and any(p.endswith(".jl") for p in files) and any(p.endswith(".c") for p in files)
    return files


def test_every_hpcla_name_in_the_sources_is_declared_by_the_header():
    declared = _declared()
    assert "hpcla_spmv_csr_f64_i32" in declared and "hpcla_set_spmv_kernel" not in declared    # retired: named in a comment only
    harness = _tuning_harness_symbols()
    assert {"hpcla_tune_spmv", "hpcla_tune_spmm", "hpcla_tune_spmm_runs"} <= harness
    known = declared | harness
    unknown = {}
    for path in _sources():
        if os.path.abspath(path) == os.path.abspath(__file__):
            continue
        for tok in set(TOKEN.findall(_read(path))):
            if tok in known or tok in NOT_SYMBOLS:
                continue
            if any(name.startswith(tok) and name != tok for name in declared):     # f"hpcla_spmv_csr_f64_{sfx}"
                continue
            unknown.setdefault(tok, []).append(os.path.relpath(path, ROOT))
    assert not unknown, f"names the library does not declare: {unknown}"
