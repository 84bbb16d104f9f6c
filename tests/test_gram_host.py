"""transpose(X) * Y for dense blocks, the parts that need no GPU: the C ABI of csrc/gram.hip as the header, the ctypes
table, the built library and the Julia extension describe it, and the host-only work-size function."""
import ctypes
import os
import re
import subprocess


from tests.test_julia_binding_signatures import header_prototypes, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAM = {"hpcla_gram_work_bytes": ("i64", ["i64", "i64", "i64"]),
        "hpcla_gram_f64": ("i32", ["ptr", "ptr", "i64", "i32", "ptr", "i64", "i32", "i64", "i64", "i64", "ptr", "ptr", "ptr"]),
        "hpcla_gram_f32": ("i32", ["ptr", "ptr", "i64", "i32", "ptr", "i64", "i32", "i64", "i64", "i64", "ptr", "ptr", "ptr"])}


def test_header_declares_the_gram_entries_and_ctypes_binds_them(hp):
    protos = header_prototypes()
    cls = {ctypes.c_void_p: "ptr", ctypes.c_int: "i32", ctypes.c_int64: "i64"}
    for name, (ret, params) in GRAM.items():
        assert protos.get(name) == (ret, params), (name, protos.get(name))
        assert name in hp._capi.EXPORTED_SYMBOLS
        assert [cls[t] for t in hp._capi._SIGNATURES[name]] == params
    assert hp._capi._RESTYPES["hpcla_gram_work_bytes"] is ctypes.c_int64


def test_library_exports_the_gram_entries(hp):
    lib = hp._capi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", hp._capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in GRAM:
        assert hasattr(lib, name)
        assert re.search(rf"\bT {name}$", out, flags=re.M), name


def test_work_bytes_is_host_only_and_monotone_in_rows(hp):
    lib = hp._capi.load()              # no device is touched: this runs on the CPU-only machine
    for m, k in [(16, 16), (64, 64), (4, 4), (1, 3), (200, 7)]:
        prev = 0
        for n in sorted(list(range(0, 2000, 37)) + [2 ** p + d for p in range(11, 26) for d in (-1, 0, 1, 12345)]):
            wb = lib.hpcla_gram_work_bytes(n, m, k)
            assert wb >= 8 and wb % 8 == 0
            assert wb >= prev, (m, k, n, wb, prev)
            prev = wb
        # a positive row count needs room for at least one m x k partial, and the scratch stays bounded
        assert lib.hpcla_gram_work_bytes(1, m, k) >= 8 * m * k
        assert lib.hpcla_gram_work_bytes(2 ** 30, m, k) <= max(8 * m * k, 32 << 20) * 2
    assert lib.hpcla_gram_work_bytes(0, 16, 16) == 8
    assert lib.hpcla_gram_work_bytes(100, 0, 16) == 8


def test_argument_errors_without_a_gpu(hp):
    """Bad sizes and layouts are refused before anything is launched."""
    lib = hp._capi.load()
    for fn in (lib.hpcla_gram_f64, lib.hpcla_gram_f32):
        assert fn(None, None, 16, 0, None, 16, 0, -1, 16, 16, None, None, None) == -1          # negative rows
        assert fn(None, None, 16, 2, None, 16, 0, 10, 16, 16, None, None, None) == -1          # bad layout
        assert fn(None, None, 15, 0, None, 16, 0, 10, 16, 16, None, None, None) == -1          # row-major ld < m
        assert fn(None, None, 9, 1, None, 16, 0, 10, 16, 16, None, None, None) == -1           # column-major ld < nrows
        assert "leading dimension" in hp._capi.last_error()
        assert fn(None, None, 16, 0, None, 16, 0, 10, 0, 16, None, None, None) == 0            # empty product: nothing to do


def test_python_operator_is_wired(hp):
    from hpcla_amd import dense
    assert hp.dense_matmat_t is dense.dense_matmat_t
    src = open(dense.__file__).read()
    body = src[src.index("class TransposedHPCMatrix"):src.index("def dense_matvec_t")]
    assert "dense_matmat_t(self.parent, x)" in body


def test_julia_extension_binds_the_gram_entries():
    text = open(os.path.join(ROOT, "integration", "HPCLinearAlgebraROCmExt.jl")).read()
    for T in ("Float64", "Float32"):
        assert re.search(r"function Base\.:\*\(At::Transpose\{" + T + r",HPCMatrix\{" + T + r",B\}\}, M::HPCMatrix\{"
                         + T + r",B\}\) where \{B<:ROCBackend\}", text), T
    protos = header_prototypes()
    calls = [c for c in julia_ccalls() if c[0].startswith("hpcla_gram")]
    assert {c[0] for c in calls} == set(GRAM)
    for name, classes, ret, line in calls:
        assert (ret, classes) == protos[name], (name, line)
    # the column-major blocks go in as they are: their own pointers, HPCLA_LAYOUT_COL (1), no conversion before the call
    body = text[text.index("function _gram("):]
    body = body[:body.index("\nend\n")]
    assert ": (_ptr(X.A), _ptr(Y.A))" in body
    for m in re.finditer(r"LIB\.hpcla_gram_f(?:32|64)\((.*?)\)::Cint\)", body, flags=re.S):
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        assert args[1] == "xp::Ptr{Cvoid}" and args[4] == "yp::Ptr{Cvoid}", args
        assert args[3] == "1::Cint" and args[6] == "1::Cint", args
    assert body.index("hpcla_transpose_f64") > body.index("hpcla_gram_f64")     # only the m x k result is relaid
