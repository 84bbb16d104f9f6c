"""The launch grids of the two-stage reductions, the elementwise kernels, the scan and the digest, restated in plain Python, and
the sizes at which the GPU tests run each kernel family on its own.

Every device primitive that reduces or scans works in two stages: a first stage on a grid of bounded size and one workgroup
that walks that grid's partial results RT at a time.  Each therefore has loop trips and ragged ends that run only above a size
threshold; this module names those regimes and tests/test_grid_regimes.py asserts that every family's size list reaches each
one.  The constants are read from the csrc/ sources by regular expression (a pattern that no longer matches raises), so a
changed constant or a rewritten grid function fails that test instead of silently un-covering a regime.

Regimes of a reduction with g partials of `width` elements per lane and load:
  R1  g = 1: stage 1 alone writes the result;
  R2  2 <= g <= RT: stage 2 takes one trip and has idle lanes (g < RT) or none;
  R3  RT < g < cap and g mod RT != 0: stage 2 ends in a ragged trip;
  R4  g = cap and the stage-1 lanes take more than one grid-stride trip.
Regimes of an elementwise kernel: one workgroup ("E1"), several ("E2"), the capped grid with a further trip ("E3").
"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "linearalgebrampi.jl_amd", "csrc")


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _ints(name, pattern):
    """The groups of `pattern`'s only match in csrc/`name`, as ints."""
    found = re.findall(pattern, _source(name))
    assert len(found) == 1, f"csrc/{name}: {len(found)} matches of {pattern!r}"
    groups = found[0] if isinstance(found[0], tuple) else (found[0],)
    return [int(g) for g in groups if g.isdigit()]                 # a pattern without a group only has to be there


_WS = r"(?:\s|//[^\n]*\n)*"                                     # white space and line comments


def _pat(text):
    """A pattern from source text: blanks match any white space, `#` stands for a captured integer."""
    return _WS.join(re.escape(tok).replace(r"\#", r"(\d+)") for tok in text.split())


# ---- the constants, from the sources -------------------------------------------------------------------------------------------
RT, = _ints("vecops.hip", _pat("constexpr int RT = # ;"))
MAX_PARTIALS, = _ints("vecops.hip", _pat("constexpr int MAX_PARTIALS = # ;"))
# reduce_grid: g = (n / 2 + RT * 4 - 1) / (RT * 4), clamped to [1, MAX_PARTIALS]
REDUCE_WIDTH, REDUCE_PER_LANE, _rpl = _ints(
    "vecops.hip", _pat("static inline int reduce_grid ( int64_t n ) { int64_t g = ( n / # + RT * # - 1 ) / ( RT * # ) ;") +
    _WS + _pat("if ( g < 1 ) g = 1 ; if ( g > MAX_PARTIALS ) g = MAX_PARTIALS ;"))
assert _rpl == REDUCE_PER_LANE
# ew_grid: g = (items + 255) / 256, clamped to [1, 4096]
_ew_m1, EW_T, EW_CAP, _ew_cap = _ints(
    "vecops.hip", _pat("static inline uint32_t ew_grid ( int64_t n_items ) { int64_t g = ( n_items + # ) / # ;") + _WS +
    _pat("if ( g < 1 ) g = 1 ; if ( g > # ) g = # ;"))
assert _ew_m1 == EW_T - 1 and _ew_cap == EW_CAP
# reduce_partials_sum: one stage while np <= 4 * RT
PARTIALS_ONE_STAGE_TRIPS, = _ints("vecops.hip", _pat("if ( np <= # * RT ) {"))
# f32.hip: g = (n / 4 + F_RT * 4 - 1) / (F_RT * 4), clamped to [1, F_MAX_PARTIALS]
F_RT, = _ints("f32.hip", _pat("constexpr int F_RT = # ;"))
F_MAX_PARTIALS, = _ints("f32.hip", _pat("constexpr int F_MAX_PARTIALS = # ;"))
F_WIDTH, F_PER_LANE, _fpl = _ints(
    "f32.hip", _pat("int64_t g = ( n / # + F_RT * # - 1 ) / ( F_RT * # ) ;") + _WS +
    _pat("if ( g < 1 ) g = 1 ; if ( g > F_MAX_PARTIALS ) g = F_MAX_PARTIALS ;"))
assert _fpl == F_PER_LANE
# scan.h
SCAN_T, = _ints("scan.h", _pat("constexpr int SCAN_T = # ;"))
SCAN_E, = _ints("scan.h", _pat("constexpr int SCAN_E = # ;"))
_ints("scan.h", _pat("constexpr int SCAN_B = SCAN_T * SCAN_E ;"))
_ints("scan.h", _pat("static inline int64_t scan_blocks ( int64_t n ) { return ( n + SCAN_B - 1 ) / SCAN_B ; }"))
_ints("scan.h", _pat("for ( int64_t c = 0 ; c < nb ; c += SCAN_T ) {"))
SCAN_B = SCAN_T * SCAN_E
# the digest (construct.hip): g = (n + 255) / 256, at most 4096 workgroups of 256 lanes
_dg_m1, DIGEST_T, DIGEST_CAP, _dg_cap, _dg_t = _ints(
    "construct.hip", _pat("int64_t g = ( n + # ) / # ; if ( g > # ) g = # ;") + _WS +
    _pat("digest_kernel < I > <<< ( uint32_t ) g , # , 0 , s >>>"))
assert _dg_m1 == DIGEST_T - 1 and _dg_cap == DIGEST_CAP and _dg_t == DIGEST_T
# the two fused smoother kernels (amg.hip): g = (n / 2 + 255) / 256, clamped to [1, 4096], workgroups of 256 lanes
AMG_SMOOTH_WIDTH, _as_m1, AMG_SMOOTH_T, AMG_SMOOTH_CAP, _as_cap, _as_t = _ints(
    "amg.hip", _pat("int64_t g = ( n / # + # ) / # ; g = g < 1 ? 1 : ( g > # ? # : g ) ;") + _WS +
    _pat("amg_smooth_kernel < MODE > <<< ( uint32_t ) g , # , 0 , as_stream ( stream ) >>>"))
_as_first, _as_stride = _ints(
    "amg.hip", _pat("int64_t i = ( int64_t ) blockIdx . x * # + threadIdx . x ; const int64_t stride = ( int64_t ) gridDim . x * # ;") +
    _WS + _pat("for ( ; i < n2 ; i += stride ) {"))
assert _as_m1 == AMG_SMOOTH_T - 1 and _as_cap == AMG_SMOOTH_CAP and _as_t == AMG_SMOOTH_T == _as_first == _as_stride
# the ILU(0) kernels (ilu.hip): one lane per row, per entry or per (row, lane of the group), workgroups of ILU_THREADS lanes
ILU_THREADS, = _ints("ilu.hip", _pat("constexpr int ILU_THREADS = # ;"))
_ints("ilu.hip", _pat("const int64_t nb = ( nrows * lanes + ILU_THREADS - 1 ) / ILU_THREADS ;"))


# ---- the grid functions ----------------------------------------------------------------------------------------------------
def _ceil_div(a, b):
    return -(-a // b)


def reduce_grid(n):
    """Stage-1 workgroups (= partials) of an f64 reduction over n elements."""
    return min(max(_ceil_div(n // REDUCE_WIDTH, RT * REDUCE_PER_LANE), 1), MAX_PARTIALS)


def f32_reduce_grid(n):
    return min(max(_ceil_div(n // F_WIDTH, F_RT * F_PER_LANE), 1), F_MAX_PARTIALS)


def ew_grid(items):
    """Workgroups of an elementwise kernel over `items` lanes' worth of work (n // 2 double2 for the solver kernels)."""
    return min(max(_ceil_div(items, EW_T), 1), EW_CAP)


def scan_blocks(n):
    return _ceil_div(n, SCAN_B)


def scan_trips(n):
    """Trips of scan_phase2_kernel's loop over the block sums of an n-element scan."""
    return _ceil_div(scan_blocks(n), SCAN_T)


def digest_grid(n):
    return min(_ceil_div(n, DIGEST_T), DIGEST_CAP)


def digest_trips(n):
    return _ceil_div(n, digest_grid(n) * DIGEST_T) if n else 0


def amg_smooth_grid(n):
    """Workgroups of amg_smooth_kernel over n doubles (n // 2 double2, the odd element by one thread)."""
    return min(max(_ceil_div(n // AMG_SMOOTH_WIDTH, AMG_SMOOTH_T), 1), AMG_SMOOTH_CAP)


def ilu_grid(items):
    """Workgroups of an ILU(0) kernel over `items` rows, entries or rows * lanes."""
    return _ceil_div(items, ILU_THREADS)


def partials_two_stage(np_):
    """Whether reduce_partials_sum takes its two-stage branch for np_ partials."""
    return np_ > PARTIALS_ONE_STAGE_TRIPS * RT


# ---- regimes -----------------------------------------------------------------------------------------------------------------
REDUCTION_REGIMES = ("R1", "R2", "R3", "R4")
ELEMENTWISE_REGIMES = ("E1", "E2", "E3")


def _regime(g, items, lanes, cap):
    if g == 1:
        return "R1"
    if g <= lanes:
        return "R2"
    if g < cap:
        return "R3" if g % lanes else None
    return "R4" if items > g * lanes else None


def reduction_regime(n):
    return _regime(reduce_grid(n), n // REDUCE_WIDTH, RT, MAX_PARTIALS)


def f32_reduction_regime(n):
    return _regime(f32_reduce_grid(n), n // F_WIDTH, F_RT, F_MAX_PARTIALS)


def elementwise_regime(n):
    """Of a solver kernel over n doubles, launched on ew_grid(n // 2)."""
    g = ew_grid(n // 2)
    if g == 1:
        return "E1"
    if g < EW_CAP:
        return "E2"
    return "E3" if n // 2 > g * EW_T else None


def amg_smooth_regime(n):
    """Of the two smoother kernels over n doubles, on their own grid: E3 is the capped grid with a further grid-stride trip."""
    g = amg_smooth_grid(n)
    if g == 1:
        return "E1"
    if g < AMG_SMOOTH_CAP:
        return "E2"
    return "E3" if n // AMG_SMOOTH_WIDTH > g * AMG_SMOOTH_T else None


def has_tail(n, width=None):
    """Whether lane 0 of workgroup 0 has a scalar tail to add at this size."""
    return n % (REDUCE_WIDTH if width is None else width) != 0


# ---- the sizes of the "kernels alone" tests ------------------------------------------------------------------------------------
# 2049: R1 with a tail; 2051: R2, two partials, with a tail; 614 403: R3, 301 partials (a second, ragged trip of 45 in stage 2),
# 1201 elementwise workgroups, with a tail; 4 194 307: R4, 2048 partials, four stage-1 trips per lane and a fifth of lane 0, the elementwise grid capped at
# 4096 with a third trip, with a tail
R3_N, R4_N = 614_403, 4_194_307
PCG_ALONE = [1, 2, 511, 2049, 2051, R3_N, R4_N]
BICGSTAB_ALONE = [1, 2, 511, 515, 2049, 2051, R3_N, R4_N]
LSQR_ALONE = [1, 2, 511, 515, 2049, 2051, R3_N, R4_N]
MINRES_ALONE = [1, 2, 3, 1023, 2046, 2049, 2051, R3_N, R4_N]
GMRES_ALONE = ([(n, c) for n in (1, 2, 511, 515, 2049, 2051) for c in (1, 2, 8, 9, 16, 17, 31)] +
               [(R3_N, 1), (R3_N, 9), (R4_N, 1), (R4_N, 9)])
EIGSH_UPDATE_ALONE = ([(n, c) for n in (1, 2, 515, 2049, 2051) for c in (1, 8, 9, 17, 31)] +
                      [(R3_N, 1), (R3_N, 9), (R4_N, 9)])
# hp.dot / hp.norm / ...: 100 003 is R2 (49 partials), 4 000 001 R3 (1954), 4 194 307 R4
PLAIN_F64 = [1, 2, 3, 511, 512, 513, 100_003, 4_000_001, R4_N]
# (n, index of the NaN).  At R4_N a stage-1 trip is 2048 * 256 = 524 288 double2: the last lane of the last workgroup reads
# double2 2 097 151 = elements 4 194 302 | 303 in its fourth and last trip, double2 2 097 152 = elements 4 194 304 | 305 is the
# fifth trip of lane 0 alone, and element 4 194 306 is the scalar tail
PLAIN_F64_NAN = [(1, 0), (64, 63), (513, 0), (513, 512), (100_003, 50_001), (4_000_001, 3_999_999),
                 (R4_N, R4_N - 4), (R4_N, R4_N - 2), (R4_N, R4_N - 1)]
# float32 (four floats per lane and load, at most 1024 partials): 1 000 003 is R2 (245 partials), 1 228 807 R3 (301, tail of
# three), 4 194 307 R4 (1024 partials, four trips, tail of three)
F32_ALONE = [0, 1, 3, 4, 1023, 1024, 1025, 1_000_003, 1_228_807, R4_N]
# cg_update_ / cg_residual_ / cg_direction_ on vectors alone
CG_TRIO_ALONE = [1, 511, 2051, R3_N, R4_N]
# hpcla_amg_presmooth_f64 / hpcla_amg_postsmooth_f64 on vectors alone: 1, 2, 3 and 511 one workgroup (the odd element alone, one
# double2, both), 2051 five workgroups, R3_N 1201, R4_N the grid capped at 4096 with a third trip and the odd element
AMG_SMOOTH_ALONE = [1, 2, 3, 511, 2051, R3_N, R4_N]

REDUCTION_FAMILIES = {
    "pcg": PCG_ALONE, "bicgstab": BICGSTAB_ALONE, "lsqr": LSQR_ALONE, "minres": MINRES_ALONE,
    "gmres": sorted({n for n, _ in GMRES_ALONE}), "eigsh_update": sorted({n for n, _ in EIGSH_UPDATE_ALONE}),
    "plain_f64": PLAIN_F64, "plain_f64_nan": sorted({n for n, _ in PLAIN_F64_NAN}), "cg_trio": CG_TRIO_ALONE,
}
# families whose step also runs an elementwise kernel on ew_grid(n // 2) (the Lanczos second pass has none)
ELEMENTWISE_FAMILIES = {k: REDUCTION_FAMILIES[k] for k in ("pcg", "bicgstab", "lsqr", "minres", "gmres", "cg_trio")}
ELEMENTWISE_FAMILIES["amg_smooth"] = AMG_SMOOTH_ALONE             # no reduction: elementwise only, on a grid of its own
ELEMENTWISE_REGIME_OF = {"amg_smooth": amg_smooth_regime}         # every other family launches on ew_grid(n // 2)


def elementwise_regime_of(family):
    return ELEMENTWISE_REGIME_OF.get(family, elementwise_regime)

# ---- the scan, the partial sums and the digest -----------------------------------------------------------------------------------
# windows of hpcla_compress_columns: 256 blocks (one trip of phase 2), 257 (a second trip with one live lane), 601 (a ragged
# third trip); (width, col_lo)
SCAN_WINDOWS = [(262_144, 0), (262_145, 1_000), (R3_N, 70_001)]
SCAN_CARRY_AT = SCAN_T * SCAN_B                                    # the first element whose offset needs a carry
# row blocks of the fused SpMV's x.y epilogue: the last one-stage count, the first two-stage count, two stage-1 workgroups
PARTIAL_BLOCKS = [1024, 1025, 2052]
DIGEST_SIZES = [1, 255, 257, 1_048_576, 1_048_577, 2_500_003]
