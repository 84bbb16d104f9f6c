// patterns.hip -- plan-time table of REPEATING row-block patterns for the row-gather SpMV (spmv.hip, IndexPolicy<Pat16>).
//
// No reference counterpart: the reference streams rowptr and colval as stored (src/sparse.jl:2055-2066).  For a structured
// grid nearly every 256-row block repeats one of a handful of index patterns -- its row lengths, its block-relative columns
// (the plan's cols16 copy) and the position of its first entry modulo 8 (the kernel's 16-byte loads start at p0 & ~7).
// The 4096-wide 5-point matrix has 18 of them in 8192 blocks, 46 KB in all: a table that lives in every XCD's L2.  A block
// in the table reads its columns and row bounds from there, so the 2 B per entry of cols16 and the 4 B per row of rowptr
// leave the HBM stream; what remains per block in HBM is one 8-byte record.  nzval is read live, as ever.
//
// Deduplication: every candidate block is hashed on the device, the hashes are counted on the host, the most frequent
// patterns are kept up to PAT_TABLE_CAP_BYTES, the table is built from one representative block per kept pattern, and
// every block is then compared EXACTLY with the pattern it was given, on the device: a mismatch (hash collision) puts the
// block back on the streamed form (id -1).  A collision can cost speed, never a bit.
#include <algorithm>
#include <unordered_map>
#include <vector>

#include "patterns.h"

namespace hpcla {

__device__ __forceinline__ uint64_t pat_mix(uint64_t key, uint64_t v)
{
    uint64_t z = key * 0x9E3779B97F4A7C15ull + v * 0xC2B2AE3D27D4EB4Full + 0x165667B19E3779F9ull;   // splitmix64 finish
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct PatMeta {
    int32_t first, len;
};

__device__ __forceinline__ int64_t pat_block(const int32_t *list, int64_t base, int64_t b) { return list ? (int64_t)list[b] : base + b; }

// hash[b] of candidate b: a sum of position-keyed mixes (any summation order gives the same hash); ~0: not a candidate for
// the table (more entries than 16-bit bounds hold, or row pointers that leave [0, nnz]).  weak: columns left out.
__global__ __launch_bounds__(PAT_RPB) void pat_hash_kernel(const int32_t *__restrict__ rowptr, const int16_t *__restrict__ cols16,
                                                           int64_t nrows, int64_t nnz, int base, const int32_t *__restrict__ list,
                                                           int64_t run_base, int weak, uint64_t *__restrict__ hash,
                                                           PatMeta *__restrict__ meta)
{
    __shared__ uint64_t s_h[PAT_RPB / 64];
    const int64_t blk = pat_block(list, run_base, blockIdx.x);
    const int64_t r0 = blk * PAT_RPB;
    const int nr = (int)((nrows - r0) < PAT_RPB ? (nrows - r0) : PAT_RPB);
    const int64_t p0 = (int64_t)rowptr[r0] - base, p1 = (int64_t)rowptr[r0 + nr] - base;
    const bool ok = p0 >= 0 && p1 >= p0 && p1 <= nnz && p1 - p0 <= PAT_MAX_LEN;
    uint64_t h = 0;
    if (ok) {
        const int tid = threadIdx.x;
        for (int i = tid; i <= nr; i += PAT_RPB) h += pat_mix(((uint64_t)1 << 32) | (uint32_t)i, (uint64_t)((int64_t)rowptr[r0 + i] - base - p0));
        if (!weak)
            for (int64_t j = tid; j < p1 - p0; j += PAT_RPB) h += pat_mix(((uint64_t)2 << 32) | (uint32_t)j, (uint16_t)cols16[p0 + j]);
        if (tid == 0) h += pat_mix((uint64_t)3 << 32, (uint64_t)(p0 & 7) | ((uint64_t)nr << 8));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) h += __shfl_down(h, off, 64);
    if ((threadIdx.x & 63) == 0) s_h[threadIdx.x >> 6] = h;
    __syncthreads();
    if (threadIdx.x == 0) {
        h = s_h[0] + s_h[1] + s_h[2] + s_h[3];
        if (h == ~(uint64_t)0) h -= 1;
        hash[blockIdx.x] = ok ? h : ~(uint64_t)0;
        meta[blockIdx.x] = PatMeta{ok ? (int32_t)p0 : 0, ok ? (int32_t)(p1 - p0) : 0};
    }
}

// table entry of one kept pattern from its representative block (the table was zeroed before)
__global__ __launch_bounds__(PAT_RPB) void pat_build_kernel(const int32_t *__restrict__ rowptr, const int16_t *__restrict__ cols16,
                                                            int64_t nrows, int base, const PatRec *__restrict__ reps,
                                                            int16_t *__restrict__ table)
{
    const int64_t blk = reps[blockIdx.x].first;
    int16_t *t = table + (int64_t)reps[blockIdx.x].id * 8;
    const int64_t r0 = blk * PAT_RPB;
    const int nr = (int)((nrows - r0) < PAT_RPB ? (nrows - r0) : PAT_RPB);
    const int64_t p0 = (int64_t)rowptr[r0] - base, len = (int64_t)rowptr[r0 + nr] - base - p0;
    const int phase = (int)(p0 & 7);
    for (int i = threadIdx.x; i <= PAT_RPB; i += PAT_RPB)
        t[i] = (int16_t)(uint16_t)((int64_t)rowptr[r0 + (i < nr ? i : nr)] - base - p0);
    if (threadIdx.x == 0) { t[PAT_NR] = (int16_t)nr; t[PAT_PHASE] = (int16_t)phase; }
    if (threadIdx.x <= PAT_RPB / 64) {
        const int i = threadIdx.x * 64;
        reinterpret_cast<int32_t *>(t + PAT_WAVE)[threadIdx.x] = (int32_t)((int64_t)rowptr[r0 + (i < nr ? i : nr)] - base - p0);
    }
    for (int64_t j = threadIdx.x; j < len; j += PAT_RPB) t[PAT_HEAD + phase + j] = cols16[p0 + j];
}

// the exact comparison: a candidate that differs from the pattern it was given anywhere goes back to the streamed form
__global__ __launch_bounds__(PAT_RPB) void pat_verify_kernel(const int32_t *__restrict__ rowptr, const int16_t *__restrict__ cols16,
                                                             int64_t nrows, int base, const int32_t *__restrict__ list,
                                                             int64_t run_base, const int16_t *__restrict__ table,
                                                             PatRec *__restrict__ rec)
{
    const int64_t blk = pat_block(list, run_base, blockIdx.x);
    const PatRec rc = rec[blk];
    if (rc.id < 0) return;                                   // workgroup-uniform
    const int16_t *t = table + (int64_t)rc.id * 8;
    const int64_t r0 = blk * PAT_RPB;
    const int nr = (int)((nrows - r0) < PAT_RPB ? (nrows - r0) : PAT_RPB);
    const int64_t p0 = (int64_t)rowptr[r0] - base, len = (int64_t)rowptr[r0 + nr] - base - p0;
    const int phase = (int)(p0 & 7);
    int bad = (p0 != rc.first) | (t[PAT_NR] != (int16_t)nr) | (t[PAT_PHASE] != (int16_t)phase) | (len > PAT_MAX_LEN);
    if (!bad) {                                              // (bounds first: len must be the pattern's before columns are read)
        for (int i = threadIdx.x; i <= PAT_RPB; i += PAT_RPB)
            bad |= ((int64_t)(uint16_t)t[i] != (int64_t)rowptr[r0 + (i < nr ? i : nr)] - base - p0);
    }
    bad = __syncthreads_or(bad);
    if (!bad) {
        for (int64_t j = threadIdx.x; j < len; j += PAT_RPB) bad |= (t[PAT_HEAD + phase + j] != cols16[p0 + j]);
        bad = __syncthreads_or(bad);
    }
    if (bad && threadIdx.x == 0) rec[blk].id = -1;
}

static void patterns_free(hpcla_block_patterns *p)
{
    if (!p) return;
    if (p->rec) (void)hipFree(p->rec);
    if (p->table) (void)hipFree(p->table);
    delete p;
}

// launch arguments of the pattern form for a product over (nrows, nnz, index_base), or an error when the handle was made
// for another structure
int patterns_args(const hpcla_block_patterns *p, int64_t nrows, int64_t nnz, int index_base, PatArgs *out)
{
    if (!p || !out) return set_error(HPCLA_ERR_INVALID, "block patterns: null handle");
    if (p->nrows != nrows || p->nnz != nnz || p->index_base != index_base)
        return set_error(HPCLA_ERR_INVALID, "block patterns: the handle was created for another structure (nrows / nnz / index_base)");
    out->rec = p->rec;
    out->table = p->table;
    return HPCLA_OK;
}

}  // namespace hpcla

using namespace hpcla;

HPCLA_API int hpcla_block_patterns_create_i32(hpcla_block_patterns_t **out, const int32_t *rowptr, const int16_t *cols16,
                                              int64_t nrows, int64_t nnz, int index_base, const int32_t *block_list,
                                              int64_t block_base, int64_t n_blocks, int flags, void *stream)
{
    if (!out) return set_error(HPCLA_ERR_INVALID, "block_patterns_create: null out");
    *out = nullptr;
    if (nrows < 0 || nnz < 0) return set_error(HPCLA_ERR_INVALID, "block_patterns_create: negative size");
    if (index_base != 0 && index_base != 1) return set_error(HPCLA_ERR_INVALID, "block_patterns_create: index_base must be 0 or 1");
    if (flags & ~HPCLA_BLOCK_PATTERNS_WEAK_HASH) return set_error(HPCLA_ERR_INVALID, "block_patterns_create: unknown flag");
    const int64_t all_blocks = (nrows + PAT_RPB - 1) / PAT_RPB;
    int64_t nc = all_blocks, run_base = 0;
    if (block_list) {
        if (n_blocks < 0 || n_blocks > all_blocks) return set_error(HPCLA_ERR_INVALID, "block_patterns_create: n_blocks out of range");
        nc = n_blocks;
    } else if (block_base >= 0) {
        if (n_blocks < 0 || block_base + n_blocks > all_blocks)
            return set_error(HPCLA_ERR_INVALID, "block_patterns_create: block run out of bounds");
        nc = n_blocks;
        run_base = block_base;
    }
    if (nc == 0 || nnz == 0) return HPCLA_OK;                  // nothing to tabulate: no handle
    if (!rowptr || !cols16) return set_error(HPCLA_ERR_INVALID, "block_patterns_create: null array");
    HPCLA_CHECK_GRID(nc, "block_patterns_create");
    hipStream_t s = as_stream(stream);

    // ---- hash every candidate on the device, count on the host ------------------------------------------------------
    uint64_t *d_hash = nullptr;
    PatMeta *d_meta = nullptr;
    PatRec *d_reps = nullptr;
    hpcla_block_patterns *p = nullptr;
    auto fail = [&](int code) {
        if (d_hash) (void)hipFree(d_hash);
        if (d_meta) (void)hipFree(d_meta);
        if (d_reps) (void)hipFree(d_reps);
        patterns_free(p);
        return code;
    };
#define PT_HIP(expr)                                                                                                   \
    do {                                                                                                               \
        hipError_t _e = (expr);                                                                                        \
        if (_e != hipSuccess) return fail(set_error(HPCLA_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(_e)));    \
    } while (0)
    PT_HIP(hipMalloc((void **)&d_hash, nc * sizeof(uint64_t)));
    PT_HIP(hipMalloc((void **)&d_meta, nc * sizeof(PatMeta)));
    pat_hash_kernel<<<(uint32_t)nc, PAT_RPB, 0, s>>>(rowptr, cols16, nrows, nnz, index_base, block_list, run_base,
                                                     (flags & HPCLA_BLOCK_PATTERNS_WEAK_HASH) ? 1 : 0, d_hash, d_meta);
    PT_HIP(hipGetLastError());
    std::vector<uint64_t> hash(nc);
    std::vector<PatMeta> meta(nc);
    std::vector<int32_t> blocks;                               // candidate -> row block (a list is read back once)
    PT_HIP(hipMemcpyAsync(hash.data(), d_hash, nc * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    PT_HIP(hipMemcpyAsync(meta.data(), d_meta, nc * sizeof(PatMeta), hipMemcpyDeviceToHost, s));
    if (block_list) {
        blocks.resize(nc);
        PT_HIP(hipMemcpyAsync(blocks.data(), block_list, nc * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    PT_HIP(hipStreamSynchronize(s));
    auto block_of = [&](int64_t b) -> int64_t { return block_list ? (int64_t)blocks[b] : run_base + b; };
    if (block_list)
        for (int64_t b = 0; b < nc; ++b)
            if (blocks[b] < 0 || blocks[b] >= all_blocks) return fail(set_error(HPCLA_ERR_INVALID, "block_patterns_create: block out of range"));

    struct Cls {
        int64_t count, first;                                  // blocks of this hash, the first of them (the representative)
    };
    std::unordered_map<uint64_t, Cls> classes;
    for (int64_t b = 0; b < nc; ++b) {
        if (hash[b] == ~(uint64_t)0) continue;
        auto it = classes.find(hash[b]);
        if (it == classes.end()) classes.emplace(hash[b], Cls{1, b});
        else ++it->second.count;
    }
    std::vector<std::pair<uint64_t, Cls>> order(classes.begin(), classes.end());
    std::sort(order.begin(), order.end(), [](const std::pair<uint64_t, Cls> &a, const std::pair<uint64_t, Cls> &b) {
        return a.second.count != b.second.count ? a.second.count > b.second.count : a.second.first < b.second.first;
    });
    // ---- keep the most frequent patterns up to the cap --------------------------------------------------------------
    std::unordered_map<uint64_t, int32_t> kept;                // hash -> place in the table, 16-byte units
    std::vector<PatRec> reps;                                  // {representative row block, place}
    int64_t used = 0, covered = 0;                             // 16-bit entries
    for (const auto &c : order) {
        const PatMeta &m = meta[c.second.first];
        const int64_t need = PAT_HEAD + (((int64_t)(m.first & 7) + m.len + 7) & ~(int64_t)7);
        if ((used + need) * (int64_t)sizeof(int16_t) > PAT_TABLE_CAP_BYTES) continue;
        kept.emplace(c.first, (int32_t)(used / 8));
        reps.push_back(PatRec{(int32_t)block_of(c.second.first), (int32_t)(used / 8)});
        used += need;
        covered += c.second.count;
    }
    // the pattern form pays when most blocks take it: otherwise no handle, and the plan launches the kernels it always did
    if (covered * 2 < nc || reps.empty()) return fail(HPCLA_OK);

    p = new hpcla_block_patterns;
    p->nrows = nrows; p->nnz = nnz; p->all_blocks = all_blocks; p->index_base = index_base;
    p->table_bytes = used * (int64_t)sizeof(int16_t);
    p->n_patterns = (int64_t)reps.size();
    p->n_candidates = nc;
    std::vector<PatRec> rec(all_blocks, PatRec{0, -1});
    for (int64_t b = 0; b < nc; ++b) {
        auto it = hash[b] == ~(uint64_t)0 ? kept.end() : kept.find(hash[b]);
        rec[block_of(b)] = PatRec{meta[b].first, it == kept.end() ? -1 : it->second};
    }
    PT_HIP(hipMalloc((void **)&p->rec, all_blocks * sizeof(PatRec)));
    PT_HIP(hipMalloc((void **)&p->table, p->table_bytes));
    PT_HIP(hipMalloc((void **)&d_reps, reps.size() * sizeof(PatRec)));
    PT_HIP(hipMemsetAsync(p->table, 0, p->table_bytes, s));
    PT_HIP(hipMemcpyAsync(p->rec, rec.data(), all_blocks * sizeof(PatRec), hipMemcpyHostToDevice, s));
    PT_HIP(hipMemcpyAsync(d_reps, reps.data(), reps.size() * sizeof(PatRec), hipMemcpyHostToDevice, s));
    pat_build_kernel<<<(uint32_t)reps.size(), PAT_RPB, 0, s>>>(rowptr, cols16, nrows, index_base, d_reps, p->table);
    PT_HIP(hipGetLastError());
    // ---- exact comparison of every block with its pattern ----------------------------------------------------------
    pat_verify_kernel<<<(uint32_t)nc, PAT_RPB, 0, s>>>(rowptr, cols16, nrows, index_base, block_list, run_base, p->table, p->rec);
    PT_HIP(hipGetLastError());
    PT_HIP(hipMemcpyAsync(rec.data(), p->rec, all_blocks * sizeof(PatRec), hipMemcpyDeviceToHost, s));
    PT_HIP(hipStreamSynchronize(s));                           // (rec, reps: host memory the copies read until here)
#undef PT_HIP
    for (const PatRec &r : rec) p->n_patterned += r.id >= 0;
    if (p->n_patterned * 2 < nc) return fail(HPCLA_OK);
    (void)hipFree(d_hash); (void)hipFree(d_meta); (void)hipFree(d_reps);
    *out = p;
    return HPCLA_OK;
}

HPCLA_API int hpcla_block_patterns_destroy(hpcla_block_patterns_t *p)
{
    patterns_free(p);
    return HPCLA_OK;
}

HPCLA_API int hpcla_block_patterns_info(const hpcla_block_patterns_t *p, int64_t *n_patterns, int64_t *table_bytes,
                                        int64_t *n_candidates, int64_t *n_patterned)
{
    if (!p) return set_error(HPCLA_ERR_INVALID, "block_patterns_info: null handle");
    if (n_patterns) *n_patterns = p->n_patterns;
    if (table_bytes) *table_bytes = p->table_bytes;
    if (n_candidates) *n_candidates = p->n_candidates;
    if (n_patterned) *n_patterned = p->n_patterned;
    return HPCLA_OK;
}
