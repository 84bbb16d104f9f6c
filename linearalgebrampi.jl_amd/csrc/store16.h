// store16.h -- V consecutive 4- or 8-byte items leave a lane in whole 16-byte accesses (cdna_hip_programming.md, Guideline 13):
// the store half of the coalesced fills of submatrix.hip and select.hip.
#pragma once
#include "common.h"

namespace hpcla {

template <typename T> struct Vec16;
template <> struct Vec16<uint32_t> { using type = uint4; static constexpr int N = 4; };
template <> struct Vec16<uint64_t> { using type = ulonglong2; static constexpr int N = 2; };
template <> struct Vec16<int32_t> { using type = uint4; static constexpr int N = 4; };
template <> struct Vec16<int64_t> { using type = ulonglong2; static constexpr int N = 2; };

// V consecutive items at a 16-byte aligned dst
template <typename T, int V>
__device__ __forceinline__ void store_run(T *dst, const T (&v)[V])
{
    using W = typename Vec16<T>::type;
    constexpr int N = Vec16<T>::N;
#pragma unroll
    for (int q = 0; q < V / N; ++q) {
        W w;
        __builtin_memcpy(&w, &v[q * N], 16);
        *reinterpret_cast<W *>(dst + q * N) = w;
    }
}

}  // namespace hpcla
