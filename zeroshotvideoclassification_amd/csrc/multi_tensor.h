// multi_tensor.h -- how a table-driven launch finds its work, and what its entry point refuses (optim.hip, sgd.hip, layerwise.hip;
// host side: _tables.py).
//
// A launch walks a device array of descriptors -- zsv_adam_tensor, zsv_pair_tensor, zsv_accum_tensor: anything with `n` and
// `first_chunk` -- with one workgroup of 256 threads per chunk of CHUNK elements.  first_chunk of a descriptor is the running
// sum of ceil(n / CHUNK) over the descriptors before it, so workgroup `chunk` belongs to the last descriptor whose first_chunk
// is <= chunk.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace zsv {
constexpr int CHUNK = 4096;                           // the 4096 of include/zsv_hip.h, CHUNK of _tables.py

// index of the last descriptor whose first_chunk <= chunk
template <typename T> __device__ __forceinline__ int find_index(const T* __restrict__ table, int count, long chunk) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <typename T> __device__ __forceinline__ T find_tensor(const T* __restrict__ table, int count, long chunk) {
    return table[find_index(table, count, chunk)];
}

// elements [base, end) of its tensor are the chunk's; base >= end for a chunk past the tensor's end (a grid larger than the table)
struct Span {
    long base, end;
};
template <typename T> __device__ __forceinline__ Span chunk_span(const T& t, long chunk) {
    const long base = (chunk - t.first_chunk) * CHUNK;
    return Span{base, min((long)t.n, base + CHUNK)};
}

__device__ __forceinline__ bool non_finite(float g) { return !(fabsf(g) <= 3.402823466e38f); }     // inf or NaN

// may this array move 16 bytes per lane?  Asked at a chunk's base: a chunk is 16 KiB, so that is the alignment of the tensor.
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bool vec16(const void* p) {
#ifdef ZSV_SGD_SCALAR
    return false;                                     // A/B build: every array 4 bytes per lane (profiles/sgd_vector_ab.json)
#else
    return ((uintptr_t)p & 15u) == 0;
#endif
}

// ---- host: what every table-driven entry point refuses ----------------------------------------------------------------------
static inline bool bad_table(int32_t count, int64_t total_chunks) {
    return count <= 0 || total_chunks <= 0 || total_chunks > 0x7fffffffL;
}

static inline bool bad_rate(double x) { return !(x >= 0.0) || !isfinite(x); }                      // lr, weight decay, eps

}  // namespace zsv
