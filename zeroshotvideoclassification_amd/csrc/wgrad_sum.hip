// wgrad_sum.hip -- the ordered sums of the fp32 weight gradients' partial slabs (gfx950).
//
// Every fp32 weight-gradient kernel (conv_wgrad*.hip) writes one partial slab per slice of its voxel range; the sums here add
// the slabs in a FIXED order -- bitwise reproducible, no float atomics -- and write dw[co][ci][tap] in the weight tensor's own
// layout.  One kernel template holds the order of addition; a finisher per slab layout holds the decode of an element and what
// is done with its sums (a permuting store, or the output transform of a Winograd form and a store).
//
// wgrad_cl_reduce_kernel (wgrad_bf16.hip) looks like one more copy of this and is NOT: it keeps four accumulators per element
// and adds them as (s0 + s1) + (s2 + s3), a different order of addition with different bits.  It stays where it is.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_params.h"
#include "knobs.h"

namespace zsv {

// A block owns 32 consecutive slab elements (coalesced reads) x 8 slice groups: group g adds slices g, g+8, ... into ONE
// accumulator per point in that order, then the 8 partials are added in group order through LDS -- with 8x the loads in flight of
// a one-thread-per-element loop (the ~250 slices of a layer1 gradient made that loop latency-bound).  The loads of AHEAD slices
// are issued before their adds: the same order of addition, the same bits, but one HBM round trip per AHEAD slices (one slice at
// a time cost 86 us for the 512 slices of a layer1 gradient).  An element has POINTS values per slice, point p of slice k at
// slabs[(k * POINTS + p) * plane + j].
//
// Finish: `bool locate(j, at)` decodes element j ONCE (false: a padding element, nothing to add) and `store(dw, at, sums)` ends
// it; these kernels are mostly index arithmetic, so a finisher must not divide for the liveness test and again for the store.
template <int POINTS, int AHEAD, class Finish>
__global__ __launch_bounds__(256) void wgrad_sum_kernel(const float* __restrict__ slabs, float* __restrict__ dw, size_t plane,
                                                        int slices, Finish fin) {
    __shared__ float part[8][POINTS][32];
    const int e = threadIdx.x & 31, grp = threadIdx.x >> 5;
    for (size_t j0 = (size_t)blockIdx.x * 32; j0 < plane; j0 += (size_t)gridDim.x * 32) {
        const size_t j = j0 + e;
        typename Finish::At at;
        const bool live = j < plane && fin.locate(j, at);
        float s[POINTS];
#pragma unroll
        for (int p = 0; p < POINTS; ++p) s[p] = 0.f;
        if (live) {
            const float* src = slabs + j;
            int k = grp;
            if constexpr (AHEAD > 1) {
                for (; k + 8 * (AHEAD - 1) < slices; k += 8 * AHEAD) {
                    float v[AHEAD][POINTS];
#pragma unroll
                    for (int u = 0; u < AHEAD; ++u)
#pragma unroll
                        for (int p = 0; p < POINTS; ++p) v[u][p] = src[((size_t)(k + 8 * u) * POINTS + p) * plane];
#pragma unroll
                    for (int u = 0; u < AHEAD; ++u)
#pragma unroll
                        for (int p = 0; p < POINTS; ++p) s[p] += v[u][p];
                }
            }
            for (; k < slices; k += 8)
#pragma unroll
                for (int p = 0; p < POINTS; ++p) s[p] += src[((size_t)k * POINTS + p) * plane];
        }
#pragma unroll
        for (int p = 0; p < POINTS; ++p) part[grp][p][e] = s[p];
        __syncthreads();
        if (grp == 0 && live) {
            float t[POINTS];
#pragma unroll
            for (int p = 0; p < POINTS; ++p) {
                t[p] = part[0][p][e];
#pragma unroll
                for (int q = 1; q < 8; ++q) t[p] += part[q][p][e];
            }
            fin.store(dw, at, t);
        }
        __syncthreads();
    }
}

// ---- what is done with an element's sums: o[0..] = the taps the element stands for --------------------------------------------
__device__ __forceinline__ void emit(float* o, const float (&m)[1]) { o[0] = m[0]; }
__device__ __forceinline__ void emit(float* o, const float (&m)[4]) {                   // G^T of F(2,3)
    const float h = 0.5f * (m[1] + m[2]);
    o[0] = m[0] + h;
    o[1] = 0.5f * (m[1] - m[2]);
    o[2] = h - m[3];
}
__device__ __forceinline__ void emit(float* o, const float (&m)[6]) {                   // G^T of F(4,3)
    const float s12 = m[1] + m[2], d12 = m[2] - m[1], s34 = m[3] + m[4], d34 = m[3] - m[4];
    o[0] = 0.25f * m[0] - s12 * (1.f / 6.f) + s34 * (1.f / 24.f);
    o[1] = d12 * (1.f / 6.f) + d34 * (1.f / 12.f);
    o[2] = m[5] - s12 * (1.f / 6.f) + s34 * (1.f / 6.f);
}

// ---- the slab layouts ---------------------------------------------------------------------------------------------------------------
// [co][r * Cpad + ci], live iff ci < Cin: the staged and LDS-DMA kernels (1 point, r = tap) and the Winograd forms along W (4 or
// 6 points, r = the (kt, kh) row tap, three kw taps out of the transform)
template <int POINTS>
struct SumRows {
    int Cin, R, Cpad;
    struct At { size_t row; int ci; };
    __device__ bool locate(size_t j, At& at) const {
        at.row = j / Cpad;
        at.ci = (int)(j - at.row * Cpad);
        return at.ci < Cin;
    }
    __device__ void store(float* dw, const At& at, const float (&t)[POINTS]) const {
        const int r = (int)(at.row % R), co = (int)(at.row / R);
        emit(dw + (((size_t)co * Cin + at.ci) * R + r) * (POINTS == 1 ? 1 : 3), t);
    }
};
// the weight tensor's own layout: the generic kernel and the stem
struct SumFlat {
    struct At { size_t j; };
    __device__ bool locate(size_t j, At& at) const { at.j = j; return true; }
    __device__ void store(float* dw, const At& at, const float (&t)[1]) const { dw[at.j] = t[0]; }
};
// [ci][kt * M + co]: the temporal frame ring
struct SumRing {
    int M, Cin;
    struct At { size_t j; };
    __device__ bool locate(size_t j, At& at) const { at.j = j; return true; }
    __device__ void store(float* dw, const At& at, const float (&t)[1]) const {
        const int co = (int)(at.j % M);
        const size_t rr = at.j / M;
        const int kt = (int)(rr % 3), ci = (int)(rr / 3);
        dw[((size_t)co * Cin + ci) * 3 + kt] = t[0];
    }
};
// [point][ci][co]: the frame ring's Winograd form, three kt taps out of the transform
struct SumRingWino {
    int M, Cin;
    struct At { size_t j; };
    __device__ bool locate(size_t j, At& at) const { at.j = j; return true; }
    __device__ void store(float* dw, const At& at, const float (&t)[4]) const {
        const int co = (int)(at.j % M), ci = (int)(at.j / M);
        emit(dw + ((size_t)co * Cin + ci) * 3, t);
    }
};

template <int POINTS, int AHEAD, class Finish>
static int sum_launch(const float* slabs, float* dw, size_t plane, int slices, long max_blocks, Finish fin, hipStream_t stream) {
    long blocks = ((long)plane + 31) / 32;
    if (blocks > max_blocks) blocks = max_blocks;
    hipLaunchKernelGGL((wgrad_sum_kernel<POINTS, AHEAD, Finish>), dim3((unsigned)blocks), dim3(256), 0, stream, slabs, dw, plane,
                       slices, fin);
    return launch_status();
}

// The staged layout's sum for FEW slices and a large slab (the small-voxel layers: 2-4 slices of a 17-21 MB gradient): one block per
// output channel reads its [taps][Cpad] row of every slice with 16-byte loads (coalesced), adds the slices in order (up to 8
// slices that is also the group sum's order: the same bits) and writes dw[co][ci][tap] through an LDS
// transpose as whole contiguous rows (the group sum's 4-byte writes at stride `taps` made it run at 1 TB/s).
__global__ __launch_bounds__(256) void slab_sum_rows_kernel(const float* __restrict__ slabs, float* __restrict__ out,
                                                            int M, int Cin, int taps, int Cpad, int slices) {
    extern __shared__ __attribute__((aligned(16))) float row[];          // [taps][Cpad]
    const int co = blockIdx.x;
    const int len = taps * Cpad;                                        // (Cpad % 16 == 0: whole float4s)
    const size_t slab = (size_t)M * len;
    const float* src = slabs + (size_t)co * len;
    for (int i = 4 * (int)threadIdx.x; i < len; i += 1024) {
        f32x4 t = *reinterpret_cast<const f32x4*>(src + i);
        int k = 1;
        for (; k + 2 < slices; k += 3) {                          // three slices' loads in flight, added in the same order
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(src + (size_t)k * slab + i);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(src + (size_t)(k + 1) * slab + i);
            const f32x4 v2 = *reinterpret_cast<const f32x4*>(src + (size_t)(k + 2) * slab + i);
            t += v0; t += v1; t += v2;
        }
        for (; k < slices; ++k) t += *reinterpret_cast<const f32x4*>(src + (size_t)k * slab + i);
        *reinterpret_cast<f32x4*>(row + i) = t;
    }
    __syncthreads();
    float* dst = out + (size_t)co * Cin * taps;
    const int n = Cin * taps;
    for (int o = (int)threadIdx.x; o < n; o += 256) {
        const int ci = o / taps, tap = o - ci * taps;
        dst[o] = row[tap * Cpad + ci];
    }
}

// first level of a two-level flat sum: block row c adds slabs [c * per, (c + 1) * per) into part[c][i] (fixed order)
__global__ __launch_bounds__(256) void slab_sum_chunks_kernel(const float* __restrict__ slabs, float* __restrict__ part, long n, int slices,
                                                              int per) {
    const int c = blockIdx.y, k0 = c * per, k1 = min(slices, k0 + per);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        float s = 0.f;
        for (int k = k0; k < k1; ++k) s += slabs[(size_t)k * n + i];
        part[(size_t)c * n + i] = s;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// launches the sum that fits the geometry (same result bits either way)
int slab_sum(const float* slabs, float* dw, int M, int Cin, int taps, int Cpad, int slices, hipStream_t stream) {
    const size_t row_bytes = (size_t)taps * Cpad * sizeof(float);
    if (slices <= 32 && (long)M * slices <= 16384 && row_bytes <= 64 * 1024 && aligned16(slabs) && !ZSV_KNOB(NO_SLAB_SUM_ROWS)) {
        static const hipError_t attr = hipFuncSetAttribute((const void*)slab_sum_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
        if (attr != hipSuccess) return ZSV_E_LAUNCH;
        hipLaunchKernelGGL(slab_sum_rows_kernel, dim3((unsigned)M), dim3(256), row_bytes, stream, slabs, dw, M, Cin, taps, Cpad, slices);
        return launch_status();
    }
    return sum_launch<1, 4>(slabs, dw, (size_t)M * taps * Cpad, slices, 8192, SumRows<1>{Cin, taps, Cpad}, stream);
}

int slab_sum_flat(const float* slabs, float* dw, long n, int slices, hipStream_t stream) {
    return sum_launch<1, 1>(slabs, dw, (size_t)n, slices, 4096, SumFlat{}, stream);
}

// two levels, both in a fixed order: 32 chunks of slabs into `part`, then the 32 partial sums
int slab_sum_flat_chunked(const float* slabs, float* part, float* dw, long n, int slices, hipStream_t stream) {
    const int per = (slices + 31) / 32, chunks = (slices + per - 1) / per;
    hipLaunchKernelGGL(slab_sum_chunks_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)chunks), dim3(256), 0, stream, slabs, part, n,
                       slices, per);
    if (hipGetLastError() != hipSuccess) return ZSV_E_LAUNCH;
    return slab_sum_flat(part, dw, n, chunks, stream);
}

int wgrad_tring_sum(const float* slabs, float* dw, int M, int Cin, int slices, bool wino_form, hipStream_t stream) {
    if (wino_form) return sum_launch<4, 4>(slabs, dw, (size_t)Cin * M, slices, 8192, SumRingWino{M, Cin}, stream);
    return sum_launch<1, 4>(slabs, dw, (size_t)Cin * 3 * M, slices, 8192, SumRing{M, Cin}, stream);
}

int wgrad_wino_sum(const float* slabs, float* dw, int M, int Cin, int R, int Cpad, int slices, int points, hipStream_t stream) {
    const size_t plane = (size_t)M * R * Cpad;               // one point of one slice
    if (points == 6) return sum_launch<6, 2>(slabs, dw, plane, slices, 8192, SumRows<6>{Cin, R, Cpad}, stream);
    return sum_launch<4, 2>(slabs, dw, plane, slices, 8192, SumRows<4>{Cin, R, Cpad}, stream);
}

}  // namespace zsv
