// fp8_c3d.hip -- what the calibrated e4m3 engine of network.C3D needs next to the convolutions of conv_bf16.hip:
//   maxpool3d_fp8   nn.MaxPool3d (kernel == stride)   network.py:148-163 on channels-last e4m3
//   absmax_bf16     max |x| of a bf16 activation      the calibration pass (one static scale per layer)
// Both are HBM-bound single passes with 16-byte accesses.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zsv_hip.h"
#include "zsv_common.h"

namespace zsv {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// e4m3 codes are sign-magnitude: flipping the sign bit of a non-negative code and every bit of a negative one gives bytes that
// order, as unsigned integers, like the values (-448 = 0xFE -> 0x01 ... -0 = 0x80 -> 0x7F, +0 -> 0x80 ... +448 = 0x7E -> 0xFE).
// The map is its own inverse up to which bytes count as negative, four codes per register.
__device__ __forceinline__ unsigned e4m3_to_keys(unsigned v) { return v ^ ((((v >> 7) & 0x01010101u) * 0x7Fu) | 0x80808080u); }
__device__ __forceinline__ unsigned keys_to_e4m3(unsigned k) { return k ^ ((((~k >> 7) & 0x01010101u) * 0x7Fu) | 0x80808080u); }

__device__ __forceinline__ unsigned max_u8x4(unsigned a, unsigned b) {
    unsigned r = 0;
#pragma unroll
    for (int s = 0; s < 32; s += 8) r |= max((a >> s) & 0xFFu, (b >> s) & 0xFFu) << s;
    return r;
}

// One thread per (output voxel, 16 channels): 16-byte loads and one 16-byte store; taps outside the input are skipped (-inf
// padding; 2 * pad <= kernel, so every window holds an input voxel and the start key 0 never survives).  The maximum of e4m3
// values is one of them: the result is exact, no conversion to float.  Channels >= C are written as zero.
__global__ __launch_bounds__(256) void maxpool3d_fp8_kernel(const u32x4* __restrict__ x, int C, int Ti, int Hi, int Wi, int G, int kT,
                                                            int kH, int kW, int pT, int pH, int pW, int To, int Ho, int Wo, long total,
                                                            u32x4* __restrict__ y) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int o = (int)(idx % G);
    long r = idx / G;
    const int wo = (int)(r % Wo); r /= Wo;
    const int ho = (int)(r % Ho); r /= Ho;
    const int to = (int)(r % To);
    const long n = r / To;
    unsigned best[4] = {0u, 0u, 0u, 0u};
    for (int a = 0; a < kT; ++a) {
        const int t = to * kT + a - pT;
        if ((unsigned)t >= (unsigned)Ti) continue;
        for (int b = 0; b < kH; ++b) {
            const int h = ho * kH + b - pH;
            if ((unsigned)h >= (unsigned)Hi) continue;
            for (int c = 0; c < kW; ++c) {
                const int w = wo * kW + c - pW;
                if ((unsigned)w >= (unsigned)Wi) continue;
                const u32x4 v = x[(((n * Ti + t) * Hi + h) * (long)Wi + w) * G + o];
#pragma unroll
                for (int q = 0; q < 4; ++q) best[q] = max_u8x4(best[q], e4m3_to_keys(v[q]));
            }
        }
    }
    u32x4 out;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int live = C - (16 * o + 4 * q);                  // channels of this register below C
        const unsigned keep = live >= 4 ? 0xFFFFFFFFu : (live <= 0 ? 0u : (1u << (8 * live)) - 1u);
        out[q] = keys_to_e4m3(best[q]) & keep;
    }
    y[idx] = out;
}

// max |x| over bf16 values as the maximum of their 15 magnitude bits (|bf16| << 16 is the fp32 pattern of |x|, and patterns of
// non-negative floats order like integers; NaN patterns lie above inf and so win).  16-byte loads over the aligned middle,
// the < 8 elements in front of it and the < 8 behind it by the first workgroup; one integer atomic max per workgroup.
__global__ __launch_bounds__(256) void absmax_bf16_kernel(const unsigned short* __restrict__ x, long head, long nvec, long count,
                                                          unsigned* __restrict__ amax) {
    __shared__ unsigned part[4];
    unsigned m = 0;
    const u32x4* xv = reinterpret_cast<const u32x4*>(x + head);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long)gridDim.x * 256) {
        const u32x4 v = xv[i];
#pragma unroll
        for (int q = 0; q < 4; ++q) m = max(m, max(v[q] & 0x7FFFu, (v[q] >> 16) & 0x7FFFu));
    }
    if (blockIdx.x == 0) {
        const long tail = head + 8 * nvec;
        if ((long)threadIdx.x < head) m = max(m, (unsigned)x[threadIdx.x] & 0x7FFFu);
        if (tail + (long)threadIdx.x < count) m = max(m, (unsigned)x[tail + threadIdx.x] & 0x7FFFu);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = max(max(part[0], part[1]), max(part[2], part[3]));
        if (m != 0) atomicMax(amax, m << 16);
    }
}

}  // namespace zsv

using namespace zsv;

extern "C" {

int zsv_maxpool3d_fp8(const void* x, int32_t N, int32_t C, int32_t Ti, int32_t Hi, int32_t Wi, int32_t kT, int32_t kH, int32_t kW,
                      int32_t pT, int32_t pH, int32_t pW, int32_t To, int32_t Ho, int32_t Wo, void* y, void* stream) {
    if (N <= 0 || C <= 4 || Ti <= 0 || Hi <= 0 || Wi <= 0 || kT <= 0 || kH <= 0 || kW <= 0 || pT < 0 || pH < 0 || pW < 0)
        return ZSV_E_BAD_SHAPE;
    if (2 * pT > kT || 2 * pH > kH || 2 * pW > kW) return ZSV_E_BAD_SHAPE;            // (every window holds at least one input voxel)
    if (To != (Ti + 2 * pT - kT) / kT + 1 || Ho != (Hi + 2 * pH - kH) / kH + 1 || Wo != (Wi + 2 * pW - kW) / kW + 1 || To <= 0 ||
        Ho <= 0 || Wo <= 0)
        return ZSV_E_BAD_SHAPE;
    if (x == nullptr || y == nullptr) return ZSV_E_NULL;
    if (!aligned16(x, y)) return ZSV_E_UNSUPPORTED;
    const int G = zsv_fp8_channel_pitch(C) / 16;
    const long total = (long)N * To * Ho * Wo * G;
    if ((long)N * Ti * Hi * Wi * G >= (1L << 31)) return ZSV_E_TOO_LARGE;
    hipLaunchKernelGGL(maxpool3d_fp8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const u32x4*)x,
                       C, Ti, Hi, Wi, G, kT, kH, kW, pT, pH, pW, To, Ho, Wo, total, (u32x4*)y);
    return launch_status();
}

int zsv_absmax_bf16(const void* x, int64_t count, float* amax, void* stream) {
    if (count < 0) return ZSV_E_BAD_SHAPE;
    if (x == nullptr || amax == nullptr) return ZSV_E_NULL;
    if (count == 0) return ZSV_OK;
    if ((reinterpret_cast<uintptr_t>(x) & 1) != 0 || (reinterpret_cast<uintptr_t>(amax) & 3) != 0) return ZSV_E_UNSUPPORTED;
    long head = (long)(((16 - (reinterpret_cast<uintptr_t>(x) & 15)) & 15) / 2);      // elements in front of the 16-byte boundary
    if (head > count) head = count;
    const long nvec = (count - head) / 8;
    long blocks = (nvec + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(absmax_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)x, head,
                       nvec, (long)count, (unsigned*)amax);
    return launch_status();
}

}  // extern "C"
