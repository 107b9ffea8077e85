// softmax_xent.hip -- softmax cross-entropy over (N, C) fp32 logits with int64 labels, and the label's rank (gfx950).
//
// torch.nn.functional.cross_entropy(logits, labels, ignore_index=, label_smoothing=, reduction="mean" | "sum") without class
// weights, its gradient, and the top-1 / top-5 hit counts of the same logits, in three launches:
//
//   xent_row_kernel    : one 256-thread workgroup per row.  One pass over the row gives the running (max, sum of exp) pair of
//                        every thread (the online form: the sum is rescaled when the maximum moves, so every exponent is <= 0),
//                        the sum of the logits (label smoothing) and the number of classes ranked before the label; a second
//                        pass over the row, which the first left in cache, writes the unscaled gradient p - target.
//   xent_reduce_kernel : one workgroup: valid rows, top-1 hits, top-5 hits, and the summed (or mean) loss.
//   xent_bwd_kernel    : dx = dlogits * grad_loss / (mean ? valid : 1), grad_loss and valid read on the device.
//
// No atomics, no workspace.  Every sum has a fixed order: a thread adds its own elements in ascending order, a wave combines by
// the xor butterfly, the four waves are added in wave order.  Which elements a thread owns follows from the element's index in
// its row alone -- groups of four, group g to thread g mod 256 -- so a row that can be read 16 bytes at a time and one that
// cannot give the same bits; contraction of a * b + c into an fma is switched off for the file for the same reason (the
// compiler would otherwise be free to contract the two load forms differently).
#include "zsv_common.h"
#include "zsv_hip.h"

#include <math.h>

#pragma clang fp contract(off)

namespace zsv {

static const int kRankNever = 0x7fffffff;       // a row that counts as valid and can never be a hit

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// exp(x - m) for x <= m; 1 where x == m, which keeps a row with -inf logits finite (-inf - -inf is a NaN).
__device__ __forceinline__ float exp_below(float x, float m) { return x == m ? 1.0f : expf(x - m); }

// Elements [4 g, 4 g + 4) of a row of C; returns how many of them exist.  `vec`: the row starts on a 16-byte boundary.
__device__ __forceinline__ int load_group(const float* __restrict__ row, int C, int g, bool vec, float v[4]) {
    const int j = 4 * g;
    const int n = min(4, C - j);
    if (vec && n == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(row + j);
        v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
    } else {
        for (int i = 0; i < 4; ++i) v[i] = i < n ? row[j + i] : 0.0f;
    }
    return n;
}

__device__ __forceinline__ void fill_row(float* __restrict__ out, int C, float value) {
    const bool vec = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const int groups = (int)(((unsigned)C + 3u) >> 2);
    for (int g = threadIdx.x; g < groups; g += 256) {
        const int j = 4 * g;
        const int n = min(4, C - j);
        if (vec && n == 4) {
            const f32x4 q = {value, value, value, value};
            *reinterpret_cast<f32x4*>(out + j) = q;
        } else {
            for (int i = 0; i < n; ++i) out[j + i] = value;
        }
    }
}

__global__ __launch_bounds__(256) void xent_row_kernel(const float* __restrict__ logits, const int64_t* __restrict__ labels, int C,
                                                       float smooth, float keep, float smooth_each, int64_t ignore_index,
                                                       float* __restrict__ row_loss, int* __restrict__ row_rank,
                                                       float* __restrict__ dlogits) {
    __shared__ float red_m[4], red_s[4];
    __shared__ double red_x[4];
    __shared__ int red_r[4];
    const int r = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t label = labels[r];                                    // (uniform over the workgroup)
    float* __restrict__ drow = dlogits ? dlogits + (size_t)r * C : nullptr;
    if (label == ignore_index || label < 0 || label >= C) {
        // an ignored row contributes nothing; any other label outside [0, C) poisons its own row.  The logits are not read.
        const bool ignored = label == ignore_index;
        const float value = ignored ? 0.0f : __builtin_nanf("");
        if (threadIdx.x == 0) {
            row_loss[r] = value;
            row_rank[r] = ignored ? -1 : kRankNever;
        }
        if (drow) fill_row(drow, C, value);
        return;
    }
    const int y = (int)label;
    const float* __restrict__ row = logits + (size_t)r * C;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const int groups = (int)(((unsigned)C + 3u) >> 2);
    const float xy = row[y];

    float m = -__builtin_huge_valf(), s = 0.0f;
    double sum_x = 0.0;
    int before = 0;
    float v[4];
    for (int g = threadIdx.x; g < groups; g += 256) {
        const int n = load_group(row, C, g, vec, v);
        float gm = v[0];
        for (int i = 1; i < 4; ++i)
            if (i < n) gm = fmaxf(gm, v[i]);
        if (gm > m) {
            s = s * exp_below(m, gm);
            m = gm;
        }
        for (int i = 0; i < 4; ++i) {
            if (i < n) {
                const float x = v[i];
                s = s + exp_below(x, m);
                sum_x += (double)x;
                before += (x > xy || (x == xy && 4 * g + i < y)) ? 1 : 0;
            }
        }
    }
    // the row maximum (exact, whatever the order)
    const float wm = wave_max(m);
    if (lane == 0) red_m[wave] = wm;
    __syncthreads();
    const float M = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
    // every thread's sum brought to that maximum, then added: lanes by the butterfly, waves in order
    const float ws = wave_sum(s * exp_below(m, M));
    const double wx = wave_sum(sum_x);
    const int wr = wave_sum(before);
    if (lane == 0) {
        red_s[wave] = ws;
        red_x[wave] = wx;
        red_r[wave] = wr;
    }
    __syncthreads();
    const float S = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
    if (threadIdx.x == 0) {
        const double total_x = ((red_x[0] + red_x[1]) + red_x[2]) + red_x[3];
        const float mean_x = (float)(total_x / (double)C);
        const float lse = M + logf(S);
        row_loss[r] = keep * (lse - xy) + smooth * (lse - mean_x);
        // a NaN at the label compares false with everything: it would rank first
        row_rank[r] = xy != xy ? kRankNever : ((red_r[0] + red_r[1]) + red_r[2]) + red_r[3];
    }
    if (!drow) return;
    const float inv_s = 1.0f / S;
    const bool vec_out = (reinterpret_cast<uintptr_t>(drow) & 15) == 0;
    for (int g = threadIdx.x; g < groups; g += 256) {
        const int n = load_group(row, C, g, vec, v);
        float d[4];
        for (int i = 0; i < 4; ++i) {
            const float target = (i < n && 4 * g + i == y) ? keep + smooth_each : smooth_each;
            d[i] = exp_below(v[i], M) * inv_s - target;
        }
        if (vec_out && n == 4) {
            const f32x4 q = {d[0], d[1], d[2], d[3]};
            *reinterpret_cast<f32x4*>(drow + 4 * g) = q;
        } else {
            for (int i = 0; i < n; ++i) drow[4 * g + i] = d[i];
        }
    }
}

__global__ __launch_bounds__(256) void xent_reduce_kernel(const float* __restrict__ row_loss, const int* __restrict__ row_rank, int N,
                                                          int mean, float* __restrict__ loss, int* __restrict__ counts) {
    __shared__ double red_l[4];
    __shared__ int red_c[3][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double total = 0.0;
    int valid = 0, top1 = 0, top5 = 0;
    for (int r = threadIdx.x; r < N; r += 256) {
        const int rank = row_rank[r];
        if (rank < 0) continue;                                         // ignored
        valid += 1;
        top1 += rank == 0 ? 1 : 0;
        top5 += rank < 5 ? 1 : 0;
        total += (double)row_loss[r];
    }
    total = wave_sum(total);
    valid = wave_sum(valid);
    top1 = wave_sum(top1);
    top5 = wave_sum(top5);
    if (lane == 0) {
        red_l[wave] = total;
        red_c[0][wave] = valid;
        red_c[1][wave] = top1;
        red_c[2][wave] = top5;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sum = ((red_l[0] + red_l[1]) + red_l[2]) + red_l[3];
        int c[3];
        for (int i = 0; i < 3; ++i) c[i] = ((red_c[i][0] + red_c[i][1]) + red_c[i][2]) + red_c[i][3];
        counts[0] = c[0];
        counts[1] = c[1];
        counts[2] = c[2];
        // every row ignored: 0, where torch divides 0 by 0
        loss[0] = mean ? (c[0] > 0 ? (float)(sum / (double)c[0]) : 0.0f) : (float)sum;
    }
}

__global__ __launch_bounds__(256) void xent_bwd_kernel(const float* dlogits, const float* __restrict__ grad_loss,
                                                       const int* __restrict__ counts, int mean, int total, float* dx, int vec) {
    float g = grad_loss[0];
    if (mean) {
        const int valid = counts[0];
        g = g / (float)(valid > 1 ? valid : 1);
    }
    const int tid = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    if (vec) {
        const int quads = total >> 2;
        for (int q = tid; q < quads; q += stride) {
            f32x4 a = reinterpret_cast<const f32x4*>(dlogits)[q];
            a[0] = a[0] * g; a[1] = a[1] * g; a[2] = a[2] * g; a[3] = a[3] * g;
            reinterpret_cast<f32x4*>(dx)[q] = a;
        }
        for (int i = 4 * quads + tid; i < total; i += stride) dx[i] = dlogits[i] * g;
    } else {
        for (int i = tid; i < total; i += stride) dx[i] = dlogits[i] * g;
    }
}

}  // namespace zsv

static int xent_shape_status(int32_t N, int32_t C) {
    if (N <= 0 || C <= 0) return ZSV_E_BAD_SHAPE;
    if ((double)N * (double)C >= 2147483648.0) return ZSV_E_TOO_LARGE;
    return ZSV_OK;
}

extern "C" int zsv_softmax_xent_fwd(const float* logits, const int64_t* labels, int32_t N, int32_t C, double label_smoothing,
                                    int64_t ignore_index, float* row_loss, int32_t* row_rank, float* dlogits, void* stream_) {
    if (!logits || !labels || !row_loss || !row_rank) return ZSV_E_NULL;
    if (!(label_smoothing >= 0.0 && label_smoothing < 1.0)) return ZSV_E_BAD_SHAPE;
    const int st = xent_shape_status(N, C);
    if (st) return st;
    hipLaunchKernelGGL(zsv::xent_row_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream_, logits, labels, C, (float)label_smoothing,
                       (float)(1.0 - label_smoothing), (float)(label_smoothing / (double)C), ignore_index, row_loss, row_rank,
                       dlogits);
    return zsv::launch_status();
}

extern "C" int zsv_softmax_xent_reduce(const float* row_loss, const int32_t* row_rank, int32_t N, int32_t mean, float* loss,
                                       int32_t* counts, void* stream_) {
    if (!row_loss || !row_rank || !loss || !counts) return ZSV_E_NULL;
    if (N <= 0) return ZSV_E_BAD_SHAPE;
    hipLaunchKernelGGL(zsv::xent_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream_, row_loss, row_rank, N, mean ? 1 : 0, loss,
                       counts);
    return zsv::launch_status();
}

extern "C" int zsv_softmax_xent_bwd(const float* dlogits, const float* grad_loss, const int32_t* counts, int32_t mean, int32_t N,
                                    int32_t C, float* dx, void* stream_) {
    if (!dlogits || !grad_loss || !counts || !dx) return ZSV_E_NULL;
    const int st = xent_shape_status(N, C);
    if (st) return st;
    const int total = N * C;
    const int vec = zsv::aligned16(dlogits, dx) ? 1 : 0;
    const int work = vec ? (total + 3) / 4 : total;
    const int blocks = (work + 255) / 256 < 2048 ? (work + 255) / 256 : 2048;
    hipLaunchKernelGGL(zsv::xent_bwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream_, dlogits, grad_loss, counts, mean ? 1 : 0,
                       total, dx, vec);
    return zsv::launch_status();
}
