// batchnorm.hip -- BatchNorm3d forward/backward (+ fused residual add and ReLU), gfx950.
//
// Supplies aten::native_batch_norm / native_batch_norm_backward for every
// nn.BatchNorm3d of the reference (resnet.py:48,95,97,183,186,272), with the
// `out += residual; relu(out)` of BasicBlock.forward (resnet.py:110-111) and the ReLU of
// Conv2Plus1D / stems (resnet.py:49,95,184,187) fused into the same HBM pass.
//
// These are HBM-bound passes over (N, C, S) fp32 tensors (S = T*H*W contiguous):
//   stats   : one read of x            -> per (channel, slice) partial (sum, sumsq)
//   finalize: C threads                -> mean, invstd, scale/shift, running stats
//   apply   : read x (+res), write y   -> float4 along S when S % 4 == 0
//   bwd     : reduce (read dy, x, y) + apply (read dy, x, y; write dx (+dres))
//   bwd_eval: one pass (read dy, x or y; write dx (+dres)) + a C-wave finalize of dgamma / dbeta
//   sync    : the same passes with batch statistics over all ranks (zsv_bn_sync_*): stats -> per-rank moments | all_gather |
//             Chan merge in rank order -> apply;  bwd reduce -> local sums | all_reduce | apply.  The collectives run in the caller.
// Per-thread partial sums are fp32 over <= ~128 elements, combined in fp64 with
// wave-level shuffles (64-wide) and a 4-entry LDS exchange; the slices of a channel are
// summed in fixed order, so results are bitwise reproducible run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include "zsv_hip.h"
#include "zsv_common.h"
#include "knobs.h"

namespace zsv {

// Streaming accesses with the non-temporal hint (`nt`, wave-uniform): the big activation tensors are read once per pass, and their
// lines only push out what the kernels running next to these passes still need (the side queue's weight-gradient kernels and
// their weight panels).  Threshold sweep inside the training step (one device, two rounds each): off 39.06 / 39.13 ms, 200 MB
// 38.87 / 38.89, 100 MB 38.88 / 38.87 (38.78 / 38.76 on another device), 30 MB 38.79 / 38.78, every tensor 38.83 / 38.84.
typedef float bn_v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const float* p, bool nt) {
    if (nt) {
        const bn_v4f v = __builtin_nontemporal_load(reinterpret_cast<const bn_v4f*>(p));
        return make_float4(v[0], v[1], v[2], v[3]);
    }
    return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ void st4(float* p, const float4& v, bool nt) {
    if (nt) {
        const bn_v4f w = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(w, reinterpret_cast<bn_v4f*>(p));
    } else {
        *reinterpret_cast<float4*>(p) = v;
    }
}
// bytes of ONE tensor of the pass above which its accesses are streamed (ZSV_BN_NT_MB: default 64; 0 = never)
static inline bool bn_stream(int N, int C, int S) {
    const char* e = ZSV_KNOB(BN_NT_MB);
    const double mb = e ? atof(e) : 64.0;
    return mb > 0.0 && (double)N * C * S * 4.0 > mb * 1e6;
}


// slices per channel so that every channel has enough workgroups in flight and a thread
// accumulates a bounded number of fp32 terms
static inline int bn_slices(int N, int C, int S) {
    const long per_channel = (long)N * S;
    long want = (2048 + C - 1) / C;                 // ~8 workgroups per CU overall
    long by_len = (per_channel + 256L * 128 - 1) / (256L * 128);   // <= 128 terms per thread
    long s = want > by_len ? want : by_len;
    long max_s = (per_channel + 1023) / 1024;       // at least 1024 elements per slice
    if (max_s < 1) max_s = 1;
    if (s > max_s) s = max_s;
    if (s < 1) s = 1;
    if (s > 4096) s = 4096;
    return (int)s;
}

// workspace layout: double part[2][C][slices] | float scale[C] | float shift[C] | float c1[C] | float c2[C]
struct BnWs {
    double* part;
    float* scale;
    float* shift;
    float* c1;
    float* c2;
};
static inline size_t bn_ws_bytes(int N, int C, int S) {
    const int sl = bn_slices(N, C, S);
    return (size_t)2 * C * sl * sizeof(double) + (size_t)4 * C * sizeof(float);
}
static inline BnWs bn_ws(void* ws, int C, int slices) {
    BnWs w;
    w.part = (double*)ws;
    w.scale = (float*)(w.part + (size_t)2 * C * slices);
    w.shift = w.scale + C;
    w.c1 = w.shift + C;
    w.c2 = w.c1 + C;
    return w;
}

// The (n, s) domain of one channel is N*S elements; slice `sl` owns the contiguous range
// [sl*len, (sl+1)*len) of it, len a multiple of 4 when S % 4 == 0.
__device__ __forceinline__ void slice_range(int total, int slices, int sl, bool vec, int& b, int& e) {
    int len = (total + slices - 1) / slices;
    if (vec) len = (len + 3) & ~3;
    const long bl = (long)sl * len;
    b = bl > total ? total : (int)bl;
    e = (total - b < len) ? total : b + len;
}

// ---- per-element arithmetic shared by the plain and the synchronised (zsv_bn_sync_*) passes ---------------------------------
// the normalise fma
__device__ __forceinline__ float bn_norm(float v, float sc, float sh) { return __fmaf_rn(v, sc, sh); }
__device__ __forceinline__ void bn_norm4(float4& v, float sc, float sh) {
    v.x = __fmaf_rn(v.x, sc, sh); v.y = __fmaf_rn(v.y, sc, sh); v.z = __fmaf_rn(v.z, sc, sh); v.w = __fmaf_rn(v.w, sc, sh);
}
// the training forward's scale / shift of channel c from the saved statistics: bn_finalize_train_kernel's expressions (its scale
// is gamma * invstd in fp32), so a mask recomputed with them has the forward's sign bit for bit
__device__ __forceinline__ void train_coeff(int c, const float* __restrict__ gamma, const float* __restrict__ beta,
                                            const float* __restrict__ mean, const float* __restrict__ invstd, float& sc, float& sh) {
    sc = (gamma ? gamma[c] : 1.f) * invstd[c];
    sh = __fmaf_rn(-mean[c], sc, beta ? beta[c] : 0.f);
}
// g = dy * mask.  RELU: 0 no mask; 1 mask = (saved output y > 0); 2 mask = (x*scale + shift > 0), the pre-activation recomputed
// with the forward's exact fma
template <int RELU>
__device__ __forceinline__ float bn_mask(float g, float xv, float yv, float sc, float sh) {
    if (RELU == 1) return yv > 0.f ? g : 0.f;
    if (RELU == 2) return bn_norm(xv, sc, sh) > 0.f ? g : 0.f;
    return g;
}
template <int RELU>
__device__ __forceinline__ void bn_mask4(float4& g, const float4& xv, const float4& yv, float sc, float sh) {
    if (RELU == 1) {
        g.x = yv.x > 0.f ? g.x : 0.f; g.y = yv.y > 0.f ? g.y : 0.f;
        g.z = yv.z > 0.f ? g.z : 0.f; g.w = yv.w > 0.f ? g.w : 0.f;
    } else if (RELU == 2) {
        g.x = bn_norm(xv.x, sc, sh) > 0.f ? g.x : 0.f; g.y = bn_norm(xv.y, sc, sh) > 0.f ? g.y : 0.f;
        g.z = bn_norm(xv.z, sc, sh) > 0.f ? g.z : 0.f; g.w = bn_norm(xv.w, sc, sh) > 0.f ? g.w : 0.f;
    }
}
// Shifted sums of one thread over the slice [b, e) of channel c: a sample of the channel is the pivot K, so
// sum (x-K)^2 - (sum (x-K))^2 / n does not cancel when |mean| >> std (biased convolutions, post-ReLU features); x - K is exact
// or 1-ulp in fp32.
__device__ __forceinline__ void pivot_sums(const float* __restrict__ x, int C, int S, int c, int b, int e, bool vec, float K,
                                           float& s1, float& s2) {
    if (vec) {
        for (int i = b + 4 * (int)threadIdx.x; i < e; i += 4 * 256) {
            const int n = i / S, s = i - n * S;
            float4 v = *reinterpret_cast<const float4*>(x + ((size_t)n * C + c) * S + s);
            v.x -= K; v.y -= K; v.z -= K; v.w -= K;
            s1 += (v.x + v.y) + (v.z + v.w);
            s2 += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        }
    } else {
        for (int i = b + (int)threadIdx.x; i < e; i += 256) {
            const int n = i / S, s = i - n * S;
            const float v = x[((size_t)n * C + c) * S + s] - K;
            s1 += v;
            s2 += v * v;
        }
    }
}
// the backward's coefficients of one channel from sum g, sum g*xhat and the element count M (all three the WHOLE batch's):
// dx = a*g + b*x + k  with  a = gamma*invstd, b = -a*invstd*sgx/M, k = -a*sg/M - b*mean
__device__ __forceinline__ void bwd_coeff(double g, double is, double mu, double sg, double sgx, double count, float& ca, float& cb,
                                          float& ck) {
    const double a = g * is;
    const double b = -a * is * sgx / count;
    const double k = -a * sg / count - b * mu;
    ca = (float)a;
    cb = (float)b;
    ck = (float)k;
}

// ---- forward statistics ------------------------------------------------------------
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ x, int N, int C, int S, int slices,
                                                       double* __restrict__ part) {
    __shared__ double red[4];
    const int c = blockIdx.x, sl = blockIdx.y;
    const bool vec = (S % 4) == 0;
    int b, e;
    slice_range(N * S, slices, sl, vec, b, e);
    const float K = x[(size_t)c * S];              // the pivot of pivot_sums
    float s1 = 0.f, s2 = 0.f;
    pivot_sums(x, C, S, c, b, e, vec, K, s1, s2);
    const double t1 = block_sum_256<double>((double)s1, red);
    const double t2 = block_sum_256<double>((double)s2, red);
    if (threadIdx.x == 0) {
        part[(size_t)c * slices + sl] = t1;
        part[(size_t)(C + c) * slices + sl] = t2;
    }
}

// `pivot_src` (may be null = pivot 0): the tensor bn_stats_kernel shifted by x[c * S]; the partial sums are then
// sums of (x - K) and (x - K)^2.
__global__ void bn_finalize_train_kernel(const double* __restrict__ part, int C, int slices, double count,
                                         const float* __restrict__ pivot_src, int S,
                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                         float* __restrict__ save_mean, float* __restrict__ save_invstd,
                                         float* __restrict__ running_mean, float* __restrict__ running_var,
                                         float momentum, float eps, float* __restrict__ scale,
                                         float* __restrict__ shift) {
    const int c = blockIdx.x;                      // one 64-lane wave per channel (as bn_bwd_finalize_kernel)
    double s1 = 0.0, s2 = 0.0;
    for (int k = threadIdx.x; k < slices; k += 64) {
        s1 += part[(size_t)c * slices + k];
        s2 += part[(size_t)(C + c) * slices + k];
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (threadIdx.x != 0) return;
    const double K = pivot_src ? (double)pivot_src[(size_t)c * S] : 0.0;
    const double dmean = s1 / count;                 // mean - K
    const double mean = K + dmean;
    double var = s2 / count - dmean * dmean;
    if (var < 0.0) var = 0.0;
    const double invstd = 1.0 / sqrt(var + (double)eps);
    save_mean[c] = (float)mean;
    save_invstd[c] = (float)invstd;
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    if (running_var) {
        const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
    }
    const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
    const float sc = g * (float)invstd;
    scale[c] = sc;
    shift[c] = __fmaf_rn(-(float)mean, sc, bt);      // (the backward recomputes exactly this)
}

// Statistics from the producing convolution's epilogue partials ([C][tiles] sums and [C][tiles] sums of squares, fp32) and the
// finalisation in ONE launch (a block per channel): a double-precision block sum in a fixed order, then exactly
// bn_finalize_train_kernel's arithmetic with pivot 0.
__global__ __launch_bounds__(256) void bn_finalize_partials_kernel(const float* __restrict__ psum, const float* __restrict__ psq,
                                                                   int C, int tiles, double count, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float* __restrict__ save_mean,
                                                                   float* __restrict__ save_invstd, float* __restrict__ running_mean,
                                                                   float* __restrict__ running_var, float momentum, float eps,
                                                                   float* __restrict__ scale, float* __restrict__ shift) {
    __shared__ double red[4];
    const int c = blockIdx.x;
    double a1 = 0.0, a2 = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 256) {
        a1 += (double)psum[(size_t)c * tiles + t];
        a2 += (double)psq[(size_t)c * tiles + t];
    }
    const double s1 = block_sum_256<double>(a1, red);
    const double s2 = block_sum_256<double>(a2, red);
    if (threadIdx.x != 0) return;
    const double mean = s1 / count;
    double var = s2 / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const double invstd = 1.0 / sqrt(var + (double)eps);
    save_mean[c] = (float)mean;
    save_invstd[c] = (float)invstd;
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    if (running_var) {
        const double unbiased = count > 1.0 ? var * count / (count - 1.0) : var;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
    }
    const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
    const float sc = g * (float)invstd;
    scale[c] = sc;
    shift[c] = __fmaf_rn(-(float)mean, sc, bt);
}

// Running-statistics affine of channel c: y = x * sc + sh, sc = gamma / sqrt(rv + eps), sh = beta - rm * sc (one fma).  Every
// eval-mode pass (forward, folded-convolution coefficients, backward masks) takes its coefficients from here: the same bits.
__device__ __forceinline__ void eval_coeff(int c, const float* __restrict__ gamma, const float* __restrict__ beta,
                                           const float* __restrict__ rm, const float* __restrict__ rv, float eps, float& invstd,
                                           float& sc, float& sh) {
    invstd = 1.f / sqrtf(rv[c] + eps);
    const float g = gamma ? gamma[c] : 1.f, bt = beta ? beta[c] : 0.f;
    sc = g * invstd;
    sh = __fmaf_rn(-rm[c], sc, bt);
}

__global__ void bn_eval_coeff_kernel(int C, const float* __restrict__ gamma, const float* __restrict__ beta,
                                     const float* __restrict__ rm, const float* __restrict__ rv, float eps,
                                     float* __restrict__ scale, float* __restrict__ shift) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float invstd, sc, sh;
    eval_coeff(c, gamma, beta, rm, rv, eps, invstd, sc, sh);
    scale[c] = sc;
    shift[c] = sh;
}

// coef = [2][pitch] (scale row, shift row) of a frozen BatchNorm for zsv_conv3d_fwd_pre / zsv_conv3d_wgrad_pre; tail entries 0
__global__ void bn_eval_coef_rows_kernel(int C, int pitch, const float* __restrict__ gamma, const float* __restrict__ beta,
                                         const float* __restrict__ rm, const float* __restrict__ rv, float eps,
                                         float* __restrict__ coef) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= pitch) return;
    float invstd = 0.f, sc = 0.f, sh = 0.f;
    if (c < C) eval_coeff(c, gamma, beta, rm, rv, eps, invstd, sc, sh);
    coef[c] = sc;
    coef[pitch + c] = sh;
}

// ---- y = relu?(x*scale[c] + shift[c] + res?) ------------------------------------------
// grid.x = row (n*C + c), grid.y = chunk of the row; 256 threads x 16 elements per chunk.
constexpr int ROW_CHUNK = 4096;

// one chunk [s0, s1) of the row at `base` (shared with bn_sync_apply_kernel)
template <bool RES, bool RELU>
__device__ __forceinline__ void apply_chunk(const float* __restrict__ x, const float* __restrict__ res, float* __restrict__ y,
                                            size_t base, int s0, int s1, int S, float sc, float sh, bool nt) {
    if ((S % 4) == 0 && s1 - s0 == ROW_CHUNK) {
        // full chunk: all 4 (8 with a residual) 16-byte loads of a thread are issued before the first use
        float4 v[4], r[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = ld4(x + base + s0 + 4 * threadIdx.x + 1024 * i, nt);
        if (RES) {
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = ld4(res + base + s0 + 4 * threadIdx.x + 1024 * i, nt);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            bn_norm4(v[i], sc, sh);
            if (RES) { v[i].x += r[i].x; v[i].y += r[i].y; v[i].z += r[i].z; v[i].w += r[i].w; }
            if (RELU) { v[i].x = fmaxf(v[i].x, 0.f); v[i].y = fmaxf(v[i].y, 0.f); v[i].z = fmaxf(v[i].z, 0.f); v[i].w = fmaxf(v[i].w, 0.f); }
            st4(y + base + s0 + 4 * threadIdx.x + 1024 * i, v[i], nt);
        }
    } else if ((S % 4) == 0) {
        for (int s = s0 + 4 * threadIdx.x; s < s1; s += 1024) {
            float4 v = *reinterpret_cast<const float4*>(x + base + s);
            bn_norm4(v, sc, sh);
            if (RES) {
                const float4 r = *reinterpret_cast<const float4*>(res + base + s);
                v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
            }
            if (RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            *reinterpret_cast<float4*>(y + base + s) = v;
        }
    } else {
        for (int s = s0 + threadIdx.x; s < s1; s += 256) {
            float v = bn_norm(x[base + s], sc, sh);
            if (RES) v += res[base + s];
            if (RELU) v = fmaxf(v, 0.f);
            y[base + s] = v;
        }
    }
}

template <bool RES, bool RELU>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                       float* __restrict__ y, int C, int S,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift, bool nt) {
    const int row = blockIdx.x;
    const int c = row % C;
    const float sc = scale[c], sh = shift[c];
    const int s0 = blockIdx.y * ROW_CHUNK;
    apply_chunk<RES, RELU>(x, res, y, (size_t)row * S, s0, min(S, s0 + ROW_CHUNK), S, sc, sh, nt);
}

// the same pass with scale / shift formed from the saved statistics (zsv_bn_sync_apply: they arrive after the collective)
template <bool RES, bool RELU>
__global__ __launch_bounds__(256) void bn_sync_apply_kernel(const float* __restrict__ x, const float* __restrict__ res,
                                                            float* __restrict__ y, int C, int S, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, bool nt) {
    const int row = blockIdx.x;
    float sc, sh;
    train_coeff(row % C, gamma, beta, mean, invstd, sc, sh);
    const int s0 = blockIdx.y * ROW_CHUNK;
    apply_chunk<RES, RELU>(x, res, y, (size_t)row * S, s0, min(S, s0 + ROW_CHUNK), S, sc, sh, nt);
}

// ---- backward reduce: sum g, sum g*xhat with g = dy * mask ------------------------------
// RELU: 0 no mask; 1 mask = (saved output y > 0); 2 mask = (x*scale + shift > 0), i.e. the
// pre-activation recomputed with the forward's exact fma -- saves reading y when the forward
// had no residual input.
// one thread's share of the slice [b, e) of channel c (shared with zsv_bn_sync_bwd_reduce, which launches the same kernel)
template <int RELU>
__device__ __forceinline__ void reduce_slice(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y,
                                             int C, int S, int c, int b, int e, bool vec, float mu, float is, float sc, float sh,
                                             float* __restrict__ gout, bool nt, float& s1, float& s2) {
    if (vec) {
        for (int i = b + 4 * (int)threadIdx.x; i < e; i += 4 * 256) {
            const int n = i / S, s = i - n * S;
            const size_t off = ((size_t)n * C + c) * S + s;
            float4 g = ld4(dy + off, nt);
            const float4 xv = ld4(x + off, nt);
            float4 yv;
            if (RELU == 1) yv = ld4(y + off, nt);
            bn_mask4<RELU>(g, xv, yv, sc, sh);
            if (RELU == 1 && gout) *reinterpret_cast<float4*>(gout + off) = g;
            s1 += (g.x + g.y) + (g.z + g.w);
            s2 += (g.x * ((xv.x - mu) * is) + g.y * ((xv.y - mu) * is)) +
                  (g.z * ((xv.z - mu) * is) + g.w * ((xv.w - mu) * is));
        }
    } else {
        for (int i = b + (int)threadIdx.x; i < e; i += 256) {
            const int n = i / S, s = i - n * S;
            const size_t off = ((size_t)n * C + c) * S + s;
            const float g = bn_mask<RELU>(dy[off], RELU == 2 ? x[off] : 0.f, RELU == 1 ? y[off] : 0.f, sc, sh);
            if (RELU == 1 && gout) gout[off] = g;
            s1 += g;
            s2 += g * ((x[off] - mu) * is);
        }
    }
}

template <int RELU>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ y, int N, int C, int S,
                                                            int slices, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            double* __restrict__ part, float* __restrict__ gout, bool nt) {
    // gout != nullptr (RELU 1 with a residual branch): the masked gradient g = dy * (y > 0) is written here -- it IS the gradient of
    // the residual branch -- and the apply pass then reads g alone instead of dy and y again (8 -> 7 passes over the tensor)
    __shared__ double red[4];
    const int c = blockIdx.x, sl = blockIdx.y;
    const bool vec = (S % 4) == 0;
    int b, e;
    slice_range(N * S, slices, sl, vec, b, e);
    const float mu = mean[c], is = invstd[c];
    float sc, sh;
    train_coeff(c, gamma, beta, mean, invstd, sc, sh);
    float s1 = 0.f, s2 = 0.f;
    reduce_slice<RELU>(dy, x, y, C, S, c, b, e, vec, mu, is, sc, sh, gout, nt, s1, s2);
    const double t1 = block_sum_256<double>((double)s1, red);
    const double t2 = block_sum_256<double>((double)s2, red);
    if (threadIdx.x == 0) {
        part[(size_t)c * slices + sl] = t1;
        part[(size_t)(C + c) * slices + sl] = t2;
    }
}

// dgamma = sum g*xhat, dbeta = sum g;  dx = a*g + b*x + k  with
//   a = gamma*invstd, b = -a*invstd*dgamma/M, k = -a*dbeta/M - b*mean
__global__ void bn_bwd_finalize_kernel(const double* __restrict__ part, int C, int slices, double count,
                                       const float* __restrict__ gamma, const float* __restrict__ mean,
                                       const float* __restrict__ invstd, float* __restrict__ dgamma,
                                       float* __restrict__ dbeta, float* __restrict__ ca, float* __restrict__ cb,
                                       float* __restrict__ ck, const float* __restrict__ beta,
                                       float* __restrict__ csh) {
    // one 64-lane wave per channel: lane l adds slices l, l + 64, ... in order, then the lanes are combined by xor-shuffles -- a
    // fixed order (bitwise reproducible); a single thread walking up to ~35 slices with dependent adds took 16 us per launch,
    // 37 launches per step on the backward's critical path
    const int c = blockIdx.x;
    double sg = 0.0, sgx = 0.0;
    for (int k = threadIdx.x; k < slices; k += 64) {
        sg += part[(size_t)c * slices + k];
        sgx += part[(size_t)(C + c) * slices + k];
    }
    sg = wave_sum(sg);
    sgx = wave_sum(sgx);
    if (threadIdx.x != 0) return;
    if (dgamma) dgamma[c] = (float)sgx;
    if (dbeta) dbeta[c] = (float)sg;
    bwd_coeff(gamma ? (double)gamma[c] : 1.0, (double)invstd[c], (double)mean[c], sg, sgx, count, ca[c], cb[c], ck[c]);
    // forward's shift, recomputed with the forward's exact arithmetic (its scale is gamma*invstd in fp32)
    float sc;
    train_coeff(c, gamma, beta, mean, invstd, sc, csh[c]);
}

// one chunk [s0, s1) of the row at `base` (shared with bn_sync_bwd_apply_kernel): g = dy * mask, d_residual = g, dx = a*g + b*x + k
template <int RELU, bool DRES>
__device__ __forceinline__ void bwd_apply_chunk(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y,
                                                float* __restrict__ dx, float* __restrict__ dres, size_t base, int s0, int s1, int S,
                                                float a, float b, float k, float sc, float sh, bool nt) {
    if ((S % 4) == 0 && s1 - s0 == ROW_CHUNK) {
        // full chunk: the 8 (12 with a saved-output mask) 16-byte loads of a thread are issued up front
        float4 gv[4], xq[4], yq[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            gv[i] = ld4(dy + base + s0 + 4 * threadIdx.x + 1024 * i, nt);
            xq[i] = ld4(x + base + s0 + 4 * threadIdx.x + 1024 * i, nt);
            if (RELU == 1) yq[i] = ld4(y + base + s0 + 4 * threadIdx.x + 1024 * i, nt);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float4 g = gv[i];
            const float4 xv = xq[i];
            const int s = s0 + 4 * threadIdx.x + 1024 * i;
            bn_mask4<RELU>(g, xv, yq[i], sc, sh);
            if (DRES) st4(dres + base + s, g, nt);
            float4 o;
            o.x = a * g.x + b * xv.x + k; o.y = a * g.y + b * xv.y + k;
            o.z = a * g.z + b * xv.z + k; o.w = a * g.w + b * xv.w + k;
            st4(dx + base + s, o, nt);
        }
    } else if ((S % 4) == 0) {
        for (int s = s0 + 4 * threadIdx.x; s < s1; s += 1024) {
            float4 g = *reinterpret_cast<const float4*>(dy + base + s);
            const float4 xv = *reinterpret_cast<const float4*>(x + base + s);
            float4 yv;
            if (RELU == 1) yv = *reinterpret_cast<const float4*>(y + base + s);
            bn_mask4<RELU>(g, xv, yv, sc, sh);
            if (DRES) *reinterpret_cast<float4*>(dres + base + s) = g;
            float4 o;
            o.x = a * g.x + b * xv.x + k; o.y = a * g.y + b * xv.y + k;
            o.z = a * g.z + b * xv.z + k; o.w = a * g.w + b * xv.w + k;
            *reinterpret_cast<float4*>(dx + base + s) = o;
        }
    } else {
        for (int s = s0 + threadIdx.x; s < s1; s += 256) {
            const float xs = x[base + s];
            const float g = bn_mask<RELU>(dy[base + s], xs, RELU == 1 ? y[base + s] : 0.f, sc, sh);
            if (DRES) dres[base + s] = g;
            dx[base + s] = a * g + b * xs + k;
        }
    }
}

template <int RELU, bool DRES>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                           const float* __restrict__ y, float* __restrict__ dx,
                                                           float* __restrict__ dres, int C, int S,
                                                           const float* __restrict__ ca, const float* __restrict__ cb,
                                                           const float* __restrict__ ck, const float* __restrict__ gamma,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ csh, bool nt) {
    const int row = blockIdx.x;
    const int c = row % C;
    const float a = ca[c], b = cb[c], k = ck[c];
    const float sc = RELU == 2 ? (gamma ? gamma[c] : 1.f) * invstd[c] : 0.f;
    const float sh = RELU == 2 ? csh[c] : 0.f;
    const int s0 = blockIdx.y * ROW_CHUNK;
    bwd_apply_chunk<RELU, DRES>(dy, x, y, dx, dres, (size_t)row * S, s0, min(S, s0 + ROW_CHUNK), S, a, b, k, sc, sh, nt);
}

// The same pass for zsv_bn_sync_bwd_apply: the sums arrive from the all-reduce as 2C doubles and the element count of the whole
// batch as one device double, so every block forms its channel's coefficients itself (bwd_coeff: bn_bwd_finalize_kernel's
// arithmetic) instead of reading them from a finalize launch.  The blocks of the first clip's rows also write dgamma / dbeta from the
// LOCAL sums.
template <int RELU, bool DRES>
__global__ __launch_bounds__(256) void bn_sync_bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                                const float* __restrict__ y, float* __restrict__ dx,
                                                                float* __restrict__ dres, int C, int S, const float* __restrict__ mean,
                                                                const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, const double* __restrict__ sums_local,
                                                                const double* __restrict__ sums_global,
                                                                const double* __restrict__ total_count, float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta, bool nt) {
    const int row = blockIdx.x;
    const int c = row % C;
    float a, b, k;
    bwd_coeff(gamma ? (double)gamma[c] : 1.0, (double)invstd[c], (double)mean[c], sums_global[c], sums_global[C + c], *total_count, a, b, k);
    float sc = 0.f, sh = 0.f;
    if (RELU == 2) train_coeff(c, gamma, beta, mean, invstd, sc, sh);
    if (row < C && blockIdx.y == 0 && threadIdx.x == 0) {
        if (dgamma) dgamma[c] = (float)sums_local[C + c];
        if (dbeta) dbeta[c] = (float)sums_local[c];
    }
    const int s0 = blockIdx.y * ROW_CHUNK;
    bwd_apply_chunk<RELU, DRES>(dy, x, y, dx, dres, (size_t)row * S, s0, min(S, s0 + ROW_CHUNK), S, a, b, k, sc, sh, nt);
}

// ---- eval-mode (frozen statistics) backward: ONE pass --------------------------------------------------------------------
// g = dy * mask (RELU as bn_bwd_reduce_kernel, the mode-2 mask with eval_coeff's scale / shift), dx = scale * g, d_residual = g;
// SUMS: the block's partial sum g and sum g * xhat (xhat = (x - running_mean) * invstd) to part[2][C][slices] -- no
// mean-subtraction terms depend on them, so the input gradient needs no second pass.  Same (channel, slice) grid and fixed
// summation order as bn_bwd_reduce_kernel: bitwise reproducible.
template <int RELU, bool DRES, bool SUMS>
__global__ __launch_bounds__(256) void bn_bwd_eval_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                          const float* __restrict__ y, float* __restrict__ dx,
                                                          float* __restrict__ dres, int N, int C, int S, int slices,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const float* __restrict__ rm, const float* __restrict__ rv, float eps,
                                                          double* __restrict__ part, bool nt) {
    __shared__ double red[4];
    const int c = blockIdx.x, sl = blockIdx.y;
    const bool vec = (S % 4) == 0;
    int b, e;
    slice_range(N * S, slices, sl, vec, b, e);
    float is, sc, sh;
    eval_coeff(c, gamma, beta, rm, rv, eps, is, sc, sh);
    const float mu = rm[c];
    float s1 = 0.f, s2 = 0.f;
    if (vec) {
        for (int i = b + 4 * (int)threadIdx.x; i < e; i += 4 * 256) {
            const int n = i / S, s = i - n * S;
            const size_t off = ((size_t)n * C + c) * S + s;
            float4 g = ld4(dy + off, nt);
            float4 xv;
            if (SUMS || RELU == 2) xv = ld4(x + off, nt);
            float4 yv;
            if (RELU == 1) yv = ld4(y + off, nt);
            bn_mask4<RELU>(g, xv, yv, sc, sh);
            if (DRES) st4(dres + off, g, nt);
            st4(dx + off, make_float4(sc * g.x, sc * g.y, sc * g.z, sc * g.w), nt);
            if (SUMS) {
                s1 += (g.x + g.y) + (g.z + g.w);
                s2 += (g.x * ((xv.x - mu) * is) + g.y * ((xv.y - mu) * is)) +
                      (g.z * ((xv.z - mu) * is) + g.w * ((xv.w - mu) * is));
            }
        }
    } else {
        for (int i = b + (int)threadIdx.x; i < e; i += 256) {
            const int n = i / S, s = i - n * S;
            const size_t off = ((size_t)n * C + c) * S + s;
            const float xs = (SUMS || RELU == 2) ? x[off] : 0.f;
            const float g = bn_mask<RELU>(dy[off], xs, RELU == 1 ? y[off] : 0.f, sc, sh);
            if (DRES) dres[off] = g;
            dx[off] = sc * g;
            if (SUMS) {
                s1 += g;
                s2 += g * ((xs - mu) * is);
            }
        }
    }
    if (SUMS) {
        const double t1 = block_sum_256<double>((double)s1, red);
        const double t2 = block_sum_256<double>((double)s2, red);
        if (threadIdx.x == 0) {
            part[(size_t)c * slices + sl] = t1;
            part[(size_t)(C + c) * slices + sl] = t2;
        }
    }
}

// dgamma = sum g*xhat, dbeta = sum g from the partials (one 64-lane wave per channel, fixed order as bn_bwd_finalize_kernel)
__global__ void bn_bwd_eval_finalize_kernel(const double* __restrict__ part, int C, int slices, float* __restrict__ dgamma,
                                            float* __restrict__ dbeta) {
    const int c = blockIdx.x;
    double sg = 0.0, sgx = 0.0;
    for (int k = threadIdx.x; k < slices; k += 64) {
        sg += part[(size_t)c * slices + k];
        sgx += part[(size_t)(C + c) * slices + k];
    }
    sg = wave_sum(sg);
    sgx = wave_sum(sgx);
    if (threadIdx.x != 0) return;
    if (dgamma) dgamma[c] = (float)sgx;
    if (dbeta) dbeta[c] = (float)sg;
}

// ---- statistics over all ranks (zsv_bn_sync_*): the C-sized steps around the two collectives ---------------------------------
// One rank's moments from bn_stats_kernel's partials (one 64-lane wave per channel, fixed order as bn_finalize_train_kernel):
// moments = [C means | C M2 | count], mean = K + s1/n, M2 = s2 - s1*s1/n with K the rank's own pivot x[c * S].
__global__ void bn_sync_moments_kernel(const double* __restrict__ part, int C, int slices, double count,
                                       const float* __restrict__ pivot_src, int S, double* __restrict__ moments) {
    const int c = blockIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int k = threadIdx.x; k < slices; k += 64) {
        s1 += part[(size_t)c * slices + k];
        s2 += part[(size_t)(C + c) * slices + k];
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if (threadIdx.x != 0) return;
    double m2 = s2 - s1 * s1 / count;
    if (m2 < 0.0) m2 = 0.0;
    moments[c] = (double)pivot_src[(size_t)c * S] + s1 / count;
    moments[C + c] = m2;
    if (c == 0) moments[2 * C] = count;
}

// gathered = [world][2C + 1] in rank order -> the whole batch's mean / M2 / count of channel c by Chan's pairwise update, rank after
// rank in fp64 (a rank whose count is 0 is skipped), then bn_finalize_train_kernel's outputs.  One thread per channel; every
// rank runs this on the same bytes in the same order, so its outputs are the same bits on every rank.
__global__ __launch_bounds__(64) void bn_sync_finalize_kernel(const double* __restrict__ gathered, int world, int C,
                                                              float* __restrict__ running_mean, float* __restrict__ running_var,
                                                              float momentum, float eps, float* __restrict__ save_mean,
                                                              float* __restrict__ save_invstd, double* __restrict__ total_count) {
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const size_t pitch = (size_t)2 * C + 1;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    for (int r = 0; r < world; ++r) {
        const double* row = gathered + (size_t)r * pitch;
        const double nb = row[2 * C];
        if (!(nb > 0.0)) continue;
        if (n == 0.0) {
            n = nb;
            mean = row[c];
            m2 = row[C + c];
            continue;
        }
        const double tot = n + nb;
        const double delta = row[c] - mean;
        mean += delta * nb / tot;
        m2 += row[C + c] + delta * delta * n * nb / tot;
        n = tot;
    }
    if (c == 0) *total_count = n;
    double var = n > 0.0 ? m2 / n : 0.0;
    if (var < 0.0) var = 0.0;
    save_mean[c] = (float)mean;
    save_invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (!(n > 0.0)) return;                          // an empty batch on every rank leaves the running statistics alone
    if (running_mean) running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)mean;
    if (running_var) {
        const double unbiased = n > 1.0 ? var * n / (n - 1.0) : var;
        running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unbiased;
    }
}

// sums = [C sum g | C sum g*xhat] from bn_bwd_reduce_kernel's partials (one wave per channel, fixed order as bn_bwd_finalize_kernel)
__global__ void bn_sync_sums_kernel(const double* __restrict__ part, int C, int slices, double* __restrict__ sums) {
    const int c = blockIdx.x;
    double sg = 0.0, sgx = 0.0;
    for (int k = threadIdx.x; k < slices; k += 64) {
        sg += part[(size_t)c * slices + k];
        sgx += part[(size_t)(C + c) * slices + k];
    }
    sg = wave_sum(sg);
    sgx = wave_sum(sgx);
    if (threadIdx.x != 0) return;
    sums[c] = sg;
    sums[C + c] = sgx;
}

// a rank without clips has no tensor pass to write dgamma / dbeta from its (zero) local sums
__global__ void bn_sync_local_grads_kernel(const double* __restrict__ sums_local, int C, float* __restrict__ dgamma,
                                           float* __restrict__ dbeta) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    if (dgamma) dgamma[c] = (float)sums_local[C + c];
    if (dbeta) dbeta[c] = (float)sums_local[c];
}

// the synchronised family takes N == 0 (a rank without clips)
static int check_sync_ncs(int N, int C, int S) {
    if (N < 0 || C <= 0 || S <= 0) return ZSV_E_BAD_SHAPE;
    if ((double)N * C * S >= 2147483647.0) return ZSV_E_TOO_LARGE;
    return ZSV_OK;
}
static inline bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
template <typename... Rest>
static inline bool aligned_to(const void* p, uintptr_t a, Rest... rest) { return aligned_to(p, a) && aligned_to(rest...); }

static int check_ncs(int N, int C, int S) {
    if (N <= 0 || C <= 0 || S <= 0) return ZSV_E_BAD_SHAPE;
    if ((double)N * C * S >= 2147483647.0) return ZSV_E_TOO_LARGE;
    return ZSV_OK;
}

static int launch_apply(const float* x, const float* res, float* y, int N, int C, int S, const float* scale,
                        const float* shift, int relu, hipStream_t stream) {
    const dim3 grid((unsigned)(N * C), (unsigned)((S + ROW_CHUNK - 1) / ROW_CHUNK));
    const bool nt = bn_stream(N, C, S);
    if (res && relu) hipLaunchKernelGGL((bn_apply_kernel<true, true>), grid, dim3(256), 0, stream, x, res, y, C, S, scale, shift, nt);
    else if (res) hipLaunchKernelGGL((bn_apply_kernel<true, false>), grid, dim3(256), 0, stream, x, res, y, C, S, scale, shift, nt);
    else if (relu) hipLaunchKernelGGL((bn_apply_kernel<false, true>), grid, dim3(256), 0, stream, x, res, y, C, S, scale, shift, nt);
    else hipLaunchKernelGGL((bn_apply_kernel<false, false>), grid, dim3(256), 0, stream, x, res, y, C, S, scale, shift, nt);
    return launch_status();
}

}  // namespace zsv

using namespace zsv;

extern "C" size_t zsv_bn_workspace_bytes(int32_t N, int32_t C, int32_t S) {
    if (check_ncs(N, C, S) != ZSV_OK) return 0;
    return bn_ws_bytes(N, C, S);
}

extern "C" int zsv_bn_fwd_train(const float* x, int32_t N, int32_t C, int32_t S, const float* gamma,
                                const float* beta, const float* residual, int fuse_relu, float* y,
                                float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                                float momentum, float eps, void* workspace, size_t workspace_bytes, void* stream_) {
    return zsv_bn_fwd_train_stats(x, N, C, S, gamma, beta, residual, fuse_relu, y, save_mean, save_invstd, running_mean,
                                  running_var, momentum, eps, nullptr, 0, workspace, workspace_bytes, stream_);
}

extern "C" int zsv_bn_fwd_train_stats(const float* x, int32_t N, int32_t C, int32_t S, const float* gamma,
                                      const float* beta, const float* residual, int fuse_relu, float* y,
                                      float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                                      float momentum, float eps, const float* conv_partials, int32_t stat_tiles,
                                      void* workspace, size_t workspace_bytes, void* stream_) {
    int st = check_ncs(N, C, S);
    if (st) return st;
    if (!x || !y || !save_mean || !save_invstd || !workspace) return ZSV_E_NULL;
    if (workspace_bytes < bn_ws_bytes(N, C, S)) return ZSV_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    int slices = bn_slices(N, C, S);
    BnWs w = bn_ws(workspace, C, slices);
    const float* pivot_src = x;
    if (conv_partials && stat_tiles > 0) {
        // statistics were accumulated by the producing convolution's epilogue (unshifted sums: bias-free convolution outputs,
        // |mean| ~ std): no pass over x, reduce + finalise in one launch
        hipLaunchKernelGGL(bn_finalize_partials_kernel, dim3(C), dim3(256), 0, stream, conv_partials,
                           conv_partials + (size_t)C * stat_tiles, C, stat_tiles, (double)N * S, gamma, beta, save_mean, save_invstd,
                           running_mean, running_var, momentum, eps, w.scale, w.shift);
    } else {
        hipLaunchKernelGGL(bn_stats_kernel, dim3(C, slices), dim3(256), 0, stream, x, N, C, S, slices, w.part);
        if ((st = launch_status())) return st;
        hipLaunchKernelGGL(bn_finalize_train_kernel, dim3(C), dim3(64), 0, stream, (const double*)w.part, C,
                           slices, (double)N * S, pivot_src, S, gamma, beta, save_mean, save_invstd, running_mean, running_var,
                           momentum, eps, w.scale, w.shift);
    }
    if ((st = launch_status())) return st;
    return launch_apply(x, residual, y, N, C, S, w.scale, w.shift, fuse_relu, stream);
}

// Training-mode BatchNorm WITHOUT the normalise pass: statistics (own pass or the producing convolution's epilogue partials),
// save_mean / save_invstd, running statistics, and the per-channel affine y = x * scale + shift written to `coef`
// ([2][coef_pitch]: scale row, shift row; entries C .. coef_pitch-1 are set to 0).  The consumer applies it (+ ReLU) while
// it reads x: zsv_conv3d_fwd_pre / zsv_conv3d_wgrad_pre.  The backward is zsv_bn_bwd with relu_mode 2 (mask recomputed from x).
extern "C" int zsv_bn_fwd_train_coeffs(const float* x, int32_t N, int32_t C, int32_t S, const float* gamma, const float* beta,
                                       float* save_mean, float* save_invstd, float* running_mean, float* running_var,
                                       float momentum, float eps, const float* conv_partials, int32_t stat_tiles, float* coef,
                                       int32_t coef_pitch, void* workspace, size_t workspace_bytes, void* stream_) {
    int st = check_ncs(N, C, S);
    if (st) return st;
    if (!x || !save_mean || !save_invstd || !workspace || !coef) return ZSV_E_NULL;
    if (coef_pitch < C) return ZSV_E_BAD_SHAPE;
    if (workspace_bytes < bn_ws_bytes(N, C, S)) return ZSV_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    int slices = bn_slices(N, C, S);
    BnWs w = bn_ws(workspace, C, slices);
    const float* pivot_src = x;
    if (coef_pitch > C && hipMemsetAsync(coef, 0, (size_t)2 * coef_pitch * sizeof(float), stream) != hipSuccess) return ZSV_E_LAUNCH;
    if (conv_partials && stat_tiles > 0) {
        hipLaunchKernelGGL(bn_finalize_partials_kernel, dim3(C), dim3(256), 0, stream, conv_partials,
                           conv_partials + (size_t)C * stat_tiles, C, stat_tiles, (double)N * S, gamma, beta, save_mean, save_invstd,
                           running_mean, running_var, momentum, eps, coef, coef + coef_pitch);
        return launch_status();
    }
    hipLaunchKernelGGL(bn_stats_kernel, dim3(C, slices), dim3(256), 0, stream, x, N, C, S, slices, w.part);
    if ((st = launch_status())) return st;
    hipLaunchKernelGGL(bn_finalize_train_kernel, dim3(C), dim3(64), 0, stream, (const double*)w.part, C,
                       slices, (double)N * S, pivot_src, S, gamma, beta, save_mean, save_invstd, running_mean, running_var,
                       momentum, eps, coef, coef + coef_pitch);
    return launch_status();
}

extern "C" int zsv_bn_fwd_eval(const float* x, int32_t N, int32_t C, int32_t S, const float* gamma, const float* beta,
                               const float* running_mean, const float* running_var, const float* residual,
                               int fuse_relu, float eps, float* y, void* workspace, size_t workspace_bytes,
                               void* stream_) {
    int st = check_ncs(N, C, S);
    if (st) return st;
    if (!x || !y || !running_mean || !running_var || !workspace) return ZSV_E_NULL;
    if (workspace_bytes < bn_ws_bytes(N, C, S)) return ZSV_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    BnWs w = bn_ws(workspace, C, bn_slices(N, C, S));
    hipLaunchKernelGGL(bn_eval_coeff_kernel, dim3((C + 127) / 128), dim3(128), 0, stream, C, gamma, beta, running_mean,
                       running_var, eps, w.scale, w.shift);
    if ((st = launch_status())) return st;
    return launch_apply(x, residual, y, N, C, S, w.scale, w.shift, fuse_relu, stream);
}

extern "C" int zsv_bn_bwd(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
                          const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                          int fuse_relu, float* dx, float* d_residual, float* dgamma, float* dbeta, void* workspace,
                          size_t workspace_bytes, void* stream_) {
    int st = check_ncs(N, C, S);
    if (st) return st;
    if (!dy || !x || !dx || !save_mean || !save_invstd || !workspace) return ZSV_E_NULL;
    if (fuse_relu < 0 || fuse_relu > 2) return ZSV_E_BAD_SHAPE;
    if (fuse_relu == 1 && !y) return ZSV_E_NULL;
    if (workspace_bytes < bn_ws_bytes(N, C, S)) return ZSV_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const int slices = bn_slices(N, C, S);
    BnWs w = bn_ws(workspace, C, slices);
    const dim3 rgrid(C, slices);
    // fuse_relu 1 with a residual gradient: the reduction writes the masked gradient (= d_residual), the apply pass reads it (mode 0)
    const bool g_from_reduce = fuse_relu == 1 && d_residual != nullptr && ZSV_KNOB(BN_NO_MASKED_G) == nullptr;
    const bool nt = bn_stream(N, C, S);
    if (fuse_relu == 2)
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<2>), rgrid, dim3(256), 0, stream, dy, x, y, N, C, S, slices, save_mean, save_invstd, gamma, beta, w.part, (float*)nullptr, nt);
    else if (fuse_relu == 1)
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<1>), rgrid, dim3(256), 0, stream, dy, x, y, N, C, S, slices, save_mean, save_invstd, gamma, beta, w.part,
                           g_from_reduce ? d_residual : (float*)nullptr, nt);
    else
        hipLaunchKernelGGL((bn_bwd_reduce_kernel<0>), rgrid, dim3(256), 0, stream, dy, x, y, N, C, S, slices, save_mean, save_invstd, gamma, beta, w.part, (float*)nullptr, nt);
    if ((st = launch_status())) return st;
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(64), 0, stream, (const double*)w.part, C, slices,
                       (double)N * S, gamma, save_mean, save_invstd, dgamma, dbeta, w.scale, w.shift, w.c1, beta, w.c2);
    if ((st = launch_status())) return st;
    const dim3 grid((unsigned)(N * C), (unsigned)((S + ROW_CHUNK - 1) / ROW_CHUNK));
#define ZSV_BWD_APPLY(R, D) hipLaunchKernelGGL((bn_bwd_apply_kernel<R, D>), grid, dim3(256), 0, stream, dy, x, y, dx, d_residual, C, S, w.scale, w.shift, w.c1, gamma, save_invstd, w.c2, nt)
    if (g_from_reduce) {
        hipLaunchKernelGGL((bn_bwd_apply_kernel<0, false>), grid, dim3(256), 0, stream, (const float*)d_residual, x, y, dx, (float*)nullptr, C, S, w.scale, w.shift, w.c1,
                           gamma, save_invstd, w.c2, nt);
        return launch_status();
    }
    if (fuse_relu == 2) { if (d_residual) ZSV_BWD_APPLY(2, true); else ZSV_BWD_APPLY(2, false); }
    else if (fuse_relu == 1) { if (d_residual) ZSV_BWD_APPLY(1, true); else ZSV_BWD_APPLY(1, false); }
    else { if (d_residual) ZSV_BWD_APPLY(0, true); else ZSV_BWD_APPLY(0, false); }
#undef ZSV_BWD_APPLY
    return launch_status();
}

extern "C" int zsv_bn_eval_coeffs(int32_t C, const float* gamma, const float* beta, const float* running_mean,
                                  const float* running_var, float eps, float* coef, int32_t coef_pitch, void* stream_) {
    if (C <= 0 || coef_pitch < C) return ZSV_E_BAD_SHAPE;
    if (!running_mean || !running_var || !coef) return ZSV_E_NULL;
    hipLaunchKernelGGL(bn_eval_coef_rows_kernel, dim3((coef_pitch + 127) / 128), dim3(128), 0, (hipStream_t)stream_, C, coef_pitch,
                       gamma, beta, running_mean, running_var, eps, coef);
    return launch_status();
}

extern "C" int zsv_bn_bwd_eval(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
                               const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                               float eps, int fuse_relu, float* dx, float* d_residual, float* dgamma, float* dbeta,
                               void* workspace, size_t workspace_bytes, void* stream_) {
    int st = check_ncs(N, C, S);
    if (st) return st;
    if (fuse_relu < 0 || fuse_relu > 2) return ZSV_E_BAD_SHAPE;
    const bool sums = dgamma != nullptr || dbeta != nullptr;
    if (!dy || !dx || !running_mean || !running_var) return ZSV_E_NULL;
    if ((sums || fuse_relu == 2) && !x) return ZSV_E_NULL;
    if (fuse_relu == 1 && !y) return ZSV_E_NULL;
    if (sums && (!workspace || workspace_bytes < bn_ws_bytes(N, C, S))) return ZSV_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const int slices = bn_slices(N, C, S);
    double* part = sums ? (double*)workspace : nullptr;
    const dim3 grid(C, slices);
    const bool nt = bn_stream(N, C, S);
#define ZSV_BWD_EVAL(R, D, SU) hipLaunchKernelGGL((bn_bwd_eval_kernel<R, D, SU>), grid, dim3(256), 0, stream, dy, x, y, dx, d_residual, \
                                                  N, C, S, slices, gamma, beta, running_mean, running_var, eps, part, nt)
#define ZSV_BWD_EVAL_R(R) do { \
        if (d_residual) { if (sums) ZSV_BWD_EVAL(R, true, true); else ZSV_BWD_EVAL(R, true, false); } \
        else { if (sums) ZSV_BWD_EVAL(R, false, true); else ZSV_BWD_EVAL(R, false, false); } } while (0)
    if (fuse_relu == 2) ZSV_BWD_EVAL_R(2);
    else if (fuse_relu == 1) ZSV_BWD_EVAL_R(1);
    else ZSV_BWD_EVAL_R(0);
#undef ZSV_BWD_EVAL_R
#undef ZSV_BWD_EVAL
    if ((st = launch_status()) || !sums) return st;
    hipLaunchKernelGGL(bn_bwd_eval_finalize_kernel, dim3(C), dim3(64), 0, stream, (const double*)part, C, slices, dgamma, dbeta);
    return launch_status();
}

// ---- BatchNorm with batch statistics over all ranks -----------------------------------------------------------------------
// The collectives run between these calls, in the caller (ops.sync_batch_norm_act): the library never sees a communicator.
extern "C" size_t zsv_bn_sync_workspace_bytes(int32_t N, int32_t C, int32_t S) {
    if (check_sync_ncs(N, C, S) != ZSV_OK) return 0;
    if (N == 0) return 16;
    return (size_t)2 * C * bn_slices(N, C, S) * sizeof(double);
}

extern "C" int zsv_bn_sync_moments(const float* x, int32_t N, int32_t C, int32_t S, double* moments, void* workspace,
                                   size_t workspace_bytes, void* stream_) {
    int st = check_sync_ncs(N, C, S);
    if (st) return st;
    if (!moments || !workspace || (N > 0 && !x)) return ZSV_E_NULL;
    if (workspace_bytes < zsv_bn_sync_workspace_bytes(N, C, S)) return ZSV_E_WORKSPACE;
    if (!aligned_to(x, 4, moments, 8, workspace, 16)) return ZSV_E_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    if (N == 0)                                      // count 0, zeros: zsv_bn_sync_finalize skips this rank
        return hipMemsetAsync(moments, 0, ((size_t)2 * C + 1) * sizeof(double), stream) == hipSuccess ? ZSV_OK : ZSV_E_LAUNCH;
    const int slices = bn_slices(N, C, S);
    double* part = (double*)workspace;
    hipLaunchKernelGGL(bn_stats_kernel, dim3(C, slices), dim3(256), 0, stream, x, N, C, S, slices, part);
    if ((st = launch_status())) return st;
    hipLaunchKernelGGL(bn_sync_moments_kernel, dim3(C), dim3(64), 0, stream, (const double*)part, C, slices, (double)N * S, x, S,
                       moments);
    return launch_status();
}

extern "C" int zsv_bn_sync_finalize(const double* gathered, int32_t world, int32_t C, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                                    float* save_invstd, double* total_count_out, void* stream_) {
    (void)gamma; (void)beta;                         // the apply passes form scale / shift themselves (include/zsv_hip.h)
    if (world <= 0 || C <= 0) return ZSV_E_BAD_SHAPE;
    if ((double)world * (2.0 * C + 1.0) >= 2147483647.0) return ZSV_E_TOO_LARGE;
    if (!gathered || !save_mean || !save_invstd || !total_count_out) return ZSV_E_NULL;
    if (!aligned_to(gathered, 8, total_count_out, 8, running_mean, 4, running_var, 4, save_mean, 4, save_invstd, 4))
        return ZSV_E_UNSUPPORTED;
    hipLaunchKernelGGL(bn_sync_finalize_kernel, dim3((C + 63) / 64), dim3(64), 0, (hipStream_t)stream_, gathered, world, C,
                       running_mean, running_var, momentum, eps, save_mean, save_invstd, total_count_out);
    return launch_status();
}

extern "C" int zsv_bn_sync_apply(const float* x, int32_t N, int32_t C, int32_t S, const float* save_mean, const float* save_invstd,
                                 const float* gamma, const float* beta, const float* residual, int fuse_relu, float* y,
                                 void* stream_) {
    int st = check_sync_ncs(N, C, S);
    if (st) return st;
    if (!save_mean || !save_invstd || (N > 0 && (!x || !y))) return ZSV_E_NULL;
    if (!aligned_to(x, 4, y, 4, residual, 4, save_mean, 4, save_invstd, 4, gamma, 4, beta, 4)) return ZSV_E_UNSUPPORTED;
    if (N == 0) return ZSV_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid((unsigned)(N * C), (unsigned)((S + ROW_CHUNK - 1) / ROW_CHUNK));
    const bool nt = bn_stream(N, C, S);
#define ZSV_SYNC_APPLY(R, A) hipLaunchKernelGGL((bn_sync_apply_kernel<R, A>), grid, dim3(256), 0, stream, x, residual, y, C, S, save_mean, save_invstd, gamma, beta, nt)
    if (residual) { if (fuse_relu) ZSV_SYNC_APPLY(true, true); else ZSV_SYNC_APPLY(true, false); }
    else { if (fuse_relu) ZSV_SYNC_APPLY(false, true); else ZSV_SYNC_APPLY(false, false); }
#undef ZSV_SYNC_APPLY
    return launch_status();
}

extern "C" int zsv_bn_sync_bwd_reduce(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
                                      const float* save_mean, const float* save_invstd, const float* gamma, const float* beta,
                                      int fuse_relu, double* sums, void* workspace, size_t workspace_bytes, void* stream_) {
    int st = check_sync_ncs(N, C, S);
    if (st) return st;
    if (fuse_relu < 0 || fuse_relu > 2) return ZSV_E_BAD_SHAPE;
    if (!save_mean || !save_invstd || !sums || !workspace) return ZSV_E_NULL;
    if (N > 0 && (!dy || !x || (fuse_relu == 1 && !y))) return ZSV_E_NULL;
    if (workspace_bytes < zsv_bn_sync_workspace_bytes(N, C, S)) return ZSV_E_WORKSPACE;
    if (!aligned_to(dy, 4, x, 4, y, 4, save_mean, 4, save_invstd, 4, gamma, 4, beta, 4, sums, 8, workspace, 16)) return ZSV_E_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    if (N == 0) return hipMemsetAsync(sums, 0, (size_t)2 * C * sizeof(double), stream) == hipSuccess ? ZSV_OK : ZSV_E_LAUNCH;
    const int slices = bn_slices(N, C, S);
    double* part = (double*)workspace;
    const dim3 rgrid(C, slices);
    const bool nt = bn_stream(N, C, S);
#define ZSV_SYNC_REDUCE(R) hipLaunchKernelGGL((bn_bwd_reduce_kernel<R>), rgrid, dim3(256), 0, stream, dy, x, y, N, C, S, slices, save_mean, save_invstd, gamma, beta, part, (float*)nullptr, nt)
    if (fuse_relu == 2) ZSV_SYNC_REDUCE(2);
    else if (fuse_relu == 1) ZSV_SYNC_REDUCE(1);
    else ZSV_SYNC_REDUCE(0);
#undef ZSV_SYNC_REDUCE
    if ((st = launch_status())) return st;
    hipLaunchKernelGGL(bn_sync_sums_kernel, dim3(C), dim3(64), 0, stream, (const double*)part, C, slices, sums);
    return launch_status();
}

extern "C" int zsv_bn_sync_bwd_apply(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
                                     const float* save_mean, const float* save_invstd, const float* gamma, const float* beta,
                                     int fuse_relu, const double* sums_local, const double* sums_global, const double* total_count,
                                     float* dx, float* d_residual, float* dgamma, float* dbeta, void* stream_) {
    int st = check_sync_ncs(N, C, S);
    if (st) return st;
    if (fuse_relu < 0 || fuse_relu > 2) return ZSV_E_BAD_SHAPE;
    if (!save_mean || !save_invstd || !sums_local || !sums_global || !total_count) return ZSV_E_NULL;
    if (N > 0 && (!dy || !x || !dx || (fuse_relu == 1 && !y))) return ZSV_E_NULL;
    if (!aligned_to(dy, 4, x, 4, y, 4, dx, 4, d_residual, 4, dgamma, 4, dbeta, 4, save_mean, 4, save_invstd, 4, gamma, 4, beta, 4,
                    sums_local, 8, sums_global, 8, total_count, 8))
        return ZSV_E_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    if (N == 0) {
        if (!dgamma && !dbeta) return ZSV_OK;
        hipLaunchKernelGGL(bn_sync_local_grads_kernel, dim3((C + 127) / 128), dim3(128), 0, stream, sums_local, C, dgamma, dbeta);
        return launch_status();
    }
    const dim3 grid((unsigned)(N * C), (unsigned)((S + ROW_CHUNK - 1) / ROW_CHUNK));
    const bool nt = bn_stream(N, C, S);
#define ZSV_SYNC_BWD_APPLY(R, D) hipLaunchKernelGGL((bn_sync_bwd_apply_kernel<R, D>), grid, dim3(256), 0, stream, dy, x, y, dx, d_residual, C, S, save_mean, save_invstd, gamma, beta, sums_local, sums_global, total_count, dgamma, dbeta, nt)
    if (fuse_relu == 2) { if (d_residual) ZSV_SYNC_BWD_APPLY(2, true); else ZSV_SYNC_BWD_APPLY(2, false); }
    else if (fuse_relu == 1) { if (d_residual) ZSV_SYNC_BWD_APPLY(1, true); else ZSV_SYNC_BWD_APPLY(1, false); }
    else { if (d_residual) ZSV_SYNC_BWD_APPLY(0, true); else ZSV_SYNC_BWD_APPLY(0, false); }
#undef ZSV_SYNC_BWD_APPLY
    return launch_status();
}
