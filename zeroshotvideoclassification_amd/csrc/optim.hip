// optim.hip -- weight decay and global-norm gradient clipping for the multi-tensor Adam step (include/zsv_hip.h).
//
//   torch                                          here
//   clip_grad_norm_(params, max_norm)              grad_norm_multi (sum of squares per 4096-element chunk, + the non-finite
//                                                  check of the loss scaler) and grad_norm_finalize (fixed-order sum in double,
//                                                  1/scale, {total_norm, clip_coef}); the coefficient is applied on the
//                                                  gradient's way into the update, the gradients in memory are not rewritten
//   Adam(weight_decay=) / AdamW                    adamw_multi / adamw_multi_scaled
//   GradScaler.unscale_                            grad_unscale_multi
//   k x loss.backward() accumulating into .grad    grad_accum_multi (table of {acc, g}: acc = [acc +] scale * g, one launch per
//                                                  gradient bucket and backward pass; ddp.GradientSync)
//   swa_utils.AveragedModel.update_parameters      the *_avg forms of the four Adam launches (the shadow is updated with the
//                                                  parameter value still in a register), avg_multi for BatchNorm running
//                                                  statistics, avg_advance (the device-resident count), swap_multi
//
// All of them walk the zsv_adam_tensor table of zsv_adam_multi (elementwise_pool.hip) the same way: one workgroup of 256
// threads per chunk, a binary search over first_chunk.  No floating-point atomics: every sum has a fixed order, so the same
// gradients give the same norm bits and the same parameter bits on every run.
#include "zsv_common.h"
#include "zsv_hip.h"
#include "adam_update.h"

#include <math.h>

namespace zsv {
constexpr int OPT_CHUNK = 4096;                       // = ADAM_CHUNK of elementwise_pool.hip

// index of the last tensor whose first_chunk <= chunk
template <typename T> __device__ __forceinline__ int find_index(const T* __restrict__ table, int count, long chunk) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ zsv_adam_tensor find_tensor(const zsv_adam_tensor* __restrict__ table, int count, long chunk) {
    return table[find_index(table, count, chunk)];
}

// where a launch with weight averaging finds the shadows and the rule
struct AvgArgs {
    float* const* shadows;          // count pointers, parallel to the table
    const zsv_avg_state* state;
    float ema_weight;               // >= 0: EMA weight of the new value; < 0: equal-weight
};

__device__ __forceinline__ bool non_finite(float g) { return !(fabsf(g) <= 3.402823466e38f); }     // inf or NaN

// partials[blockIdx.x] = sum of g^2 over the chunk: <= 16 serial adds per lane, then a fixed 8-level tree over 256 lanes.
__global__ __launch_bounds__(256) void grad_norm_multi_kernel(const zsv_adam_tensor* __restrict__ table, int count,
                                                              float* __restrict__ partials, zsv_scaler_state* __restrict__ st) {
    __shared__ float red[4];
    const long chunk = blockIdx.x;
    const zsv_adam_tensor t = find_tensor(table, count, chunk);
    const long base = (chunk - t.first_chunk) * OPT_CHUNK;
    const long end = min(t.n, base + OPT_CHUNK);
    float s = 0.f;
    bool bad = false;
    for (long i = base + threadIdx.x; i < end; i += 256) {
        const float g = t.g[i];
        bad |= non_finite(g);
        s += g * g;
    }
    if (st != nullptr && __any(bad) && (threadIdx.x & 63) == 0) st->found_inf = 1;   // benign race: every writer stores 1
    const float total = block_sum_256<float>(s, red);
    if (threadIdx.x == 0) partials[chunk] = total;
}

// One workgroup: lane k sums partials[k], partials[k + 256], ... in double, then the same fixed tree.
__global__ __launch_bounds__(256) void grad_norm_finalize_kernel(const float* __restrict__ partials, long total_chunks,
                                                                 float max_norm, const zsv_scaler_state* __restrict__ st,
                                                                 zsv_clip_record* __restrict__ record) {
    __shared__ double red[4];
    double s = 0.0;
    for (long i = threadIdx.x; i < total_chunks; i += 256) s += (double)partials[i];
    const double sum = block_sum_256<double>(s, red);
    if (threadIdx.x != 0) return;
    float norm = (float)sqrt(sum);
    if (st != nullptr) norm *= (float)(1.0 / (double)st->scale);      // the gradients in memory are scaled
    const float coef = max_norm / (norm + 1e-6f);                     // clip_grad_norm_: max_norm / (total_norm + 1e-6),
    record->total_norm = norm;                                        // clamped to at most 1 (a NaN stays a NaN)
    record->clip_coef = coef > 1.f ? 1.f : coef;
}

__global__ __launch_bounds__(256) void grad_unscale_multi_kernel(const zsv_adam_tensor* __restrict__ table, int count,
                                                                 zsv_scaler_state* __restrict__ st) {
    const float inv_scale = (float)(1.0 / (double)st->scale);
    const long chunk = blockIdx.x;
    const zsv_adam_tensor t = find_tensor(table, count, chunk);
    const long base = (chunk - t.first_chunk) * OPT_CHUNK;
    const long end = min(t.n, base + OPT_CHUNK);
    float* g = const_cast<float*>(t.g);
    bool bad = false;
    for (long i = base + threadIdx.x; i < end; i += 256) {
        const float gi = g[i];
        bad |= non_finite(gi);
        g[i] = gi * inv_scale;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) st->found_inf = 1;
}

struct AdamwArgs {
    float b1, b2, eps;
    float wd_l2;            // L2 mode: g += wd_l2 * p                (0 otherwise)
    float decay_factor;     // decoupled mode: p *= decay_factor      (1 otherwise)
    int decoupled;
    const zsv_clip_record* clip;
};

// g = g_mem * inv_scale * clip_coef; L2: g += wd * p; moments; decoupled: p *= 1 - lr * wd; Adam update; AVG: the shadow takes
// the new p.
template <bool AVG>
__device__ __forceinline__ void adamw_chunk(const zsv_adam_tensor* __restrict__ table, int count, const AdamwArgs& a,
                                            float inv_scale, float step_size, float inv_sqrt_bc2, const AvgArgs& avg) {
    const float clip = a.clip != nullptr ? a.clip->clip_coef : 1.f;
    const long chunk = blockIdx.x;
    const int index = find_index(table, count, chunk);
    const zsv_adam_tensor t = table[index];
    float* shadow = nullptr;
    AvgWeight k{};
    if (AVG) {
        shadow = avg.shadows[index];
        k = avg_weight(avg.state, avg.ema_weight);
    }
    const long base = (chunk - t.first_chunk) * OPT_CHUNK;
    const long end = min(t.n, base + OPT_CHUNK);
    for (long i = base + threadIdx.x; i < end; i += 256) {
        float pi = t.p[i];
        float gi = t.g[i] * inv_scale;                 // two separate fp32 products, as unscale_ and clip_grad_norm_ store them
        gi = gi * clip;
        if (!a.decoupled) gi = gi + a.wd_l2 * pi;      // grad.add(param, alpha=weight_decay)
        const float mi = a.b1 * t.exp_avg[i] + (1.f - a.b1) * gi;
        const float vi = a.b2 * t.exp_avg_sq[i] + (1.f - a.b2) * gi * gi;
        t.exp_avg[i] = mi;
        t.exp_avg_sq[i] = vi;
        if (a.decoupled) pi *= a.decay_factor;         // param.mul_(1 - lr * weight_decay)
        pi = pi - step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + a.eps));
        t.p[i] = pi;
        if (AVG) avg_element(shadow, i, pi, k);
    }
}

template <bool AVG>
__global__ __launch_bounds__(256) void adamw_multi_kernel(const zsv_adam_tensor* __restrict__ table, int count, AdamwArgs a,
                                                          float step_size, float inv_sqrt_bc2, AvgArgs avg) {
    adamw_chunk<AVG>(table, count, a, 1.f, step_size, inv_sqrt_bc2, avg);
}

template <bool AVG>
__global__ __launch_bounds__(256) void adamw_multi_scaled_kernel(const zsv_adam_tensor* __restrict__ table, int count, AdamwArgs a,
                                                                 double lr, const zsv_scaler_state* __restrict__ st,
                                                                 int grads_unscaled, AvgArgs avg) {
    if (st->found_inf) return;                     // scaler.step skips optimizer.step, weight decay and averaging included
    const float inv_scale = grads_unscaled ? 1.f : (float)(1.0 / (double)st->scale);
    const int step = st->steps_done + 1;
    const float step_size = (float)(lr / (1.0 - pow((double)a.b1, (double)step)));
    const float inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)a.b2, (double)step)));
    adamw_chunk<AVG>(table, count, a, inv_scale, step_size, inv_sqrt_bc2, avg);
}

// ---- zsv_adam_multi[_scaled] with the average: the plain update (adam_element, the body elementwise_pool.hip runs) ------------
__device__ __forceinline__ void adam_avg_chunk(const zsv_adam_tensor* __restrict__ table, int count, float b1, float b2, float eps,
                                               float inv_scale, bool scaled, float step_size, float inv_sqrt_bc2,
                                               const AvgArgs& avg) {
    const long chunk = blockIdx.x;
    const int index = find_index(table, count, chunk);
    const zsv_adam_tensor t = table[index];
    float* shadow = avg.shadows[index];
    const AvgWeight k = avg_weight(avg.state, avg.ema_weight);
    const long base = (chunk - t.first_chunk) * OPT_CHUNK;
    const long end = min(t.n, base + OPT_CHUNK);
    if (scaled) {
        for (long i = base + threadIdx.x; i < end; i += 256)
            adam_element<true>(t, i, t.g[i] * inv_scale, b1, b2, eps, step_size, inv_sqrt_bc2, shadow, k);
    } else {
        for (long i = base + threadIdx.x; i < end; i += 256)
            adam_element<true>(t, i, t.g[i], b1, b2, eps, step_size, inv_sqrt_bc2, shadow, k);
    }
}

__global__ __launch_bounds__(256) void adam_multi_avg_kernel(const zsv_adam_tensor* __restrict__ table, int count, float b1,
                                                             float b2, float eps, float step_size, float inv_sqrt_bc2,
                                                             AvgArgs avg) {
    adam_avg_chunk(table, count, b1, b2, eps, 1.f, false, step_size, inv_sqrt_bc2, avg);
}

__global__ __launch_bounds__(256) void adam_multi_scaled_avg_kernel(const zsv_adam_tensor* __restrict__ table, int count, float lr,
                                                                    float b1, float b2, float eps,
                                                                    const zsv_scaler_state* __restrict__ st, AvgArgs avg) {
    if (st->found_inf) return;                                     // a skipped step averages nothing
    const float inv_scale = (float)(1.0 / (double)st->scale);
    const int step = st->steps_done + 1;
    const float step_size = (float)((double)lr / (1.0 - pow((double)b1, (double)step)));
    const float inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)b2, (double)step)));
    adam_avg_chunk(table, count, b1, b2, eps, inv_scale, true, step_size, inv_sqrt_bc2, avg);
}

// ---- pairs of arrays: b = rule(b, a) (avg_multi) and a <-> b (swap_multi) ------------------------------------------------------
// Streaming passes over a table of {a, b}, chunked like everything above and with the alignment handling of grad_accum_multi
// below: `b` (a slice of the flat shadow buffer, at an arbitrary ELEMENT offset) is walked as head (0-3 scalars up to its first
// 16-byte boundary), aligned float4 body, tail (0-3 scalars); `a` moves as a float4 where it is aligned at the same element
// (wave-uniform test) and as four dwords otherwise.  F maps one element: f(a_i, b_i) updates both in registers.
typedef float pair_v4f __attribute__((ext_vector_type(4)));

template <bool WRITE_A, typename F>
__device__ __forceinline__ void pair_chunk(const zsv_pair_tensor* __restrict__ table, int count, F f) {
    const long chunk = blockIdx.x;
    const zsv_pair_tensor t = table[find_index(table, count, chunk)];
    const long base = (chunk - t.first_chunk) * OPT_CHUNK;
    if (base >= t.n) return;
    const int len = (int)min((long)OPT_CHUNK, t.n - base);
    float* __restrict__ a = t.a + base;
    float* __restrict__ b = t.b + base;

    const int head = min(len, (int)(((16u - (unsigned)((uintptr_t)b & 15u)) & 15u) >> 2));
    const int nvec = (len - head) >> 2;
    const int tail0 = head + 4 * nvec;                // [tail0, len): 0-3 elements
    auto one = [&](int i) {
        float av = a[i], bv = shadow_load(b + i);
        f(av, bv);
        if (WRITE_A) a[i] = av;
        shadow_store(bv, b + i);
    };
    if ((int)threadIdx.x < head) one(threadIdx.x);
    if ((int)threadIdx.x < len - tail0) one(tail0 + threadIdx.x);
    pair_v4f* __restrict__ bvec = reinterpret_cast<pair_v4f*>(b + head);
    float* __restrict__ ab = a + head;
    const bool a_aligned = ((uintptr_t)ab & 15u) == 0;        // same for every lane of the chunk
#pragma unroll 2
    for (int v = threadIdx.x; v < nvec; v += 256) {
        pair_v4f av;
        if (a_aligned) {
            av = reinterpret_cast<const pair_v4f*>(ab)[v];
        } else {
            av[0] = ab[4 * v];
            av[1] = ab[4 * v + 1];
            av[2] = ab[4 * v + 2];
            av[3] = ab[4 * v + 3];
        }
        pair_v4f bv = shadow_load(bvec + v);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float x = av[e], y = bv[e];
            f(x, y);
            av[e] = x;
            bv[e] = y;
        }
        if (WRITE_A) {
            if (a_aligned) {
                reinterpret_cast<pair_v4f*>(ab)[v] = av;
            } else {
                ab[4 * v] = av[0];
                ab[4 * v + 1] = av[1];
                ab[4 * v + 2] = av[2];
                ab[4 * v + 3] = av[3];
            }
        }
        shadow_store(bv, bvec + v);
    }
}

__global__ __launch_bounds__(256) void avg_multi_kernel(const zsv_pair_tensor* __restrict__ table, int count,
                                                        const zsv_avg_state* __restrict__ avg, float ema_weight,
                                                        const zsv_scaler_state* __restrict__ st) {
    if (st != nullptr && st->found_inf) return;                    // the optimizer step was skipped: so is its average
    const AvgWeight k = avg_weight(avg, ema_weight);
    pair_chunk<false>(table, count, [k](float& a, float& b) { b = avg_value(b, a, k); });
}

__global__ __launch_bounds__(256) void swap_multi_kernel(const zsv_pair_tensor* __restrict__ table, int count) {
    pair_chunk<true>(table, count, [](float& a, float& b) { const float x = a; a = b; b = x; });
}

__global__ void avg_advance_kernel(zsv_avg_state* avg, const zsv_scaler_state* st) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st == nullptr || !st->found_inf) avg->n_averaged += 1;
}

// ---- gradient accumulation: acc = [acc +] scale * g over a table of {accumulator slice, fresh gradient} ---------------------
// One workgroup per 4096-element chunk, as above.  An HBM-bound streaming pass (read g, read-modify-write acc), so the body
// moves 16 bytes per lane: the accumulator slices start at arbitrary ELEMENT offsets of a flat bucket and the gradients are
// allocations of their own, i.e. the two pointers of an entry are only 4-byte aligned and differently so.  Per chunk:
//   head   0-3 scalar elements up to the first 16-byte boundary of `acc`
//   body   aligned float4 on `acc`; `g` as an aligned float4 when it happens to be aligned there too (wave-uniform test),
//          else as four dword loads
//   tail   0-3 scalar elements
// `g` is read once per pass and never again: non-temporal loads, so its lines do not push the kernels running next to this
// pass (the backward still in flight on the other queue) out of the cache.  No element outside [acc, acc + n) is touched.
// fl(acc + fl(scale * g)) with the contraction into an fma switched off: the sum has the bits torch's mul + add gives.
typedef float acc_v4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float accum_one(float a, float g, float scale, bool assign) {
#pragma clang fp contract(off)
    const float sg = scale * g;
    return assign ? sg : a + sg;
}

__global__ __launch_bounds__(256) void grad_accum_multi_kernel(const zsv_accum_tensor* __restrict__ table, int count, float scale,
                                                               int assign) {
    const long chunk = blockIdx.x;
    int lo = 0, hi = count - 1;                       // last tensor whose first_chunk <= chunk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
    }
    const zsv_accum_tensor t = table[lo];
    const long base = (chunk - t.first_chunk) * OPT_CHUNK;
    if (base >= t.n) return;
    const int len = (int)min((long)OPT_CHUNK, t.n - base);
    float* __restrict__ acc = t.acc + base;
    const float* __restrict__ g = t.g + base;
    const bool set = assign != 0;

    const int head = min(len, (int)(((16u - (unsigned)((uintptr_t)acc & 15u)) & 15u) >> 2));
    const int nvec = (len - head) >> 2;
    const int tail0 = head + 4 * nvec;                // [tail0, len): 0-3 elements
    if ((int)threadIdx.x < head) {
        const int i = threadIdx.x;
        acc[i] = accum_one(set ? 0.f : acc[i], __builtin_nontemporal_load(g + i), scale, set);
    }
    if ((int)threadIdx.x < len - tail0) {
        const int i = tail0 + threadIdx.x;
        acc[i] = accum_one(set ? 0.f : acc[i], __builtin_nontemporal_load(g + i), scale, set);
    }
    acc_v4f* __restrict__ av = reinterpret_cast<acc_v4f*>(acc + head);
    const float* __restrict__ gb = g + head;
    const bool g_aligned = ((uintptr_t)gb & 15u) == 0;        // same for every lane of the chunk
#pragma unroll 2
    for (int v = threadIdx.x; v < nvec; v += 256) {
        acc_v4f gv;
        if (g_aligned) {
            gv = __builtin_nontemporal_load(reinterpret_cast<const acc_v4f*>(gb) + v);
        } else {
            gv[0] = __builtin_nontemporal_load(gb + 4 * v);
            gv[1] = __builtin_nontemporal_load(gb + 4 * v + 1);
            gv[2] = __builtin_nontemporal_load(gb + 4 * v + 2);
            gv[3] = __builtin_nontemporal_load(gb + 4 * v + 3);
        }
        acc_v4f a;
        if (set) a = acc_v4f{0.f, 0.f, 0.f, 0.f}; else a = av[v];
        acc_v4f r;
        r[0] = accum_one(a[0], gv[0], scale, set);
        r[1] = accum_one(a[1], gv[1], scale, set);
        r[2] = accum_one(a[2], gv[2], scale, set);
        r[3] = accum_one(a[3], gv[3], scale, set);
        av[v] = r;
    }
}

static inline bool bad_table(int32_t count, int64_t total_chunks) {
    return count <= 0 || total_chunks <= 0 || total_chunks > 0x7fffffffL;
}

static inline bool make_args(AdamwArgs& a, double lr, float beta1, float beta2, float eps, double weight_decay, int32_t decoupled,
                             const zsv_clip_record* clip) {
    if (!(lr >= 0.0) || !(weight_decay >= 0.0) || !isfinite(lr) || !isfinite(weight_decay)) return false;
    a.b1 = beta1;
    a.b2 = beta2;
    a.eps = eps;
    a.decoupled = decoupled != 0 && weight_decay != 0.0;
    a.wd_l2 = a.decoupled ? 0.f : (float)weight_decay;
    a.decay_factor = a.decoupled ? (float)(1.0 - lr * weight_decay) : 1.f;
    a.clip = clip;
    return true;
}
}  // namespace zsv

using namespace zsv;

extern "C" size_t zsv_grad_norm_workspace_bytes(int64_t total_chunks) {
    return total_chunks > 0 ? (size_t)total_chunks * sizeof(float) : 0;
}

extern "C" int zsv_grad_norm_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, int64_t chunk_offset,
                                   void* partials_device, size_t partials_bytes, zsv_scaler_state* state_device, void* stream) {
    if (!table_device || !partials_device) return ZSV_E_NULL;
    if (bad_table(count, total_chunks) || chunk_offset < 0) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    if (partials_bytes < zsv_grad_norm_workspace_bytes(chunk_offset + total_chunks)) return ZSV_E_WORKSPACE;
    hipLaunchKernelGGL(grad_norm_multi_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device, count,
                       (float*)partials_device + chunk_offset, state_device);
    return launch_status();
}

extern "C" int zsv_grad_norm_finalize(const void* partials_device, int64_t total_chunks, float max_norm,
                                      const zsv_scaler_state* state_device, zsv_clip_record* record_device, void* stream) {
    if (!partials_device || !record_device) return ZSV_E_NULL;
    if (total_chunks <= 0 || total_chunks > 0x7fffffffL || !(max_norm > 0.f)) return ZSV_E_BAD_SHAPE;
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)partials_device,
                       (long)total_chunks, max_norm, state_device, record_device);
    return launch_status();
}

extern "C" int zsv_grad_unscale_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks,
                                      zsv_scaler_state* state_device, void* stream) {
    if (!table_device || !state_device) return ZSV_E_NULL;
    if (bad_table(count, total_chunks)) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    hipLaunchKernelGGL(grad_unscale_multi_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device,
                       count, state_device);
    return launch_status();
}

extern "C" int zsv_adamw_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr, float beta1,
                               float beta2, float eps, double weight_decay, int32_t decoupled,
                               const zsv_clip_record* clip_device, int32_t step, void* stream) {
    if (!table_device) return ZSV_E_NULL;
    if (bad_table(count, total_chunks) || step <= 0) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    AdamwArgs a;
    if (!make_args(a, lr, beta1, beta2, eps, weight_decay, decoupled, clip_device)) return ZSV_E_BAD_SHAPE;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(adamw_multi_kernel<false>, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device,
                       count, a, (float)(lr / bc1), (float)(1.0 / sqrt(bc2)), AvgArgs{});
    return launch_status();
}

extern "C" int zsv_adamw_multi_scaled(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr,
                                      float beta1, float beta2, float eps, double weight_decay, int32_t decoupled,
                                      const zsv_clip_record* clip_device, const zsv_scaler_state* state_device,
                                      int32_t grads_unscaled, void* stream) {
    if (!table_device || !state_device) return ZSV_E_NULL;
    if (bad_table(count, total_chunks)) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    AdamwArgs a;
    if (!make_args(a, lr, beta1, beta2, eps, weight_decay, decoupled, clip_device)) return ZSV_E_BAD_SHAPE;
    hipLaunchKernelGGL(adamw_multi_scaled_kernel<false>, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream,
                       table_device, count, a, lr, state_device, grads_unscaled, AvgArgs{});
    return launch_status();
}

extern "C" int zsv_grad_accum_multi(const zsv_accum_tensor* table_device, int32_t count, int64_t total_chunks, float scale,
                                    int32_t assign, void* stream) {
    if (!table_device) return ZSV_E_NULL;
    if (bad_table(count, total_chunks)) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    hipLaunchKernelGGL(grad_accum_multi_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device,
                       count, scale, (int)assign);
    return launch_status();
}

// ---- weight averaging -------------------------------------------------------------------------------------------------------
static inline bool bad_avg(float* const* shadows_device, const zsv_avg_state* avg_state_device, float ema_weight) {
    return !shadows_device || !avg_state_device || !(ema_weight <= 1.f);          // (a NaN weight is refused too)
}

extern "C" int zsv_adam_multi_avg(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, float lr, float beta1,
                                  float beta2, float eps, int32_t step, float* const* shadows_device,
                                  const zsv_avg_state* avg_state_device, float ema_weight, void* stream) {
    if (!table_device) return ZSV_E_NULL;
    if (bad_table(count, total_chunks) || step <= 0) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    if (bad_avg(shadows_device, avg_state_device, ema_weight)) return shadows_device && avg_state_device ? ZSV_E_BAD_SHAPE : ZSV_E_NULL;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(adam_multi_avg_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device, count,
                       beta1, beta2, eps, (float)((double)lr / bc1), (float)(1.0 / sqrt(bc2)),
                       AvgArgs{shadows_device, avg_state_device, ema_weight});
    return launch_status();
}

extern "C" int zsv_adam_multi_scaled_avg(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, float lr,
                                         float beta1, float beta2, float eps, const zsv_scaler_state* state_device,
                                         float* const* shadows_device, const zsv_avg_state* avg_state_device,
                                         float ema_weight, void* stream) {
    if (!table_device || !state_device) return ZSV_E_NULL;
    if (bad_table(count, total_chunks)) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    if (bad_avg(shadows_device, avg_state_device, ema_weight)) return shadows_device && avg_state_device ? ZSV_E_BAD_SHAPE : ZSV_E_NULL;
    hipLaunchKernelGGL(adam_multi_scaled_avg_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device,
                       count, lr, beta1, beta2, eps, state_device, AvgArgs{shadows_device, avg_state_device, ema_weight});
    return launch_status();
}

extern "C" int zsv_adamw_multi_avg(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr,
                                   float beta1, float beta2, float eps, double weight_decay, int32_t decoupled,
                                   const zsv_clip_record* clip_device, int32_t step, float* const* shadows_device,
                                   const zsv_avg_state* avg_state_device, float ema_weight, void* stream) {
    if (!table_device) return ZSV_E_NULL;
    if (bad_table(count, total_chunks) || step <= 0) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    if (bad_avg(shadows_device, avg_state_device, ema_weight)) return shadows_device && avg_state_device ? ZSV_E_BAD_SHAPE : ZSV_E_NULL;
    AdamwArgs a;
    if (!make_args(a, lr, beta1, beta2, eps, weight_decay, decoupled, clip_device)) return ZSV_E_BAD_SHAPE;
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    hipLaunchKernelGGL(adamw_multi_kernel<true>, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device,
                       count, a, (float)(lr / bc1), (float)(1.0 / sqrt(bc2)), AvgArgs{shadows_device, avg_state_device, ema_weight});
    return launch_status();
}

extern "C" int zsv_adamw_multi_scaled_avg(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr,
                                          float beta1, float beta2, float eps, double weight_decay, int32_t decoupled,
                                          const zsv_clip_record* clip_device, const zsv_scaler_state* state_device,
                                          int32_t grads_unscaled, float* const* shadows_device,
                                          const zsv_avg_state* avg_state_device, float ema_weight, void* stream) {
    if (!table_device || !state_device) return ZSV_E_NULL;
    if (bad_table(count, total_chunks)) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    if (bad_avg(shadows_device, avg_state_device, ema_weight)) return shadows_device && avg_state_device ? ZSV_E_BAD_SHAPE : ZSV_E_NULL;
    AdamwArgs a;
    if (!make_args(a, lr, beta1, beta2, eps, weight_decay, decoupled, clip_device)) return ZSV_E_BAD_SHAPE;
    hipLaunchKernelGGL(adamw_multi_scaled_kernel<true>, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream,
                       table_device, count, a, lr, state_device, grads_unscaled,
                       AvgArgs{shadows_device, avg_state_device, ema_weight});
    return launch_status();
}

extern "C" int zsv_avg_multi(const zsv_pair_tensor* table_device, int32_t count, int64_t total_chunks,
                             const zsv_avg_state* avg_state_device, float ema_weight,
                             const zsv_scaler_state* scaler_state_device, void* stream) {
    if (!table_device || !avg_state_device) return ZSV_E_NULL;
    if (bad_table(count, total_chunks)) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    if (!(ema_weight <= 1.f)) return ZSV_E_BAD_SHAPE;
    hipLaunchKernelGGL(avg_multi_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device, count,
                       avg_state_device, ema_weight, scaler_state_device);
    return launch_status();
}

extern "C" int zsv_avg_advance(zsv_avg_state* avg_state_device, const zsv_scaler_state* scaler_state_device, void* stream) {
    if (!avg_state_device) return ZSV_E_NULL;
    hipLaunchKernelGGL(avg_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, avg_state_device, scaler_state_device);
    return launch_status();
}

extern "C" int zsv_swap_multi(const zsv_pair_tensor* table_device, int32_t count, int64_t total_chunks, void* stream) {
    if (!table_device) return ZSV_E_NULL;
    if (bad_table(count, total_chunks)) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    hipLaunchKernelGGL(swap_multi_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device, count);
    return launch_status();
}
