// optim.hip -- the multi-tensor optimiser step (include/zsv_hip.h): Adam with all its options, the loss scaler, the gradient
// norm, gradient accumulation and weight averaging.  (SGD: sgd.hip.  The single-tensor zsv_adam_step: elementwise_pool.hip.)
//
//   torch                                          here
//   Adam.step() over every parameter               adam_multi_kernel<DECAY_CLIP, SCALED, AVG>: ONE kernel template behind the eight
//                                                  zsv_adam[w]_multi[_scaled][_avg] entry points, one launch per table
//   GradScaler.step / .update                      grad_check_multi (found_inf), the SCALED forms (skipped on found_inf, 1/scale
//                                                  folded into the gradient read, step number read on the device), scaler_update
//   clip_grad_norm_(params, max_norm)              grad_norm_multi (sum of squares per 4096-element chunk, + the non-finite
//                                                  check of the loss scaler) and grad_norm_finalize (fixed-order sum in double,
//                                                  1/scale, {total_norm, clip_coef}); the coefficient is applied on the
//                                                  gradient's way into the update, the gradients in memory are not rewritten
//   Adam(weight_decay=) / AdamW                    the DECAY_CLIP forms (zsv_adamw_multi*)
//   GradScaler.unscale_                            grad_unscale_multi
//   k x loss.backward() accumulating into .grad    grad_accum_multi (table of {acc, g}: acc = [acc +] scale * g, one launch per
//                                                  gradient bucket and backward pass; ddp.GradientSync)
//   swa_utils.AveragedModel.update_parameters      the AVG forms (the shadow is updated with the parameter value still in a
//                                                  register), avg_multi for BatchNorm running statistics, avg_advance (the
//                                                  device-resident count), swap_multi
//
// All of them walk a descriptor table the same way (multi_tensor.h): one workgroup of 256 threads per chunk, a binary search
// over first_chunk; what every entry point refuses of a table (bad_table, bad_rate) is there too.  The per-element Adam updates
// and the averaging rule are adam_update.h.  No floating-point atomics: every sum has a fixed order, so the same gradients give
// the same norm bits and the same parameter bits on every run.
//
// lr: the four zsv_adam_multi* entry points take it as float, the four zsv_adamw_multi* as double, and both families form
// lr / (1 - beta1^step) in double -- of (double)(float)lr in the first, which is what their callers have always got.
#include "zsv_common.h"
#include "zsv_hip.h"
#include "multi_tensor.h"
#include "adam_update.h"

#include <math.h>

namespace zsv {

// ---- the loss scaler: found_inf |= any non-finite gradient; scaler.update() -----------------------------------------------------
__global__ __launch_bounds__(256) void grad_check_multi_kernel(const zsv_adam_tensor* __restrict__ table, int count,
                                                               zsv_scaler_state* __restrict__ st) {
    const long chunk = blockIdx.x;
    const zsv_adam_tensor t = find_tensor(table, count, chunk);
    const Span s = chunk_span(t, chunk);
    bool bad = false;
    for (long i = s.base + threadIdx.x; i < s.end; i += 256) bad |= non_finite(t.g[i]);
    if (__any(bad) && (threadIdx.x & 63) == 0) st->found_inf = 1;   // benign race: every writer stores 1
}

// _amp_update_scale_ (backoff / growth) + steps_done += !found_inf, found_inf = 0
__global__ void scaler_update_kernel(zsv_scaler_state* st, float growth, float backoff, int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st->found_inf) {
        st->scale *= backoff;
        st->growth_tracker = 0;
    } else {
        const int ok = st->growth_tracker + 1;
        if (ok == interval) {
            const float grown = st->scale * growth;
            if (!non_finite(grown)) st->scale = grown;              // torch keeps the old scale if growth overflows
            st->growth_tracker = 0;
        } else {
            st->growth_tracker = ok;
        }
        st->steps_done += 1;
    }
    st->found_inf = 0;
}

// ---- the gradient norm and unscale_ ---------------------------------------------------------------------------------------------
// partials[blockIdx.x] = sum of g^2 over the chunk: <= 16 serial adds per lane, then a fixed 8-level tree over 256 lanes.
__global__ __launch_bounds__(256) void grad_norm_multi_kernel(const zsv_adam_tensor* __restrict__ table, int count,
                                                              float* __restrict__ partials, zsv_scaler_state* __restrict__ st) {
    __shared__ float red[4];
    const long chunk = blockIdx.x;
    const zsv_adam_tensor t = find_tensor(table, count, chunk);
    const Span span = chunk_span(t, chunk);
    float s = 0.f;
    bool bad = false;
    for (long i = span.base + threadIdx.x; i < span.end; i += 256) {
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
    const Span span = chunk_span(t, chunk);
    float* g = const_cast<float*>(t.g);
    bool bad = false;
    for (long i = span.base + threadIdx.x; i < span.end; i += 256) {
        const float gi = g[i];
        bad |= non_finite(gi);
        g[i] = gi * inv_scale;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) st->found_inf = 1;
}

// ---- Adam: one kernel template, one argument struct --------------------------------------------------------------------------
// What a form does not use stays unset and is never read: the flags are compile-time, so an instantiation holds the loads and
// the arithmetic of its options and nothing else.
struct AdamArgs {
    double lr;                          // SCALED: step_size is formed on the device, from the scaler's count of steps taken
    float b1, b2, eps;
    int grads_unscaled;                 // DECAY_CLIP && SCALED: zsv_grad_unscale_multi has already run on this table
    const zsv_scaler_state* st;         // SCALED
    const zsv_clip_record* clip;        // DECAY_CLIP; NULL: no clipping
    AdamDecay decay;                    // DECAY_CLIP
    float ema_weight;                   // AVG; >= 0: EMA weight of the new value; < 0: equal-weight
    float* const* shadows;              // AVG: count pointers, parallel to the table
    const zsv_avg_state* avg;           // AVG
};

// step_size = lr / (1 - b1^step) and inv_sqrt_bc2 = 1 / sqrt(1 - b2^step) come from the host, formed in double, in the !SCALED
// forms.  They are arguments of their own and not fields of AdamArgs: which product of `b1 * m + (1 - b1) * g` the compiler
// contracts into the fma depends on it, and this is the choice every build so far has made.
template <bool DECAY_CLIP, bool SCALED, bool AVG>
__global__ __launch_bounds__(256) void adam_multi_kernel(const zsv_adam_tensor* __restrict__ table, int count, AdamArgs a,
                                                         float step_size, float inv_sqrt_bc2) {
    float inv_scale = 1.f;
    if (SCALED) {
        if (a.st->found_inf) return;           // scaler.step skips optimizer.step: weight decay and the average included
        if (!(DECAY_CLIP && a.grads_unscaled)) inv_scale = (float)(1.0 / (double)a.st->scale);   // scale.double().reciprocal().float()
        const int step = a.st->steps_done + 1;
        step_size = (float)(a.lr / (1.0 - pow((double)a.b1, (double)step)));
        inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)a.b2, (double)step)));
    }
    const float clip = DECAY_CLIP && a.clip != nullptr ? a.clip->clip_coef : 1.f;
    const long chunk = blockIdx.x;
    const int index = find_index(table, count, chunk);
    const zsv_adam_tensor t = table[index];
    float* shadow = nullptr;
    AvgWeight k{};
    if (AVG) {
        shadow = a.shadows[index];
        k = avg_weight(a.avg, a.ema_weight);
    }
    const Span s = chunk_span(t, chunk);
    for (long i = s.base + threadIdx.x; i < s.end; i += 256) {
        if (DECAY_CLIP)
            adamw_element<AVG>(t, i, inv_scale, clip, a.decay, a.b1, a.b2, a.eps, step_size, inv_sqrt_bc2, shadow, k);
        else            // the unscaled plain form has no product on the gradient at all
            adam_element<AVG>(t, i, SCALED ? t.g[i] * inv_scale : t.g[i], a.b1, a.b2, a.eps, step_size, inv_sqrt_bc2, shadow, k);
    }
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
    const zsv_pair_tensor t = find_tensor(table, count, chunk);
    const Span s = chunk_span(t, chunk);
    if (s.base >= s.end) return;
    const int len = (int)(s.end - s.base);
    float* __restrict__ a = t.a + s.base;
    float* __restrict__ b = t.b + s.base;

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
    const zsv_accum_tensor t = find_tensor(table, count, chunk);
    const Span s = chunk_span(t, chunk);
    if (s.base >= s.end) return;
    const int len = (int)(s.end - s.base);
    float* __restrict__ acc = t.acc + s.base;
    const float* __restrict__ g = t.g + s.base;
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

// ---- the host half of every Adam launch ------------------------------------------------------------------------------------------
static inline AdamArgs adam_args(double lr, float beta1, float beta2, float eps) {
    AdamArgs a{};                       // every pointer NULL until an entry point sets it
    a.lr = lr;
    a.b1 = beta1;
    a.b2 = beta2;
    a.eps = eps;
    return a;
}

// Validates in the order every entry point has always used -- NULL table / scaler state; an empty table is fine; the table's shape
// (and the step number, which only the unscaled forms take); the averaging arguments; lr and weight_decay, which only the
// DECAY_CLIP forms check -- and launches the instantiation the three flags name.
static int adam_launch(bool decay_clip, bool scaled, bool avg, const zsv_adam_tensor* table, int32_t count, int64_t total_chunks,
                       AdamArgs a, double weight_decay, int32_t decoupled, int32_t step, void* stream) {
    if (!table || (scaled && !a.st)) return ZSV_E_NULL;
    if (bad_table(count, total_chunks) || (!scaled && step <= 0)) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    if (avg) {
        if (!a.shadows || !a.avg) return ZSV_E_NULL;
        if (!(a.ema_weight <= 1.f)) return ZSV_E_BAD_SHAPE;                 // (a NaN weight is refused too)
    }
    a.decay = AdamDecay{0.f, 1.f, 0};
    if (decay_clip) {
        if (bad_rate(a.lr) || bad_rate(weight_decay)) return ZSV_E_BAD_SHAPE;
        a.decay.decoupled = decoupled != 0 && weight_decay != 0.0;
        if (a.decay.decoupled) a.decay.decay_factor = (float)(1.0 - a.lr * weight_decay);
        else a.decay.wd_l2 = (float)weight_decay;
    }
    float step_size = 0.f, inv_sqrt_bc2 = 0.f;                              // SCALED: formed on the device
    if (!scaled) {
        step_size = (float)(a.lr / (1.0 - pow((double)a.b1, (double)step)));
        inv_sqrt_bc2 = (float)(1.0 / sqrt(1.0 - pow((double)a.b2, (double)step)));
    }
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table, count, a, step_size,
                           inv_sqrt_bc2);
    };
    switch ((decay_clip ? 4 : 0) | (scaled ? 2 : 0) | (avg ? 1 : 0)) {
        case 0: launch(adam_multi_kernel<false, false, false>); break;
        case 1: launch(adam_multi_kernel<false, false, true>); break;
        case 2: launch(adam_multi_kernel<false, true, false>); break;
        case 3: launch(adam_multi_kernel<false, true, true>); break;
        case 4: launch(adam_multi_kernel<true, false, false>); break;
        case 5: launch(adam_multi_kernel<true, false, true>); break;
        case 6: launch(adam_multi_kernel<true, true, false>); break;
        case 7: launch(adam_multi_kernel<true, true, true>); break;
    }
    return launch_status();
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

extern "C" int zsv_grad_accum_multi(const zsv_accum_tensor* table_device, int32_t count, int64_t total_chunks, float scale,
                                    int32_t assign, void* stream) {
    if (!table_device) return ZSV_E_NULL;
    if (bad_table(count, total_chunks)) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    hipLaunchKernelGGL(grad_accum_multi_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device,
                       count, scale, (int)assign);
    return launch_status();
}

// ---- the loss scaler ------------------------------------------------------------------------------------------------------------
extern "C" int zsv_grad_check_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks,
                                    zsv_scaler_state* state_device, void* stream) {
    if (!table_device || !state_device) return ZSV_E_NULL;
    if (bad_table(count, total_chunks)) return count == 0 ? ZSV_OK : ZSV_E_BAD_SHAPE;
    hipLaunchKernelGGL(grad_check_multi_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device,
                       count, state_device);
    return launch_status();
}

extern "C" int zsv_scaler_update(zsv_scaler_state* state_device, float growth_factor, float backoff_factor,
                                 int32_t growth_interval, void* stream) {
    if (!state_device) return ZSV_E_NULL;
    if (!(growth_factor > 1.f) || !(backoff_factor > 0.f && backoff_factor < 1.f) || growth_interval <= 0) return ZSV_E_BAD_SHAPE;
    hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state_device, growth_factor,
                       backoff_factor, growth_interval);
    return launch_status();
}

// ---- Adam: the eight entry points fill AdamArgs; adam_launch does the rest --------------------------------------------------------
// (a float `lr` widens here, exactly: the header comment)
extern "C" int zsv_adam_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, float lr, float beta1,
                              float beta2, float eps, int32_t step, void* stream) {
    return adam_launch(false, false, false, table_device, count, total_chunks, adam_args(lr, beta1, beta2, eps), 0.0, 0, step, stream);
}

extern "C" int zsv_adam_multi_scaled(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, float lr,
                                     float beta1, float beta2, float eps, const zsv_scaler_state* state_device, void* stream) {
    AdamArgs a = adam_args(lr, beta1, beta2, eps);
    a.st = state_device;
    return adam_launch(false, true, false, table_device, count, total_chunks, a, 0.0, 0, 0, stream);
}

extern "C" int zsv_adamw_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr, float beta1,
                               float beta2, float eps, double weight_decay, int32_t decoupled,
                               const zsv_clip_record* clip_device, int32_t step, void* stream) {
    AdamArgs a = adam_args(lr, beta1, beta2, eps);
    a.clip = clip_device;
    return adam_launch(true, false, false, table_device, count, total_chunks, a, weight_decay, decoupled, step, stream);
}

extern "C" int zsv_adamw_multi_scaled(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr,
                                      float beta1, float beta2, float eps, double weight_decay, int32_t decoupled,
                                      const zsv_clip_record* clip_device, const zsv_scaler_state* state_device,
                                      int32_t grads_unscaled, void* stream) {
    AdamArgs a = adam_args(lr, beta1, beta2, eps);
    a.clip = clip_device;
    a.st = state_device;
    a.grads_unscaled = grads_unscaled;
    return adam_launch(true, true, false, table_device, count, total_chunks, a, weight_decay, decoupled, 0, stream);
}

static inline void set_average(AdamArgs& a, float* const* shadows_device, const zsv_avg_state* avg_state_device, float ema_weight) {
    a.shadows = shadows_device;
    a.avg = avg_state_device;
    a.ema_weight = ema_weight;
}

extern "C" int zsv_adam_multi_avg(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, float lr, float beta1,
                                  float beta2, float eps, int32_t step, float* const* shadows_device,
                                  const zsv_avg_state* avg_state_device, float ema_weight, void* stream) {
    AdamArgs a = adam_args(lr, beta1, beta2, eps);
    set_average(a, shadows_device, avg_state_device, ema_weight);
    return adam_launch(false, false, true, table_device, count, total_chunks, a, 0.0, 0, step, stream);
}

extern "C" int zsv_adam_multi_scaled_avg(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, float lr,
                                         float beta1, float beta2, float eps, const zsv_scaler_state* state_device,
                                         float* const* shadows_device, const zsv_avg_state* avg_state_device,
                                         float ema_weight, void* stream) {
    AdamArgs a = adam_args(lr, beta1, beta2, eps);
    a.st = state_device;
    set_average(a, shadows_device, avg_state_device, ema_weight);
    return adam_launch(false, true, true, table_device, count, total_chunks, a, 0.0, 0, 0, stream);
}

extern "C" int zsv_adamw_multi_avg(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr,
                                   float beta1, float beta2, float eps, double weight_decay, int32_t decoupled,
                                   const zsv_clip_record* clip_device, int32_t step, float* const* shadows_device,
                                   const zsv_avg_state* avg_state_device, float ema_weight, void* stream) {
    AdamArgs a = adam_args(lr, beta1, beta2, eps);
    a.clip = clip_device;
    set_average(a, shadows_device, avg_state_device, ema_weight);
    return adam_launch(true, false, true, table_device, count, total_chunks, a, weight_decay, decoupled, step, stream);
}

extern "C" int zsv_adamw_multi_scaled_avg(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr,
                                          float beta1, float beta2, float eps, double weight_decay, int32_t decoupled,
                                          const zsv_clip_record* clip_device, const zsv_scaler_state* state_device,
                                          int32_t grads_unscaled, float* const* shadows_device,
                                          const zsv_avg_state* avg_state_device, float ema_weight, void* stream) {
    AdamArgs a = adam_args(lr, beta1, beta2, eps);
    a.clip = clip_device;
    a.st = state_device;
    a.grads_unscaled = grads_unscaled;
    set_average(a, shadows_device, avg_state_device, ema_weight);
    return adam_launch(true, true, true, table_device, count, total_chunks, a, weight_decay, decoupled, 0, stream);
}

// ---- weight averaging on its own ------------------------------------------------------------------------------------------------

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
