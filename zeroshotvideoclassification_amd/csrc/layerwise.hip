// layerwise.hip -- LARS and LAMB: the SGD and Adam rules with every tensor's update scaled by a trust ratio built from two
// 2-norms over that tensor (include/zsv_hip.h: zsv_layerwise_*, zsv_lars_norms, zsv_lamb_*).  Three passes per parameter group
// over the zsv_adam_tensor table of zsv_adam_multi, none of which meets the host:
//
//   partials   one workgroup of 256 per 4096-element chunk (multi_tensor.h) leaves {sum p^2, sum q^2} of its chunk.
//              LARS: q = g as it lies in memory (the scalar factors 1/scale and clip_coef are applied to the norm in the finalize).
//              LAMB: the pass updates m and v in place and forms u = mhat / (sqrt(vhat) + eps) + wd * p, so q = u; u is not stored.
//   finalize   one workgroup per TENSOR sums the partials of its chunks [first_chunk, first_chunk + ceil(n / 4096)) in double in a
//              fixed order and writes the record {p_norm, q_norm, ratio}.
//   apply      one workgroup per chunk again; the chunk finds its tensor by the binary search it always used and reads
//              records[index].ratio.  LARS: zsv_lars_multi, which is sgd.hip's -- the kernel of zsv_sgd_multi with the ratio
//              compiled in.  LAMB, here: u is recomputed from the updated m, v and the old p by the very function the first pass
//              ran (lamb_u, contraction off), p -= lr * ratio * u.
//
// HBM-bound like sgd.hip, so every array moves 16 bytes per lane where its own base is 16-byte aligned and 4 bytes per lane
// otherwise.  Both forms walk a chunk as 1024 quads of four consecutive elements, quad v belonging to lane v mod 256, and run the
// same body on registers: which elements a lane sums, and in which order (<= 16 serial adds, then the fixed 8-level tree of
// block_sum_256), does not depend on the alignment, so neither do the bits.  (The LARS apply has no sum to keep in order and walks
// a chunk sgd.hip's way, which is the faster one for a chunk with an array off the boundary.)  No atomics: the same inputs give
// the same bits on every run.  No element outside [0, n) of any array is read or written, and nothing outside the workspace.
//
// Under the loss scaler every pass returns on found_inf before it touches m, v, buf, p, the shadows or the records.
#include "zsv_common.h"
#include "zsv_hip.h"
#include "multi_tensor.h"
#include "adam_update.h"

#include <math.h>

namespace zsv {
namespace layerwise {
// quad v of an array: elements [4 v, 4 v + valid), valid in 1..4 (less than 4 only in the last quad of a tensor)
__device__ __forceinline__ v4f load4(const float* __restrict__ a, int v, int valid, bool vec) {
    if (vec && valid == 4) return reinterpret_cast<const v4f*>(a)[v];
    v4f r = v4f{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < valid) r[e] = a[4 * v + e];
    return r;
}

__device__ __forceinline__ void store4(float* __restrict__ a, int v, int valid, bool vec, v4f x) {
    if (vec && valid == 4) {
        reinterpret_cast<v4f*>(a)[v] = x;
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (e < valid) a[4 * v + e] = x[e];
}

// the shadow of the weight average after the new parameter values p4 (adam_update.h's rule)
__device__ __forceinline__ void average4(float* __restrict__ shadow, int v, int valid, bool vec, v4f p4, const AvgWeight k) {
    v4f s4 = p4;
    if (!k.copy) {
        s4 = load4(shadow, v, valid, vec);
#pragma unroll
        for (int e = 0; e < 4; ++e) s4[e] = avg_value(s4[e], p4[e], k);
    }
    store4(shadow, v, valid, vec, s4);
}

// ---- LARS -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lars_norms_kernel(const zsv_adam_tensor* __restrict__ table, int count,
                                                         float* __restrict__ partials, const zsv_scaler_state* __restrict__ st) {
    __shared__ float red[4];
    if (st != nullptr && st->found_inf) return;
    const long chunk = blockIdx.x;
    const zsv_adam_tensor t = find_tensor(table, count, chunk);
    const Span span = chunk_span(t, chunk);
    const int len = span.base < span.end ? (int)(span.end - span.base) : 0;
    const float* __restrict__ p = t.p + span.base;
    const float* __restrict__ g = t.g + span.base;
    const bool pv = vec16(p), gv = vec16(g);
    float sp = 0.f, sg = 0.f;
    const int quads = (len + 3) >> 2;
    for (int v = threadIdx.x; v < quads; v += 256) {
        const int valid = min(4, len - 4 * v);
        const v4f p4 = load4(p, v, valid, pv), g4 = load4(g, v, valid, gv);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < valid) {
                sp += p4[e] * p4[e];
                sg += g4[e] * g4[e];
            }
    }
    const float tp = block_sum_256<float>(sp, red);
    const float tg = block_sum_256<float>(sg, red);
    if (threadIdx.x == 0) {
        partials[2 * chunk] = tp;
        partials[2 * chunk + 1] = tg;
    }
}

// ---- LAMB -------------------------------------------------------------------------------------------------------------------
struct LambArgs {
    float b1, b2, one_minus_b1, one_minus_b2, eps, wd, lr;
    float bc1, bc2;                     // 1 - beta^t formed on the host in double; under a scaler formed on the device
    int grads_unscaled;
    const zsv_clip_record* clip;        // NULL: no clipping
    const zsv_scaler_state* st;         // NULL: no loss scaler
    float* const* shadows;              // NULL: no averaging
    const zsv_avg_state* avg;
    float ema_weight;
};

struct LambStep {
    float inv_scale, clip, bc1, bc2;
};

// what a workgroup of either LAMB pass reads once: the two passes of a step form the same four numbers
__device__ __forceinline__ LambStep lamb_step(const LambArgs& a) {
    LambStep s;
    s.inv_scale = a.st != nullptr && !a.grads_unscaled ? (float)(1.0 / (double)a.st->scale) : 1.f;
    s.clip = a.clip != nullptr ? a.clip->clip_coef : 1.f;
    s.bc1 = a.bc1;
    s.bc2 = a.bc2;
    if (a.st != nullptr) {                                // t = steps taken + 1, the scaler's device-resident count
        const int step = a.st->steps_done + 1;
        s.bc1 = (float)(1.0 - pow((double)a.b1, (double)step));
        s.bc2 = (float)(1.0 - pow((double)a.b2, (double)step));
    }
    return s;
}

// u of one element from the UPDATED moments and the OLD parameter.  Both passes call this: no contraction, explicit fma, so the
// bits do not depend on the code around the call.
__device__ __forceinline__ float lamb_u(float m, float v, float p, const LambArgs& a, const LambStep& s) {
#pragma clang fp contract(off)
    const float mh = m / s.bc1;
    const float vh = v / s.bc2;
    const float u = mh / (sqrtf(vh) + a.eps);
    return a.wd != 0.f ? fmaf(a.wd, p, u) : u;
}

__global__ __launch_bounds__(256) void lamb_moments_kernel(const zsv_adam_tensor* __restrict__ table, int count,
                                                           float* __restrict__ partials, LambArgs a) {
    __shared__ float red[4];
    if (a.st != nullptr && a.st->found_inf) return;
    const LambStep s = lamb_step(a);
    const long chunk = blockIdx.x;
    const zsv_adam_tensor t = find_tensor(table, count, chunk);
    const Span span = chunk_span(t, chunk);
    const int len = span.base < span.end ? (int)(span.end - span.base) : 0;
    const float* __restrict__ p = t.p + span.base;
    const float* __restrict__ g = t.g + span.base;
    float* __restrict__ m = t.exp_avg + span.base;
    float* __restrict__ vv = t.exp_avg_sq + span.base;
    const bool pv = vec16(p), gv = vec16(g), mv = vec16(m), vvv = vec16(vv);
    float sp = 0.f, su = 0.f;
    const int quads = (len + 3) >> 2;
#pragma unroll 2
    for (int q = threadIdx.x; q < quads; q += 256) {
        const int valid = min(4, len - 4 * q);
        const v4f p4 = load4(p, q, valid, pv), g4 = load4(g, q, valid, gv);
        v4f m4 = load4(m, q, valid, mv), v4 = load4(vv, q, valid, vvv);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            {
#pragma clang fp contract(off)
                float gi = g4[e] * s.inv_scale;           // two separate fp32 products, as unscale_ and clip_grad_norm_ store them
                gi = gi * s.clip;
                m4[e] = fmaf(a.b1, m4[e], a.one_minus_b1 * gi);
                v4[e] = fmaf(a.b2, v4[e], (a.one_minus_b2 * gi) * gi);
            }
            if (e < valid) {
                const float u = lamb_u(m4[e], v4[e], p4[e], a, s);
                sp += p4[e] * p4[e];
                su += u * u;
            }
        }
        store4(m, q, valid, mv, m4);
        store4(vv, q, valid, vvv, v4);
    }
    const float tp = block_sum_256<float>(sp, red);
    const float tu = block_sum_256<float>(su, red);
    if (threadIdx.x == 0) {
        partials[2 * chunk] = tp;
        partials[2 * chunk + 1] = tu;
    }
}

__global__ __launch_bounds__(256) void lamb_multi_kernel(const zsv_adam_tensor* __restrict__ table, int count,
                                                         const zsv_layer_record* __restrict__ records, LambArgs a) {
    if (a.st != nullptr && a.st->found_inf) return;
    const LambStep s = lamb_step(a);
    const long chunk = blockIdx.x;
    const int index = find_index(table, count, chunk);
    const zsv_adam_tensor t = table[index];
    const Span span = chunk_span(t, chunk);
    if (span.base >= span.end) return;
    const int len = (int)(span.end - span.base);
    const float step_size = a.lr * records[index].ratio;
    float* __restrict__ p = t.p + span.base;
    const float* __restrict__ m = t.exp_avg + span.base;
    const float* __restrict__ vv = t.exp_avg_sq + span.base;
    float* __restrict__ shadow = a.shadows != nullptr ? a.shadows[index] + span.base : nullptr;
    AvgWeight k{};
    if (shadow != nullptr) k = avg_weight(a.avg, a.ema_weight);
    const bool pv = vec16(p), mv = vec16(m), vvv = vec16(vv), sv = vec16(shadow);

    const int quads = (len + 3) >> 2;
#pragma unroll 2
    for (int q = threadIdx.x; q < quads; q += 256) {
        const int valid = min(4, len - 4 * q);
        v4f p4 = load4(p, q, valid, pv);
        const v4f m4 = load4(m, q, valid, mv), v4 = load4(vv, q, valid, vvv);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < valid) p4[e] = fmaf(-step_size, lamb_u(m4[e], v4[e], p4[e], a, s), p4[e]);
        store4(p, q, valid, pv, p4);
        if (shadow != nullptr) average4(shadow, q, valid, sv, p4, k);
    }
}

// ---- the segmented finalize: one workgroup per tensor -----------------------------------------------------------------------------
struct FinalizeArgs {
    int lamb;                           // 0: LARS, 1: LAMB
    int adapt;                          // 0: every ratio is 1 (the norms are still recorded)
    double trust_coefficient, wd, eps;  // LARS
    double trust_clip;                  // LAMB; <= 0: none
    int grads_unscaled;
    const zsv_clip_record* clip;        // LARS: the gradient norm takes the factors the update applies per element
    const zsv_scaler_state* st;
};

// lane k sums the partials of chunks first + k, first + k + 256, ... of ITS tensor in double, then the fixed tree: the way
// grad_norm_finalize_kernel sums the whole table.
__global__ __launch_bounds__(256) void finalize_kernel(const zsv_adam_tensor* __restrict__ table, const float* __restrict__ partials,
                                                       zsv_layer_record* __restrict__ records, FinalizeArgs a) {
    __shared__ double red[4];
    if (a.st != nullptr && a.st->found_inf) return;
    const int index = blockIdx.x;
    const long first = table[index].first_chunk;
    const long chunks = (table[index].n + CHUNK - 1) / CHUNK;
    double sp = 0.0, sq = 0.0;
    for (long c = threadIdx.x; c < chunks; c += 256) {
        sp += (double)partials[2 * (first + c)];
        sq += (double)partials[2 * (first + c) + 1];
    }
    sp = block_sum_256<double>(sp, red);
    sq = block_sum_256<double>(sq, red);
    if (threadIdx.x != 0) return;
    const double pn = sqrt(sp);
    double qn = sqrt(sq);
    double ratio = 1.0;
    if (a.lamb) {
        if (a.adapt && pn > 0.0 && qn > 0.0) ratio = pn / qn;
        if (a.trust_clip > 0.0 && ratio > a.trust_clip) ratio = a.trust_clip;
    } else {
        if (a.st != nullptr && !a.grads_unscaled) qn *= (double)(float)(1.0 / (double)a.st->scale);   // the gradients in memory are scaled
        if (a.clip != nullptr) qn *= (double)a.clip->clip_coef;
        if (a.adapt && pn > 0.0 && qn > 0.0) ratio = a.trust_coefficient * pn / (qn + a.wd * pn + a.eps);
    }
    records[index].p_norm = (float)pn;
    records[index].q_norm = (float)qn;
    records[index].ratio = (float)ratio;
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static inline size_t records_bytes(int64_t count) { return ((size_t)count * sizeof(zsv_layer_record) + 15) & ~(size_t)15; }

struct Workspace {
    zsv_layer_record* records;          // of this table's first tensor
    float* partials;                    // of this table's first chunk
};

// NULL, then shape, then size: every refusal before any launch
static int resolve(const void* table, void* workspace, size_t workspace_bytes, int32_t count, int64_t total_chunks,
                   int64_t chunk_offset, int32_t tensor_offset, int32_t all_count, Workspace& w) {
    if (!table || !workspace) return ZSV_E_NULL;
    if (bad_table(count, total_chunks) || chunk_offset < 0 || tensor_offset < 0 || chunk_offset + total_chunks > 0x7fffffffL ||
        (int64_t)tensor_offset + count > (int64_t)all_count)
        return ZSV_E_BAD_SHAPE;
    if (workspace_bytes < zsv_layerwise_workspace_bytes(chunk_offset + total_chunks, all_count)) return ZSV_E_WORKSPACE;
    w.records = (zsv_layer_record*)workspace + tensor_offset;
    w.partials = (float*)((char*)workspace + records_bytes(all_count)) + 2 * chunk_offset;
    return ZSV_OK;
}

}  // namespace layerwise
}  // namespace zsv

using namespace zsv;
using namespace zsv::layerwise;

extern "C" size_t zsv_layerwise_workspace_bytes(int64_t total_chunks, int32_t count) {
    if (total_chunks <= 0 || count <= 0) return 0;
    return records_bytes(count) + (size_t)total_chunks * 2 * sizeof(float);
}

extern "C" int zsv_lars_norms(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, int64_t chunk_offset,
                              int32_t tensor_offset, int32_t all_count, void* workspace_device, size_t workspace_bytes,
                              const zsv_scaler_state* state_device, void* stream) {
    Workspace w;
    const int status = resolve(table_device, workspace_device, workspace_bytes, count, total_chunks, chunk_offset, tensor_offset,
                               all_count, w);
    if (status != ZSV_OK) return status;
    hipLaunchKernelGGL(lars_norms_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device, count,
                       w.partials, state_device);
    return launch_status();
}

static int lamb_args(LambArgs& a, double lr, float beta1, float beta2, float eps, double weight_decay,
                     const zsv_clip_record* clip_device, const zsv_scaler_state* state_device, int32_t grads_unscaled, int32_t step) {
    if (bad_rate(lr) || bad_rate(weight_decay) || !(eps >= 0.f) || !isfinite(eps)) return ZSV_E_BAD_SHAPE;
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return ZSV_E_BAD_SHAPE;
    if (state_device == nullptr && step <= 0) return ZSV_E_BAD_SHAPE;
    a = LambArgs{};
    a.b1 = beta1;
    a.b2 = beta2;
    a.one_minus_b1 = (float)(1.0 - (double)beta1);
    a.one_minus_b2 = (float)(1.0 - (double)beta2);
    a.eps = eps;
    a.wd = (float)weight_decay;
    a.lr = (float)lr;
    if (state_device == nullptr) {
        a.bc1 = (float)(1.0 - pow((double)beta1, (double)step));
        a.bc2 = (float)(1.0 - pow((double)beta2, (double)step));
    }
    a.grads_unscaled = grads_unscaled != 0;
    a.clip = clip_device;
    a.st = state_device;
    return ZSV_OK;
}

extern "C" int zsv_lamb_moments(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, int64_t chunk_offset,
                                int32_t tensor_offset, int32_t all_count, void* workspace_device, size_t workspace_bytes,
                                float beta1, float beta2, float eps, double weight_decay, const zsv_clip_record* clip_device,
                                const zsv_scaler_state* state_device, int32_t grads_unscaled, int32_t step, void* stream) {
    Workspace w;
    int status = resolve(table_device, workspace_device, workspace_bytes, count, total_chunks, chunk_offset, tensor_offset,
                         all_count, w);
    if (status != ZSV_OK) return status;
    LambArgs a;
    status = lamb_args(a, 0.0, beta1, beta2, eps, weight_decay, clip_device, state_device, grads_unscaled, step);
    if (status != ZSV_OK) return status;
    hipLaunchKernelGGL(lamb_moments_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device, count,
                       w.partials, a);
    return launch_status();
}

extern "C" int zsv_layerwise_finalize(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks,
                                      int64_t chunk_offset, int32_t tensor_offset, int32_t all_count, void* workspace_device,
                                      size_t workspace_bytes, int32_t lamb, int32_t adapt, double trust_coefficient,
                                      double weight_decay, double eps, double trust_clip, const zsv_clip_record* clip_device,
                                      const zsv_scaler_state* state_device, int32_t grads_unscaled, void* stream) {
    Workspace w;
    const int status = resolve(table_device, workspace_device, workspace_bytes, count, total_chunks, chunk_offset, tensor_offset,
                               all_count, w);
    if (status != ZSV_OK) return status;
    if (!lamb && (!(trust_coefficient > 0.0) || !isfinite(trust_coefficient) || bad_rate(weight_decay) || bad_rate(eps)))
        return ZSV_E_BAD_SHAPE;
    if (lamb && trust_clip != trust_clip) return ZSV_E_BAD_SHAPE;
    FinalizeArgs a{};
    a.lamb = lamb != 0;
    a.adapt = adapt != 0;
    a.trust_coefficient = trust_coefficient;
    a.wd = weight_decay;
    a.eps = eps;
    a.trust_clip = trust_clip;
    a.grads_unscaled = grads_unscaled != 0;
    a.clip = clip_device;
    a.st = state_device;
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)count), dim3(256), 0, (hipStream_t)stream, table_device, w.partials,
                       w.records, a);
    return launch_status();
}

extern "C" int zsv_lamb_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks,
                              const zsv_layer_record* records_device, double lr, float beta1, float beta2, float eps,
                              double weight_decay, const zsv_scaler_state* state_device, int32_t step, float* const* shadows_device,
                              const zsv_avg_state* avg_state_device, float ema_weight, void* stream) {
    if (!table_device || !records_device) return ZSV_E_NULL;
    if ((shadows_device == nullptr) != (avg_state_device == nullptr)) return ZSV_E_NULL;
    if (bad_table(count, total_chunks)) return ZSV_E_BAD_SHAPE;
    if (shadows_device != nullptr && !(ema_weight <= 1.f)) return ZSV_E_BAD_SHAPE;
    LambArgs a;
    const int status = lamb_args(a, lr, beta1, beta2, eps, weight_decay, nullptr, state_device, 0, step);
    if (status != ZSV_OK) return status;
    a.shadows = shadows_device;
    a.avg = avg_state_device;
    a.ema_weight = ema_weight;
    hipLaunchKernelGGL(lamb_multi_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table_device, count,
                       records_device, a);
    return launch_status();
}
