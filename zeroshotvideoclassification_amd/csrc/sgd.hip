// sgd.hip -- torch.optim.SGD (momentum, dampening, Nesterov, L2 weight decay, maximize) over the zsv_adam_tensor table of
// zsv_adam_multi, with the loss scaler, the clip coefficient and the weight average folded into the same launch, and LARS, the
// same rule with every tensor's g + wd * p scaled by a trust ratio (include/zsv_hip.h: zsv_sgd_multi, zsv_lars_multi; the ratio
// comes from the records layerwise.hip leaves).  ONE kernel template behind both entry points, and what a step does not use is
// a NULL pointer, tested once per workgroup.
//
// One workgroup of 256 threads per 4096-element chunk, found through multi_tensor.h as in optim.hip; the averaging rule is
// adam_update.h's.  The pass is HBM-bound (read p, g, buf, write p, buf: 20 bytes per element, 28 with the average), so the body
// moves 16 bytes per lane:
//   * every pointer of the tensor (p, g, and buf / shadow where present) 16-byte aligned at the chunk's base -- a chunk is 16 KiB,
//     so that is the alignment of the tensor itself: float4 loads and stores, then a scalar tail of 0-3 elements;
//   * otherwise (a slice of a flat bucket at an element offset that is no multiple of 4): the whole chunk element by element, lane
//     i on elements i, i + 256, ...  All or nothing on purpose: keeping the aligned arrays of such a chunk on 16 bytes, as the sums
//     of layerwise.hip do for the sake of their bits, leaves the others four strided 4-byte accesses per lane, and that measured
//     13 % slower here with g and buf off the boundary.
// Both forms run sgd_one() on every element: explicit fmaf where torch applies `alpha` inside one op, contraction switched off
// everywhere else, so a value does not depend on which form its tensor took, and the same inputs give the same bits on every
// run (no atomics, no sums).  No element outside [0, n) of any array is read or written.
#include "zsv_common.h"
#include "zsv_hip.h"
#include "multi_tensor.h"
#include "adam_update.h"

#include <math.h>

namespace zsv {
namespace sgd {
struct Args {
    float lr, momentum, one_minus_dampening, wd;
    int use_momentum, nesterov, maximize;
    int grads_unscaled;
    int first_step;                     // "first" iff steps_done (0 without a scaler) == first_step
    const zsv_clip_record* clip;        // NULL: no clipping
    const zsv_scaler_state* st;         // NULL: no loss scaler
    float* const* shadows;              // NULL: no averaging
    const zsv_avg_state* avg;
    float ema_weight;
};

// what a workgroup reads once
struct Step {
    float inv_scale, clip;
    float ratio;                        // LAYERWISE: the trust ratio of the chunk's tensor
    bool first;
};

// torch/optim/sgd.py::_single_tensor_sgd on one element; returns the new parameter, `buf` is updated in place.  LAYERWISE: LARS,
// d = ratio * (g + wd * p) in the place of g + wd * p; with ratio == 1 (1 * x is x) that is the plain rule bit for bit.
template <bool LAYERWISE>
__device__ __forceinline__ float sgd_one(float p, float g, float& buf, const Args& a, const Step& s) {
#pragma clang fp contract(off)
    g = g * s.inv_scale;                                  // two separate fp32 products, as unscale_ and clip_grad_norm_ store them
    g = g * s.clip;
    if (a.maximize) g = -g;
    if (a.wd != 0.f) g = fmaf(a.wd, p, g);                // grad.add(param, alpha=weight_decay)
    if (LAYERWISE) g = s.ratio * g;
    if (a.use_momentum) {
        if (s.first) {
            buf = g;                                      // torch.clone(grad)
        } else {
            const float mb = a.momentum * buf;            // buf.mul_(momentum)
            buf = fmaf(a.one_minus_dampening, g, mb);     //    .add_(grad, alpha=1 - dampening)
        }
        g = a.nesterov ? fmaf(a.momentum, buf, g) : buf;  // grad.add(buf, alpha=momentum)
    }
    return fmaf(-a.lr, g, p);                             // param.add_(grad, alpha=-lr)
}

// `records` is read only by the LAYERWISE instantiation (zsv_sgd_multi passes NULL)
template <bool LAYERWISE>
__global__ __launch_bounds__(256) void sgd_multi_kernel(const zsv_adam_tensor* __restrict__ table, int count,
                                                        const zsv_layer_record* __restrict__ records, Args a) {
    if (a.st != nullptr && a.st->found_inf) return;      // scaler.step skips optimizer.step: decay, buffers and the average too
    Step s;
    s.inv_scale = a.st != nullptr && !a.grads_unscaled ? (float)(1.0 / (double)a.st->scale) : 1.f;
    s.clip = a.clip != nullptr ? a.clip->clip_coef : 1.f;
    s.first = (a.st != nullptr ? a.st->steps_done : 0) == a.first_step;

    const long chunk = blockIdx.x;
    const int index = find_index(table, count, chunk);
    const zsv_adam_tensor t = table[index];
    const Span span = chunk_span(t, chunk);
    if (span.base >= span.end) return;
    const int len = (int)(span.end - span.base);
    s.ratio = LAYERWISE ? records[index].ratio : 1.f;
    float* __restrict__ p = t.p + span.base;
    const float* __restrict__ g = t.g + span.base;
    float* __restrict__ buf = a.use_momentum ? t.exp_avg + span.base : nullptr;
    float* __restrict__ shadow = a.shadows != nullptr ? a.shadows[index] + span.base : nullptr;
    AvgWeight k{};
    if (shadow != nullptr) k = avg_weight(a.avg, a.ema_weight);
    const bool load_buf = buf != nullptr && !s.first;     // a first step never reads the buffer (torch has none yet)

    auto one = [&](int i) {
        float b = load_buf ? buf[i] : 0.f;
        const float pi = sgd_one<LAYERWISE>(p[i], g[i], b, a, s);
        if (buf != nullptr) buf[i] = b;
        p[i] = pi;
        if (shadow != nullptr) avg_element(shadow, i, pi, k);
    };

    // a NULL pointer is aligned: only the arrays this launch touches decide (same answer for every lane of the chunk)
    if (!(vec16(p) && vec16(g) && vec16(buf) && vec16(shadow))) {
        for (int i = threadIdx.x; i < len; i += 256) one(i);
        return;
    }
    const int nvec = len >> 2;
    v4f* __restrict__ pv = reinterpret_cast<v4f*>(p);
    const v4f* __restrict__ gv = reinterpret_cast<const v4f*>(g);
    v4f* __restrict__ bv = reinterpret_cast<v4f*>(buf);
    v4f* __restrict__ sv = reinterpret_cast<v4f*>(shadow);
#pragma unroll 2
    for (int v = threadIdx.x; v < nvec; v += 256) {
        v4f p4 = pv[v];
        const v4f g4 = gv[v];
        v4f b4 = v4f{0.f, 0.f, 0.f, 0.f};
        if (load_buf) b4 = bv[v];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float b = b4[e];
            p4[e] = sgd_one<LAYERWISE>(p4[e], g4[e], b, a, s);
            b4[e] = b;
        }
        if (buf != nullptr) bv[v] = b4;
        pv[v] = p4;
        if (shadow != nullptr) {
            v4f s4 = p4;
            if (!k.copy) {
                s4 = shadow_load(sv + v);
#pragma unroll
                for (int e = 0; e < 4; ++e) s4[e] = avg_value(s4[e], p4[e], k);
            }
            shadow_store(s4, sv + v);
        }
    }
    const int i = 4 * nvec + (int)threadIdx.x;            // tail: 0-3 elements
    if (i < len) one(i);
}

// The host half of both entry points: every refusal before the launch, NULL first, then the table's shape, then the options.
// `records` NULL: the plain rule; otherwise LARS.
static int launch(const zsv_adam_tensor* table, int32_t count, int64_t total_chunks, const zsv_layer_record* records, double lr,
                  float momentum, float dampening, int32_t nesterov, double weight_decay, int32_t maximize,
                  const zsv_clip_record* clip, const zsv_scaler_state* st, int32_t grads_unscaled, int32_t first_step,
                  float* const* shadows, const zsv_avg_state* avg, float ema_weight, void* stream) {
    if (!table) return ZSV_E_NULL;
    if ((shadows == nullptr) != (avg == nullptr)) return ZSV_E_NULL;
    if (bad_table(count, total_chunks)) return ZSV_E_BAD_SHAPE;
    if (bad_rate(lr) || bad_rate(weight_decay)) return ZSV_E_BAD_SHAPE;
    if (!(momentum >= 0.f) || !isfinite(momentum) || !isfinite(dampening)) return ZSV_E_BAD_SHAPE;
    if (nesterov && (!(momentum > 0.f) || dampening != 0.f)) return ZSV_E_BAD_SHAPE;     // torch: "Nesterov momentum requires ..."
    if (shadows != nullptr && !(ema_weight <= 1.f)) return ZSV_E_BAD_SHAPE;              // (a NaN weight is refused too)
    Args a;
    a.lr = (float)lr;
    a.momentum = momentum;
    a.one_minus_dampening = (float)(1.0 - (double)dampening);
    a.wd = (float)weight_decay;
    a.use_momentum = momentum != 0.f;
    a.nesterov = nesterov != 0;
    a.maximize = maximize != 0;
    a.grads_unscaled = grads_unscaled != 0;
    a.first_step = first_step;
    a.clip = clip;
    a.st = st;
    a.shadows = shadows;
    a.avg = avg;
    a.ema_weight = ema_weight;
    const auto kernel = records != nullptr ? sgd_multi_kernel<true> : sgd_multi_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, table, count, records, a);
    return launch_status();
}
}  // namespace sgd
}  // namespace zsv

using namespace zsv;

extern "C" int zsv_sgd_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr, float momentum,
                             float dampening, int32_t nesterov, double weight_decay, int32_t maximize,
                             const zsv_clip_record* clip_device, const zsv_scaler_state* state_device, int32_t grads_unscaled,
                             int32_t first_step, float* const* shadows_device, const zsv_avg_state* avg_state_device,
                             float ema_weight, void* stream) {
    return sgd::launch(table_device, count, total_chunks, nullptr, lr, momentum, dampening, nesterov, weight_decay, maximize,
                       clip_device, state_device, grads_unscaled, first_step, shadows_device, avg_state_device, ema_weight, stream);
}

extern "C" int zsv_lars_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks,
                              const zsv_layer_record* records_device, double lr, float momentum, float dampening, int32_t nesterov,
                              double weight_decay, int32_t maximize, const zsv_clip_record* clip_device,
                              const zsv_scaler_state* state_device, int32_t grads_unscaled, int32_t first_step,
                              float* const* shadows_device, const zsv_avg_state* avg_state_device, float ema_weight, void* stream) {
    if (!records_device) return ZSV_E_NULL;
    return sgd::launch(table_device, count, total_chunks, records_device, lr, momentum, dampening, nesterov, weight_decay, maximize,
                       clip_device, state_device, grads_unscaled, first_step, shadows_device, avg_state_device, ema_weight, stream);
}
