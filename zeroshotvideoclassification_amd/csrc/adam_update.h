// adam_update.h -- the per-element Adam update, plain and with weight decay / clipping, and the weight-averaging rule: what the
// one Adam kernel template of optim.hip runs per element, and what sgd.hip and zsv_avg_multi average with.  One body per mode, so
// the parameters and moments of a step with averaging carry the bits of the same step without it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zsv_hip.h"

namespace zsv {

// ---- the averaging rule of torch.optim.swa_utils.AveragedModel (include/zsv_hip.h) ------------------------------------------
struct AvgWeight {
    bool copy;        // n_averaged == 0: avg = p exactly
    float w;          // weight of the new value
};

// ema_weight >= 0: EMA, w = (float)(1 - decay) formed on the host; < 0: equal-weight, w = 1 / (n_averaged + 1)
__device__ __forceinline__ AvgWeight avg_weight(const zsv_avg_state* __restrict__ st, float ema_weight) {
    const int n = st->n_averaged;
    AvgWeight k;
    k.copy = n == 0;
    k.w = ema_weight >= 0.f ? ema_weight : 1.f / (float)(n + 1);
    return k;
}

// torch's lerp(avg, p, w): the form that is exact at its own end of the interval
__device__ __forceinline__ float avg_value(float avg, float p, const AvgWeight k) {
    if (k.copy) return p;
    const float d = p - avg;
    return k.w < 0.5f ? avg + k.w * d : p - d * (1.f - k.w);
}

// The shadow is read once and written once per step and touched by nothing else in between, which makes it a candidate for the
// non-temporal hints of the BatchNorm passes and grad_accum_multi.  Measured, they gained nothing here: plain
// accesses are the default, -DZSV_AVG_NONTEMPORAL builds the other form for an A/B.
template <typename T> __device__ __forceinline__ T shadow_load(const T* p) {
#ifdef ZSV_AVG_NONTEMPORAL
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
template <typename T> __device__ __forceinline__ void shadow_store(T v, T* p) {
#ifdef ZSV_AVG_NONTEMPORAL
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

__device__ __forceinline__ void avg_element(float* __restrict__ shadow, long i, float p, const AvgWeight k) {
    const float a = k.copy ? p : shadow_load(shadow + i);
    shadow_store(avg_value(a, p, k), shadow + i);
}

// ---- torch.optim.Adam, no weight decay: element i of tensor t with gradient value gi -----------------------------------------
template <bool AVG>
__device__ __forceinline__ void adam_element(const zsv_adam_tensor& t, long i, float gi, float b1, float b2, float eps,
                                             float step_size, float inv_sqrt_bc2, float* __restrict__ shadow, const AvgWeight k) {
    const float mi = b1 * t.exp_avg[i] + (1.f - b1) * gi;
    const float vi = b2 * t.exp_avg_sq[i] + (1.f - b2) * gi * gi;
    t.exp_avg[i] = mi;
    t.exp_avg_sq[i] = vi;
    const float pi = t.p[i] - step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
    t.p[i] = pi;
    if (AVG) avg_element(shadow, i, pi, k);
}

// ---- torch.optim.Adam(weight_decay=) / AdamW with the clip coefficient: element i of tensor t --------------------------------
// g = g_mem * inv_scale * clip; L2: g += wd_l2 * p; moments; decoupled: p *= decay_factor (1 - lr * wd); the Adam update.
struct AdamDecay {
    float wd_l2;            // L2 mode: g += wd_l2 * p                (0 otherwise)
    float decay_factor;     // decoupled mode: p *= decay_factor      (1 otherwise)
    int decoupled;
};

template <bool AVG>
__device__ __forceinline__ void adamw_element(const zsv_adam_tensor& t, long i, float inv_scale, float clip, const AdamDecay& d,
                                              float b1, float b2, float eps, float step_size, float inv_sqrt_bc2,
                                              float* __restrict__ shadow, const AvgWeight k) {
    float pi = t.p[i];
    float gi = t.g[i] * inv_scale;                 // two separate fp32 products, as unscale_ and clip_grad_norm_ store them
    gi = gi * clip;
    if (!d.decoupled) gi = gi + d.wd_l2 * pi;      // grad.add(param, alpha=weight_decay)
    const float mi = b1 * t.exp_avg[i] + (1.f - b1) * gi;
    const float vi = b2 * t.exp_avg_sq[i] + (1.f - b2) * gi * gi;
    t.exp_avg[i] = mi;
    t.exp_avg_sq[i] = vi;
    if (d.decoupled) pi *= d.decay_factor;         // param.mul_(1 - lr * weight_decay)
    pi = pi - step_size * (mi / (sqrtf(vi) * inv_sqrt_bc2 + eps));
    t.p[i] = pi;
    if (AVG) avg_element(shadow, i, pi, k);
}

}  // namespace zsv
