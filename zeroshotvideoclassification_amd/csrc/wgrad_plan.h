// wgrad_plan.h -- the slice arithmetic shared by the weight-gradient plans (host only).
//
// Every weight-gradient kernel cuts its voxel range into `slices` contiguous ranges of whole chunks so that a launch fills the
// chip although the output has a handful of tiles; each slice writes a partial slab and wgrad_sum.hip adds the slabs in order.
// The plans (conv_wgrad*.hip) keep their own constants, caps and knobs and call these helpers with them.
#pragma once
#include <stddef.h>

namespace zsv {

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

inline long clamp1(long v, long cap) { return v < 1 ? 1 : (v > cap ? cap : v); }       // into [1, cap]

// the row tile, 144 or 128, that pads `n` rows less (144 on ties)
inline int rows_144_or_128(int n) { return (n + 143) / 144 * 144 <= (n + 127) / 128 * 128 ? 144 : 128; }
inline int pad_144_or_128(int n) { const int t = rows_144_or_128(n); return (n + t - 1) / t * t; }

// The slice count that minimises (MFMA time / fill of the rounds of `resident` workgroups) + (slab write + read) per slice;
// fewer slices unless more gain 0.1 %.
inline long slices_by_cost(long tiles, long resident, double t_mfma, double t_slice, long max_slices) {
    long sl = 1;
    double best = 1e300;
    for (long c = 1; c <= max_slices; ++c) {
        const long wgs = tiles * c, rounds = (wgs + resident - 1) / resident;
        const double cost = t_mfma * (double)(rounds * resident) / (double)wgs + t_slice * (double)c;
        if (cost < best * 0.999) { best = cost; sl = c; }
    }
    return sl;
}

// The slice count that best fills whole rounds of `resident` workgroups, at most four rounds, every workgroup costing 2 % of a
// round in slab traffic (fewer slices on ties).  `efficiency` = the round fill of that count.
inline long slices_by_fill(long tiles, long resident, long max_slices, double* efficiency) {
    long slices = 1;
    double best_eff = -1.0;
    for (long s = 1; s <= max_slices && tiles * s <= 4 * resident + tiles; ++s) {
        const long wgs = tiles * s, rounds = (wgs + resident - 1) / resident;
        const double eff = (double)wgs / (double)(rounds * resident) - 0.02 * (double)wgs / (double)resident;
        if (eff > best_eff + 1e-9) { best_eff = eff; slices = s; }
    }
    *efficiency = best_eff;
    return slices;
}

// `slices` equal shares of whole chunks; the count is rounded down to the shares that are not empty
inline void split_chunks(long chunks, long slices, int* chunks_per_slice, int* slices_out) {
    *chunks_per_slice = (int)((chunks + slices - 1) / slices);
    *slices_out = (int)((chunks + *chunks_per_slice - 1) / *chunks_per_slice);
}

}  // namespace zsv
