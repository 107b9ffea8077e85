// still_image.hip -- camera-motion clips from still images on the GPU (gfx950): u8 images -> model input.
//
// The reference's third data source (main.py --dataset sun2both) turns one SUN397 image into a clip by sliding and
// zooming a square window along a straight trajectory (auxiliary/auxiliary_stillimages.py:92-138,
// ImageDataset.extract_camera_motion).  Every frame is img[top:top+side, left:left+side] through crop_transform
// (:56-62): ToPILImage -> Resize((crop, crop)) = PIL's antialiased bilinear resample on uint8 -> ToTensor (u8/255,
// HWC->CHW) -> Normalize(Kinetics mean / std), one PIL resize per frame on a CPU worker.  Here one launch makes the
// (B, n_clips, 3, T, crop, crop) batch from the uint8 images, which stay L2-resident.
//
// PIL's uint8 resample is integer arithmetic over coefficients derived in double precision, and the normalisation is
// three correctly rounded fp32 operations, so the kernel reproduces the reference bit for bit:
//   coefficients (fp64, nothing fused):  scale = side/crop; support = filterscale = max(scale, 1); ss = 1/filterscale;
//     center = (xx + 0.5)*scale; first = max(int(center - support + 0.5), 0); last = min(int(center + support + 0.5), side);
//     w[x] = triangle((x + first - center + 0.5)*ss); k[x] = int(0.5 + (w[x] / sum(w)) * 2^22)
//   a pass:  u8 = clip((2^21 + sum(pixel * k)) >> 22, 0, 255); horizontal first, uint8 between the passes.
//   (side == crop gives k = {2^22, 0}: the pass PIL skips is the identity here too.)
//   normalise:  ((u8 / 255) - mean_c) / std_c in fp32 with IEEE division.
//
// One workgroup per (frame, band of BAND output rows): it derives the frame's coefficient table (the window is
// square, so both axes share it), runs the horizontal pass for the input rows its band needs into LDS as uint8,
// then the vertical pass out of LDS; lanes walk the output W axis (coalesced 4-B stores).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zsv_hip.h"
#include "zsv_common.h"

namespace zsv {

constexpr int STILL_BAND = 8;              // output rows per workgroup
constexpr int STILL_MAX_RATIO = 8;         // side / crop <= 8: 17 taps per axis
constexpr int STILL_PRECISION_BITS = 22;   // PIL: 32 - 8 - 2

struct StillGeom {
    int crop, T, n_clips, frames_per_image;   // frames_per_image = n_clips * T
    int bands;                                // ceil(crop / STILL_BAND)
    int kstride;                              // coefficient row length for the largest side of the batch
    int max_side;
    Magic m_bands, m_pitch, m_crop;           // divisions by bands, crop * 3, crop
};

// Row xx of the side -> crop coefficient table: k[0..kstride) (zero past the window) and the window (first, count).
// The order of the fp64 operations is PIL's (Resample.c precompute_coeffs / normalize_coeffs_8bpc); no contraction.
__device__ __forceinline__ void resample_row(int side, int crop, int xx, int kstride, int* k, int* first_out, int* count_out) {
#pragma clang fp contract(off)
    const double scale = (double)side / (double)crop;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = filterscale;                      // the triangle filter's support is 1
    const double ss = 1.0 / filterscale;
    const double center = ((double)xx + 0.5) * scale;
    int first = (int)(center - support + 0.5);
    if (first < 0) first = 0;
    int last = (int)(center + support + 0.5);
    if (last > side) last = side;
    const int count = last - first;                          // <= 2*ceil(support) + 1 = the caller's kstride
    double ww = 0.0;
    for (int x = 0; x < count; ++x) {
        double a = ((double)(x + first) - center + 0.5) * ss;
        a = a < 0.0 ? -a : a;
        ww += a < 1.0 ? 1.0 - a : 0.0;
    }
    for (int x = 0; x < kstride; ++x) {
        int v = 0;
        if (x < count) {
            double a = ((double)(x + first) - center + 0.5) * ss;
            a = a < 0.0 ? -a : a;
            double w = a < 1.0 ? 1.0 - a : 0.0;
            if (ww != 0.0) w = w / ww;
            v = (int)(0.5 + w * (double)(1 << STILL_PRECISION_BITS));
        }
        k[x] = v;
    }
    *first_out = first;
    *count_out = count;
}

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> STILL_PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ToTensor + Normalize (auxiliary_stillimages.py:59-61): three correctly rounded fp32 operations, never fused
__device__ __forceinline__ float normalise_u8(int u8, float mean, float stdev) {
#pragma clang fp contract(off)
    const float x = (float)u8 / 255.0f;
    const float d = x - mean;
    return d / stdev;
}

__global__ __launch_bounds__(256) void resample_coeffs_kernel(int side, int crop, int kstride, int* __restrict__ coeffs,
                                                              int* __restrict__ bounds) {
    const int xx = blockIdx.x * 256 + threadIdx.x;
    if (xx < crop) resample_row(side, crop, xx, kstride, coeffs + (size_t)xx * kstride, bounds + 2 * xx, bounds + 2 * xx + 1);
}

__global__ __launch_bounds__(256) void still_image_clips_kernel(const int64_t* __restrict__ images, const int32_t* __restrict__ frames,
                                                                StillGeom g, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char still_smem[];
    int* kk = (int*)still_smem;                               // [crop][kstride] coefficients of this frame's side
    int* bnd = kk + g.crop * g.kstride;                       // [crop][2] (first, count)
    uint8_t* mid = (uint8_t*)(bnd + 2 * g.crop);              // [rows][crop * 3]: the band's rows after the horizontal pass

    const int tid = threadIdx.x;
    const unsigned frame = mdiv(blockIdx.x, g.m_bands);
    const int band = (int)(blockIdx.x - frame * (unsigned)g.bands);
    const int b = (int)(frame / (unsigned)g.frames_per_image);
    const int f = (int)(frame - (unsigned)b * (unsigned)g.frames_per_image);
    const int clip = f / g.T, t = f - clip * g.T;             // frame f of image b lands at clip f // T, time f % T
    const int top = frames[3 * (size_t)frame + 0], left = frames[3 * (size_t)frame + 1], side = frames[3 * (size_t)frame + 2];
    const uint8_t* img = (const uint8_t*)(uintptr_t)images[3 * (size_t)b + 0];
    const long H = images[3 * (size_t)b + 1], W = images[3 * (size_t)b + 2];

    const int crop = g.crop, pitch = crop * 3;
    const int y0 = band * STILL_BAND;
    const int nb = min(STILL_BAND, crop - y0);
    const size_t plane = (size_t)crop * crop;
    // out[b][clip][c][t][yy][xx]
    float* obase = out + (((size_t)b * g.n_clips + clip) * 3 * g.T + t) * plane + (size_t)y0 * crop;
    const size_t cstride = (size_t)g.T * plane;
    const int nout = nb * 3 * crop;

    // The caller validates the tables; a frame that breaks the contract all the same is never read: its band becomes NaN.
    bool valid = img != nullptr && side >= crop && side <= g.max_side && top >= 0 && left >= 0 && (long)top + side <= H &&
                 (long)left + side <= W;
    int row0 = 0, nrows = 0;
    if (valid) {
        for (int xx = tid; xx < crop; xx += 256) resample_row(side, crop, xx, g.kstride, kk + xx * g.kstride, bnd + 2 * xx, bnd + 2 * xx + 1);
        __syncthreads();
        row0 = bnd[2 * y0];
        nrows = bnd[2 * (y0 + nb - 1)] + bnd[2 * (y0 + nb - 1) + 1] - row0;   // <= (BAND + 1) * side / crop + 1 <= rows_cap
    }
    if (!valid) {                                             // uniform over the workgroup
        for (int i = tid; i < nout; i += 256) {
            const int q = (int)mdiv((unsigned)i, g.m_crop), xx = i - q * crop;
            const int c = (q >= nb) + (q >= 2 * nb), yy = q - c * nb;
            obase[c * cstride + (size_t)yy * crop + xx] = __builtin_nanf("");
        }
        return;
    }

    // horizontal pass: input rows [row0, row0 + nrows) of the window -> mid, uint8
    const uint8_t* src = img + ((size_t)(top + row0) * (size_t)W + (size_t)left) * 3;
    const size_t src_pitch = (size_t)W * 3;
    for (int i = tid; i < nrows * pitch; i += 256) {
        const int r = (int)mdiv((unsigned)i, g.m_pitch), j = i - r * pitch;
        const int xx = j / 3, c = j - xx * 3;
        const int first = bnd[2 * xx], count = bnd[2 * xx + 1];
        const uint8_t* p = src + (size_t)r * src_pitch + (size_t)first * 3 + c;
        const int* k = kk + xx * g.kstride;
        int acc = 1 << (STILL_PRECISION_BITS - 1);
        for (int x = 0; x < count; ++x) acc += (int)p[3 * x] * k[x];
        mid[i] = (uint8_t)clip8(acc);
    }
    __syncthreads();

    // vertical pass out of LDS, then normalise; consecutive lanes -> consecutive xx of one output row
    const float mean[3] = {0.43216f, 0.394666f, 0.37645f}, stdev[3] = {0.22803f, 0.22145f, 0.216989f};
    for (int i = tid; i < nout; i += 256) {
        const int q = (int)mdiv((unsigned)i, g.m_crop), xx = i - q * crop;
        const int c = (q >= nb) + (q >= 2 * nb), yy = q - c * nb;
        const int first = bnd[2 * (y0 + yy)] - row0, count = bnd[2 * (y0 + yy) + 1];
        const uint8_t* p = mid + first * pitch + xx * 3 + c;
        const int* k = kk + (y0 + yy) * g.kstride;
        int acc = 1 << (STILL_PRECISION_BITS - 1);
        for (int y = 0; y < count; ++y) acc += (int)p[y * pitch] * k[y];
        const float m = c == 0 ? mean[0] : (c == 1 ? mean[1] : mean[2]);
        const float s = c == 0 ? stdev[0] : (c == 1 ? stdev[1] : stdev[2]);
        obase[c * cstride + (size_t)yy * crop + xx] = normalise_u8(clip8(acc), m, s);
    }
}

static inline int still_kstride(int side, int crop) { return 2 * ((side + crop - 1) / crop) + 1; }   // 2*ceil(support) + 1

}  // namespace zsv

using namespace zsv;

extern "C" int zsv_resample_coeffs(int32_t side, int32_t crop, int32_t* coeffs, int32_t* bounds, void* stream) {
    if (crop <= 0 || side < crop || (long)side > (long)STILL_MAX_RATIO * crop) return ZSV_E_BAD_SHAPE;
    if (!coeffs || !bounds) return ZSV_E_NULL;
    hipLaunchKernelGGL(resample_coeffs_kernel, dim3((unsigned)((crop + 255) / 256)), dim3(256), 0, (hipStream_t)stream, side, crop,
                       still_kstride(side, crop), coeffs, bounds);
    return launch_status();
}

extern "C" int zsv_still_image_clips(const int64_t* image_table_device, const int32_t* frame_table_device, int32_t B, int32_t n_clips,
                                     int32_t T, int32_t crop, int32_t max_side, float* out, void* stream) {
    if (B <= 0 || n_clips <= 0 || T <= 0 || crop <= 0 || max_side < crop || (long)max_side > (long)STILL_MAX_RATIO * crop)
        return ZSV_E_BAD_SHAPE;
    if (!image_table_device || !frame_table_device || !out) return ZSV_E_NULL;
    const int bands = (crop + STILL_BAND - 1) / STILL_BAND;
    const double nframes = (double)B * n_clips * T;
    if (nframes * 3.0 * crop * crop >= 2147483647.0 * 4 || nframes * bands >= 2147483647.0) return ZSV_E_TOO_LARGE;
    StillGeom g;
    g.crop = crop, g.T = T, g.n_clips = n_clips, g.frames_per_image = n_clips * T, g.bands = bands, g.max_side = max_side;
    g.kstride = still_kstride(max_side, crop);
    const int rows_cap = (STILL_BAND + 1) * ((max_side + crop - 1) / crop) + 2;   // rows of the LDS intermediate a band can need
    g.m_bands = make_magic((unsigned)bands), g.m_pitch = make_magic((unsigned)crop * 3), g.m_crop = make_magic((unsigned)crop);
    const size_t lds = ((size_t)crop * g.kstride + 2 * (size_t)crop) * sizeof(int) + (size_t)rows_cap * crop * 3;
    if (lds > 64 * 1024) return ZSV_E_UNSUPPORTED;           // crop far beyond the reference's 112
    hipLaunchKernelGGL(still_image_clips_kernel, dim3((unsigned)(nframes * bands)), dim3(256), lds, (hipStream_t)stream,
                       image_table_device, frame_table_device, g, out);
    return launch_status();
}
