// preprocess.hip -- clip pre-processing on the GPU (gfx950): u8 frames -> model input.
//
// Fuses the reference's per-clip transform chain (auxiliary/transforms.py:41-56) into one
// HBM pass:  ToFloatTensorInZeroOne ((u8/255 - 1)/2 and THWC -> CTHW, transforms.py:116-117)
//            -> Resize(short side 128, bilinear, align_corners=False, transforms.py:99-107)
//            -> Center/RandomCrop(112) (transforms.py:80-97,132-158)
//            -> RandomHorizontalFlip (transforms.py:188-195)
// The CPU pipeline materialises the resized 3xTx128xW' float tensor per clip; here every
// output voxel reads its 4 source pixels directly (u8, 1 B each) -- 13 MB of u8 in, 53 MB of
// fp32 out per 22-clip batch instead of an fp32 host->device copy.  HBM-bound; lanes walk the
// output W axis (coalesced 4-B stores; the u8 gathers of a row hit the same cache lines).
// Two entry points share the per-pixel arithmetic (clip_pixel): zsv_clip_transform for one dense (N, T, H, W, 3) tensor and
// zsv_clip_transform_batch for a batch of videos of different frame sizes behind a device table, which also does the
// reference loader's (nc*T) -> (nc, 3, T) reshuffle (auxiliary/auxiliary_dataset.py:506-510).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "zsv_hip.h"
#include "zsv_common.h"

namespace zsv {

struct ClipGeom {
    int T, Hin, Win;         // source frames (T, Hin, Win, 3) u8, HWC interleaved
    int Hres, Wres;          // size after the resize
    int crop;                // output is crop x crop
    float inv_scale;         // source step per resized pixel (1 / scale_factor)
};

// (u8/255 - 1)/2 (transforms.py:116-117): an IEEE division, a subtraction and an exact halving
__device__ __forceinline__ float norm_u8(uint8_t v) {
#pragma clang fp contract(off)
    return ((float)v / 255.f - 1.0f) * 0.5f;
}

// One output pixel of the chain: resized-frame pixel (ry, rx) of the frame whose channel-0 byte of pixel (0, 0) is `px`, for
// the NC consecutive channels px[0..NC).  Both kernels below call this.  The clamps (sy, sx >= 0, indices <= Hin-1 / Win-1)
// keep every read inside the frame whatever (ry, rx) is.
// Every multiply-add is written out and nothing else may be contracted: left to the compiler, the choice of which product of
// a blend is fused depends on how the surrounding loop was unrolled and vectorised (the dense kernel once held two versions of
// its loop that rounded differently), and the two kernels must agree bit for bit.
template <int NC>
__device__ __forceinline__ void clip_pixel(const uint8_t* __restrict__ px, int Hin, int Win, float inv_scale, int ry, int rx,
                                           float (&v)[NC]) {
#pragma clang fp contract(off)
    // torch upsample_bilinear2d, align_corners=False: src = scale*(dst+0.5)-0.5, clamped at 0
    float sy = __builtin_fmaf(inv_scale, (float)ry + 0.5f, -0.5f);
    float sx = __builtin_fmaf(inv_scale, (float)rx + 0.5f, -0.5f);
    sy = sy < 0.f ? 0.f : sy;
    sx = sx < 0.f ? 0.f : sx;
    const int y0 = min((int)sy, Hin - 1), x0 = min((int)sx, Win - 1);
    const int y1 = min(y0 + 1, Hin - 1), x1 = min(x0 + 1, Win - 1);
    const float ly = sy - (float)y0, lx = sx - (float)x0;
    const float my = 1.f - ly, mx = 1.f - lx;
    const uint8_t* p00 = px + ((size_t)y0 * Win + x0) * 3;
    const uint8_t* p01 = px + ((size_t)y0 * Win + x1) * 3;
    const uint8_t* p10 = px + ((size_t)y1 * Win + x0) * 3;
    const uint8_t* p11 = px + ((size_t)y1 * Win + x1) * 3;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float v00 = norm_u8(p00[c]), v01 = norm_u8(p01[c]);
        const float v10 = norm_u8(p10[c]), v11 = norm_u8(p11[c]);
        const float top_row = __builtin_fmaf(lx, v01, mx * v00);     // (1 - lx) * v00 + lx * v01
        const float bot_row = __builtin_fmaf(lx, v11, mx * v10);
        v[c] = __builtin_fmaf(ly, bot_row, my * top_row);            // (1 - ly) * top_row + ly * bot_row
    }
}

__global__ __launch_bounds__(256) void clip_transform_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ params,
                                                             ClipGeom g, long total, float* __restrict__ out) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        int x = (int)(i % g.crop);
        long r = i / g.crop;
        const int y = (int)(r % g.crop);
        r /= g.crop;
        const int t = (int)(r % g.T);
        r /= g.T;
        const int c = (int)(r % 3);
        const int n = (int)(r / 3);
        const int top = params[3 * n + 0], left = params[3 * n + 1], flip = params[3 * n + 2];
        if (flip) x = g.crop - 1 - x;                       // flip acts on the cropped clip
        const uint8_t* f = frames + (((size_t)n * g.T + t) * g.Hin) * g.Win * 3 + c;
        float v[1];
        clip_pixel<1>(f, g.Hin, g.Win, g.inv_scale, top + y, left + x, v);
        out[i] = v[0];
    }
}

// The same chain for B videos of different frame sizes: grid (pixel tile, frame of the video, video), so a workgroup never
// straddles two videos and its row of the table is wave-uniform (scalar loads, read once).  One thread makes one output pixel
// of all three channels: four source pixels of 3 contiguous bytes in, three coalesced plane stores out.
__global__ __launch_bounds__(256) void clip_transform_batch_kernel(const int64_t* __restrict__ table, int n_clips, int T, int crop,
                                                                   Magic m_crop, float* __restrict__ out) {
    const int b = blockIdx.z, f = blockIdx.y;
    const int64_t* row = table + (size_t)b * ZSV_CLIP_ROW;
    const uint8_t* frames = (const uint8_t*)(uintptr_t)row[0];
    const long Hin = row[1], Win = row[2], Hres = row[3], Wres = row[4], top = row[5], left = row[6];
    const int flip = (int)(row[7] & 1);
    const float inv_scale = __int_as_float((int)(row[7] >> 32));
    const int cc = crop * crop;
    const int p = blockIdx.x * 256 + threadIdx.x;           // pixel of the crop x crop plane
    if (p >= cc) return;
    const int clip = f / T, t = f - clip * T;               // frame f of video b lands at clip f / T, time f % T
    // out[b][clip][c][t][y][x]
    float* o = out + (((size_t)b * n_clips + clip) * 3 * T + t) * (size_t)cc + p;
    const size_t cstride = (size_t)T * cc;
    // The caller validates the table; a row that breaks the contract all the same is never read: its frames become NaN.
    const bool valid = frames != nullptr && Hin > 0 && Win > 0 && Hin <= 2147483647L && Win <= 2147483647L && inv_scale > 0.f &&
                       top >= 0 && left >= 0 && top + crop <= Hres && left + crop <= Wres && Hres <= 2147483647L && Wres <= 2147483647L;
    if (!valid) {                                           // uniform over the workgroup
        o[0] = o[cstride] = o[2 * cstride] = __builtin_nanf("");
        return;
    }
    const int y = (int)mdiv((unsigned)p, m_crop);
    int x = p - y * crop;
    if (flip) x = crop - 1 - x;                             // flip acts on the cropped clip
    float v[3];
    clip_pixel<3>(frames + (size_t)f * (size_t)Hin * (size_t)Win * 3, (int)Hin, (int)Win, inv_scale, (int)top + y, (int)left + x, v);
    o[0] = v[0];
    o[cstride] = v[1];
    o[2 * cstride] = v[2];
}

}  // namespace zsv

using namespace zsv;

extern "C" int zsv_clip_transform(const uint8_t* frames_u8, int32_t N, int32_t T, int32_t Hin, int32_t Win,
                                  int32_t Hres, int32_t Wres, float inv_scale, int32_t crop,
                                  const int32_t* crop_flip_params_device, float* out, void* stream) {
    if (!frames_u8 || !crop_flip_params_device || !out) return ZSV_E_NULL;
    if (N <= 0 || T <= 0 || Hin <= 0 || Win <= 0 || crop <= 0 || Hres < crop || Wres < crop || !(inv_scale > 0.f))
        return ZSV_E_BAD_SHAPE;
    const long total = (long)N * 3 * T * crop * crop;
    if ((double)total >= 2147483647.0 * 4 || (double)N * T * Hin * Win * 3 >= 4.0e9) return ZSV_E_TOO_LARGE;
    ClipGeom g = {T, Hin, Win, Hres, Wres, crop, inv_scale};
    long blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(clip_transform_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames_u8,
                       (const int*)crop_flip_params_device, g, total, out);
    return launch_status();
}

extern "C" int zsv_clip_transform_batch(const int64_t* video_table_device, int32_t B, int32_t n_clips, int32_t T, int32_t crop,
                                        float* out, void* stream) {
    if (!video_table_device || !out) return ZSV_E_NULL;
    if (B <= 0 || n_clips <= 0 || T <= 0 || crop <= 0) return ZSV_E_BAD_SHAPE;
    const double frames = (double)n_clips * T;
    if ((double)B * 3.0 * frames * crop * crop >= 2147483647.0 * 4 || (double)crop * crop >= 2147483647.0 || frames > 65535.0 ||
        B > 65535)                                          // (the last two: grid y and z)
        return ZSV_E_TOO_LARGE;
    const unsigned tiles = (unsigned)(((long)crop * crop + 255) / 256);
    hipLaunchKernelGGL(clip_transform_batch_kernel, dim3(tiles, (unsigned)(n_clips * T), (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       video_table_device, n_clips, T, crop, make_magic((unsigned)crop), out);
    return launch_status();
}
