// conv_depthwise.hip -- depthwise Conv3d (groups == channels) in fp32 NCDHW: forward, input gradient, weight gradient (gfx950).
//
// The residual unit of the channel-separated networks is 1x1x1 -> 3x3x3 depthwise -> 1x1x1.  A depthwise convolution is a
// stencil: 2 * taps FLOP per 8 bytes of compulsory traffic, no reduction over channels, nothing for the matrix cores.  The
// entry points read zsv_conv_desc with Cin == Cout == C as x (N,C,Ti,Hi,Wi), w (C,1,kT,kH,kW), y (N,C,To,Ho,Wo).
//
// dw_tile_kernel<KT,KH,KW,SH,SW,MODE>: a workgroup owns one (n, c) plane and a tile of output rows x columns and walks the
// output frames.  The input rows of the tile (+ halo, zero-filled where the image ends) of the KT frames an output frame reads
// sit in a ring of KT frame slots in LDS, so an input element comes from HBM once per workgroup; consecutive lanes hold
// consecutive output columns (conflict-free 4-byte LDS reads, coalesced 4-byte global accesses: no operand needs more than its
// element's alignment, and the bits do not depend on the addresses) and a lane produces R vertically adjacent outputs from the
// row values it holds in registers.  The channel's weights are indexed by blockIdx: uniform, kept in scalar registers.
//   MODE 0  y = conv(x, w) (+ bias, ReLU); with flipped taps and padding k-1-p it is the stride-1 input gradient.
//   MODE 1  weight gradient: the same staging of x, the lane's dY values times the staged row values into taps accumulators in
//           registers; reduced over lanes (butterfly) and waves (in wave order) -- a fixed order -- and written as one
//           [slice][C * taps] slab row; wgrad_sum.hip adds the slabs in slice order.
// dw_dgrad_class_kernel<KT,KH,KW,SH,SW>: the input gradient of a strided convolution in gather form: dx[i] sums the taps k with
// (i + p - k) % s == 0, resolved at compile time per residue class of the rows and columns; EVERY element of dx is stored, the
// voxels no output touches as 0.  No zero-fill, no scatter, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "conv_params.h"
#include "wgrad_plan.h"

namespace zsv {

struct DwParams {
    int C;
    int Ti, Hi, Wi;            // the staged (gathered) tensor
    int To, Ho, Wo;            // the positions a lane owns (MODE 0: the produced tensor; MODE 1: dY)
    int sT, pT, pH, pW;
    int tw, tw_shift, ty;      // lanes along W (8 .. 64, a power of two), thread rows; tw * ty threads, a multiple of 64
    int tiles_w, tiles;        // tiles of one plane
    int in_rows, in_cols;      // staged rows / columns of one frame slot
    Magic cols_magic;          // division by in_cols
    int flip, relu;
    int units, units_per_slice;    // MODE 1: a unit is one (n, tile) with all its frames
};

template <int KT, int KH, int KW, int SH, int SW, int MODE>
__global__ __launch_bounds__(256) void dw_tile_kernel(DwParams p, const float* __restrict__ X, const float* __restrict__ W,
                                                      const float* __restrict__ B, float* __restrict__ OUT) {
    constexpr int R = SH == 1 ? 4 : 2;                  // output rows per lane
    constexpr int K = KT * KH * KW;
    constexpr int RIN = (R - 1) * SH + KH;              // input rows a lane reads per frame
    constexpr int STAGE = 5;                            // (an 18 x 66 slot of the 56 x 56 planes is 4.6 elements per lane)
    extern __shared__ float lds[];                      // [KT][in_rows][in_cols]
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int tx = tid & (p.tw - 1), tyi = tid >> p.tw_shift;
    const int slot_elems = p.in_rows * p.in_cols;
    const size_t in_frame = (size_t)p.Hi * p.Wi, out_frame = (size_t)p.Ho * p.Wo;

    int c, unit, unit_end;
    if constexpr (MODE == 0) {
        unit = blockIdx.x;                              // (n * C + c) * tiles + tile
        unit_end = unit + 1;
        c = (unit / p.tiles) % p.C;
    } else {
        c = blockIdx.x;
        unit = blockIdx.y * p.units_per_slice;          // n * tiles + tile
        unit_end = min(p.units, unit + p.units_per_slice);
    }

    float wr[K];                                        // MODE 0: the channel's taps (uniform); MODE 1: the partial sums
#pragma unroll
    for (int i = 0; i < K; ++i) wr[i] = MODE == 0 ? W[(size_t)c * K + (p.flip ? K - 1 - i : i)] : 0.f;

    bool first_step = true;
    for (; unit < unit_end; ++unit) {
        const int tile = unit % p.tiles;
        const int nc = MODE == 0 ? unit / p.tiles : (unit / p.tiles) * p.C + c;
        const int tile_h = tile / p.tiles_w, tile_w = tile - tile_h * p.tiles_w;
        const int oh0 = tile_h * p.ty * R, ow0 = tile_w * p.tw;
        const int ih0 = oh0 * SH - p.pH, iw0 = ow0 * SW - p.pW;
        const float* xin = X + (size_t)nc * p.Ti * in_frame;
        int next = -p.pT;                               // the first frame that is not staged yet
        for (int to = 0; to < p.To; ++to) {
            const int first = to * p.sT - p.pT;         // this output frame reads input frames first .. first + KT - 1
            if (next < first) next = first;
            if (!first_step) __syncthreads();           // the previous step's reads of the slots are over
            first_step = false;
            for (int ti = next; ti < first + KT; ++ti) {
                float* dst = lds + ((ti + p.pT) % KT) * slot_elems;
                const bool tin = ti >= 0 && ti < p.Ti;
                const float* src = xin + (size_t)(tin ? ti : 0) * in_frame;
                // flat over the slot, STAGE elements per lane and trip: their loads are in flight together (one HBM round trip per
                // frame for the usual tiles), then they go to LDS
                for (int i0 = tid; i0 < slot_elems; i0 += STAGE * nthr) {
                    float v[STAGE];
#pragma unroll
                    for (int e = 0; e < STAGE; ++e) {
                        const int i = i0 + e * nthr;
                        const int r = (int)mdiv((unsigned)i, p.cols_magic), cc = i - r * p.in_cols;
                        const int hi = ih0 + r, wi = iw0 + cc;
                        v[e] = 0.f;
                        if (i < slot_elems && tin && (unsigned)hi < (unsigned)p.Hi && (unsigned)wi < (unsigned)p.Wi) v[e] = src[(size_t)hi * p.Wi + wi];
                    }
#pragma unroll
                    for (int e = 0; e < STAGE; ++e)
                        if (i0 + e * nthr < slot_elems) dst[i0 + e * nthr] = v[e];
                }
            }
            next = first + KT;
            __syncthreads();

            const int ow = ow0 + tx, ohl = oh0 + tyi * R;
            const size_t obase = ((size_t)nc * p.To + to) * out_frame + (size_t)ohl * p.Wo + ow;
            const float* base = lds + (tyi * R * SH) * p.in_cols + tx * SW;
            float acc[R];
            bool live[R];
#pragma unroll
            for (int j = 0; j < R; ++j) {
                live[j] = ohl + j < p.Ho && ow < p.Wo;
                acc[j] = 0.f;
                if constexpr (MODE == 1) { if (live[j]) acc[j] = B[obase + (size_t)j * p.Wo]; }      // the lane's dY values
            }
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                const float* fb = base + ((first + kt + p.pT) % KT) * slot_elems;
#pragma unroll
                for (int r = 0; r < RIN; ++r) {
                    float v[KW];
#pragma unroll
                    for (int kw = 0; kw < KW; ++kw) v[kw] = fb[r * p.in_cols + kw];
#pragma unroll
                    for (int j = 0; j < R; ++j) {
                        const int kh = r - j * SH;
                        if (kh < 0 || kh >= KH) continue;
#pragma unroll
                        for (int kw = 0; kw < KW; ++kw) {
                            const int tap = (kt * KH + kh) * KW + kw;
                            if constexpr (MODE == 0) acc[j] = fmaf(wr[tap], v[kw], acc[j]);
                            else { if (live[j]) wr[tap] = fmaf(acc[j], v[kw], wr[tap]); }
                        }
                    }
                }
            }
            if constexpr (MODE == 0) {
                const float b = B != nullptr ? B[c] : 0.f;
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    if (!live[j]) continue;
                    float v = acc[j] + b;
                    if (p.relu) v = fmaxf(v, 0.f);
                    OUT[obase + (size_t)j * p.Wo] = v;
                }
            }
        }
    }

    if constexpr (MODE == 1) {
        // lanes by butterfly, waves in wave order: a fixed order of addition
        const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
#pragma unroll
        for (int i = 0; i < K; ++i) wr[i] = wave_sum(wr[i]);
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < K; ++i) lds[wave * K + i] = wr[i];
        }
        __syncthreads();
        if (tid < K) {
            float s = lds[tid];
            for (int q = 1; q < nw; ++q) s += lds[q * K + tid];
            OUT[((size_t)blockIdx.y * p.C + c) * K + tid] = s;
        }
    }
}

struct DwGatherParams {
    int C, Ti, Hi, Wi, To, Ho, Wo;
    int sT, pT, pH, pW;
    int cells_w, cells;        // cells of one input frame: one per dY voxel a frame's dx rows / columns hang on
    int tiles;                 // 256-cell tiles of one input frame
};

// A lane owns the SH x SW input voxels i = a * s - p + r, r < s, of cell (a, b): the taps that reach residue r are k = r + s * m
// (resolved at compile time) and read dY at a - m, so the lane loads ceil(KH / SH) x ceil(KW / SW) values of dY per live frame
// and forms all its voxels from them.  The frame test (it + pT - kt) % sT is uniform.  Every voxel of dx belongs to exactly
// one cell and is stored, the ones no output touches as 0.
template <int KT, int KH, int KW, int SH, int SW>
__global__ __launch_bounds__(256) void dw_dgrad_class_kernel(DwGatherParams p, const float* __restrict__ DY,
                                                             const float* __restrict__ W, float* __restrict__ DX) {
    constexpr int K = KT * KH * KW, MH = (KH + SH - 1) / SH, MW = (KW + SW - 1) / SW;
    const int tile = blockIdx.x % p.tiles, q = blockIdx.x / p.tiles;
    const int it = q % p.Ti, nc = q / p.Ti, c = nc % p.C;
    float wr[K];
#pragma unroll
    for (int i = 0; i < K; ++i) wr[i] = W[(size_t)c * K + i];
    const int pos = tile * 256 + (int)threadIdx.x;
    if (pos >= p.cells) return;
    const int a = pos / p.cells_w, b = pos - a * p.cells_w;
    const size_t out_frame = (size_t)p.Ho * p.Wo;
    float acc[SH][SW];
#pragma unroll
    for (int rh = 0; rh < SH; ++rh)
#pragma unroll
        for (int rw = 0; rw < SW; ++rw) acc[rh][rw] = 0.f;
#pragma unroll
    for (int kt = 0; kt < KT; ++kt) {
        const int t = it + p.pT - kt;
        if (t < 0 || (t & (p.sT - 1)) != 0 || (t >> (p.sT - 1)) >= p.To) continue;      // (strides are 1 or 2)
        const float* dyf = DY + ((size_t)nc * p.To + (t >> (p.sT - 1))) * out_frame;
        float v[MH][MW];
#pragma unroll
        for (int mh = 0; mh < MH; ++mh)
#pragma unroll
            for (int mw = 0; mw < MW; ++mw) {
                const int j = a - mh, i = b - mw;
                v[mh][mw] = 0.f;
                if (j >= 0 && j < p.Ho && i >= 0 && i < p.Wo) v[mh][mw] = dyf[(size_t)j * p.Wo + i];
            }
#pragma unroll
        for (int rh = 0; rh < SH; ++rh)
#pragma unroll
            for (int rw = 0; rw < SW; ++rw)
#pragma unroll
                for (int mh = 0; mh < MH; ++mh)
#pragma unroll
                    for (int mw = 0; mw < MW; ++mw) {
                        const int kh = rh + SH * mh, kw = rw + SW * mw;
                        if (kh < KH && kw < KW) acc[rh][rw] = fmaf(wr[(kt * KH + kh) * KW + kw], v[mh][mw], acc[rh][rw]);
                    }
    }
    float* dxf = DX + ((size_t)nc * p.Ti + it) * p.Hi * p.Wi;
#pragma unroll
    for (int rh = 0; rh < SH; ++rh)
#pragma unroll
        for (int rw = 0; rw < SW; ++rw) {
            const int ih = a * SH - p.pH + rh, iw = b * SW - p.pW + rw;
            if (ih >= 0 && ih < p.Hi && iw >= 0 && iw < p.Wi) dxf[(size_t)ih * p.Wi + iw] = acc[rh][rw];
        }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
static bool one_or(int v, int other) { return v == 1 || v == other; }

// every refusal of the depthwise entry points that depends on the descriptor alone
static int dw_check(const zsv_conv_desc* d) {
    if (!d) return ZSV_E_NULL;
    if (d->N <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->Ti <= 0 || d->Hi <= 0 || d->Wi <= 0) return ZSV_E_BAD_SHAPE;
    if (d->Cin != d->Cout) return ZSV_E_BAD_SHAPE;
    if (d->kT <= 0 || d->kH <= 0 || d->kW <= 0 || d->sT <= 0 || d->sH <= 0 || d->sW <= 0 || d->pT < 0 || d->pH < 0 || d->pW < 0)
        return ZSV_E_BAD_SHAPE;
    const long to = ((long)d->Ti + 2L * d->pT - d->kT) / d->sT + 1, ho = ((long)d->Hi + 2L * d->pH - d->kH) / d->sH + 1,
               wo = ((long)d->Wi + 2L * d->pW - d->kW) / d->sW + 1;
    if ((long)d->Ti + 2L * d->pT < d->kT || (long)d->Hi + 2L * d->pH < d->kH || (long)d->Wi + 2L * d->pW < d->kW) return ZSV_E_BAD_SHAPE;
    if (d->To != to || d->Ho != ho || d->Wo != wo || to <= 0 || ho <= 0 || wo <= 0) return ZSV_E_BAD_SHAPE;
    if (!one_or(d->kT, 3) || !one_or(d->kH, 3) || !one_or(d->kW, 3) || !one_or(d->sT, 2) || !one_or(d->sH, 2) || !one_or(d->sW, 2))
        return ZSV_E_UNSUPPORTED;
    if (d->pT >= d->kT || d->pH >= d->kH || d->pW >= d->kW) return ZSV_E_UNSUPPORTED;
    const double lim = 2147483648.0;
    if ((double)d->N * d->Cin * d->Ti * d->Hi * d->Wi >= lim || (double)d->N * d->Cout * d->To * d->Ho * d->Wo >= lim) return ZSV_E_TOO_LARGE;
    return ZSV_OK;
}

// the tile of dw_tile_kernel for positions (Ho, Wo) read at spatial stride (sh, sw) through a (kt, kh, kw) window
static void dw_tile_plan(DwParams& p, int Ho, int Wo, int kt, int kh, int kw, int sh, int sw) {
    const int R = sh == 1 ? 4 : 2;
    p.tw = Wo <= 8 ? 8 : Wo <= 16 ? 16 : Wo <= 32 ? 32 : 64;
    p.tw_shift = p.tw == 8 ? 3 : p.tw == 16 ? 4 : p.tw == 32 ? 5 : 6;
    const int step = 64 / p.tw, cap = 256 / p.tw;               // whole waves
    int ty = ((Ho + R - 1) / R + step - 1) / step * step;
    p.ty = ty > cap ? cap : ty;
    p.tiles_w = (Wo + p.tw - 1) / p.tw;
    p.tiles = p.tiles_w * ((Ho + p.ty * R - 1) / (p.ty * R));
    p.in_rows = (p.ty * R - 1) * sh + kh;
    p.in_cols = (p.tw - 1) * sw + kw;
    p.cols_magic = make_magic((unsigned)p.in_cols);
    (void)kt;
}
static size_t dw_lds_bytes(const DwParams& p, int kt, int taps) {
    const size_t ring = (size_t)kt * p.in_rows * p.in_cols, fold = (size_t)4 * taps;      // (MODE 1 folds its waves through LDS)
    return (ring > fold ? ring : fold) * sizeof(float);
}

template <int MODE>
static int dw_tile_launch(int kt, int kh, int kw, int sh, int sw, dim3 grid, const DwParams& p, const float* a, const float* b,
                          const float* c, float* out, hipStream_t stream) {
    const dim3 block((unsigned)(p.tw * p.ty));
    const size_t lds = dw_lds_bytes(p, kt, kt * kh * kw);
    const int key = ((kt == 3) << 4) | ((kh == 3) << 3) | ((kw == 3) << 2) | ((sh == 2) << 1) | (sw == 2);
    switch (key) {
#define DW_CASE(KT, KH, KW, SH, SW)                                                                                              \
    case (((KT) == 3) << 4) | (((KH) == 3) << 3) | (((KW) == 3) << 2) | (((SH) == 2) << 1) | ((SW) == 2):                         \
        hipLaunchKernelGGL((dw_tile_kernel<KT, KH, KW, SH, SW, MODE>), grid, block, lds, stream, p, a, b, c, out);                \
        break;
#define DW_STRIDES(KT, KH, KW) DW_CASE(KT, KH, KW, 1, 1) DW_CASE(KT, KH, KW, 1, 2) DW_CASE(KT, KH, KW, 2, 1) DW_CASE(KT, KH, KW, 2, 2)
        DW_STRIDES(1, 1, 1) DW_STRIDES(1, 1, 3) DW_STRIDES(1, 3, 1) DW_STRIDES(1, 3, 3)
        DW_STRIDES(3, 1, 1) DW_STRIDES(3, 1, 3) DW_STRIDES(3, 3, 1) DW_STRIDES(3, 3, 3)
#undef DW_STRIDES
#undef DW_CASE
        default: return ZSV_E_UNSUPPORTED;
    }
    return launch_status();
}

static int dw_gather_launch(const zsv_conv_desc* d, const float* dy, const float* w, float* dx, hipStream_t stream) {
    DwGatherParams p;
    p.C = d->Cin; p.Ti = d->Ti; p.Hi = d->Hi; p.Wi = d->Wi; p.To = d->To; p.Ho = d->Ho; p.Wo = d->Wo;
    p.sT = d->sT; p.pT = d->pT; p.pH = d->pH; p.pW = d->pW;
    p.cells_w = (d->Wi - 1 + d->pW) / d->sW + 1;
    p.cells = ((d->Hi - 1 + d->pH) / d->sH + 1) * p.cells_w;
    p.tiles = (p.cells + 255) / 256;
    const dim3 grid((unsigned)((long)d->N * d->Cin * d->Ti * p.tiles)), block(256);
    switch (((d->kT == 3) << 4) | ((d->kH == 3) << 3) | ((d->kW == 3) << 2) | ((d->sH == 2) << 1) | (d->sW == 2)) {
#define DW_CASE(KT, KH, KW, SH, SW)                                                                                              \
    case (((KT) == 3) << 4) | (((KH) == 3) << 3) | (((KW) == 3) << 2) | (((SH) == 2) << 1) | ((SW) == 2):                         \
        hipLaunchKernelGGL((dw_dgrad_class_kernel<KT, KH, KW, SH, SW>), grid, block, 0, stream, p, dy, w, dx);                    \
        break;
#define DW_STRIDES(KT, KH, KW) DW_CASE(KT, KH, KW, 1, 1) DW_CASE(KT, KH, KW, 1, 2) DW_CASE(KT, KH, KW, 2, 1) DW_CASE(KT, KH, KW, 2, 2)
        DW_STRIDES(1, 1, 1) DW_STRIDES(1, 1, 3) DW_STRIDES(1, 3, 1) DW_STRIDES(1, 3, 3)
        DW_STRIDES(3, 1, 1) DW_STRIDES(3, 1, 3) DW_STRIDES(3, 3, 1) DW_STRIDES(3, 3, 3)
#undef DW_STRIDES
#undef DW_CASE
        default: return ZSV_E_UNSUPPORTED;
    }
    return launch_status();
}

// The weight gradient's slices: a unit is one (clip, tile) with all its frames; about eight workgroups per CU over all channels,
// every slice a whole number of units.
struct DwWgradPlan { DwParams p; int slices; };
static DwWgradPlan dw_wgrad_plan(const zsv_conv_desc* d) {
    DwWgradPlan pl;
    DwParams& p = pl.p;
    p.C = d->Cin; p.Ti = d->Ti; p.Hi = d->Hi; p.Wi = d->Wi; p.To = d->To; p.Ho = d->Ho; p.Wo = d->Wo;
    p.sT = d->sT; p.pT = d->pT; p.pH = d->pH; p.pW = d->pW; p.flip = 0; p.relu = 0;
    dw_tile_plan(p, d->Ho, d->Wo, d->kT, d->kH, d->kW, d->sH, d->sW);
    p.units = d->N * p.tiles;
    const long want = clamp1((2048 + d->Cin - 1) / d->Cin, p.units < 1024 ? p.units : 1024);
    split_chunks(p.units, want, &p.units_per_slice, &pl.slices);
    return pl;
}
static size_t dw_wgrad_bytes(const zsv_conv_desc* d, int slices) {
    if (slices <= 1) return 0;
    return align256(((size_t)slices + 32) * d->Cin * d->kT * d->kH * d->kW * sizeof(float));     // slabs + the chunked sum's partials
}

}  // namespace zsv

using namespace zsv;

extern "C" {

int32_t zsv_dwconv3d_supported(const zsv_conv_desc* d) { return dw_check(d) == ZSV_OK ? 1 : 0; }

int zsv_dwconv3d_fwd(const zsv_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int fuse_relu, void* stream) {
    if (!d || !x || !w || !y) return ZSV_E_NULL;
    const int st = dw_check(d);
    if (st != ZSV_OK) return st;
    DwParams p;
    p.C = d->Cin; p.Ti = d->Ti; p.Hi = d->Hi; p.Wi = d->Wi; p.To = d->To; p.Ho = d->Ho; p.Wo = d->Wo;
    p.sT = d->sT; p.pT = d->pT; p.pH = d->pH; p.pW = d->pW; p.flip = 0; p.relu = fuse_relu ? 1 : 0;
    p.units = p.units_per_slice = 0;
    dw_tile_plan(p, d->Ho, d->Wo, d->kT, d->kH, d->kW, d->sH, d->sW);
    const dim3 grid((unsigned)((long)d->N * d->Cin * p.tiles));
    return dw_tile_launch<0>(d->kT, d->kH, d->kW, d->sH, d->sW, grid, p, x, w, bias, y, (hipStream_t)stream);
}

int zsv_dwconv3d_dgrad(const zsv_conv_desc* d, const float* dy, const float* w, float* dx, void* stream) {
    if (!d || !dy || !w || !dx) return ZSV_E_NULL;
    const int st = dw_check(d);
    if (st != ZSV_OK) return st;
    if (d->sT != 1 || d->sH != 1 || d->sW != 1) return dw_gather_launch(d, dy, w, dx, (hipStream_t)stream);
    // stride 1: the forward kernel on dY with flipped taps and padding k - 1 - p
    DwParams p;
    p.C = d->Cin; p.Ti = d->To; p.Hi = d->Ho; p.Wi = d->Wo; p.To = d->Ti; p.Ho = d->Hi; p.Wo = d->Wi;
    p.sT = 1; p.pT = d->kT - 1 - d->pT; p.pH = d->kH - 1 - d->pH; p.pW = d->kW - 1 - d->pW; p.flip = 1; p.relu = 0;
    p.units = p.units_per_slice = 0;
    dw_tile_plan(p, d->Hi, d->Wi, d->kT, d->kH, d->kW, 1, 1);
    const dim3 grid((unsigned)((long)d->N * d->Cin * p.tiles));
    return dw_tile_launch<0>(d->kT, d->kH, d->kW, 1, 1, grid, p, dy, w, nullptr, dx, (hipStream_t)stream);
}

size_t zsv_dwconv3d_wgrad_workspace_bytes(const zsv_conv_desc* d) {
    if (dw_check(d) != ZSV_OK) return 0;
    return dw_wgrad_bytes(d, dw_wgrad_plan(d).slices);
}

int zsv_dwconv3d_wgrad(const zsv_conv_desc* d, const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                       void* stream) {
    if (!d || !x || !dy || !dw) return ZSV_E_NULL;
    const int st = dw_check(d);
    if (st != ZSV_OK) return st;
    const DwWgradPlan pl = dw_wgrad_plan(d);
    const size_t need = dw_wgrad_bytes(d, pl.slices);
    if (need > 0 && (!workspace || workspace_bytes < need || !aligned16(workspace))) return ZSV_E_WORKSPACE;
    float* slabs = pl.slices > 1 ? (float*)workspace : dw;
    const dim3 grid((unsigned)d->Cin, (unsigned)pl.slices);
    const int rc = dw_tile_launch<1>(d->kT, d->kH, d->kW, d->sH, d->sW, grid, pl.p, x, nullptr, dy, slabs, (hipStream_t)stream);
    if (rc != ZSV_OK || pl.slices <= 1) return rc;
    const long n = (long)d->Cin * d->kT * d->kH * d->kW;
    if (pl.slices <= 64) return slab_sum_flat(slabs, dw, n, pl.slices, (hipStream_t)stream);
    return slab_sum_flat_chunked(slabs, slabs + (size_t)pl.slices * n, dw, n, pl.slices, (hipStream_t)stream);
}

}  // extern "C"
