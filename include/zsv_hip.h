/*
 * zsv_hip.h -- C ABI of libzsv_hip.so: the MI355X (gfx950) kernels behind the
 * 3D-conv video hot path of damien911224/ZeroShotVideoClassification.
 *
 * The reference has no native code and no FFI of its own: every entry point below
 * replaces an ATen operator that the reference's Python reaches through torch.nn
 * (SURVEY.md section 2a / 8b).  Each declaration cites the reference call site whose
 * arithmetic it supplies.  Conventions:
 *
 *   - all tensors are contiguous fp32, channel-major "NCS": (N, C, T, H, W) with
 *     S = T*H*W; pointers are device pointers owned by the caller;
 *   - kernels never allocate: workspaces are passed in (query the size first);
 *   - no byte outside the stated extent of an input may influence a result, and no input (const pointer) is written;
 *   - alignment of pointer arguments:
 *       fp32 tensors and vectors -- x, w, bias, y, dy, dx, dw, residual, add, sub, the BatchNorm vectors (gamma, beta, save_*,
 *         running_*, dgamma, dbeta), bn_partials / conv_partials, the linear operands, the cosine_topk / split_accuracy
 *         embeddings, out_dist (8 bytes: a double), zsv_clip_to_bf16's input, the clip-transform outputs -- need only their
 *         element's alignment (4 bytes), each on its own: a contiguous view that starts at an odd element offset of a larger
 *         buffer (a parameter inside one flat buffer, a bucket slice) is a legal operand.  int32 / int64 tables, labels, argmax
 *         and index outputs keep their natural alignment (4 / 8 bytes).  uint8 frames and images: any address;
 *       workspaces, weight panels, blobs, mask tables and the coefficient rows (pre_coef / coef of zsv_bn_fwd_train_coeffs,
 *         zsv_bn_eval_coeffs) are 16-byte aligned, and a size query covers every route a call with any legal alignment of
 *         its tensors can take;
 *       channels-last bf16 / e4m3 tensors (activations, residuals, fanin, dz, dx, the folded clip of zsv_clip_to_bf16) are
 *         16-byte aligned: their rows are 64-byte (clip: 8-byte) units moved as 16-byte pieces.  An entry point handed one
 *         off a 16-byte boundary returns ZSV_E_UNSUPPORTED before any launch and writes nothing.  zsv_absmax_bf16 is the
 *         exception: it takes any 2-byte aligned address;
 *     results do not depend on the alignment of the fp32 operands: a call gives the same bits as on 16-byte aligned ones
 *     wherever it runs the same kernel.  Some entry points choose the kernel by `pointer & 15`; where the other kernel sums
 *     in another order the result is that kernel's (as deterministic, within the same tolerance of the exact value).  These
 *     are: the weight gradients zsv_conv3d_wgrad and zsv_conv3d_wgrad_masked, whose LDS-DMA,
 *     temporal-ring, Winograd-form and stem-row kernels are given only x and dy on 16-byte boundaries -- otherwise the
 *     register-staged / generic kernels run, the ones ZSV_NO_WGRAD_DMA, ZSV_NO_WGRAD_TRING, ZSV_NO_WGRAD_WINO and
 *     ZSV_NO_STEM_WGRAD select (zsv_conv3d_wgrad_pre has one kernel and gives the same bits at any alignment);
 *     zsv_conv3d_fwd_stat_tiles(d, y), which answers for the y it is given: the tap kernel's statistics epilogue needs y on a
 *     16-byte boundary, 0 means "call the plain form for this y" (y itself has the same bits either way; statistic tiles asked
 *     for one y and passed with another are refused, ZSV_E_UNSUPPORTED, by zsv_conv3d_fwd_stats / _full / _pre); and
 *     zsv_relu_bwd_bias, whose db is summed in another order when S % 4 != 0 or one of dy, y, dx is off a 16-byte boundary
 *     (dx is the same bits).  Everywhere else -- the float4 forms of the element-wise, pool, BatchNorm, split-K reduce and
 *     generic-convolution kernels, the 16-byte image pieces of the Winograd and stride-2 input-gradient kernels -- alignment
 *     selects only the width of the loads and stores;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on it;
 *   - return value: 0 = OK, otherwise a ZSV_E_* code (zsv_status_string() names it);
 *     nothing throws across this boundary;
 *   - re-entrant and thread-safe (backward is called from autograd's worker thread).
 */
#ifndef ZSV_HIP_H
#define ZSV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZSV_OK 0
#define ZSV_E_BAD_SHAPE 1      /* inconsistent or unsupported geometry            */
#define ZSV_E_NULL 2           /* required pointer is NULL                        */
#define ZSV_E_WORKSPACE 3      /* workspace smaller than the *_workspace_bytes()  */
#define ZSV_E_TOO_LARGE 4      /* a tensor has >= 2^31 elements                   */
#define ZSV_E_LAUNCH 5         /* hipGetLastError() after the launch was not OK   */
#define ZSV_E_UNSUPPORTED 6    /* valid but not implemented (e.g. overlapping pool) */

/* Geometry of one Conv3d call site.  Replaces the arguments of
 * nn.Conv3d / F.conv3d at resnet.py:40-52 (Conv2Plus1D spatial 1xkxk and temporal
 * tx1x1), resnet.py:23-30 (3x3x3), resnet.py:63-70 (1x3x3), resnet.py:170,181,184
 * (stems), resnet.py:270 (1x1x1 strided shortcut) and network.py:102-117 (C3D).
 * Dilation is 1 and groups is 1 everywhere in the reference. */
typedef struct zsv_conv_desc {
    int32_t N, Cin, Ti, Hi, Wi;    /* input  (N, Cin, Ti, Hi, Wi)                 */
    int32_t Cout, To, Ho, Wo;      /* output (N, Cout, To, Ho, Wo)                */
    int32_t kT, kH, kW;            /* weight (Cout, Cin, kT, kH, kW)              */
    int32_t sT, sH, sW;            /* stride                                      */
    int32_t pT, pH, pW;            /* zero padding                                */
} zsv_conv_desc;

const char* zsv_status_string(int status);
/* build identification: "zsv_hip gfx950 <date>" */
const char* zsv_version(void);
/* The ZSV_* debug / A-B environment switches are snapshotted when the library is loaded; the launch
 * path never calls getenv().  After changing one of them in a live process call this (no launch in flight on another
 * thread); returns the number of switches that are set.  Not needed in normal use. */
int32_t zsv_reload_knobs(void);

/* ---- convolution (aten::conv3d and its autograd formulas) ------------------- */
/* y = conv3d(x, w) (+ bias[c]) (relu optional, for network.py:147-162 `relu(conv(x))`).
 * `workspace` holds the weights re-packed tap-major for the fast kernel (query the size;
 * 0 means the call needs none).  It must be 16-byte aligned; x, w, bias, residual, y (and dy, dx, dw, add, sub, bn_partials
 * below) need 4 bytes each (Conventions: alignment). */
size_t zsv_conv3d_fwd_workspace_bytes(const zsv_conv_desc* d);
/* Same, and the epilogue also emits BatchNorm partial statistics of y: bn_partials[0..Cout*tiles)
 * = per (channel, column tile) sums, then Cout*tiles sums of squares, tiles =
 * zsv_conv3d_fwd_stat_tiles(d, y) (0 = this geometry cannot; then call the plain form).  Only
 * without bias / ReLU.  Feeds zsv_bn_fwd_train_stats, which then skips its pass over y. */
int32_t zsv_conv3d_fwd_stat_tiles(const zsv_conv_desc* d, const float* y);
int zsv_conv3d_fwd_stats(const zsv_conv_desc* d, const float* x, const float* w, const float* bias,
                         float* y, int fuse_relu, float* bn_partials, int32_t stat_tiles, void* workspace,
                         size_t workspace_bytes, void* stream);
/* Inference forward with the block tail fused: y = relu?(conv3d(x, w) + bias + residual) -- with the
 * eval-mode BatchNorm folded into (w, bias) this is Conv3d -> BatchNorm3d -> `out += residual` -> ReLU
 * (resnet.py:97,110-111) in one pass.  Only where zsv_conv3d_fwd_add_supported(d) != 0 (tap kernel, no
 * split-K); `residual` has y's shape.  zsv_conv3d_fwd_full is the common form of the three entry points. */
int32_t zsv_conv3d_fwd_add_supported(const zsv_conv_desc* d);
int zsv_conv3d_fwd_add(const zsv_conv_desc* d, const float* x, const float* w, const float* bias,
                       const float* residual, float* y, int fuse_relu, void* workspace, size_t workspace_bytes,
                       void* stream);
int zsv_conv3d_fwd_full(const zsv_conv_desc* d, const float* x, const float* w, const float* bias,
                        const float* residual, float* y, int fuse_relu, float* bn_partials, int32_t stat_tiles,
                        void* workspace, size_t workspace_bytes, void* stream);
int zsv_conv3d_fwd(const zsv_conv_desc* d, const float* x, const float* w, const float* bias,
                   float* y, int fuse_relu, void* workspace, size_t workspace_bytes, void* stream);
/* dx = conv3d_input_grad(dy, w): what autograd runs for every conv but the first.  Strided
 * convolutions are solved per residue class of input voxels (no multiplies by inserted zeros). */
size_t zsv_conv3d_dgrad_workspace_bytes(const zsv_conv_desc* d);
int zsv_conv3d_dgrad(const zsv_conv_desc* d, const float* dy, const float* w, float* dx,
                     void* workspace, size_t workspace_bytes, void* stream);
/* dx = conv3d_input_grad(dy, w) + add: the gradient arriving over an identity shortcut
 * (`out += residual`, resnet.py:108-110, residual = the convolution's own input) is added in the
 * epilogue instead of by a separate pass.  Only where zsv_conv3d_dgrad_add_supported(d) != 0 (stride 1,
 * no split-K); `add` has dx's shape; add == NULL = zsv_conv3d_dgrad. */
int32_t zsv_conv3d_dgrad_add_supported(const zsv_conv_desc* d);
int zsv_conv3d_dgrad_add(const zsv_conv_desc* d, const float* dy, const float* w, const float* add, float* dx,
                         void* workspace, size_t workspace_bytes, void* stream);
/* dx = conv3d_input_grad(dy, w) + the gradient of the block's strided 1x1x1 shortcut convolution, which reads the same input
 * (`downsample`, resnet.py:240-246, next to the strided first convolution of the block, resnet.py:40-45).  `sub` is that gradient
 * in COMPACT form [N][Cin][ceil(Ti/st)][Hi/sh][Wi/sw] -- the input gradient of the 1x1x1 convolution taken at stride 1 over its
 * own output voxels -- and is added where dx[.., st*a, sh*b, sw*c] is produced: no zero-filled full-size tensor, no separate add
 * over the block input (aten's autograd: two full-size gradients summed).  Only where
 * zsv_conv3d_dgrad_add_strided_supported(d, st, sh, sw) != 0 (the merged stride-(1,2,2) kernel; st = 1 or 2, sh = sw = 2);
 * workspace as zsv_conv3d_dgrad. */
int32_t zsv_conv3d_dgrad_add_strided_supported(const zsv_conv_desc* d, int32_t st, int32_t sh, int32_t sw);
int zsv_conv3d_dgrad_add_strided(const zsv_conv_desc* d, const float* dy, const float* w, const float* sub, int32_t st, int32_t sh,
                                 int32_t sw, float* dx, void* workspace, size_t workspace_bytes, void* stream);
/* dw = conv3d_weight_grad(x, dy).  Deterministic: position range is cut into a fixed
 * number of slices, each slice writes a partial slab into `workspace`, a second kernel
 * sums the slabs in slice order. */
size_t zsv_conv3d_wgrad_workspace_bytes(const zsv_conv_desc* d);
int zsv_conv3d_wgrad(const zsv_conv_desc* d, const float* x, const float* dy, float* dw,
                     void* workspace, size_t workspace_bytes, void* stream);
/* The tap-validity table the stride-1 weight-gradient kernels read depends on the geometry only (input extents, kernel,
 * padding): zsv_conv3d_wgrad rebuilds it on every call; a caller that keeps it -- zsv_conv3d_wgrad_mask_bytes(d) bytes
 * (0: this geometry's kernel reads no table), filled once by zsv_conv3d_wgrad_mask -- passes it to zsv_conv3d_wgrad_masked
 * and saves a launch per call (mask == NULL behaves like zsv_conv3d_wgrad).  Same results bit for bit. */
size_t zsv_conv3d_wgrad_mask_bytes(const zsv_conv_desc* d);
int zsv_conv3d_wgrad_mask(const zsv_conv_desc* d, void* mask, void* stream);
int zsv_conv3d_wgrad_masked(const zsv_conv_desc* d, const float* x, const float* dy, float* dw, void* workspace,
                            size_t workspace_bytes, const void* mask, void* stream);

/* ---- depthwise convolution (groups == channels) ------------------------------------------------------ */
/* nn.Conv3d(C, C, k, groups=C): the 3x3x3 middle convolution of the channel-separated residual unit
 * (1x1x1 -> 3x3x3 depthwise -> 1x1x1 in resnet.Bottleneck's frame, resnet.py:116-162), and the 1x3x3 / 3x1x1 depthwise pairs.
 * The descriptor is zsv_conv_desc read as depthwise: Cin == Cout == C, x (N,C,Ti,Hi,Wi), w (C,1,kT,kH,kW), y (N,C,To,Ho,Wo),
 * contiguous fp32.  Supported: every kernel extent 1 or 3, every stride 1 or 2, every padding < its kernel extent
 * (zsv_dwconv3d_supported(d) == 1 exactly when the launching entry points take d).  Decided on the host before any launch:
 * ZSV_E_NULL (a missing pointer; bias may be NULL), ZSV_E_BAD_SHAPE (Cin != Cout, extents that do not follow from the formula),
 * ZSV_E_UNSUPPORTED (a consistent descriptor outside the set above), ZSV_E_TOO_LARGE (x or y of 2^31 elements or more),
 * ZSV_E_WORKSPACE.  Every operand needs 4-byte alignment only and the same inputs give the same bits at any alignment (the
 * kernels take 4-byte accesses); the workspace is 16-byte aligned.  No atomics.
 *   zsv_dwconv3d_fwd    y = relu?(conv(x, w) + bias[c]) in one launch: a ring of kT input frames' rows in LDS per workgroup.
 *   zsv_dwconv3d_dgrad  one launch that writes EVERY element of dx (voxels no output touches: 0.0).  Stride 1: the forward
 *                       kernel with flipped taps and padding k-1-p; otherwise the gather form over the taps with
 *                       (i + p - k) % s == 0.
 *   zsv_dwconv3d_wgrad  dw (C,1,kT,kH,kW): per (channel, slice of the clips x tiles) the taps' partial sums in registers,
 *                       reduced in a fixed order into a [slice][C * taps] slab row; the slabs are added in slice order. */
int32_t zsv_dwconv3d_supported(const zsv_conv_desc* d);
int zsv_dwconv3d_fwd(const zsv_conv_desc* d, const float* x, const float* w, const float* bias, float* y, int fuse_relu, void* stream);
int zsv_dwconv3d_dgrad(const zsv_conv_desc* d, const float* dy, const float* w, float* dx, void* stream);
size_t zsv_dwconv3d_wgrad_workspace_bytes(const zsv_conv_desc* d);
int zsv_dwconv3d_wgrad(const zsv_conv_desc* d, const float* x, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---- convolution fed by a BatchNorm + ReLU that is never written out ------------------------------ */
/* Conv2Plus1D runs `Conv3d(1x3x3) -> BatchNorm3d -> ReLU -> Conv3d(3x1x1)` (resnet.py:40-52).  Instead of one HBM pass
 * that normalises the 636 MB mid tensor and a second that reads it back, the temporal convolution (forward and weight
 * gradient) reads the RAW spatial output x and applies relu(x * scale[c] + shift[c]) on its way into the MFMA -- the same
 * fmaf / max as the BatchNorm apply pass: results are bit-identical to the unfused sequence.
 *   zsv_bn_fwd_train_coeffs : training-mode BatchNorm up to, but without, the normalise pass: batch statistics (from the
 *       producing convolution's epilogue partials when given), save_mean / save_invstd, running statistics, and
 *       coef = [2][coef_pitch] (scale row, shift row; coef_pitch >= C, a multiple of 16, tail zeroed; 16-byte aligned).
 *   zsv_conv3d_pre_supported: 1 when both zsv_conv3d_fwd_pre and zsv_conv3d_wgrad_pre can run this geometry.
 *   zsv_conv3d_fwd_pre / zsv_conv3d_wgrad_pre: zsv_conv3d_fwd_stats / zsv_conv3d_wgrad with x read through the affine + ReLU
 *       (same workspace sizes as their plain forms).  The input gradient is zsv_conv3d_dgrad as usual (it is the gradient
 *       w.r.t. the virtual activation), followed by zsv_bn_bwd(relu_mode = 2), which recomputes the ReLU mask from x. */
int zsv_bn_fwd_train_coeffs(const float* x, int32_t N, int32_t C, int32_t S, const float* gamma, const float* beta,
                            float* save_mean, float* save_invstd, float* running_mean, float* running_var, float momentum,
                            float eps, const float* conv_partials, int32_t stat_tiles, float* coef, int32_t coef_pitch,
                            void* workspace, size_t workspace_bytes, void* stream);
int32_t zsv_conv3d_pre_supported(const zsv_conv_desc* d);
int zsv_conv3d_fwd_pre(const zsv_conv_desc* d, const float* x, const float* pre_coef, int32_t coef_pitch, const float* w,
                       float* y, float* bn_partials, int32_t stat_tiles, void* workspace, size_t workspace_bytes,
                       void* stream);
int zsv_conv3d_wgrad_pre(const zsv_conv_desc* d, const float* x, const float* pre_coef, int32_t coef_pitch,
                         const float* dy, float* dw, void* workspace, size_t workspace_bytes, void* stream);
/* db[c] = sum over (n, s) of dy  (bias gradient of C3D's convs, network.py:102-117,
 * and of nn.Linear when S == 1). */
size_t zsv_channel_sum_workspace_bytes(int32_t N, int32_t C, int32_t S);
int zsv_channel_sum(const float* dy, int32_t N, int32_t C, int32_t S, float* db,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ---- BatchNorm3d (+ fused residual add / ReLU) ------------------------------- */
/* Training-mode forward of nn.BatchNorm3d (resnet.py:48,95,97,183,186,272) followed,
 * optionally, by `out += residual` (resnet.py:110) and ReLU (resnet.py:49,95,111):
 *   mean/var over (N, S) per channel (biased var for normalising),
 *   running_mean/var updated in place with `momentum` (unbiased var), like torch;
 *   y = relu?((x - mean) * invstd * gamma + beta + residual?)
 * save_mean / save_invstd (C floats each) are kept for backward.  Every tensor and vector of this family needs 4-byte
 * alignment only (the float4 routes are taken on S % 4 == 0 and work at any such address); the workspace 16. */
size_t zsv_bn_workspace_bytes(int32_t N, int32_t C, int32_t S);
int zsv_bn_fwd_train(const float* x, int32_t N, int32_t C, int32_t S, const float* gamma,
                     const float* beta, const float* residual, int fuse_relu, float* y,
                     float* save_mean, float* save_invstd, float* running_mean,
                     float* running_var, float momentum, float eps, void* workspace,
                     size_t workspace_bytes, void* stream);
/* Same with the batch statistics taken from the producing convolution's epilogue partials
 * (zsv_conv3d_fwd_stats) instead of a pass over x. */
int zsv_bn_fwd_train_stats(const float* x, int32_t N, int32_t C, int32_t S, const float* gamma,
                           const float* beta, const float* residual, int fuse_relu, float* y,
                           float* save_mean, float* save_invstd, float* running_mean,
                           float* running_var, float momentum, float eps, const float* conv_partials,
                           int32_t stat_tiles, void* workspace, size_t workspace_bytes, void* stream);
/* Eval-mode forward (model.eval(), main.py:229): uses the running statistics. */
int zsv_bn_fwd_eval(const float* x, int32_t N, int32_t C, int32_t S, const float* gamma,
                    const float* beta, const float* running_mean, const float* running_var,
                    const float* residual, int fuse_relu, float eps, float* y, void* workspace,
                    size_t workspace_bytes, void* stream);
/* Backward of the fused op.  fuse_relu: 0 = none; 1 = ReLU mask from the saved OUTPUT `y`
 * (cf. nn.ReLU(inplace=True), which also keeps only its output); 2 = ReLU mask recomputed from x
 * with the forward's exact fma (x*scale + shift > 0) -- valid when the forward had no residual
 * input, `y` may then be NULL and one tensor read is saved per pass.  Writes dx, dgamma, dbeta
 * and, when d_residual != NULL, the gradient flowing into the residual branch (= masked dy). */
int zsv_bn_bwd(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
               const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
               int fuse_relu, float* dx, float* d_residual, float* dgamma, float* dbeta,
               void* workspace, size_t workspace_bytes, void* stream);
/* Backward of the eval-mode (frozen statistics) fused op, y = relu?(a*x + b (+ residual)) with a = gamma / sqrt(running_var + eps),
 * b = beta - running_mean * a: g = dy * mask, dx = a * g, d_residual = g (when != NULL), dgamma = sum g * xhat with
 * xhat = (x - running_mean) / sqrt(running_var + eps), dbeta = sum g.  ONE pass over the tensors (no mean-subtraction terms),
 * then a C-wave finalize of the fixed-order partials (bitwise reproducible).  fuse_relu as zsv_bn_bwd (2: mask recomputed from
 * x with zsv_bn_fwd_eval's / zsv_bn_eval_coeffs' exact fma).  dgamma and dbeta both NULL: no reduction at all, and neither the
 * workspace nor x (with fuse_relu != 2) is read.  Workspace: zsv_bn_workspace_bytes(N, C, S). */
int zsv_bn_bwd_eval(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
                    const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                    int fuse_relu, float* dx, float* d_residual, float* dgamma, float* dbeta,
                    void* workspace, size_t workspace_bytes, void* stream);
/* Frozen (eval-mode) BatchNorm feeding a convolution that applies it: coef = [2][coef_pitch] (scale row a, shift row b as in
 * zsv_bn_bwd_eval; entries C .. coef_pitch-1 are 0) for zsv_conv3d_fwd_pre / zsv_conv3d_wgrad_pre, from the running statistics.
 * Nothing else is written.  The backward is zsv_bn_bwd_eval with fuse_relu = 2. */
int zsv_bn_eval_coeffs(int32_t C, const float* gamma, const float* beta, const float* running_mean, const float* running_var,
                       float eps, float* coef, int32_t coef_pitch, void* stream);

/* ---- BatchNorm3d with batch statistics over all ranks of a data-parallel job (torch.nn.SyncBatchNorm) ---------------------
 * The training-mode forward and backward above, cut where the ranks have to talk: the caller runs ONE collective between
 * two calls per direction and the library never sees a communicator.
 *
 *   forward :  zsv_bn_sync_moments  -> all_gather of 2C+1 doubles -> zsv_bn_sync_finalize -> zsv_bn_sync_apply
 *   backward:  zsv_bn_sync_bwd_reduce -> all_reduce(SUM) of 2C doubles -> zsv_bn_sync_bwd_apply
 *
 * The passes over the big tensors are the plain family's kernels (one read of x for the moments; read x (+ residual), write y;
 * read dy, x (, y) for the sums; read dy, x (, y), write dx (+ d_residual)) with the same float4 route on S % 4 == 0, the same
 * non-temporal streaming, the same fixed-order fp64 block sums (bitwise reproducible, no atomics) and the same per-element
 * arithmetic: the normalise fma, the ReLU masks of zsv_bn_bwd's modes 1 and 2 and the pivoted sums are the same device
 * functions.  One difference: with fuse_relu = 1 AND a residual gradient zsv_bn_bwd writes the masked gradient in its
 * reduction and reads it alone in its apply pass (7 passes); here the reduction has no tensor output and the apply pass reads
 * dy and y again (8 passes).
 *
 * moments (one rank's contribution): double[2*C + 1] = C local means | C local M2 (sum of squared deviations from the local
 *   mean) | the local count N*S.  The sums are shifted by this rank's own x[c*S] (the pivot never leaves the rank) and
 *   finalised in fp64: mean = K + s1/n, M2 = s2 - s1*s1/n (clamped at 0).  N == 0 is legal: zeros and count 0, x is not read.
 * zsv_bn_sync_finalize: gathered = double[world][2*C + 1] in rank order.  The ranks are merged in that order with Chan's
 *   pairwise update in fp64 (n = n_a + n_b, delta = mean_b - mean_a, mean += delta * n_b / n, M2 += M2_b + delta^2 * n_a * n_b / n;
 *   a rank whose count is 0 is skipped).  save_mean = mean, save_invstd = 1 / sqrt(M2 / n + eps) (biased variance);
 *   running_mean / running_var (both may be NULL) are updated in place with `momentum` and the unbiased variance over the
 *   TOTAL count, like torch; total_count_out (one double, device) = n.  Every rank computes this from the same bytes in the same
 *   order: the outputs are bit-identical across ranks.  gamma and beta are accepted for symmetry with zsv_bn_fwd_train and are
 *   not read (the apply passes form scale and shift themselves).  One launch, one thread per channel.
 * zsv_bn_sync_apply: y = relu?(fma(x, scale, shift) (+ residual)), scale = gamma * save_invstd, shift = fma(-save_mean, scale,
 *   beta) -- the expressions zsv_bn_fwd_train's finalize uses, so the mode-2 mask of the backward recomputes y's sign exactly.
 * zsv_bn_sync_bwd_reduce: sums = double[2*C] = C local sums of g | C local sums of g * xhat, g = dy * mask, xhat =
 *   (x - save_mean) * save_invstd.  fuse_relu 0, 1 (mask from y) or 2 (mask recomputed from x; y may be NULL), as zsv_bn_bwd.
 * zsv_bn_sync_bwd_apply: dx = gamma * invstd * (g - sum_g / M - xhat * sum_gx / M) with the sums of sums_global (the
 *   all-reduced buffer) and M = *total_count (a device pointer: no host read); d_residual = g when not NULL;
 *   dgamma = sum_gx, dbeta = sum_g of sums_LOCAL (either may be NULL), as torch.nn.SyncBatchNorm: the gradient all-reduce
 *   averages them afterwards.
 *
 * gamma, beta may be NULL (affine=False).  N == 0 is legal everywhere (no tensor is touched; sums are zeros, dgamma / dbeta 0).
 * Alignment: fp32 tensors and vectors 4 bytes, each on its own; the double buffers (moments, gathered, sums, total_count)
 * 8 bytes; the workspace 16.  Status: ZSV_E_BAD_SHAPE (N < 0, C <= 0, S <= 0, world <= 0, fuse_relu outside 0..2),
 * ZSV_E_TOO_LARGE (N*C*S >= 2^31), ZSV_E_NULL, ZSV_E_WORKSPACE, ZSV_E_UNSUPPORTED (a misaligned pointer); all before any launch.
 * zsv_bn_sync_workspace_bytes(N, C, S): bytes for moments and bwd_reduce on this shape (0 = illegal shape; 16 when N == 0). */
size_t zsv_bn_sync_workspace_bytes(int32_t N, int32_t C, int32_t S);
int zsv_bn_sync_moments(const float* x, int32_t N, int32_t C, int32_t S, double* moments, void* workspace,
                        size_t workspace_bytes, void* stream);
int zsv_bn_sync_finalize(const double* gathered, int32_t world, int32_t C, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, float momentum, float eps, float* save_mean,
                         float* save_invstd, double* total_count_out, void* stream);
int zsv_bn_sync_apply(const float* x, int32_t N, int32_t C, int32_t S, const float* save_mean, const float* save_invstd,
                      const float* gamma, const float* beta, const float* residual, int fuse_relu, float* y, void* stream);
int zsv_bn_sync_bwd_reduce(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
                           const float* save_mean, const float* save_invstd, const float* gamma, const float* beta,
                           int fuse_relu, double* sums, void* workspace, size_t workspace_bytes, void* stream);
int zsv_bn_sync_bwd_apply(const float* dy, const float* x, const float* y, int32_t N, int32_t C, int32_t S,
                          const float* save_mean, const float* save_invstd, const float* gamma, const float* beta,
                          int fuse_relu, const double* sums_local, const double* sums_global, const double* total_count,
                          float* dx, float* d_residual, float* dgamma, float* dbeta, void* stream);

/* ---- elementwise -------------------------------------------------------------- */
/* nn.ReLU / F.relu (resnet.py:49; network.py:147-166,614). */
int zsv_relu_fwd(const float* x, float* y, int64_t n, void* stream);
/* dx = dy * (y > 0), y = saved output. */
int zsv_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream);
/* dx = dy * (y > 0) AND db[c] = sum over (n, s) of that, in one pass (backward of C3D's fused `relu(conv(x) + bias)`,
 * network.py:147-162); (N, C, S) tensors; workspace as zsv_channel_sum. */
int zsv_relu_bwd_bias(const float* dy, const float* y, float* dx, int32_t N, int32_t C, int32_t S, float* db,
                      void* workspace, size_t workspace_bytes, void* stream);
/* out = relu(a + b): `out += residual; relu(out)` (resnet.py:110-111) when no BN is fused. */
int zsv_add_relu_fwd(const float* a, const float* b, float* y, int64_t n, void* stream);

/* ---- pooling -------------------------------------------------------------------- */
/* torch.mean(f, dim=(2,3,4)) (network.py:595) / AdaptiveAvgPool3d(1) (resnet.py:251). */
int zsv_meanpool_fwd(const float* x, int32_t N, int32_t C, int32_t S, float* y, void* stream);
int zsv_meanpool_bwd(const float* dy, int32_t N, int32_t C, int32_t S, float* dx, void* stream);
/* nn.MaxPool3d with kernel == stride (network.py:103-118); padding is -inf padding.
 * `argmax` (int32, one per output element) holds the flat (t*H+h)*W+w input index. */
int zsv_maxpool3d_fwd(const float* x, int32_t N, int32_t C, int32_t Ti, int32_t Hi, int32_t Wi,
                      int32_t kT, int32_t kH, int32_t kW, int32_t pT, int32_t pH, int32_t pW,
                      int32_t To, int32_t Ho, int32_t Wo, float* y, int32_t* argmax, void* stream);
int zsv_maxpool3d_bwd(const float* dy, const int32_t* argmax, int32_t N, int32_t C, int32_t Ti,
                      int32_t Hi, int32_t Wi, int32_t kT, int32_t kH, int32_t kW, int32_t pT,
                      int32_t pH, int32_t pW, int32_t To, int32_t Ho, int32_t Wo, float* dx,
                      void* stream);

/* ---- dense head ----------------------------------------------------------------- */
/* nn.Linear (network.py:611-616 MLP, :120,132 fc6/regressor): y = x W^T + b, optional ReLU.
 * x (rows, in), w (out, in), y (rows, out).  Implemented on the same MFMA GEMM core. */
size_t zsv_linear_fwd_workspace_bytes(int32_t rows, int32_t in_features, int32_t out_features);
int zsv_linear_fwd(const float* x, const float* w, const float* bias, float* y, int32_t rows,
                   int32_t in_features, int32_t out_features, int fuse_relu, void* workspace,
                   size_t workspace_bytes, void* stream);
size_t zsv_linear_dgrad_workspace_bytes(int32_t rows, int32_t in_features, int32_t out_features);
int zsv_linear_dgrad(const float* dy, const float* w, float* dx, int32_t rows, int32_t in_features,
                     int32_t out_features, void* workspace, size_t workspace_bytes, void* stream);
size_t zsv_linear_wgrad_workspace_bytes(int32_t rows, int32_t in_features, int32_t out_features);
int zsv_linear_wgrad(const float* x, const float* dy, float* dw, int32_t rows,
                     int32_t in_features, int32_t out_features, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- cosine nearest classes (evaluate / train accuracy) -------------------------------------- */
/* cdist(embed, class_embed, 'cosine').argsort(1)[:, :k] of compute_accuracy (main.py:316-325; k = 5 and
 * k = 1) and of the per-step train accuracy (main.py:182-185).  embed (rows, dim) and class_embed
 * (n_classes, dim) fp32, not necessarily normalised.  Distances 1 - <u,v>/(|u||v|) are formed in double
 * precision on the matrix core (v_mfma_f64_16x16x4_f64), like scipy's double cdist; out_index (rows, k)
 * int32 = the k nearest classes, ties by lower index (stable argsort); out_dist (rows, k) double may be
 * NULL.  workspace = the (rows, n_classes rounded up to 16) double distance matrix. */
size_t zsv_cosine_topk_workspace_bytes(int32_t rows, int32_t n_classes);
int zsv_cosine_topk(const float* embed, const float* class_embed, int32_t rows, int32_t dim, int32_t n_classes,
                    int32_t k, int32_t* out_index, double* out_dist, void* workspace, size_t workspace_bytes,
                    void* stream);

/* evaluate()'s scoring in one device pass: top-1 / top-5 over the whole class table (main.py:264-266 ->
 * compute_accuracy, main.py:316-325) and over the ten np.random.seed(split) half-class splits (main.py:281-304),
 * without gathering a sub-table.  pred, true_embed (rows, dim) and class_embed (n_classes, dim) fp32; labels (rows)
 * int64 (may be NULL when n_tables == 1).  split_pos (n_tables, n_classes) int32 describes the class tables:
 * split_pos[t][c] = the row of class c in class_embedding[sel_classes] (main.py:286-288; permutation order, not
 * sorted), -1 when c is not in table t; table 0 is the whole table (split_pos[0][c] = c).  Table 0 scores every row and
 * does not look at the labels; table t >= 1 scores the rows with 0 <= label < n_classes and split_pos[t][label] >= 0
 * (`l in sel_classes`, main.py:287).  Both embeddings are measured against the full table once with the double-precision
 * distances of zsv_cosine_topk (same kernel, same bits; a NaN distance ranks last).  Inside a table classes are ordered by
 * (distance, split_pos[t][c]) -- the stable argsort of the gathered sub-table; y = the first class of the true row
 * (argmin), rank = the number of classes of the table before y in the pred row; top-1 hit: rank == 0, top-5 hit: rank < 5.
 * counts (n_tables, 3) int32 = rows scored, top-1 hits, top-5 hits per table; class_counts (n_classes, 3) int32, may be
 * NULL: the same three numbers of table 0 per true class y (main.py:322, not the label).  Both are zeroed by the call, on
 * the stream.  workspace = the two (rows, n_classes rounded up to 16) double distance matrices.  ZSV_E_NULL,
 * ZSV_E_BAD_SHAPE for rows / dim / n_classes / n_tables <= 0, ZSV_E_TOO_LARGE at zsv_cosine_topk's bounds or for more
 * than 2048 tables, ZSV_E_WORKSPACE; all before any launch. */
size_t zsv_split_accuracy_workspace_bytes(int32_t rows, int32_t n_classes);
int zsv_split_accuracy(const float* pred, const float* true_embed, const int64_t* labels, const float* class_embed,
                       int32_t rows, int32_t dim, int32_t n_classes, const int32_t* split_pos, int32_t n_tables,
                       int32_t* counts, int32_t* class_counts, void* workspace, size_t workspace_bytes, void* stream);

/* ---- softmax cross-entropy (training a trunk as a classifier) -------------------------------- */
/* torch.nn.functional.cross_entropy(logits, labels, ignore_index=, label_smoothing=, reduction="mean" | "sum") without
 * class weights, its gradient, and the top-1 / top-5 hit counts of the same logits (csrc/softmax_xent.hip).  The reference
 * has no such call: it is how the trunks it downloads (resnet.py:287-289) are trained.  logits (N, C) fp32 row-major (4-byte
 * alignment is enough), labels (N) int64, both on the device.  Three launches; no atomics, no workspace, no host
 * synchronisation; the same inputs give the same bits run to run and at any alignment of logits, dlogits and dx (a thread
 * owns the same elements of a row whether the row is moved 16 or 4 bytes at a time).  The row maximum is subtracted before
 * every exp.
 *
 * _fwd, one 256-thread workgroup per row.  With lse the row's log-sum-exp, p its softmax, y its label, e = label_smoothing:
 *   row_loss[r] = (1 - e) (lse - x[y]) + e (lse - mean_j x[j]);
 *   row_rank[r] = the number of classes j with x[j] > x[y], or x[j] == x[y] and j < y (ties go to the lower index, as in
 *                 the cosine ranking above): the row is a top-k hit iff 0 <= rank < k;
 *   dlogits[r]  = p - ((1 - e) onehot(y) + e / C), NOT yet scaled by the reduction; dlogits may be NULL (no gradient wanted).
 * A row whose label equals ignore_index: loss 0, rank -1, a gradient row of zeros (written: the buffer arrives
 * uninitialised).  A row with any other label outside [0, C) breaks the contract: its loss and gradient row are NaN, its
 * rank is INT32_MAX (it counts as valid and is never a hit), and its logits are not read.  A NaN logit at the label gives
 * rank INT32_MAX as well (and a NaN loss).
 *
 * _reduce, one workgroup, fixed order: counts = {valid rows (rank >= 0), top-1 hits (rank == 0), top-5 hits (rank < 5)},
 * loss[0] = the sum of row_loss over the valid rows, divided by `valid` when mean != 0.  When EVERY row is ignored the loss
 * is 0 (and the gradient, below, is 0) -- a deliberate departure from torch, which returns NaN (0 / 0) for the mean: the
 * filter is on the device so that a batch of failed loads (label -1, auxiliary_dataset.py:502-505) needs no decision on
 * the host.
 *
 * _bwd: dx = dlogits * grad_loss[0] * (mean ? 1 / max(valid, 1) : 1) with valid = counts[0]; grad_loss is a DEVICE scalar
 * (the gradient arriving at the loss; a loss scale costs no synchronisation).  dx may be dlogits itself.
 *
 * All refusals are decided before any launch: ZSV_E_NULL; ZSV_E_BAD_SHAPE for N <= 0, C <= 0 or label_smoothing outside
 * [0, 1); ZSV_E_TOO_LARGE for N * C >= 2^31. */
int zsv_softmax_xent_fwd(const float* logits, const int64_t* labels, int32_t N, int32_t C, double label_smoothing,
                         int64_t ignore_index, float* row_loss, int32_t* row_rank, float* dlogits, void* stream);
int zsv_softmax_xent_reduce(const float* row_loss, const int32_t* row_rank, int32_t N, int32_t mean, float* loss,
                            int32_t* counts, void* stream);
int zsv_softmax_xent_bwd(const float* dlogits, const float* grad_loss, const int32_t* counts, int32_t mean, int32_t N,
                         int32_t C, float* dx, void* stream);

/* ---- optimiser ------------------------------------------------------------------ */
/* One torch.optim.Adam step (main.py:131; betas (0.9, 0.999), eps 1e-8, no weight decay,
 * no amsgrad) over a flat fp32 buffer: p, g, exp_avg, exp_avg_sq of n elements.
 * `step` is the 1-based step count (bias correction). */
int zsv_adam_step(float* p, const float* g, float* exp_avg, float* exp_avg_sq, int64_t n,
                  float lr, float beta1, float beta2, float eps, int32_t step, void* stream);

/* ---- bf16 inference path (BASELINE config 5: 32-frame bf16 eval, main.py:224-313) ------------ */
/* Forward-only convolution with eval-mode BatchNorm folded in:
 *     y = relu?( conv3d(x, w * scale[cout]) + shift[cout] (+ residual) )
 * = Conv3d -> BatchNorm3d.eval() -> ReLU (resnet.py:40-52,94-98) and `out += residual; relu`
 * (resnet.py:110-111); scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale.
 * bf16 x bf16 products accumulate in fp32 (v_mfma_f32_16x16x32_bf16).
 *
 * Activations are channels-last bf16: [N][T][H][W][Cp] with Cp = zsv_bf16_channel_pitch(C)
 * (C rounded up to 32; pad channels are written as zero).  A clip (Cin <= 4) is the exception: it is
 * stored [N][T][Hi][Wi][4] with the H/W zero border already materialised (zsv_clip_to_bf16), so its
 * conv desc carries the padded Hi/Wi and pH = pW = 0, and needs (Wo-1)*sW + 8 <= Wi.
 * `blob` = the packed bf16 weights followed by the fp32 shifts (zsv_conv3d_bf16_blob_bytes), built
 * once per layer by zsv_conv3d_bf16_pack (scale / shift may be NULL = 1 / 0: plain conv or bias).
 * `residual` (may be NULL) and y have the output's layout.  x, residual, y (dz, fanin, dx of the input gradient; the clip) and
 * the blob are 16-byte aligned -- ZSV_E_UNSUPPORTED otherwise, before any launch; w, scale, shift need 4 bytes. */
int32_t zsv_bf16_channel_pitch(int32_t channels);
size_t zsv_conv3d_bf16_blob_bytes(const zsv_conv_desc* d);
int zsv_conv3d_bf16_pack(const zsv_conv_desc* d, const float* w, const float* scale, const float* shift,
                         void* blob, void* stream);
/* The blob of the INPUT-GRADIENT problem of a convolution (bf16 training step, amp.py): `d` describes that problem -- a
 * stride-1 convolution of the (zero-interleaved) output gradient, d->Cin = the forward's Cout, d->Cout = the forward's Cin,
 * padding k-1-p -- and `w_fwd` is the FORWARD weight (forward Cout, forward Cin, kT, kH, kW) as the module holds it: channel
 * roles are swapped and the taps flipped while packing (aten::convolution_backward's input gradient, resnet.py:40-52). */
int zsv_conv3d_bf16_pack_dgrad(const zsv_conv_desc* d, const float* w_fwd, void* blob, void* stream);
/* Input gradient of a bf16 convolution (aten::convolution_backward's grad_input; resnet.py:40-52 the (2+1)D pairs, resnet.py:23-30
 * 3x3x3, resnet.py:266-273 the strided 1x1x1 shortcut), ANY stride with sT*sH*sW <= 8, in ONE convolution launch.  `d` is the FORWARD
 * descriptor.  dz is [N][To][Ho][Wo][pitch(Cout)], dx and `fanin` are [N][Ti][Hi][Wi][pitch(Cin)], channels-last bf16; pad channels
 * of dx are written zero (fanin's are zero by its layout); no workspace, nothing allocates.
 *   zsv_conv3d_bf16_dgrad_blob_bytes: bytes of the packed weights; 0 = unsupported geometry (the folded clip form Cin <= 4, more
 *     than 8 residue classes, more than 32 taps in a class, padding > kernel - 1); for stride (1,1,1) it is
 *     zsv_conv3d_bf16_blob_bytes of the stride-1 input-gradient problem and the blob is zsv_conv3d_bf16_pack_dgrad's.
 *   zsv_conv3d_bf16_dgrad_pack: one launch; reads the FORWARD weight (Cout, Cin, kT, kH, kW) as the module holds it and writes, for
 *     every residue class (rho_t, rho_h, rho_w) of the input positions i = s*j + rho, the sub-weight of the taps r + s*m,
 *     r = (rho + p) mod s, channel roles swapped and taps flipped.
 *   zsv_conv3d_bf16_dgrad: one launch whose grid is the column tiles of all classes; a class no tap reaches (7 of the 8 classes of the
 *     1x1x1 stride-2 shortcut, the remainder rows / columns of odd extents) stores zero; every element of dx is written exactly
 *     once.  `fanin` (may be NULL, may equal dx): dx = bf16( float(bf16(acc)) + float(fanin) ) -- the gradient is rounded to bf16
 *     first and the fan-in added to that, exactly what an element-wise bf16 add of the two tensors gives (the residual joins of
 *     resnet.py:110-111's backward); zsv_conv3d_bf16_fwd's `residual` adds BEFORE the rounding and is unchanged.  Stride (1,1,1)
 *     runs zsv_conv3d_bf16_fwd's kernels on the stride-1 problem.
 * ZSV_E_NULL for a NULL d / w_fwd / blob / dz / dx, ZSV_E_UNSUPPORTED where blob_bytes is 0 for a valid descriptor; all before
 * any launch. */
size_t zsv_conv3d_bf16_dgrad_blob_bytes(const zsv_conv_desc* d);
int zsv_conv3d_bf16_dgrad_pack(const zsv_conv_desc* d, const float* w_fwd, void* blob, void* stream);
int zsv_conv3d_bf16_dgrad(const zsv_conv_desc* d, const void* dz, const void* blob, const void* fanin, void* dx, void* stream);
int zsv_conv3d_bf16_fwd(const zsv_conv_desc* d, const void* x, const void* blob, const void* residual,
                        int fuse_relu, void* y, void* stream);
/* The same forward in front of a training-mode BatchNorm (no residual, no ReLU) with the BatchNorm's batch statistics taken in the
 * epilogue: per column tile the per-channel sum and sum of squares of the values AS STORED (rounded to bf16: what a pass over y would
 * read) go to bn_partials[row][0 / 1][Cp] (Cp = Cout rounded up to 32), `*rows` rows of them; zsv_conv3d_bf16_stat_rows(d) is an
 * upper bound for the caller's allocation.  zsv_bn_cl_fwd_train_stats then skips its statistics pass (resnet.py:46-47,96-97 under
 * main.py:172's autocast). */
int32_t zsv_conv3d_bf16_stat_rows(const zsv_conv_desc* d);
int zsv_conv3d_bf16_fwd_stats(const zsv_conv_desc* d, const void* x, const void* blob, void* y, float* bn_partials,
                              int32_t rows_capacity, int32_t* rows, void* stream);
/* (N, C<=4, T, H, W) fp32 clip -> [N][T][Hp][Wp][4] bf16, the frame placed at (padH, padW) inside a
 * zero border; Hp >= H + padH, Wp >= W + padW. */
int zsv_clip_to_bf16(const float* x, int32_t N, int32_t C, int32_t T, int32_t H, int32_t W, int32_t padH,
                     int32_t padW, int32_t Hp, int32_t Wp, void* out, void* stream);
/* nn.MaxPool3d with kernel == stride (network.py:148-163: C3D's five pools) on channels-last bf16 [N][T][H][W][Cp]; padding is
 * -inf padding (2 * pad <= kernel).  The bf16 evaluation engine of network.C3D (inference.Bf16EngineC3D). */
int zsv_maxpool3d_bf16(const void* x, int32_t N, int32_t C, int32_t Ti, int32_t Hi, int32_t Wi, int32_t kT, int32_t kH, int32_t kW,
                       int32_t pT, int32_t pH, int32_t pW, int32_t To, int32_t Ho, int32_t Wo, void* y, void* stream);
/* [N][S][Cp] bf16 -> (N, C) fp32 mean over the S voxels (resnet.py:251-254 avgpool + flatten). */
int zsv_meanpool_bf16(const void* x, int32_t N, int32_t S, int32_t C, float* out, void* stream);

/* ---- e4m3 inference path (the eval loop of main.py:224-313 in OCP fp8) ------------ */
/* The same folded forward as zsv_conv3d_bf16_fwd (Conv3d -> BatchNorm3d.eval() -> ReLU, resnet.py:40-52,94-98, and
 * `out += residual; relu`, resnet.py:110-111) with e4m3 (float8_e4m3fn: max 448, no inf) operands:
 *     y = sat_e4m3( relu?( acc * wscale[cout] + shift[cout] (+ residual) ) ),  acc = sum of e4m3 x e4m3 products in fp32
 * (v_mfma_f32_16x16x32_fp8_fp8).  Weights: w * scale quantised per produced channel, wscale = max|w * scale| / 448.
 * Activations are not scaled.  Conversions saturate: beyond +-448 gives +-448, never NaN.
 *
 * Activations are channels-last e4m3: [N][T][H][W][Cp] with Cp = zsv_fp8_channel_pitch(C) (C rounded up to 64, one K chunk;
 * pad channels are written as zero).  A clip (Cin <= 4) stays in the bf16 folded form of zsv_clip_to_bf16 (same descriptor
 * rules as zsv_conv3d_bf16_fwd, bf16 operands) and only its output is e4m3.  `blob` = the packed weights (e4m3, or bf16 for a
 * clip) followed by Mp fp32 shifts and Mp fp32 wscale factors (zsv_conv3d_fp8_blob_bytes), built once per layer by
 * zsv_conv3d_fp8_pack (scale / shift may be NULL = 1 / 0).  `residual` (may be NULL) and y have the output's layout, e4m3.
 * Alignment as in the bf16 path: 16 bytes for x, residual, y and the blob (ZSV_E_UNSUPPORTED otherwise), 4 for w, scale, shift. */
int32_t zsv_fp8_channel_pitch(int32_t channels);
size_t zsv_conv3d_fp8_blob_bytes(const zsv_conv_desc* d);
int zsv_conv3d_fp8_pack(const zsv_conv_desc* d, const float* w, const float* scale, const float* shift, void* blob, void* stream);
int zsv_conv3d_fp8_fwd(const zsv_conv_desc* d, const void* x, const void* blob, const void* residual, int fuse_relu, void* y,
                       void* stream);
/* [N][S][Cp] e4m3 -> (N, C) fp32 mean over the S voxels (resnet.py:251-254 avgpool + flatten). */
int zsv_meanpool_fp8(const void* x, int32_t N, int32_t S, int32_t C, float* out, void* stream);
/* network.C3D in e4m3 (inference.Fp8EngineC3D).  C3D has no normalisation, so layer l stores true / a_l with one
 * static power-of-two scale a_l per layer taken from calibration clips; the convolutions above do the arithmetic unchanged
 * (pack with scale[m] = a_{l-1} / a_l and shift[m] = bias[m] / a_l).
 * zsv_maxpool3d_fp8: nn.MaxPool3d with kernel == stride (network.py:148-163: C3D's five pools) on channels-last e4m3
 *   [N][T][H][W][Cp], Cp = zsv_fp8_channel_pitch(C); the rules of zsv_maxpool3d_bf16 (-inf padding, 2 * pad <= kernel).  The
 *   codes are compared as sign-magnitude integers: the result is exact (one of the inputs), pad channels are written as zero;
 *   what comes out for the two NaN codes (which the saturating epilogue never writes) is unspecified.
 * zsv_absmax_bf16: *amax = max(*amax, max_i |x_i|) over `count` bf16 values (the calibration pass over network.py:147-162's
 *   relu(conv(x)) outputs on the bf16 engine): one read, no temporary, no host synchronisation; *amax is a device scalar >= 0
 *   that several calls fold into (integer maximum of the bit patterns: deterministic); inf / NaN inputs give inf / NaN. */
int zsv_maxpool3d_fp8(const void* x, int32_t N, int32_t C, int32_t Ti, int32_t Hi, int32_t Wi, int32_t kT, int32_t kH, int32_t kW,
                      int32_t pT, int32_t pH, int32_t pW, int32_t To, int32_t Ho, int32_t Wo, void* y, void* stream);
int zsv_absmax_bf16(const void* x, int64_t count, float* amax, void* stream);

/* ---- bf16 TRAINING step: the reference's mixed-precision step (main.py:172 `with autocast():`, main.py:137,195-203
 * GradScaler) on channels-last bf16 activations [R = N*T*H*W][Cp] (the layout of the bf16 convolution above).  Under
 * autocast aten::batch_norm keeps fp32 statistics / affine parameters on a reduced-precision input and writes the reduced
 * precision; `out += residual; relu` (resnet.py:110-111) are element-wise passes in it.
 * zsv_bn_cl_fwd_train: train-mode BatchNorm3d (resnet.py:42,50,96,97,184,272) of the raw convolution output z: batch
 *   statistics (fp32 / fp64 accumulation), running statistics updated as torch does (unbiased variance, `momentum`),
 *   y = relu?(gamma*(z-mean)*invstd + beta (+ residual)) rounded once to bf16; save_mean / save_invstd (C floats) for backward.
 * zsv_bn_cl_bwd: g = dy * (y > 0) when relu_mask (y = the forward's output), dgamma / dbeta (C floats, may be NULL),
 *   dz (bf16) = the BatchNorm input gradient; g_out (may be NULL) receives g itself -- the gradient of a residual branch.
 *   save_coef (may be NULL): 2 * Cp floats, the forward's scale a and shift b per (padded) channel.  Passed back as `fwd_coef`
 *   with y == NULL (no residual in the forward) the backward recomputes the ReLU mask as fma(z, a, b) > 0 -- exactly what the
 *   forward rounded to y -- and does not read the saved output at all (4 of its 14 bytes per element).
 * workspace: zsv_bn_cl_workspace_bytes(R, C) bytes (0 = unsupported shape).  Every channels-last operand of this family (z, residual,
 * y, dy, dz, g_out, x / dx of the pools and converters) is 16-byte aligned, ZSV_E_UNSUPPORTED otherwise; the fp32 vectors,
 * coefficient rows and fp32 tensors (dw, dpooled, the NCS side of the converters) need 4 bytes. */
size_t zsv_bn_cl_workspace_bytes(int64_t R, int32_t C);
int zsv_bn_cl_fwd_train(const void* z, const void* residual, int64_t R, int32_t C, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float momentum, float eps, int fuse_relu, void* y,
                        float* save_mean, float* save_invstd, float* save_coef, void* workspace, size_t workspace_bytes, void* stream);
/* The same with the batch statistics taken by the producing convolution's epilogue (zsv_conv3d_bf16_fwd_stats: `conv_rows` rows of
 * [2][Cp] partial sums): the statistics pass over z is skipped. */
int zsv_bn_cl_fwd_train_stats(const void* z, const void* residual, int64_t R, int32_t C, const float* gamma, const float* beta,
                              float* running_mean, float* running_var, float momentum, float eps, int fuse_relu, void* y,
                              float* save_mean, float* save_invstd, float* save_coef, const float* conv_partials, int32_t conv_rows,
                              void* workspace, size_t workspace_bytes, void* stream);
int zsv_bn_cl_bwd(const void* dy, const void* y, const void* z, int64_t R, int32_t C, const float* gamma, const float* save_mean,
                  const float* save_invstd, const float* fwd_coef, int relu_mask, void* dz, void* g_out, float* dgamma, float* dbeta,
                  void* workspace, size_t workspace_bytes, void* stream);
/* Eval-mode (frozen statistics) BatchNorm3d on channels-last bf16, statistics and affine fp32 (frozen-BatchNorm fine-tuning under
 * autocast):
 * zsv_bn_cl_fwd_eval: coef = [4][Cp] floats (a = gamma/sqrt(running_var + eps), b = beta - running_mean*a, invstd, running_mean;
 *   pad channels 0) and y = relu?(fma(z, a, b) (+ residual)) rounded once to bf16.  No statistics pass; the running statistics
 *   are only read.  Keep coef for the backward.
 * zsv_bn_cl_bwd_eval: ONE pass: g = dy * mask (relu_mask: y > 0 with y != NULL, else fma(z, a, b) > 0 -- the forward's exact
 *   mask), dz = a*g (bf16), g_out = g (may be NULL); with dgamma and/or dbeta (C floats, may be NULL) fixed-order partials of
 *   sum g, sum g*z in the workspace (zsv_bn_cl_workspace_bytes(R, C)) and a finalize: dbeta = sum g,
 *   dgamma = invstd * (sum g*z - running_mean * sum g).  Neither: no reduction, no workspace, z read only for the mask. */
int zsv_bn_cl_fwd_eval(const void* z, const void* residual, int64_t R, int32_t C, const float* gamma, const float* beta,
                       const float* running_mean, const float* running_var, float eps, int fuse_relu, void* y, float* coef,
                       void* stream);
int zsv_bn_cl_bwd_eval(const void* dy, const void* y, const void* z, int64_t R, int32_t C, const float* coef, int relu_mask, void* dz,
                       void* g_out, float* dgamma, float* dbeta, void* workspace, size_t workspace_bytes, void* stream);
/* Weight gradient of a convolution from channels-last bf16 operands (x [N][Ti][Hi][Wi][CinP], dz [N][To][Ho][Wo][CoutP]) with
 * fp32 accumulation: dw (Cout, Cin, kT, kH, kW) fp32 -- aten::convolution_backward's weight gradient under autocast
 * (resnet.py:40-52 1x3x3 / 3x1x1 incl. the strided ones, resnet.py:23-30 3x3x3, resnet.py:270 1x1x1).  The workspace holds
 * per-slice partial sums; zsv_conv3d_bf16_wgrad_workspace_bytes() == 0 means "not this kernel's geometry" (the clip
 * convolution, other kernel shapes, tensors of 4 GiB and more): the caller converts the operands (below) and uses
 * zsv_conv3d_wgrad. */
size_t zsv_conv3d_bf16_wgrad_workspace_bytes(const zsv_conv_desc* d);
int zsv_conv3d_bf16_wgrad(const zsv_conv_desc* d, const void* x, const void* dz, float* dw, void* workspace, size_t workspace_bytes,
                          void* stream);
/* C3D's half of the mixed-precision step (network.py:147-163 under autocast: `relu(conv(x) + bias)` and MaxPool3d backward):
 * zsv_maxpool3d_bf16_bwd: gradient of zsv_maxpool3d_bf16 -- dy goes to each window's FIRST maximum in (t, h, w) order per channel
 *   (aten::max_pool3d_with_indices' argmax, recomputed from the saved input x), zero elsewhere;
 * zsv_relu_bias_bwd_cl: g = dy * (y > 0) in bf16 and dbias[c] = sum of g over the R rows (fp32 / fp64 accumulation); workspace =
 *   zsv_bn_cl_workspace_bytes(R, C). */
int zsv_maxpool3d_bf16_bwd(const void* dy, const void* x, int32_t N, int32_t C, int32_t Ti, int32_t Hi, int32_t Wi, int32_t kT, int32_t kH,
                           int32_t kW, int32_t pT, int32_t pH, int32_t pW, int32_t To, int32_t Ho, int32_t Wo, void* dx, void* stream);
int zsv_relu_bias_bwd_cl(const void* dy, const void* y, int64_t R, int32_t C, void* g_out, float* dbias, void* workspace,
                         size_t workspace_bytes, void* stream);
/* layout converters between the two activation layouts: [N][S][Cp] bf16 <-> (N, C, S) fp32 (C > 4; pad channels read as /
 * written with zero): they hand a bf16 tensor to the fp32 NCDHW kernels (weight gradients of the mixed-precision step). */
int zsv_cl_bf16_to_ncs_f32(const void* x, int32_t N, int32_t S, int32_t C, float* out, void* stream);
int zsv_ncs_f32_to_cl_bf16(const float* x, int32_t N, int32_t S, int32_t C, void* out, void* stream);
/* gradient of zsv_meanpool_bf16 (network.py:595 under autocast): dx[n][s][c] = dpooled[n][c] / S in bf16 */
int zsv_meanpool_bf16_bwd(const float* dpooled, int32_t N, int32_t S, int32_t C, void* dx, void* stream);

/* ---- clip pre-processing ------------------------------------------------------ */
/* The reference's transform chain (auxiliary/transforms.py:41-56): (u8/255 - 1)/2 and THWC->CTHW
 * (:116-117), bilinear resize of the short side to 128 with align_corners=False (:99-107), a
 * crop x crop window at (top, left) of the resized frame (:80-97,132-158) and an optional horizontal
 * flip (:188-195), fused into one pass.  frames_u8: (N, T, Hin, Win, 3) uint8;
 * crop_flip_params_device: N x {top, left, flip} int32 on the device; out: (N, 3, T, crop, crop)
 * fp32.  Hres/Wres = floor(Hin*scale), floor(Win*scale); inv_scale = (float)(1/scale).
 * Rounding: the source coordinate is fma(inv_scale, dst + 0.5, -0.5) and each of the three blends is
 * fma(l, b, (1 - l) * a), nothing else fused.  The uint8 frames and images of this family may start at any address, the int32 /
 * int64 tables at their natural alignment, out at 4 bytes.  Builds before zsv_clip_transform_batch existed left the fusing to the
 * compiler, and which product of a blend was fused depended on the loop version a pixel went through: against those
 * builds an output can differ in its last bit (within the 2e-6 of the reference's chain either way). */
int zsv_clip_transform(const uint8_t* frames_u8, int32_t N, int32_t T, int32_t Hin, int32_t Win,
                       int32_t Hres, int32_t Wres, float inv_scale, int32_t crop,
                       const int32_t* crop_flip_params_device, float* out, void* stream);
/* The same chain for a batch of B videos of different frame sizes in one launch: what the reference's loader
 * (auxiliary/auxiliary_dataset.py:158-208,498-510) does per video on a CPU worker -- native-size decode, ONE crop / flip
 * draw shared by the n_clips clips of the video, then the (nc*T) -> (nc, 3, T) reshuffle of :506-510 -- before it
 * collates.  video_table_device: B rows of ZSV_CLIP_ROW int64 on the device, row b =
 *   [0] device pointer of the video's (n_clips*T, Hin, Win, 3) uint8 frames, contiguous
 *   [1] Hin  [2] Win  [3] Hres  [4] Wres      (Hres/Wres = floor(Hin*scale), floor(Win*scale), as above)
 *   [5] top  [6] left                         (0 <= top <= Hres - crop, 0 <= left <= Wres - crop)
 *   [7] low 32 bits: flip (0 / 1); high 32 bits: the bits of inv_scale = (float)(1/scale)
 * out: (B, n_clips, 3, T, crop, crop) fp32; frame f of video b lands at clip f / T, time f % T (the
 * reshape(3, nc, T, c, c).transpose(0, 1) of :510).  Per pixel the arithmetic is zsv_clip_transform's (one device
 * function serves both kernels): on videos of one size the two agree bit for bit.  Checked before any launch:
 * ZSV_E_NULL, ZSV_E_BAD_SHAPE for B, n_clips, T, crop <= 0, ZSV_E_TOO_LARGE when out has >= 2^33 elements (the rule
 * above) or n_clips*T or B exceeds 65535 (grid y / z).  The table lives on the device: the caller checks its rows
 * (preprocess.VideoClips does).  The kernel clamps its source indices to the frame, so no top / left / flip value
 * can make a read leave the video's own frames; a row that breaks the contract (null pointer, window outside the
 * resized frame, inv_scale <= 0) is never read and its frames become NaN. */
#define ZSV_CLIP_ROW 8
int zsv_clip_transform_batch(const int64_t* video_table_device, int32_t B, int32_t n_clips, int32_t T,
                             int32_t crop, float* out, void* stream);

/* ---- camera-motion clips from still images (main.py --dataset sun2both) ---------------------- */
/* ImageDataset.extract_camera_motion (auxiliary/auxiliary_stillimages.py:130-137) on the device: every frame is
 * img[top:top+side, left:left+side] through crop_transform (:56-62) = PIL's antialiased bilinear uint8 resample to
 * crop x crop (two integer passes, horizontal first, 22-bit coefficients), then ((u8/255) - mean_c) / std_c in fp32
 * with the Kinetics mean / std of :60-61.  Bit-identical to the reference, not a tolerance.
 * image_table_device: B x {pointer, H, W} int64 on the device, each image (H, W, 3) uint8 contiguous, sizes may
 * differ; frame_table_device: B*n_clips*T x {top, left, side} int32 on the device, frame f of image b lands at
 * clip f / T, time f % T (the reshape + transpose(1, 2) of :137); out: (B, n_clips, 3, T, crop, crop) fp32.
 * max_side = the largest side in the frame table; crop <= max_side <= 8 * crop (17 taps per axis), otherwise
 * ZSV_E_BAD_SHAPE before any launch.  The frame table itself lives on the device: the caller checks that every
 * window lies inside its image and crop <= side <= max_side (preprocess.StillImageClips does); a frame that breaks
 * this is never read and its output becomes NaN. */
int zsv_still_image_clips(const int64_t* image_table_device, const int32_t* frame_table_device, int32_t B,
                          int32_t n_clips, int32_t T, int32_t crop, int32_t max_side, float* out, void* stream);
/* The integer coefficient table of one side -> crop resample, from the device code zsv_still_image_clips uses
 * (PIL's precompute_coeffs + normalize_coeffs_8bpc behind Resize at auxiliary_stillimages.py:58; computed in
 * fp64 without contraction).  coeffs: [crop][ksize] int32 with ksize = 2 * ceil(side / crop) + 1, zero past each
 * window; bounds: [crop][2] int32 = (first, count).  crop <= side <= 8 * crop. */
int zsv_resample_coeffs(int32_t side, int32_t crop, int32_t* coeffs, int32_t* bounds, void* stream);

/* The same update for every parameter tensor of a model in ONE launch (the reference's
 * optimizer.step(), main.py:200, is ~113 tensors).  `table_device` is a device array of `count`
 * descriptors sorted by first_chunk; a chunk is 4096 elements; first_chunk = running sum of
 * ceil(n / 4096) over the preceding tensors; total_chunks = that sum over all tensors. */
typedef struct zsv_adam_tensor {
    float* p;
    const float* g;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    int64_t first_chunk;
} zsv_adam_tensor;
/* `lr` is a float in the four zsv_adam_multi* entry points and a double in the four zsv_adamw_multi*; both families form
 * lr / (1 - beta1^step) in double, the first from (double)(float)lr. */
int zsv_adam_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, float lr,
                   float beta1, float beta2, float eps, int32_t step, void* stream);

/* ---- loss scaling: torch.cuda.amp.GradScaler on the device (main.py:137,195-203) ------------------ */
/* The reference trains with `scaler.scale(loss).backward(); scaler.step(optimizer); scaler.update()`.
 * The state lives in device memory so a step never waits for the host:
 *   scale          current loss scale (GradScaler default 65536)
 *   growth_tracker consecutive steps without a non-finite gradient
 *   found_inf      set by zsv_grad_check_multi, consumed by zsv_adam_multi_scaled, cleared by zsv_scaler_update
 *   steps_done     optimizer steps actually taken (skipped steps do not count): the Adam bias correction uses it */
typedef struct zsv_scaler_state {
    float scale;
    int32_t growth_tracker;
    int32_t found_inf;
    int32_t steps_done;
} zsv_scaler_state;
/* found_inf |= any(!isfinite(g)) over the gradients named by an Adam table (the `g` / `n` / `first_chunk` fields;
 * typically the flat all-reduce buckets of the data-parallel exchange): _amp_foreach_non_finite_check_and_unscale_
 * without the write-back -- the unscale itself happens inside zsv_adam_multi_scaled. */
int zsv_grad_check_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks,
                         zsv_scaler_state* state_device, void* stream);
/* zsv_adam_multi with g * (1 / scale) as the gradient, skipped entirely when found_inf is set (scaler.step,
 * main.py:200); step number = steps_done + 1 read on the device. */
int zsv_adam_multi_scaled(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, float lr,
                          float beta1, float beta2, float eps, const zsv_scaler_state* state_device, void* stream);
/* scaler.update() (main.py:203): found_inf ? scale *= backoff, tracker = 0 : (++tracker == interval ? scale *= growth,
 * tracker = 0); steps_done += !found_inf; found_inf = 0.  GradScaler defaults: 2.0, 0.5, 2000. */
int zsv_scaler_update(zsv_scaler_state* state_device, float growth_factor, float backoff_factor,
                      int32_t growth_interval, void* stream);

/* ---- weight decay and global-norm gradient clipping for the multi-tensor Adam step ---------------------------------
 * torch.optim.Adam(weight_decay=) / torch.optim.AdamW, torch.nn.utils.clip_grad_norm_ (norm_type 2) and
 * GradScaler.unscale_ over the same descriptor tables as zsv_adam_multi.  A clipped step is three launches:
 *   zsv_grad_norm_multi     one pass over the gradients: sum of squares per 4096-element chunk (+ the non-finite check)
 *   zsv_grad_norm_finalize  fixed-order sum of the partials in double -> {total_norm, clip_coef} in device memory
 *   zsv_adamw_multi[_scaled] the update, reading clip_coef on the device (the gradients in memory are not rewritten)
 * No floating-point atomics: equal gradients give equal norm bits and equal parameter bits on every run. */
typedef struct zsv_clip_record {
    float total_norm;   /* 2-norm of all (unscaled) gradients, before clipping */
    float clip_coef;    /* min(1, max_norm / (total_norm + 1e-6)) */
} zsv_clip_record;
/* Bytes of the partials buffer for `total_chunks` chunks (one float per chunk), summed over every table that
 * contributes to one norm. */
size_t zsv_grad_norm_workspace_bytes(int64_t total_chunks);
/* partials[chunk_offset + c] = sum of g^2 over chunk c of the table, c in [0, total_chunks).  Several parameter groups are
 * several tables: launch once per table with chunk_offset = the chunks of the tables before it.  With a non-NULL
 * `state_device`, found_inf is set exactly as zsv_grad_check_multi sets it, so one read of the gradients serves both. */
int zsv_grad_norm_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, int64_t chunk_offset,
                        void* partials_device, size_t partials_bytes, zsv_scaler_state* state_device, void* stream);
/* total_norm = sqrt(sum of partials[0 .. total_chunks)) (summed in double, fixed order), times (float)(1 / (double)scale)
 * when `state_device` is non-NULL (the gradients in memory are scaled); clip_coef = min(1, max_norm / (total_norm + 1e-6)).
 * max_norm > 0; +inf gives the norm alone (clip_coef 1). */
int zsv_grad_norm_finalize(const void* partials_device, int64_t total_chunks, float max_norm,
                           const zsv_scaler_state* state_device, zsv_clip_record* record_device, void* stream);
/* GradScaler.unscale_: g *= (float)(1 / (double)scale) in place (the table's `g` is written), found_inf |= any
 * non-finite gradient. */
int zsv_grad_unscale_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks,
                           zsv_scaler_state* state_device, void* stream);
/* zsv_adam_multi with weight decay and clipping.  Per element, in this order:
 *   g = g_mem * clip_coef                       (clip_device may be NULL: 1)
 *   L2 (decoupled == 0):   g += weight_decay * p                                  torch.optim.Adam(weight_decay=)
 *   exp_avg, exp_avg_sq as in zsv_adam_multi
 *   decoupled != 0:        p *= (float)(1 - lr * weight_decay)  (formed in double) torch.optim.AdamW
 *   p -= step_size * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^step) + eps) */
int zsv_adamw_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr, float beta1,
                    float beta2, float eps, double weight_decay, int32_t decoupled, const zsv_clip_record* clip_device,
                    int32_t step, void* stream);
/* The same under the loss scaler: skipped entirely (decay included) when found_inf is set; g = g_mem * (1 / scale) *
 * clip_coef, or g_mem * clip_coef when `grads_unscaled` != 0 (zsv_grad_unscale_multi has already run on this table);
 * step number = steps_done + 1 read on the device. */
int zsv_adamw_multi_scaled(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr, float beta1,
                           float beta2, float eps, double weight_decay, int32_t decoupled,
                           const zsv_clip_record* clip_device, const zsv_scaler_state* state_device,
                           int32_t grads_unscaled, void* stream);

/* ---- gradient accumulation over several backward passes (ddp.GradientSync, begin_step(passes=k)) ---------------------
 * Folds a set of freshly produced gradient tensors into their slices of a flat accumulator (a gradient bucket) in ONE
 * launch.  `table_device`: `count` descriptors sorted by first_chunk, chunks of 4096 elements exactly as for
 * zsv_adam_multi.  `acc` and `g` need only be 4-byte aligned, each on its own (bucket slices start at element offsets);
 * no element outside [acc, acc + n) is written and none outside [g, g + n) is read.
 *   assign != 0: acc = scale * g        (first pass of a step: no zero-fill pass over the bucket)
 *   assign == 0: acc = acc + scale * g  (computed as fl(acc + fl(scale * g)): no contraction into an fma)
 * No atomics: the result is bit-reproducible.  Non-finite gradients are data: they propagate into acc as IEEE
 * arithmetic says (the loss scaler's check then sees them in the accumulated bucket). */
typedef struct zsv_accum_tensor {
    float* acc;
    const float* g;
    int64_t n;
    int64_t first_chunk;
} zsv_accum_tensor;
int zsv_grad_accum_multi(const zsv_accum_tensor* table_device, int32_t count, int64_t total_chunks, float scale,
                         int32_t assign, void* stream);

/* ---- weight averaging (EMA / SWA) fused into the Adam step: torch.optim.swa_utils.AveragedModel on the device ----------
 * A "shadow" holds the running average of a parameter (or of a BatchNorm running statistic).  The count of optimizer
 * steps averaged so far lives in device memory, so neither the "first averaged step copies" rule nor a step the loss
 * scaler skips needs the host.  Per element, with p the value the update has just produced:
 *   n_averaged == 0:           avg = p                                   (AveragedModel's first update: an exact copy)
 *   w = ema_weight             when ema_weight >= 0: EMA, the caller passes (float)(1.0 - decay)
 *   w = 1.f / (n_averaged + 1) when ema_weight <  0: equal-weight running mean (SWA)
 *   avg = w < 0.5 ? avg + w * (p - avg) : p - (p - avg) * (1 - w)        (torch.lerp(avg, p, w))
 * All fp32, chunked by 4096 elements, no atomics: the same inputs give the same bits on every run. */
typedef struct zsv_avg_state {
    int32_t n_averaged;   /* optimizer steps averaged so far (skipped steps do not count) */
} zsv_avg_state;
/* zsv_adam_multi / zsv_adam_multi_scaled / zsv_adamw_multi / zsv_adamw_multi_scaled with the average folded in:
 * `shadows_device` is a device array of `count` pointers, parallel to the table (shadows_device[i] has table[i].n elements,
 * 4-byte aligned); each launch updates p, exp_avg and exp_avg_sq to the very bits its plain form gives and then applies
 * the rule above to the shadow with the new p.  They read `avg_state_device` and do not advance it (zsv_avg_advance).
 * Under the loss scaler a launch that returns on found_inf leaves the shadows untouched. */
int zsv_adam_multi_avg(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, float lr, float beta1,
                       float beta2, float eps, int32_t step, float* const* shadows_device,
                       const zsv_avg_state* avg_state_device, float ema_weight, void* stream);
int zsv_adam_multi_scaled_avg(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, float lr,
                              float beta1, float beta2, float eps, const zsv_scaler_state* state_device,
                              float* const* shadows_device, const zsv_avg_state* avg_state_device, float ema_weight,
                              void* stream);
int zsv_adamw_multi_avg(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr, float beta1,
                        float beta2, float eps, double weight_decay, int32_t decoupled, const zsv_clip_record* clip_device,
                        int32_t step, float* const* shadows_device, const zsv_avg_state* avg_state_device,
                        float ema_weight, void* stream);
int zsv_adamw_multi_scaled_avg(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr,
                               float beta1, float beta2, float eps, double weight_decay, int32_t decoupled,
                               const zsv_clip_record* clip_device, const zsv_scaler_state* state_device,
                               int32_t grads_unscaled, float* const* shadows_device,
                               const zsv_avg_state* avg_state_device, float ema_weight, void* stream);
/* A pair of equally long fp32 arrays for zsv_avg_multi (a = the live value, read; b = its shadow) and zsv_swap_multi.
 * `a` and `b` need only be 4-byte aligned, each on its own (shadows are slices of a flat buffer); tables are sorted by
 * first_chunk exactly as for zsv_adam_multi.  No element outside [b, b + n) -- and, for the swap, [a, a + n) -- is written. */
typedef struct zsv_pair_tensor {
    float* a;
    float* b;
    int64_t n;
    int64_t first_chunk;
} zsv_pair_tensor;
/* The averaging rule over a table, b = rule(b, a): for values no Adam launch produces (BatchNorm running statistics).
 * `scaler_state_device` may be NULL; when its found_inf is set the launch writes nothing.  Reads `avg_state_device`. */
int zsv_avg_multi(const zsv_pair_tensor* table_device, int32_t count, int64_t total_chunks,
                  const zsv_avg_state* avg_state_device, float ema_weight, const zsv_scaler_state* scaler_state_device,
                  void* stream);
/* n_averaged += (scaler_state_device == NULL || !found_inf): once per optimizer step, after every launch of the step that
 * reads the counter and before zsv_scaler_update clears the flag.  One thread. */
int zsv_avg_advance(zsv_avg_state* avg_state_device, const zsv_scaler_state* scaler_state_device, void* stream);
/* Exchanges a[i] and b[i] in place over a table, one launch: the averaged values move INTO the live tensors (whose
 * addresses everything else is keyed on) and back, exactly. */
int zsv_swap_multi(const zsv_pair_tensor* table_device, int32_t count, int64_t total_chunks, void* stream);

/* ---- torch.optim.SGD (momentum, dampening, Nesterov, L2 weight decay, maximize) in one launch ---------------------------
 * ONE entry point over the zsv_adam_tensor table: `exp_avg` is the momentum buffer (may be NULL when momentum == 0, must
 * not be otherwise), `exp_avg_sq` is not read (may be NULL), so zsv_grad_check_multi, zsv_grad_norm_multi / _finalize and
 * zsv_grad_unscale_multi work on the same table.  What a step does not use is a NULL pointer:
 *   clip_device        NULL: no clipping
 *   state_device       NULL: no loss scaler.  Otherwise found_inf != 0 skips the whole launch (decay, buffers and the average
 *                      included) and g_mem is multiplied by (float)(1 / (double)scale) unless `grads_unscaled` != 0
 *   shadows_device,    both NULL: no weight average.  Otherwise as for zsv_adam_multi_avg (`count` pointers parallel to the
 *   avg_state_device   table; the state is read, zsv_avg_advance advances it)
 * Per element, in torch's order (torch/optim/sgd.py::_single_tensor_sgd), all fp32:
 *   g = g_mem * inv_scale; g = g * clip_coef      (two separate products)
 *   g = maximize ? -g : g
 *   g = fma(weight_decay, p, g)                   (weight_decay != 0)
 *   momentum != 0:  buf = first ? g : fma(1 - dampening, g, momentum * buf);  g = nesterov ? fma(momentum, buf, g) : buf
 *   p = fma(-lr, g, p)
 *   shadow <- the averaging rule with the new p
 * `first` is torch's "the momentum buffer does not exist yet" (the buffer is then written and not read).  It differs from a
 * zero-initialised buffer only when dampening != 0.  ONE rule decides it, on the device:
 *       first  iff  steps_done == first_step,   steps_done = state_device->steps_done, or 0 without a scaler
 * so without a scaler the host passes 0 on the first step and -1 (never) afterwards; with a scaler it passes the value
 * steps_done had when the optimizer had no buffers yet (-1: it has them) and the device decides: a first step the scaler skips
 * leaves steps_done where it was, and the next step is the first one again, as under GradScaler, which never calls
 * optimizer.step() on a skipped step.
 * p, g, buf and the shadows need only be 4-byte aligned, each on its own: a tensor whose pointers are all 16-byte aligned is
 * walked 16 bytes per lane, any other 4 bytes per lane, to the same bits (all or nothing per tensor: measured faster than
 * keeping only the aligned arrays of such a tensor on 16 bytes).  No atomics.  No element outside [0, n) of any
 * array is read or written.  ZSV_E_NULL: table NULL, or one of shadows / avg state NULL; ZSV_E_BAD_SHAPE: count <= 0,
 * total_chunks out of range, lr / momentum / weight_decay negative or not finite, nesterov without momentum > 0 and
 * dampening == 0, ema_weight > 1. */
int zsv_sgd_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, double lr, float momentum,
                  float dampening, int32_t nesterov, double weight_decay, int32_t maximize,
                  const zsv_clip_record* clip_device, const zsv_scaler_state* state_device, int32_t grads_unscaled,
                  int32_t first_step, float* const* shadows_device, const zsv_avg_state* avg_state_device, float ema_weight,
                  void* stream);

/* ---- LARS and LAMB: layer-wise trust ratios on the device (csrc/layerwise.hip; zsv_lars_multi: csrc/sgd.hip) ------------------
 * The SGD and Adam rules above with the update of every TENSOR scaled by a ratio of two 2-norms over that tensor.  With
 * g = g_mem * inv_scale * clip_coef exactly as in zsv_sgd_multi / zsv_adamw_multi_scaled:
 *   LARS   r = trust_coefficient * |p| / (|g| + weight_decay * |p| + eps)  if adapt and |p| > 0 and |g| > 0, else 1
 *          d = r * (g + weight_decay * p), then zsv_sgd_multi's momentum rule on d and p = fma(-lr, ., p); with r == 1 the
 *          element rule is zsv_sgd_multi's, operation for operation
 *   LAMB   m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2; t = `step`, or steps_done + 1 read on the device
 *          u = (m / (1 - beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps) + weight_decay * p
 *          r = |p| / |u|  if adapt and |p| > 0 and |u| > 0, else 1;  r = min(r, trust_clip) when trust_clip > 0
 *          p = fma(-(lr * r), u, p)
 * A step of one table is three launches: the partials (zsv_lars_norms, or zsv_lamb_moments, which updates m and v in place
 * and forms u without storing it), zsv_layerwise_finalize (one workgroup per tensor: the partials of its chunks summed in
 * double in a fixed order, one record written), and the apply (zsv_lars_multi / zsv_lamb_multi, which recomputes u from the
 * updated m, v and the old p).  No atomics: equal inputs give equal bits, at any alignment -- every array needs 4-byte
 * alignment only, each on its own, and moves 16 bytes per lane where its base allows (zsv_lars_multi: where all bases of the
 * tensor allow, as zsv_sgd_multi).  With a non-NULL scaler state whose found_inf is set every launch returns before it
 * touches m, v, the momentum buffer, p, the shadows or the records.
 *
 * The workspace is ONE buffer for all tables (parameter groups) of a step: `all_count` records, then two floats
 * {sum p^2, sum q^2} per chunk.  A launch names its table's place in it: `tensor_offset` = tensors of the tables before it,
 * `chunk_offset` = their chunks.  ZSV_E_NULL (table or workspace NULL), ZSV_E_BAD_SHAPE (count, total_chunks, an offset,
 * tensor_offset + count > all_count, a hyper-parameter out of range), ZSV_E_WORKSPACE (fewer bytes than the query gives for
 * chunk_offset + total_chunks chunks and all_count tensors): all before any launch. */
typedef struct zsv_layer_record {
    float p_norm;   /* 2-norm of the parameter tensor before the update */
    float q_norm;   /* LARS: 2-norm of its gradient, unscaled and clipped; LAMB: 2-norm of u */
    float ratio;    /* the trust ratio the apply launch multiplied the update by (1 where it does not adapt) */
} zsv_layer_record;
/* Bytes of the workspace: `count` records rounded up to 16 bytes, then 8 bytes per chunk.  0 for total_chunks or count <= 0. */
size_t zsv_layerwise_workspace_bytes(int64_t total_chunks, int32_t count);
int zsv_lars_norms(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, int64_t chunk_offset,
                   int32_t tensor_offset, int32_t all_count, void* workspace_device, size_t workspace_bytes,
                   const zsv_scaler_state* state_device, void* stream);
/* `step` (> 0) is read only when `state_device` is NULL; the exp_avg and exp_avg_sq of the table are written. */
int zsv_lamb_moments(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, int64_t chunk_offset,
                     int32_t tensor_offset, int32_t all_count, void* workspace_device, size_t workspace_bytes, float beta1,
                     float beta2, float eps, double weight_decay, const zsv_clip_record* clip_device,
                     const zsv_scaler_state* state_device, int32_t grads_unscaled, int32_t step, void* stream);
/* lamb == 0: the LARS ratio from trust_coefficient (> 0), weight_decay and eps, the gradient norm multiplied by
 * (float)(1 / (double)scale) (state_device non-NULL and grads_unscaled == 0) and by clip_coef (clip_device non-NULL);
 * lamb != 0: the LAMB ratio, clamped to trust_clip when that is > 0.  adapt == 0: the norms are recorded, every ratio is 1. */
int zsv_layerwise_finalize(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks, int64_t chunk_offset,
                           int32_t tensor_offset, int32_t all_count, void* workspace_device, size_t workspace_bytes,
                           int32_t lamb, int32_t adapt, double trust_coefficient, double weight_decay, double eps,
                           double trust_clip, const zsv_clip_record* clip_device, const zsv_scaler_state* state_device,
                           int32_t grads_unscaled, void* stream);
/* The apply launches.  `records_device`: the `count` records of THIS table (workspace + tensor_offset records), read only.
 * Clip record, scaler state, shadows and averaging state are NULL-able exactly as in zsv_sgd_multi; the other arguments of
 * zsv_lars_multi are zsv_sgd_multi's, and so is its kernel (one template, the ratio compiled in).  zsv_lamb_multi takes no
 * clip record: the gradient is not read again. */
int zsv_lars_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks,
                   const zsv_layer_record* records_device, double lr, float momentum, float dampening, int32_t nesterov,
                   double weight_decay, int32_t maximize, const zsv_clip_record* clip_device,
                   const zsv_scaler_state* state_device, int32_t grads_unscaled, int32_t first_step,
                   float* const* shadows_device, const zsv_avg_state* avg_state_device, float ema_weight, void* stream);
int zsv_lamb_multi(const zsv_adam_tensor* table_device, int32_t count, int64_t total_chunks,
                   const zsv_layer_record* records_device, double lr, float beta1, float beta2, float eps, double weight_decay,
                   const zsv_scaler_state* state_device, int32_t step, float* const* shadows_device,
                   const zsv_avg_state* avg_state_device, float ema_weight, void* stream);

/* ---- weight panels packed ahead of the call ---------------------------------------------------------------------------
 * Every forward / dgrad entry point above first re-lays its weights out (a "panel": the direct kernel's [block][tap][16][m]
 * image, the Winograd kernels' transformed weights, the stride-2 dgrad's tap-major image) in a small launch of its own: 76
 * launches and 1.1-1.3 ms per R(2+1)D-18 training step (profiles/r03_pack_launches_cost.txt), although the weights change once
 * per step.  A caller that knows when they change can keep the panels: query the panel size, ask for the job that fills it,
 * run ALL jobs of a step in one zsv_pack_multi launch, and call the *_panel forms, which skip the pack launch.
 * `direction` 0 = forward, 1 = input gradient; `extras` != 0 = the forward call carries a bias / ReLU / residual / statistics
 * (some geometries then take another kernel and so another panel).  *panel_bytes = 0: this geometry has no single panel
 * (3-channel stems, class-by-class strided gradients): use the ordinary entry points.  The job holds raw pointers (w, panel):
 * it stays valid while those allocations do.  Panels depend on the ZSV_* switches: re-query after zsv_reload_knobs(). */
typedef struct zsv_pack_job {
    int32_t kind;            /* 0 direct kernel, 1 Winograd F(2,3), 2 Winograd F(4,3), 3 stride-2 input gradient */
    int32_t reserved;
    int64_t total;           /* elements of the panel */
    int64_t first_block;     /* filled by the caller: running sum of ceil(total / 1024) over the preceding jobs of the table */
    const float* w;
    float* out;
    int64_t l[2];            /* kind-specific strides */
    int32_t i[20];           /* kind-specific integers */
} zsv_pack_job;
int zsv_conv3d_panel_query(const zsv_conv_desc* d, int32_t direction, int32_t extras, size_t* panel_bytes);
int zsv_conv3d_panel_job(const zsv_conv_desc* d, int32_t direction, int32_t extras, const float* w, void* panel,
                         size_t panel_bytes, zsv_pack_job* job);
/* one launch for `count` jobs (device array sorted by first_block; total_blocks = sum of ceil(total / 1024)) */
int zsv_pack_multi(const zsv_pack_job* jobs_device, int32_t count, int64_t total_blocks, void* stream);
/* the entry points above with the panel supplied (packed by zsv_pack_multi from this call's job): no pack launch */
int zsv_conv3d_fwd_full_panel(const zsv_conv_desc* d, const float* x, const float* w, const float* bias,
                              const float* residual, float* y, int fuse_relu, float* bn_partials, int32_t stat_tiles,
                              void* workspace, size_t workspace_bytes, void* stream, const void* panel, size_t panel_bytes);
int zsv_conv3d_fwd_pre_panel(const zsv_conv_desc* d, const float* x, const float* pre_coef, int32_t coef_pitch,
                             const float* w, float* y, float* bn_partials, int32_t stat_tiles, void* workspace,
                             size_t workspace_bytes, void* stream, const void* panel, size_t panel_bytes);
int zsv_conv3d_dgrad_add_panel(const zsv_conv_desc* d, const float* dy, const float* w, const float* add, float* dx,
                               void* workspace, size_t workspace_bytes, void* stream, const void* panel, size_t panel_bytes);
int zsv_conv3d_dgrad_add_strided_panel(const zsv_conv_desc* d, const float* dy, const float* w, const float* sub, int32_t st,
                                       int32_t sh, int32_t sw, float* dx, void* workspace, size_t workspace_bytes,
                                       void* stream, const void* panel, size_t panel_bytes);

#ifdef __cplusplus
}
#endif
#endif /* ZSV_HIP_H */
