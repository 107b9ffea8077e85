// nearest_class.hip -- cosine nearest classes in the 300-d embedding space (gfx950).
//
// Replaces, on the device, `cdist(embed, class_embed, 'cosine').argsort(1)[:, :k]` of the
// reference's compute_accuracy (main.py:316-325) and the per-step train accuracy
// (main.py:182-185).  Two launches:
//
//   cosine_dist_kernel : D[r][c] = 1 - <p_r, e_c> / (|p_r| |e_c|) in DOUBLE precision on the matrix
//                        core (v_mfma_f64_16x16x4_f64; the fp32 inputs convert exactly, so the
//                        distances agree with scipy's double cdist to ~1e-16 and the ranking is the
//                        same down to genuine ties);
//   row_topk_kernel    : per row the k smallest (distance, class index) pairs in lexicographic
//                        order -- what a stable argsort returns.
//
// The problem is tiny (rows x classes x 300: UCF101 / HMDB51 / ActivityNet tables of 101 / 51 / 200
// classes), so the kernels are written for exactness, not for a roofline.
//
// evaluate()'s scoring (main.py:264-266 over the whole class table, main.py:281-304 over the ten seeded
// half-class splits) builds on the first kernel:
//
//   split_score_kernel : rows scored / top-1 hits / top-5 hits for K class tables at once, from the distance
//                        matrices of `pred` and `true` against the FULL table.  A table is a row of positions
//                        pos[t][c] (the class's row in class_embedding[sel_classes], -1 = not in the table), and
//                        the order inside a table is (distance, position) -- the stable argsort of the gathered
//                        sub-table -- so no sub-table is ever gathered and no top-k list is written.
#include "zsv_common.h"
#include "zsv_hip.h"

namespace zsv {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// One wave = one 16-row block of `pred` against every 16-class block of `classes`.
// A fragment: lane holds A[m = lane & 15][k = lane >> 4]; B fragment: B[k = lane >> 4][n = lane & 15];
// C/D (f64 form): col = lane & 15, row = (lane >> 4) + 4 * reg   (cdna_hip_programming.md, MFMA maps).
__global__ __launch_bounds__(256) void cosine_dist_kernel(const float* __restrict__ pred, const float* __restrict__ classes,
                                                          int rows, int dim, int n_classes, int cpad,
                                                          double* __restrict__ dist) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rb = blockIdx.x * 4 + wave;                      // 16-row block of this wave
    if (rb * 16 >= rows) return;
    const int m = lane & 15, kq = lane >> 4;
    const int row_a = min(rb * 16 + m, rows - 1);              // clamped: the extra rows are never stored
    const float* pa = pred + (size_t)row_a * dim;
    const int ksteps = (dim + 3) >> 2;

    // |p_r|^2 for the row this lane feeds (partial over k = kq mod 4, then over the 4 lane groups)
    double na = 0.0;
    for (int s = 0; s < ksteps; ++s) {
        const int k = 4 * s + kq;
        const double a = k < dim ? (double)pa[k] : 0.0;
        na += a * a;
    }
    na += __shfl_xor(na, 16, 64);
    na += __shfl_xor(na, 32, 64);                              // every lane: |row (lane & 15)|^2
    double nrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) nrow[i] = sqrt(__shfl(na, kq + 4 * i, 64));

    for (int cb = 0; cb * 16 < n_classes; ++cb) {
        const int cls = min(cb * 16 + m, n_classes - 1);
        const float* pb = classes + (size_t)cls * dim;
        f64x4 acc = {0.0, 0.0, 0.0, 0.0};
        double nb = 0.0;
        for (int s = 0; s < ksteps; ++s) {
            const int k = 4 * s + kq;
            const double a = k < dim ? (double)pa[k] : 0.0;
            const double b = k < dim ? (double)pb[k] : 0.0;
            nb += b * b;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
        nb += __shfl_xor(nb, 16, 64);
        nb += __shfl_xor(nb, 32, 64);                          // |class (lane & 15) of this block|^2
        const double ncol = sqrt(nb);
        const int c = cb * 16 + m;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = rb * 16 + kq + 4 * i;
            if (r < rows && c < n_classes) {
                double cosine = acc[i] / (nrow[i] * ncol);
                if (fabs(cosine) > 1.0) cosine = copysign(1.0, cosine);      // scipy clips rounding error the same way
                dist[(size_t)r * cpad + c] = 1.0 - cosine;
            }
        }
    }
}

// One wave per row: k rounds of "smallest (d, c) greater than the last one taken".
__global__ __launch_bounds__(256) void row_topk_kernel(const double* __restrict__ dist, int rows, int n_classes, int cpad,
                                                       int k, int* __restrict__ out_index, double* __restrict__ out_dist) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const double* d = dist + (size_t)r * cpad;
    const double inf = __builtin_huge_val();
    double last_d = -inf;
    int last_c = -1;
    for (int j = 0; j < k; ++j) {
        double best_d = inf;
        int best_c = 0x7fffffff;
        for (int c = lane; c < n_classes; c += 64) {
            double v = d[c];
            if (v != v) v = inf;                                // NaN (zero-norm row) ranks last
            const bool after = v > last_d || (v == last_d && c > last_c);
            const bool better = v < best_d || (v == best_d && c < best_c);
            if (after && better) { best_d = v; best_c = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double od = __shfl_xor(best_d, o, 64);
            const int oc = __shfl_xor(best_c, o, 64);
            if (od < best_d || (od == best_d && oc < best_c)) { best_d = od; best_c = oc; }
        }
        last_d = best_d;
        last_c = best_c;
        if (lane == 0) {
            const bool found = best_c != 0x7fffffff;
            out_index[(size_t)r * k + j] = found ? best_c : -1;
            if (out_dist) out_dist[(size_t)r * k + j] = found ? d[best_c] : inf;
        }
    }
}

// One wave per row (grid-stride), lanes across classes, a loop over the tables.  Per table t:
//   y    = the class with the smallest (dist_true[c], pos[t][c]) among pos[t][c] >= 0       (argmin, first occurrence);
//   rank = the number of classes of the table whose (dist_pred[c], pos[t][c]) is smaller than y's;
//   top-1 hit: rank == 0, top-5 hit: rank < 5   (= membership in the first five of the stable argsort).
// Table 0 scores every row; table t >= 1 the rows whose label is in it.  Partial counts live in LDS: a workgroup
// issues at most one atomicAdd per counter.  class_counts (table 0 only, may be NULL): per true class y.
__global__ __launch_bounds__(256) void split_score_kernel(const double* __restrict__ dist_pred, const double* __restrict__ dist_true,
                                                          const int64_t* __restrict__ labels, const int* __restrict__ pos,
                                                          int rows, int n_classes, int cpad, int n_tables,
                                                          int* __restrict__ counts, int* __restrict__ class_counts) {
    extern __shared__ int part[];                              // (n_tables, 3)
    for (int i = threadIdx.x; i < 3 * n_tables; i += 256) part[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const double inf = __builtin_huge_val();
    for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4) {      // wave-uniform
        const double* dp = dist_pred + (size_t)r * cpad;
        const double* dt = dist_true + (size_t)r * cpad;
        const int64_t label = labels ? labels[r] : -1;
        for (int t = 0; t < n_tables; ++t) {
            const int* pt = pos + (size_t)t * n_classes;
            if (t > 0 && !(label >= 0 && label < n_classes && pt[label] >= 0)) continue;
            // y: argmin of the true row over the table
            double best_d = inf;
            int best_p = 0x7fffffff, best_c = -1;
            for (int c = lane; c < n_classes; c += 64) {
                const int p = pt[c];
                if (p < 0) continue;
                double v = dt[c];
                if (v != v) v = inf;                           // NaN (zero-norm row) ranks last
                if (v < best_d || (v == best_d && p < best_p)) { best_d = v; best_p = p; best_c = c; }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double od = __shfl_xor(best_d, o, 64);
                const int op = __shfl_xor(best_p, o, 64);
                const int oc = __shfl_xor(best_c, o, 64);
                if (od < best_d || (od == best_d && op < best_p)) { best_d = od; best_p = op; best_c = oc; }
            }
            if (best_c < 0) continue;                          // a table without classes scores nothing
            // rank of y in the pred row
            double yd = dp[best_c];
            if (yd != yd) yd = inf;
            int below = 0;
            for (int c = lane; c < n_classes; c += 64) {
                const int p = pt[c];
                if (p < 0) continue;
                double v = dp[c];
                if (v != v) v = inf;
                below += (v < yd || (v == yd && p < best_p)) ? 1 : 0;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) below += __shfl_xor(below, o, 64);
            if (lane == 0) {
                atomicAdd(&part[3 * t + 0], 1);
                if (below == 0) atomicAdd(&part[3 * t + 1], 1);
                if (below < 5) atomicAdd(&part[3 * t + 2], 1);
                if (t == 0 && class_counts) {
                    atomicAdd(&class_counts[3 * best_c + 0], 1);
                    if (below == 0) atomicAdd(&class_counts[3 * best_c + 1], 1);
                    if (below < 5) atomicAdd(&class_counts[3 * best_c + 2], 1);
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * n_tables; i += 256)
        if (part[i]) atomicAdd(&counts[i], part[i]);
}

}  // namespace zsv

static inline int32_t class_pitch(int32_t n_classes) { return (n_classes + 15) & ~15; }

extern "C" size_t zsv_cosine_topk_workspace_bytes(int32_t rows, int32_t n_classes) {
    if (rows <= 0 || n_classes <= 0) return 0;
    return (size_t)rows * (size_t)class_pitch(n_classes) * sizeof(double);
}

extern "C" int zsv_cosine_topk(const float* embed, const float* class_embed, int32_t rows, int32_t dim, int32_t n_classes,
                               int32_t k, int32_t* out_index, double* out_dist, void* workspace, size_t workspace_bytes,
                               void* stream_) {
    if (!embed || !class_embed || !out_index || !workspace) return ZSV_E_NULL;
    if (rows <= 0 || dim <= 0 || n_classes <= 0 || k <= 0 || k > n_classes) return ZSV_E_BAD_SHAPE;
    if ((double)rows * dim >= 2147483647.0 || (double)n_classes * dim >= 2147483647.0) return ZSV_E_TOO_LARGE;
    if (workspace_bytes < zsv_cosine_topk_workspace_bytes(rows, n_classes)) return ZSV_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const int cpad = class_pitch(n_classes);
    const int row_blocks = (rows + 15) / 16;
    hipLaunchKernelGGL(zsv::cosine_dist_kernel, dim3((row_blocks + 3) / 4), dim3(256), 0, stream, embed, class_embed, rows, dim,
                       n_classes, cpad, (double*)workspace);
    int st = zsv::launch_status();
    if (st) return st;
    hipLaunchKernelGGL(zsv::row_topk_kernel, dim3((rows + 3) / 4), dim3(256), 0, stream, (const double*)workspace, rows,
                       n_classes, cpad, k, out_index, out_dist);
    return zsv::launch_status();
}

// ---- evaluate()'s scoring: the whole class table and the seeded half-class splits in one pass -------------------
static const int32_t kMaxScoreTables = 2048;                   // (n_tables, 3) int32 partial counts in LDS: 24 KiB at most
static const int kMaxScoreBlocks = 1024;

extern "C" size_t zsv_split_accuracy_workspace_bytes(int32_t rows, int32_t n_classes) {
    return 2 * zsv_cosine_topk_workspace_bytes(rows, n_classes);
}

extern "C" int zsv_split_accuracy(const float* pred, const float* true_embed, const int64_t* labels, const float* class_embed,
                                  int32_t rows, int32_t dim, int32_t n_classes, const int32_t* split_pos, int32_t n_tables,
                                  int32_t* counts, int32_t* class_counts, void* workspace, size_t workspace_bytes, void* stream_) {
    if (!pred || !true_embed || !class_embed || !split_pos || !counts || !workspace) return ZSV_E_NULL;
    if (!labels && n_tables > 1) return ZSV_E_NULL;            // table 0 alone does not consult the labels
    if (rows <= 0 || dim <= 0 || n_classes <= 0 || n_tables <= 0) return ZSV_E_BAD_SHAPE;
    if ((double)rows * dim >= 2147483647.0 || (double)n_classes * dim >= 2147483647.0) return ZSV_E_TOO_LARGE;
    if (n_tables > kMaxScoreTables || (double)n_tables * n_classes >= 2147483647.0) return ZSV_E_TOO_LARGE;
    if (workspace_bytes < zsv_split_accuracy_workspace_bytes(rows, n_classes)) return ZSV_E_WORKSPACE;
    hipStream_t stream = (hipStream_t)stream_;
    const int cpad = class_pitch(n_classes);
    double* dist_pred = (double*)workspace;
    double* dist_true = dist_pred + (size_t)rows * cpad;
    if (hipMemsetAsync(counts, 0, (size_t)n_tables * 3 * sizeof(int32_t), stream) != hipSuccess) return ZSV_E_LAUNCH;
    if (class_counts && hipMemsetAsync(class_counts, 0, (size_t)n_classes * 3 * sizeof(int32_t), stream) != hipSuccess)
        return ZSV_E_LAUNCH;
    const int row_blocks = (rows + 15) / 16;
    hipLaunchKernelGGL(zsv::cosine_dist_kernel, dim3((row_blocks + 3) / 4), dim3(256), 0, stream, pred, class_embed, rows, dim,
                       n_classes, cpad, dist_pred);
    int st = zsv::launch_status();
    if (st) return st;
    hipLaunchKernelGGL(zsv::cosine_dist_kernel, dim3((row_blocks + 3) / 4), dim3(256), 0, stream, true_embed, class_embed, rows, dim,
                       n_classes, cpad, dist_true);
    st = zsv::launch_status();
    if (st) return st;
    const int blocks = (rows + 3) / 4 < kMaxScoreBlocks ? (rows + 3) / 4 : kMaxScoreBlocks;
    hipLaunchKernelGGL(zsv::split_score_kernel, dim3(blocks), dim3(256), (size_t)n_tables * 3 * sizeof(int), stream,
                       (const double*)dist_pred, (const double*)dist_true, labels, split_pos, rows, n_classes, cpad, n_tables, counts,
                       class_counts);
    return zsv::launch_status();
}
