// torch_binding.cpp -- the thin torch-extension layer BASELINE.json's north_star names ("bound through a thin torch
// cpp_extension C-ABI layer"): `torch.ops.zsv.*` operators over the C ABI of libzsv_hip.so (include/zsv_hip.h).
//
// Host C++ only (built with g++ against the torch headers; no device code, nothing generated): every operator builds the POD
// descriptor from the tensor sizes, takes the stream torch is currently recording on, allocates the workspace from torch's caching
// allocator and calls the same `zsv_*` entry point the ctypes glue (`_lib.py` / `ops.py`) calls -- after checking every operand
// (`want`, `describe`, `fit`) and under a device guard on the operands' device.  The differentiable forms
// (`zsv::conv3d`, `zsv::depthwise_conv3d`, `zsv::batch_norm_relu`, `zsv::batch_norm_relu_eval`, `zsv::relu`, `zsv::linear`) register an Autograd kernel,
// so C++ / TorchScript callers get the reference's
// `nn.Conv3d` (resnet.py:23-30,40-52; network.py:102-117) and `nn.BatchNorm3d (+ ReLU)` (resnet.py:46-49,94-98) semantics
// without Python.  The training harness of this repo keeps the ctypes path (panel cache, side-stream weight gradients, fused
// block tails live in ops.py); tests/test_torch_binding_gpu.py checks both bindings against each other bit for bit.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/autograd.h>
#include <torch/library.h>

#include <cstdint>
#include <vector>

#include "zsv_hip.h"

namespace {

void ok(int status, const char* what) { TORCH_CHECK(status == 0, what, ": ", zsv_status_string(status)); }

void* stream_of(const at::Tensor& t) {
    return static_cast<void*>(c10::hip::getCurrentHIPStream(t.device().index()).stream());
}

// One tensor operand, completely, in this order: device (a GPU, and the one the operator runs on: `dev`, its first operand's),
// dtype, rank, contiguity, extents (`sizes`; -1: any).  Every operand of every operator goes through here before anything is
// allocated or launched: the kernels take raw pointers and trust the descriptor.
void want(const at::Tensor& t, const char* name, c10::Device dev, at::IntArrayRef sizes) {
    TORCH_CHECK(t.is_cuda(), name, " must live on the GPU");       // (ROCm devices are `cuda` devices to torch)
    TORCH_CHECK(t.device() == dev, name, " is on ", t.device(), ", the operator's first operand on ", dev, ": one device per call");
    TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32, not ", t.scalar_type());
    TORCH_CHECK(t.dim() == (int64_t)sizes.size(), name, " must have ", sizes.size(), " dimensions, not ", t.dim());
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous (NCDHW)");
    for (size_t i = 0; i < sizes.size(); ++i)
        TORCH_CHECK(sizes[i] < 0 || t.size(i) == sizes[i], name, " has shape ", t.sizes(), ", expected ", sizes, " (-1: any)");
}

const int64_t ANY5[5] = {-1, -1, -1, -1, -1};

// an extent on its way into an `int32_t` field of the C ABI
int32_t fit(int64_t v, const char* name, int64_t index = -1) {
    if (index < 0) {
        TORCH_CHECK(v >= 0 && v <= INT32_MAX, name, " = ", v, " does not fit the C ABI's int32 field");
    } else {
        TORCH_CHECK(v >= 0 && v <= INT32_MAX, name, "[", index, "] = ", v, " does not fit the C ABI's int32 field");
    }
    return (int32_t)v;
}

// T * H * W of an (N, C, T, H, W) shape whose entries already fit int32: the kernels index one channel's voxels with an int32
int32_t voxels(int64_t t, int64_t h, int64_t w, const char* name) {
    const int64_t th = t * h;
    TORCH_CHECK(th <= INT32_MAX && th * w <= INT32_MAX, name, ": T*H*W = ", t, "*", h, "*", w, " does not fit the C ABI's int32 field");
    return (int32_t)(th * w);
}

at::Tensor scratch(size_t bytes, const at::Tensor& like) {
    return at::empty({static_cast<int64_t>(bytes ? bytes : 1)}, like.options().dtype(at::kByte));
}

// `xname` / `wname`: what the caller calls the two shapes (an operand, or the `x_sizes` / `w_sizes` list), for the refusals
zsv_conv_desc describe(at::IntArrayRef x, const char* xname, at::IntArrayRef w, const char* wname, at::IntArrayRef stride,
                       at::IntArrayRef padding) {
    TORCH_CHECK(x.size() == 5 && w.size() == 5 && stride.size() == 3 && padding.size() == 3,
                "conv3d: ", xname, " and ", wname, " are 5-d, stride and padding have three entries");
    for (int i = 0; i < 3; ++i) {
        TORCH_CHECK(stride[i] >= 1, "conv3d: stride[", i, "] = ", stride[i], " must be >= 1");
        TORCH_CHECK(padding[i] >= 0, "conv3d: padding[", i, "] = ", padding[i], " must be >= 0");
    }
    TORCH_CHECK(x[1] == w[1], "conv3d: x has ", x[1], " channels, w expects ", w[1]);
    zsv_conv_desc d;
    d.N = fit(x[0], xname, 0); d.Cin = fit(x[1], xname, 1); d.Ti = fit(x[2], xname, 2); d.Hi = fit(x[3], xname, 3); d.Wi = fit(x[4], xname, 4);
    d.Cout = fit(w[0], wname, 0); d.kT = fit(w[2], wname, 2); d.kH = fit(w[3], wname, 3); d.kW = fit(w[4], wname, 4);
    d.sT = fit(stride[0], "stride", 0); d.sH = fit(stride[1], "stride", 1); d.sW = fit(stride[2], "stride", 2);
    d.pT = fit(padding[0], "padding", 0); d.pH = fit(padding[1], "padding", 1); d.pW = fit(padding[2], "padding", 2);
    const int64_t to = (x[2] + 2 * padding[0] - w[2]) / stride[0] + 1;          // (64-bit: 2 * padding can leave int32)
    const int64_t ho = (x[3] + 2 * padding[1] - w[3]) / stride[1] + 1;
    const int64_t wo = (x[4] + 2 * padding[2] - w[4]) / stride[2] + 1;
    TORCH_CHECK(x[2] + 2 * padding[0] >= w[2] && x[3] + 2 * padding[1] >= w[3] && x[4] + 2 * padding[2] >= w[4] && to > 0 && ho > 0 &&
                    wo > 0, "conv3d: empty output");
    d.To = fit(to, "output T"); d.Ho = fit(ho, "output H"); d.Wo = fit(wo, "output W");
    voxels(x[2], x[3], x[4], xname);
    voxels(to, ho, wo, "conv3d output");
    return d;
}

struct BnShape { int32_t N, C, S; };

BnShape bn_shape(const at::Tensor& x) {
    return {fit(x.size(0), "x", 0), fit(x.size(1), "x", 1),
            voxels(fit(x.size(2), "x", 2), fit(x.size(3), "x", 3), fit(x.size(4), "x", 4), "x")};
}

// ---- plain operators: one C-ABI call each -----------------------------------------------------------------------------------
at::Tensor conv3d_fwd(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, at::IntArrayRef stride,
                      at::IntArrayRef padding, bool relu) {
    const c10::Device dev = x.device();
    want(x, "x", dev, ANY5);
    want(w, "w", dev, ANY5);
    const zsv_conv_desc d = describe(x.sizes(), "x", w.sizes(), "w", stride, padding);
    const float* b = nullptr;
    if (bias.has_value() && bias->defined()) {
        want(*bias, "bias", dev, {d.Cout});
        b = bias->data_ptr<float>();
    }
    const c10::DeviceGuard guard(dev);               // allocation, workspace query and launch on the operands' device
    at::Tensor y = at::empty({d.N, d.Cout, d.To, d.Ho, d.Wo}, x.options());
    const size_t bytes = zsv_conv3d_fwd_workspace_bytes(&d);
    at::Tensor ws = scratch(bytes, x);
    ok(zsv_conv3d_fwd(&d, x.data_ptr<float>(), w.data_ptr<float>(), b, y.data_ptr<float>(), relu ? 1 : 0, ws.data_ptr(), bytes,
                      stream_of(x)),
       "zsv_conv3d_fwd");
    return y;
}

at::Tensor conv3d_dgrad(const at::Tensor& dy, const at::Tensor& w, at::IntArrayRef x_sizes, at::IntArrayRef stride,
                        at::IntArrayRef padding) {
    const c10::Device dev = dy.device();
    want(dy, "dy", dev, ANY5);
    want(w, "w", dev, ANY5);
    const zsv_conv_desc d = describe(x_sizes, "x_sizes", w.sizes(), "w", stride, padding);
    want(dy, "dy", dev, {d.N, d.Cout, d.To, d.Ho, d.Wo});
    const c10::DeviceGuard guard(dev);
    at::Tensor dx = at::empty(x_sizes, dy.options());
    const size_t bytes = zsv_conv3d_dgrad_workspace_bytes(&d);
    at::Tensor ws = scratch(bytes, dy);
    ok(zsv_conv3d_dgrad(&d, dy.data_ptr<float>(), w.data_ptr<float>(), dx.data_ptr<float>(), ws.data_ptr(), bytes, stream_of(dy)),
       "zsv_conv3d_dgrad");
    return dx;
}

at::Tensor conv3d_wgrad(const at::Tensor& x, const at::Tensor& dy, at::IntArrayRef w_sizes, at::IntArrayRef stride,
                        at::IntArrayRef padding) {
    const c10::Device dev = x.device();
    want(x, "x", dev, ANY5);
    want(dy, "dy", dev, ANY5);
    const zsv_conv_desc d = describe(x.sizes(), "x", w_sizes, "w_sizes", stride, padding);
    want(dy, "dy", dev, {d.N, d.Cout, d.To, d.Ho, d.Wo});
    const c10::DeviceGuard guard(dev);
    at::Tensor dw = at::empty(w_sizes, x.options());
    const size_t bytes = zsv_conv3d_wgrad_workspace_bytes(&d);
    at::Tensor ws = scratch(bytes, x);
    ok(zsv_conv3d_wgrad(&d, x.data_ptr<float>(), dy.data_ptr<float>(), dw.data_ptr<float>(), ws.data_ptr(), bytes, stream_of(x)),
       "zsv_conv3d_wgrad");
    return dw;
}

// ---- depthwise convolution (groups == channels): w is (C, 1, kT, kH, kW) ------------------------------------------------------
// the dense descriptor of a (C, C, kT, kH, kW) weight, which the zsv_dwconv3d_* entry points read as depthwise
zsv_conv_desc describe_depthwise(at::IntArrayRef x, const char* xname, at::IntArrayRef w, const char* wname, at::IntArrayRef stride,
                                 at::IntArrayRef padding) {
    TORCH_CHECK(x.size() == 5 && w.size() == 5, "depthwise_conv3d: ", xname, " and ", wname, " are 5-d");
    TORCH_CHECK(w[0] == x[1] && w[1] == 1, "depthwise_conv3d: ", wname, " is (C, 1, kT, kH, kW) with C = ", x[1], " channels of ", xname,
                ", got ", w);
    const int64_t dense[5] = {w[0], w[0], w[2], w[3], w[4]};
    const zsv_conv_desc d = describe(x, xname, dense, wname, stride, padding);
    TORCH_CHECK(zsv_dwconv3d_supported(&d) == 1, "depthwise_conv3d: kernel extents 1 or 3, strides 1 or 2, padding < kernel and tensors "
                "below 2^31 elements are supported");
    return d;
}

at::Tensor depthwise_conv3d_fwd(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, at::IntArrayRef stride,
                                at::IntArrayRef padding, bool relu) {
    const c10::Device dev = x.device();
    want(x, "x", dev, ANY5);
    want(w, "w", dev, ANY5);
    const zsv_conv_desc d = describe_depthwise(x.sizes(), "x", w.sizes(), "w", stride, padding);
    const float* b = nullptr;
    if (bias.has_value() && bias->defined()) {
        want(*bias, "bias", dev, {d.Cout});
        b = bias->data_ptr<float>();
    }
    const c10::DeviceGuard guard(dev);
    at::Tensor y = at::empty({d.N, d.Cout, d.To, d.Ho, d.Wo}, x.options());
    ok(zsv_dwconv3d_fwd(&d, x.data_ptr<float>(), w.data_ptr<float>(), b, y.data_ptr<float>(), relu ? 1 : 0, stream_of(x)),
       "zsv_dwconv3d_fwd");
    return y;
}

at::Tensor depthwise_conv3d_dgrad(const at::Tensor& dy, const at::Tensor& w, at::IntArrayRef x_sizes, at::IntArrayRef stride,
                                  at::IntArrayRef padding) {
    const c10::Device dev = dy.device();
    want(dy, "dy", dev, ANY5);
    want(w, "w", dev, ANY5);
    const zsv_conv_desc d = describe_depthwise(x_sizes, "x_sizes", w.sizes(), "w", stride, padding);
    want(dy, "dy", dev, {d.N, d.Cout, d.To, d.Ho, d.Wo});
    const c10::DeviceGuard guard(dev);
    at::Tensor dx = at::empty(x_sizes, dy.options());
    ok(zsv_dwconv3d_dgrad(&d, dy.data_ptr<float>(), w.data_ptr<float>(), dx.data_ptr<float>(), stream_of(dy)), "zsv_dwconv3d_dgrad");
    return dx;
}

at::Tensor depthwise_conv3d_wgrad(const at::Tensor& x, const at::Tensor& dy, at::IntArrayRef w_sizes, at::IntArrayRef stride,
                                  at::IntArrayRef padding) {
    const c10::Device dev = x.device();
    want(x, "x", dev, ANY5);
    want(dy, "dy", dev, ANY5);
    const zsv_conv_desc d = describe_depthwise(x.sizes(), "x", w_sizes, "w_sizes", stride, padding);
    want(dy, "dy", dev, {d.N, d.Cout, d.To, d.Ho, d.Wo});
    const c10::DeviceGuard guard(dev);
    at::Tensor dw = at::empty(w_sizes, x.options());
    const size_t bytes = zsv_dwconv3d_wgrad_workspace_bytes(&d);
    at::Tensor ws = scratch(bytes, x);
    ok(zsv_dwconv3d_wgrad(&d, x.data_ptr<float>(), dy.data_ptr<float>(), dw.data_ptr<float>(), ws.data_ptr(), bytes, stream_of(x)),
       "zsv_dwconv3d_wgrad");
    return dw;
}

// training-mode BatchNorm3d (+ ReLU): y, save_mean, save_invstd; running statistics updated in place like torch
std::tuple<at::Tensor, at::Tensor, at::Tensor> bn_train_fwd(const at::Tensor& x, const at::Tensor& gamma, const at::Tensor& beta,
                                                            at::Tensor running_mean, at::Tensor running_var, double momentum,
                                                            double eps, bool relu) {
    const c10::Device dev = x.device();
    want(x, "x", dev, ANY5);
    const auto [N, C, S] = bn_shape(x);
    want(gamma, "weight", dev, {C});
    want(beta, "bias", dev, {C});
    want(running_mean, "running_mean", dev, {C});
    want(running_var, "running_var", dev, {C});
    const c10::DeviceGuard guard(dev);
    at::Tensor y = at::empty_like(x), mean = at::empty({C}, x.options()), invstd = at::empty({C}, x.options());
    const size_t bytes = zsv_bn_workspace_bytes(N, C, S);
    at::Tensor ws = scratch(bytes, x);
    ok(zsv_bn_fwd_train(x.data_ptr<float>(), N, C, S, gamma.data_ptr<float>(), beta.data_ptr<float>(), nullptr, relu ? 1 : 0,
                        y.data_ptr<float>(), mean.data_ptr<float>(), invstd.data_ptr<float>(), running_mean.data_ptr<float>(),
                        running_var.data_ptr<float>(), (float)momentum, (float)eps, ws.data_ptr(), bytes, stream_of(x)),
       "zsv_bn_fwd_train");
    // the kernel wrote the two running statistics through raw pointers, below the ADInplaceOrView key: move their version
    // counters by hand, as an in-place torch operator would, so that saved-tensor checks and caches keyed on `_version`
    // (inference.engine_for) see the write
    running_mean.unsafeGetTensorImpl()->bump_version();
    running_var.unsafeGetTensorImpl()->bump_version();
    return {y, mean, invstd};
}

// backward of the op above: dx, dgamma, dbeta (ReLU mask from the saved output)
std::tuple<at::Tensor, at::Tensor, at::Tensor> bn_train_bwd(const at::Tensor& dy, const at::Tensor& x, const at::Tensor& y,
                                                            const at::Tensor& gamma, const at::Tensor& beta, const at::Tensor& mean,
                                                            const at::Tensor& invstd, bool relu) {
    const c10::Device dev = x.device();
    want(x, "x", dev, ANY5);
    const auto [N, C, S] = bn_shape(x);
    want(dy, "dy", dev, x.sizes());
    want(y, "y", dev, x.sizes());
    want(gamma, "weight", dev, {C});
    want(beta, "bias", dev, {C});
    want(mean, "save_mean", dev, {C});
    want(invstd, "save_invstd", dev, {C});
    const c10::DeviceGuard guard(dev);
    at::Tensor dx = at::empty_like(x), dgamma = at::empty({C}, x.options()), dbeta = at::empty({C}, x.options());
    const size_t bytes = zsv_bn_workspace_bytes(N, C, S);
    at::Tensor ws = scratch(bytes, x);
    ok(zsv_bn_bwd(dy.data_ptr<float>(), x.data_ptr<float>(), y.data_ptr<float>(), N, C, S, gamma.data_ptr<float>(),
                  beta.data_ptr<float>(), mean.data_ptr<float>(), invstd.data_ptr<float>(), relu ? 1 : 0, dx.data_ptr<float>(),
                  nullptr, dgamma.data_ptr<float>(), dbeta.data_ptr<float>(), ws.data_ptr(), bytes, stream_of(x)),
       "zsv_bn_bwd");
    return {dx, dgamma, dbeta};
}

// eval-mode (frozen statistics) BatchNorm3d (+ ReLU): y = relu?(x * a + b) from the running statistics, which are only read
at::Tensor bn_eval_fwd(const at::Tensor& x, const at::Tensor& gamma, const at::Tensor& beta, const at::Tensor& running_mean,
                       const at::Tensor& running_var, double eps, bool relu) {
    const c10::Device dev = x.device();
    want(x, "x", dev, ANY5);
    const auto [N, C, S] = bn_shape(x);
    want(gamma, "weight", dev, {C});
    want(beta, "bias", dev, {C});
    want(running_mean, "running_mean", dev, {C});
    want(running_var, "running_var", dev, {C});
    const c10::DeviceGuard guard(dev);
    at::Tensor y = at::empty_like(x);
    const size_t bytes = zsv_bn_workspace_bytes(N, C, S);
    at::Tensor ws = scratch(bytes, x);
    ok(zsv_bn_fwd_eval(x.data_ptr<float>(), N, C, S, gamma.data_ptr<float>(), beta.data_ptr<float>(), running_mean.data_ptr<float>(),
                       running_var.data_ptr<float>(), nullptr, relu ? 1 : 0, (float)eps, y.data_ptr<float>(), ws.data_ptr(), bytes,
                       stream_of(x)),
       "zsv_bn_fwd_eval");
    return y;
}

// backward of the op above in one pass: dx, dgamma, dbeta (ReLU mask recomputed from x with the forward's exact fma)
std::tuple<at::Tensor, at::Tensor, at::Tensor> bn_eval_bwd(const at::Tensor& dy, const at::Tensor& x, const at::Tensor& gamma,
                                                           const at::Tensor& beta, const at::Tensor& running_mean,
                                                           const at::Tensor& running_var, double eps, bool relu,
                                                           bool want_dgamma = true, bool want_dbeta = true) {
    const c10::Device dev = x.device();
    want(x, "x", dev, ANY5);
    const auto [N, C, S] = bn_shape(x);
    want(dy, "dy", dev, x.sizes());
    want(gamma, "weight", dev, {C});
    want(beta, "bias", dev, {C});
    want(running_mean, "running_mean", dev, {C});
    want(running_var, "running_var", dev, {C});
    const c10::DeviceGuard guard(dev);
    at::Tensor dx = at::empty_like(x);
    at::Tensor dgamma = want_dgamma ? at::empty({C}, x.options()) : at::Tensor();
    at::Tensor dbeta = want_dbeta ? at::empty({C}, x.options()) : at::Tensor();
    const size_t bytes = zsv_bn_workspace_bytes(N, C, S);
    at::Tensor ws = scratch(bytes, x);
    ok(zsv_bn_bwd_eval(dy.data_ptr<float>(), x.data_ptr<float>(), nullptr, N, C, S, gamma.data_ptr<float>(), beta.data_ptr<float>(),
                       running_mean.data_ptr<float>(), running_var.data_ptr<float>(), (float)eps, relu ? 2 : 0, dx.data_ptr<float>(),
                       nullptr, want_dgamma ? dgamma.data_ptr<float>() : nullptr, want_dbeta ? dbeta.data_ptr<float>() : nullptr,
                       ws.data_ptr(), bytes, stream_of(x)),
       "zsv_bn_bwd_eval");
    return {dx, dgamma, dbeta};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor> bn_eval_bwd_op(const at::Tensor& dy, const at::Tensor& x, const at::Tensor& gamma,
                                                              const at::Tensor& beta, const at::Tensor& running_mean,
                                                              const at::Tensor& running_var, double eps, bool relu) {
    return bn_eval_bwd(dy, x, gamma, beta, running_mean, running_var, eps, relu);
}

// nn.ReLU (resnet.py:49; network.py:147-166,614) and its backward (mask from the saved output, like ReLU(inplace=True))
at::Tensor relu_fwd(const at::Tensor& x) {
    want(x, "x", x.device(), x.sizes());                     // (any rank)
    const c10::DeviceGuard guard(x.device());
    at::Tensor y = at::empty_like(x);
    ok(zsv_relu_fwd(x.data_ptr<float>(), y.data_ptr<float>(), x.numel(), stream_of(x)), "zsv_relu_fwd");
    return y;
}

at::Tensor relu_bwd(const at::Tensor& dy, const at::Tensor& y) {
    want(dy, "dy", dy.device(), dy.sizes());                 // (any rank)
    want(y, "y", dy.device(), dy.sizes());
    const c10::DeviceGuard guard(dy.device());
    at::Tensor dx = at::empty_like(dy);
    ok(zsv_relu_bwd(dy.data_ptr<float>(), y.data_ptr<float>(), dx.data_ptr<float>(), dy.numel(), stream_of(dy)), "zsv_relu_bwd");
    return dx;
}

// nn.Linear (+ ReLU) of network.MLP (network.py:603-617): y = relu?(x w^T + b), x (rows, in), w (out, in)
at::Tensor linear_fwd(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, bool relu) {
    const c10::Device dev = x.device();
    want(x, "x", dev, {-1, -1});
    want(w, "w", dev, {-1, x.size(1)});
    const int32_t rows = fit(x.size(0), "x", 0), in = fit(x.size(1), "x", 1), out = fit(w.size(0), "w", 0);
    const float* b = nullptr;
    if (bias.has_value() && bias->defined()) {
        want(*bias, "bias", dev, {out});
        b = bias->data_ptr<float>();
    }
    const c10::DeviceGuard guard(dev);
    at::Tensor y = at::empty({rows, out}, x.options());
    const size_t bytes = zsv_linear_fwd_workspace_bytes(rows, in, out);
    at::Tensor ws = scratch(bytes, x);
    ok(zsv_linear_fwd(x.data_ptr<float>(), w.data_ptr<float>(), b, y.data_ptr<float>(), rows, in, out, relu ? 1 : 0, ws.data_ptr(), bytes,
                      stream_of(x)),
       "zsv_linear_fwd");
    return y;
}

at::Tensor linear_dgrad(const at::Tensor& dy, const at::Tensor& w) {
    const c10::Device dev = dy.device();
    want(dy, "dy", dev, {-1, -1});
    want(w, "w", dev, {dy.size(1), -1});
    const int32_t rows = fit(dy.size(0), "dy", 0), in = fit(w.size(1), "w", 1), out = fit(w.size(0), "w", 0);
    const c10::DeviceGuard guard(dev);
    at::Tensor dx = at::empty({rows, in}, dy.options());
    const size_t bytes = zsv_linear_dgrad_workspace_bytes(rows, in, out);
    at::Tensor ws = scratch(bytes, dy);
    ok(zsv_linear_dgrad(dy.data_ptr<float>(), w.data_ptr<float>(), dx.data_ptr<float>(), rows, in, out, ws.data_ptr(), bytes, stream_of(dy)),
       "zsv_linear_dgrad");
    return dx;
}

at::Tensor linear_wgrad(const at::Tensor& x, const at::Tensor& dy) {
    const c10::Device dev = x.device();
    want(x, "x", dev, {-1, -1});
    want(dy, "dy", dev, {x.size(0), -1});
    const int32_t rows = fit(x.size(0), "x", 0), in = fit(x.size(1), "x", 1), out = fit(dy.size(1), "dy", 1);
    const c10::DeviceGuard guard(dev);
    at::Tensor dw = at::empty({out, in}, x.options());
    const size_t bytes = zsv_linear_wgrad_workspace_bytes(rows, in, out);
    at::Tensor ws = scratch(bytes, x);
    ok(zsv_linear_wgrad(x.data_ptr<float>(), dy.data_ptr<float>(), dw.data_ptr<float>(), rows, in, out, ws.data_ptr(), bytes, stream_of(x)),
       "zsv_linear_wgrad");
    return dw;
}

std::string version() { return zsv_version(); }

// ---- differentiable forms ---------------------------------------------------------------------------------------------------
struct Conv3dFn : public torch::autograd::Function<Conv3dFn> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, const at::Tensor& x, const at::Tensor& w,
                              const c10::optional<at::Tensor>& bias, std::vector<int64_t> stride, std::vector<int64_t> padding) {
        at::AutoDispatchBelowADInplaceOrView guard;
        ctx->save_for_backward({x, w});
        ctx->saved_data["stride"] = stride;
        ctx->saved_data["padding"] = padding;
        ctx->saved_data["has_bias"] = bias.has_value() && bias->defined();
        return conv3d_fwd(x, w, bias, stride, padding, false);
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grads) {
        const auto saved = ctx->get_saved_variables();
        const at::Tensor &x = saved[0], &w = saved[1];
        const auto stride = ctx->saved_data["stride"].toIntVector(), padding = ctx->saved_data["padding"].toIntVector();
        const at::Tensor dy = grads[0].contiguous();
        at::Tensor dx, dw, db;
        if (ctx->needs_input_grad(0)) dx = conv3d_dgrad(dy, w, x.sizes(), stride, padding);
        if (ctx->needs_input_grad(1)) dw = conv3d_wgrad(x, dy, w.sizes(), stride, padding);
        if (ctx->saved_data["has_bias"].toBool() && ctx->needs_input_grad(2)) db = dy.sum({0, 2, 3, 4});
        return {dx, dw, db, at::Tensor(), at::Tensor()};
    }
};

at::Tensor conv3d_autograd(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, at::IntArrayRef stride,
                           at::IntArrayRef padding) {
    return Conv3dFn::apply(x, w, bias, stride.vec(), padding.vec());
}

struct DepthwiseConv3dFn : public torch::autograd::Function<DepthwiseConv3dFn> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, const at::Tensor& x, const at::Tensor& w,
                              const c10::optional<at::Tensor>& bias, std::vector<int64_t> stride, std::vector<int64_t> padding) {
        at::AutoDispatchBelowADInplaceOrView guard;
        ctx->save_for_backward({x, w});
        ctx->saved_data["stride"] = stride;
        ctx->saved_data["padding"] = padding;
        ctx->saved_data["has_bias"] = bias.has_value() && bias->defined();
        return depthwise_conv3d_fwd(x, w, bias, stride, padding, false);
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grads) {
        const auto saved = ctx->get_saved_variables();
        const at::Tensor &x = saved[0], &w = saved[1];
        const auto stride = ctx->saved_data["stride"].toIntVector(), padding = ctx->saved_data["padding"].toIntVector();
        const at::Tensor dy = grads[0].contiguous();
        at::Tensor dx, dw, db;
        if (ctx->needs_input_grad(0)) dx = depthwise_conv3d_dgrad(dy, w, x.sizes(), stride, padding);
        if (ctx->needs_input_grad(1)) dw = depthwise_conv3d_wgrad(x, dy, w.sizes(), stride, padding);
        if (ctx->saved_data["has_bias"].toBool() && ctx->needs_input_grad(2)) db = dy.sum({0, 2, 3, 4});
        return {dx, dw, db, at::Tensor(), at::Tensor()};
    }
};

at::Tensor depthwise_conv3d_autograd(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias,
                                     at::IntArrayRef stride, at::IntArrayRef padding) {
    return DepthwiseConv3dFn::apply(x, w, bias, stride.vec(), padding.vec());
}
at::Tensor depthwise_conv3d_plain(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, at::IntArrayRef stride,
                                  at::IntArrayRef padding) {
    return depthwise_conv3d_fwd(x, w, bias, stride, padding, false);
}

struct BatchNormReluFn : public torch::autograd::Function<BatchNormReluFn> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, const at::Tensor& x, const at::Tensor& gamma, const at::Tensor& beta,
                              at::Tensor running_mean, at::Tensor running_var, double momentum, double eps, bool relu) {
        at::AutoDispatchBelowADInplaceOrView guard;
        auto [y, mean, invstd] = bn_train_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, relu);
        ctx->save_for_backward({x, y, gamma, beta, mean, invstd});
        ctx->saved_data["relu"] = relu;
        return y;
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grads) {
        const auto s = ctx->get_saved_variables();
        auto [dx, dgamma, dbeta] = bn_train_bwd(grads[0].contiguous(), s[0], s[1], s[2], s[3], s[4], s[5], ctx->saved_data["relu"].toBool());
        return {dx, dgamma, dbeta, at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
    }
};

at::Tensor batch_norm_relu_autograd(const at::Tensor& x, const at::Tensor& gamma, const at::Tensor& beta, at::Tensor running_mean,
                                    at::Tensor running_var, double momentum, double eps, bool relu) {
    return BatchNormReluFn::apply(x, gamma, beta, running_mean, running_var, momentum, eps, relu);
}

struct BatchNormReluEvalFn : public torch::autograd::Function<BatchNormReluEvalFn> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, const at::Tensor& x, const at::Tensor& gamma, const at::Tensor& beta,
                              const at::Tensor& running_mean, const at::Tensor& running_var, double eps, bool relu) {
        at::AutoDispatchBelowADInplaceOrView guard;
        at::Tensor y = bn_eval_fwd(x, gamma, beta, running_mean, running_var, eps, relu);
        ctx->save_for_backward({x, gamma, beta, running_mean.clone(), running_var.clone()});       // (statistics as the forward saw them)
        ctx->saved_data["eps"] = eps;
        ctx->saved_data["relu"] = relu;
        return y;
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grads) {
        const auto s = ctx->get_saved_variables();
        // (a frozen affine -- gamma / beta without gradients -- skips the reduction)
        auto [dx, dgamma, dbeta] = bn_eval_bwd(grads[0].contiguous(), s[0], s[1], s[2], s[3], s[4], ctx->saved_data["eps"].toDouble(),
                                               ctx->saved_data["relu"].toBool(), ctx->needs_input_grad(1), ctx->needs_input_grad(2));
        return {dx, dgamma, dbeta, at::Tensor(), at::Tensor(), at::Tensor(), at::Tensor()};
    }
};

at::Tensor batch_norm_relu_eval_autograd(const at::Tensor& x, const at::Tensor& gamma, const at::Tensor& beta,
                                         const at::Tensor& running_mean, const at::Tensor& running_var, double eps, bool relu) {
    return BatchNormReluEvalFn::apply(x, gamma, beta, running_mean, running_var, eps, relu);
}

struct ReluFn : public torch::autograd::Function<ReluFn> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, const at::Tensor& x) {
        at::AutoDispatchBelowADInplaceOrView guard;
        at::Tensor y = relu_fwd(x.contiguous());
        ctx->save_for_backward({y});
        return y;
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grads) {
        return {relu_bwd(grads[0].contiguous(), ctx->get_saved_variables()[0])};
    }
};
at::Tensor relu_autograd(const at::Tensor& x) { return ReluFn::apply(x); }

struct LinearFn : public torch::autograd::Function<LinearFn> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, const at::Tensor& x, const at::Tensor& w,
                              const c10::optional<at::Tensor>& bias) {
        at::AutoDispatchBelowADInplaceOrView guard;
        ctx->save_for_backward({x, w});
        ctx->saved_data["has_bias"] = bias.has_value() && bias->defined();
        return linear_fwd(x, w, bias, false);
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grads) {
        const auto saved = ctx->get_saved_variables();
        const at::Tensor dy = grads[0].contiguous();
        at::Tensor dx, dw, db;
        if (ctx->needs_input_grad(0)) dx = linear_dgrad(dy, saved[1]);
        if (ctx->needs_input_grad(1)) dw = linear_wgrad(saved[0], dy);
        if (ctx->saved_data["has_bias"].toBool() && ctx->needs_input_grad(2)) db = dy.sum(0);
        return {dx, dw, db};
    }
};
at::Tensor linear_autograd(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias) {
    return LinearFn::apply(x, w, bias);
}
at::Tensor linear_plain(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias) {
    return linear_fwd(x, w, bias, false);
}

// without autograd in the key set (inference mode): the forward alone
at::Tensor conv3d_plain(const at::Tensor& x, const at::Tensor& w, const c10::optional<at::Tensor>& bias, at::IntArrayRef stride,
                        at::IntArrayRef padding) {
    return conv3d_fwd(x, w, bias, stride, padding, false);
}

at::Tensor batch_norm_relu_plain(const at::Tensor& x, const at::Tensor& gamma, const at::Tensor& beta, at::Tensor running_mean,
                                 at::Tensor running_var, double momentum, double eps, bool relu) {
    return std::get<0>(bn_train_fwd(x, gamma, beta, running_mean, running_var, momentum, eps, relu));
}

}  // namespace

TORCH_LIBRARY(zsv, m) {
    m.def("version() -> str", version);
    m.def("conv3d_fwd(Tensor x, Tensor w, Tensor? bias, int[3] stride, int[3] padding, bool relu=False) -> Tensor");
    m.def("conv3d_dgrad(Tensor dy, Tensor w, int[] x_sizes, int[3] stride, int[3] padding) -> Tensor");
    m.def("conv3d_wgrad(Tensor x, Tensor dy, int[] w_sizes, int[3] stride, int[3] padding) -> Tensor");
    m.def("depthwise_conv3d_fwd(Tensor x, Tensor w, Tensor? bias, int[3] stride, int[3] padding, bool relu=False) -> Tensor");
    m.def("depthwise_conv3d_dgrad(Tensor dy, Tensor w, int[] x_sizes, int[3] stride, int[3] padding) -> Tensor");
    m.def("depthwise_conv3d_wgrad(Tensor x, Tensor dy, int[] w_sizes, int[3] stride, int[3] padding) -> Tensor");
    m.def("depthwise_conv3d(Tensor x, Tensor w, Tensor? bias, int[3] stride, int[3] padding) -> Tensor");
    m.def("bn_train_fwd(Tensor x, Tensor weight, Tensor bias, Tensor(a!) running_mean, Tensor(b!) running_var, float momentum, "
          "float eps, bool relu=False) -> (Tensor, Tensor, Tensor)");
    m.def("bn_train_bwd(Tensor dy, Tensor x, Tensor y, Tensor weight, Tensor bias, Tensor save_mean, Tensor save_invstd, "
          "bool relu=False) -> (Tensor, Tensor, Tensor)");
    m.def("bn_eval_fwd(Tensor x, Tensor weight, Tensor bias, Tensor running_mean, Tensor running_var, float eps, bool relu=False) "
          "-> Tensor");
    m.def("bn_eval_bwd(Tensor dy, Tensor x, Tensor weight, Tensor bias, Tensor running_mean, Tensor running_var, float eps, "
          "bool relu=False) -> (Tensor, Tensor, Tensor)");
    m.def("relu_fwd(Tensor x) -> Tensor");
    m.def("relu_bwd(Tensor dy, Tensor y) -> Tensor");
    m.def("linear_fwd(Tensor x, Tensor w, Tensor? bias, bool relu=False) -> Tensor");
    m.def("linear_dgrad(Tensor dy, Tensor w) -> Tensor");
    m.def("linear_wgrad(Tensor x, Tensor dy) -> Tensor");
    m.def("relu(Tensor x) -> Tensor");
    m.def("linear(Tensor x, Tensor w, Tensor? bias) -> Tensor");
    m.def("conv3d(Tensor x, Tensor w, Tensor? bias, int[3] stride, int[3] padding) -> Tensor");
    m.def("batch_norm_relu(Tensor x, Tensor weight, Tensor bias, Tensor(a!) running_mean, Tensor(b!) running_var, float momentum, "
          "float eps, bool relu=False) -> Tensor");
    m.def("batch_norm_relu_eval(Tensor x, Tensor weight, Tensor bias, Tensor running_mean, Tensor running_var, float eps, "
          "bool relu=False) -> Tensor");
}

TORCH_LIBRARY_IMPL(zsv, CUDA, m) {      // torch's name of the HIP backend on ROCm builds
    m.impl("conv3d_fwd", conv3d_fwd);
    m.impl("conv3d_dgrad", conv3d_dgrad);
    m.impl("conv3d_wgrad", conv3d_wgrad);
    m.impl("depthwise_conv3d_fwd", depthwise_conv3d_fwd);
    m.impl("depthwise_conv3d_dgrad", depthwise_conv3d_dgrad);
    m.impl("depthwise_conv3d_wgrad", depthwise_conv3d_wgrad);
    m.impl("depthwise_conv3d", depthwise_conv3d_plain);
    m.impl("bn_train_fwd", bn_train_fwd);
    m.impl("bn_train_bwd", bn_train_bwd);
    m.impl("conv3d", conv3d_plain);
    m.impl("batch_norm_relu", batch_norm_relu_plain);
    m.impl("bn_eval_fwd", bn_eval_fwd);
    m.impl("bn_eval_bwd", bn_eval_bwd_op);
    m.impl("batch_norm_relu_eval", bn_eval_fwd);
    m.impl("relu_fwd", relu_fwd);
    m.impl("relu_bwd", relu_bwd);
    m.impl("linear_fwd", linear_fwd);
    m.impl("linear_dgrad", linear_dgrad);
    m.impl("linear_wgrad", linear_wgrad);
    m.impl("relu", relu_fwd);
    m.impl("linear", linear_plain);
}

TORCH_LIBRARY_IMPL(zsv, Autograd, m) {
    m.impl("conv3d", conv3d_autograd);
    m.impl("depthwise_conv3d", depthwise_conv3d_autograd);
    m.impl("batch_norm_relu", batch_norm_relu_autograd);
    m.impl("batch_norm_relu_eval", batch_norm_relu_eval_autograd);
    m.impl("relu", relu_autograd);
    m.impl("linear", linear_autograd);
}
