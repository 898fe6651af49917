// PyTorch-ROCm custom-op registration of the hot path: torch.ops.osi.* (TORCH_LIBRARY), the form BASELINE.json's north_star names
// ("surfaced through PyTorch-ROCm custom ops") for the arithmetic the reference runs at openset_imagenet/train.py:132-139:
//
//   torch.ops.osi.resnet50_forward    model.py:28-39   (logits, features = model(images))
//   torch.ops.osi.resnet50_forward_frozen  the same on frozen BatchNorm statistics, differentiable (eval-mode gradients, freeze_bn())
//   torch.ops.osi.resnet50_backward   train.py:138     (j.backward() through the network, stage range for the DP bucket schedule)
//   torch.ops.osi.resnet50_backward_ex  the same, plus dJ/dimage and the input-only backward (adversarial samples, attribution)
//   torch.ops.osi.resnet50_backward_adv the same, the last stage writing the FGSM batch; torch.ops.osi.grad_accumulate sums two arenas
//   torch.ops.osi.resnet50_backward_attack  full or input-only backward ending in a projected attack step (PGD); stem_dgrad_pgd: that kernel
//   torch.ops.osi.resnet50_grads_ready  config/train.yaml:18,35-39 (hand a finished stage's gradients to the communication stream)
//   torch.ops.osi.loss_fwd_bwd        losses.py:16-29, train.py:343-347 (the three losses + objectosphere term, value and gradient)
//   torch.ops.osi.adam_step / sgd_step    train.py:139, 356-359; adam_step_groups / sgd_step_groups: the same with parameter groups;
//                                         grad_clip_scale + *_step_groups_dev: gradient-norm clipping, the scalar left on the device
//   torch.ops.osi.average_update      EMA / SWA of the arenas in one launch (averaging.py); resnet50_set_bn_momentum: update_bn's 1 / k
//   torch.ops.osi.stage_canvas        train.py:259-263 after decode + resize (crop, flip, ToTensor, NHWC4)
//   torch.ops.osi.softmax / confidence_accumulate    train.py:177, metrics.py:8-42
//   torch.ops.osi.openmax_class_means / _distances / _fit_tails / _wscores / _recalibrate    OpenMax (openset_imagenet/openmax.py)
//   torch.ops.osi.evm_distances / _fit_rows / _set_cover / _probs                            the Extreme Value Machine (openset_imagenet/evm.py)
//   torch.ops.osi.knn_topk / knn_class_kth                                                   deep nearest neighbours (openset_imagenet/knn.py)
//   torch.ops.osi.maha_class_means / _scatter / _factor / _whiten / _sqdist                  Mahalanobis scores (openset_imagenet/mahalanobis.py)
//   torch.ops.osi.eigh_begin / eigh_sweep / eigh_finish / vim_project / vim_scores           ViM scores, symmetric eigensolver (openset_imagenet/vim.py)
//   torch.ops.osi.resnet50_pooled / order_stats / shape_rows / logit_scores                  activation shaping: ReAct, ASH, SCALE (openset_imagenet/shaping.py)
//   torch.ops.osi.odin_head / gradnorm_scores                                                ODIN's head and GradNorm (openset_imagenet/odin.py)
//   torch.ops.osi.mix_rows_pairs / resnet50_set_mix / proser_loss_fwd_bwd / proser_scores / linear_fwd / linear_bwd    PROSER (openset_imagenet/proser.py)
//
// This file contains no arithmetic: every op validates its arguments, takes the CURRENT HIP stream of its tensors' device inside the
// op, and forwards raw pointers to the C ABI of libosi_hip.so (include/osi.h), which stays the boundary a non-Python host binds.
// Tensor arguments keep their storage alive for the duration of the call and the dispatcher / profiler see the ops by name; stream
// and lifetime safety do not depend on the caller passing data_ptr()s.
//
// One vocabulary of checks, all of them TORCH_CHECKs (RuntimeError) that report as "osi::<op>: ..." and format nothing unless they fail:
//   Op op("name", ref, dtype, "arg", align)   the op's context: checks its reference tensor (usually the first tensor argument; W in
//                                             maha_whiten, the workspace in resnet50_pooled), guards that tensor's device; op.stream()
//   op.need(t, dtype, "arg", align)           a required tensor: defined, on the GPU, dtype, contiguous, aligned, on ref's device
//   op.opt<S>(t, "arg", align, numel)         an optional tensor: the same checks when present (+ its element count), S* or nullptr
//   op.workspace(t, align, at_least)          a scratch tensor: pointer and size; at_least where the C ABI offers a size query
//   op.dim(v) / op.size(v) / clamped(v)       an int64 that must lie in [1, INT_MAX] / in [0, INT_MAX] / that the C ABI is to refuse
//   op.rows(a, b) / op.entries(t, n, "arg") / op.square(t, "arg") / OP_CHECK(cond, ...)     shape relations
//   i64(t)                                    the long long* the C ABI spells an int64 tensor with
// Alignment classes, per op as its kernels read: 16 for 16-byte vector accesses (the arenas, images, attack batches, the executor's
// workspace); 8 for the workspaces of EVM, kNN, Mahalanobis, ViM / eigh and shaping and for the fp64 matrices and vectors of
// Mahalanobis, ViM and eigh; NATURAL for tensors read element-wise (logits, targets, features, class weights, gradients of the head,
// OpenMax's workspace, the fp64 Weibull parameters of OpenMax / EVM, acc4), so a contiguous row slice such as logits[3:] with an odd
// class count is accepted; 1 for byte flags. opt() has no default alignment: an optional arena has to say 16. Sizes the C ABI
// validates itself (enum values, tail sizes, overlaps) are passed through, clamped into int where they are int64 here.
#include <torch/library.h>
#include <ATen/ATen.h>
// PyTorch-ROCm keeps the device type spelled "cuda"; these are its own HIP stream / guard classes for that spelling
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <algorithm>
#include <climits>
#include <optional>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/osi.h"

namespace {

using at::Tensor;
using std::optional;

void ok(int code, const char* what) {
    TORCH_CHECK(code == OSI_OK, "libosi_hip ", what, " failed: ", osi_strerror(code), " (code ", code, ")");
}

osi_resnet50_t handle(int64_t h) {
    TORCH_CHECK(h != 0, "osi: null executor handle");
    return reinterpret_cast<osi_resnet50_t>(static_cast<uintptr_t>(h));
}

constexpr uintptr_t NATURAL = 4;   // element-wise readers: fp32 / int64 / fp64 tensors from the allocator or row slices of them

bool present(const optional<Tensor>& t) { return t.has_value() && t->defined(); }
long long* i64(const Tensor& t) { return reinterpret_cast<long long*>(t.data_ptr<int64_t>()); }
int clamped(int64_t v) { return (int)std::min<int64_t>(std::max<int64_t>(v, -1), INT_MAX); }

struct Workspace { void* ptr; size_t bytes; };

struct Op {
    const char* name;       // every refusal reports as osi::<name>
    const char* ref_name;
    const Tensor& ref;      // the tensor whose device runs the op: guard, stream, and where every other tensor has to live
    const c10::Device device;
    c10::hip::HIPGuardMasqueradingAsCUDA guard;

    Op(const char* name, const Tensor& ref, at::ScalarType dt, const char* arg, uintptr_t align = 16)
        : name(name), ref_name(arg), ref(ref), device(checked(ref, dt, arg, align)), guard(device) {}
    Op(const char* name, at::TensorList refs, at::ScalarType dt, const char* arg, uintptr_t align = 16)
        : Op(name, first(name, refs, arg), dt, arg, align) {}

    osi_stream_t stream() const { return (osi_stream_t)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(device.index()).stream(); }

    void need(const Tensor& t, at::ScalarType dt, const char* arg, uintptr_t align = 16) const {
        TORCH_CHECK(checked(t, dt, arg, align) == device, "osi::", name, ": ", arg, " lives on another device than ", ref_name);
    }

    template <typename S>
    S* opt(const optional<Tensor>& t, const char* arg, uintptr_t align, int64_t numel = -1) const {
        if (!present(t)) return nullptr;
        constexpr bool ll = std::is_same_v<std::remove_const_t<S>, long long>;
        need(*t, ll ? at::kLong : c10::CppTypeToScalarType<std::conditional_t<ll, int64_t, S>>::value, arg, align);
        if (numel >= 0) entries(*t, numel, arg);
        if constexpr (ll) return i64(*t); else return t->template data_ptr<S>();
    }

    Workspace workspace(const Tensor& ws, uintptr_t align, size_t at_least = 0) const {
        need(ws, at::kByte, "workspace", align);
        TORCH_CHECK((size_t)ws.numel() >= at_least, "osi::", name, ": workspace too small (", ws.numel(), " bytes, ", at_least, " needed)");
        return {ws.data_ptr(), (size_t)ws.numel()};
    }

    int dim(int64_t v) const { TORCH_CHECK(v >= 1 && v <= INT_MAX, "osi::", name, ": sizes out of range"); return (int)v; }
    int size(int64_t v) const { TORCH_CHECK(v >= 0 && v <= INT_MAX, "osi::", name, ": sizes out of range"); return (int)v; }

    void rows(const Tensor& a, const Tensor& b) const {
        TORCH_CHECK(a.size(0) == b.size(0), "osi::", name, ": tensors disagree on the number of rows");
    }
    void entries(const Tensor& t, int64_t n, const char* arg) const {
        TORCH_CHECK(t.numel() == n, "osi::", name, ": ", arg, " must hold ", n, " entries, got ", t.numel());
    }
    void square(const Tensor& t, const char* arg) const {
        TORCH_CHECK(t.dim() == 2 && t.size(0) == t.size(1), "osi::", name, ": ", arg, " must be [n, n], got ", t.sizes());
    }

private:
    // what a tensor has to be on its own; returns its device. Reads `name` only, so the constructor may call it before the guard exists
    c10::Device checked(const Tensor& t, at::ScalarType dt, const char* arg, uintptr_t align) const {
        TORCH_CHECK(t.defined(), "osi::", name, ": ", arg, " is an undefined tensor");
        TORCH_CHECK(t.is_cuda(), "osi::", name, ": ", arg, " must live on the GPU: the MI355X build has no CPU path");
        TORCH_CHECK(t.scalar_type() == dt, "osi::", name, ": ", arg, " has dtype ", t.scalar_type(), ", expected ", dt);
        TORCH_CHECK(t.is_contiguous(), "osi::", name, ": ", arg, " must be contiguous");
        TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & (align - 1)) == 0, "osi::", name, ": ", arg, " must be ", align, "-byte aligned");
        return t.device();
    }
    static const Tensor& first(const char* name, at::TensorList refs, const char* arg) {
        TORCH_CHECK(!refs.empty(), "osi::", name, ": ", arg, " is an empty list");
        return refs[0];
    }
};
// any other relation, in the function that holds `op`
#define OP_CHECK(cond, ...) TORCH_CHECK(cond, "osi::", op.name, ": ", __VA_ARGS__)

// the executor was created for ONE geometry: a batch of another shape would read / write outside its workspace
struct Geometry { int B = 0, H = 0, W = 0; };
Geometry geometry(osi_resnet50_t h) {
    Geometry g;
    ok(osi_resnet50_geometry(h, &g.B, &g.H, &g.W), "osi_resnet50_geometry");
    return g;
}
void nhwc4(const Op& op, const Tensor& t, const char* arg, const Geometry& g) {
    OP_CHECK(t.dim() == 4 && t.size(0) == g.B && t.size(1) == g.H && t.size(2) == g.W && t.size(3) == 4, arg, " must be [", g.B, ", ", g.H, ", ",
             g.W, ", 4] (NHWC4), got ", t.sizes());
}

// image: fp32 NCHW [B,3,H,W] (the reference's batch), fp32 NHWC4 [B,H,W,4] (bound in place) or uint8 [B,H,W,3] (+ flip flags)
// nbt == nullptr: the frozen-statistics forward (osi_resnet50_forward_frozen: buffers read-only, no num_batches_tracked)
std::tuple<Tensor, Tensor> forward_common(const Op& op, int64_t net, const Tensor& params, const Tensor& buffers, const Tensor* nbt_p,
                                          const Tensor& image, const optional<Tensor>& flip, const Tensor& workspace, int64_t fc_dim,
                                          int64_t out_features, bool training) {
    op.need(buffers, at::kFloat, "buffers");
    if (nbt_p) op.need(*nbt_p, at::kLong, "num_batches_tracked");
    const Workspace ws = op.workspace(workspace, 16);
    OP_CHECK(image.dim() == 4, "image must be 4-D");
    osi_resnet50_t h = handle(net);
    OP_CHECK(ws.bytes >= osi_resnet50_workspace_bytes(h), "workspace too small");
    OP_CHECK((size_t)params.numel() == osi_resnet50_param_floats(h), "parameter arena size mismatch");
    OP_CHECK((size_t)buffers.numel() == osi_resnet50_buffer_floats(h), "buffer arena size mismatch");
    OP_CHECK(!nbt_p || nbt_p->numel() == osi_resnet50_num_bn(h), "num_batches_tracked size mismatch");
    osi_stream_t st = op.stream();
    const int64_t B = image.size(0);
    const bool u8 = image.scalar_type() == at::kByte, nhwc = !u8 && image.size(3) == 4 && image.size(1) != 3;
    {
        const Geometry g = geometry(h);
        const int64_t ih = u8 || nhwc ? image.size(1) : image.size(2), iw = u8 || nhwc ? image.size(2) : image.size(3);
        OP_CHECK(B == g.B && ih == g.H && iw == g.W, "image batch ", B, "x", ih, "x", iw, " does not match the executor's geometry ", g.B, "x",
                 g.H, "x", g.W);
    }
    const float* img = nullptr;
    if (u8) {
        op.need(image, at::kByte, "image"); OP_CHECK(image.size(3) == 3, "uint8 image batch must be [B,H,W,3]");
        const unsigned char* fl = op.opt<unsigned char>(flip, "flip", 16, B);
        ok(osi_resnet50_stage_input_u8(h, image.data_ptr<unsigned char>(), fl, ws.ptr, st), "osi_resnet50_stage_input_u8");
    } else if (nhwc) {
        op.need(image, at::kFloat, "image");
        ok(osi_resnet50_bind_input_nhwc4(h, image.data_ptr<float>()), "osi_resnet50_bind_input_nhwc4");
    } else {
        op.need(image, at::kFloat, "image"); OP_CHECK(image.size(1) == 3, "fp32 image batch must be [B,3,H,W]");
        img = image.data_ptr<float>();
    }
    Tensor logits = at::empty({B, out_features}, params.options());
    Tensor features = at::empty({B, fc_dim}, params.options());
    if (nbt_p)
        ok(osi_resnet50_forward(h, params.data_ptr<float>(), buffers.data_ptr<float>(), i64(*nbt_p), img, ws.ptr, logits.data_ptr<float>(),
                                features.data_ptr<float>(), training ? 1 : 0, st), "osi_resnet50_forward");
    else
        ok(osi_resnet50_forward_frozen(h, params.data_ptr<float>(), buffers.data_ptr<float>(), img, ws.ptr, logits.data_ptr<float>(),
                                       features.data_ptr<float>(), st), "osi_resnet50_forward_frozen");
    return {logits, features};
}

std::tuple<Tensor, Tensor> resnet50_forward(int64_t net, const Tensor& params, Tensor buffers, Tensor nbt, const Tensor& image,
                                            const optional<Tensor>& flip, Tensor workspace, int64_t fc_dim, int64_t out_features,
                                            bool training) {
    Op op("resnet50_forward", params, at::kFloat, "params");
    return forward_common(op, net, params, buffers, &nbt, image, flip, workspace, fc_dim, out_features, training);
}

// ABI 12: the differentiable forward on frozen BatchNorm statistics (eval-mode gradients, freeze_bn()); the running statistics are read,
// never written, and the backward ops that follow run the frozen dataflow
std::tuple<Tensor, Tensor> resnet50_forward_frozen(int64_t net, const Tensor& params, const Tensor& buffers, const Tensor& image,
                                                   const optional<Tensor>& flip, Tensor workspace, int64_t fc_dim, int64_t out_features) {
    Op op("resnet50_forward_frozen", params, at::kFloat, "params");
    return forward_common(op, net, params, buffers, nullptr, image, flip, workspace, fc_dim, out_features, false);
}

// what every backward op takes: the arenas, the executor's workspace and the gradients of the head. param_grads = false: `grads` is not
// touched and may be an empty tensor
struct Backward { float* grads; void* ws; const float* dfeatures; };
Backward backward_args(const Op& op, const Tensor& params, const Tensor& grads, const Tensor& workspace, const Tensor& dlogits,
                       const optional<Tensor>& dfeatures, bool param_grads = true) {
    const Workspace ws = op.workspace(workspace, 16);
    op.need(dlogits, at::kFloat, "dlogits", NATURAL);
    const float* df = op.opt<float>(dfeatures, "dfeatures", NATURAL);
    if (!param_grads) return {nullptr, ws.ptr, df};
    op.need(grads, at::kFloat, "grads");
    OP_CHECK(grads.numel() == params.numel(), "gradient arena size mismatch");
    return {grads.data_ptr<float>(), ws.ptr, df};
}

void resnet50_backward(int64_t net, const Tensor& params, Tensor grads, Tensor workspace, const Tensor& dlogits,
                       const optional<Tensor>& dfeatures, int64_t stage_lo, int64_t stage_hi) {
    Op op("resnet50_backward", params, at::kFloat, "params");
    const Backward b = backward_args(op, params, grads, workspace, dlogits, dfeatures);
    ok(osi_resnet50_backward(handle(net), params.data_ptr<float>(), b.grads, b.ws, dlogits.data_ptr<float>(), b.dfeatures, (int)stage_lo,
                             (int)stage_hi, op.stream()), "osi_resnet50_backward");
}

// ABI 8: the same backward that can also write dJ/dimage (NCHW fp32 [B][3][H][W] of the executor's geometry) and/or skip every
// parameter gradient
void resnet50_backward_ex(int64_t net, const Tensor& params, Tensor grads, Tensor workspace, const Tensor& dlogits,
                          const optional<Tensor>& dfeatures, const optional<Tensor>& dimage, bool param_grads, int64_t stage_lo,
                          int64_t stage_hi) {
    Op op("resnet50_backward_ex", params, at::kFloat, "params");
    const Backward b = backward_args(op, params, grads, workspace, dlogits, dfeatures, param_grads);
    OP_CHECK(present(dimage) || param_grads, "neither dimage nor parameter gradients requested");
    float* dx = op.opt<float>(dimage, "dimage", NATURAL);
    if (present(dimage)) {
        const Geometry g = geometry(handle(net));
        OP_CHECK(dimage->dim() == 4 && dimage->size(0) == g.B && dimage->size(1) == 3 && dimage->size(2) == g.H && dimage->size(3) == g.W,
                 "dimage must be [", g.B, ", 3, ", g.H, ", ", g.W, "] (NCHW), got ", dimage->sizes());
    }
    ok(osi_resnet50_backward_ex(handle(net), params.data_ptr<float>(), b.grads, b.ws, dlogits.data_ptr<float>(), b.dfeatures, dx,
                                param_grads ? 1 : 0, (int)stage_lo, (int)stage_hi, op.stream()), "osi_resnet50_backward_ex");
}

// ABI 10: the training backward whose last stage writes the FGSM batch x_adv = clamp(x + eps * sign(dJ/dimage), lo, hi) as NHWC4
// [B, H, W, 4] from the input the forward read (adversarial negatives, openset_imagenet/adversary.py)
void resnet50_backward_adv(int64_t net, const Tensor& params, Tensor grads, Tensor workspace, const Tensor& dlogits,
                           const optional<Tensor>& dfeatures, Tensor x_adv, double eps, double lo, double hi, int64_t stage_lo,
                           int64_t stage_hi) {
    Op op("resnet50_backward_adv", params, at::kFloat, "params");
    const Backward b = backward_args(op, params, grads, workspace, dlogits, dfeatures);
    op.need(x_adv, at::kFloat, "x_adv");
    nhwc4(op, x_adv, "x_adv", geometry(handle(net)));
    ok(osi_resnet50_backward_adv(handle(net), params.data_ptr<float>(), b.grads, b.ws, dlogits.data_ptr<float>(), b.dfeatures,
                                 x_adv.data_ptr<float>(), (float)eps, (float)lo, (float)hi, (int)stage_lo, (int)stage_hi, op.stream()),
       "osi_resnet50_backward_adv");
}

// ABI 19: a backward whose last launch is one projected attack step (osi_stem_dgrad_pgd) from the batch the forward read towards x_next,
// projected onto the eps-ball around x_anchor (None: around the forward's own batch). param_grads = false: input-only, nothing runs on
// the side stream (the inner steps of a PGD attack, attacks inside validate())
void resnet50_backward_attack(int64_t net, const Tensor& params, Tensor grads, Tensor workspace, const Tensor& dlogits,
                              const optional<Tensor>& dfeatures, Tensor x_next, const optional<Tensor>& x_anchor, double alpha, double eps,
                              double lo, double hi, bool param_grads, int64_t stage_lo, int64_t stage_hi) {
    Op op("resnet50_backward_attack", params, at::kFloat, "params");
    const Backward b = backward_args(op, params, grads, workspace, dlogits, dfeatures, param_grads);
    op.need(x_next, at::kFloat, "x_next");
    const Geometry g = geometry(handle(net));
    nhwc4(op, x_next, "x_next", g);
    osi_attack a{x_next.data_ptr<float>(), op.opt<float>(x_anchor, "x_anchor", 16), (float)alpha, (float)eps, (float)lo, (float)hi};
    if (present(x_anchor)) nhwc4(op, *x_anchor, "x_anchor", g);
    ok(osi_resnet50_backward_attack(handle(net), params.data_ptr<float>(), b.grads, b.ws, dlogits.data_ptr<float>(), b.dfeatures, &a,
                                    param_grads ? 1 : 0, (int)stage_lo, (int)stage_hi, op.stream()), "osi_resnet50_backward_attack");
}

// ABI 19: the stem's input gradient ending in one projected attack step, on its own (dy [B, Hs, Ws, 64] NHWC, w [64, 7, 7, 3] storage
// order, three NHWC4 batches of one shape); returns nothing, x_next is written
void stem_dgrad_pgd(const Tensor& dy, const Tensor& w_krsc3, const Tensor& x_cur, const Tensor& x_anchor, Tensor x_next, double alpha,
                    double eps, double lo, double hi) {
    Op op("stem_dgrad_pgd", x_cur, at::kFloat, "x_cur");
    op.need(dy, at::kFloat, "dy"); op.need(w_krsc3, at::kFloat, "w_krsc3", NATURAL);
    op.need(x_anchor, at::kFloat, "x_anchor"); op.need(x_next, at::kFloat, "x_next");
    OP_CHECK(x_cur.dim() == 4 && x_cur.size(3) == 4, "x_cur must be [B, H, W, 4] (NHWC4), got ", x_cur.sizes());
    OP_CHECK(x_anchor.sizes() == x_cur.sizes() && x_next.sizes() == x_cur.sizes(), "the three batches differ in shape");
    const int64_t B = x_cur.size(0), H = x_cur.size(1), W = x_cur.size(2);
    OP_CHECK(dy.dim() == 4 && dy.size(0) == B && dy.size(1) == (H - 1) / 2 + 1 && dy.size(2) == (W - 1) / 2 + 1 && dy.size(3) == 64,
             "dy must be [", B, ", ", (H - 1) / 2 + 1, ", ", (W - 1) / 2 + 1, ", 64] (NHWC), got ", dy.sizes());
    op.entries(w_krsc3, 64 * 7 * 7 * 3, "w_krsc3");
    ok(osi_stem_dgrad_pgd(dy.data_ptr<float>(), w_krsc3.data_ptr<float>(), x_cur.data_ptr<float>(), x_anchor.data_ptr<float>(),
                          x_next.data_ptr<float>(), (float)alpha, (float)eps, (float)lo, (float)hi, (int)B, (int)H, (int)W, op.stream()),
       "osi_stem_dgrad_pgd");
}

// dst += src over two gradient arenas of the same length
void grad_accumulate(Tensor dst, const Tensor& src) {
    Op op("grad_accumulate", dst, at::kFloat, "dst");
    op.need(src, at::kFloat, "src");
    op.entries(src, dst.numel(), "src");
    ok(osi_grad_accumulate(dst.data_ptr<float>(), src.data_ptr<float>(), (size_t)dst.numel(), op.stream()), "osi_grad_accumulate");
}

// ABI 20: avg[i] = lerp(avg[i], cur[i], weight) over 1 .. OSI_AVG_MAX_SPANS pairs of contiguous fp32 tensors in ONE launch (EMA / SWA of
// the parameter and buffer arenas, openset_imagenet/averaging.py); overlaps and the weight are validated by the C ABI
void average_update(at::TensorList avg, at::TensorList cur, double weight) {
    Op op("average_update", avg, at::kFloat, "avg");
    OP_CHECK(avg.size() <= OSI_AVG_MAX_SPANS && cur.size() == avg.size(), "1 .. ", OSI_AVG_MAX_SPANS,
             " tensors in each list, as many current as averaged ones");
    osi_avg_span spans[OSI_AVG_MAX_SPANS];
    for (size_t i = 0; i < avg.size(); ++i) {
        op.need(avg[i], at::kFloat, "avg"); op.need(cur[i], at::kFloat, "cur");
        OP_CHECK(avg[i].numel() == cur[i].numel(), "pair ", i, " differs in size");
        spans[i] = osi_avg_span{avg[i].data_ptr<float>(), cur[i].data_ptr<float>(), (size_t)avg[i].numel()};
    }
    ok(osi_average_update(spans, (int)avg.size(), (float)weight, op.stream()), "osi_average_update");
}

// ABI 20: the executor's running-statistics update factor, in force from its next training-mode forward (no tensor: a host setting)
void resnet50_set_bn_momentum(int64_t net, double momentum) {
    ok(osi_resnet50_set_bn_momentum(handle(net), (float)momentum), "osi_resnet50_set_bn_momentum");
}

// Data parallel: the stream `waiter` (a raw hipStream_t handle: torch.cuda.Stream.cuda_stream of the communication stream) waits for the
// gradients of the backward stages enqueued so far on the CURRENT stream and on the executor's side stream; the current stream waits for nothing
void resnet50_grads_ready(int64_t net, const Tensor& grads, int64_t waiter) {
    Op op("resnet50_grads_ready", grads, at::kFloat, "grads");
    ok(osi_resnet50_grads_ready(handle(net), op.stream(), reinterpret_cast<osi_stream_t>(static_cast<uintptr_t>(waiter))),
       "osi_resnet50_grads_ready");
}

// returns (loss [], dlogits [B,C] or empty, dfeatures [B,F] or empty)
std::tuple<Tensor, Tensor, Tensor> loss_fwd_bwd(int64_t mode, const Tensor& logits, const Tensor& target, double unk_weight,
                                                int64_t ignore_index, const optional<Tensor>& class_weights,
                                                const optional<Tensor>& features, double xi, double alpha, bool need_grad) {
    Op op("loss_fwd_bwd", logits, at::kFloat, "logits", NATURAL);
    op.need(target, at::kLong, "target", NATURAL);
    OP_CHECK(logits.dim() == 2 && target.dim() == 1 && target.size(0) == logits.size(0), "expected logits [B, C] and target [B]");
    const int B = (int)logits.size(0), C = (int)logits.size(1);
    Tensor loss = at::empty({}, logits.options());
    Tensor dlogits = need_grad ? at::empty_like(logits) : at::empty({0}, logits.options());
    Tensor dfeat = at::empty({0}, logits.options());
    int F = 0;
    const float* cw = op.opt<float>(class_weights, "class_weights", NATURAL, C);
    const float* feat = op.opt<float>(features, "features", NATURAL);
    if (present(features)) {
        OP_CHECK(features->dim() == 2 && features->size(0) == B, "features must be [B, F]");
        F = (int)features->size(1);
        dfeat = at::empty_like(*features);
    }
    ok(osi_loss_fwd_bwd((int)mode, logits.data_ptr<float>(), i64(target), B, C, (float)unk_weight, (long long)ignore_index, cw, feat, F,
                        (float)xi, (float)alpha, loss.data_ptr<float>(), need_grad ? dlogits.data_ptr<float>() : nullptr,
                        F ? dfeat.data_ptr<float>() : nullptr, op.stream()), "osi_loss_fwd_bwd");
    return {loss, dlogits, dfeat};
}

// an optimizer state arena: fp32, 16-byte aligned, as long as the parameter arena
float* state(const Op& op, const Tensor& t, const char* arg) {
    op.need(t, at::kFloat, arg);
    op.entries(t, op.ref.numel(), arg);
    return t.data_ptr<float>();
}

void adam_step(Tensor params, const Tensor& grads, Tensor exp_avg, Tensor exp_avg_sq, double lr, double beta1, double beta2, double eps,
               int64_t step, double grad_scale) {
    Op op("adam_step", params, at::kFloat, "params");
    float* g = state(op, grads, "grads");
    float* m = state(op, exp_avg, "exp_avg");
    float* v = state(op, exp_avg_sq, "exp_avg_sq");
    ok(osi_adam_step(params.data_ptr<float>(), g, m, v, (size_t)params.numel(), lr, beta1, beta2, eps, (long long)step, (float)grad_scale,
                     op.stream()), "osi_adam_step");
}

void sgd_step(Tensor params, const Tensor& grads, Tensor momentum_buffer, double lr, double momentum, bool first, double grad_scale) {
    Op op("sgd_step", params, at::kFloat, "params");
    float* g = state(op, grads, "grads");
    float* m = state(op, momentum_buffer, "momentum_buffer");
    ok(osi_sgd_step(params.data_ptr<float>(), g, m, (size_t)params.numel(), (float)lr, (float)momentum, first ? 1 : 0, (float)grad_scale,
                    op.stream()), "osi_sgd_step");
}

// segments: flat (begin4, end4, group) triples; the group tables are flat rows of doubles in the field order of osi_adam_group /
// osi_sgd_group. Everything else is validated by the C ABI.
std::vector<osi_opt_segment> opt_segments(const Op& op, c10::ArrayRef<int64_t> segments) {
    OP_CHECK(segments.size() % 3 == 0, "segments: flat (begin4, end4, group) triples");
    std::vector<osi_opt_segment> seg(segments.size() / 3);
    for (size_t i = 0; i < seg.size(); ++i) {
        for (int j = 0; j < 2; ++j)
            OP_CHECK(segments[3 * i + j] >= 0 && segments[3 * i + j] <= 0xFFFFFFFFll, "segment bounds out of range");
        OP_CHECK(segments[3 * i + 2] >= 0 && segments[3 * i + 2] < OSI_OPT_MAX_GROUPS, "segment group index out of range");
        seg[i] = osi_opt_segment{(unsigned)segments[3 * i], (unsigned)segments[3 * i + 1], (int)segments[3 * i + 2]};
    }
    return seg;
}

// the scalar of a *_dev step: one fp32 element on the arena's device (e.g. the second element of grad_clip_scale's out2)
const float* dev_scalar(const Op& op, const Tensor& s) {
    op.need(s, at::kFloat, "grad_scale", NATURAL);
    op.entries(s, 1, "grad_scale");
    return s.data_ptr<float>();
}

// grad_scale_dev == nullptr: the scalar by value (osi_adam_step_groups); else the kernel reads it from device memory (_dev)
void adam_groups_common(const Op& op, Tensor& params, const Tensor& grads, Tensor& exp_avg, Tensor& exp_avg_sq,
                        const optional<Tensor>& max_exp_avg_sq, c10::ArrayRef<int64_t> segments, c10::ArrayRef<double> groups,
                        double grad_scale, const float* grad_scale_dev) {
    float* g = state(op, grads, "grads");
    float* m = state(op, exp_avg, "exp_avg");
    float* v = state(op, exp_avg_sq, "exp_avg_sq");
    float* vmax = op.opt<float>(max_exp_avg_sq, "max_exp_avg_sq", 16, params.numel());
    OP_CHECK(groups.size() % 9 == 0, "groups: rows of (lr, beta1, beta2, eps, weight_decay, step, decoupled, amsgrad, maximize)");
    const std::vector<osi_opt_segment> seg = opt_segments(op, segments);
    std::vector<osi_adam_group> gs(groups.size() / 9);
    for (size_t i = 0; i < gs.size(); ++i) {
        const double* r = &groups[9 * i];
        gs[i] = osi_adam_group{r[0], r[1], r[2], r[3], r[4], (long long)r[5], r[6] != 0.0, r[7] != 0.0, r[8] != 0.0};
    }
    if (grad_scale_dev)
        ok(osi_adam_step_groups_dev(params.data_ptr<float>(), g, m, v, vmax, (size_t)params.numel(), seg.data(), (int)seg.size(), gs.data(),
                                    (int)gs.size(), grad_scale_dev, op.stream()), "osi_adam_step_groups_dev");
    else
        ok(osi_adam_step_groups(params.data_ptr<float>(), g, m, v, vmax, (size_t)params.numel(), seg.data(), (int)seg.size(), gs.data(),
                                (int)gs.size(), (float)grad_scale, op.stream()), "osi_adam_step_groups");
}

void sgd_groups_common(const Op& op, Tensor& params, const Tensor& grads, Tensor& momentum_buffer, c10::ArrayRef<int64_t> segments,
                       c10::ArrayRef<double> groups, double grad_scale, const float* grad_scale_dev) {
    float* g = state(op, grads, "grads");
    float* m = state(op, momentum_buffer, "momentum_buffer");
    OP_CHECK(groups.size() % 7 == 0, "groups: rows of (lr, momentum, dampening, weight_decay, nesterov, first_step, maximize)");
    const std::vector<osi_opt_segment> seg = opt_segments(op, segments);
    std::vector<osi_sgd_group> gs(groups.size() / 7);
    for (size_t i = 0; i < gs.size(); ++i) {
        const double* r = &groups[7 * i];
        gs[i] = osi_sgd_group{r[0], r[1], r[2], r[3], r[4] != 0.0, r[5] != 0.0, r[6] != 0.0};
    }
    if (grad_scale_dev)
        ok(osi_sgd_step_groups_dev(params.data_ptr<float>(), g, m, (size_t)params.numel(), seg.data(), (int)seg.size(), gs.data(),
                                   (int)gs.size(), grad_scale_dev, op.stream()), "osi_sgd_step_groups_dev");
    else
        ok(osi_sgd_step_groups(params.data_ptr<float>(), g, m, (size_t)params.numel(), seg.data(), (int)seg.size(), gs.data(), (int)gs.size(),
                               (float)grad_scale, op.stream()), "osi_sgd_step_groups");
}

void adam_step_groups(Tensor params, const Tensor& grads, Tensor exp_avg, Tensor exp_avg_sq, const optional<Tensor>& max_exp_avg_sq,
                      c10::ArrayRef<int64_t> segments, c10::ArrayRef<double> groups, double grad_scale) {
    Op op("adam_step_groups", params, at::kFloat, "params");
    adam_groups_common(op, params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, segments, groups, grad_scale, nullptr);
}

void sgd_step_groups(Tensor params, const Tensor& grads, Tensor momentum_buffer, c10::ArrayRef<int64_t> segments,
                     c10::ArrayRef<double> groups, double grad_scale) {
    Op op("sgd_step_groups", params, at::kFloat, "params");
    sgd_groups_common(op, params, grads, momentum_buffer, segments, groups, grad_scale, nullptr);
}

void adam_step_groups_dev(Tensor params, const Tensor& grads, Tensor exp_avg, Tensor exp_avg_sq, const optional<Tensor>& max_exp_avg_sq,
                          c10::ArrayRef<int64_t> segments, c10::ArrayRef<double> groups, const Tensor& grad_scale) {
    Op op("adam_step_groups_dev", params, at::kFloat, "params");
    adam_groups_common(op, params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, segments, groups, 0.0, dev_scalar(op, grad_scale));
}

void sgd_step_groups_dev(Tensor params, const Tensor& grads, Tensor momentum_buffer, c10::ArrayRef<int64_t> segments,
                         c10::ArrayRef<double> groups, const Tensor& grad_scale) {
    Op op("sgd_step_groups_dev", params, at::kFloat, "params");
    sgd_groups_common(op, params, grads, momentum_buffer, segments, groups, 0.0, dev_scalar(op, grad_scale));
}

// spans: flat (begin, numel) pairs in floats, empty = the whole arena. out2 <- (norm of grad_scale * g over the spans, the scalar a
// clipped step multiplies the gradients by); nothing is read back. Everything else is validated by the C ABI.
void grad_clip_scale(const Tensor& grads, c10::ArrayRef<int64_t> spans, int64_t norm_type, double grad_scale, double max_norm,
                     Tensor workspace, Tensor out2) {
    Op op("grad_clip_scale", grads, at::kFloat, "grads");
    op.need(out2, at::kFloat, "out2", NATURAL);
    op.entries(out2, 2, "out2");
    const Workspace ws = op.workspace(workspace, 16, osi_grad_norm_workspace((size_t)grads.numel()));
    OP_CHECK(spans.size() % 2 == 0, "spans: flat (begin, numel) pairs");
    std::vector<osi_grad_span> sp(spans.size() / 2);
    for (size_t i = 0; i < sp.size(); ++i) {
        OP_CHECK(spans[2 * i] >= 0 && spans[2 * i + 1] >= 0, "span bounds out of range");
        sp[i] = osi_grad_span{(unsigned long long)spans[2 * i], (unsigned long long)spans[2 * i + 1]};
    }
    ok(osi_grad_clip_scale(grads.data_ptr<float>(), (size_t)grads.numel(), sp.empty() ? nullptr : sp.data(), (int)sp.size(), (int)norm_type,
                           (float)grad_scale, (float)max_norm, ws.ptr, ws.bytes, out2.data_ptr<float>(), op.stream()), "osi_grad_clip_scale");
}

Tensor stage_canvas(const Tensor& canvas, const optional<Tensor>& crop_xy, const optional<Tensor>& flip, int64_t H, int64_t W) {
    Op op("stage_canvas", canvas, at::kByte, "canvas");
    OP_CHECK(canvas.dim() == 4 && canvas.size(3) == 3, "canvas must be uint8 [B,Hc,Wc,3]");
    const int B = (int)canvas.size(0);
    const int* cp = op.opt<int>(crop_xy, "crop_xy", NATURAL, 2 * B);
    const unsigned char* fl = op.opt<unsigned char>(flip, "flip", 1, B);
    Tensor out = at::empty({B, H, W, 4}, canvas.options().dtype(at::kFloat));
    ok(osi_u8_crop_flip_to_nhwc4(canvas.data_ptr<unsigned char>(), cp, fl, out.data_ptr<float>(), B, (int)canvas.size(1), (int)canvas.size(2),
                                 (int)H, (int)W, op.stream()), "osi_u8_crop_flip_to_nhwc4");
    return out;
}

Tensor softmax(const Tensor& logits) {
    Op op("softmax", logits, at::kFloat, "logits", NATURAL);
    OP_CHECK(logits.dim() == 2, "logits must be [B, C]");
    Tensor out = at::empty_like(logits);
    ok(osi_softmax(logits.data_ptr<float>(), out.data_ptr<float>(), (int)logits.size(0), (int)logits.size(1), op.stream()), "osi_softmax");
    return out;
}

void confidence_accumulate(const Tensor& logits, const Tensor& target, double offset, int64_t unknown_class, int64_t last_valid_class,
                           Tensor acc4) {
    Op op("confidence_accumulate", logits, at::kFloat, "logits", NATURAL);
    op.need(target, at::kLong, "target", NATURAL); op.need(acc4, at::kDouble, "acc4", NATURAL);
    OP_CHECK(logits.dim() == 2, "logits must be [B, C]");
    op.entries(target, logits.size(0), "target"); op.entries(acc4, 4, "acc4");
    ok(osi_confidence_accumulate(logits.data_ptr<float>(), i64(target), (int)logits.size(0), (int)logits.size(1), (float)offset,
                                 (long long)unknown_class, (int)last_valid_class, acc4.data_ptr<double>(), op.stream()),
       "osi_confidence_accumulate");
}

// ---- OpenMax (include/osi.h, ABI 21): every op allocates its outputs and leaves them on the device
std::tuple<Tensor, Tensor, Tensor> openmax_class_means(const Tensor& features, const Tensor& logits, const Tensor& gt, Tensor workspace) {
    Op op("openmax_class_means", features, at::kFloat, "features", NATURAL);
    op.need(logits, at::kFloat, "logits", NATURAL); op.need(gt, at::kLong, "gt", NATURAL);
    OP_CHECK(features.dim() == 2 && logits.dim() == 2 && gt.dim() == 1, "features [N,F], logits [N,C], gt [N]");
    op.rows(features, logits); op.rows(features, gt);
    const int N = (int)features.size(0), F = (int)features.size(1), C = (int)logits.size(1);
    const Workspace ws = op.workspace(workspace, NATURAL, osi_openmax_workspace(N, C, F));
    Tensor mav = at::empty({C, F}, features.options());
    Tensor count = at::empty({C}, features.options().dtype(at::kLong));
    Tensor correct = at::empty({N}, features.options().dtype(at::kByte));
    ok(osi_openmax_class_means(features.data_ptr<float>(), logits.data_ptr<float>(), i64(gt), N, C, F, mav.data_ptr<float>(), i64(count),
                               correct.data_ptr<unsigned char>(), ws.ptr, ws.bytes, op.stream()), "osi_openmax_class_means");
    return {mav, count, correct};
}

Tensor openmax_distances(const Tensor& features, const Tensor& mav, const optional<Tensor>& cls, int64_t metric) {
    Op op("openmax_distances", features, at::kFloat, "features", NATURAL);
    op.need(mav, at::kFloat, "mav", NATURAL);
    OP_CHECK(features.dim() == 2 && mav.dim() == 2 && features.size(1) == mav.size(1), "features [N,F] and mav [C,F]");
    const int N = (int)features.size(0), F = (int)features.size(1), C = (int)mav.size(0);
    const long long* cp = op.opt<long long>(cls, "cls", NATURAL);
    if (present(cls)) {
        OP_CHECK(cls->dim() == 1, "cls is [N]");
        op.rows(features, *cls);
    }
    Tensor dist = cp ? at::empty({N}, features.options()) : at::empty({N, C}, features.options());
    ok(osi_openmax_distances(features.data_ptr<float>(), mav.data_ptr<float>(), cp, N, C, F, (int)metric, dist.data_ptr<float>(), op.stream()),
       "osi_openmax_distances");
    return dist;
}

// what a per-row / per-class Weibull fit returns, on the device of `like`: (shape, scale, shift, fitted, tail_count, flags2)
using Fits = std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor>;
Fits fit_outputs(const Tensor& like, int64_t n) {
    const auto f64 = like.options().dtype(at::kDouble), i64o = like.options().dtype(at::kLong);
    return {at::empty({n}, f64), at::empty({n}, f64), at::empty({n}, f64), at::empty({n}, like.options().dtype(at::kByte)), at::empty({n}, i64o),
            at::empty({2}, i64o)};
}

Fits openmax_fit_tails(const Tensor& dist, const Tensor& gt, const Tensor& correct, int64_t C, int64_t tailsize, Tensor workspace) {
    Op op("openmax_fit_tails", dist, at::kFloat, "dist", NATURAL);
    op.need(gt, at::kLong, "gt", NATURAL); op.need(correct, at::kByte, "correct", 1);
    OP_CHECK(dist.dim() == 1 && gt.dim() == 1 && correct.dim() == 1, "dist, gt and correct are [N]");
    op.rows(dist, gt); op.rows(dist, correct);
    OP_CHECK(C > 0 && C <= INT_MAX, "C out of range");
    const int N = (int)dist.size(0);
    const Workspace ws = op.workspace(workspace, NATURAL, osi_openmax_workspace(N, (int)C, 1));
    Fits out = fit_outputs(dist, C);
    auto& [shape, scale, shift, fitted, tail_count, flags2] = out;
    ok(osi_openmax_fit_tails(dist.data_ptr<float>(), i64(gt), correct.data_ptr<unsigned char>(), N, (int)C, (int)tailsize,
                             shape.data_ptr<double>(), scale.data_ptr<double>(), shift.data_ptr<double>(), fitted.data_ptr<unsigned char>(),
                             i64(tail_count), i64(flags2), ws.ptr, ws.bytes, op.stream()), "osi_openmax_fit_tails");
    return out;
}

Tensor openmax_wscores(const Tensor& dist, const Tensor& shape, const Tensor& scale, const Tensor& shift, const Tensor& fitted) {
    Op op("openmax_wscores", dist, at::kFloat, "dist", NATURAL);
    op.need(shape, at::kDouble, "shape", NATURAL); op.need(scale, at::kDouble, "scale", NATURAL);
    op.need(shift, at::kDouble, "shift", NATURAL); op.need(fitted, at::kByte, "fitted", 1);
    OP_CHECK(dist.dim() == 2, "dist is [N,C]");
    const int64_t C = dist.size(1);
    OP_CHECK(shape.numel() == C && scale.numel() == C && shift.numel() == C && fitted.numel() == C,
             "shape, scale, shift and fitted hold one entry per column of dist");
    Tensor w = at::empty_like(dist);
    ok(osi_openmax_wscores(dist.data_ptr<float>(), (int)dist.size(0), (int)C, shape.data_ptr<double>(), scale.data_ptr<double>(),
                           shift.data_ptr<double>(), fitted.data_ptr<unsigned char>(), w.data_ptr<float>(), op.stream()),
       "osi_openmax_wscores");
    return w;
}

Tensor openmax_recalibrate(const Tensor& logits, const Tensor& w, int64_t alpha) {
    Op op("openmax_recalibrate", logits, at::kFloat, "logits", NATURAL);
    op.need(w, at::kFloat, "w", NATURAL);
    OP_CHECK(logits.dim() == 2 && w.sizes() == logits.sizes(), "logits and w are [N,C]");
    OP_CHECK(alpha >= 1, "alpha must be >= 1");
    const int N = (int)logits.size(0), C = (int)logits.size(1);
    Tensor probs = at::empty({N, C + 1}, logits.options());
    ok(osi_openmax_recalibrate(logits.data_ptr<float>(), w.data_ptr<float>(), N, C, clamped(alpha), probs.data_ptr<float>(), op.stream()),
       "osi_openmax_recalibrate");
    return probs;
}

// ---- Extreme Value Machine (include/osi.h, ABI 22): every op allocates its outputs and leaves them on the device
Tensor evm_distances(const Tensor& a, const Tensor& b, int64_t metric, Tensor workspace) {
    Op op("evm_distances", a, at::kFloat, "a", NATURAL);
    op.need(b, at::kFloat, "b", NATURAL);
    const Workspace ws = op.workspace(workspace, 8);
    OP_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(1), "a [R,F] and b [N,F]");
    const int R = op.size(a.size(0)), N = op.size(b.size(0)), F = op.size(a.size(1));
    Tensor dist = at::empty({R, N}, a.options());
    ok(osi_evm_distances(a.data_ptr<float>(), R, b.data_ptr<float>(), N, F, (int)metric, dist.data_ptr<float>(), ws.ptr, ws.bytes, op.stream()),
       "osi_evm_distances");
    return dist;
}

Fits evm_fit_rows(const Tensor& dist, const Tensor& gt, int64_t cls, int64_t tailsize, double multiplier, Tensor workspace) {
    Op op("evm_fit_rows", dist, at::kFloat, "dist", NATURAL);
    op.need(gt, at::kLong, "gt", NATURAL);
    const Workspace ws = op.workspace(workspace, 8);
    OP_CHECK(dist.dim() == 2 && gt.dim() == 1 && gt.size(0) <= dist.size(1), "dist [R,ld] and gt [N], N <= ld");
    const int R = op.size(dist.size(0)), N = op.size(gt.size(0));
    Fits out = fit_outputs(dist, R);
    auto& [shape, scale, shift, fitted, tail_count, flags2] = out;
    ok(osi_evm_fit_rows(dist.data_ptr<float>(), R, N, (long long)dist.size(1), i64(gt), (long long)cls, (int)std::min<int64_t>(tailsize, INT_MAX),
                        (float)multiplier, shape.data_ptr<double>(), scale.data_ptr<double>(), shift.data_ptr<double>(),
                        fitted.data_ptr<unsigned char>(), i64(tail_count), i64(flags2), ws.ptr, ws.bytes, op.stream()), "osi_evm_fit_rows");
    return out;
}

// the fitted Weibull parameters: three fp64 tensors of n entries
void evm_params(const Op& op, const Tensor& shape, const Tensor& scale, const Tensor& shift, int64_t n) {
    op.need(shape, at::kDouble, "shape", NATURAL); op.need(scale, at::kDouble, "scale", NATURAL); op.need(shift, at::kDouble, "shift", NATURAL);
    OP_CHECK(shape.numel() == n && scale.numel() == n && shift.numel() == n, "shape, scale and shift hold ", n, " entries");
}

std::tuple<Tensor, Tensor> evm_set_cover(const Tensor& dpp, const Tensor& shape, const Tensor& scale, const Tensor& shift,
                                         const Tensor& fitted, double multiplier, double cover_threshold, Tensor workspace) {
    Op op("evm_set_cover", dpp, at::kFloat, "dpp", NATURAL);
    op.need(fitted, at::kByte, "fitted", 1);
    const Workspace ws = op.workspace(workspace, 8);
    op.square(dpp, "dpp");
    const int R = op.size(dpp.size(0));
    evm_params(op, shape, scale, shift, R);
    op.entries(fitted, R, "fitted");
    const auto i64o = dpp.options().dtype(at::kLong);
    Tensor order = at::empty({R}, i64o), n_ev = at::empty({1}, i64o);
    ok(osi_evm_set_cover(dpp.data_ptr<float>(), R, shape.data_ptr<double>(), scale.data_ptr<double>(), shift.data_ptr<double>(),
                         fitted.data_ptr<unsigned char>(), (float)multiplier, (float)cover_threshold, i64(order), i64(n_ev), ws.ptr, ws.bytes,
                         op.stream()), "osi_evm_set_cover");
    return {order, n_ev};
}

Tensor evm_probs(const Tensor& dist, const Tensor& shape, const Tensor& scale, const Tensor& shift, const Tensor& ev_start,
                 double multiplier) {
    Op op("evm_probs", dist, at::kFloat, "dist", NATURAL);
    op.need(ev_start, at::kLong, "ev_start", NATURAL);
    OP_CHECK(dist.dim() == 2 && ev_start.dim() == 1 && ev_start.numel() >= 2, "dist is [M,ld], ev_start [C+1]");
    const int64_t V = shape.numel();
    evm_params(op, shape, scale, shift, V);
    OP_CHECK(V <= dist.size(1), "V <= ld");
    const int M = op.size(dist.size(0)), C = op.size(ev_start.numel() - 1);
    Tensor probs = at::empty({dist.size(0), (int64_t)C}, dist.options());
    ok(osi_evm_probs(dist.data_ptr<float>(), M, op.size(V), (long long)dist.size(1), shape.data_ptr<double>(), scale.data_ptr<double>(),
                     shift.data_ptr<double>(), i64(ev_start), C, (float)multiplier, probs.data_ptr<float>(), op.stream()), "osi_evm_probs");
    return probs;
}

// ---- deep nearest neighbours (include/osi.h, ABI 24): dist is [M,ld], every column of it takes part (N = ld)
int knn_k(const Op& op, int64_t k) {
    OP_CHECK(k >= 1 && k <= OSI_KNN_MAX_K, "k must lie in [1, ", OSI_KNN_MAX_K, "]");
    return (int)k;
}

std::tuple<Tensor, Tensor> knn_topk(const Tensor& dist, int64_t k, const optional<Tensor>& skip, Tensor workspace) {
    Op op("knn_topk", dist, at::kFloat, "dist", NATURAL);
    const Workspace ws = op.workspace(workspace, 8);
    OP_CHECK(dist.dim() == 2, "dist is [M,N]");
    const int M = op.size(dist.size(0)), N = op.size(dist.size(1)), K = knn_k(op, k);
    Tensor out_dist = at::empty({M, K}, dist.options()), out_idx = at::empty({M, K}, dist.options().dtype(at::kLong));
    ok(osi_knn_topk(dist.data_ptr<float>(), M, N, (long long)N, K, op.opt<long long>(skip, "skip", NATURAL, M), out_dist.data_ptr<float>(),
                    i64(out_idx), ws.ptr, ws.bytes, op.stream()), "osi_knn_topk");
    return {out_dist, out_idx};
}

Tensor knn_class_kth(const Tensor& dist, const Tensor& start, int64_t k, const optional<Tensor>& skip, int64_t transform,
                     Tensor workspace) {
    Op op("knn_class_kth", dist, at::kFloat, "dist", NATURAL);
    op.need(start, at::kLong, "start", NATURAL);
    const Workspace ws = op.workspace(workspace, 8);
    OP_CHECK(dist.dim() == 2 && start.dim() == 1 && start.numel() >= 2, "dist is [M,N], start [C+1]");
    const int M = op.size(dist.size(0)), N = op.size(dist.size(1)), C = op.size(start.numel() - 1), K = knn_k(op, k);
    Tensor out = at::empty({M, C}, dist.options());
    ok(osi_knn_class_kth(dist.data_ptr<float>(), M, N, (long long)N, i64(start), C, K, op.opt<long long>(skip, "skip", NATURAL, M),
                         clamped(transform), out.data_ptr<float>(), ws.ptr, ws.bytes, op.stream()), "osi_knn_class_kth");
    return out;
}

// ---- Mahalanobis / Relative Mahalanobis (include/osi.h, ABI 25): fp32 features, int64 labels, every fitted tensor fp64
std::tuple<Tensor, Tensor> maha_class_means(const Tensor& features, const Tensor& gt, int64_t C, Tensor workspace) {
    Op op("maha_class_means", features, at::kFloat, "features", NATURAL);
    op.need(gt, at::kLong, "gt", NATURAL);
    const Workspace ws = op.workspace(workspace, 8);
    OP_CHECK(features.dim() == 2 && gt.dim() == 1 && gt.numel() == features.size(0), "features [N,F], gt [N]");
    const int N = op.dim(features.size(0)), F = op.dim(features.size(1)), c = op.dim(C);
    Tensor mean = at::empty({C + 1, (int64_t)F}, features.options().dtype(at::kDouble));
    Tensor count = at::empty({C + 1}, features.options().dtype(at::kLong));
    ok(osi_maha_class_means(features.data_ptr<float>(), i64(gt), N, c, F, mean.data_ptr<double>(), i64(count), ws.ptr, ws.bytes, op.stream()),
       "osi_maha_class_means");
    return {mean, count};
}

void maha_scatter(const Tensor& features, const Tensor& gt, const Tensor& mean, int64_t mode, bool accumulate, Tensor S, Tensor workspace) {
    Op op("maha_scatter", features, at::kFloat, "features", NATURAL);
    op.need(gt, at::kLong, "gt", NATURAL); op.need(mean, at::kDouble, "mean", 8); op.need(S, at::kDouble, "S", 8);
    const Workspace ws = op.workspace(workspace, 8);
    OP_CHECK(features.dim() == 2 && gt.dim() == 1 && gt.numel() == features.size(0) && mean.dim() == 2 && mean.size(0) >= 2 &&
             mean.size(1) == features.size(1) && S.dim() == 2 && S.size(0) == features.size(1) && S.size(1) == features.size(1),
             "features [N,F], gt [N], mean [C+1,F], S [F,F]");
    const int N = op.dim(features.size(0)), F = op.dim(features.size(1)), C = op.dim(mean.size(0) - 1);
    ok(osi_maha_scatter(features.data_ptr<float>(), i64(gt), mean.data_ptr<double>(), N, C, F, clamped(mode), accumulate ? 1 : 0,
                        S.data_ptr<double>(), ws.ptr, ws.bytes, op.stream()), "osi_maha_scatter");
}

std::tuple<Tensor, Tensor, Tensor, Tensor> maha_factor(const Tensor& S, double scale, double shrinkage, Tensor workspace) {
    Op op("maha_factor", S, at::kDouble, "S", 8);
    const Workspace ws = op.workspace(workspace, 8);
    op.square(S, "S");
    const int F = op.dim(S.size(0));
    Tensor L = at::empty_like(S), W = at::empty_like(S);
    Tensor logdet = at::empty({1}, S.options()), info = at::empty({1}, S.options().dtype(at::kInt));
    ok(osi_maha_factor(S.data_ptr<double>(), F, scale, shrinkage, L.data_ptr<double>(), W.data_ptr<double>(), logdet.data_ptr<double>(),
                       info.data_ptr<int>(), ws.ptr, ws.bytes, op.stream()), "osi_maha_factor");
    return {L, W, logdet, info};
}

Tensor maha_whiten(const Tensor& x, const Tensor& W, Tensor workspace) {
    Op op("maha_whiten", W, at::kDouble, "W", 8);
    const Workspace ws = op.workspace(workspace, 8);
    OP_CHECK(x.defined() && (x.scalar_type() == at::kFloat || x.scalar_type() == at::kDouble), "x is fp32 or fp64");
    op.need(x, x.scalar_type(), "x", NATURAL);
    op.square(W, "W");
    OP_CHECK(x.dim() == 2 && W.size(0) == x.size(1), "x [M,F], W [F,F]");
    const int M = op.dim(x.size(0)), F = op.dim(x.size(1));
    Tensor z = at::empty({(int64_t)M, (int64_t)F}, W.options());
    if (x.scalar_type() == at::kFloat)
        ok(osi_maha_whiten_f32(x.data_ptr<float>(), M, F, W.data_ptr<double>(), z.data_ptr<double>(), ws.ptr, ws.bytes, op.stream()),
           "osi_maha_whiten_f32");
    else
        ok(osi_maha_whiten_f64(x.data_ptr<double>(), M, F, W.data_ptr<double>(), z.data_ptr<double>(), ws.ptr, ws.bytes, op.stream()),
           "osi_maha_whiten_f64");
    return z;
}

Tensor maha_sqdist(const Tensor& z, const Tensor& zm, const optional<Tensor>& minus, int64_t transform, bool f64_out, Tensor workspace) {
    Op op("maha_sqdist", z, at::kDouble, "z", 8);
    op.need(zm, at::kDouble, "zm", 8);
    const Workspace ws = op.workspace(workspace, 8);
    OP_CHECK(z.dim() == 2 && zm.dim() == 2 && zm.size(1) == z.size(1), "z [M,F], zm [C,F]");
    const double* mp = op.opt<double>(minus, "minus", 8, z.size(0));
    const int M = op.dim(z.size(0)), F = op.dim(z.size(1)), C = op.dim(zm.size(0));
    Tensor out = at::empty({(int64_t)M, (int64_t)C}, z.options().dtype(f64_out ? at::kDouble : at::kFloat));
    ok(osi_maha_sqdist(z.data_ptr<double>(), M, zm.data_ptr<double>(), C, F, mp, clamped(transform), f64_out ? nullptr : out.data_ptr<float>(),
                       f64_out ? out.data_ptr<double>() : nullptr, ws.ptr, ws.bytes, op.stream()), "osi_maha_sqdist");
    return out;
}

// ---- ViM and the symmetric eigensolver (include/osi.h, ABI 26): fp32 features and logits, every fitted tensor fp64
std::tuple<Tensor, Tensor, Tensor, Tensor> eigh_begin(const Tensor& S, Tensor workspace) {
    Op op("eigh_begin", S, at::kDouble, "S", 8);
    const Workspace ws = op.workspace(workspace, 8);
    op.square(S, "S");
    const int F = op.dim(S.size(0));
    Tensor A = at::empty_like(S), Vt = at::empty_like(S);
    Tensor head = at::empty({2}, S.options()), info = at::empty({1}, S.options().dtype(at::kInt));
    ok(osi_eigh_begin(S.data_ptr<double>(), F, A.data_ptr<double>(), Vt.data_ptr<double>(), head.data_ptr<double>(), info.data_ptr<int>(),
                      ws.ptr, ws.bytes, op.stream()), "osi_eigh_begin");
    return {A, Vt, head, info};
}

// the solver's state between its calls: A and Vt [F,F] fp64, info one int; returns F
int eigh_state(const Op& op, const Tensor& A, const Tensor& Vt, const Tensor& info) {
    op.need(Vt, at::kDouble, "Vt", 8); op.need(info, at::kInt, "info", NATURAL);
    op.square(A, "A");
    OP_CHECK(Vt.sizes() == A.sizes(), "Vt must have the shape of A");
    op.entries(info, 1, "info");
    return op.dim(A.size(0));
}

Tensor eigh_sweep(Tensor A, Tensor Vt, const Tensor& head, const Tensor& info, Tensor workspace) {
    Op op("eigh_sweep", A, at::kDouble, "A", 8);
    op.need(head, at::kDouble, "head", 8);
    const Workspace ws = op.workspace(workspace, 8);
    const int F = eigh_state(op, A, Vt, info);
    op.entries(head, 2, "head");
    Tensor rotations = at::empty({1}, A.options().dtype(at::kLong));
    ok(osi_eigh_sweep(A.data_ptr<double>(), Vt.data_ptr<double>(), F, head.data_ptr<double>(), info.data_ptr<int>(), i64(rotations), ws.ptr,
                      ws.bytes, op.stream()), "osi_eigh_sweep");
    return rotations;
}

std::tuple<Tensor, Tensor> eigh_finish(const Tensor& A, const Tensor& Vt, const Tensor& info, Tensor workspace) {
    Op op("eigh_finish", A, at::kDouble, "A", 8);
    const Workspace ws = op.workspace(workspace, 8);
    const int F = eigh_state(op, A, Vt, info);
    Tensor evals = at::empty({(int64_t)F}, A.options()), evecs = at::empty_like(A);
    ok(osi_eigh_finish(A.data_ptr<double>(), Vt.data_ptr<double>(), F, info.data_ptr<int>(), evals.data_ptr<double>(), evecs.data_ptr<double>(),
                       ws.ptr, ws.bytes, op.stream()), "osi_eigh_finish");
    return {evals, evecs};
}

Tensor vim_project(const Tensor& x, const Tensor& origin, const Tensor& R, Tensor workspace) {
    Op op("vim_project", x, at::kFloat, "x", NATURAL);
    op.need(origin, at::kDouble, "origin", 8); op.need(R, at::kDouble, "R", 8);
    const Workspace ws = op.workspace(workspace, 8);
    OP_CHECK(x.dim() == 2 && R.dim() == 2 && R.size(1) == x.size(1), "x [M,F], R [K,F]");
    op.entries(origin, x.size(1), "origin");
    const int M = op.dim(x.size(0)), F = op.dim(x.size(1)), K = op.dim(R.size(0));
    Tensor z = at::empty({(int64_t)M, (int64_t)K}, R.options());
    ok(osi_vim_project_f32(x.data_ptr<float>(), origin.data_ptr<double>(), M, F, R.data_ptr<double>(), K, z.data_ptr<double>(), ws.ptr, ws.bytes,
                           op.stream()), "osi_vim_project_f32");
    return z;
}

Tensor vim_scores(const Tensor& z, const optional<Tensor>& logits, double alpha, int64_t mode, bool f64_out, Tensor workspace) {
    Op op("vim_scores", z, at::kDouble, "z", 8);
    const Workspace ws = op.workspace(workspace, 8);
    OP_CHECK(z.dim() == 2, "z [M,K]");
    const int M = op.dim(z.size(0)), K = op.dim(z.size(1));
    const float* lp = op.opt<float>(logits, "logits", NATURAL);
    int C = 1;
    if (present(logits)) {
        OP_CHECK(logits->dim() == 2 && logits->size(0) == z.size(0), "logits [M,C]");
        C = op.dim(logits->size(1));
    }
    const int md = clamped(mode);
    const auto dt = z.options().dtype(f64_out ? at::kDouble : at::kFloat);
    Tensor out = md == OSI_VIM_PROBS ? at::empty({(int64_t)M, (int64_t)C + 1}, dt) : at::empty({(int64_t)M}, dt);
    ok(osi_vim_scores(z.data_ptr<double>(), M, K, lp, C, alpha, md, f64_out ? nullptr : out.data_ptr<float>(),
                      f64_out ? out.data_ptr<double>() : nullptr, ws.ptr, ws.bytes, op.stream()), "osi_vim_scores");
    return out;
}

// ---- activation shaping (include/osi.h, ABI 27): the pooled activation, exact order statistics, shaped rows, logit scores
Tensor resnet50_pooled(int64_t net, const Tensor& workspace) {
    Op op("resnet50_pooled", workspace, at::kByte, "workspace");
    osi_resnet50_t h = handle(net);
    OP_CHECK((size_t)workspace.numel() >= osi_resnet50_workspace_bytes(h), "workspace too small");
    size_t floats = 0;
    ok(osi_resnet50_pooled(h, nullptr, nullptr, &floats, nullptr), "osi_resnet50_pooled");
    Tensor out = at::empty({(int64_t)(floats / 2048), 2048}, workspace.options().dtype(at::kFloat));
    ok(osi_resnet50_pooled(h, workspace.data_ptr(), out.data_ptr<float>(), &floats, op.stream()), "osi_resnet50_pooled");
    return out;
}

Tensor order_stats(const Tensor& v, at::IntArrayRef ranks, Tensor workspace) {
    Op op("order_stats", v, at::kFloat, "v", NATURAL);
    const Workspace ws = op.workspace(workspace, 8);
    OP_CHECK(v.numel() >= 1, "v is not empty");
    OP_CHECK(ranks.size() >= 1 && ranks.size() <= OSI_ORDER_STATS_MAX_R, "1 .. ", OSI_ORDER_STATS_MAX_R, " ranks");
    long long rk[OSI_ORDER_STATS_MAX_R];
    for (size_t r = 0; r < ranks.size(); ++r) {
        OP_CHECK(ranks[r] >= 0 && ranks[r] < v.numel(), "rank ", ranks[r], " outside [0, ", v.numel(), ")");
        rk[r] = (long long)ranks[r];
    }
    Tensor out = at::empty({(int64_t)ranks.size()}, v.options());
    ok(osi_order_stats_f32(v.data_ptr<float>(), (long long)v.numel(), rk, (int)ranks.size(), out.data_ptr<float>(), ws.ptr, ws.bytes,
                           op.stream()), "osi_order_stats_f32");
    return out;
}

Tensor shape_rows(const Tensor& x, int64_t mode, int64_t keep, double clip, Tensor workspace) {
    Op op("shape_rows", x, at::kFloat, "x", NATURAL);
    const Workspace ws = op.workspace(workspace, 8);
    OP_CHECK(x.dim() == 2, "x [M,F]");
    const int M = op.dim(x.size(0)), F = op.dim(x.size(1));
    Tensor out = at::empty_like(x);
    ok(osi_shape_rows(x.data_ptr<float>(), M, F, clamped(mode), clamped(keep), (float)clip, out.data_ptr<float>(), ws.ptr, ws.bytes,
                      op.stream()), "osi_shape_rows");
    return out;
}

Tensor logit_scores(const Tensor& logits, int64_t mode) {
    Op op("logit_scores", logits, at::kFloat, "logits", NATURAL);
    OP_CHECK(logits.dim() == 2, "logits [M,C]");
    const int M = op.dim(logits.size(0)), C = op.dim(logits.size(1));
    Tensor out = at::empty({(int64_t)M}, logits.options());
    ok(osi_logit_scores(logits.data_ptr<float>(), M, C, clamped(mode), out.data_ptr<float>(), op.stream()), "osi_logit_scores");
    return out;
}

// ---- gradient-based scores (include/osi.h, ABI 29): returns (dlogits [M,C] or empty, pred [M] int64, score [M])
std::tuple<Tensor, Tensor, Tensor> odin_head(const Tensor& logits, double temperature, bool need_grad) {
    Op op("odin_head", logits, at::kFloat, "logits", NATURAL);
    OP_CHECK(logits.dim() == 2, "logits [M,C]");
    const int M = op.dim(logits.size(0)), C = op.dim(logits.size(1));
    Tensor dlogits = need_grad ? at::empty_like(logits) : at::empty({0}, logits.options());
    Tensor pred = at::empty({(int64_t)M}, logits.options().dtype(at::kLong)), score = at::empty({(int64_t)M}, logits.options());
    ok(osi_odin_head(logits.data_ptr<float>(), M, C, (float)temperature, need_grad ? dlogits.data_ptr<float>() : nullptr, i64(pred),
                     score.data_ptr<float>(), op.stream()), "osi_odin_head");
    return {dlogits, pred, score};
}

Tensor gradnorm_scores(const Tensor& features, const Tensor& logits, double temperature) {
    Op op("gradnorm_scores", features, at::kFloat, "features", NATURAL);
    op.need(logits, at::kFloat, "logits", NATURAL);
    OP_CHECK(features.dim() == 2 && logits.dim() == 2, "features [M,F] and logits [M,C]");
    op.rows(features, logits);
    const int M = op.dim(features.size(0)), F = op.dim(features.size(1)), C = op.dim(logits.size(1));
    Tensor out = at::empty({(int64_t)M}, features.options());
    ok(osi_gradnorm_scores(features.data_ptr<float>(), logits.data_ptr<float>(), M, F, C, (float)temperature, out.data_ptr<float>(),
                           op.stream()), "osi_gradnorm_scores");
    return out;
}

// ---- PROSER (include/osi.h, ABI 23)
void need_pairs(const Op& op, const Tensor& partner, const Tensor& weight, int64_t B) {
    op.need(partner, at::kInt, "partner", NATURAL); op.need(weight, at::kFloat, "weight", NATURAL);
    OP_CHECK(partner.numel() == B && weight.numel() == B, "partner and weight hold one entry per row (", B, ")");
}

void mix_rows_pairs(Tensor x, const Tensor& partner, const Tensor& weight) {
    Op op("mix_rows_pairs", x, at::kFloat, "x");
    OP_CHECK(x.dim() >= 2 && x.size(0) <= INT_MAX && x.numel() > 0, "x is [B, ...] with at least one element");
    const int64_t B = x.size(0), L = x.numel() / B;
    OP_CHECK(L % 4 == 0, "the row length must be a multiple of 4, got ", L);
    need_pairs(op, partner, weight, B);
    ok(osi_mix_rows_pairs(x.data_ptr<float>(), partner.data_ptr<int>(), weight.data_ptr<float>(), (int)B, (size_t)L, op.stream()),
       "osi_mix_rows_pairs");
}

// the one-shot request of the executor's next differentiable forward; both tensors absent clears it. The caller keeps them alive until
// that forward has been enqueued (model.py holds them)
void resnet50_set_mix(int64_t net, const optional<Tensor>& partner, const optional<Tensor>& weight) {
    osi_resnet50_t h = handle(net);
    // checked before there is a tensor to build an Op on: the one message that spells the op's name itself
    TORCH_CHECK(present(partner) == present(weight), "osi::resnet50_set_mix: partner and weight go together");
    if (!present(partner)) { ok(osi_resnet50_set_mix(h, nullptr, nullptr), "osi_resnet50_set_mix"); return; }
    int B = 0;
    ok(osi_resnet50_geometry(h, &B, nullptr, nullptr), "osi_resnet50_geometry");
    Op op("resnet50_set_mix", *partner, at::kInt, "partner", NATURAL);
    need_pairs(op, *partner, *weight, B);
    ok(osi_resnet50_set_mix(h, partner->data_ptr<int>(), weight->data_ptr<float>()), "osi_resnet50_set_mix");
}

// returns (loss4 [4] = {J, mean t1, mean t2, mean t3}, dlogits [B,C] or empty, ddummy [B,D] or empty)
std::tuple<Tensor, Tensor, Tensor> proser_loss_fwd_bwd(const Tensor& logits, const Tensor& dummy, const Tensor& target, int64_t n_mixed,
                                                       double l0, double l1, double l2, bool need_grad) {
    Op op("proser_loss_fwd_bwd", logits, at::kFloat, "logits", NATURAL);
    op.need(dummy, at::kFloat, "dummy", NATURAL); op.need(target, at::kLong, "target", NATURAL);
    OP_CHECK(logits.dim() == 2 && dummy.dim() == 2 && target.dim() == 1 && dummy.size(0) == logits.size(0) && target.size(0) == logits.size(0),
             "expected logits [B, C], dummy [B, D] and target [B]");
    OP_CHECK(n_mixed >= 0 && n_mixed <= logits.size(0), "n_mixed outside [0, B]");
    const int B = op.size(logits.size(0)), C = op.size(logits.size(1)), D = op.size(dummy.size(1));
    Tensor loss4 = at::empty({4}, logits.options());
    Tensor dlogits = need_grad ? at::empty_like(logits) : at::empty({0}, logits.options());
    Tensor ddummy = need_grad ? at::empty_like(dummy) : at::empty({0}, logits.options());
    ok(osi_proser_loss_fwd_bwd(logits.data_ptr<float>(), dummy.data_ptr<float>(), i64(target), B, C, D, (int)n_mixed, (float)l0, (float)l1,
                               (float)l2, loss4.data_ptr<float>(), need_grad ? dlogits.data_ptr<float>() : nullptr,
                               need_grad ? ddummy.data_ptr<float>() : nullptr, op.stream()), "osi_proser_loss_fwd_bwd");
    return {loss4, dlogits, ddummy};
}

Tensor proser_scores(const Tensor& logits, const Tensor& dummy, double bias) {
    Op op("proser_scores", logits, at::kFloat, "logits", NATURAL);
    op.need(dummy, at::kFloat, "dummy", NATURAL);
    OP_CHECK(logits.dim() == 2 && dummy.dim() == 2 && dummy.size(0) == logits.size(0), "expected logits [B, C] and dummy [B, D]");
    OP_CHECK(logits.size(1) < INT_MAX, "sizes out of range");   // C + 1 columns
    const int B = op.size(logits.size(0)), C = (int)logits.size(1), D = op.size(dummy.size(1));
    Tensor probs = at::empty({logits.size(0), logits.size(1) + 1}, logits.options());
    ok(osi_proser_scores(logits.data_ptr<float>(), dummy.data_ptr<float>(), (float)bias, B, C, D, probs.data_ptr<float>(), op.stream()),
       "osi_proser_scores");
    return probs;
}

// the small dense layer of the package's own kernels (csrc/linear.hip) for layers outside the executor: y = x w^T + bias
Tensor linear_fwd(const Tensor& x, const Tensor& w, const optional<Tensor>& bias) {
    Op op("linear_fwd", x, at::kFloat, "x", NATURAL);
    op.need(w, at::kFloat, "w", NATURAL);
    OP_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(1), "x [B, K] and w [O, K]");
    const float* bp = op.opt<float>(bias, "bias", NATURAL, w.size(0));
    const int K = op.size(x.size(1));
    // the 16-byte loads of the K % 4 == 0 form need aligned rows
    OP_CHECK(K % 4 != 0 || ((reinterpret_cast<uintptr_t>(x.data_ptr()) | reinterpret_cast<uintptr_t>(w.data_ptr())) & 15) == 0,
             "x and w must be 16-byte aligned when K is a multiple of 4");
    Tensor y = at::empty({x.size(0), w.size(0)}, x.options());
    ok(osi_linear_fwd(x.data_ptr<float>(), w.data_ptr<float>(), bp, y.data_ptr<float>(), (int)x.size(0), K, (int)w.size(0), op.stream()),
       "osi_linear_fwd");
    return y;
}

// returns (dx [B,K] or empty, dw [O,K], db [O])
std::tuple<Tensor, Tensor, Tensor> linear_bwd(const Tensor& dy, const Tensor& x, const Tensor& w, bool need_dx) {
    Op op("linear_bwd", dy, at::kFloat, "dy", NATURAL);
    op.need(x, at::kFloat, "x", NATURAL); op.need(w, at::kFloat, "w", NATURAL);
    OP_CHECK(dy.dim() == 2 && x.dim() == 2 && w.dim() == 2 && dy.size(0) == x.size(0) && dy.size(1) == w.size(0) && x.size(1) == w.size(1),
             "dy [B, O], x [B, K] and w [O, K]");
    const int K = op.size(x.size(1));
    Tensor dx = need_dx ? at::empty_like(x) : at::empty({0}, x.options());
    Tensor dw = at::empty_like(w), db = at::empty({w.size(0)}, w.options());
    ok(osi_linear_bwd(dy.data_ptr<float>(), x.data_ptr<float>(), w.data_ptr<float>(), need_dx ? dx.data_ptr<float>() : nullptr, 0,
                      dw.data_ptr<float>(), db.data_ptr<float>(), (int)dy.size(0), K, (int)w.size(0), op.stream()), "osi_linear_bwd");
    return {dx, dw, db};
}

}  // namespace

TORCH_LIBRARY(osi, m) {
    m.def("mix_rows_pairs(Tensor(a!) x, Tensor partner, Tensor weight) -> ()");
    m.def("resnet50_set_mix(int net, Tensor? partner, Tensor? weight) -> ()", &resnet50_set_mix);   // both absent clears: no dispatch key
    m.def("proser_loss_fwd_bwd(Tensor logits, Tensor dummy, Tensor target, int n_mixed, float l0, float l1, float l2, bool need_grad) -> "
          "(Tensor, Tensor, Tensor)");
    m.def("proser_scores(Tensor logits, Tensor dummy, float bias) -> Tensor");
    m.def("linear_fwd(Tensor x, Tensor w, Tensor? bias) -> Tensor");
    m.def("linear_bwd(Tensor dy, Tensor x, Tensor w, bool need_dx) -> (Tensor, Tensor, Tensor)");
    m.def("evm_distances(Tensor a, Tensor b, int metric, Tensor(a!) workspace) -> Tensor");
    m.def("evm_fit_rows(Tensor dist, Tensor gt, int cls, int tailsize, float multiplier, Tensor(a!) workspace) -> "
          "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("evm_set_cover(Tensor dpp, Tensor shape, Tensor scale, Tensor shift, Tensor fitted, float multiplier, float cover_threshold, "
          "Tensor(a!) workspace) -> (Tensor, Tensor)");
    m.def("evm_probs(Tensor dist, Tensor shape, Tensor scale, Tensor shift, Tensor ev_start, float multiplier) -> Tensor");
    m.def("knn_topk(Tensor dist, int k, Tensor? skip, Tensor(a!) workspace) -> (Tensor, Tensor)");
    m.def("knn_class_kth(Tensor dist, Tensor start, int k, Tensor? skip, int transform, Tensor(a!) workspace) -> Tensor");
    m.def("maha_class_means(Tensor features, Tensor gt, int C, Tensor(a!) workspace) -> (Tensor, Tensor)");
    m.def("maha_scatter(Tensor features, Tensor gt, Tensor mean, int mode, bool accumulate, Tensor(a!) S, Tensor(b!) workspace) -> ()");
    m.def("maha_factor(Tensor S, float scale, float shrinkage, Tensor(a!) workspace) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("maha_whiten(Tensor x, Tensor W, Tensor(a!) workspace) -> Tensor");
    m.def("maha_sqdist(Tensor z, Tensor zm, Tensor? minus, int transform, bool f64_out, Tensor(a!) workspace) -> Tensor");
    m.def("eigh_begin(Tensor S, Tensor(a!) workspace) -> (Tensor, Tensor, Tensor, Tensor)");
    m.def("eigh_sweep(Tensor(a!) A, Tensor(b!) Vt, Tensor head, Tensor info, Tensor(c!) workspace) -> Tensor");
    m.def("eigh_finish(Tensor A, Tensor Vt, Tensor info, Tensor(a!) workspace) -> (Tensor, Tensor)");
    m.def("vim_project(Tensor x, Tensor origin, Tensor R, Tensor(a!) workspace) -> Tensor");
    m.def("vim_scores(Tensor z, Tensor? logits, float alpha, int mode, bool f64_out, Tensor(a!) workspace) -> Tensor");
    m.def("resnet50_pooled(int net, Tensor workspace) -> Tensor");
    m.def("order_stats(Tensor v, int[] ranks, Tensor(a!) workspace) -> Tensor");
    m.def("shape_rows(Tensor x, int mode, int keep, float clip, Tensor(a!) workspace) -> Tensor");
    m.def("logit_scores(Tensor logits, int mode) -> Tensor");
    m.def("odin_head(Tensor logits, float temperature, bool need_grad) -> (Tensor, Tensor, Tensor)");
    m.def("gradnorm_scores(Tensor features, Tensor logits, float temperature) -> Tensor");
    m.def("openmax_class_means(Tensor features, Tensor logits, Tensor gt, Tensor(a!) workspace) -> (Tensor, Tensor, Tensor)");
    m.def("openmax_distances(Tensor features, Tensor mav, Tensor? cls, int metric) -> Tensor");
    m.def("openmax_fit_tails(Tensor dist, Tensor gt, Tensor correct, int C, int tailsize, Tensor(a!) workspace) -> "
          "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)");
    m.def("openmax_wscores(Tensor dist, Tensor shape, Tensor scale, Tensor shift, Tensor fitted) -> Tensor");
    m.def("openmax_recalibrate(Tensor logits, Tensor w, int alpha) -> Tensor");
    m.def("resnet50_forward(int net, Tensor params, Tensor(a!) buffers, Tensor(b!) nbt, Tensor image, Tensor? flip, Tensor(c!) workspace, "
          "int fc_dim, int out_features, bool training) -> (Tensor, Tensor)");
    m.def("resnet50_forward_frozen(int net, Tensor params, Tensor buffers, Tensor image, Tensor? flip, Tensor(a!) workspace, "
          "int fc_dim, int out_features) -> (Tensor, Tensor)");
    m.def("resnet50_backward(int net, Tensor params, Tensor(a!) grads, Tensor(b!) workspace, Tensor dlogits, Tensor? dfeatures, "
          "int stage_lo, int stage_hi) -> ()");
    m.def("resnet50_backward_ex(int net, Tensor params, Tensor(a!) grads, Tensor(b!) workspace, Tensor dlogits, Tensor? dfeatures, "
          "Tensor(c!)? dimage, bool param_grads, int stage_lo, int stage_hi) -> ()");
    m.def("resnet50_backward_adv(int net, Tensor params, Tensor(a!) grads, Tensor(b!) workspace, Tensor dlogits, Tensor? dfeatures, "
          "Tensor(c!) x_adv, float eps, float lo, float hi, int stage_lo, int stage_hi) -> ()");
    m.def("resnet50_backward_attack(int net, Tensor params, Tensor(a!) grads, Tensor(b!) workspace, Tensor dlogits, Tensor? dfeatures, "
          "Tensor(c!) x_next, Tensor? x_anchor, float alpha, float eps, float lo, float hi, bool param_grads, int stage_lo, int stage_hi) -> ()");
    m.def("stem_dgrad_pgd(Tensor dy, Tensor w_krsc3, Tensor x_cur, Tensor x_anchor, Tensor(a!) x_next, float alpha, float eps, float lo, "
          "float hi) -> ()");
    m.def("grad_accumulate(Tensor(a!) dst, Tensor src) -> ()");
    m.def("resnet50_grads_ready(int net, Tensor grads, int waiter_stream) -> ()");
    m.def("average_update(Tensor(a!)[] avg, Tensor[] cur, float weight) -> ()");
    m.def("resnet50_set_bn_momentum(int net, float momentum) -> ()", &resnet50_set_bn_momentum);   // no tensor argument: no dispatch key
    m.def("loss_fwd_bwd(int mode, Tensor logits, Tensor target, float unk_weight, int ignore_index, Tensor? class_weights, "
          "Tensor? features, float xi, float alpha, bool need_grad) -> (Tensor, Tensor, Tensor)");
    m.def("adam_step(Tensor(a!) params, Tensor grads, Tensor(b!) exp_avg, Tensor(c!) exp_avg_sq, float lr, float beta1, float beta2, "
          "float eps, int step, float grad_scale) -> ()");
    m.def("sgd_step(Tensor(a!) params, Tensor grads, Tensor(b!) momentum_buffer, float lr, float momentum, bool first, float grad_scale) -> ()");
    m.def("adam_step_groups(Tensor(a!) params, Tensor grads, Tensor(b!) exp_avg, Tensor(c!) exp_avg_sq, Tensor(d!)? max_exp_avg_sq, "
          "int[] segments, float[] groups, float grad_scale) -> ()");
    m.def("sgd_step_groups(Tensor(a!) params, Tensor grads, Tensor(b!) momentum_buffer, int[] segments, float[] groups, float grad_scale) -> ()");
    m.def("adam_step_groups_dev(Tensor(a!) params, Tensor grads, Tensor(b!) exp_avg, Tensor(c!) exp_avg_sq, Tensor(d!)? max_exp_avg_sq, "
          "int[] segments, float[] groups, Tensor grad_scale) -> ()");
    m.def("sgd_step_groups_dev(Tensor(a!) params, Tensor grads, Tensor(b!) momentum_buffer, int[] segments, float[] groups, Tensor grad_scale) -> ()");
    m.def("grad_clip_scale(Tensor grads, int[] spans, int norm_type, float grad_scale, float max_norm, Tensor(a!) workspace, "
          "Tensor(b!) out2) -> ()");
    m.def("stage_canvas(Tensor canvas, Tensor? crop_xy, Tensor? flip, int H, int W) -> Tensor");   // crop corners are read-only (clamped in registers)
    m.def("softmax(Tensor logits) -> Tensor");
    m.def("confidence_accumulate(Tensor logits, Tensor target, float offset, int unknown_class, int last_valid_class, Tensor(a!) acc4) -> ()");
}

// The ops are MI355X-only: registered for the HIP device key (spelled CUDA in PyTorch-ROCm); a CPU tensor finds no kernel and raises.
TORCH_LIBRARY_IMPL(osi, CUDA, m) {
    m.impl("resnet50_forward", &resnet50_forward);
    m.impl("resnet50_forward_frozen", &resnet50_forward_frozen);
    m.impl("resnet50_backward", &resnet50_backward);
    m.impl("resnet50_backward_ex", &resnet50_backward_ex);
    m.impl("resnet50_backward_adv", &resnet50_backward_adv);
    m.impl("resnet50_backward_attack", &resnet50_backward_attack);
    m.impl("stem_dgrad_pgd", &stem_dgrad_pgd);
    m.impl("grad_accumulate", &grad_accumulate);
    m.impl("resnet50_grads_ready", &resnet50_grads_ready);
    m.impl("average_update", &average_update);
    m.impl("loss_fwd_bwd", &loss_fwd_bwd);
    m.impl("adam_step", &adam_step);
    m.impl("sgd_step", &sgd_step);
    m.impl("adam_step_groups", &adam_step_groups);
    m.impl("sgd_step_groups", &sgd_step_groups);
    m.impl("adam_step_groups_dev", &adam_step_groups_dev);
    m.impl("sgd_step_groups_dev", &sgd_step_groups_dev);
    m.impl("grad_clip_scale", &grad_clip_scale);
    m.impl("stage_canvas", &stage_canvas);
    m.impl("softmax", &softmax);
    m.impl("confidence_accumulate", &confidence_accumulate);
    m.impl("openmax_class_means", &openmax_class_means);
    m.impl("openmax_distances", &openmax_distances);
    m.impl("openmax_fit_tails", &openmax_fit_tails);
    m.impl("openmax_wscores", &openmax_wscores);
    m.impl("openmax_recalibrate", &openmax_recalibrate);
    m.impl("evm_distances", &evm_distances);
    m.impl("evm_fit_rows", &evm_fit_rows);
    m.impl("evm_set_cover", &evm_set_cover);
    m.impl("evm_probs", &evm_probs);
    m.impl("knn_topk", &knn_topk);
    m.impl("knn_class_kth", &knn_class_kth);
    m.impl("maha_class_means", &maha_class_means);
    m.impl("maha_scatter", &maha_scatter);
    m.impl("maha_factor", &maha_factor);
    m.impl("maha_whiten", &maha_whiten);
    m.impl("maha_sqdist", &maha_sqdist);
    m.impl("eigh_begin", &eigh_begin);
    m.impl("eigh_sweep", &eigh_sweep);
    m.impl("eigh_finish", &eigh_finish);
    m.impl("vim_project", &vim_project);
    m.impl("vim_scores", &vim_scores);
    m.impl("resnet50_pooled", &resnet50_pooled);
    m.impl("order_stats", &order_stats);
    m.impl("shape_rows", &shape_rows);
    m.impl("logit_scores", &logit_scores);
    m.impl("odin_head", &odin_head);
    m.impl("gradnorm_scores", &gradnorm_scores);
    m.impl("mix_rows_pairs", &mix_rows_pairs);
    m.impl("proser_loss_fwd_bwd", &proser_loss_fwd_bwd);
    m.impl("proser_scores", &proser_scores);
    m.impl("linear_fwd", &linear_fwd);
    m.impl("linear_bwd", &linear_bwd);
}
