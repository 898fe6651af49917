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
//   torch.ops.osi.mix_rows_pairs / resnet50_set_mix / proser_loss_fwd_bwd / proser_scores / linear_fwd / linear_bwd    PROSER (openset_imagenet/proser.py)
//
// This file contains no arithmetic: every op validates its tensor arguments (device, dtype, contiguity, sizes), takes the CURRENT
// HIP stream of the tensors' device inside the op, and forwards raw pointers to the C ABI of libosi_hip.so (include/osi.h), which
// stays the boundary a non-Python host binds. Tensor arguments keep their storage alive for the duration of the call and the
// dispatcher / profiler see the ops by name; stream and lifetime safety no longer depend on the caller passing data_ptr()s.
#include <torch/library.h>
#include <ATen/ATen.h>
// PyTorch-ROCm keeps the device type spelled "cuda"; these are its own HIP stream / guard classes for that spelling
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>

#include <optional>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/osi.h"

namespace {

using at::Tensor;

void ok(int code, const char* what) {
    TORCH_CHECK(code == OSI_OK, "libosi_hip ", what, " failed: ", osi_strerror(code), " (code ", code, ")");
}

// align = 16 for the tensors the kernels read with 16-byte vector accesses (the arenas, images, the workspace); the small per-row
// tensors (logits, targets, features, class weights, gradients of the head) are read element-wise and only need their natural
// alignment, so a contiguous row slice such as logits[3:] with an odd class count is accepted
void need(const Tensor& t, at::ScalarType dt, const char* name, uintptr_t align = 16) {
    TORCH_CHECK(t.defined(), name, ": undefined tensor");
    TORCH_CHECK(t.is_cuda(), "osi::", name, " must live on the GPU: the MI355X build has no CPU path");
    TORCH_CHECK(t.scalar_type() == dt, "osi::", name, " has dtype ", t.scalar_type(), ", expected ", dt);
    TORCH_CHECK(t.is_contiguous(), "osi::", name, " must be contiguous");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & (align - 1)) == 0, "osi::", name, " must be ", align, "-byte aligned");
}
constexpr uintptr_t NATURAL = 4;   // element-wise readers: fp32 / int64 / fp64 tensors from the allocator or row slices of them

osi_stream_t stream_of(const Tensor& t) {
    return (osi_stream_t)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream();
}

osi_resnet50_t handle(int64_t h) {
    TORCH_CHECK(h != 0, "osi: null executor handle");
    return reinterpret_cast<osi_resnet50_t>(static_cast<uintptr_t>(h));
}

const float* fptr(const std::optional<Tensor>& t) { return t.has_value() && t->defined() ? t->data_ptr<float>() : nullptr; }

// image: fp32 NCHW [B,3,H,W] (the reference's batch), fp32 NHWC4 [B,H,W,4] (bound in place) or uint8 [B,H,W,3] (+ flip flags)
// nbt == nullptr: the frozen-statistics forward (osi_resnet50_forward_frozen: buffers read-only, no num_batches_tracked)
std::tuple<Tensor, Tensor> forward_common(int64_t net, const Tensor& params, const Tensor& buffers, const Tensor* nbt_p, const Tensor& image,
                                          const std::optional<Tensor>& flip, Tensor workspace, int64_t fc_dim, int64_t out_features,
                                          bool training) {
    need(params, at::kFloat, "params"); need(buffers, at::kFloat, "buffers");
    if (nbt_p) need(*nbt_p, at::kLong, "num_batches_tracked");
    need(workspace, at::kByte, "workspace");
    TORCH_CHECK(image.dim() == 4, "osi::resnet50_forward: image must be 4-D");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
    osi_resnet50_t h = handle(net);
    TORCH_CHECK((size_t)workspace.numel() >= osi_resnet50_workspace_bytes(h), "osi::resnet50_forward: workspace too small");
    TORCH_CHECK((size_t)params.numel() == osi_resnet50_param_floats(h), "osi::resnet50_forward: parameter arena size mismatch");
    TORCH_CHECK((size_t)buffers.numel() == osi_resnet50_buffer_floats(h), "osi::resnet50_forward: buffer arena size mismatch");
    TORCH_CHECK(!nbt_p || nbt_p->numel() == osi_resnet50_num_bn(h), "osi::resnet50_forward: num_batches_tracked size mismatch");
    osi_stream_t st = stream_of(params);
    const int64_t B = image.size(0);
    {   // the executor was created for ONE geometry: a batch of another shape would read / write outside its workspace
        int eb = 0, eh = 0, ew = 0;
        ok(osi_resnet50_geometry(h, &eb, &eh, &ew), "osi_resnet50_geometry");
        const bool chw = image.scalar_type() != at::kByte && !(image.size(3) == 4 && image.size(1) != 3);
        const int64_t ih = chw ? image.size(2) : image.size(1), iw = chw ? image.size(3) : image.size(2);
        TORCH_CHECK(B == eb && ih == eh && iw == ew, "osi::resnet50_forward: image batch ", B, "x", ih, "x", iw,
                    " does not match the executor's geometry ", eb, "x", eh, "x", ew);
    }
    const float* img = nullptr;
    if (image.scalar_type() == at::kByte) {
        need(image, at::kByte, "image"); TORCH_CHECK(image.size(3) == 3, "uint8 image batch must be [B,H,W,3]");
        const unsigned char* fl = nullptr;
        if (flip.has_value() && flip->defined()) { need(*flip, at::kByte, "flip"); TORCH_CHECK(flip->numel() == B); fl = flip->data_ptr<unsigned char>(); }
        ok(osi_resnet50_stage_input_u8(h, image.data_ptr<unsigned char>(), fl, workspace.data_ptr(), st), "osi_resnet50_stage_input_u8");
    } else if (image.size(3) == 4 && image.size(1) != 3) {
        need(image, at::kFloat, "image");
        ok(osi_resnet50_bind_input_nhwc4(h, image.data_ptr<float>()), "osi_resnet50_bind_input_nhwc4");
    } else {
        need(image, at::kFloat, "image"); TORCH_CHECK(image.size(1) == 3, "fp32 image batch must be [B,3,H,W]");
        img = image.data_ptr<float>();
    }
    Tensor logits = at::empty({B, out_features}, params.options());
    Tensor features = at::empty({B, fc_dim}, params.options());
    if (nbt_p)
        ok(osi_resnet50_forward(h, params.data_ptr<float>(), buffers.data_ptr<float>(), (long long*)nbt_p->data_ptr<int64_t>(), img,
                                workspace.data_ptr(), logits.data_ptr<float>(), features.data_ptr<float>(), training ? 1 : 0, st),
           "osi_resnet50_forward");
    else
        ok(osi_resnet50_forward_frozen(h, params.data_ptr<float>(), buffers.data_ptr<float>(), img, workspace.data_ptr(),
                                       logits.data_ptr<float>(), features.data_ptr<float>(), st),
           "osi_resnet50_forward_frozen");
    return {logits, features};
}

std::tuple<Tensor, Tensor> resnet50_forward(int64_t net, const Tensor& params, Tensor buffers, Tensor nbt, const Tensor& image,
                                            const std::optional<Tensor>& flip, Tensor workspace, int64_t fc_dim, int64_t out_features,
                                            bool training) {
    return forward_common(net, params, buffers, &nbt, image, flip, workspace, fc_dim, out_features, training);
}

// ABI 12: the differentiable forward on frozen BatchNorm statistics (eval-mode gradients, freeze_bn()); the running statistics are read,
// never written, and the backward ops that follow run the frozen dataflow
std::tuple<Tensor, Tensor> resnet50_forward_frozen(int64_t net, const Tensor& params, const Tensor& buffers, const Tensor& image,
                                                   const std::optional<Tensor>& flip, Tensor workspace, int64_t fc_dim,
                                                   int64_t out_features) {
    return forward_common(net, params, buffers, nullptr, image, flip, workspace, fc_dim, out_features, false);
}

void resnet50_backward(int64_t net, const Tensor& params, Tensor grads, Tensor workspace, const Tensor& dlogits,
                       const std::optional<Tensor>& dfeatures, int64_t stage_lo, int64_t stage_hi) {
    need(params, at::kFloat, "params"); need(grads, at::kFloat, "grads"); need(workspace, at::kByte, "workspace");
    need(dlogits, at::kFloat, "dlogits", NATURAL);
    if (dfeatures.has_value() && dfeatures->defined()) need(*dfeatures, at::kFloat, "dfeatures", NATURAL);
    TORCH_CHECK(grads.numel() == params.numel(), "osi::resnet50_backward: gradient arena size mismatch");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
    ok(osi_resnet50_backward(handle(net), params.data_ptr<float>(), grads.data_ptr<float>(), workspace.data_ptr(),
                             dlogits.data_ptr<float>(), fptr(dfeatures), (int)stage_lo, (int)stage_hi, stream_of(params)),
       "osi_resnet50_backward");
}

// ABI 8: the same backward that can also write dJ/dimage (NCHW fp32 [B][3][H][W] of the executor's geometry) and/or skip every
// parameter gradient (param_grads = false: `grads` is not touched and may be an empty tensor)
void resnet50_backward_ex(int64_t net, const Tensor& params, Tensor grads, Tensor workspace, const Tensor& dlogits,
                          const std::optional<Tensor>& dfeatures, const std::optional<Tensor>& dimage, bool param_grads,
                          int64_t stage_lo, int64_t stage_hi) {
    need(params, at::kFloat, "params"); need(workspace, at::kByte, "workspace");
    need(dlogits, at::kFloat, "dlogits", NATURAL);
    if (dfeatures.has_value() && dfeatures->defined()) need(*dfeatures, at::kFloat, "dfeatures", NATURAL);
    if (param_grads) {
        need(grads, at::kFloat, "grads");
        TORCH_CHECK(grads.numel() == params.numel(), "osi::resnet50_backward_ex: gradient arena size mismatch");
    }
    const bool want_dx = dimage.has_value() && dimage->defined();
    TORCH_CHECK(want_dx || param_grads, "osi::resnet50_backward_ex: neither dimage nor parameter gradients requested");
    float* dx = nullptr;
    if (want_dx) {
        need(*dimage, at::kFloat, "dimage", NATURAL);
        TORCH_CHECK(dimage->device() == params.device(), "osi::resnet50_backward_ex: dimage lives on another device than params");
        int B = 0, H = 0, W = 0;
        ok(osi_resnet50_geometry(handle(net), &B, &H, &W), "osi_resnet50_geometry");
        TORCH_CHECK(dimage->dim() == 4 && dimage->size(0) == B && dimage->size(1) == 3 && dimage->size(2) == H && dimage->size(3) == W,
                    "osi::resnet50_backward_ex: dimage must be [", B, ", 3, ", H, ", ", W, "] (NCHW), got ", dimage->sizes());
        dx = dimage->data_ptr<float>();
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
    ok(osi_resnet50_backward_ex(handle(net), params.data_ptr<float>(), param_grads ? grads.data_ptr<float>() : nullptr, workspace.data_ptr(),
                                dlogits.data_ptr<float>(), fptr(dfeatures), dx, param_grads ? 1 : 0, (int)stage_lo, (int)stage_hi,
                                stream_of(params)),
       "osi_resnet50_backward_ex");
}

// ABI 10: the training backward whose last stage writes the FGSM batch x_adv = clamp(x + eps * sign(dJ/dimage), lo, hi) as NHWC4
// [B, H, W, 4] from the input the forward read (adversarial negatives, openset_imagenet/adversary.py)
void resnet50_backward_adv(int64_t net, const Tensor& params, Tensor grads, Tensor workspace, const Tensor& dlogits,
                           const std::optional<Tensor>& dfeatures, Tensor x_adv, double eps, double lo, double hi, int64_t stage_lo,
                           int64_t stage_hi) {
    need(params, at::kFloat, "params"); need(grads, at::kFloat, "grads"); need(workspace, at::kByte, "workspace");
    need(dlogits, at::kFloat, "dlogits", NATURAL); need(x_adv, at::kFloat, "x_adv");
    if (dfeatures.has_value() && dfeatures->defined()) need(*dfeatures, at::kFloat, "dfeatures", NATURAL);
    TORCH_CHECK(grads.numel() == params.numel(), "osi::resnet50_backward_adv: gradient arena size mismatch");
    TORCH_CHECK(x_adv.device() == params.device(), "osi::resnet50_backward_adv: x_adv lives on another device than params");
    int B = 0, H = 0, W = 0;
    ok(osi_resnet50_geometry(handle(net), &B, &H, &W), "osi_resnet50_geometry");
    TORCH_CHECK(x_adv.dim() == 4 && x_adv.size(0) == B && x_adv.size(1) == H && x_adv.size(2) == W && x_adv.size(3) == 4,
                "osi::resnet50_backward_adv: x_adv must be [", B, ", ", H, ", ", W, ", 4] (NHWC4), got ", x_adv.sizes());
    c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
    ok(osi_resnet50_backward_adv(handle(net), params.data_ptr<float>(), grads.data_ptr<float>(), workspace.data_ptr(),
                                 dlogits.data_ptr<float>(), fptr(dfeatures), x_adv.data_ptr<float>(), (float)eps, (float)lo, (float)hi,
                                 (int)stage_lo, (int)stage_hi, stream_of(params)),
       "osi_resnet50_backward_adv");
}

// ABI 19: a backward whose last launch is one projected attack step (osi_stem_dgrad_pgd) from the batch the forward read towards x_next,
// projected onto the eps-ball around x_anchor (None: around the forward's own batch). param_grads = false: input-only — `grads` is not
// touched and may be an empty tensor, nothing runs on the side stream (the inner steps of a PGD attack, attacks inside validate())
void resnet50_backward_attack(int64_t net, const Tensor& params, Tensor grads, Tensor workspace, const Tensor& dlogits,
                              const std::optional<Tensor>& dfeatures, Tensor x_next, const std::optional<Tensor>& x_anchor, double alpha,
                              double eps, double lo, double hi, bool param_grads, int64_t stage_lo, int64_t stage_hi) {
    need(params, at::kFloat, "params"); need(workspace, at::kByte, "workspace");
    need(dlogits, at::kFloat, "dlogits", NATURAL); need(x_next, at::kFloat, "x_next");
    if (dfeatures.has_value() && dfeatures->defined()) need(*dfeatures, at::kFloat, "dfeatures", NATURAL);
    if (param_grads) {
        need(grads, at::kFloat, "grads");
        TORCH_CHECK(grads.numel() == params.numel(), "osi::resnet50_backward_attack: gradient arena size mismatch");
    }
    TORCH_CHECK(x_next.device() == params.device(), "osi::resnet50_backward_attack: x_next lives on another device than params");
    int B = 0, H = 0, W = 0;
    ok(osi_resnet50_geometry(handle(net), &B, &H, &W), "osi_resnet50_geometry");
    TORCH_CHECK(x_next.dim() == 4 && x_next.size(0) == B && x_next.size(1) == H && x_next.size(2) == W && x_next.size(3) == 4,
                "osi::resnet50_backward_attack: x_next must be [", B, ", ", H, ", ", W, ", 4] (NHWC4), got ", x_next.sizes());
    osi_attack a{x_next.data_ptr<float>(), nullptr, (float)alpha, (float)eps, (float)lo, (float)hi};
    if (x_anchor.has_value() && x_anchor->defined()) {
        need(*x_anchor, at::kFloat, "x_anchor");
        TORCH_CHECK(x_anchor->device() == params.device(), "osi::resnet50_backward_attack: x_anchor lives on another device than params");
        TORCH_CHECK(x_anchor->sizes() == x_next.sizes(), "osi::resnet50_backward_attack: x_anchor must be [", B, ", ", H, ", ", W,
                    ", 4] (NHWC4), got ", x_anchor->sizes());
        a.x_anchor = x_anchor->data_ptr<float>();
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
    ok(osi_resnet50_backward_attack(handle(net), params.data_ptr<float>(), param_grads ? grads.data_ptr<float>() : nullptr,
                                    workspace.data_ptr(), dlogits.data_ptr<float>(), fptr(dfeatures), &a, param_grads ? 1 : 0, (int)stage_lo,
                                    (int)stage_hi, stream_of(params)),
       "osi_resnet50_backward_attack");
}

// ABI 19: the stem's input gradient ending in one projected attack step, on its own (dy [B, Hs, Ws, 64] NHWC, w [64, 7, 7, 3] storage
// order, three NHWC4 batches of one shape); returns nothing, x_next is written
void stem_dgrad_pgd(const Tensor& dy, const Tensor& w_krsc3, const Tensor& x_cur, const Tensor& x_anchor, Tensor x_next, double alpha,
                    double eps, double lo, double hi) {
    need(dy, at::kFloat, "dy"); need(w_krsc3, at::kFloat, "w_krsc3", NATURAL);
    need(x_cur, at::kFloat, "x_cur"); need(x_anchor, at::kFloat, "x_anchor"); need(x_next, at::kFloat, "x_next");
    TORCH_CHECK(x_cur.dim() == 4 && x_cur.size(3) == 4, "osi::stem_dgrad_pgd: x_cur must be [B, H, W, 4] (NHWC4), got ", x_cur.sizes());
    TORCH_CHECK(x_anchor.sizes() == x_cur.sizes() && x_next.sizes() == x_cur.sizes(), "osi::stem_dgrad_pgd: the three batches differ in shape");
    TORCH_CHECK(dy.device() == x_cur.device() && w_krsc3.device() == x_cur.device() && x_anchor.device() == x_cur.device() &&
                x_next.device() == x_cur.device(), "osi::stem_dgrad_pgd: tensors live on different devices");
    const int64_t B = x_cur.size(0), H = x_cur.size(1), W = x_cur.size(2);
    TORCH_CHECK(dy.dim() == 4 && dy.size(0) == B && dy.size(1) == (H - 1) / 2 + 1 && dy.size(2) == (W - 1) / 2 + 1 && dy.size(3) == 64,
                "osi::stem_dgrad_pgd: dy must be [", B, ", ", (H - 1) / 2 + 1, ", ", (W - 1) / 2 + 1, ", 64] (NHWC), got ", dy.sizes());
    TORCH_CHECK(w_krsc3.numel() == 64 * 7 * 7 * 3, "osi::stem_dgrad_pgd: w_krsc3 must hold 64 x 7 x 7 x 3 floats");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x_cur.device());
    ok(osi_stem_dgrad_pgd(dy.data_ptr<float>(), w_krsc3.data_ptr<float>(), x_cur.data_ptr<float>(), x_anchor.data_ptr<float>(),
                          x_next.data_ptr<float>(), (float)alpha, (float)eps, (float)lo, (float)hi, (int)B, (int)H, (int)W, stream_of(x_cur)),
       "osi_stem_dgrad_pgd");
}

// dst += src over two gradient arenas of the same length
void grad_accumulate(Tensor dst, const Tensor& src) {
    need(dst, at::kFloat, "dst"); need(src, at::kFloat, "src");
    TORCH_CHECK(dst.numel() == src.numel() && dst.device() == src.device(), "osi::grad_accumulate: arenas differ in size or device");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dst.device());
    ok(osi_grad_accumulate(dst.data_ptr<float>(), src.data_ptr<float>(), (size_t)dst.numel(), stream_of(dst)), "osi_grad_accumulate");
}

// ABI 20: avg[i] = lerp(avg[i], cur[i], weight) over 1 .. OSI_AVG_MAX_SPANS pairs of contiguous fp32 tensors in ONE launch (EMA / SWA of
// the parameter and buffer arenas, openset_imagenet/averaging.py); overlaps and the weight are validated by the C ABI
void average_update(at::TensorList avg, at::TensorList cur, double weight) {
    TORCH_CHECK(!avg.empty() && avg.size() <= OSI_AVG_MAX_SPANS && cur.size() == avg.size(), "osi::average_update: 1 .. ",
                OSI_AVG_MAX_SPANS, " tensors in each list, as many current as averaged ones");
    osi_avg_span spans[OSI_AVG_MAX_SPANS];
    for (size_t i = 0; i < avg.size(); ++i) {
        need(avg[i], at::kFloat, "avg"); need(cur[i], at::kFloat, "cur");
        TORCH_CHECK(avg[i].numel() == cur[i].numel() && avg[i].device() == avg[0].device() && cur[i].device() == avg[0].device(),
                    "osi::average_update: pair ", i, " differs in size or lives on another device");
        spans[i] = osi_avg_span{avg[i].data_ptr<float>(), cur[i].data_ptr<float>(), (size_t)avg[i].numel()};
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(avg[0].device());
    ok(osi_average_update(spans, (int)avg.size(), (float)weight, stream_of(avg[0])), "osi_average_update");
}

// ABI 20: the executor's running-statistics update factor, in force from its next training-mode forward (no tensor: a host setting)
void resnet50_set_bn_momentum(int64_t net, double momentum) {
    ok(osi_resnet50_set_bn_momentum(handle(net), (float)momentum), "osi_resnet50_set_bn_momentum");
}

// Data parallel: the stream `waiter` (a raw hipStream_t handle: torch.cuda.Stream.cuda_stream of the communication stream) waits for the
// gradients of the backward stages enqueued so far on the CURRENT stream and on the executor's side stream; the current stream waits for nothing
void resnet50_grads_ready(int64_t net, const Tensor& grads, int64_t waiter) {
    need(grads, at::kFloat, "grads");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(grads.device());
    ok(osi_resnet50_grads_ready(handle(net), stream_of(grads), reinterpret_cast<osi_stream_t>(static_cast<uintptr_t>(waiter))),
       "osi_resnet50_grads_ready");
}

// returns (loss [], dlogits [B,C] or empty, dfeatures [B,F] or empty)
std::tuple<Tensor, Tensor, Tensor> loss_fwd_bwd(int64_t mode, const Tensor& logits, const Tensor& target, double unk_weight,
                                                int64_t ignore_index, const std::optional<Tensor>& class_weights,
                                                const std::optional<Tensor>& features, double xi, double alpha, bool need_grad) {
    need(logits, at::kFloat, "logits", NATURAL); need(target, at::kLong, "target", NATURAL);
    TORCH_CHECK(logits.dim() == 2 && target.dim() == 1 && target.size(0) == logits.size(0), "expected logits [B, C] and target [B]");
    const int B = (int)logits.size(0), C = (int)logits.size(1);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
    Tensor loss = at::empty({}, logits.options());
    Tensor dlogits = need_grad ? at::empty_like(logits) : at::empty({0}, logits.options());
    Tensor dfeat = at::empty({0}, logits.options());
    int F = 0;
    if (class_weights.has_value() && class_weights->defined()) { need(*class_weights, at::kFloat, "class_weights", NATURAL); TORCH_CHECK(class_weights->numel() == C); }
    if (features.has_value() && features->defined()) {
        need(*features, at::kFloat, "features", NATURAL); TORCH_CHECK(features->dim() == 2 && features->size(0) == B);
        F = (int)features->size(1);
        dfeat = at::empty_like(*features);
    }
    ok(osi_loss_fwd_bwd((int)mode, logits.data_ptr<float>(), (const long long*)target.data_ptr<int64_t>(), B, C, (float)unk_weight,
                        (long long)ignore_index, fptr(class_weights), fptr(features), F, (float)xi, (float)alpha, loss.data_ptr<float>(),
                        need_grad ? dlogits.data_ptr<float>() : nullptr, F ? dfeat.data_ptr<float>() : nullptr, stream_of(logits)),
       "osi_loss_fwd_bwd");
    return {loss, dlogits, dfeat};
}

void adam_step(Tensor params, const Tensor& grads, Tensor exp_avg, Tensor exp_avg_sq, double lr, double beta1, double beta2, double eps,
               int64_t step, double grad_scale) {
    need(params, at::kFloat, "params"); need(grads, at::kFloat, "grads"); need(exp_avg, at::kFloat, "exp_avg"); need(exp_avg_sq, at::kFloat, "exp_avg_sq");
    TORCH_CHECK(grads.numel() == params.numel() && exp_avg.numel() == params.numel() && exp_avg_sq.numel() == params.numel());
    c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
    ok(osi_adam_step(params.data_ptr<float>(), grads.data_ptr<float>(), exp_avg.data_ptr<float>(), exp_avg_sq.data_ptr<float>(),
                     (size_t)params.numel(), lr, beta1, beta2, eps, (long long)step, (float)grad_scale, stream_of(params)), "osi_adam_step");
}

void sgd_step(Tensor params, const Tensor& grads, Tensor momentum_buffer, double lr, double momentum, bool first, double grad_scale) {
    need(params, at::kFloat, "params"); need(grads, at::kFloat, "grads"); need(momentum_buffer, at::kFloat, "momentum_buffer");
    TORCH_CHECK(grads.numel() == params.numel() && momentum_buffer.numel() == params.numel());
    c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
    ok(osi_sgd_step(params.data_ptr<float>(), grads.data_ptr<float>(), momentum_buffer.data_ptr<float>(), (size_t)params.numel(),
                    (float)lr, (float)momentum, first ? 1 : 0, (float)grad_scale, stream_of(params)), "osi_sgd_step");
}

// segments: flat (begin4, end4, group) triples; the group tables are flat rows of doubles in the field order of osi_adam_group /
// osi_sgd_group. Everything else is validated by the C ABI.
std::vector<osi_opt_segment> opt_segments(c10::ArrayRef<int64_t> segments) {
    TORCH_CHECK(segments.size() % 3 == 0, "segments: flat (begin4, end4, group) triples");
    std::vector<osi_opt_segment> seg(segments.size() / 3);
    for (size_t i = 0; i < seg.size(); ++i) {
        for (int j = 0; j < 2; ++j)
            TORCH_CHECK(segments[3 * i + j] >= 0 && segments[3 * i + j] <= 0xFFFFFFFFll, "segment bounds out of range");
        TORCH_CHECK(segments[3 * i + 2] >= 0 && segments[3 * i + 2] < OSI_OPT_MAX_GROUPS, "segment group index out of range");
        seg[i] = osi_opt_segment{(unsigned)segments[3 * i], (unsigned)segments[3 * i + 1], (int)segments[3 * i + 2]};
    }
    return seg;
}

// grad_scale_dev == nullptr: the scalar by value (osi_adam_step_groups); else the kernel reads it from device memory (_dev)
void adam_groups_common(Tensor& params, const Tensor& grads, Tensor& exp_avg, Tensor& exp_avg_sq, const std::optional<Tensor>& max_exp_avg_sq,
                        c10::ArrayRef<int64_t> segments, c10::ArrayRef<double> groups, double grad_scale, const Tensor* grad_scale_dev) {
    need(params, at::kFloat, "params"); need(grads, at::kFloat, "grads"); need(exp_avg, at::kFloat, "exp_avg"); need(exp_avg_sq, at::kFloat, "exp_avg_sq");
    TORCH_CHECK(grads.numel() == params.numel() && exp_avg.numel() == params.numel() && exp_avg_sq.numel() == params.numel());
    float* vmax = nullptr;
    if (max_exp_avg_sq.has_value() && max_exp_avg_sq->defined()) {
        need(*max_exp_avg_sq, at::kFloat, "max_exp_avg_sq");
        TORCH_CHECK(max_exp_avg_sq->numel() == params.numel());
        vmax = max_exp_avg_sq->data_ptr<float>();
    }
    TORCH_CHECK(groups.size() % 9 == 0, "groups: rows of (lr, beta1, beta2, eps, weight_decay, step, decoupled, amsgrad, maximize)");
    const std::vector<osi_opt_segment> seg = opt_segments(segments);
    std::vector<osi_adam_group> gs(groups.size() / 9);
    for (size_t i = 0; i < gs.size(); ++i) {
        const double* r = &groups[9 * i];
        gs[i] = osi_adam_group{r[0], r[1], r[2], r[3], r[4], (long long)r[5], r[6] != 0.0, r[7] != 0.0, r[8] != 0.0};
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
    if (grad_scale_dev)
        ok(osi_adam_step_groups_dev(params.data_ptr<float>(), grads.data_ptr<float>(), exp_avg.data_ptr<float>(), exp_avg_sq.data_ptr<float>(),
                                    vmax, (size_t)params.numel(), seg.data(), (int)seg.size(), gs.data(), (int)gs.size(),
                                    grad_scale_dev->data_ptr<float>(), stream_of(params)), "osi_adam_step_groups_dev");
    else
        ok(osi_adam_step_groups(params.data_ptr<float>(), grads.data_ptr<float>(), exp_avg.data_ptr<float>(), exp_avg_sq.data_ptr<float>(), vmax,
                                (size_t)params.numel(), seg.data(), (int)seg.size(), gs.data(), (int)gs.size(), (float)grad_scale,
                                stream_of(params)), "osi_adam_step_groups");
}

void sgd_groups_common(Tensor& params, const Tensor& grads, Tensor& momentum_buffer, c10::ArrayRef<int64_t> segments,
                       c10::ArrayRef<double> groups, double grad_scale, const Tensor* grad_scale_dev) {
    need(params, at::kFloat, "params"); need(grads, at::kFloat, "grads"); need(momentum_buffer, at::kFloat, "momentum_buffer");
    TORCH_CHECK(grads.numel() == params.numel() && momentum_buffer.numel() == params.numel());
    TORCH_CHECK(groups.size() % 7 == 0, "groups: rows of (lr, momentum, dampening, weight_decay, nesterov, first_step, maximize)");
    const std::vector<osi_opt_segment> seg = opt_segments(segments);
    std::vector<osi_sgd_group> gs(groups.size() / 7);
    for (size_t i = 0; i < gs.size(); ++i) {
        const double* r = &groups[7 * i];
        gs[i] = osi_sgd_group{r[0], r[1], r[2], r[3], r[4] != 0.0, r[5] != 0.0, r[6] != 0.0};
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(params.device());
    if (grad_scale_dev)
        ok(osi_sgd_step_groups_dev(params.data_ptr<float>(), grads.data_ptr<float>(), momentum_buffer.data_ptr<float>(), (size_t)params.numel(),
                                   seg.data(), (int)seg.size(), gs.data(), (int)gs.size(), grad_scale_dev->data_ptr<float>(),
                                   stream_of(params)), "osi_sgd_step_groups_dev");
    else
        ok(osi_sgd_step_groups(params.data_ptr<float>(), grads.data_ptr<float>(), momentum_buffer.data_ptr<float>(), (size_t)params.numel(),
                               seg.data(), (int)seg.size(), gs.data(), (int)gs.size(), (float)grad_scale, stream_of(params)),
           "osi_sgd_step_groups");
}

void adam_step_groups(Tensor params, const Tensor& grads, Tensor exp_avg, Tensor exp_avg_sq, const std::optional<Tensor>& max_exp_avg_sq,
                      c10::ArrayRef<int64_t> segments, c10::ArrayRef<double> groups, double grad_scale) {
    adam_groups_common(params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, segments, groups, grad_scale, nullptr);
}

void sgd_step_groups(Tensor params, const Tensor& grads, Tensor momentum_buffer, c10::ArrayRef<int64_t> segments,
                     c10::ArrayRef<double> groups, double grad_scale) {
    sgd_groups_common(params, grads, momentum_buffer, segments, groups, grad_scale, nullptr);
}

// the scalar of a *_dev step: one fp32 element on the arena's device (e.g. the second element of grad_clip_scale's out2)
void need_scalar(const Tensor& s, const Tensor& params) {
    need(s, at::kFloat, "grad_scale", NATURAL);
    TORCH_CHECK(s.numel() == 1 && s.device() == params.device(), "osi: grad_scale must be one fp32 element on the arena's device");
}

void adam_step_groups_dev(Tensor params, const Tensor& grads, Tensor exp_avg, Tensor exp_avg_sq, const std::optional<Tensor>& max_exp_avg_sq,
                          c10::ArrayRef<int64_t> segments, c10::ArrayRef<double> groups, const Tensor& grad_scale) {
    need_scalar(grad_scale, params);
    adam_groups_common(params, grads, exp_avg, exp_avg_sq, max_exp_avg_sq, segments, groups, 0.0, &grad_scale);
}

void sgd_step_groups_dev(Tensor params, const Tensor& grads, Tensor momentum_buffer, c10::ArrayRef<int64_t> segments,
                         c10::ArrayRef<double> groups, const Tensor& grad_scale) {
    need_scalar(grad_scale, params);
    sgd_groups_common(params, grads, momentum_buffer, segments, groups, 0.0, &grad_scale);
}

// spans: flat (begin, numel) pairs in floats, empty = the whole arena. out2 <- (norm of grad_scale * g over the spans, the scalar a
// clipped step multiplies the gradients by); nothing is read back. Everything else is validated by the C ABI.
void grad_clip_scale(const Tensor& grads, c10::ArrayRef<int64_t> spans, int64_t norm_type, double grad_scale, double max_norm,
                     Tensor workspace, Tensor out2) {
    need(grads, at::kFloat, "grads"); need(workspace, at::kByte, "workspace"); need(out2, at::kFloat, "out2", NATURAL);
    TORCH_CHECK(out2.numel() == 2, "osi::grad_clip_scale: out2 holds two floats (norm, scalar)");
    TORCH_CHECK(workspace.device() == grads.device() && out2.device() == grads.device(), "osi::grad_clip_scale: tensors on different devices");
    TORCH_CHECK((size_t)workspace.numel() >= osi_grad_norm_workspace((size_t)grads.numel()), "osi::grad_clip_scale: workspace too small");
    TORCH_CHECK(spans.size() % 2 == 0, "spans: flat (begin, numel) pairs");
    std::vector<osi_grad_span> sp(spans.size() / 2);
    for (size_t i = 0; i < sp.size(); ++i) {
        TORCH_CHECK(spans[2 * i] >= 0 && spans[2 * i + 1] >= 0, "span bounds out of range");
        sp[i] = osi_grad_span{(unsigned long long)spans[2 * i], (unsigned long long)spans[2 * i + 1]};
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(grads.device());
    ok(osi_grad_clip_scale(grads.data_ptr<float>(), (size_t)grads.numel(), sp.empty() ? nullptr : sp.data(), (int)sp.size(), (int)norm_type,
                           (float)grad_scale, (float)max_norm, workspace.data_ptr(), (size_t)workspace.numel(), out2.data_ptr<float>(),
                           stream_of(grads)), "osi_grad_clip_scale");
}

Tensor stage_canvas(const Tensor& canvas, const std::optional<Tensor>& crop_xy, const std::optional<Tensor>& flip, int64_t H, int64_t W) {
    need(canvas, at::kByte, "canvas");
    TORCH_CHECK(canvas.dim() == 4 && canvas.size(3) == 3, "canvas must be uint8 [B,Hc,Wc,3]");
    const int B = (int)canvas.size(0);
    const int* cp = nullptr; const unsigned char* fl = nullptr;
    if (crop_xy.has_value() && crop_xy->defined()) { need(*crop_xy, at::kInt, "crop_xy", NATURAL); TORCH_CHECK(crop_xy->numel() == 2 * B); cp = crop_xy->data_ptr<int>(); }
    if (flip.has_value() && flip->defined()) { need(*flip, at::kByte, "flip", 1); TORCH_CHECK(flip->numel() == B); fl = flip->data_ptr<unsigned char>(); }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(canvas.device());
    Tensor out = at::empty({B, H, W, 4}, canvas.options().dtype(at::kFloat));
    ok(osi_u8_crop_flip_to_nhwc4(canvas.data_ptr<unsigned char>(), cp, fl, out.data_ptr<float>(), B, (int)canvas.size(1), (int)canvas.size(2),
                                 (int)H, (int)W, stream_of(canvas)), "osi_u8_crop_flip_to_nhwc4");
    return out;
}

Tensor softmax(const Tensor& logits) {
    need(logits, at::kFloat, "logits", NATURAL); TORCH_CHECK(logits.dim() == 2);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
    Tensor out = at::empty_like(logits);
    ok(osi_softmax(logits.data_ptr<float>(), out.data_ptr<float>(), (int)logits.size(0), (int)logits.size(1), stream_of(logits)), "osi_softmax");
    return out;
}

void confidence_accumulate(const Tensor& logits, const Tensor& target, double offset, int64_t unknown_class, int64_t last_valid_class,
                           Tensor acc4) {
    need(logits, at::kFloat, "logits", NATURAL); need(target, at::kLong, "target", NATURAL); need(acc4, at::kDouble, "acc4", NATURAL);
    TORCH_CHECK(logits.dim() == 2 && target.numel() == logits.size(0) && acc4.numel() == 4);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
    ok(osi_confidence_accumulate(logits.data_ptr<float>(), (const long long*)target.data_ptr<int64_t>(), (int)logits.size(0),
                                 (int)logits.size(1), (float)offset, (long long)unknown_class, (int)last_valid_class,
                                 acc4.data_ptr<double>(), stream_of(logits)), "osi_confidence_accumulate");
}

// ---- OpenMax (include/osi.h, ABI 21): every op allocates its outputs and leaves them on the device
void openmax_rows(const Tensor& a, const Tensor& b, const char* what) {
    TORCH_CHECK(a.device() == b.device(), "osi::", what, ": tensors on different devices");
    TORCH_CHECK(a.size(0) == b.size(0), "osi::", what, ": tensors disagree on the number of rows");
}

std::tuple<Tensor, Tensor, Tensor> openmax_class_means(const Tensor& features, const Tensor& logits, const Tensor& gt, Tensor workspace) {
    need(features, at::kFloat, "features", NATURAL); need(logits, at::kFloat, "logits", NATURAL); need(gt, at::kLong, "gt", NATURAL);
    need(workspace, at::kByte, "workspace", NATURAL);
    TORCH_CHECK(features.dim() == 2 && logits.dim() == 2 && gt.dim() == 1, "osi::openmax_class_means: features [N,F], logits [N,C], gt [N]");
    openmax_rows(features, logits, "openmax_class_means"); openmax_rows(features, gt, "openmax_class_means");
    const int N = (int)features.size(0), F = (int)features.size(1), C = (int)logits.size(1);
    TORCH_CHECK(workspace.device() == features.device() && (size_t)workspace.numel() >= osi_openmax_workspace(N, C, F),
                "osi::openmax_class_means: workspace too small");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(features.device());
    Tensor mav = at::empty({C, F}, features.options());
    Tensor count = at::empty({C}, features.options().dtype(at::kLong));
    Tensor correct = at::empty({N}, features.options().dtype(at::kByte));
    ok(osi_openmax_class_means(features.data_ptr<float>(), logits.data_ptr<float>(), (const long long*)gt.data_ptr<int64_t>(), N, C, F,
                               mav.data_ptr<float>(), (long long*)count.data_ptr<int64_t>(), correct.data_ptr<unsigned char>(),
                               workspace.data_ptr(), (size_t)workspace.numel(), stream_of(features)), "osi_openmax_class_means");
    return {mav, count, correct};
}

Tensor openmax_distances(const Tensor& features, const Tensor& mav, const std::optional<Tensor>& cls, int64_t metric) {
    need(features, at::kFloat, "features", NATURAL); need(mav, at::kFloat, "mav", NATURAL);
    TORCH_CHECK(features.dim() == 2 && mav.dim() == 2 && features.size(1) == mav.size(1) && mav.device() == features.device(),
                "osi::openmax_distances: features [N,F] and mav [C,F] on one device");
    const int N = (int)features.size(0), F = (int)features.size(1), C = (int)mav.size(0);
    const long long* cp = nullptr;
    if (cls.has_value() && cls->defined()) {
        need(*cls, at::kLong, "cls", NATURAL);
        TORCH_CHECK(cls->dim() == 1, "osi::openmax_distances: cls is [N]");
        openmax_rows(features, *cls, "openmax_distances");
        cp = (const long long*)cls->data_ptr<int64_t>();
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(features.device());
    Tensor dist = cp ? at::empty({N}, features.options()) : at::empty({N, C}, features.options());
    ok(osi_openmax_distances(features.data_ptr<float>(), mav.data_ptr<float>(), cp, N, C, F, (int)metric, dist.data_ptr<float>(),
                             stream_of(features)), "osi_openmax_distances");
    return dist;
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> openmax_fit_tails(const Tensor& dist, const Tensor& gt, const Tensor& correct,
                                                                             int64_t C, int64_t tailsize, Tensor workspace) {
    need(dist, at::kFloat, "dist", NATURAL); need(gt, at::kLong, "gt", NATURAL); need(correct, at::kByte, "correct", 1);
    need(workspace, at::kByte, "workspace", NATURAL);
    TORCH_CHECK(dist.dim() == 1 && gt.dim() == 1 && correct.dim() == 1, "osi::openmax_fit_tails: dist, gt and correct are [N]");
    openmax_rows(dist, gt, "openmax_fit_tails"); openmax_rows(dist, correct, "openmax_fit_tails");
    TORCH_CHECK(C > 0 && C <= INT_MAX, "osi::openmax_fit_tails: C out of range");
    const int N = (int)dist.size(0);
    TORCH_CHECK(workspace.device() == dist.device() && (size_t)workspace.numel() >= osi_openmax_workspace(N, (int)C, 1),
                "osi::openmax_fit_tails: workspace too small");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dist.device());
    const auto f64 = dist.options().dtype(at::kDouble), i64 = dist.options().dtype(at::kLong);
    Tensor shape = at::empty({C}, f64), scale = at::empty({C}, f64), shift = at::empty({C}, f64);
    Tensor fitted = at::empty({C}, dist.options().dtype(at::kByte)), tail_count = at::empty({C}, i64), flags2 = at::empty({2}, i64);
    ok(osi_openmax_fit_tails(dist.data_ptr<float>(), (const long long*)gt.data_ptr<int64_t>(), correct.data_ptr<unsigned char>(), N, (int)C,
                             (int)tailsize, shape.data_ptr<double>(), scale.data_ptr<double>(), shift.data_ptr<double>(),
                             fitted.data_ptr<unsigned char>(), (long long*)tail_count.data_ptr<int64_t>(),
                             (long long*)flags2.data_ptr<int64_t>(), workspace.data_ptr(), (size_t)workspace.numel(), stream_of(dist)),
       "osi_openmax_fit_tails");
    return {shape, scale, shift, fitted, tail_count, flags2};
}

Tensor openmax_wscores(const Tensor& dist, const Tensor& shape, const Tensor& scale, const Tensor& shift, const Tensor& fitted) {
    need(dist, at::kFloat, "dist", NATURAL); need(shape, at::kDouble, "shape", NATURAL); need(scale, at::kDouble, "scale", NATURAL);
    need(shift, at::kDouble, "shift", NATURAL); need(fitted, at::kByte, "fitted", 1);
    TORCH_CHECK(dist.dim() == 2, "osi::openmax_wscores: dist is [N,C]");
    const int64_t C = dist.size(1);
    TORCH_CHECK(shape.numel() == C && scale.numel() == C && shift.numel() == C && fitted.numel() == C,
                "osi::openmax_wscores: shape, scale, shift and fitted hold one entry per column of dist");
    TORCH_CHECK(shape.device() == dist.device() && scale.device() == dist.device() && shift.device() == dist.device() &&
                fitted.device() == dist.device(), "osi::openmax_wscores: tensors on different devices");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dist.device());
    Tensor w = at::empty_like(dist);
    ok(osi_openmax_wscores(dist.data_ptr<float>(), (int)dist.size(0), (int)C, shape.data_ptr<double>(), scale.data_ptr<double>(),
                           shift.data_ptr<double>(), fitted.data_ptr<unsigned char>(), w.data_ptr<float>(), stream_of(dist)),
       "osi_openmax_wscores");
    return w;
}

Tensor openmax_recalibrate(const Tensor& logits, const Tensor& w, int64_t alpha) {
    need(logits, at::kFloat, "logits", NATURAL); need(w, at::kFloat, "w", NATURAL);
    TORCH_CHECK(logits.dim() == 2 && w.sizes() == logits.sizes() && w.device() == logits.device(),
                "osi::openmax_recalibrate: logits and w are [N,C] on one device");
    TORCH_CHECK(alpha >= 1, "osi::openmax_recalibrate: alpha must be >= 1");
    const int N = (int)logits.size(0), C = (int)logits.size(1);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
    Tensor probs = at::empty({N, C + 1}, logits.options());
    ok(osi_openmax_recalibrate(logits.data_ptr<float>(), w.data_ptr<float>(), N, C, (int)std::min<int64_t>(alpha, INT_MAX),
                               probs.data_ptr<float>(), stream_of(logits)), "osi_openmax_recalibrate");
    return probs;
}

// ---- Extreme Value Machine (include/osi.h, ABI 22): every op allocates its outputs and leaves them on the device
Tensor evm_distances(const Tensor& a, const Tensor& b, int64_t metric, Tensor workspace) {
    need(a, at::kFloat, "a", NATURAL); need(b, at::kFloat, "b", NATURAL); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(1) && a.device() == b.device() && workspace.device() == a.device(),
                "osi::evm_distances: a [R,F] and b [N,F] on one device");
    TORCH_CHECK(a.size(0) <= INT_MAX && b.size(0) <= INT_MAX && a.size(1) <= INT_MAX, "osi::evm_distances: sizes out of range");
    const int R = (int)a.size(0), N = (int)b.size(0), F = (int)a.size(1);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(a.device());
    Tensor dist = at::empty({R, N}, a.options());
    ok(osi_evm_distances(a.data_ptr<float>(), R, b.data_ptr<float>(), N, F, (int)metric, dist.data_ptr<float>(), workspace.data_ptr(),
                         (size_t)workspace.numel(), stream_of(a)), "osi_evm_distances");
    return dist;
}

std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor, Tensor> evm_fit_rows(const Tensor& dist, const Tensor& gt, int64_t cls, int64_t tailsize,
                                                                        double multiplier, Tensor workspace) {
    need(dist, at::kFloat, "dist", NATURAL); need(gt, at::kLong, "gt", NATURAL); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(dist.dim() == 2 && gt.dim() == 1 && gt.size(0) <= dist.size(1) && gt.device() == dist.device() &&
                workspace.device() == dist.device(), "osi::evm_fit_rows: dist [R,ld] and gt [N], N <= ld, on one device");
    TORCH_CHECK(dist.size(0) <= INT_MAX && gt.size(0) <= INT_MAX, "osi::evm_fit_rows: sizes out of range");
    const int64_t R = dist.size(0);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dist.device());
    const auto f64 = dist.options().dtype(at::kDouble), i64 = dist.options().dtype(at::kLong);
    Tensor shape = at::empty({R}, f64), scale = at::empty({R}, f64), shift = at::empty({R}, f64);
    Tensor fitted = at::empty({R}, dist.options().dtype(at::kByte)), tail_count = at::empty({R}, i64), flags2 = at::empty({2}, i64);
    ok(osi_evm_fit_rows(dist.data_ptr<float>(), (int)R, (int)gt.size(0), (long long)dist.size(1), (const long long*)gt.data_ptr<int64_t>(),
                        (long long)cls, (int)std::min<int64_t>(tailsize, INT_MAX), (float)multiplier, shape.data_ptr<double>(),
                        scale.data_ptr<double>(), shift.data_ptr<double>(), fitted.data_ptr<unsigned char>(),
                        (long long*)tail_count.data_ptr<int64_t>(), (long long*)flags2.data_ptr<int64_t>(), workspace.data_ptr(),
                        (size_t)workspace.numel(), stream_of(dist)), "osi_evm_fit_rows");
    return {shape, scale, shift, fitted, tail_count, flags2};
}

void evm_params(const Tensor& ref, const Tensor& shape, const Tensor& scale, const Tensor& shift, int64_t n, const char* what) {
    need(shape, at::kDouble, "shape", NATURAL); need(scale, at::kDouble, "scale", NATURAL); need(shift, at::kDouble, "shift", NATURAL);
    TORCH_CHECK(shape.numel() == n && scale.numel() == n && shift.numel() == n, "osi::", what, ": shape, scale and shift hold ", n, " entries");
    TORCH_CHECK(shape.device() == ref.device() && scale.device() == ref.device() && shift.device() == ref.device(), "osi::", what,
                ": tensors on different devices");
}

std::tuple<Tensor, Tensor> evm_set_cover(const Tensor& dpp, const Tensor& shape, const Tensor& scale, const Tensor& shift,
                                         const Tensor& fitted, double multiplier, double cover_threshold, Tensor workspace) {
    need(dpp, at::kFloat, "dpp", NATURAL); need(fitted, at::kByte, "fitted", 1); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(dpp.dim() == 2 && dpp.size(0) == dpp.size(1) && dpp.size(0) <= INT_MAX, "osi::evm_set_cover: dpp is [R,R]");
    const int64_t R = dpp.size(0);
    evm_params(dpp, shape, scale, shift, R, "evm_set_cover");
    TORCH_CHECK(fitted.numel() == R && fitted.device() == dpp.device() && workspace.device() == dpp.device(),
                "osi::evm_set_cover: fitted holds one entry per row, on the device of dpp");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dpp.device());
    const auto i64 = dpp.options().dtype(at::kLong);
    Tensor order = at::empty({R}, i64), n_ev = at::empty({1}, i64);
    ok(osi_evm_set_cover(dpp.data_ptr<float>(), (int)R, shape.data_ptr<double>(), scale.data_ptr<double>(), shift.data_ptr<double>(),
                         fitted.data_ptr<unsigned char>(), (float)multiplier, (float)cover_threshold, (long long*)order.data_ptr<int64_t>(),
                         (long long*)n_ev.data_ptr<int64_t>(), workspace.data_ptr(), (size_t)workspace.numel(), stream_of(dpp)),
       "osi_evm_set_cover");
    return {order, n_ev};
}

Tensor evm_probs(const Tensor& dist, const Tensor& shape, const Tensor& scale, const Tensor& shift, const Tensor& ev_start,
                 double multiplier) {
    need(dist, at::kFloat, "dist", NATURAL); need(ev_start, at::kLong, "ev_start", NATURAL);
    TORCH_CHECK(dist.dim() == 2 && ev_start.dim() == 1 && ev_start.numel() >= 2 && ev_start.device() == dist.device(),
                "osi::evm_probs: dist is [M,ld], ev_start [C+1] on its device");
    const int64_t V = shape.numel(), C = ev_start.numel() - 1;
    evm_params(dist, shape, scale, shift, V, "evm_probs");
    TORCH_CHECK(V <= dist.size(1) && dist.size(0) <= INT_MAX && V <= INT_MAX && C <= INT_MAX, "osi::evm_probs: V <= ld, sizes in range");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dist.device());
    Tensor probs = at::empty({dist.size(0), C}, dist.options());
    ok(osi_evm_probs(dist.data_ptr<float>(), (int)dist.size(0), (int)V, (long long)dist.size(1), shape.data_ptr<double>(),
                     scale.data_ptr<double>(), shift.data_ptr<double>(), (const long long*)ev_start.data_ptr<int64_t>(), (int)C,
                     (float)multiplier, probs.data_ptr<float>(), stream_of(dist)), "osi_evm_probs");
    return probs;
}

// ---- deep nearest neighbours (include/osi.h, ABI 24): dist is [M,ld], every column of it takes part (N = ld)
const long long* knn_skip(const Tensor& dist, const c10::optional<Tensor>& skip, const char* what) {
    if (!skip.has_value() || !skip->defined()) return nullptr;
    need(*skip, at::kLong, "skip", NATURAL);
    TORCH_CHECK(skip->numel() == dist.size(0) && skip->device() == dist.device(), "osi::", what, ": skip holds one column per row, on the device of dist");
    return (const long long*)skip->data_ptr<int64_t>();
}

std::tuple<Tensor, Tensor> knn_topk(const Tensor& dist, int64_t k, const c10::optional<Tensor>& skip, Tensor workspace) {
    need(dist, at::kFloat, "dist", NATURAL); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(dist.dim() == 2 && dist.size(0) <= INT_MAX && dist.size(1) <= INT_MAX && workspace.device() == dist.device(),
                "osi::knn_topk: dist is [M,N], sizes in range, workspace on its device");
    TORCH_CHECK(k >= 1 && k <= OSI_KNN_MAX_K, "osi::knn_topk: k must lie in [1, ", OSI_KNN_MAX_K, "]");
    const int64_t M = dist.size(0);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dist.device());
    Tensor out_dist = at::empty({M, k}, dist.options()), out_idx = at::empty({M, k}, dist.options().dtype(at::kLong));
    ok(osi_knn_topk(dist.data_ptr<float>(), (int)M, (int)dist.size(1), (long long)dist.size(1), (int)k, knn_skip(dist, skip, "knn_topk"),
                    out_dist.data_ptr<float>(), (long long*)out_idx.data_ptr<int64_t>(), workspace.data_ptr(), (size_t)workspace.numel(),
                    stream_of(dist)), "osi_knn_topk");
    return {out_dist, out_idx};
}

Tensor knn_class_kth(const Tensor& dist, const Tensor& start, int64_t k, const c10::optional<Tensor>& skip, int64_t transform,
                     Tensor workspace) {
    need(dist, at::kFloat, "dist", NATURAL); need(start, at::kLong, "start", NATURAL); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(dist.dim() == 2 && start.dim() == 1 && start.numel() >= 2 && start.device() == dist.device() &&
                workspace.device() == dist.device(), "osi::knn_class_kth: dist is [M,N], start [C+1] on its device");
    TORCH_CHECK(dist.size(0) <= INT_MAX && dist.size(1) <= INT_MAX && start.numel() - 1 <= INT_MAX, "osi::knn_class_kth: sizes out of range");
    TORCH_CHECK(k >= 1 && k <= OSI_KNN_MAX_K, "osi::knn_class_kth: k must lie in [1, ", OSI_KNN_MAX_K, "]");
    const int64_t M = dist.size(0), C = start.numel() - 1;
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dist.device());
    Tensor out = at::empty({M, C}, dist.options());
    ok(osi_knn_class_kth(dist.data_ptr<float>(), (int)M, (int)dist.size(1), (long long)dist.size(1), (const long long*)start.data_ptr<int64_t>(),
                         (int)C, (int)k, knn_skip(dist, skip, "knn_class_kth"), (int)std::min<int64_t>(std::max<int64_t>(transform, -1), INT_MAX),
                         out.data_ptr<float>(), workspace.data_ptr(), (size_t)workspace.numel(), stream_of(dist)), "osi_knn_class_kth");
    return out;
}

// ---- Mahalanobis / Relative Mahalanobis (include/osi.h, ABI 25): fp32 features, int64 labels, every fitted tensor fp64
int maha_dim(int64_t v, const char* what) {
    TORCH_CHECK(v >= 1 && v <= INT_MAX, "osi::", what, ": sizes out of range");
    return (int)v;
}

std::tuple<Tensor, Tensor> maha_class_means(const Tensor& features, const Tensor& gt, int64_t C, Tensor workspace) {
    need(features, at::kFloat, "features", NATURAL); need(gt, at::kLong, "gt", NATURAL); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(features.dim() == 2 && gt.dim() == 1 && gt.numel() == features.size(0) && gt.device() == features.device() &&
                workspace.device() == features.device(), "osi::maha_class_means: features [N,F], gt [N] on one device");
    const int N = maha_dim(features.size(0), "maha_class_means"), F = maha_dim(features.size(1), "maha_class_means");
    const int c = maha_dim(C, "maha_class_means");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(features.device());
    Tensor mean = at::empty({C + 1, (int64_t)F}, features.options().dtype(at::kDouble));
    Tensor count = at::empty({C + 1}, features.options().dtype(at::kLong));
    ok(osi_maha_class_means(features.data_ptr<float>(), (const long long*)gt.data_ptr<int64_t>(), N, c, F, mean.data_ptr<double>(),
                            (long long*)count.data_ptr<int64_t>(), workspace.data_ptr(), (size_t)workspace.numel(), stream_of(features)),
       "osi_maha_class_means");
    return {mean, count};
}

void maha_scatter(const Tensor& features, const Tensor& gt, const Tensor& mean, int64_t mode, bool accumulate, Tensor S, Tensor workspace) {
    need(features, at::kFloat, "features", NATURAL); need(gt, at::kLong, "gt", NATURAL); need(mean, at::kDouble, "mean", 8);
    need(S, at::kDouble, "S", 8); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(features.dim() == 2 && gt.dim() == 1 && gt.numel() == features.size(0) && mean.dim() == 2 && mean.size(0) >= 2 &&
                mean.size(1) == features.size(1) && S.dim() == 2 && S.size(0) == features.size(1) && S.size(1) == features.size(1),
                "osi::maha_scatter: features [N,F], gt [N], mean [C+1,F], S [F,F]");
    TORCH_CHECK(gt.device() == features.device() && mean.device() == features.device() && S.device() == features.device() &&
                workspace.device() == features.device(), "osi::maha_scatter: tensors on different devices");
    const int N = maha_dim(features.size(0), "maha_scatter"), F = maha_dim(features.size(1), "maha_scatter");
    const int C = maha_dim(mean.size(0) - 1, "maha_scatter");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(features.device());
    ok(osi_maha_scatter(features.data_ptr<float>(), (const long long*)gt.data_ptr<int64_t>(), mean.data_ptr<double>(), N, C, F,
                        (int)std::min<int64_t>(std::max<int64_t>(mode, -1), INT_MAX), accumulate ? 1 : 0, S.data_ptr<double>(),
                        workspace.data_ptr(), (size_t)workspace.numel(), stream_of(features)), "osi_maha_scatter");
}

std::tuple<Tensor, Tensor, Tensor, Tensor> maha_factor(const Tensor& S, double scale, double shrinkage, Tensor workspace) {
    need(S, at::kDouble, "S", 8); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(S.dim() == 2 && S.size(0) == S.size(1) && workspace.device() == S.device(), "osi::maha_factor: S is [F,F], workspace on its device");
    const int F = maha_dim(S.size(0), "maha_factor");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(S.device());
    Tensor L = at::empty_like(S), W = at::empty_like(S);
    Tensor logdet = at::empty({1}, S.options()), info = at::empty({1}, S.options().dtype(at::kInt));
    ok(osi_maha_factor(S.data_ptr<double>(), F, scale, shrinkage, L.data_ptr<double>(), W.data_ptr<double>(), logdet.data_ptr<double>(),
                       info.data_ptr<int>(), workspace.data_ptr(), (size_t)workspace.numel(), stream_of(S)), "osi_maha_factor");
    return {L, W, logdet, info};
}

Tensor maha_whiten(const Tensor& x, const Tensor& W, Tensor workspace) {
    need(W, at::kDouble, "W", 8); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(x.defined() && (x.scalar_type() == at::kFloat || x.scalar_type() == at::kDouble), "osi::maha_whiten: x is fp32 or fp64");
    need(x, x.scalar_type(), "x", NATURAL);
    TORCH_CHECK(x.dim() == 2 && W.dim() == 2 && W.size(0) == x.size(1) && W.size(1) == x.size(1) && W.device() == x.device() &&
                workspace.device() == x.device(), "osi::maha_whiten: x [M,F], W [F,F] on one device");
    const int M = maha_dim(x.size(0), "maha_whiten"), F = maha_dim(x.size(1), "maha_whiten");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    Tensor z = at::empty({(int64_t)M, (int64_t)F}, W.options());
    if (x.scalar_type() == at::kFloat)
        ok(osi_maha_whiten_f32(x.data_ptr<float>(), M, F, W.data_ptr<double>(), z.data_ptr<double>(), workspace.data_ptr(),
                               (size_t)workspace.numel(), stream_of(x)), "osi_maha_whiten_f32");
    else
        ok(osi_maha_whiten_f64(x.data_ptr<double>(), M, F, W.data_ptr<double>(), z.data_ptr<double>(), workspace.data_ptr(),
                               (size_t)workspace.numel(), stream_of(x)), "osi_maha_whiten_f64");
    return z;
}

Tensor maha_sqdist(const Tensor& z, const Tensor& zm, const c10::optional<Tensor>& minus, int64_t transform, bool f64_out, Tensor workspace) {
    need(z, at::kDouble, "z", 8); need(zm, at::kDouble, "zm", 8); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(z.dim() == 2 && zm.dim() == 2 && zm.size(1) == z.size(1) && zm.device() == z.device() && workspace.device() == z.device(),
                "osi::maha_sqdist: z [M,F], zm [C,F] on one device");
    const double* mp = nullptr;
    if (minus.has_value() && minus->defined()) {
        need(*minus, at::kDouble, "minus", 8);
        TORCH_CHECK(minus->numel() == z.size(0) && minus->device() == z.device(), "osi::maha_sqdist: minus holds one value per row, on the device of z");
        mp = minus->data_ptr<double>();
    }
    const int M = maha_dim(z.size(0), "maha_sqdist"), F = maha_dim(z.size(1), "maha_sqdist"), C = maha_dim(zm.size(0), "maha_sqdist");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(z.device());
    Tensor out = at::empty({(int64_t)M, (int64_t)C}, z.options().dtype(f64_out ? at::kDouble : at::kFloat));
    ok(osi_maha_sqdist(z.data_ptr<double>(), M, zm.data_ptr<double>(), C, F, mp, (int)std::min<int64_t>(std::max<int64_t>(transform, -1), INT_MAX),
                       f64_out ? nullptr : out.data_ptr<float>(), f64_out ? out.data_ptr<double>() : nullptr, workspace.data_ptr(),
                       (size_t)workspace.numel(), stream_of(z)), "osi_maha_sqdist");
    return out;
}

// ---- ViM and the symmetric eigensolver (include/osi.h, ABI 26): fp32 features and logits, every fitted tensor fp64
std::tuple<Tensor, Tensor, Tensor, Tensor> eigh_begin(const Tensor& S, Tensor workspace) {
    need(S, at::kDouble, "S", 8); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(S.dim() == 2 && S.size(0) == S.size(1) && workspace.device() == S.device(), "osi::eigh_begin: S is [F,F], workspace on its device");
    const int F = maha_dim(S.size(0), "eigh_begin");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(S.device());
    Tensor A = at::empty_like(S), Vt = at::empty_like(S);
    Tensor head = at::empty({2}, S.options()), info = at::empty({1}, S.options().dtype(at::kInt));
    ok(osi_eigh_begin(S.data_ptr<double>(), F, A.data_ptr<double>(), Vt.data_ptr<double>(), head.data_ptr<double>(), info.data_ptr<int>(),
                      workspace.data_ptr(), (size_t)workspace.numel(), stream_of(S)), "osi_eigh_begin");
    return {A, Vt, head, info};
}

Tensor eigh_sweep(Tensor A, Tensor Vt, const Tensor& head, const Tensor& info, Tensor workspace) {
    need(A, at::kDouble, "A", 8); need(Vt, at::kDouble, "Vt", 8); need(head, at::kDouble, "head", 8); need(info, at::kInt, "info", NATURAL);
    need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(A.dim() == 2 && A.size(0) == A.size(1) && Vt.sizes() == A.sizes() && head.numel() == 2 && info.numel() == 1,
                "osi::eigh_sweep: A and Vt are [F,F], head holds 2 values, info 1");
    TORCH_CHECK(Vt.device() == A.device() && head.device() == A.device() && info.device() == A.device() && workspace.device() == A.device(),
                "osi::eigh_sweep: tensors on different devices");
    const int F = maha_dim(A.size(0), "eigh_sweep");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(A.device());
    Tensor rotations = at::empty({1}, A.options().dtype(at::kLong));
    ok(osi_eigh_sweep(A.data_ptr<double>(), Vt.data_ptr<double>(), F, head.data_ptr<double>(), info.data_ptr<int>(),
                      (long long*)rotations.data_ptr<int64_t>(), workspace.data_ptr(), (size_t)workspace.numel(), stream_of(A)), "osi_eigh_sweep");
    return rotations;
}

std::tuple<Tensor, Tensor> eigh_finish(const Tensor& A, const Tensor& Vt, const Tensor& info, Tensor workspace) {
    need(A, at::kDouble, "A", 8); need(Vt, at::kDouble, "Vt", 8); need(info, at::kInt, "info", NATURAL); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(A.dim() == 2 && A.size(0) == A.size(1) && Vt.sizes() == A.sizes() && info.numel() == 1 && Vt.device() == A.device() &&
                info.device() == A.device() && workspace.device() == A.device(), "osi::eigh_finish: A and Vt are [F,F], info 1 value, on one device");
    const int F = maha_dim(A.size(0), "eigh_finish");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(A.device());
    Tensor evals = at::empty({(int64_t)F}, A.options()), evecs = at::empty_like(A);
    ok(osi_eigh_finish(A.data_ptr<double>(), Vt.data_ptr<double>(), F, info.data_ptr<int>(), evals.data_ptr<double>(), evecs.data_ptr<double>(),
                       workspace.data_ptr(), (size_t)workspace.numel(), stream_of(A)), "osi_eigh_finish");
    return {evals, evecs};
}

Tensor vim_project(const Tensor& x, const Tensor& origin, const Tensor& R, Tensor workspace) {
    need(x, at::kFloat, "x", NATURAL); need(origin, at::kDouble, "origin", 8); need(R, at::kDouble, "R", 8); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(x.dim() == 2 && R.dim() == 2 && R.size(1) == x.size(1) && origin.numel() == x.size(1) && origin.device() == x.device() &&
                R.device() == x.device() && workspace.device() == x.device(), "osi::vim_project: x [M,F], origin [F], R [K,F] on one device");
    const int M = maha_dim(x.size(0), "vim_project"), F = maha_dim(x.size(1), "vim_project"), K = maha_dim(R.size(0), "vim_project");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    Tensor z = at::empty({(int64_t)M, (int64_t)K}, R.options());
    ok(osi_vim_project_f32(x.data_ptr<float>(), origin.data_ptr<double>(), M, F, R.data_ptr<double>(), K, z.data_ptr<double>(),
                           workspace.data_ptr(), (size_t)workspace.numel(), stream_of(x)), "osi_vim_project_f32");
    return z;
}

Tensor vim_scores(const Tensor& z, const c10::optional<Tensor>& logits, double alpha, int64_t mode, bool f64_out, Tensor workspace) {
    need(z, at::kDouble, "z", 8); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(z.dim() == 2 && workspace.device() == z.device(), "osi::vim_scores: z [M,K], workspace on its device");
    const int M = maha_dim(z.size(0), "vim_scores"), K = maha_dim(z.size(1), "vim_scores");
    const float* lp = nullptr;
    int C = 1;
    if (logits.has_value() && logits->defined()) {
        need(*logits, at::kFloat, "logits", NATURAL);
        TORCH_CHECK(logits->dim() == 2 && logits->size(0) == z.size(0) && logits->device() == z.device(),
                    "osi::vim_scores: logits [M,C] on the device of z");
        C = maha_dim(logits->size(1), "vim_scores");
        lp = logits->data_ptr<float>();
    }
    const int md = (int)std::min<int64_t>(std::max<int64_t>(mode, -1), INT_MAX);
    c10::hip::HIPGuardMasqueradingAsCUDA guard(z.device());
    Tensor out = md == OSI_VIM_PROBS ? at::empty({(int64_t)M, (int64_t)C + 1}, z.options().dtype(f64_out ? at::kDouble : at::kFloat))
                                     : at::empty({(int64_t)M}, z.options().dtype(f64_out ? at::kDouble : at::kFloat));
    ok(osi_vim_scores(z.data_ptr<double>(), M, K, lp, C, alpha, md, f64_out ? nullptr : out.data_ptr<float>(),
                      f64_out ? out.data_ptr<double>() : nullptr, workspace.data_ptr(), (size_t)workspace.numel(), stream_of(z)), "osi_vim_scores");
    return out;
}

// ---- activation shaping (include/osi.h, ABI 27): the pooled activation, exact order statistics, shaped rows, logit scores
Tensor resnet50_pooled(int64_t net, const Tensor& workspace) {
    need(workspace, at::kByte, "workspace");
    osi_resnet50_t h = handle(net);
    TORCH_CHECK((size_t)workspace.numel() >= osi_resnet50_workspace_bytes(h), "osi::resnet50_pooled: workspace too small");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(workspace.device());
    size_t floats = 0;
    ok(osi_resnet50_pooled(h, nullptr, nullptr, &floats, nullptr), "osi_resnet50_pooled");
    Tensor out = at::empty({(int64_t)(floats / 2048), 2048}, workspace.options().dtype(at::kFloat));
    ok(osi_resnet50_pooled(h, workspace.data_ptr(), out.data_ptr<float>(), &floats, stream_of(workspace)), "osi_resnet50_pooled");
    return out;
}

Tensor order_stats(const Tensor& v, at::IntArrayRef ranks, Tensor workspace) {
    need(v, at::kFloat, "v", NATURAL); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(v.numel() >= 1 && workspace.device() == v.device(), "osi::order_stats: v is not empty, workspace on its device");
    TORCH_CHECK(ranks.size() >= 1 && ranks.size() <= OSI_ORDER_STATS_MAX_R, "osi::order_stats: 1 .. ", OSI_ORDER_STATS_MAX_R, " ranks");
    long long rk[OSI_ORDER_STATS_MAX_R];
    for (size_t r = 0; r < ranks.size(); ++r) {
        TORCH_CHECK(ranks[r] >= 0 && ranks[r] < v.numel(), "osi::order_stats: rank ", ranks[r], " outside [0, ", v.numel(), ")");
        rk[r] = (long long)ranks[r];
    }
    c10::hip::HIPGuardMasqueradingAsCUDA guard(v.device());
    Tensor out = at::empty({(int64_t)ranks.size()}, v.options());
    ok(osi_order_stats_f32(v.data_ptr<float>(), (long long)v.numel(), rk, (int)ranks.size(), out.data_ptr<float>(), workspace.data_ptr(),
                           (size_t)workspace.numel(), stream_of(v)), "osi_order_stats_f32");
    return out;
}

Tensor shape_rows(const Tensor& x, int64_t mode, int64_t keep, double clip, Tensor workspace) {
    need(x, at::kFloat, "x", NATURAL); need(workspace, at::kByte, "workspace", 8);
    TORCH_CHECK(x.dim() == 2 && workspace.device() == x.device(), "osi::shape_rows: x [M,F], workspace on its device");
    const int M = maha_dim(x.size(0), "shape_rows"), F = maha_dim(x.size(1), "shape_rows");
    const auto clamp = [](int64_t a) { return (int)std::min<int64_t>(std::max<int64_t>(a, -1), INT_MAX); };
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    Tensor out = at::empty_like(x);
    ok(osi_shape_rows(x.data_ptr<float>(), M, F, clamp(mode), clamp(keep), (float)clip, out.data_ptr<float>(), workspace.data_ptr(),
                      (size_t)workspace.numel(), stream_of(x)), "osi_shape_rows");
    return out;
}

Tensor logit_scores(const Tensor& logits, int64_t mode) {
    need(logits, at::kFloat, "logits", NATURAL);
    TORCH_CHECK(logits.dim() == 2, "osi::logit_scores: logits [M,C]");
    const int M = maha_dim(logits.size(0), "logit_scores"), C = maha_dim(logits.size(1), "logit_scores");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
    Tensor out = at::empty({(int64_t)M}, logits.options());
    ok(osi_logit_scores(logits.data_ptr<float>(), M, C, (int)std::min<int64_t>(std::max<int64_t>(mode, -1), INT_MAX), out.data_ptr<float>(),
                        stream_of(logits)), "osi_logit_scores");
    return out;
}

// ---- PROSER (include/osi.h, ABI 23)
void need_pairs(const Tensor& ref, const Tensor& partner, const Tensor& weight, int64_t B, const char* what) {
    need(partner, at::kInt, "partner", NATURAL); need(weight, at::kFloat, "weight", NATURAL);
    TORCH_CHECK(partner.numel() == B && weight.numel() == B, "osi::", what, ": partner and weight hold one entry per row (", B, ")");
    TORCH_CHECK(partner.device() == ref.device() && weight.device() == ref.device(), "osi::", what, ": tensors on different devices");
}

void mix_rows_pairs(Tensor x, const Tensor& partner, const Tensor& weight) {
    need(x, at::kFloat, "x");
    TORCH_CHECK(x.dim() >= 2 && x.size(0) <= INT_MAX && x.numel() > 0, "osi::mix_rows_pairs: x is [B, ...] with at least one element");
    const int64_t B = x.size(0), L = x.numel() / B;
    TORCH_CHECK(L % 4 == 0, "osi::mix_rows_pairs: the row length must be a multiple of 4, got ", L);
    need_pairs(x, partner, weight, B, "mix_rows_pairs");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    ok(osi_mix_rows_pairs(x.data_ptr<float>(), partner.data_ptr<int>(), weight.data_ptr<float>(), (int)B, (size_t)L, stream_of(x)),
       "osi_mix_rows_pairs");
}

// the one-shot request of the executor's next differentiable forward; both tensors absent clears it. The caller keeps them alive until
// that forward has been enqueued (model.py holds them)
void resnet50_set_mix(int64_t net, const std::optional<Tensor>& partner, const std::optional<Tensor>& weight) {
    osi_resnet50_t h = handle(net);
    const bool hp = partner.has_value() && partner->defined(), hw = weight.has_value() && weight->defined();
    TORCH_CHECK(hp == hw, "osi::resnet50_set_mix: partner and weight go together");
    if (!hp) { ok(osi_resnet50_set_mix(h, nullptr, nullptr), "osi_resnet50_set_mix"); return; }
    int B = 0;
    ok(osi_resnet50_geometry(h, &B, nullptr, nullptr), "osi_resnet50_geometry");
    need_pairs(*partner, *partner, *weight, B, "resnet50_set_mix");
    ok(osi_resnet50_set_mix(h, partner->data_ptr<int>(), weight->data_ptr<float>()), "osi_resnet50_set_mix");
}

// returns (loss4 [4] = {J, mean t1, mean t2, mean t3}, dlogits [B,C] or empty, ddummy [B,D] or empty)
std::tuple<Tensor, Tensor, Tensor> proser_loss_fwd_bwd(const Tensor& logits, const Tensor& dummy, const Tensor& target, int64_t n_mixed,
                                                       double l0, double l1, double l2, bool need_grad) {
    need(logits, at::kFloat, "logits", NATURAL); need(dummy, at::kFloat, "dummy", NATURAL); need(target, at::kLong, "target", NATURAL);
    TORCH_CHECK(logits.dim() == 2 && dummy.dim() == 2 && target.dim() == 1 && dummy.size(0) == logits.size(0) &&
                target.size(0) == logits.size(0), "osi::proser_loss_fwd_bwd: expected logits [B, C], dummy [B, D] and target [B]");
    TORCH_CHECK(dummy.device() == logits.device() && target.device() == logits.device(), "osi::proser_loss_fwd_bwd: tensors on different devices");
    TORCH_CHECK(logits.size(0) <= INT_MAX && logits.size(1) <= INT_MAX && dummy.size(1) <= INT_MAX && n_mixed >= 0 && n_mixed <= logits.size(0),
                "osi::proser_loss_fwd_bwd: sizes out of range or n_mixed outside [0, B]");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
    Tensor loss4 = at::empty({4}, logits.options());
    Tensor dlogits = need_grad ? at::empty_like(logits) : at::empty({0}, logits.options());
    Tensor ddummy = need_grad ? at::empty_like(dummy) : at::empty({0}, logits.options());
    ok(osi_proser_loss_fwd_bwd(logits.data_ptr<float>(), dummy.data_ptr<float>(), (const long long*)target.data_ptr<int64_t>(),
                               (int)logits.size(0), (int)logits.size(1), (int)dummy.size(1), (int)n_mixed, (float)l0, (float)l1, (float)l2,
                               loss4.data_ptr<float>(), need_grad ? dlogits.data_ptr<float>() : nullptr,
                               need_grad ? ddummy.data_ptr<float>() : nullptr, stream_of(logits)), "osi_proser_loss_fwd_bwd");
    return {loss4, dlogits, ddummy};
}

Tensor proser_scores(const Tensor& logits, const Tensor& dummy, double bias) {
    need(logits, at::kFloat, "logits", NATURAL); need(dummy, at::kFloat, "dummy", NATURAL);
    TORCH_CHECK(logits.dim() == 2 && dummy.dim() == 2 && dummy.size(0) == logits.size(0) && dummy.device() == logits.device(),
                "osi::proser_scores: expected logits [B, C] and dummy [B, D] on one device");
    TORCH_CHECK(logits.size(0) <= INT_MAX && logits.size(1) < INT_MAX && dummy.size(1) <= INT_MAX, "osi::proser_scores: sizes out of range");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(logits.device());
    Tensor probs = at::empty({logits.size(0), logits.size(1) + 1}, logits.options());
    ok(osi_proser_scores(logits.data_ptr<float>(), dummy.data_ptr<float>(), (float)bias, (int)logits.size(0), (int)logits.size(1),
                         (int)dummy.size(1), probs.data_ptr<float>(), stream_of(logits)), "osi_proser_scores");
    return probs;
}

// the small dense layer of the package's own kernels (csrc/linear.hip) for layers outside the executor: y = x w^T + bias
Tensor linear_fwd(const Tensor& x, const Tensor& w, const std::optional<Tensor>& bias) {
    need(x, at::kFloat, "x", NATURAL); need(w, at::kFloat, "w", NATURAL);
    TORCH_CHECK(x.dim() == 2 && w.dim() == 2 && x.size(1) == w.size(1) && w.device() == x.device(), "osi::linear_fwd: x [B, K] and w [O, K] on one device");
    const bool hb = bias.has_value() && bias->defined();
    if (hb) { need(*bias, at::kFloat, "bias", NATURAL); TORCH_CHECK(bias->numel() == w.size(0) && bias->device() == x.device(), "osi::linear_fwd: bias holds O entries"); }
    TORCH_CHECK(x.size(1) <= INT_MAX, "osi::linear_fwd: sizes out of range");
    // the 16-byte loads of the K % 4 == 0 form need aligned rows
    TORCH_CHECK(x.size(1) % 4 != 0 || ((reinterpret_cast<uintptr_t>(x.data_ptr()) | reinterpret_cast<uintptr_t>(w.data_ptr())) & 15) == 0,
                "osi::linear_fwd: x and w must be 16-byte aligned when K is a multiple of 4");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
    Tensor y = at::empty({x.size(0), w.size(0)}, x.options());
    ok(osi_linear_fwd(x.data_ptr<float>(), w.data_ptr<float>(), fptr(bias), y.data_ptr<float>(), (int)x.size(0), (int)x.size(1), (int)w.size(0),
                      stream_of(x)), "osi_linear_fwd");
    return y;
}

// returns (dx [B,K] or empty, dw [O,K], db [O])
std::tuple<Tensor, Tensor, Tensor> linear_bwd(const Tensor& dy, const Tensor& x, const Tensor& w, bool need_dx) {
    need(dy, at::kFloat, "dy", NATURAL); need(x, at::kFloat, "x", NATURAL); need(w, at::kFloat, "w", NATURAL);
    TORCH_CHECK(dy.dim() == 2 && x.dim() == 2 && w.dim() == 2 && dy.size(0) == x.size(0) && dy.size(1) == w.size(0) && x.size(1) == w.size(1) &&
                x.device() == dy.device() && w.device() == dy.device(), "osi::linear_bwd: dy [B, O], x [B, K] and w [O, K] on one device");
    TORCH_CHECK(x.size(1) <= INT_MAX, "osi::linear_bwd: sizes out of range");
    c10::hip::HIPGuardMasqueradingAsCUDA guard(dy.device());
    Tensor dx = need_dx ? at::empty_like(x) : at::empty({0}, x.options());
    Tensor dw = at::empty_like(w), db = at::empty({w.size(0)}, w.options());
    ok(osi_linear_bwd(dy.data_ptr<float>(), x.data_ptr<float>(), w.data_ptr<float>(), need_dx ? dx.data_ptr<float>() : nullptr, 0,
                      dw.data_ptr<float>(), db.data_ptr<float>(), (int)dy.size(0), (int)x.size(1), (int)w.size(0), stream_of(dy)),
       "osi_linear_bwd");
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
    m.impl("mix_rows_pairs", &mix_rows_pairs);
    m.impl("proser_loss_fwd_bwd", &proser_loss_fwd_bwd);
    m.impl("proser_scores", &proser_scores);
    m.impl("linear_fwd", &linear_fwd);
    m.impl("linear_bwd", &linear_bwd);
}
