// ABI bookkeeping for libosi_hip.so.
#include "osi_common.h"

#include <cstring>

OsiTuning g_osi_tuning;   // every field at the default of its row in OSI_TUNING_KNOBS

namespace {
struct Knob { const char* name; int OsiTuning::*slot; int def, lo, hi, plan; };
const Knob kKnobs[] = {
#define OSI_KNOB_ROW(name, def, lo, hi, plan) {#name, &OsiTuning::name, def, lo, hi, plan},
    OSI_TUNING_KNOBS(OSI_KNOB_ROW)
#undef OSI_KNOB_ROW
};
const int kNumKnobs = (int)(sizeof(kKnobs) / sizeof(kKnobs[0]));
const Knob* find_knob(const char* name) {
    if (!name) return nullptr;
    for (const Knob& k : kKnobs)
        if (!strcmp(name, k.name)) return &k;
    return nullptr;
}
}  // namespace

extern "C" {
int osi_abi_version(void) { return 29; }   // 29: gradient-based open-set scores (osi_odin_head: the temperature-scaled largest softmax probability, torch.argmax's prediction and the seed of ODIN's input-only backward; osi_gradnorm_scores: GradNorm's closed form for the last linear layer); 28: detection metrics and the OSCR curve by rejection score (osi_det_workspace, osi_det_ranks_f32 / _f64, osi_det_summary, osi_det_curve_f32 / _f64: six all-pairs rank counts per row, from them the Mann-Whitney pair counts, the average-precision sums, FPR counts at TPR levels and the curve over the known rows' distinct values); 27: activation shaping on the pooled layer (osi_resnet50_pooled, osi_order_stats_workspace, osi_order_stats_f32, osi_shape_rows_workspace, osi_shape_rows, osi_logit_scores: the penultimate activation, exact order statistics by radix select, ReAct / ASH-P / ASH-B / ASH-S / SCALE rows, energy / max-logit / MSP scores); 26: ViM scores and the symmetric eigensolver (osi_vim_workspace, osi_eigh_begin, osi_eigh_sweep, osi_eigh_finish, osi_vim_project_f32, osi_vim_scores: parallel cyclic Jacobi in fp64, the residual projection on the fp64 matrix cores, norm / unknown score / softmax with the virtual logit); 25: Mahalanobis / Relative Mahalanobis scores on the fp64 matrix cores (osi_maha_workspace, osi_maha_class_means, osi_maha_scatter, osi_maha_factor, osi_maha_whiten_f32 / _f64, osi_maha_sqdist); 24: deep nearest neighbours (osi_knn_workspace, osi_knn_topk, osi_knn_class_kth: the k smallest of a distance row with their columns, the k-th smallest inside every class segment, ties by column); 23: PROSER (osi_mix_rows_pairs, osi_resnet50_set_mix, osi_resnet50_debug_unit_input, osi_proser_loss_fwd_bwd, osi_proser_scores: manifold mixup at the frozen cut, the three-term placeholder loss, scores with the unknown column last); 22: the Extreme Value Machine (osi_evm_workspace, osi_evm_distances, osi_evm_fit_rows, osi_evm_set_cover, osi_evm_probs: all-pairs distances on the fp32 matrix cores, one Weibull per row, greedy model reduction, class scores); 21: OpenMax (osi_openmax_workspace, osi_openmax_class_means, osi_openmax_distances, osi_openmax_fit_tails, osi_openmax_wscores, osi_openmax_recalibrate: class means, Weibull tails, recalibrated scores with the unknown column last); 20: weight averaging (osi_average_update, osi_avg_span) and the executor's BatchNorm momentum (osi_resnet50_set_bn_momentum, osi_resnet50_get_bn_momentum); 19: projected attack steps (osi_stem_dgrad_pgd, osi_attack, osi_resnet50_backward_attack: input-only or full backward ending in the PGD epilogue); 18: evaluation histograms (osi_eval_values_workspace, osi_eval_values_f32 / _f64, osi_hist_f32 / _f64); 17: gradient-norm clipping (osi_grad_norm_workspace, osi_grad_clip_scale: norm and step scalar left in device memory; osi_adam_step_groups_dev, osi_sgd_step_groups_dev: the grouped steps reading that scalar); 16: ROC-AUC counting (osi_auc_workspace, osi_auc_binary_f32 / _f64, osi_auc_ovr_f32 / _f64); 15: osi_tuning_info (the knob table: names, defaults, ranges, plan relevance); 14: osi_bn_backward_fused2, osi_bn_backward_fused2_workspace (one pass for the two BatchNorm backwards of a projection block); 13: fine-tuning units (osi_resnet50_num_units, _tensor_unit, _bn_unit, _set_trainable, _get_trainable: backward stops at the frozen prefix, no weight gradient for a frozen unit, inference-form prefix in a differentiable forward), executor action "forget_forward"; 12: frozen-statistics BatchNorm backward (osi_bn_frozen_coeffs_multi, osi_conv_dgrad_fused_frozen, osi_bn_backward_frozen, osi_bn_relu_maxpool_bwd_frozen, osi_resnet50_forward_frozen); 11: osi_adam_step_groups, osi_sgd_step_groups (parameter groups, weight decay, AdamW, amsgrad, nesterov in one launch); 10: osi_stem_dgrad_fgsm, osi_grad_accumulate, osi_resnet50_backward_adv (adversarial negatives in the training step); 9: eight settled executor A/B options retired (osi_resnet50_set_option refuses their names), the duplicate setter of "overlap" removed; 8: osi_stem_dgrad, osi_resnet50_backward_ex (dJ/dimage, input-only backward); 7: inference forms (osi_conv_fwd_epilogue, osi_conv_fwd_wino_epilogue_pre, osi_bn_eval_coeffs_multi), executor option "eval_fused"; 6: Winograd forms (osi_conv_*_wino), knobs "fwd_wino" / "dgrad_wino"; 5: osi_resnet50_grads_ready, executor option "stage_join", knob "dp_reserved_cus", range-checked knobs, plan snapshot (4: addend_stride, accumulate = 2)
int osi_set_tuning(const char* name, int value) {
    const Knob* k = find_knob(name);
    if (!k) return OSI_ERR_ARG;
    // every knob has a range; a value outside it is refused instead of silently switching a plan off
    if (value < k->lo || value > k->hi) return OSI_ERR_ARG;
    if (k->slot == &OsiTuning::wgrad_tile && value != 0 && value != 64) return OSI_ERR_ARG;   // the one knob whose range has a hole
    g_osi_tuning.*(k->slot) = value;
    return OSI_OK;
}
int osi_get_tuning(const char* name, int* value) {
    const Knob* k = find_knob(name);
    if (!k || !value) return OSI_ERR_ARG;
    *value = g_osi_tuning.*(k->slot);
    return OSI_OK;
}
int osi_tuning_info(int i, const char** name, int* def, int* lo, int* hi, int* plan_relevant) {
    if (i < 0 || i >= kNumKnobs) return OSI_ERR_ARG;
    const Knob& k = kKnobs[i];
    if (name) *name = k.name;
    if (def) *def = k.def;
    if (lo) *lo = k.lo;
    if (hi) *hi = k.hi;
    if (plan_relevant) *plan_relevant = k.plan;
    return OSI_OK;
}
const char* osi_build_arch(void) { return "gfx950"; }
const char* osi_strerror(int code) {
    switch (code) {
        case OSI_OK: return "ok";
        case OSI_ERR_ARG: return "invalid argument (shape, pointer or alignment precondition)";
        case OSI_ERR_LAUNCH: return "HIP launch failed";
        case OSI_ERR_STATE: return "executor called out of order, or a plan-relevant tuning knob changed after osi_resnet50_create";
        default: return "unknown error";
    }
}
}
