"""Adversarial negatives for open-set training: FGSM and noise samples made from the batch in flight and trained as negatives.

Not in the reference snapshot (upstream's loop grew an `adv` block later: who / epsilon / decay), so the arithmetic is defined HERE,
as it is for the objectosphere loss. Per training step, when `cfg.adv.who` is not `no_adv` (train.train):

    logits, features = model(x);  j = loss(logits, y);  j.backward()                      the clean pass
    x_neg = fgsm_attack(x, dJ/dx, epsilon)      (who = fgsm)    or    noise_negatives(x, who, ...)   (who = gaussian | uniform)
    logits_n, features_n = model(x_neg);  j_adv = loss(logits_n, negative label);  j_adv.backward()   gradients ADD to the clean ones
    optimizer.step()                                                                      one step on dJ/dp of J = j + j_adv

Both forwards run in training mode, so BatchNorm running statistics (and num_batches_tracked) are updated twice per step — what torch
does with two training-mode forwards. j and j_adv are each a mean over their own batch of B samples.

  fgsm_attack(images, grad, epsilon, lo=0., hi=1.)      clamp(x + epsilon * sign(grad), lo, hi) with torch ops on NCHW tensors: the
        documented semantics. On the MI355X ResNet50 the loop does not call it: the executor's backward ends in a stem input-gradient
        kernel whose epilogue applies exactly this formula to the NHWC4 batch the forward read (ResNet50.next_backward(fgsm=epsilon),
        osi_stem_dgrad_fgsm) — dJ/dx is never written, and NCHW, NHWC4 and uint8-staged batches are served alike.
  noise_negatives(images, who, std_or_width, generator)  x + std * randn  |  x + width * (2 * rand - 1), clamped to [0, 1]. Torch ops
        on the batch's device; no gradient and no kernel of its own.
  negative_label(loss_type, n_classes)                  -1 (entropic, objectosphere) | n_classes - 1 (garbage: the background class)
  scheduled_epsilon(adv_cfg, epoch)                     max(min_epsilon, epsilon * mu ** (epoch // decay));  decay = 0: constant

Out of scope: "filter" mode (perturbing only the correctly classified known samples changes the batch size per step, and with it the
executor's geometry), multi-step attacks, adversaries in validate() — no longer for want of a gradient: in eval mode
`model.next_backward(fgsm=eps)` BEFORE the forward makes it differentiable on the running statistics and its backward ends in the same
FGSM epilogue (`adversarial_batch()`), the statistics untouched; wiring that into validate() is not done here.
"""
import torch

WHO = ("no_adv", "fgsm", "gaussian", "uniform")


def fgsm_attack(images, grad, epsilon, lo=0.0, hi=1.0):
    """clamp(images + epsilon * sign(grad), lo, hi) — NCHW tensors of one shape; sign is torch.sign (+1 / 0 / -1)."""
    if images.shape != grad.shape:
        raise ValueError("fgsm_attack: images and grad must have the same shape")
    if not float(epsilon) >= 0.0 or not float(lo) <= float(hi):
        raise ValueError("fgsm_attack: epsilon >= 0 and lo <= hi")
    return torch.clamp(images + float(epsilon) * torch.sign(grad), float(lo), float(hi))


def _is_nhwc4(images):
    return images.dtype == torch.float32 and images.dim() == 4 and images.shape[3] == 4 and images.shape[1] != 3


def noise_negatives(images, who, std_or_width, generator=None):
    """Noise samples from a clean batch: `gaussian` x + std * randn, `uniform` x + width * (2 * rand - 1), clamped to [0, 1].

    The noise is always drawn as ONE [B, 3, H, W] tensor on the batch's device from `generator` (None: the device's default one), so a
    seed means the same negatives whatever layout the batch came in: an NCHW batch gives an NCHW result, an NHWC4 batch
    (pipeline.device_batch's) an NHWC4 one with a zero 4th lane. A uint8 batch has no value range to add noise in: ValueError."""
    if who not in ("gaussian", "uniform"):
        raise ValueError(f"noise_negatives: who must be gaussian or uniform, got {who!r}")
    if not isinstance(images, torch.Tensor) or images.dtype != torch.float32 or images.dim() != 4:
        raise ValueError("noise_negatives takes an fp32 batch, [B, 3, H, W] or NHWC4 [B, H, W, 4] (a uint8 batch is staged inside the "
                         "executor: use who = fgsm, or hand the loop fp32 batches)")
    nhwc4 = _is_nhwc4(images)
    if not nhwc4 and images.shape[1] != 3:
        raise ValueError("noise_negatives: expected [B, 3, H, W] or [B, H, W, 4]")
    x = images[..., :3].permute(0, 3, 1, 2) if nhwc4 else images
    B, _, H, W = x.shape
    draw = torch.randn if who == "gaussian" else torch.rand
    noise = draw((B, 3, H, W), generator=generator, device=images.device, dtype=torch.float32)
    if who == "uniform":
        noise = 2.0 * noise - 1.0
    out = torch.clamp(x.detach() + float(std_or_width) * noise, 0.0, 1.0)
    if not nhwc4:
        return out
    out4 = torch.zeros_like(images)
    out4[..., :3] = out.permute(0, 2, 3, 1)
    return out4


def negative_label(loss_type, n_classes):
    """The target of a generated negative: -1 under entropic / objectosphere, the background index under garbage. softmax has none
    (ignore_index = -1 would drop the whole second batch): ValueError."""
    if loss_type in ("entropic", "objectosphere"):
        return -1
    if loss_type == "garbage":
        return int(n_classes) - 1
    raise ValueError(f"adversarial negatives need a loss with a target for negatives (entropic, objectosphere, garbage), not {loss_type!r}")


def who_of(cfg):
    """cfg.adv.who, `no_adv` when the block or the key is absent; an unknown name is a ValueError."""
    adv = getattr(cfg, "adv", None)
    who = getattr(adv, "who", None) or "no_adv"
    if who not in WHO:
        raise ValueError(f"adv.who must be one of {WHO}, got {who!r}")
    return who


def scheduled_epsilon(adv, epoch):
    """max(min_epsilon, epsilon * mu ** (epoch // decay)) of the `adv` block; decay = 0 (or absent): constant epsilon."""
    eps = float(getattr(adv, "epsilon", 0.0) or 0.0)
    decay = int(getattr(adv, "decay", 0) or 0)
    if decay > 0:
        eps = eps * float(getattr(adv, "mu", 1.0)) ** (int(epoch) // decay)
    return max(float(getattr(adv, "min_epsilon", 0.0) or 0.0), eps)


class Plan:
    """What train() needs per step, fixed when the loop is set up: who, the strength (epsilon for fgsm, adv.std for gaussian, epsilon as
    the half-width for uniform), the loss type for the negative label, and the generator of the noise modes (adv.generator, optional)."""

    def __init__(self, cfg, epsilon=None):
        self.who = who_of(cfg)
        adv = cfg.adv
        self.loss_type = cfg.loss.type
        negative_label(self.loss_type, 2)     # refuses softmax here, before the first batch
        eps = float(getattr(adv, "epsilon", 0.0) or 0.0) if epsilon is None else float(epsilon)
        self.strength = float(getattr(adv, "std", 0.0) or 0.0) if self.who == "gaussian" else eps
        if not self.strength >= 0.0:
            raise ValueError("adv: epsilon / std must be >= 0")
        self.generator = getattr(adv, "generator", None)
        from .model import freeze_below_of
        if self.who == "fgsm" and freeze_below_of(cfg) is not None:
            # the loop asks for the adversarial batch after the clean forward, which by then has run the frozen prefix in the inference
            # form: there is no image gradient behind it (the noise modes need none)
            raise ValueError("adv.who: fgsm needs the image gradient through the whole network and cannot be combined with freeze_below; "
                             "use a noise mode (gaussian, uniform), or freeze by hand with train_only and freeze_bn")

    def labels(self, labels, n_logits):
        return torch.full_like(labels, negative_label(self.loss_type, n_logits))


def two_pass_step(model, net, images, labels, loss, plan, accumulate=False):
    """The clean and the adversarial pass of one step (between zero_grad() and optimizer.step()); returns (j, j_adv) detached.
    `loss(logits, features, labels)` is the loop's loss; `net` is the MI355X ResNet50 behind `model` (fused route), or None: any
    torch model on the autograd route. `accumulate`: this is a later micro-step of a gradient-accumulation group (train(), key
    opt.accumulate), so the clean pass adds to the gradients in place as well (autograd does that by itself)."""
    fgsm = plan.who == "fgsm"
    if net is None:
        x = images.detach().requires_grad_() if fgsm else images
        logits, features = model(x)
        j = loss(logits, features, labels)
        j.backward()
        negatives = fgsm_attack(x.detach(), x.grad, plan.strength) if fgsm else noise_negatives(images, plan.who, plan.strength, plan.generator)
        logits_n, features_n = model(negatives)
        j_adv = loss(logits_n, features_n, plan.labels(labels, logits_n.shape[1]))
        j_adv.backward()                      # autograd adds into p.grad
        return j.detach(), j_adv.detach()
    logits, features = model(images)
    j = loss(logits, features, labels)
    if fgsm or accumulate:
        net.next_backward(fgsm=plan.strength if fgsm else None, accumulate=accumulate)
    j.backward()
    negatives = net.adversarial_batch() if fgsm else noise_negatives(images, plan.who, plan.strength, plan.generator)
    logits_n, features_n = model(negatives)
    j_adv = loss(logits_n, features_n, plan.labels(labels, logits_n.shape[1]))
    net.next_backward(accumulate=True)        # into the second arena, then added to the clean gradients
    j_adv.backward()
    return j.detach(), j_adv.detach()
