"""Adversarial negatives for open-set training: FGSM, PGD and noise samples made from the batch in flight and trained as negatives,
and the same attacks on the validation batches.

Not in the reference snapshot (upstream's loop grew an `adv` block later: who / epsilon / decay), so the arithmetic is defined HERE,
as it is for the objectosphere loss. Per training step, when `cfg.adv.who` is not `no_adv` (train.train):

    logits, features = model(x);  j = loss(logits, y);  j.backward()                      the clean pass
    x_neg = fgsm_attack(x, dJ/dx, epsilon)      (who = fgsm)    or    noise_negatives(x, who, ...)   (who = gaussian | uniform)
            or K projected steps (who = pgd): step 1 is pgd_step(x, dJ/dx, x, alpha, epsilon) from the clean backward, steps 2..K are
            pgd_attack's input-only steps on the running statistics with x as the anchor
    logits_n, features_n = model(x_neg);  j_adv = loss(logits_n, negative label);  j_adv.backward()   gradients ADD to the clean ones
    optimizer.step()                                                                      one step on dJ/dp of J = j + j_adv

Both forwards run in training mode, so BatchNorm running statistics (and num_batches_tracked) are updated twice per step — what torch
does with two training-mode forwards, whatever K is: the inner steps of who = pgd read the running statistics and write nothing. j and
j_adv are each a mean over their own batch of B samples.

  fgsm_attack(images, grad, epsilon, lo=0., hi=1.)      clamp(x + epsilon * sign(grad), lo, hi) with torch ops on NCHW tensors: the
        documented semantics. On the MI355X ResNet50 the loop does not call it: the executor's backward ends in a stem input-gradient
        kernel whose epilogue applies exactly this formula to the NHWC4 batch the forward read (ResNet50.next_backward(fgsm=epsilon),
        osi_stem_dgrad_fgsm) — dJ/dx is never written, and NCHW, NHWC4 and uint8-staged batches are served alike.
  pgd_step(images, grad, anchor, alpha, epsilon, lo=0., hi=1.)
        clamp(min(max(x + alpha * sign(grad), a - epsilon), a + epsilon), lo, hi): one step of a projected attack from the iterate x,
        projected onto the epsilon-ball around the anchor a (the clean batch), torch ops on NCHW tensors, every operation one fp32
        rounding: the documented semantics, the counterpart of fgsm_attack. alpha < 0 descends; epsilon = 0 gives clamp(a); with
        a = x and 0 <= alpha <= epsilon it is fgsm_attack(x, grad, alpha). On the MI355X ResNet50 the same formula is the epilogue of
        the stem's input-gradient kernel (ResNet50.next_backward(pgd=(alpha, epsilon, anchor)), osi_stem_dgrad_pgd).
  as_nhwc4(images)       NCHW fp32, NHWC4 or uint8 [B, H, W, 3] -> an NHWC4 fp32 batch (uint8: value / 255, the bits the executor
        stages); made once per attack, it is the anchor of every step.
  pgd_attack(model, images, labels, loss, epsilon, alpha, steps, random_start=False, generator=None, lo=0., hi=1.)
        K steps ascending `loss(logits, features, labels)` on the TRUE labels, each a differentiable forward on the running statistics
        (eval mode for the duration: neither the statistics nor num_batches_tracked are touched; the model's mode is restored
        afterwards, also on an exception) and an INPUT-ONLY backward: no parameter gradient is computed, p.grad, the gradient arena
        and the optimizers' state are untouched, under data parallel no collective runs. On the MI355X ResNet50 every step is
        next_backward(pgd=..., input_only=True) + forward + backward ending in the PGD epilogue: the result is adversarial_batch()
        (NHWC4) and dJ/dx is never written. Any other model: torch.autograd.grad w.r.t. the iterate, then pgd_step; the result is
        NCHW. random_start: the iterate starts at clamp(x + epsilon * (2 * rand - 1), lo, hi), the noise drawn as ONE [B, 3, H, W]
        tensor from `generator`, as noise_negatives draws.
  noise_negatives(images, who, std_or_width, generator)  x + std * randn  |  x + width * (2 * rand - 1), clamped to [0, 1]. Torch ops
        on the batch's device; no gradient and no kernel of its own.
  negative_label(loss_type, n_classes)                  -1 (entropic, objectosphere) | n_classes - 1 (garbage: the background class)
  scheduled_epsilon(adv_cfg, epoch)                     max(min_epsilon, epsilon * mu ** (epoch // decay));  decay = 0: constant

validate() (train.py) scores every batch a second time under attack when the config holds `adv.validate: {who: fgsm | pgd, epsilon,
alpha, steps, random_start}` (validation_attack below): pgd_attack on the batch's own labels, fgsm = one step of alpha = epsilon. Under
the softmax loss the negatives (label -1, ignore_index) have no loss term, hence a zero gradient: they come back unperturbed (random
start aside).

Out of scope: "filter" mode (perturbing only the correctly classified known samples changes the batch size per step, and with it the
executor's geometry), targeted attacks, attacks through a freeze_below prefix.
"""
import math

import torch

WHO = ("no_adv", "fgsm", "pgd", "gaussian", "uniform")


def fgsm_attack(images, grad, epsilon, lo=0.0, hi=1.0):
    """clamp(images + epsilon * sign(grad), lo, hi) — NCHW tensors of one shape; sign is torch.sign (+1 / 0 / -1)."""
    if images.shape != grad.shape:
        raise ValueError("fgsm_attack: images and grad must have the same shape")
    if not float(epsilon) >= 0.0 or not float(lo) <= float(hi):
        raise ValueError("fgsm_attack: epsilon >= 0 and lo <= hi")
    return torch.clamp(images + float(epsilon) * torch.sign(grad), float(lo), float(hi))


def pgd_step(images, grad, anchor, alpha, epsilon, lo=0.0, hi=1.0):
    """clamp(min(max(images + alpha * sign(grad), anchor - epsilon), anchor + epsilon), lo, hi) — NCHW tensors of one shape; sign is
    torch.sign (+1 / 0 / -1), so alpha * sign is exact and every operation is one fp32 rounding."""
    if images.shape != grad.shape or images.shape != anchor.shape:
        raise ValueError("pgd_step: images, grad and anchor must have the same shape")
    if not math.isfinite(float(alpha)) or not float(epsilon) >= 0.0 or not float(lo) <= float(hi):
        raise ValueError("pgd_step: alpha finite, epsilon >= 0 and lo <= hi")
    moved = images + float(alpha) * torch.sign(grad)
    projected = torch.min(torch.max(moved, anchor - float(epsilon)), anchor + float(epsilon))
    return torch.clamp(projected, float(lo), float(hi))


def _is_nhwc4(images):
    return images.dtype == torch.float32 and images.dim() == 4 and images.shape[3] == 4 and images.shape[1] != 3


def as_nhwc4(images):
    """An NHWC4 fp32 batch [B, H, W, 4] (4th lane zero) from NCHW fp32 [B, 3, H, W], from uint8 [B, H, W, 3] (value / 255, a true
    division: the bits osi_u8hwc3_to_nhwc4 stages) or from an NHWC4 batch, which is returned as it is. A uint8 batch on the GPU goes
    through osi_u8hwc3_to_nhwc4 itself, the executor's own staging kernel: torch's device kernel for a division by a Python scalar
    multiplies by the rounded reciprocal, which is not the correctly rounded quotient for about half of the 256 byte values."""
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ValueError("as_nhwc4: expected a 4-D image batch")
    if images.dtype == torch.uint8:
        if images.shape[3] != 3:
            raise ValueError("as_nhwc4: a uint8 image batch must be [B, H, W, 3]")
        if images.is_cuda:
            from . import _native as N
            B, H, W, _ = images.shape
            src = images.contiguous()
            out = torch.empty(B, H, W, 4, dtype=torch.float32, device=images.device)
            with torch.cuda.device(images.device):
                N.check(N.lib().osi_u8hwc3_to_nhwc4(N.ptr(src), None, N.ptr(out), B, H, W, N.stream_of(src)), "osi_u8hwc3_to_nhwc4")
            return out
        out = torch.zeros(*images.shape[:3], 4, dtype=torch.float32, device=images.device)
        out[..., :3] = images.float().div(255)       # (the CPU kernel divides)
        return out
    if images.dtype != torch.float32:
        raise ValueError("as_nhwc4: expected an fp32 or uint8 batch")
    if _is_nhwc4(images):
        return images.detach()
    if images.shape[1] != 3:
        raise ValueError("as_nhwc4: expected [B, 3, H, W], [B, H, W, 4] or uint8 [B, H, W, 3]")
    B, _, H, W = images.shape
    out = torch.zeros(B, H, W, 4, dtype=torch.float32, device=images.device)
    out[..., :3] = images.detach().permute(0, 2, 3, 1)
    return out


def _mi355x_net(model):
    """the MI355X ResNet50 behind `model` (itself, or wrapped for data parallel), None for any other model"""
    from .model import ResNet50
    inner = getattr(model, "module", model)
    return inner if isinstance(inner, ResNet50) else None


def _pgd_steps(model, net, x, anchor, labels, loss, epsilon, alpha, steps, lo, hi):
    """`steps` input-only projected steps from the iterate x around `anchor`, on the running statistics (eval mode for the duration).
    net = the MI355X ResNet50 behind model: x is anything its forward takes, anchor NHWC4, the result adversarial_batch().
    net = None: x and anchor NCHW, autograd w.r.t. the iterate, pgd_step."""
    module = model if net is None else net
    was_training = module.training
    try:
        model.eval()
        with torch.enable_grad():
            for _ in range(steps):
                if net is not None:
                    net.next_backward(pgd=(alpha, epsilon, anchor), lo=lo, hi=hi, input_only=True)
                    logits, features = model(x)
                    loss(logits, features, labels).backward()
                    x = net.adversarial_batch()
                else:
                    xi = x.detach().requires_grad_()
                    logits, features = model(xi)
                    grad, = torch.autograd.grad(loss(logits, features, labels), xi)
                    x = pgd_step(xi.detach(), grad, anchor, alpha, epsilon, lo, hi)
    except BaseException:
        if net is not None:
            net._bw_request = None       # a request whose backward never ran must not reach a later one
        raise
    finally:
        model.train(was_training)
    return x


def pgd_attack(model, images, labels, loss, epsilon, alpha, steps, random_start=False, generator=None, lo=0.0, hi=1.0):
    """`steps` projected steps of size alpha ascending loss(logits, features, labels) from the clean batch (or a random start in its
    epsilon-ball), each projected onto the ball and clamped to [lo, hi]; see the module docstring. Returns the adversarial batch:
    NHWC4 (model-owned, ResNet50.adversarial_batch()) on the MI355X ResNet50, NCHW on any other model."""
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
        raise ValueError(f"pgd_attack: steps must be an integer >= 1, got {steps!r}")
    epsilon, alpha, lo, hi = float(epsilon), float(alpha), float(lo), float(hi)
    if not epsilon >= 0.0 or not math.isfinite(alpha) or not lo <= hi:
        raise ValueError("pgd_attack: epsilon >= 0, alpha finite and lo <= hi")
    net = _mi355x_net(model)
    anchor = as_nhwc4(images) if net is not None else images.detach()
    x = images if net is not None else anchor
    if random_start:
        clean = anchor[..., :3].permute(0, 3, 1, 2) if net is not None else anchor
        noise = torch.rand(clean.shape, generator=generator, device=clean.device, dtype=torch.float32)
        x = torch.clamp(clean + epsilon * (2.0 * noise - 1.0), lo, hi)
        if net is not None:
            x = as_nhwc4(x)
    return _pgd_steps(model, net, x, anchor, labels, loss, epsilon, alpha, steps, lo, hi)


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
    """cfg.adv.who, `no_adv` when the block or the key is absent; an unknown name is a ValueError, and so is who = pgd in a block
    without `steps` (the number of steps has no default: a PGD attack is defined by it)."""
    adv = getattr(cfg, "adv", None)
    who = getattr(adv, "who", None) or "no_adv"
    if who not in WHO:
        raise ValueError(f"adv.who must be one of {WHO}, got {who!r}")
    if who == "pgd" and getattr(adv, "steps", None) is None:
        raise ValueError("adv.who: pgd needs adv.steps (an integer >= 1)")
    return who


def scheduled_epsilon(adv, epoch):
    """max(min_epsilon, epsilon * mu ** (epoch // decay)) of the `adv` block; decay = 0 (or absent): constant epsilon."""
    eps = float(getattr(adv, "epsilon", 0.0) or 0.0)
    decay = int(getattr(adv, "decay", 0) or 0)
    if decay > 0:
        eps = eps * float(getattr(adv, "mu", 1.0)) ** (int(epoch) // decay)
    return max(float(getattr(adv, "min_epsilon", 0.0) or 0.0), eps)


def attack_steps(block, epsilon, base_epsilon=None):
    """(steps, alpha) of a block with the keys `steps` (integer >= 1, required) and `alpha` (finite; default epsilon / steps * 1.25).
    `epsilon` is the strength in force; a configured alpha is scaled by epsilon / base_epsilon when the two differ (the schedule)."""
    steps = getattr(block, "steps", None)
    if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
        raise ValueError(f"adv: steps must be an integer >= 1, got {steps!r}")
    alpha = getattr(block, "alpha", None)
    if alpha is None:
        alpha = epsilon / steps * 1.25
    else:
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float)) or not math.isfinite(alpha):
            raise ValueError(f"adv: alpha must be a finite number, got {alpha!r}")
        alpha = float(alpha)
        if base_epsilon is not None and base_epsilon > 0.0 and epsilon != base_epsilon:
            alpha = alpha * (epsilon / base_epsilon)
    return steps, alpha


class ValidationAttack:
    """The optional block `adv.validate: {who: fgsm | pgd, epsilon, alpha, steps, random_start}` of validate(), checked when the loop is
    set up. fgsm = one step of alpha = epsilon; `generator` (optional) feeds the random start."""

    def __init__(self, block):
        who = getattr(block, "who", None)
        if who not in ("fgsm", "pgd"):
            raise ValueError(f"adv.validate.who must be fgsm or pgd, got {who!r}")
        self.who = who
        self.epsilon = float(getattr(block, "epsilon", 0.0) or 0.0)
        if not self.epsilon >= 0.0:
            raise ValueError("adv.validate: epsilon must be >= 0")
        self.steps, self.alpha = (1, self.epsilon) if who == "fgsm" else attack_steps(block, self.epsilon)
        self.random_start = bool(getattr(block, "random_start", False))
        self.generator = getattr(block, "generator", None)

    def __call__(self, model, images, labels, loss):
        return pgd_attack(model, images, labels, loss, self.epsilon, self.alpha, self.steps, self.random_start, self.generator)


def validation_attack(cfg):
    """ValidationAttack of cfg.adv.validate, None when the block is absent."""
    block = getattr(getattr(cfg, "adv", None), "validate", None)
    return None if block is None else ValidationAttack(block)


class Plan:
    """What train() needs per step, fixed when the loop is set up: who, the strength (epsilon for fgsm and pgd, adv.std for gaussian,
    epsilon as the half-width for uniform), the loss type for the negative label, and the generator of the noise modes (adv.generator,
    optional). who = pgd: adv.steps (integer >= 1) and adv.alpha (default epsilon / steps * 1.25); an `epsilon` override (the scheduled
    value) scales a configured alpha by the same factor."""

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
        self.steps, self.alpha = 1, self.strength
        if self.who == "pgd":
            self.steps, self.alpha = attack_steps(adv, self.strength, float(getattr(adv, "epsilon", 0.0) or 0.0))
        from .model import freeze_below_of
        if self.who in ("fgsm", "pgd") and freeze_below_of(cfg) is not None:
            # the loop asks for the adversarial batch after the clean forward, which by then has run the frozen prefix in the inference
            # form: there is no image gradient behind it (the noise modes need none)
            raise ValueError(f"adv.who: {self.who} needs the image gradient through the whole network and cannot be combined with freeze_below; "
                             "use a noise mode (gaussian, uniform), or freeze by hand with train_only and freeze_bn")

    def labels(self, labels, n_logits):
        return torch.full_like(labels, negative_label(self.loss_type, n_logits))


def two_pass_step(model, net, images, labels, loss, plan, accumulate=False):
    """The clean and the adversarial pass of one step (between zero_grad() and optimizer.step()); returns (j, j_adv) detached.
    `loss(logits, features, labels)` is the loop's loss; `net` is the MI355X ResNet50 behind `model` (fused route), or None: any
    torch model on the autograd route. `accumulate`: this is a later micro-step of a gradient-accumulation group (train(), key
    opt.accumulate), so the clean pass adds to the gradients in place as well (autograd does that by itself)."""
    fgsm, pgd = plan.who == "fgsm", plan.who == "pgd"
    if net is None:
        x = images.detach().requires_grad_() if fgsm or pgd else images
        logits, features = model(x)
        j = loss(logits, features, labels)
        j.backward()
        if pgd:      # step 1 from the clean backward's dJ/dx, steps 2..K input-only on the running statistics
            negatives = pgd_step(x.detach(), x.grad, x.detach(), plan.alpha, plan.strength)
            if plan.steps > 1:
                negatives = _pgd_steps(model, None, negatives, x.detach(), labels, loss, plan.strength, plan.alpha, plan.steps - 1, 0.0, 1.0)
        else:
            negatives = fgsm_attack(x.detach(), x.grad, plan.strength) if fgsm else noise_negatives(images, plan.who, plan.strength, plan.generator)
        logits_n, features_n = model(negatives)
        j_adv = loss(logits_n, features_n, plan.labels(labels, logits_n.shape[1]))
        j_adv.backward()                      # autograd adds into p.grad
        return j.detach(), j_adv.detach()
    logits, features = model(images)
    j = loss(logits, features, labels)
    if pgd:          # step 1 rides on the clean training backward, as FGSM does: the anchor is the forward's own input
        net.next_backward(pgd=(plan.alpha, plan.strength, None), accumulate=accumulate)
    elif fgsm or accumulate:
        net.next_backward(fgsm=plan.strength if fgsm else None, accumulate=accumulate)
    j.backward()
    if pgd:
        negatives = net.adversarial_batch()
        if plan.steps > 1:
            negatives = _pgd_steps(model, net, negatives, as_nhwc4(images), labels, loss, plan.strength, plan.alpha, plan.steps - 1, 0.0, 1.0)
    else:
        negatives = net.adversarial_batch() if fgsm else noise_negatives(images, plan.who, plan.strength, plan.generator)
    logits_n, features_n = model(negatives)
    j_adv = loss(logits_n, features_n, plan.labels(labels, logits_n.shape[1]))
    net.next_backward(accumulate=True)        # into the second arena, then added to the clean gradients
    j_adv.backward()
    return j.detach(), j_adv.detach()
