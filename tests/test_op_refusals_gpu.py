"""What the torch.ops.osi.* bindings (csrc/osi_torch_ops.cpp) refuse, pinned op by op. The bindings are the only thing between a Python
caller and a raw-pointer kernel launch; this file holds one malformed call per check they make and asserts the RuntimeError, with the
op's or the argument's name in its text wherever the binding puts it there.

The table was derived by READING the bindings, never by trying calls: a case is listed only if the source shows the refusal in the
binding itself, before any launch through the C ABI. No call in this file is valid, so nothing launches; the parity tests make the
valid calls. Shapes are the smallest that are valid up to the mutated argument.

Per tensor argument that goes through the bindings' tensor check: wrong dtype, non-contiguous with the right shape, and misaligned by
one element where the required alignment exceeds the element size. Per size relation: broken once.

Left out because torch cannot construct them on one GPU:
  * a misaligned fp64 / int64 / int32 tensor whose required alignment is its element size (8-byte fp64 at a 4-byte offset: Tensor.view
    refuses the reinterpretation), and misaligned tensors of alignment 1;
  * a non-contiguous tensor of one element (grad_scale, info): every stride of a one-element tensor is contiguous;
  * tensors on different devices (the suite runs on one GPU);
  * an undefined tensor (None for a `Tensor` argument is refused by the dispatcher, not the binding);
  * empty tensor lists for average_update (without a tensor the dispatcher finds no kernel before the binding runs);
  * sizes above INT_MAX (several GiB per case)."""
import functools
import types

import numpy as np
import pytest
import torch

from openset_imagenet import _native as NL

pytestmark = pytest.mark.gpu

F32, F64, I64, I32, U8 = torch.float32, torch.float64, torch.int64, torch.int32, torch.uint8
SIZE = {F32: 4, F64: 8, I64: 8, I32: 4, U8: 1}


class T:
    """One tensor argument as the binding checks it: dtype, shape, required alignment in bytes (0: that of the element) and the name the
    message uses where it differs from the schema's. `mut` selects the malformed form."""

    def __init__(self, dtype, *shape, align=0, name=None, mut=None):
        self.dtype, self.shape, self.align, self.name, self.mut = dtype, shape, align, name, mut

    def mutated(self, mut):
        return T(self.dtype, *self.shape, align=self.align, name=self.name, mut=mut)

    def mutations(self):
        n = int(np.prod(self.shape))
        return ["dtype"] + (["strided"] if n > 1 else []) + (["offset"] if self.align > SIZE[self.dtype] else [])

    def build(self, dev):
        n = int(np.prod(self.shape))
        if self.mut == "dtype":
            return torch.zeros(self.shape, dtype=F64 if self.dtype is F32 else F32, device=dev)
        if self.mut == "strided":
            return torch.zeros(*self.shape[:-1], 2 * self.shape[-1], dtype=self.dtype, device=dev)[..., ::2]
        if self.mut == "offset":
            return torch.zeros(n + 1, dtype=self.dtype, device=dev)[1:].view(self.shape)
        return torch.zeros(self.shape, dtype=self.dtype, device=dev)


PHRASE = {"dtype": "dtype", "strided": "contiguous", "offset": "aligned"}
CASES = []


def tensors(v):
    return isinstance(v, T) or (isinstance(v, list) and bool(v) and isinstance(v[0], T))


def case(op, note, base, match, **swap):
    """One refusal: `base` is the op's valid argument list in schema order (name -> T, [T], a plain value or a callable of the
    environment), `swap` the malformed arguments, `match` a regular expression the message must contain (None: the check has no text)."""
    CASES.append(pytest.param(op, {**base, **swap}, match, id=f"{op}-{note}".replace(" ", "_")))


def needs(op, base, *names):
    """The dtype / contiguity / alignment refusals of the named tensor arguments (default: every T of `base`)."""
    for name in names or [k for k, v in base.items() if tensors(v)]:
        v = base[name]
        t = v[0] if isinstance(v, list) else v
        for mut in t.mutations():
            bad = t.mutated(mut)
            case(op, f"{name} {mut}", base, f"{t.name or name}.*{PHRASE[mut]}", **{name: [bad] + v[1:] if isinstance(v, list) else bad})


def E(attr):
    return lambda e: getattr(e, attr)


WS16, WS8, WS4 = T(U8, 1 << 16, align=16), T(U8, 1 << 16, align=8), T(U8, 1 << 16, align=4)
NULL = "null executor handle"

# ---- the executor ops without an executor: the tensor checks and the arena relation come before the handle is looked at ----------------
ARENA = dict(net=0, params=T(F32, 8, align=16), grads=T(F32, 8, align=16), workspace=WS16)
HEAD = dict(dlogits=T(F32, 2, 4), dfeatures=T(F32, 2, 4))
STAGES = dict(stage_lo=0, stage_hi=1)

fwd = dict(net=0, params=T(F32, 8, align=16), buffers=T(F32, 8, align=16), nbt=T(I64, 2, align=16, name="num_batches_tracked"),
           image=T(F32, 2, 3, 8, 8, align=16), flip=None, workspace=WS16, fc_dim=4, out_features=4, training=False)
needs("resnet50_forward", fwd, "params", "buffers", "nbt", "workspace")
case("resnet50_forward", "image 3-D", fwd, "osi::resnet50_forward.*image", image=T(F32, 3, 8, 8))
case("resnet50_forward", "null handle", fwd, NULL)
fwz = {k: v for k, v in fwd.items() if k not in ("nbt", "training")}
needs("resnet50_forward_frozen", fwz, "params", "buffers", "workspace")
case("resnet50_forward_frozen", "image 3-D", fwz, "image", image=T(F32, 3, 8, 8))
case("resnet50_forward_frozen", "null handle", fwz, NULL)

bwd = {**ARENA, **HEAD, **STAGES}
needs("resnet50_backward", bwd)
case("resnet50_backward", "grads numel", bwd, "osi::resnet50_backward.*gradient arena", grads=T(F32, 12, align=16))
case("resnet50_backward", "null handle", bwd, NULL)

bex = {**ARENA, **HEAD, "dimage": T(F32, 2, 3, 8, 8), "param_grads": True, **STAGES}
needs("resnet50_backward_ex", bex)
case("resnet50_backward_ex", "grads numel", bex, "osi::resnet50_backward_ex.*gradient arena", grads=T(F32, 12, align=16))
case("resnet50_backward_ex", "nothing requested", bex, "osi::resnet50_backward_ex.*neither dimage nor parameter", dimage=None, param_grads=False)
case("resnet50_backward_ex", "null handle", bex, NULL)

adv = {**ARENA, **HEAD, "x_adv": T(F32, 2, 8, 8, 4, align=16), "eps": 0.1, "lo": 0.0, "hi": 1.0, **STAGES}
needs("resnet50_backward_adv", adv)
case("resnet50_backward_adv", "grads numel", adv, "osi::resnet50_backward_adv.*gradient arena", grads=T(F32, 12, align=16))
case("resnet50_backward_adv", "null handle", adv, NULL)

atk = {**ARENA, **HEAD, "x_next": T(F32, 2, 8, 8, 4, align=16), "x_anchor": None, "alpha": 0.1, "eps": 0.1, "lo": 0.0, "hi": 1.0,
       "param_grads": True, **STAGES}
needs("resnet50_backward_attack", atk)
case("resnet50_backward_attack", "grads numel", atk, "osi::resnet50_backward_attack.*gradient arena", grads=T(F32, 12, align=16))
case("resnet50_backward_attack", "null handle", atk, NULL)

rdy = dict(net=0, grads=T(F32, 8, align=16), waiter_stream=0)
needs("resnet50_grads_ready", rdy)
case("resnet50_grads_ready", "null handle", rdy, NULL)
case("resnet50_set_bn_momentum", "null handle", dict(net=0, momentum=0.1), NULL)
pld = dict(net=0, workspace=WS16)
needs("resnet50_pooled", pld)
case("resnet50_pooled", "null handle", pld, NULL)
case("resnet50_set_mix", "null handle", dict(net=0, partner=None, weight=None), NULL)

# ---- the executor ops on a real executor: the checks that sit after a handle query (arena sizes, geometry) -----------------------------
rfw = dict(net=E("h"), params=E("params"), buffers=E("buffers"), nbt=E("nbt"), image=E("image"), flip=None, workspace=E("ws"),
           fc_dim=E("F"), out_features=E("O"), training=False)
rfz = {k: v for k, v in rfw.items() if k not in ("nbt", "training")}
for op, base in (("resnet50_forward", rfw), ("resnet50_forward_frozen", rfz)):
    case(op, "workspace one byte short", base, "osi::resnet50_forward.*workspace too small", workspace=lambda e: e.ws[:-1])
    case(op, "params numel", base, "osi::resnet50_forward.*parameter arena", params=lambda e: e.params[:-4])
    case(op, "buffers numel", base, "osi::resnet50_forward.*buffer arena", buffers=lambda e: e.buffers[:-4])
    case(op, "batch off by one", base, "osi::resnet50_forward.*geometry", image=lambda e: e.zeros(F32, e.B + 1, 3, e.H, e.W))
    case(op, "height off by one", base, "osi::resnet50_forward.*geometry", image=lambda e: e.zeros(F32, e.B, 3, e.H + 1, e.W))
    case(op, "fp32 image dtype", base, "image.*dtype", image=lambda e: e.zeros(F64, e.B, 3, e.H, e.W))
    case(op, "fp32 image strided", base, "image.*contiguous", image=lambda e: e.zeros(F32, e.B, 3, e.H, 2 * e.W)[..., ::2])
    case(op, "fp32 image offset", base, "image.*aligned", image=lambda e: e.zeros(F32, e.B * 3 * e.H * e.W + 1)[1:].view(e.B, 3, e.H, e.W))
    case(op, "fp32 image 2 planes", base, "image", image=lambda e: e.zeros(F32, e.B, 2, e.H, e.W))
    case(op, "nhwc4 image strided", base, "image.*contiguous", image=lambda e: e.zeros(F32, e.B, e.H, e.W, 8)[..., ::2])
    case(op, "nhwc4 image offset", base, "image.*aligned", image=lambda e: e.zeros(F32, e.B * e.H * e.W * 4 + 1)[1:].view(e.B, e.H, e.W, 4))
    case(op, "u8 image strided", base, "image.*contiguous", image=lambda e: e.zeros(U8, e.B, e.H, e.W, 6)[..., ::2])
    case(op, "u8 image offset", base, "image.*aligned", image=lambda e: e.zeros(U8, e.B * e.H * e.W * 3 + 1)[1:].view(e.B, e.H, e.W, 3))
    case(op, "u8 image 2 channels", base, "image", image=lambda e: e.zeros(U8, e.B, e.H, e.W, 2))
    u8 = {**base, "image": lambda e: e.zeros(U8, e.B, e.H, e.W, 3)}
    case(op, "flip dtype", u8, "flip.*dtype", flip=lambda e: e.zeros(F32, e.B))
    case(op, "flip strided", u8, "flip.*contiguous", flip=lambda e: e.zeros(U8, 2 * e.B)[::2])
    case(op, "flip offset", u8, "flip.*aligned", flip=lambda e: e.zeros(U8, e.B + 1)[1:])
    case(op, "flip numel", u8, None, flip=lambda e: e.zeros(U8, e.B + 1))
case("resnet50_forward", "nbt numel", rfw, "osi::resnet50_forward.*num_batches_tracked", nbt=lambda e: e.nbt[:-2])

rar = dict(net=E("h"), params=E("params"), grads=E("grads"), workspace=E("ws"), dlogits=lambda e: e.zeros(F32, e.B, e.O),
           dfeatures=None)
rex = {**rar, "dimage": lambda e: e.zeros(F32, e.B, 3, e.H, e.W), "param_grads": True, **STAGES}
case("resnet50_backward_ex", "dimage batch off by one", rex, "osi::resnet50_backward_ex.*dimage", dimage=lambda e: e.zeros(F32, e.B + 1, 3, e.H, e.W))
case("resnet50_backward_ex", "dimage NHWC4", rex, "osi::resnet50_backward_ex.*dimage", dimage=lambda e: e.zeros(F32, e.B, e.H, e.W, 4))
rad = {**rar, "x_adv": lambda e: e.zeros(F32, e.B, e.H, e.W, 4), "eps": 0.1, "lo": 0.0, "hi": 1.0, **STAGES}
case("resnet50_backward_adv", "x_adv width off by one", rad, "osi::resnet50_backward_adv.*x_adv", x_adv=lambda e: e.zeros(F32, e.B, e.H, e.W + 1, 4))
case("resnet50_backward_adv", "x_adv NCHW", rad, "osi::resnet50_backward_adv.*x_adv", x_adv=lambda e: e.zeros(F32, e.B, 3, e.H, e.W))
rat = {**rar, "x_next": lambda e: e.zeros(F32, e.B, e.H, e.W, 4), "x_anchor": lambda e: e.zeros(F32, e.B, e.H, e.W, 4), "alpha": 0.1,
       "eps": 0.1, "lo": 0.0, "hi": 1.0, "param_grads": True, **STAGES}
case("resnet50_backward_attack", "x_next batch off by one", rat, "osi::resnet50_backward_attack.*x_next", x_next=lambda e: e.zeros(F32, e.B + 1, e.H, e.W, 4))
case("resnet50_backward_attack", "x_anchor dtype", rat, "x_anchor.*dtype", x_anchor=lambda e: e.zeros(F64, e.B, e.H, e.W, 4))
case("resnet50_backward_attack", "x_anchor strided", rat, "x_anchor.*contiguous", x_anchor=lambda e: e.zeros(F32, e.B, e.H, e.W, 8)[..., ::2])
case("resnet50_backward_attack", "x_anchor offset", rat, "x_anchor.*aligned", x_anchor=lambda e: e.zeros(F32, e.B * e.H * e.W * 4 + 1)[1:].view(e.B, e.H, e.W, 4))
case("resnet50_backward_attack", "x_anchor height off by one", rat, "osi::resnet50_backward_attack.*x_anchor", x_anchor=lambda e: e.zeros(F32, e.B, e.H + 1, e.W, 4))
case("resnet50_pooled", "workspace one byte short", dict(net=E("h"), workspace=lambda e: e.ws[:-1]), "osi::resnet50_pooled.*workspace too small")
rmx = dict(net=E("h"), partner=lambda e: e.zeros(I32, e.B), weight=lambda e: e.zeros(F32, e.B))
case("resnet50_set_mix", "partner alone", rmx, "osi::resnet50_set_mix.*go together", weight=None)
case("resnet50_set_mix", "partner dtype", rmx, "partner.*dtype", partner=lambda e: e.zeros(I64, e.B))
case("resnet50_set_mix", "partner strided", rmx, "partner.*contiguous", partner=lambda e: e.zeros(I32, 2 * e.B)[::2])
case("resnet50_set_mix", "weight dtype", rmx, "weight.*dtype", weight=lambda e: e.zeros(F64, e.B))
case("resnet50_set_mix", "weight strided", rmx, "weight.*contiguous", weight=lambda e: e.zeros(F32, 2 * e.B)[::2])
case("resnet50_set_mix", "partner numel", rmx, "osi::resnet50_set_mix.*one entry per row", partner=lambda e: e.zeros(I32, e.B + 1))
case("resnet50_set_mix", "weight numel", rmx, "osi::resnet50_set_mix.*one entry per row", weight=lambda e: e.zeros(F32, e.B - 1))

# ---- attack step, arenas, optimizers, staging, metrics ---------------------------------------------------------------------------------
pgd = dict(dy=T(F32, 1, 2, 2, 64, align=16), w_krsc3=T(F32, 64 * 7 * 7 * 3), x_cur=T(F32, 1, 4, 4, 4, align=16),
           x_anchor=T(F32, 1, 4, 4, 4, align=16), x_next=T(F32, 1, 4, 4, 4, align=16), alpha=0.1, eps=0.1, lo=0.0, hi=1.0)
needs("stem_dgrad_pgd", pgd)
case("stem_dgrad_pgd", "x_cur 3 channels", pgd, "osi::stem_dgrad_pgd.*x_cur", x_cur=T(F32, 1, 4, 4, 3), x_anchor=T(F32, 1, 4, 4, 3), x_next=T(F32, 1, 4, 4, 3))
case("stem_dgrad_pgd", "x_anchor shape", pgd, "osi::stem_dgrad_pgd.*shape", x_anchor=T(F32, 1, 4, 8, 4))
case("stem_dgrad_pgd", "x_next shape", pgd, "osi::stem_dgrad_pgd.*shape", x_next=T(F32, 2, 4, 4, 4))
case("stem_dgrad_pgd", "dy rows", pgd, "osi::stem_dgrad_pgd.*dy", dy=T(F32, 1, 3, 2, 64))
case("stem_dgrad_pgd", "dy channels", pgd, "osi::stem_dgrad_pgd.*dy", dy=T(F32, 1, 2, 2, 32))
case("stem_dgrad_pgd", "w numel", pgd, "osi::stem_dgrad_pgd.*w_krsc3", w_krsc3=T(F32, 64 * 7 * 7 * 3 + 1))

acc = dict(dst=T(F32, 8, align=16), src=T(F32, 8, align=16))
needs("grad_accumulate", acc)
case("grad_accumulate", "src numel", acc, "osi::grad_accumulate", src=T(F32, 12, align=16))

avg = dict(avg=[T(F32, 8, align=16)], cur=[T(F32, 8, align=16)], weight=0.5)
needs("average_update", avg)
case("average_update", "one more current", avg, "osi::average_update", cur=[T(F32, 8), T(F32, 8)])
case("average_update", "too many pairs", avg, "osi::average_update", avg=[T(F32, 8)] * (NL.AVG_MAX_SPANS + 1), cur=[T(F32, 8)] * (NL.AVG_MAX_SPANS + 1))
case("average_update", "pair numel", avg, "osi::average_update.*pair", cur=[T(F32, 12)])

lss = dict(mode=0, logits=T(F32, 2, 4), target=T(I64, 2), unk_weight=1.0, ignore_index=-100, class_weights=T(F32, 4), features=T(F32, 2, 8),
           xi=1.0, alpha=1.0, need_grad=True)
needs("loss_fwd_bwd", lss)
case("loss_fwd_bwd", "logits 1-D", lss, "logits", logits=T(F32, 8))
case("loss_fwd_bwd", "target rows", lss, "logits", target=T(I64, 3))
case("loss_fwd_bwd", "class_weights numel", lss, None, class_weights=T(F32, 5))
case("loss_fwd_bwd", "features rows", lss, None, features=T(F32, 3, 8))
case("loss_fwd_bwd", "features 1-D", lss, None, features=T(F32, 2))

P16 = T(F32, 8, align=16)
adm = dict(params=P16, grads=P16, exp_avg=P16, exp_avg_sq=P16, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_scale=1.0)
needs("adam_step", adm)
for k in ("grads", "exp_avg", "exp_avg_sq"):
    case("adam_step", f"{k} numel", adm, None, **{k: T(F32, 12)})
sgd = dict(params=P16, grads=P16, momentum_buffer=P16, lr=1e-3, momentum=0.9, first=True, grad_scale=1.0)
needs("sgd_step", sgd)
for k in ("grads", "momentum_buffer"):
    case("sgd_step", f"{k} numel", sgd, None, **{k: T(F32, 12)})

SEG = [0, 2, 0]                                      # one (begin4, end4, group) triple over the 8 floats
AG = [1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 0.0, 1.0, 0.0]   # (lr, beta1, beta2, eps, weight_decay, step, decoupled, amsgrad, maximize)
SG = [1e-3, 0.9, 0.0, 0.0, 0.0, 1.0, 0.0]            # (lr, momentum, dampening, weight_decay, nesterov, first_step, maximize)
SCALAR = T(F32, 1, name="grad_scale")
for op, scale in (("adam_step_groups", 1.0), ("adam_step_groups_dev", SCALAR)):
    g = dict(params=P16, grads=P16, exp_avg=P16, exp_avg_sq=P16, max_exp_avg_sq=P16, segments=SEG, groups=AG, grad_scale=scale)
    needs(op, g)
    for k in ("grads", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
        case(op, f"{k} numel", g, None, **{k: T(F32, 12)})
    case(op, "groups row short", g, "groups", groups=AG[:-1])
    case(op, "segments not triples", g, "segments", segments=SEG + [0])
    case(op, "segment begin negative", g, "segment", segments=[-1, 2, 0])
    case(op, "segment end beyond 32 bits", g, "segment", segments=[0, 1 << 32, 0])
    case(op, "segment group negative", g, "segment", segments=[0, 2, -1])
    case(op, "segment group too large", g, "segment", segments=[0, 2, NL.OPT_MAX_GROUPS])
for op, scale in (("sgd_step_groups", 1.0), ("sgd_step_groups_dev", SCALAR)):
    g = dict(params=P16, grads=P16, momentum_buffer=P16, segments=SEG, groups=SG, grad_scale=scale)
    needs(op, g)
    for k in ("grads", "momentum_buffer"):
        case(op, f"{k} numel", g, None, **{k: T(F32, 12)})
    case(op, "groups row short", g, "groups", groups=SG[:-1])
    case(op, "segments not triples", g, "segments", segments=SEG + [0])
    case(op, "segment begin negative", g, "segment", segments=[-1, 2, 0])
    case(op, "segment group too large", g, "segment", segments=[0, 2, NL.OPT_MAX_GROUPS])
for op, g in (("adam_step_groups_dev", dict(params=P16, grads=P16, exp_avg=P16, exp_avg_sq=P16, max_exp_avg_sq=None, segments=SEG, groups=AG,
                                            grad_scale=SCALAR)),
              ("sgd_step_groups_dev", dict(params=P16, grads=P16, momentum_buffer=P16, segments=SEG, groups=SG, grad_scale=SCALAR))):
    case(op, "grad_scale two elements", g, "grad_scale", grad_scale=T(F32, 2))

clp = dict(grads=T(F32, 8, align=16), spans=[], norm_type=2, grad_scale=1.0, max_norm=1.0, workspace=WS16, out2=T(F32, 2))
needs("grad_clip_scale", clp)
case("grad_clip_scale", "out2 numel", clp, "osi::grad_clip_scale.*out2", out2=T(F32, 3))
case("grad_clip_scale", "workspace one byte short", clp, "osi::grad_clip_scale.*workspace too small",
     workspace=lambda e: e.zeros(U8, NL.lib().osi_grad_norm_workspace(8) - 1))
case("grad_clip_scale", "spans not pairs", clp, "spans", spans=[0, 4, 4])
case("grad_clip_scale", "span begin negative", clp, "span", spans=[-1, 4])
case("grad_clip_scale", "span numel negative", clp, "span", spans=[0, -4])

cnv = dict(canvas=T(U8, 2, 8, 8, 3, align=16), crop_xy=T(I32, 4), flip=T(U8, 2), H=4, W=4)
needs("stage_canvas", cnv)
case("stage_canvas", "canvas 3-D", cnv, "canvas", canvas=T(U8, 8, 8, 3))
case("stage_canvas", "canvas 4 channels", cnv, "canvas", canvas=T(U8, 2, 8, 8, 4))
case("stage_canvas", "crop_xy numel", cnv, None, crop_xy=T(I32, 5))
case("stage_canvas", "flip numel", cnv, None, flip=T(U8, 3))

needs("softmax", dict(logits=T(F32, 2, 4)))
case("softmax", "logits 1-D", dict(logits=T(F32, 8)), None)
cnf = dict(logits=T(F32, 2, 4), target=T(I64, 2), offset=0.0, unknown_class=-1, last_valid_class=3, acc4=T(F64, 4))
needs("confidence_accumulate", cnf)
case("confidence_accumulate", "logits 1-D", cnf, None, logits=T(F32, 8))
case("confidence_accumulate", "target numel", cnf, None, target=T(I64, 3))
case("confidence_accumulate", "acc4 numel", cnf, None, acc4=T(F64, 5))

# ---- OpenMax: natural alignment throughout, the binding itself compares the workspace size ------------------------------------------
omm = dict(features=T(F32, 4, 8), logits=T(F32, 4, 4), gt=T(I64, 4), workspace=WS4)
needs("openmax_class_means", omm)
case("openmax_class_means", "features 1-D", omm, "osi::openmax_class_means", features=T(F32, 4))
case("openmax_class_means", "gt 2-D", omm, "osi::openmax_class_means", gt=T(I64, 4, 1))
case("openmax_class_means", "logits rows", omm, "osi::openmax_class_means.*rows", logits=T(F32, 5, 4))
case("openmax_class_means", "gt rows", omm, "osi::openmax_class_means.*rows", gt=T(I64, 3))
case("openmax_class_means", "workspace one byte short", omm, "osi::openmax_class_means.*workspace too small",
     workspace=lambda e: e.zeros(U8, NL.lib().osi_openmax_workspace(4, 4, 8) - 1))
omd = dict(features=T(F32, 4, 8), mav=T(F32, 4, 8), cls=T(I64, 4), metric=0)
needs("openmax_distances", omd)
case("openmax_distances", "mav columns", omd, "osi::openmax_distances", mav=T(F32, 4, 7))
case("openmax_distances", "features 1-D", omd, "osi::openmax_distances", features=T(F32, 8))
case("openmax_distances", "cls 2-D", omd, "osi::openmax_distances.*cls", cls=T(I64, 4, 1))
case("openmax_distances", "cls rows", omd, "osi::openmax_distances.*rows", cls=T(I64, 5))
omf = dict(dist=T(F32, 4), gt=T(I64, 4), correct=T(U8, 4), C=4, tailsize=2, workspace=WS4)
needs("openmax_fit_tails", omf)
case("openmax_fit_tails", "dist 2-D", omf, "osi::openmax_fit_tails", dist=T(F32, 4, 1))
case("openmax_fit_tails", "gt rows", omf, "osi::openmax_fit_tails.*rows", gt=T(I64, 5))
case("openmax_fit_tails", "correct rows", omf, "osi::openmax_fit_tails.*rows", correct=T(U8, 3))
case("openmax_fit_tails", "C zero", omf, "osi::openmax_fit_tails.*C", C=0)
case("openmax_fit_tails", "C beyond int", omf, "osi::openmax_fit_tails.*C", C=1 << 31)
case("openmax_fit_tails", "workspace one byte short", omf, "osi::openmax_fit_tails.*workspace too small",
     workspace=lambda e: e.zeros(U8, NL.lib().osi_openmax_workspace(4, 4, 1) - 1))
omw = dict(dist=T(F32, 2, 4), shape=T(F64, 4), scale=T(F64, 4), shift=T(F64, 4), fitted=T(U8, 4))
needs("openmax_wscores", omw)
case("openmax_wscores", "dist 1-D", omw, "osi::openmax_wscores.*dist", dist=T(F32, 4))
for k in ("shape", "scale", "shift"):
    case("openmax_wscores", f"{k} numel", omw, "osi::openmax_wscores.*one entry per column", **{k: T(F64, 5)})
case("openmax_wscores", "fitted numel", omw, "osi::openmax_wscores.*one entry per column", fitted=T(U8, 3))
omr = dict(logits=T(F32, 2, 4), w=T(F32, 2, 4), alpha=2)
needs("openmax_recalibrate", omr)
case("openmax_recalibrate", "w columns", omr, "osi::openmax_recalibrate", w=T(F32, 2, 5))
case("openmax_recalibrate", "logits 1-D", omr, "osi::openmax_recalibrate", logits=T(F32, 8), w=T(F32, 8))
case("openmax_recalibrate", "alpha zero", omr, "osi::openmax_recalibrate.*alpha", alpha=0)

# ---- the Extreme Value Machine: workspace 8-byte aligned ------------------------------------------------------------------------------
evd = dict(a=T(F32, 2, 8), b=T(F32, 4, 8), metric=0, workspace=WS8)
needs("evm_distances", evd)
case("evm_distances", "b columns", evd, "osi::evm_distances", b=T(F32, 4, 7))
case("evm_distances", "a 1-D", evd, "osi::evm_distances", a=T(F32, 8))
evf = dict(dist=T(F32, 2, 4), gt=T(I64, 4), cls=0, tailsize=2, multiplier=0.5, workspace=WS8)
needs("evm_fit_rows", evf)
case("evm_fit_rows", "gt longer than a row", evf, "osi::evm_fit_rows", gt=T(I64, 5))
case("evm_fit_rows", "dist 1-D", evf, "osi::evm_fit_rows", dist=T(F32, 8))
evc = dict(dpp=T(F32, 4, 4), shape=T(F64, 4), scale=T(F64, 4), shift=T(F64, 4), fitted=T(U8, 4), multiplier=0.5, cover_threshold=0.5,
           workspace=WS8)
needs("evm_set_cover", evc)
case("evm_set_cover", "dpp not square", evc, "osi::evm_set_cover.*dpp", dpp=T(F32, 4, 5))
for k in ("shape", "scale", "shift"):
    case("evm_set_cover", f"{k} numel", evc, "osi::evm_set_cover.*shape, scale and shift", **{k: T(F64, 5)})
case("evm_set_cover", "fitted numel", evc, "osi::evm_set_cover.*fitted", fitted=T(U8, 3))
evp = dict(dist=T(F32, 2, 4), shape=T(F64, 4), scale=T(F64, 4), shift=T(F64, 4), ev_start=T(I64, 3), multiplier=0.5)
needs("evm_probs", evp)
case("evm_probs", "dist 1-D", evp, "osi::evm_probs", dist=T(F32, 8))
case("evm_probs", "ev_start one entry", evp, "osi::evm_probs.*ev_start", ev_start=T(I64, 1))
case("evm_probs", "scale numel", evp, "osi::evm_probs.*shape, scale and shift", scale=T(F64, 3))
case("evm_probs", "shift numel", evp, "osi::evm_probs.*shape, scale and shift", shift=T(F64, 5))
case("evm_probs", "more values than columns", evp, "osi::evm_probs", shape=T(F64, 5), scale=T(F64, 5), shift=T(F64, 5))

# ---- deep nearest neighbours -------------------------------------------------------------------------------------------------------------
knt = dict(dist=T(F32, 2, 4), k=1, skip=T(I64, 2), workspace=WS8)
needs("knn_topk", knt)
case("knn_topk", "dist 1-D", knt, "osi::knn_topk", dist=T(F32, 8))
case("knn_topk", "k zero", knt, "osi::knn_topk.*k must", k=0)
case("knn_topk", "k beyond the maximum", knt, "osi::knn_topk.*k must", k=NL.KNN_MAX_K + 1)
case("knn_topk", "skip numel", knt, "osi::knn_topk.*skip", skip=T(I64, 3))
knc = dict(dist=T(F32, 2, 4), start=T(I64, 3), k=1, skip=T(I64, 2), transform=0, workspace=WS8)
needs("knn_class_kth", knc)
case("knn_class_kth", "dist 1-D", knc, "osi::knn_class_kth", dist=T(F32, 8))
case("knn_class_kth", "start one entry", knc, "osi::knn_class_kth.*start", start=T(I64, 1))
case("knn_class_kth", "start 2-D", knc, "osi::knn_class_kth.*start", start=T(I64, 3, 1))
case("knn_class_kth", "k zero", knc, "osi::knn_class_kth.*k must", k=0)
case("knn_class_kth", "k beyond the maximum", knc, "osi::knn_class_kth.*k must", k=NL.KNN_MAX_K + 1)
case("knn_class_kth", "skip numel", knc, "osi::knn_class_kth.*skip", skip=T(I64, 1))

# ---- Mahalanobis ---------------------------------------------------------------------------------------------------------------------
mcm = dict(features=T(F32, 4, 8), gt=T(I64, 4), C=2, workspace=WS8)
needs("maha_class_means", mcm)
case("maha_class_means", "gt numel", mcm, "osi::maha_class_means", gt=T(I64, 5))
case("maha_class_means", "features 1-D", mcm, "osi::maha_class_means", features=T(F32, 4), gt=T(I64, 4))
case("maha_class_means", "no rows", mcm, "osi::maha_class_means", features=T(F32, 0, 8), gt=T(I64, 0))
case("maha_class_means", "C zero", mcm, "osi::maha_class_means", C=0)
msc = dict(features=T(F32, 4, 8), gt=T(I64, 4), mean=T(F64, 3, 8, align=8), mode=0, accumulate=False, S=T(F64, 8, 8, align=8), workspace=WS8)
needs("maha_scatter", msc)
case("maha_scatter", "gt numel", msc, "osi::maha_scatter", gt=T(I64, 3))
case("maha_scatter", "mean one row", msc, "osi::maha_scatter.*mean", mean=T(F64, 1, 8))
case("maha_scatter", "mean columns", msc, "osi::maha_scatter.*mean", mean=T(F64, 3, 7))
case("maha_scatter", "S not square", msc, "osi::maha_scatter.*S", S=T(F64, 8, 7))
case("maha_scatter", "S of another size", msc, "osi::maha_scatter.*S", S=T(F64, 7, 7))
mfa = dict(S=T(F64, 8, 8, align=8), scale=1.0, shrinkage=0.0, workspace=WS8)
needs("maha_factor", mfa)
case("maha_factor", "S not square", mfa, "osi::maha_factor.*S", S=T(F64, 8, 7))
case("maha_factor", "S empty", mfa, "osi::maha_factor", S=T(F64, 0, 0))
mwh = dict(x=T(F32, 2, 8), W=T(F64, 8, 8, align=8), workspace=WS8)
needs("maha_whiten", mwh, "W", "workspace")
case("maha_whiten", "x int64", mwh, "osi::maha_whiten.*x", x=lambda e: e.zeros(I64, 2, 8))
case("maha_whiten", "x strided", mwh, "x.*contiguous", x=T(F32, 2, 8, mut="strided"))
case("maha_whiten", "x fp64 strided", mwh, "x.*contiguous", x=T(F64, 2, 8, mut="strided"))
case("maha_whiten", "W not square", mwh, "osi::maha_whiten.*W", W=T(F64, 8, 7))
case("maha_whiten", "W of another size", mwh, "osi::maha_whiten.*W", W=T(F64, 7, 7))
msq = dict(z=T(F64, 2, 8, align=8), zm=T(F64, 3, 8, align=8), minus=T(F64, 2, align=8), transform=0, f64_out=True, workspace=WS8)
needs("maha_sqdist", msq)
case("maha_sqdist", "zm columns", msq, "osi::maha_sqdist.*zm", zm=T(F64, 3, 7))
case("maha_sqdist", "minus numel", msq, "osi::maha_sqdist.*minus", minus=T(F64, 3))
case("maha_sqdist", "no classes", msq, "osi::maha_sqdist", zm=T(F64, 0, 8))

# ---- the eigensolver and ViM ------------------------------------------------------------------------------------------------------------
SQ = T(F64, 4, 4, align=8)
egb = dict(S=SQ, workspace=WS8)
needs("eigh_begin", egb)
case("eigh_begin", "S not square", egb, "osi::eigh_begin.*S", S=T(F64, 4, 5))
egs = dict(A=SQ, Vt=SQ, head=T(F64, 2, align=8), info=T(I32, 1), workspace=WS8)
needs("eigh_sweep", egs)
case("eigh_sweep", "A not square", egs, "osi::eigh_sweep.*A", A=T(F64, 4, 5), Vt=T(F64, 4, 5))
case("eigh_sweep", "Vt of another size", egs, "osi::eigh_sweep.*Vt", Vt=T(F64, 5, 5))
case("eigh_sweep", "head numel", egs, "osi::eigh_sweep.*head", head=T(F64, 3))
case("eigh_sweep", "info numel", egs, "osi::eigh_sweep.*info", info=T(I32, 2))
egf = dict(A=SQ, Vt=SQ, info=T(I32, 1), workspace=WS8)
needs("eigh_finish", egf)
case("eigh_finish", "A not square", egf, "osi::eigh_finish.*A", A=T(F64, 4, 5), Vt=T(F64, 4, 5))
case("eigh_finish", "Vt of another size", egf, "osi::eigh_finish.*Vt", Vt=T(F64, 3, 3))
case("eigh_finish", "info numel", egf, "osi::eigh_finish.*info", info=T(I32, 2))
vpr = dict(x=T(F32, 2, 8), origin=T(F64, 8, align=8), R=T(F64, 3, 8, align=8), workspace=WS8)
needs("vim_project", vpr)
case("vim_project", "R columns", vpr, "osi::vim_project.*R", R=T(F64, 3, 7))
case("vim_project", "origin numel", vpr, "osi::vim_project.*origin", origin=T(F64, 7))
case("vim_project", "x 1-D", vpr, "osi::vim_project.*x", x=T(F32, 8))
vsc = dict(z=T(F64, 2, 4, align=8), logits=T(F32, 2, 4), alpha=1.0, mode=0, f64_out=True, workspace=WS8)
needs("vim_scores", vsc)
case("vim_scores", "z 1-D", vsc, "osi::vim_scores.*z", z=T(F64, 8))
case("vim_scores", "logits rows", vsc, "osi::vim_scores.*logits", logits=T(F32, 3, 4))
case("vim_scores", "logits 1-D", vsc, "osi::vim_scores.*logits", logits=T(F32, 2))
case("vim_scores", "no components", vsc, "osi::vim_scores", z=T(F64, 2, 0))

# ---- activation shaping -----------------------------------------------------------------------------------------------------------------
ost = dict(v=T(F32, 8), ranks=[0, 7], workspace=WS8)
needs("order_stats", ost)
case("order_stats", "v empty", ost, "osi::order_stats.*v", v=T(F32, 0))
case("order_stats", "no ranks", ost, "osi::order_stats.*ranks", ranks=[])
case("order_stats", "nine ranks", ost, "osi::order_stats.*ranks", ranks=list(range(NL.ORDER_STATS_MAX_R + 1)), v=T(F32, 16))
case("order_stats", "rank equal to numel", ost, "osi::order_stats.*rank", ranks=[0, 8])
case("order_stats", "rank negative", ost, "osi::order_stats.*rank", ranks=[-1])
shr = dict(x=T(F32, 2, 8), mode=0, keep=4, clip=1.0, workspace=WS8)
needs("shape_rows", shr)
case("shape_rows", "x 1-D", shr, "osi::shape_rows.*x", x=T(F32, 8))
case("shape_rows", "no columns", shr, "osi::shape_rows", x=T(F32, 2, 0))
lgs = dict(logits=T(F32, 2, 4), mode=0)
needs("logit_scores", lgs)
case("logit_scores", "logits 1-D", lgs, "osi::logit_scores.*logits", logits=T(F32, 8))
case("logit_scores", "no rows", lgs, "osi::logit_scores", logits=T(F32, 0, 4))

# ---- PROSER and the small dense layer -----------------------------------------------------------------------------------------------------
mix = dict(x=T(F32, 4, 8, align=16), partner=T(I32, 4), weight=T(F32, 4))
needs("mix_rows_pairs", mix)
case("mix_rows_pairs", "x 1-D", mix, "osi::mix_rows_pairs.*x", x=T(F32, 8))
case("mix_rows_pairs", "x empty", mix, "osi::mix_rows_pairs.*x", x=T(F32, 4, 0))
case("mix_rows_pairs", "row of 6", mix, "osi::mix_rows_pairs.*multiple of 4", x=T(F32, 4, 6))
case("mix_rows_pairs", "partner numel", mix, "osi::mix_rows_pairs.*one entry per row", partner=T(I32, 3))
case("mix_rows_pairs", "weight numel", mix, "osi::mix_rows_pairs.*one entry per row", weight=T(F32, 5))
pls = dict(logits=T(F32, 2, 4), dummy=T(F32, 2, 2), target=T(I64, 2), n_mixed=1, l0=0.01, l1=1.0, l2=1.0, need_grad=True)
needs("proser_loss_fwd_bwd", pls)
case("proser_loss_fwd_bwd", "dummy rows", pls, "osi::proser_loss_fwd_bwd.*dummy", dummy=T(F32, 3, 2))
case("proser_loss_fwd_bwd", "target rows", pls, "osi::proser_loss_fwd_bwd.*target", target=T(I64, 3))
case("proser_loss_fwd_bwd", "logits 1-D", pls, "osi::proser_loss_fwd_bwd.*logits", logits=T(F32, 2))
case("proser_loss_fwd_bwd", "n_mixed negative", pls, "osi::proser_loss_fwd_bwd.*n_mixed", n_mixed=-1)
case("proser_loss_fwd_bwd", "n_mixed beyond B", pls, "osi::proser_loss_fwd_bwd.*n_mixed", n_mixed=3)
psc = dict(logits=T(F32, 2, 4), dummy=T(F32, 2, 2), bias=0.0)
needs("proser_scores", psc)
case("proser_scores", "dummy rows", psc, "osi::proser_scores.*dummy", dummy=T(F32, 3, 2))
case("proser_scores", "dummy 1-D", psc, "osi::proser_scores.*dummy", dummy=T(F32, 2))
case("proser_scores", "logits 1-D", psc, "osi::proser_scores.*logits", logits=T(F32, 2))
lfw = dict(x=T(F32, 2, 6), w=T(F32, 3, 6), bias=T(F32, 3))
needs("linear_fwd", lfw)
case("linear_fwd", "w columns", lfw, "osi::linear_fwd.*w", w=T(F32, 3, 5))
case("linear_fwd", "x 1-D", lfw, "osi::linear_fwd.*x", x=T(F32, 6))
case("linear_fwd", "bias numel", lfw, "osi::linear_fwd.*bias", bias=T(F32, 4))
lf4 = dict(x=T(F32, 2, 8, align=16), w=T(F32, 3, 8, align=16), bias=None)   # K % 4 == 0: the 16-byte loads need aligned rows
case("linear_fwd", "x offset at K of 8", lf4, "osi::linear_fwd.*aligned", x=lf4["x"].mutated("offset"))
case("linear_fwd", "w offset at K of 8", lf4, "osi::linear_fwd.*aligned", w=lf4["w"].mutated("offset"))
lbw = dict(dy=T(F32, 2, 3), x=T(F32, 2, 6), w=T(F32, 3, 6), need_dx=True)
needs("linear_bwd", lbw)
case("linear_bwd", "x rows", lbw, "osi::linear_bwd.*dy", x=T(F32, 3, 6))
case("linear_bwd", "dy columns", lbw, "osi::linear_bwd.*dy", dy=T(F32, 2, 4))
case("linear_bwd", "w columns", lbw, "osi::linear_bwd.*dy", w=T(F32, 3, 5))
case("linear_bwd", "dy 1-D", lbw, "osi::linear_bwd.*dy", dy=T(F32, 6))


# ---------------------------------------------------------------------------------------------------------------------------- the test
@functools.lru_cache(maxsize=None)
def _executor():
    """One executor at the geometry of the whole-network cases, created the way test_proser_gpu._net creates its model; used for
    refusals only: no forward ever runs on it."""
    from test_frozen_bn_gpu import _case, _model
    cuda = torch.device("cuda:0")
    sd, x, _, _ = _case("signed")
    model = _model(sd, cuda)
    B, _, H, W = x.shape
    net = model._net(B, H, W)
    return dict(model=model, net=net, h=net.h.value, params=model._flat_params, buffers=model._flat_buffers, nbt=model._nbt,
                grads=model._flat_grads, ws=model._ws, image=x.to(cuda), B=B, H=H, W=W, F=model._F, O=model._O)


class Env:
    def __init__(self, dev):
        self.dev = dev

    def zeros(self, dtype, *shape):
        return torch.zeros(shape, dtype=dtype, device=self.dev)

    def __getattr__(self, name):                     # anything else: a field of the shared executor
        return _executor()[name]


def materialise(v, env):
    if tensors(v):
        return [t.build(env.dev) for t in v] if isinstance(v, list) else v.build(env.dev)
    return v(env) if isinstance(v, types.FunctionType) else v


@pytest.mark.parametrize("op, args, match", CASES)
def test_binding_refuses(cuda, op, args, match):
    env = Env(cuda)
    values = [materialise(v, env) for v in args.values()]
    with pytest.raises(RuntimeError, match=match) as err:
        getattr(NL.ops(), op)(*values)
    assert "libosi_hip" not in str(err.value), "the refusal came from the C ABI, not from the binding"
    torch.cuda.synchronize()
