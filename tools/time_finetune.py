"""Dev tool: what fine-tuning a suffix costs at the benchmark geometry (B = 128, 224 x 224, C = 30, entropic loss), as interleaved
rounds of forward + loss + backward + Adam step so box drift hits all modes alike:
  full                 every parameter trainable, training mode: the default step;
  flags<cut            requires_grad = False on everything below <cut> (layer3, layer4, fc), training mode, nothing declared: the
                       full forward, the backward stops at the cut (ABI 13; on an older library this is the full step);
  below<cut            model.freeze_below(<cut>), training mode: the prefix in the inference forms, batch-statistics suffix;
  below<cut>+bn        the same under freeze_bn(): the suffix on the running statistics as well.
On a build without ABI 13 (no osi_resnet50_set_trainable, no ResNet50.freeze_below: copy this file into a checkout of the commit
before it) the freeze_below modes are skipped: the flags-only modes then time what that build pays for the same flags.
Device events around each window. The table goes to profiles/finetune_b128.txt (or the path given).
usage: python tools/time_finetune.py [rounds] [steps per window] [output path]"""
import os
import statistics
import sys

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path[:0] = [ROOT, os.path.join(ROOT, "openset-imagenet_amd")]
import torch

from openset_imagenet import ResNet50, EntropicOpensetLoss, optim
from openset_imagenet import _native as N

B, H, W, C = 128, 224, 224, 30
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 6
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
OUT = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "finetune_b128.txt")
CUTS = ("layer3", "layer4", "fc")


def main():
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on an MI355X only")
    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = ResNet50(C, C, False).to(dev)
    has_cut = hasattr(model, "freeze_below") and N.lib().osi_abi_version() >= 13
    with torch.no_grad():                       # running statistics of a model that has seen data, not the 0 / 1 initialisation
        for name, buf in model.named_buffers():
            if name.endswith("running_var"):
                buf.uniform_(0.5, 1.5)
            elif name.endswith("running_mean"):
                buf.normal_(0.0, 0.1)
    start = model._flat_params.clone()
    loss_fn = EntropicOpensetLoss(C, 1.0)
    opt = optim.Adam(model.parameters(), lr=1e-5)
    x = torch.rand(B, 3, H, W, device=dev)
    y = torch.randint(-1, C, (B,), device=dev)

    def prefix(cut):
        stop = "resnet_base." + cut
        names = [n for n, _ in model.named_parameters()]
        return set(names[:next(i for i, n in enumerate(names) if n.startswith(stop))])

    modes = {"full": (None, None, False)}       # name -> (flags cut, declared cut, freeze_bn)
    for cut in CUTS:
        modes["flags<" + cut] = (cut, None, False)
    if has_cut:
        for cut in CUTS:
            modes["below<" + cut] = (None, cut, False)
        for cut in CUTS:
            modes["below<" + cut + "+bn"] = (None, cut, True)

    def setup(flags_cut, declared, frozen_bn):
        if has_cut:
            model.freeze_below(None)
        frozen = prefix(flags_cut) if flags_cut else set()
        for n, p in model.named_parameters():
            p.requires_grad_(n not in frozen)
            p.grad = None
        model.train().freeze_bn(frozen_bn)
        if declared:
            model.freeze_below(declared)

    def step():
        opt.zero_grad()
        loss_fn(model(x)[0], y).backward()
        opt.step()

    def window(mode):
        setup(*modes[mode])
        for _ in range(2):
            step()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(STEPS):
            step()
        e1.record()
        torch.cuda.synchronize()
        with torch.no_grad():                   # every window starts from the same weights
            model._flat_params.copy_(start)
        return e0.elapsed_time(e1) / STEPS

    for m in modes:                             # settle the clock
        window(m)
    res = {m: [] for m in modes}
    names = tuple(modes)
    for r in range(ROUNDS):
        for m in (names if r % 2 == 0 else names[::-1]):
            res[m].append(window(m))

    full = statistics.median(res["full"])
    lines = [f"fine-tuning a suffix, B = {B}, {H} x {W}, C = {C}, entropic loss; forward + loss + backward + Adam step, ms per step",
             f"library ABI {N.lib().osi_abi_version()}" + ("" if has_cut else " (no osi_resnet50_set_trainable: freeze_below modes skipped)"),
             f"{ROUNDS} interleaved rounds of {STEPS} steps (order reversed every other round), device events", "",
             f"{'mode':<18} {'median':>8} {'min':>8} {'max':>8} {'/ full':>7}   rounds"]
    for m, v in res.items():
        med = statistics.median(v)
        lines.append(f"{m:<18} {med:8.3f} {min(v):8.3f} {max(v):8.3f} {med / full:7.3f}   " + " ".join(f"{t:.3f}" for t in v))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
