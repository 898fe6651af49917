"""Dev tool: ODIN (csrc/odin.hip, openset_imagenet/odin.py) - device time per batch of the four legs of ODIN.scores on the MI355X
ResNet50 from HIP events (median of 10 after 3 warm calls, the batch resident on the device as NHWC4): the differentiable forward on
the running statistics, the input-only backward ending in the projected step, the inference forward on the perturbed batch and the
head launch (osi_odin_head with and without dlogits), then ODIN.scores as a whole next to what a plain train.get_arrays batch costs
(one inference forward and the softmax), and osi_gradnorm_scores on the batch's (features, logits). B = 64, 224 x 224, C = F = 116
by default. Prints one JSON document.
usage: python tools/time_odin.py [--batch 64] [--classes 116]"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.normpath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(ROOT, "openset-imagenet_amd"))
from openset_imagenet import ResNet50, _native as NL, tools
from openset_imagenet.adversary import as_nhwc4
from openset_imagenet.odin import ODIN

p = argparse.ArgumentParser()
p.add_argument("--batch", type=int, default=64)
p.add_argument("--classes", type=int, default=116)
p.add_argument("--size", type=int, default=224)
args = p.parse_args()
B, C, HW = args.batch, args.classes, args.size
tools.set_device_gpu(0)
dev = torch.device("cuda:0")
torch.manual_seed(0)
model = tools.device(ResNet50(C, C, False)).eval()
x = as_nhwc4(torch.rand(B, 3, HW, HW).to(dev))
odin = ODIN()
ops = NL.ops()


def timed(fn, warm=3, reps=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1])


def timed_legs(warm=3, reps=10):
    """The forward, the head launch and the backward of one perturb, each between its own pair of events on the stream."""
    legs = ([], [], [])
    for i in range(warm + reps):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        model.next_backward(pgd=(-odin.epsilon, math.inf, None), input_only=True)
        with torch.enable_grad():
            e[0].record()
            logits, _ = model(x)
            e[1].record()
            seed = ops.odin_head(logits.detach(), odin.temperature, True)[0]
            e[2].record()
            logits.backward(seed)
            e[3].record()
        torch.cuda.synchronize()
        if i >= warm:
            for k in range(3):
                legs[k].append(e[k].elapsed_time(e[k + 1]))
    return [dict(median_ms=sorted(ms)[len(ms) // 2], min_ms=min(ms), max_ms=max(ms)) for ms in legs]


def inference(batch):
    with torch.no_grad():
        return model(batch)


logits, features = inference(x)
x_t = odin.perturb(model, x)[2]
fwd, head_in_line, bwd = timed_legs()
report = {
    "device": torch.cuda.get_device_name(0), "batch": B, "size": HW, "classes": C, "temperature": odin.temperature, "epsilon": odin.epsilon,
    "differentiable_forward": fwd,
    "head_in_line": head_in_line,
    "input_only_backward": bwd,
    "inference_forward": timed(lambda: inference(x_t)),
    "head_with_dlogits": timed(lambda: ops.odin_head(logits, odin.temperature, True)),
    "head_score_only": timed(lambda: ops.odin_head(logits, odin.temperature, False)),
    "odin_scores_total": timed(lambda: odin.scores(model, x)),
    "get_arrays_batch": timed(lambda: ops.softmax(inference(x)[0])),
    "gradnorm_scores": timed(lambda: ops.gradnorm_scores(features, logits, 1.0)),
}
report["odin_over_get_arrays"] = report["odin_scores_total"]["median_ms"] / report["get_arrays_batch"]["median_ms"]
print(json.dumps(report, indent=1))
