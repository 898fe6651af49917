"""Evaluation entry point with the surface of the reference's script/evaluate.py (evaluate.py:15-149): same positional arguments
and options, same checkpoint naming (`{loss}_best.pth` / `{loss}_curr.pth` in the output directory), same output files
`{loss}_{val,test}_arr{suffix}.npz` with `gt`, `logits`, `features`, `scores`. The forward passes run on the MI355X executor in
eval mode (train.get_arrays); there is no CPU evaluation path. `--oscr` (this build's addition) also prints the area-free summary
of the OSCR curve computed on the GPU (util.calculate_oscr); `--auc` (likewise) prints the binary ROC-AUC of known against negative
(-1) and against unknown (-2) samples, counted on the GPU (metrics.auc_score_binary); `--report` (likewise) writes `{loss}_{split}_report{suffix}.json` with
the confidences, the CCR at FPR 1e-3 / 1e-2 / 0.1 / 1 and the 30-bin score and feature-norm histograms (evaluation_report), and
prints the row of the reference's table (script/plot_all.py:344-385). `--openmax TAILSIZE` (likewise; softmax and entropic losses)
fits OpenMax (openmax.OpenMax) on the arrays of the training split, saves it as `{loss}_openmax{suffix}.pth` and writes, next to each
split's .npz, `{loss}_{split}_arr{suffix}_openmax.npz` with `gt`, `logits`, `features`, `scores` (the recalibrated class
probabilities) and `unknown` (the probability of the unknown class); with `--oscr` the same OSCR line is printed for those scores.
`--evm TAILSIZE` (likewise; softmax and entropic losses) fits the Extreme Value Machine (evm.EVM; `--evm-cover`, `--evm-multiplier`,
`--evm-distance`) on the features of the training split, saves it as `{loss}_evm{suffix}.pth` and writes
`{loss}_{split}_arr{suffix}_evm.npz` with `gt`, `logits`, `features` and `scores` (the per-class inclusion probabilities).
`--knn K` (likewise; softmax and entropic losses) keeps the features of the training split as the bank of deep nearest neighbours
(knn.KNN; `--knn-distance`, `--knn-fraction`), saves it as `{loss}_knn{suffix}.pth` and writes `{loss}_{split}_arr{suffix}_knn.npz`
with `gt`, `logits`, `features`, `scores` (per class the similarity of the K-th nearest bank row of that class) and `unknown` (the
distance to the K-th nearest bank row overall).
`--mahalanobis` (likewise; softmax and entropic losses) fits the Mahalanobis detector (mahalanobis.Mahalanobis: class means and one tied
covariance in fp64; `--mahalanobis-shrinkage`, `--mahalanobis-relative`) on the features of the training split, saves it as
`{loss}_mahalanobis{suffix}.pth` and writes `{loss}_{split}_arr{suffix}_mahalanobis.npz` with `gt`, `logits`, `features`, `scores`
(per class the similarity of the squared distance) and `unknown` (the smallest squared distance of the row).
`--vim` (likewise; softmax and entropic losses) fits ViM (vim.ViM: the principal subspace of the training split's features from the
device eigensolver, `--vim-dim`; the evaluation network has no logit bias, so the origin is zero), saves it as `{loss}_vim{suffix}.pth`
and writes `{loss}_{split}_arr{suffix}_vim.npz` with `gt`, `logits`, `features`, `scores` (the known classes' softmax with the virtual
logit) and `unknown` (alpha * residual norm - logsumexp of the logits).
`--shaping METHOD` (likewise; softmax and entropic losses; react, ash_p, ash_b, ash_s or scale, `--shaping-percentile`) shapes the
network's pooled activation (shaping.ActivationShaping; get_arrays(pooled=True) gathers it, react takes its clip from the training
split), saves the detector as `{loss}_shaping{suffix}.pth` and writes `{loss}_{split}_arr{suffix}_shaping.npz` with `gt`, `logits`,
`features` (the network's own), `scores` (the softmax of the logits re-computed from the shaped activation) and `unknown` (minus their
logsumexp).
`--proser` (likewise; softmax and entropic losses) loads the fine-tuned network, dummy classifier and calibrated bias that
`python -m openset_imagenet.script.proser` saved as `{loss}_proser{suffix}.pth` (proser.PROSER) and writes
`{loss}_{split}_arr{suffix}_proser.npz` with `gt`, `logits`, `features` of THAT network, `scores` = probs[:, :C] and `unknown` =
probs[:, C]; with `--oscr` the same OSCR line is printed for those scores.
`--odin` (likewise; softmax and entropic losses) scores with ODIN (odin.ODIN: the temperature-scaled largest softmax probability after
one signed-gradient step on the image; `--odin-temperature`, `--odin-epsilon`, in this network's [0, 1] pixel units). It needs a pass of
its own over the images: one differentiable forward, one input-only backward and one inference forward per batch. `--odin-tune` first
selects both settings on the `val` split against label -1 over the paper's grid (ODIN_TEMPERATURES x ODIN_EPSILONS). The detector is saved
as `{loss}_odin{suffix}.pth`, and `{loss}_{split}_arr{suffix}_odin.npz` holds `gt`, `logits`, `features`, `scores` (the clean forward's),
`logits_odin` (the logits of the perturbed batch) and `unknown` (minus the score).
`--gradnorm` (likewise; `--gradnorm-temperature`; needs `--detection`) adds the scorer GradNorm (odin.gradnorm_scores, negated) beside the
logit baselines; it has no fit and writes no file of its own.
`--detection` (likewise) scores every REJECTION score of the run, one value per sample where higher means more unknown: the baselines
read off the logits (MSP, MaxLogit, Energy: the negated osi_logit_scores values; for the garbage loss without the background column),
the `unknown` vector of every detector fitted in the same run and of `--proser`, and for a detector without one (the EVM) minus its
largest class score, tagged "(-max score)". For every split, each negative label present (-1, -2) and each scorer it prints one line
with AUROC, AUPR-in, AUPR-out, FPR at 95 % TPR (metrics.detection_metrics: known rows against the rows of that label) and the trapezoid
area of the OSCR curve by rejection (util.oscr_by_rejection / util.oscr_area: the scorer's `scores` decide the closed-set prediction,
its rejection score rejects), all counted on the GPU (csrc/detection.hip), and collects the same numbers in
`{loss}_{split}_detection{suffix}.json` (`rows`: scorer, unk_label, auroc, aupr_in, aupr_out, fpr_at_tpr95, known, unknown, oscr_area,
oscr_points; `error` instead of figures where a score holds a NaN)."""
import argparse
import json
import pathlib

import numpy as np
import torch

from .. import metrics, tools, util
from ..evm import EVM
from ..knn import KNN
from ..mahalanobis import Mahalanobis
from ..model import ResNet50
from ..odin import ODIN, gradnorm_scores
from ..openmax import OpenMax
from ..shaping import METHODS as SHAPING_METHODS, ActivationShaping, head_of
from ..train import _image_loader, get_arrays, load_checkpoint
from ..vim import ViM


def _known_and_unknown(probs):
    """[M, C + 1] device probabilities with the unknown class last -> numpy `scores` [M, C] and `unknown` [M]."""
    probs = probs.cpu().numpy()
    c = probs.shape[1] - 1
    return dict(scores=probs[:, :c], unknown=probs[:, c])


# One record per post-hoc detector, in the order main() fits, scores and prints them:
#   name      in the option (--name), the file names and the keys of main()'s `written`
#   tag       of the OSCR line
#   cls       the detector
#   on        args -> whether the option asks for it
#   options   args -> the keyword arguments of cls
#   fit       (detector, the `features`, `logits`, `gt` of the training split as a mapping; with the shaping row on, `pooled` and
#             `head` too, here and in the arrays of a split)
#   score     (detector, arrays of a split) -> numpy `scores` [M, C] and, where the method has one, `unknown` [M]
#   summary   (detector, args) -> the line printed after the fit, up to "; saved in: ..."
DETECTORS = (
    dict(name="openmax", tag="OpenMax ", cls=OpenMax, on=lambda args: args.openmax is not None,
         options=lambda args: dict(tailsize=args.openmax, distance=args.openmax_distance, alpha=args.openmax_alpha),
         fit=lambda om, t: om.fit(t["features"], t["logits"], t["gt"]),
         score=lambda om, a: _known_and_unknown(om.predict(a["logits"], a["features"])),
         summary=lambda om, args: f"OpenMax (tail {args.openmax}, alpha {args.openmax_alpha}, {args.openmax_distance}) fitted on "
         f"{int(om.count.sum())} correct training samples, " + "{1} classes unfitted, {0} distances not finite".format(*om.flags.tolist())),
    dict(name="evm", tag="EVM ", cls=EVM, on=lambda args: args.evm is not None,
         options=lambda args: dict(tailsize=args.evm, cover_threshold=args.evm_cover, distance_multiplier=args.evm_multiplier,
                                   distance=args.evm_distance),
         fit=lambda evm, t: evm.fit(t["features"], t["gt"]),
         score=lambda evm, a: dict(scores=evm.predict(a["features"]).cpu().numpy()),
         summary=lambda evm, args: f"EVM (tail {args.evm}, cover {args.evm_cover}, multiplier {args.evm_multiplier}, {args.evm_distance}) keeps "
         f"{evm.ev_features.shape[0]} extreme vectors, " + "{1} rows unfitted, {0} distances not finite".format(*evm.flags.tolist())),
    dict(name="knn", tag="KNN ", cls=KNN, on=lambda args: args.knn is not None,
         options=lambda args: dict(k=args.knn, distance=args.knn_distance, bank_fraction=args.knn_fraction),
         fit=lambda knn, t: knn.fit(t["features"], t["gt"]),
         score=lambda knn, a: dict(scores=knn.predict(a["features"]).cpu().numpy(), unknown=knn.unknown_score(a["features"]).cpu().numpy()),
         summary=lambda knn, args: f"KNN (k {args.knn}, {args.knn_distance}, fraction {args.knn_fraction}) keeps a bank of "
         f"{knn.bank_features.shape[0]} rows"),
    dict(name="mahalanobis", tag="Mahalanobis ", cls=Mahalanobis, on=lambda args: args.mahalanobis,
         options=lambda args: dict(shrinkage=args.mahalanobis_shrinkage, relative=args.mahalanobis_relative),
         fit=lambda maha, t: maha.fit(t["features"], t["gt"]),
         score=lambda maha, a: dict(scores=maha.predict(a["features"]).cpu().numpy(), unknown=maha.unknown_score(a["features"]).cpu().numpy()),
         summary=lambda maha, args: f"Mahalanobis (shrinkage {args.mahalanobis_shrinkage}, relative {args.mahalanobis_relative}) fitted on "
         f"{int(maha.counts[-1])} training samples, log-determinant {float(maha.logdet):.6f}"),
    dict(name="vim", tag="ViM ", cls=ViM, on=lambda args: args.vim,
         options=lambda args: dict(dim=args.vim_dim),
         fit=lambda vim, t: vim.fit(t["features"], t["logits"], t["gt"]),       # no weight or bias: the origin is zero
         score=lambda vim, a: dict(scores=vim.predict(a["features"], a["logits"]).cpu().numpy(),
                                   unknown=vim.unknown_score(a["features"], a["logits"]).cpu().numpy()),
         summary=lambda vim, args: f"ViM (dim {vim.dim} of {vim.components.shape[0]}) fitted on {vim.count} training samples in "
         f"{vim.sweeps} Jacobi sweeps, alpha {vim.alpha:.6f}"),
    dict(name="shaping", tag="Shaping ", cls=ActivationShaping, on=lambda args: args.shaping is not None,
         options=lambda args: dict(method=args.shaping, percentile=args.shaping_percentile),
         fit=lambda sh, t: sh.fit(t["pooled"], t["gt"], head=t["head"]),
         score=lambda sh, a: dict(scores=sh.predict(a["pooled"]).cpu().numpy(), unknown=sh.unknown_score(a["pooled"]).cpu().numpy()),
         summary=lambda sh, args: f"Activation shaping ({sh.method}, percentile {sh.percentile}) " +
         (f"clips at {sh.clip:.6f}, fitted on {sh.count} training samples" if sh.method == "react" else
          f"keeps {sh.keep(sh.fc_weight.shape[1])} of {sh.fc_weight.shape[1]} columns")),
)


ODIN_TEMPERATURES = (1, 2, 5, 10, 20, 50, 100, 200, 500, 1000)      # the grid of the ODIN paper
ODIN_EPSILONS = tuple(float(e) for e in np.linspace(0.0, 0.004, 21))


def get_args(command_line_options=None):
    p = argparse.ArgumentParser("Get parameters for evaluation", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("loss", choices=["entropic", "softmax", "garbage"], help="Which loss function to evaluate")
    p.add_argument("protocol", type=int, choices=(1, 2, 3), help="Which protocol to evaluate")
    p.add_argument("--use-best", "-b", action="store_true", help="Take the best model of the validation set, otherwise the last")
    p.add_argument("--gpu", "-g", type=int, nargs="?", default=None, const=0, help="GPU index (bare -g = 0); required")
    p.add_argument("--imagenet-directory", type=pathlib.Path, default=pathlib.Path("/local/scratch/datasets/ImageNet/ILSVRC2012/"))
    p.add_argument("--protocol-directory", type=pathlib.Path, default="protocols", help="Where are the protocol files stored")
    p.add_argument("--output-directory", default="experiments/Protocol_{}", help="Where to find the results of the experiments")
    p.add_argument("--batch-size", type=int, default=64)
    p.add_argument("--workers", type=int, default=4)
    p.add_argument("--oscr", action="store_true", help="also compute the OSCR curve of each split on the GPU")
    p.add_argument("--auc", action="store_true", help="also compute the binary ROC-AUC of each split (known vs -1, known vs -2) on the GPU")
    p.add_argument("--report", action="store_true", help="also write {loss}_{split}_report{suffix}.json (confidences, CCR at FPR, score and "
                   "norm histograms, all counted on the GPU) next to the .npz and print the row of the reference's table")
    p.add_argument("--detection", action="store_true", help="also score every rejection score of the run (MSP, max-logit and energy of the "
                   "logits, the `unknown` vector of every fitted detector and of PROSER) with AUROC, AUPR-in, AUPR-out, FPR at 95%% TPR "
                   "and the area of the OSCR curve by that score, counted on the GPU; writes {loss}_{split}_detection{suffix}.json")
    p.add_argument("--averaged", action="store_true", help="evaluate the averaged weights (EMA / SWA) the checkpoint carries under "
                   "avg_state_dict (config block avg) instead of the trained ones; the output files get the suffix _avg")
    p.add_argument("--openmax", type=int, default=None, metavar="TAILSIZE", help="also fit OpenMax with this tail size on the training "
                   "split (softmax and entropic losses) and write {loss}_{split}_arr{suffix}_openmax.npz with the recalibrated scores")
    p.add_argument("--openmax-alpha", type=int, default=3, help="OpenMax: how many top-ranked logits are recalibrated")
    p.add_argument("--openmax-distance", choices=["euclidean", "cosine"], default="euclidean", help="OpenMax: distance to the class means")
    p.add_argument("--evm", type=int, default=None, metavar="TAILSIZE", help="also fit the Extreme Value Machine with this tail size on the "
                   "training split (softmax and entropic losses) and write {loss}_{split}_arr{suffix}_evm.npz with its class scores")
    p.add_argument("--evm-cover", type=float, default=None, metavar="THRESHOLD", help="EVM: reduce every class to the extreme vectors of a "
                   "greedy set cover at this inclusion probability (default: keep every fitted row)")
    p.add_argument("--evm-multiplier", type=float, default=0.5, help="EVM: the factor on the distances before the Weibull fit")
    p.add_argument("--evm-distance", choices=["euclidean", "cosine"], default="cosine", help="EVM: distance between feature rows")
    p.add_argument("--knn", type=int, default=None, metavar="K", help="also score with deep nearest neighbours: the K-th nearest row of the "
                   "training split's features (softmax and entropic losses); writes {loss}_{split}_arr{suffix}_knn.npz")
    p.add_argument("--knn-distance", choices=["euclidean", "cosine"], default="cosine", help="KNN: distance between feature rows")
    p.add_argument("--knn-fraction", type=float, default=1.0, metavar="F", help="KNN: the share of every class's training rows kept as the bank")
    p.add_argument("--mahalanobis", action="store_true", help="also score with the Mahalanobis detector fitted on the training split's "
                   "features (softmax and entropic losses); writes {loss}_{split}_arr{suffix}_mahalanobis.npz")
    p.add_argument("--mahalanobis-shrinkage", type=float, default=0.0, metavar="A", help="Mahalanobis: shrink the covariance towards a scaled "
                   "identity by this share in [0, 1] (needed when it is not positive definite)")
    p.add_argument("--mahalanobis-relative", action="store_true", help="Mahalanobis: subtract the distance under one background Gaussian "
                   "(Relative Mahalanobis)")
    p.add_argument("--vim", action="store_true", help="also score with ViM (virtual-logit matching) fitted on the training split's features "
                   "and logits (softmax and entropic losses); writes {loss}_{split}_arr{suffix}_vim.npz. The evaluation network has "
                   "logit_bias=False, so ViM's origin is zero")
    p.add_argument("--vim-dim", type=int, default=None, metavar="D", help="ViM: the dimension of the principal subspace (default: the "
                   "paper's rule, 1000 for 2048 or more feature columns, 512 for 768 or more, else half of them)")
    p.add_argument("--shaping", choices=sorted(SHAPING_METHODS), default=None, metavar="METHOD", help="also score with activation shaping "
                   "on the pooled layer (react, ash_p, ash_b, ash_s or scale; softmax and entropic losses): the energy of the logits "
                   "re-computed from the shaped activation; writes {loss}_{split}_arr{suffix}_shaping.npz")
    p.add_argument("--shaping-percentile", type=float, default=None, metavar="P", help="shaping: the percentile, 0 < P < 100 (default: "
                   "the method's own)")
    p.add_argument("--proser", action="store_true", help="also evaluate the PROSER stage saved as {loss}_proser{suffix}.pth (softmax and "
                   "entropic losses) and write {loss}_{split}_arr{suffix}_proser.npz with its scores and the probability of the unknown class")
    p.add_argument("--odin", action="store_true", help="also score with ODIN (softmax and entropic losses): a pass of its own over the "
                   "images, one input-only backward per batch; writes {loss}_{split}_arr{suffix}_odin.npz")
    p.add_argument("--odin-temperature", type=float, default=1000.0, metavar="T", help="ODIN: the temperature of the softmax")
    p.add_argument("--odin-epsilon", type=float, default=0.0014, metavar="E", help="ODIN: the size of the signed-gradient step, in the "
                   "network's [0, 1] pixel units")
    p.add_argument("--odin-tune", action="store_true", help="ODIN: select temperature and epsilon on the val split against label -1 over "
                   "the paper's grid (lowest FPR at 95%% TPR)")
    p.add_argument("--gradnorm", action="store_true", help="--detection also scores GradNorm for the last linear layer (softmax and "
                   "entropic losses)")
    p.add_argument("--gradnorm-temperature", type=float, default=1.0, metavar="T", help="GradNorm: the temperature of the softmax")
    args = p.parse_args(command_line_options)
    post_hoc = ["proser"] * args.proser + [row["name"] for row in DETECTORS if row["on"](args)] + ["odin"] * args.odin + ["gradnorm"] * args.gradnorm
    if post_hoc and args.loss == "garbage":
        p.error(f"--{post_hoc[0]} needs a network without a background class: use it with the softmax or entropic loss, not with garbage")
    if args.odin_tune and not args.odin:
        p.error("--odin-tune goes with --odin")
    if not (np.isfinite(args.odin_temperature) and args.odin_temperature > 0.0) or not (np.isfinite(args.odin_epsilon) and args.odin_epsilon >= 0.0):
        p.error(f"--odin-temperature must be finite and > 0 and --odin-epsilon finite and >= 0, got {args.odin_temperature}, {args.odin_epsilon}")
    if not (np.isfinite(args.gradnorm_temperature) and args.gradnorm_temperature > 0.0):
        p.error(f"--gradnorm-temperature must be finite and > 0, got {args.gradnorm_temperature}")
    if args.gradnorm and not args.detection:
        p.error("--gradnorm adds a scorer to --detection and writes nothing of its own: pass --detection as well")
    if args.shaping_percentile is not None and not 0.0 < args.shaping_percentile < 100.0:
        p.error(f"--shaping-percentile must satisfy 0 < P < 100, got {args.shaping_percentile}")
    if args.vim_dim is not None and args.vim_dim < 1:
        p.error(f"--vim-dim must be positive, got {args.vim_dim}")
    if not 0.0 <= args.mahalanobis_shrinkage <= 1.0:
        p.error(f"--mahalanobis-shrinkage must lie in [0, 1], got {args.mahalanobis_shrinkage}")
    try:
        args.output_directory = str(args.output_directory).format(args.protocol)
    except Exception:
        pass
    args.output_directory = pathlib.Path(args.output_directory)
    return args


def auc_rows(gt, scores, unk, loss):
    """What `--auc` hands to metrics.auc_score_binary for the label `unk` (-1 or -2): the known rows (gt >= 0) and the rows labelled
    `unk` only - auc_score_binary counts every label other than unk_class as known, so the rows of the OTHER negative label have to
    go - and, for the garbage loss, the scores without the background column (as `--oscr`). None when no row carries `unk`."""
    gt = np.asarray(gt)
    if not (gt == unk).any():
        return None
    keep = (gt >= 0) | (gt == unk)
    s = scores[:, :-1] if loss == "garbage" else scores
    return gt[keep], s[keep]


FPR_QUERIES = (1e-3, 1e-2, 0.1, 1.0)      # the "CCR at FPR" columns of the reference's table (plot_all.py:352)
REPORT_BINS = 30                          # plot_all.plot_softmax


def evaluation_report(gt, scores, features, loss):
    """The numbers behind the reference's table row and histogram page (script/plot_all.py:277-385) for one split, as a dict of
    plain Python values (JSON-ready), all counted on the GPU:

      conf_kn, conf_unk     metrics.confidence under plot_all.py:366-372: offset 0 for the garbage loss and 1 / (max(gt) + 1) otherwise,
                            unknown_class -2, last_valid_class -1 for garbage (conf_kn_count / conf_unk_count: the samples behind them)
      ccr_at_fpr            {"-1": [...], "-2": [...]}: util.ccr_at_fpr at FPR_QUERIES for each of the two labels present in gt
      score_hist, norm_hist {"-1": {...}, "-2": {...}}: util.get_histogram with 30 bins (kn_hist, kn_edges, unk_hist, unk_edges)

    For the garbage loss the background column is dropped for the curve and the score histograms, as plot_oscr and `--oscr` do (the
    reference's table keeps it in the curve: DESIGN.md, divergences). Inputs: numpy arrays or torch tensors, host or device."""
    dev = util._need_gpu("evaluation_report")
    y = gt.detach().cpu().numpy() if isinstance(gt, torch.Tensor) else np.asarray(gt)
    y = y.astype(np.int64)
    if len(y) == 0:
        raise ValueError("evaluation_report needs at least one sample")
    s = torch.as_tensor(scores).detach().to(dev)
    f = torch.as_tensor(features).detach().to(dev)
    y_dev = torch.from_numpy(y).to(dev)
    garbage = loss == "garbage"
    offset = 0 if garbage else 1 / (int(y.max()) + 1)
    conf = metrics.confidence(s.float(), y_dev, offset=offset, unknown_class=-2, last_valid_class=-1 if garbage else None)
    report = {"loss": loss, "samples": int(len(y)), "conf_kn": conf[0], "conf_kn_count": conf[1], "conf_unk": conf[2],
              "conf_unk_count": conf[3], "fpr_values": list(FPR_QUERIES), "ccr_at_fpr": {}, "score_hist": {}, "norm_hist": {}}
    curve_scores = s[:, :-1] if garbage else s
    arrays = {"scores": s, "gt": y_dev, "features": f}
    names = ("kn_hist", "kn_edges", "unk_hist", "unk_edges")
    for unk in (-1, -2):
        if not (y == unk).any():
            continue
        report["ccr_at_fpr"][str(unk)] = util.ccr_at_fpr(y_dev, curve_scores, fpr_values=FPR_QUERIES, unk_label=unk)
        for key, metric in (("score_hist", "score"), ("norm_hist", "norm")):
            hist = util.get_histogram(arrays, unk_label=unk, metric=metric, bins=REPORT_BINS, drop_bg=garbage)
            report[key][str(unk)] = {n: v.tolist() for n, v in zip(names, hist)}
    return report


def table_row(report, protocol, label, epoch, unk=-2):
    """One row of the reference's table (plot_all.py:376-385): `$P_n$ - label & epoch & conf_kn & conf_unk & ccr...`, `---` where no
    curve point is near the FPR (or the split has no sample labelled `unk`)."""
    ccr = report["ccr_at_fpr"].get(str(unk), [None] * len(report["fpr_values"]))
    row = f"$P_{protocol}$ - {label} & {epoch} & {report['conf_kn']:1.3f} & {report['conf_unk']:1.3f}"
    return row + "".join(" & ---" if v is None else f" & {v:1.3f}" for v in ccr) + "\\\\"


def oscr_lines(split, gt, scores, tag=""):
    """The one-line OSCR summary of `--oscr` for each negative label present in gt."""
    lines = []
    for unk in (-1, -2):
        if (gt == unk).any():
            ccr, fpr = util.calculate_oscr(gt, scores, unk_label=unk)
            at = ccr[np.searchsorted(-fpr, -0.1)] if len(ccr) and np.isfinite(fpr).all() and (fpr <= 0.1).any() else float("nan")
            lines.append(f"{split}: {tag}OSCR vs label {unk}: {len(ccr)} points, CCR@FPR<=0.1 = {at:.4f}")
    return lines


DETECTION_TPR = (0.95,)                   # the FPR@TPR95 column of the out-of-distribution literature
LOGIT_BASELINES = (("MSP", "SCORE_MSP"), ("MaxLogit", "SCORE_MAXLOGIT"), ("Energy", "SCORE_ENERGY"))


def logit_baselines(logits):
    """The three rejection scores read off the logits alone, each the NEGATED osi_logit_scores value so that higher means more
    unknown: {"MSP": -max softmax probability, "MaxLogit": -max logit, "Energy": -logsumexp}, numpy fp32 [N]."""
    from .. import _native as N
    dev = util._need_gpu("logit_baselines")
    z = torch.as_tensor(logits).detach().to(dev).float().contiguous()
    return {name: (-N.ops().logit_scores(z, getattr(N, mode))).cpu().numpy() for name, mode in LOGIT_BASELINES}


def detection_scorer(tag, arrays):
    """(tag, scores, unknown) of one detector's arrays for detection_rows: its `unknown` vector, or - for a detector without one (the
    EVM) - minus its largest class score, and then the tag says so."""
    if "unknown" in arrays:
        return tag.strip(), arrays["scores"], arrays["unknown"]
    return f"{tag.strip()} (-max score)", arrays["scores"], -np.asarray(arrays["scores"]).max(1)


def detection_rows(gt, scorers):
    """`--detection` on arrays: for each negative label present in gt (-1, -2) and each scorer (tag, scores [N, C], unknown [N]) one
    dict of plain values: metrics.detection_metrics of `unknown` at DETECTION_TPR, and the area (util.oscr_area) and number of points
    of util.oscr_by_rejection, where `scores` decides the closed-set prediction and `unknown` rejects. A scorer whose `unknown` holds
    a NaN gets a row with `error` set instead of figures."""
    gt = np.asarray(gt)
    rows = []
    for unk in (-1, -2):
        if not (gt == unk).any():
            continue
        for tag, scores, unknown in scorers:
            row = {"scorer": tag, "unk_label": unk}
            try:
                m = metrics.detection_metrics(gt, unknown, unk_label=unk, tpr=DETECTION_TPR)
                ccr, fpr = util.oscr_by_rejection(gt, scores, unknown, unk_label=unk)
                row.update(auroc=m["auroc"], aupr_in=m["aupr_in"], aupr_out=m["aupr_out"], fpr_at_tpr95=m["fpr_at_tpr"][0],
                           known=m["known"], unknown=m["unknown"], oscr_area=util.oscr_area(ccr, fpr), oscr_points=len(ccr))
            except ValueError as refusal:
                row["error"] = str(refusal)
            rows.append(row)
    return rows


def detection_line(split, row):
    """The line `--detection` prints for one row of detection_rows."""
    head = f"{split}: detection {row['scorer']} vs label {row['unk_label']}: "
    if "error" in row:
        return head + f"refused ({row['error']})"
    return head + (f"AUROC {row['auroc']:.4f} AUPR-in {row['aupr_in']:.4f} AUPR-out {row['aupr_out']:.4f} FPR@TPR95 {row['fpr_at_tpr95']:.4f} "
                   f"OSCR-by-rejection area {row['oscr_area']:.4f} ({row['oscr_points']} points)")


def scored_arrays(score, detector, split_arrays):
    """The numpy `gt`, `logits`, `features` of one split (a mapping as get_arrays' .npz holds them) and, after them, what
    `score(detector, split_arrays)` gives: `scores` and perhaps `unknown`. This is what main() writes next to the split's .npz."""
    host = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    scored = score(detector, split_arrays)
    return dict({key: host(split_arrays[key]) for key in ("gt", "logits", "features")}, **scored)


def _detector_arrays(name, train_arrays, split_arrays, **options):
    """Behind the *_arrays helpers below: the detector `name` of DETECTORS, built with `options` and fitted on the training split's
    arrays (a mapping as get_arrays' .npz holds them) unless `train_arrays` is that detector, already fitted and then taken as it is;
    one split scored with it. Returns (detector, arrays of scored_arrays)."""
    row = next(row for row in DETECTORS if row["name"] == name)
    detector = train_arrays
    if not isinstance(detector, row["cls"]):
        detector = row["cls"](**options)
        row["fit"](detector, train_arrays)
    return detector, scored_arrays(row["score"], detector, split_arrays)


def openmax_arrays(train_arrays, split_arrays, tailsize, alpha, distance):
    """`--openmax` on arrays: OpenMax fitted on the training split's `gt`, `logits`, `features`. Returns (om, arrays) with `scores` =
    probs[:, :C] and `unknown` = probs[:, C]."""
    return _detector_arrays("openmax", train_arrays, split_arrays, tailsize=tailsize, distance=distance, alpha=alpha)


def evm_arrays(train_arrays, split_arrays, tailsize, cover_threshold=None, multiplier=0.5, distance="cosine"):
    """`--evm` on arrays: the Extreme Value Machine fitted on the training split's `gt` and `features`. Returns (evm, arrays) with
    `scores` = the [M, C] inclusion probabilities."""
    return _detector_arrays("evm", train_arrays, split_arrays, tailsize=tailsize, cover_threshold=cover_threshold,
                            distance_multiplier=multiplier, distance=distance)


def knn_arrays(train_arrays, split_arrays, k, distance="cosine", fraction=1.0, seed=0):
    """`--knn` on arrays: the training split's `gt` and `features` kept as the bank of deep nearest neighbours. Returns (knn, arrays)
    with `scores` = the [M, C] class similarities and `unknown` = the [M] distances to the k-th nearest bank row."""
    return _detector_arrays("knn", train_arrays, split_arrays, k=k, distance=distance, bank_fraction=fraction, seed=seed)


def mahalanobis_arrays(train_arrays, split_arrays, shrinkage=0.0, relative=False):
    """`--mahalanobis` on arrays: the class means and the tied covariance fitted on the training split's `gt` and `features`. Returns
    (maha, arrays) with `scores` = the [M, C] class similarities and `unknown` = the [M] smallest squared distances."""
    return _detector_arrays("mahalanobis", train_arrays, split_arrays, shrinkage=shrinkage, relative=relative)


def vim_arrays(train_arrays, split_arrays, dim=None):
    """`--vim` on arrays: ViM fitted on the training split's `gt`, `logits` and `features` (the origin is zero, as for a network without
    a logit bias). Returns (vim, arrays) with `scores` = the [M, C] known columns of the softmax with the virtual logit and `unknown` =
    the [M] values alpha * residual norm - logsumexp(logits)."""
    return _detector_arrays("vim", train_arrays, split_arrays, dim=dim)


def shaping_arrays(train_arrays, split_arrays, head, method, percentile=None):
    """`--shaping` on arrays: ActivationShaping over `head` (shaping.head_of(model)), fitted on the training split's `pooled` and `gt`
    (react; the other methods read no data) and run on the split's `pooled`. Returns (shaping, arrays) with `scores` = the [M, C]
    softmax of the logits re-computed from the shaped activation and `unknown` = the [M] values -logsumexp of them."""
    if not isinstance(train_arrays, ActivationShaping):
        train_arrays = dict(train_arrays, head=head)
    return _detector_arrays("shaping", train_arrays, split_arrays, method=method, percentile=percentile)


def proser_arrays(proser, split_arrays):
    """`--proser` on arrays: `gt`, `logits`, `features` of one split as the fine-tuned network of `proser` (proser.PROSER) gave them
    (mappings as get_arrays' .npz holds them). Returns the numpy `gt`, `logits`, `features`, `scores` = probs[:, :C] and `unknown` =
    probs[:, C] of PROSER.predict over the dummy classifier's logits."""
    return scored_arrays(lambda p, a: _known_and_unknown(p.predict(a["logits"], p.dummy_logits(a["features"]))), proser, split_arrays)


def odin_arrays(odin, model, loader):
    """`--odin` on a loader: ODIN.arrays - numpy `gt`, `logits`, `features`, `scores` (the clean forward's), `logits_odin` and `unknown`."""
    return odin.arrays(model, loader)


def gradnorm_scorer(scores, features, logits, temperature=1.0):
    """The `--detection` scorer of `--gradnorm`: ("GradNorm", scores, -gradnorm_scores(features, logits, temperature)) - higher means
    more unknown -, numpy fp32 [N]."""
    return "GradNorm", scores, (-gradnorm_scores(features, logits, temperature)).cpu().numpy()


def load_proser(path, n_classes):
    """The PROSER module of a file written by script/proser.py, on the device, with a network of its own."""
    from ..proser import PROSER
    sd = torch.load(path, map_location="cpu", weights_only=False)
    net = ResNet50(fc_layer_dim=n_classes, out_features=n_classes, logit_bias=False)
    proser = PROSER(net, dummy_count=int(sd["dummy_count"]), mix_at=sd["mix_at"], lambdas=tuple(sd["lambdas"]), alpha=float(sd["alpha"]))
    proser.load_state_dict(sd)
    return tools.device(proser)


def averaged_module(model, checkpoint):
    """`--averaged`: the module of the checkpoint's "avg_state_dict" (averaging.AveragedModel over `model`'s geometry); exits with a
    clear message when the checkpoint was written without an `avg` block."""
    from ..averaging import AveragedModel
    data = torch.load(checkpoint, map_location="cpu", weights_only=False)
    if "avg_state_dict" not in data:
        raise SystemExit(f"--averaged: {checkpoint} holds no averaged weights (no 'avg_state_dict': it was trained without an avg block)")
    averaged = AveragedModel(model)
    averaged.load_state_dict(data["avg_state_dict"])
    print(f"Evaluating the averaged weights ({int(averaged.n_averaged)} updates)")
    return averaged.module


def main(command_line_options=None):
    args = get_args(command_line_options)
    if args.gpu is None:
        raise RuntimeError("No GPU device selected: the MI355X build has no CPU evaluation path (pass -g [index])")
    tools.set_device_gpu(index=args.gpu)
    splits = {}
    for split in ("val", "test"):
        ds = _image_loader(args.protocol_directory / f"p{args.protocol}_{split}.csv", args.imagenet_directory, False, "eval")
        splits[split] = ds
        print(f"{split} dataset len:{len(ds)}, labels:{ds.table.label_count}")
    n_labels = splits["val"].table.label_count
    n_classes = n_labels if args.loss == "garbage" else n_labels - 1     # evaluate.py:121-124
    suffix = "_best" if args.use_best else "_curr"
    model = ResNet50(fc_layer_dim=n_classes, out_features=n_classes, logit_bias=False)
    checkpoint = args.output_directory / (args.loss + suffix + ".pth")
    start_epoch, best_score = load_checkpoint(model, checkpoint)
    print(f"Taking model from epoch {start_epoch} that achieved best score {best_score}")
    if args.averaged:
        model = averaged_module(model, checkpoint)
        suffix += "_avg"
    tools.device(model)
    written = {}
    proser = None
    if args.proser:
        proser_path = args.output_directory / f"{args.loss}_proser{suffix}.pth"
        if not proser_path.is_file():
            raise SystemExit(f"--proser: {proser_path} not found; run python -m openset_imagenet.script.proser {args.loss} {args.protocol} first")
        proser = load_proser(proser_path, n_classes)
        print(f"PROSER stage loaded from: {proser_path} (dummy {proser.dummy_count}, mix at {proser.mix_at}, bias {float(proser.bias):.6f})")
    fitted = [(row, row["cls"](**row["options"](args))) for row in DETECTORS if row["on"](args)]      # refuses bad options first
    odin = ODIN(args.odin_temperature, args.odin_epsilon) if args.odin else None
    shaping = any(row["name"] == "shaping" for row, _ in fitted)     # the one row that reads the pooled activation and the head:
    extra = {}                                                       # with it on, `pooled` and `head` join the mappings below
    if fitted:
        train_ds = _image_loader(args.protocol_directory / f"p{args.protocol}_train.csv", args.imagenet_directory, False, "eval")
        print(f"train dataset len:{len(train_ds)}, labels:{train_ds.table.label_count}")
        loader = torch.utils.data.DataLoader(train_ds, batch_size=args.batch_size, num_workers=args.workers)
        arrays = get_arrays(model=model, loader=loader, pooled=shaping)
        t_gt, t_logits, t_features = arrays[:3]
        if shaping:
            extra = dict(pooled=arrays[4], head=head_of(model))
    for row, detector in fitted:
        row["fit"](detector, dict(gt=t_gt, logits=t_logits, features=t_features, **extra))
        path = args.output_directory / f"{args.loss}_{row['name']}{suffix}.pth"
        torch.save(detector.state_dict(), path)
        print(f"{row['summary'](detector, args)}; saved in: {path}")

    if odin is not None:
        if args.odin_tune:
            loader = torch.utils.data.DataLoader(splits["val"], batch_size=args.batch_size, num_workers=args.workers)
            odin.tune(model, loader, ODIN_TEMPERATURES, ODIN_EPSILONS, unk_label=-1)
        path = args.output_directory / f"{args.loss}_odin{suffix}.pth"
        torch.save(odin.state_dict(), path)
        print(f"ODIN (temperature {odin.temperature:g}, epsilon {odin.epsilon:g}" +
              (f", selected on val among {odin.grid.shape[0]} grid points" if args.odin_tune else "") + f"); saved in: {path}")

    def write(split, name, tag, gt, arrays):
        """One detector's arrays of a split next to the split's .npz, and its OSCR line."""
        file_path = args.output_directory / f"{args.loss}_{split}_arr{suffix}_{name}.npz"
        np.savez(file_path, **arrays)
        print(f"{tag}scores saved in: {file_path}")
        written[f"{split}_{name}"] = file_path
        if args.detection:
            scorers.append(detection_scorer(tag, arrays))
        if args.oscr:
            for line in oscr_lines(split, gt, arrays["scores"], tag=tag):
                print(line)

    for split, ds in splits.items():
        loader = torch.utils.data.DataLoader(ds, batch_size=args.batch_size, num_workers=args.workers)
        arrays = get_arrays(model=model, loader=loader, pooled=shaping)
        gt, logits, features, scores = arrays[:4]
        if shaping:
            extra = dict(extra, pooled=arrays[4])
        file_path = args.output_directory / f"{args.loss}_{split}_arr{suffix}.npz"
        np.savez(file_path, gt=gt, logits=logits, features=features, scores=scores)
        print(f"Target labels, logits, features and scores saved in: {file_path}")
        written[split] = file_path
        scorers = []                                      # what `--detection` scores: write() adds the detectors' rows
        if args.detection:                                # the background column is neither a known class nor a logit of one
            class_scores, class_logits = (scores[:, :-1], logits[:, :-1]) if args.loss == "garbage" else (scores, logits)
            scorers += [(name, class_scores, unknown) for name, unknown in logit_baselines(class_logits).items()]
            if args.gradnorm:
                scorers.append(gradnorm_scorer(class_scores, features, class_logits, args.gradnorm_temperature))
        if args.oscr:
            s = scores[:, :-1] if args.loss == "garbage" else scores           # the background column is not a known class
            for line in oscr_lines(split, gt, s):
                print(line)
        for row, detector in fitted:
            write(split, row["name"], row["tag"], gt,
                  scored_arrays(row["score"], detector, dict(gt=gt, logits=logits, features=features, **extra)))
        if proser is not None:
            p_gt, p_logits, p_features, _ = get_arrays(model=proser.model, loader=loader)
            write(split, "proser", "PROSER ", p_gt, proser_arrays(proser, dict(gt=p_gt, logits=p_logits, features=p_features)))
        if odin is not None:
            write(split, "odin", "ODIN ", gt, odin_arrays(odin, model, loader))
        if args.detection:
            rows = detection_rows(gt, scorers)
            for row in rows:
                print(detection_line(split, row))
            detection_path = args.output_directory / f"{args.loss}_{split}_detection{suffix}.json"
            with open(detection_path, "w") as handle:
                json.dump({"split": split, "protocol": args.protocol, "loss": args.loss, "epoch": start_epoch, "tpr": list(DETECTION_TPR),
                           "rows": rows}, handle, default=str)
            print(f"Detection metrics saved in: {detection_path}")
            written[f"{split}_detection"] = detection_path
        if args.auc:
            for unk in (-1, -2):
                sel = auc_rows(gt, scores, unk, args.loss)
                if sel is not None:
                    print(f"{split}: AUC known vs label {unk}: {metrics.auc_score_binary(sel[0], sel[1], unk_class=unk):.6f}")
        if args.report:
            report = evaluation_report(gt, scores, features, args.loss)
            report.update(split=split, protocol=args.protocol, epoch=start_epoch)
            report_path = args.output_directory / f"{args.loss}_{split}_report{suffix}.json"
            with open(report_path, "w") as handle:
                json.dump(report, handle, default=str)
            print(f"Evaluation report saved in: {report_path}")
            unk = -2 if "-2" in report["ccr_at_fpr"] else -1
            print(f"{split}: table row (CCR vs label {unk}): {table_row(report, args.protocol, args.loss, start_epoch, unk)}")
    return written


if __name__ == "__main__":
    main()
