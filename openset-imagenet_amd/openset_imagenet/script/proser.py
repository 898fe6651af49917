"""PROSER fine-tuning stage from a trained closed-set checkpoint (openset_imagenet/proser.py):
`python -m openset_imagenet.script.proser LOSS PROTOCOL -g [IDX] [--epochs E] [--dummy-count D] [--mix-at CUT] ...`.
Loads `{loss}_best.pth` (`--use-best`) or `{loss}_curr.pth` from the output directory, runs PROSER.train_epoch `--epochs` times on the
training split (the stem and the layers below `--mix-at` stay frozen; the suffix takes the fused SGD, the dummy classifier torch's),
calibrates the bias on the validation split and saves PROSER.state_dict() as `{loss}_proser{suffix}.pth`, which
`evaluate.py --proser` reads. Softmax and entropic losses only: the garbage loss already has a background class."""
import argparse
import pathlib

import torch

from .. import losses, optim, tools
from ..model import ResNet50
from ..proser import PROSER
from ..train import _image_loader, get_arrays, load_checkpoint


def get_args(command_line_options=None):
    p = argparse.ArgumentParser("PROSER fine-tuning parameters", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("loss", choices=["entropic", "softmax", "garbage"], help="Which trained network to fine-tune")
    p.add_argument("protocol", type=int, choices=(1, 2, 3), help="Open set protocol: 1, 2 or 3")
    p.add_argument("--use-best", "-b", action="store_true", help="Take the best model of the validation set, otherwise the last")
    p.add_argument("--gpu", "-g", type=int, nargs="?", default=None, const=0, help="GPU index (bare -g = 0); required")
    p.add_argument("--imagenet-directory", type=pathlib.Path, default=pathlib.Path("/local/scratch/datasets/ImageNet/ILSVRC2012/"))
    p.add_argument("--protocol-directory", type=pathlib.Path, default="protocols", help="Where are the protocol files stored")
    p.add_argument("--output-directory", default="experiments/Protocol_{}", help="Where the trained checkpoint lies and the result goes")
    p.add_argument("--batch-size", type=int, default=64)
    p.add_argument("--workers", type=int, default=4)
    p.add_argument("--epochs", type=int, default=3, help="epochs of the fine-tuning stage")
    p.add_argument("--dummy-count", type=int, default=5, help="outputs of the dummy classifier (placeholders)")
    p.add_argument("--mix-at", default="layer3", help="the cut: layers below it are frozen, its input is mixed")
    p.add_argument("--lambdas", type=float, nargs=3, default=(0.01, 1.0, 1.0), help="factors of the mixed, the clean and the left-out term")
    p.add_argument("--alpha", type=float, default=1.0, help="the mixing weight is drawn from Beta(alpha, alpha)")
    p.add_argument("--lr", type=float, default=1e-3, help="learning rate of both optimizers (SGD, momentum 0.9)")
    p.add_argument("--known-rate", type=float, default=0.95, help="share of the known validation rows the calibrated bias keeps known")
    p.add_argument("--seed", type=int, default=None, help="seed of the pair / weight generator")
    args = p.parse_args(command_line_options)
    if args.loss == "garbage":
        p.error("PROSER needs a network without a background class: use it with the softmax or entropic loss, not with garbage")
    try:
        args.output_directory = str(args.output_directory).format(args.protocol)
    except Exception:
        pass
    args.output_directory = pathlib.Path(args.output_directory)
    return args


def main(command_line_options=None):
    import numpy as np
    args = get_args(command_line_options)
    if args.gpu is None:
        raise RuntimeError("No GPU device selected: the MI355X build has no CPU path (pass -g [index])")
    tools.set_device_gpu(index=args.gpu)
    train_ds = _image_loader(args.protocol_directory / f"p{args.protocol}_train.csv", args.imagenet_directory, True, args.loss)
    val_ds = _image_loader(args.protocol_directory / f"p{args.protocol}_val.csv", args.imagenet_directory, False, "eval")
    n_classes = val_ds.table.label_count - 1
    suffix = "_best" if args.use_best else "_curr"
    model = ResNet50(fc_layer_dim=n_classes, out_features=n_classes, logit_bias=False)
    checkpoint = args.output_directory / (args.loss + suffix + ".pth")
    start_epoch, best_score = load_checkpoint(model, checkpoint)
    print(f"Fine-tuning the model of epoch {start_epoch} (score {best_score}) from {checkpoint}")
    tools.device(model)
    proser = PROSER(model, dummy_count=args.dummy_count, mix_at=args.mix_at, lambdas=tuple(args.lambdas), alpha=args.alpha,
                    generator=np.random.default_rng(args.seed))
    opt_model = optim.SGD(model, lr=args.lr, momentum=0.9)
    opt_dummy = torch.optim.SGD(proser.dummy_classifier.parameters(), lr=args.lr, momentum=0.9)
    # whole batches only: the executor is built for one geometry
    loader = torch.utils.data.DataLoader(train_ds, batch_size=args.batch_size, shuffle=True, num_workers=args.workers, drop_last=True)
    trackers = {"j": losses.AverageMeter()}
    for epoch in range(1, args.epochs + 1):
        proser.train_epoch(loader, opt_model, opt_dummy, trackers)
        print(f"PROSER epoch {epoch}/{args.epochs}: loss {trackers['j'].avg:.6f}")
    val_loader = torch.utils.data.DataLoader(val_ds, batch_size=args.batch_size, num_workers=args.workers)
    gt, logits, features, _ = get_arrays(model=model, loader=val_loader)
    proser.fit_bias(logits, proser.dummy_logits(features), gt, known_rate=args.known_rate)
    out = args.output_directory / f"{args.loss}_proser{suffix}.pth"
    torch.save(proser.state_dict(), out)
    print(f"PROSER (dummy {args.dummy_count}, mix at {args.mix_at}, bias {float(proser.bias):.6f}) saved in: {out}")
    return out


if __name__ == "__main__":
    main()
