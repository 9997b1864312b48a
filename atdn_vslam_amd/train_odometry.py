"""`train_odometry.py` of the reference on the HBM flow bank: CLVO training from KITTI frames.

    python -m atdn_vslam_amd.train_odometry --config config.yaml --flow-weights gma-kitti.pth [--geometry slam|crop]
    python -m atdn_vslam_amd.train_odometry --config config.yaml --flows2          # import dataset/flows2 instead
    ... [--init PATH] [--save-flows2] [--gpus N] [--composite reference|gradient]

The configuration is the reference's YAML (`Arguments`, README): data_path, train_sequences, batch_size, sequence_length,
epochs, lr, wd, epsilon, stage, weight_file, log_file, augment_flow, alpha, w. The loop is train_odometry.py:59-145:
`torch.manual_seed(4265664478)`, a shuffling DataLoader that drops the last partial batch, ATDNVO's default
initialisation (or the previous stage's weights), AdamW under CosineAnnealingLR(epochs * len(loader), eta_min=1e-9),
and per epoch a loss log `log_file + str(stage-1) + "_" + str(epoch) + ".txt"` and a checkpoint
`weight_file + str(stage) + "_atdnvo_c.pth"`. Every batch is one atdn_flow_gather_clips into a persistent fp32 buffer
and one CLVOTrainer.step.

Targets are computed in float64 (as the reference does) and rounded to fp32 when handed to the trainer, whose contract is
fp32 targets; the reference subtracts float64 targets from fp32 predictions.

`alpha` and `w` (CLVO_Loss): without `--composite` only alpha = 1 is accepted and `w` is read and unused, since the composite
term that takes it is multiplied by zero. `--composite reference|gradient` hands the YAML's `alpha` and `w` to the trainer:
"reference" evaluates the composite term for the logged loss only and scales the relative-pose gradient by alpha (the
reference's detached graph, as the CPU oracle restates it), "gradient" lets the term steer the weights
(atdn_vslam_amd/training.py). The per-epoch log holds the total loss either way, as the reference's does.

`--gpus N`: N ranks started here (launch.spawn_ranks_if_needed); every rank builds or loads the whole bank and draws the
same seeded stream, and rank r trains on the contiguous slice [r*B/N, (r+1)*B/N) of each global batch.
"""
import argparse
import os
import sys

if __name__ == "__main__":   # before torch is imported / any GPU call: the parent only starts the ranks
    # (the ranks run this file as a script: the package is imported from the repository root, not from this directory)
    _here = os.path.dirname(os.path.abspath(__file__))
    sys.path = [p for p in sys.path if os.path.abspath(p or ".") != _here]
    sys.path.insert(0, os.path.dirname(_here))
    from atdn_vslam_amd.launch import spawn_ranks_if_needed
    _rc = spawn_ranks_if_needed(os.path.abspath(__file__))
    if _rc is not None:
        sys.exit(_rc)

import numpy as np
import torch

from atdn_vslam_amd import flowbank as fb

CONFIG_KEYS = ("data_path", "train_sequences", "batch_size", "sequence_length", "epochs", "lr", "wd", "epsilon", "stage",
               "weight_file", "log_file", "augment_flow", "alpha", "w")
ARGUMENT_TAGS = ("tag:yaml.org,2002:python/object:utils.arguments.Arguments",
                 "tag:yaml.org,2002:python/object:atdn_vslam.utils.arguments.Arguments")


class Config(argparse.Namespace):
    """The reference's `Arguments` object, as plain attributes."""


def load_config(path):
    """The reference's config.yaml through a safe loader. Both the README's `!!python/object:utils.arguments.Arguments`
    tag and the package path `atdn_vslam.utils.arguments.Arguments` are accepted (nothing is imported or executed)."""
    import yaml

    class _Loader(yaml.SafeLoader):
        pass

    for tag in ARGUMENT_TAGS:
        _Loader.add_constructor(tag, lambda loader, node: loader.construct_mapping(node, deep=True))
    with open(path) as f:
        d = yaml.load(f, Loader=_Loader)
    if not isinstance(d, dict):
        raise ValueError("%s: expected a mapping of Arguments fields" % path)
    missing = [k for k in CONFIG_KEYS if k not in d and k not in ("alpha", "w")]
    if missing:
        raise KeyError("%s lacks %s" % (path, ", ".join(missing)))
    cfg = Config(**d)
    cfg.alpha = d.get("alpha", 1)
    cfg.w = d.get("w", 3)
    cfg.train_sequences = [str(s) for s in cfg.train_sequences]
    return cfg


def check_alpha(cfg, composite=None):
    """Without a composite mode only alpha = 1 trains; with one, `w` must fit the clip. Runs before any GPU work."""
    if composite is None:
        if cfg.alpha != 1:
            raise NotImplementedError("alpha = %r: without --composite the trainer runs CLVO_Loss(alpha = 1) only; choose "
                                      "--composite reference (the composite term is detached, as in the reference, and alpha scales "
                                      "the relative-pose gradient) or --composite gradient (the term gets its true gradient)"
                                      % (cfg.alpha,))
        return
    from atdn_vslam_amd.training import composite_mode
    composite_mode(composite)
    if not 1 <= int(cfg.w) <= int(cfg.sequence_length):
        raise ValueError("w = %r: the composite window needs 1 <= w <= sequence_length (%d)" % (cfg.w, int(cfg.sequence_length)))


def checkpoint_path(cfg):
    """train_odometry.py:138: weight_file + stage + "_" + "ATDNVO_c".lower() + ".pth"."""
    return cfg.weight_file + str(cfg.stage) + "_atdnvo_c.pth"


def log_path(cfg, epoch):
    """train_odometry.py:136."""
    return cfg.log_file + str(cfg.stage - 1) + "_" + str(epoch) + ".txt"


def init_path(cfg, init=None, warn=sys.stderr):
    """The weights a stage starts from: `init` when given; for stage > 1 the reference's
    weight_file + str(stage-1) + ".pth" (train_odometry.py:94-97), or, when that file is missing, what the previous stage
    actually saved (weight_file + str(stage-1) + "_atdnvo_c.pth"); None for stage 1 (default initialisation)."""
    if init:
        return init
    if cfg.stage <= 1:
        return None
    ref = cfg.weight_file + str(cfg.stage - 1) + ".pth"
    if os.path.exists(ref):
        return ref
    saved = cfg.weight_file + str(cfg.stage - 1) + "_atdnvo_c.pth"
    if os.path.exists(saved):
        if warn is not None:
            warn.write("train_odometry: %s does not exist; loading %s, the checkpoint stage %d saved\n" % (ref, saved, cfg.stage - 1))
        return saved
    raise FileNotFoundError("stage %d starts from %s (or %s): neither exists" % (cfg.stage, ref, saved))


def count_frames(data_path, sequence):
    import glob
    im = os.path.join(data_path, "dataset", "sequences", sequence, "image_2")
    n = len(glob.glob(os.path.join(im, "*.png")))
    return n if n else len(fb.read_poses(data_path, sequence))


def build_bank(cfg, device, flow_weights=None, flows2=False, geometry="slam", batch=16, log=None):
    """A FlowBank holding every training sequence: computed by the flow network from the PNG frames, or imported from
    dataset/flows2."""
    n_frames = [count_frames(cfg.data_path, s) for s in cfg.train_sequences]
    bank = fb.FlowBank(device, sum(n - 1 for n in n_frames))
    if flows2:
        bank.load_flows2(cfg.data_path, cfg.train_sequences)
        return bank
    if flow_weights is None:
        raise ValueError("computing the flow bank needs --flow-weights (a GMA checkpoint), or --flows2 to import flows")
    from atdn_vslam_amd.modules import RAFTGMA
    net = RAFTGMA(max_batch=batch)
    sd = torch.load(flow_weights, map_location="cpu") if isinstance(flow_weights, (str, os.PathLike)) else flow_weights
    net.load_state_dict(sd)
    net = net.to(device).eval()
    for s in cfg.train_sequences:
        frames = fb.KittiSequence(cfg.data_path, s)
        try:
            bank.add_sequence(s, frames, fb.read_poses(cfg.data_path, s), net, geometry=geometry, batch=batch)
        finally:
            frames.close()
        if log:
            log("flow bank: sequence %s, %d flows" % (s, bank.sequence(s).n_flows))
    return bank


def train(cfg, bank, device, init_state=None, rank=0, world=1, group=None, on_step=None, log=None, save=True, composite=None):
    """The epoch loop of train_odometry.py on `bank`. Seeds torch, builds the sampler and the initial weights exactly as
    the reference orders them, then trains; returns (trainer, per-epoch loss lists). `on_step(epoch, batch, seq_idx,
    clips, reverse, loss)` is called after every iteration with this rank's slice of the batch. `composite` (None,
    "reference" or "gradient"): None trains CLVO_Loss(alpha = 1) and refuses any other alpha; a mode hands cfg.alpha and
    cfg.w to the trainer (training.py)."""
    from atdn_vslam_amd.training import CLVOTrainer
    check_alpha(cfg, composite)
    loss_args = {} if composite is None else dict(alpha=float(cfg.alpha), w=int(cfg.w), composite=composite)
    B, N = int(cfg.batch_size), int(cfg.sequence_length)
    lo, hi = fb.rank_slice(B, world, rank)
    seqs = [bank.sequence(s) for s in cfg.train_sequences]
    torch.manual_seed(fb.TRAIN_SEED)
    index = fb.ClipIndex([s.n_frames for s in seqs], N, augment=cfg.augment_flow)
    loader = fb.make_loader(index, B)
    state = fb.initial_clvo_state(B)
    if init_state is not None:
        state = init_state
    trainer = CLVOTrainer(state, hi - lo, N, hw=bank.hw, device=device, lr=cfg.lr, weight_decay=cfg.wd, eps=cfg.epsilon,
                          total_steps=cfg.epochs * len(loader), eta_min=1e-9, group=group, **loss_args)
    buf = torch.empty((hi - lo, N, 2) + bank.hw, dtype=torch.float32, device=device)
    firsts = np.array([s.first for s in seqs], dtype=np.int64)
    history = []
    for epoch in range(int(cfg.epochs)):
        losses = []
        for it, (si, ci, rv) in enumerate(loader):
            si, ci, rv = si[lo:hi].numpy(), ci[lo:hi].numpy(), rv[lo:hi].numpy()
            bank.gather(firsts[si] + ci, rv, N, out=buf)
            rot, tr = fb.batch_targets(seqs, si, ci, rv, N)
            loss = trainer.step(buf, torch.from_numpy(rot).float(), torch.from_numpy(tr).float())
            losses.append(loss)
            if on_step is not None:
                on_step(epoch, it, si, ci, rv, loss)
        if world > 1:
            import torch.distributed as dist
            t = torch.tensor(losses, dtype=torch.float64, device=device)
            dist.all_reduce(t, group=group)
            losses = (t / world).cpu().tolist()
        history.append(losses)
        if save and rank == 0:
            np.savetxt(log_path(cfg, epoch), np.array(losses))
            torch.save(trainer.state_dict(), checkpoint_path(cfg))
            if log:
                log("epoch %d/%d: mean loss %.6g; saved %s" % (epoch + 1, cfg.epochs, float(np.mean(losses)) if losses else float("nan"),
                                                             checkpoint_path(cfg)))
    return trainer, history


def main(argv=None):
    ap = argparse.ArgumentParser(description="CLVO training on the HBM flow bank (the reference's train_odometry.py)")
    ap.add_argument("--config", required=True, help="the reference's config.yaml (Arguments)")
    ap.add_argument("--flow-weights", default=None, help="GMA checkpoint used to compute the flows")
    ap.add_argument("--flows2", action="store_true", help="import <data_path>/dataset/flows2 instead of computing flows")
    ap.add_argument("--save-flows2", action="store_true", help="write the computed bank as <data_path>/dataset/flows2")
    ap.add_argument("--geometry", default="slam", choices=fb.GEOMETRIES)
    ap.add_argument("--flow-batch", type=int, default=16, help="frame pairs per flow-network call while building the bank")
    ap.add_argument("--init", default=None, help="starting weights (overrides the stage rule)")
    ap.add_argument("--gpus", type=int, default=None)
    ap.add_argument("--composite", default=None, choices=("reference", "gradient"),
                    help="train with the YAML's alpha and w: the composite term detached as in the reference, or with its gradient")
    a = ap.parse_args(argv)
    cfg = load_config(a.config)
    check_alpha(cfg, a.composite)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus is not None and a.gpus != world:
        raise SystemExit("%d rank(s) for --gpus %d" % (world, a.gpus))
    fb.rank_slice(int(cfg.batch_size), world, rank)   # (a batch that does not divide fails before any GPU work)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    group = None
    if world > 1:
        import torch.distributed as dist
        dist.init_process_group("nccl", device_id=dev)

    def log(msg):
        if rank == 0:
            print(msg, flush=True)

    bank = build_bank(cfg, dev, flow_weights=a.flow_weights, flows2=a.flows2, geometry=a.geometry, batch=a.flow_batch, log=log)
    if a.save_flows2 and rank == 0:
        bank.save_flows2(cfg.data_path)
    p = init_path(cfg, a.init)
    init_state = None
    if p is not None:
        log("loading weights from %s" % p)
        init_state = torch.load(p, map_location="cpu")
    train(cfg, bank, dev, init_state=init_state, rank=rank, world=world, group=group, log=log, composite=a.composite)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
