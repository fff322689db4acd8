"""``dquartic`` command line -- same commands and options as the reference's ``dquartic/cli.py`` (:26-188):
``dquartic train CONFIG [--parquet_directory --ms2-data-path --ms1-data-path --batch-size --checkpoint-path --use-wandb
--threads]`` and ``dquartic generate-config PATH``; ``dquartic evaluate CONFIG --checkpoint PATH`` (this build) prints held-out loss and
reconstruction metrics; ``dquartic deconvolve CONFIG --checkpoint PATH --ms2 RUN.npy --ms1 RUN.npy --out OUT.npz --window W`` (this build)
deconvolves whole chromatograms (``--joint``: the P precursors of one run as groups under mixture consistency,
section 40); ``dquartic evaluate-joint CONFIG --checkpoint PATH --num-steps N --group-size P`` (this build) scores joint sampling on
held-out groups against P independent calls (section 45).  A ``data.mixture`` block in the config (absent by default) makes ``train`` and ``evaluate`` form K-component
mixtures with drawn weights on the GPU (``ResidentMixLoader``).  ``generate-train-data`` (offline sqMass ETL) is outside the hot path
and reports so.  Under ``torch.distributed.run`` (WORLD_SIZE > 1) training is data-parallel: one process per GPU, the
dataset is sharded by rank and the flat gradient is all-reduced over RCCL."""
import ast
import dataclasses
import functools
import json
import os

import click
import torch
from torch.utils.data import DataLoader

from .model.model import DDIMDiffusionModel, JointSampleOptions
from .model.unet1d import UNet1d
from .utils.config_loader import generate_train_config, load_train_config, mixture_config, validation_config


class PythonLiteralOption(click.Option):
    def type_cast_value(self, ctx, value):
        if not isinstance(value, str):
            return value
        try:
            return ast.literal_eval(value)
        except Exception:
            raise click.BadParameter(value)


@click.group(chain=True)
@click.version_option(package_name=None, version="0.1.0")
def cli():
    """Diffusion Deconvolution of DIA-MS/MS Data (D^4) -- MI355X build"""


@cli.command()
@click.argument("config-path", type=click.Path(exists=True), required=True)
@click.option("--parquet_directory", default=None, help="Directory of parquet slices (overrides the config)")
@click.option("--ms2-data-path", default=None, help="Path to MS2 .npy data (overrides the config)")
@click.option("--ms1-data-path", default=None, help="Path to MS1 .npy data (overrides the config)")
@click.option("--batch-size", default=None, help="Batch size (overrides the config)")
@click.option("--checkpoint-path", default=None, help="Where to save the best model (overrides the config)")
@click.option("--use-wandb", default=None, cls=PythonLiteralOption, help="Use wandb for logging (overrides the config)")
@click.option("--threads", default=None, help="Data-loading worker processes (overrides the config)")
@click.option("--resident-dataset", is_flag=True, default=False,
              help="Keep the whole dataset in HBM and form batches on the GPU (dq_pair_batch) instead of a DataLoader")
def train(config_path, parquet_directory, ms2_data_path, ms1_data_path, batch_size, checkpoint_path, use_wandb, threads,
          resident_dataset):
    """Train a DDIM model on DIA-MS windows."""
    world, rank, local = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise click.ClickException("no GPU visible: this build runs the hot path on MI355X only (no CPU fallback)")
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local))
    if rank == 0:
        click.echo("--" * 30)
        for i in range(torch.cuda.device_count()):
            click.echo(f"GPU {i}: {torch.cuda.get_device_name(i)}  {torch.cuda.get_device_properties(i).total_memory / 2**20:.0f} MB")
        click.echo("--" * 30)
        click.echo(f"Info: Loading config from {config_path}")
    config = load_train_config(config_path, parquet_directory=parquet_directory, ms2_data_path=ms2_data_path,
                               ms1_data_path=ms1_data_path, batch_size=batch_size, checkpoint_path=checkpoint_path,
                               use_wandb=use_wandb, threads=threads)
    m = config["model"]
    syn = config["data"].get("synthetic")
    dataset = build_dataset(config["data"], m, rank, world)
    per_rank = max(1, int(m["batch_size"]) // world)
    device = torch.device("cuda", local)
    mix = mixture_config(config["data"].get("mixture"))
    if mix is not None:
        # K-component mixtures with drawn weights: always formed on the GPU from the resident dataset.  The
        # synthetic dataset has sharded its window pool by rank itself; a file-backed one is shared and its epoch is divided.
        from .utils.data_loader import ResidentMixLoader

        shards = 1 if syn else world
        loader = ResidentMixLoader(dataset, per_rank, device=device, drop_last=len(dataset) // shards > per_rank, rank=rank,
                                   world_size=shards, **mix)
    elif resident_dataset and not syn:
        from .utils.data_loader import ResidentPairLoader

        loader = ResidentPairLoader(dataset, per_rank, device=device, drop_last=len(dataset) // world > per_rank, rank=rank, world_size=world)
    elif world > 1 and not syn:
        # data-parallel over a file-backed dataset: rank r draws the indices i with i % world == r of a per-epoch permutation
        # (SURVEY 8e).  (DIAMSDataset ignores the index and returns a random pair, data_loader.py:60-69, so this fixes the number
        # of batches per rank and epoch rather than the windows a rank sees; the synthetic dataset shards its window pool itself.)
        from torch.utils.data.distributed import DistributedSampler

        sampler = DistributedSampler(dataset, num_replicas=world, rank=rank, shuffle=True, drop_last=False)
        loader = DataLoader(dataset, batch_size=per_rank, sampler=sampler, num_workers=int(config["threads"]),
                            drop_last=len(dataset) // world > per_rank)
    else:
        loader = DataLoader(dataset, batch_size=per_rank, shuffle=True, num_workers=int(config["threads"]), drop_last=len(dataset) > per_rank)
    dm = build_model(m, device)
    enable_ema_from_config(dm, m)
    enable_cond_dropout_from_config(dm, m)
    val = validation_config(config)
    val_loader = None if val is None else build_validation_loader(val, m, per_rank, rank, world)
    wb = None
    if config["wandb"]["use_wandb"] and rank == 0:
        try:
            import wandb as wb

            w = config["wandb"]
            wb.init(project=w["wandb_project"], name=w["wandb_name"], id=w["wandb_id"], resume=w["wandb_resume"],
                    config={"architecture": w["wandb_architecture"], "dataset": w["wandb_dataset"], **m}, mode=w["wandb_mode"])
        except ImportError:
            click.echo("wandb is not installed; continuing without it")
            wb = None
    if val_loader is None:
        dm.train(loader, m["batch_size"], m["num_epochs"], m["warmup_epochs"], m["learning_rate"], wb is not None, m["checkpoint_path"])
    else:
        dm.train(loader, m["batch_size"], m["num_epochs"], m["warmup_epochs"], m["learning_rate"], wb is not None, m["checkpoint_path"],
                 val_dataloader=val_loader, val_every=val["val_every"])
    if wb is not None:
        wb.finish()
    if world > 1:
        torch.distributed.destroy_process_group()


def build_dataset(data, m, rank=0, world=1):
    """The dataset a ``data`` section (or a completed ``data.validation`` block) describes: the built-in synthetic one, or the files."""
    syn = data.get("synthetic")
    if syn:
        from .utils.synthetic import SyntheticDIAMSDataset

        return SyntheticDIAMSDataset(n_windows=int(syn.get("n_windows", 32)), RT=int(syn.get("RT", 400)),
                                     MZ=int(syn.get("MZ", m["UNet1d"]["downsample_dim"])), normalize=data["normalize"],
                                     rank=rank, world=world,
                                     ms1_channels=None if syn.get("ms1_channels") is None else int(syn["ms1_channels"]),
                                     start=int(syn.get("start", 0)))
    from .utils.data_loader import DIAMSDataset

    return DIAMSDataset(data["parquet_directory"], data["ms2_data_path"], data["ms1_data_path"], normalize=data["normalize"])


def build_validation_loader(val, m, batch_size, rank=0, world=1):
    """The held-out loader of a completed ``data.validation`` block (``validation_config``): ``n_pairs`` index pairs of its windows drawn
    from a generator of their own under the block's ``seed`` (``FrozenPairDataset``: the same pairs in every process and run), served in
    order -- what makes two ``evaluate`` runs comparable.  With a ``mixture`` in the block: the frozen form of ``ResidentMixLoader``, ``n_pairs``
    K-component items (None: one per window) whose indices and weights depend on the mixture's seed alone."""
    from .utils.synthetic import FrozenPairDataset

    if val.get("mixture") is not None:
        from .utils.data_loader import ResidentMixLoader

        dataset = build_dataset(val, m, rank, world)
        return ResidentMixLoader(dataset, batch_size, frozen_items=len(dataset) if val["n_pairs"] is None else val["n_pairs"],
                                 device=torch.device("cuda", torch.cuda.current_device()), **val["mixture"])
    return DataLoader(FrozenPairDataset(build_dataset(val, m, rank, world), val["n_pairs"], seed=val.get("seed", 0)),
                      batch_size=batch_size, shuffle=False)


def build_model(m, device):
    """The network and diffusion process a ``model`` section describes."""
    if m["use_model"] == "UNet1d":
        u = m["UNet1d"]
        net = UNet1d(dim=u["dim"], channels=u["channels"], dim_mults=tuple(u["dim_mults"]), conditional=u["conditional"],
                     init_cond_channels=u["init_cond_channels"], attn_cond_channels=u["attn_cond_channels"],
                     tfer_dim_mult=u["tfer_dim_mult"], downsample_dim=u["downsample_dim"], simple=u["simple"],
                     pos_output_only=bool(u.get("pos_output_only", False))).to(device)  # (reference configs without the key: False)
    elif m["use_model"] == "CustomTransformer":  # reference cli.py:102-109; served through the 4-argument adapter
        from .model.building_blocks import CustomTransformer, DDIMTransformerAdapter

        c = m["CustomTransformer"]
        net = DDIMTransformerAdapter(CustomTransformer(input_dim=c["input_dim"], hidden_dim=c["hidden_dim"], num_heads=c["num_heads"],
                                                       num_layers=c["num_layers"])).to(device)
    else:
        raise click.ClickException(f"Invalid model class: {m['use_model']}")  # reference cli.py:111 (ValueError there)
    dm = DDIMDiffusionModel(model_class=net, num_timesteps=m["num_timesteps"], beta_schedule_type=m["beta_schedule_type"],
                            pred_type=m["pred_type"], auto_normalize=m["auto_normalize"], ms1_loss_weight=m["ms1_loss_weight"],
                            device=device)
    if m["use_model"] == "CustomTransformer":  # "native_sampler": true sends every sample() to the library's loop (off by default)
        dm.native_tfm_sampler = bool(m["CustomTransformer"].get("native_sampler", False))
    return dm


def enable_ema_from_config(dm, m) -> bool:
    """``model.ema_decay`` (absent or null: off) and ``model.ema_warmup`` (default true) of a train config: keep an exponential moving
    average of the weights inside the optimiser step (``ModelInterface.enable_ema``).  The optimiser is created here, at the configured
    learning rate, because the average lives in it; ``train`` then finds it in place.  Returns whether EMA was enabled."""
    decay = m.get("ema_decay")
    if decay is None:
        return False
    dm._set_lr(m["learning_rate"])
    dm.enable_ema(float(decay), bool(m.get("ema_warmup", True)))
    return True


def enable_cond_dropout_from_config(dm, m) -> bool:
    """``model.cond_drop_prob`` (absent, null or 0: off) with the optional ``model.cond_drop_seed`` (default 0) and ``model.null_ms1``
    (default 0.0) of a train config: conditioning dropout for classifier-free guidance (``ModelInterface.set_cond_dropout``).  Returns
    whether it was turned on."""
    p = m.get("cond_drop_prob")
    if p is None:
        return False
    dm.set_cond_dropout(float(p), seed=int(m.get("cond_drop_seed", 0)), null_ms1=float(m.get("null_ms1", 0.0)))
    return dm.cond_dropout_enabled


def load_inference_checkpoint(dm, m, checkpoint, device, use_ema):
    """A checkpoint written by ``train`` into ``dm``: the weights, and its averaged weights when it has them and ``use_ema`` is not False
    (``use_ema`` True without an average in the file is an error)."""
    ck = torch.load(checkpoint, map_location=device, weights_only=False)
    dm.model.load_state_dict(ck["model_state_dict"])
    if ck.get("ema_state_dict") is not None and use_ema is not False:
        dm._set_lr(m["learning_rate"])
        dm.enable_ema(float(ck.get("ema_decay", 0.999)), bool(ck.get("ema_warmup", True)))
        dm.optimizer.load_ema_state_dict(ck["ema_state_dict"])
    elif use_ema:
        raise click.ClickException(f"--use-ema: {checkpoint} holds no averaged weights")


# The options of a sampling call, declared once for ``evaluate`` and ``deconvolve`` (between each command's own --num-steps and --use-ema)
_SAMPLING_OPTIONS = (
    click.option("--eta", default=0.0, type=float, help="DDIM eta of the sampling (0: deterministic update, 1: ancestral)"),
    click.option("--sampler", default="reference", type=click.Choice(["reference", "ddim", "dpmpp_2m"]),
                 help="Update of the sampling: the reference's, strided DDIM, or DPM-Solver++(2M)"),
    click.option("--clip-x0", default=None, type=float, help="Clamp every step's x0 estimate to [-C, C] (ddim / dpmpp_2m, eta 0)"),
    click.option("--guidance-scale", default=None, type=float,
                 help="Classifier-free guidance scale W of the sampling (UNet1d trained with model.cond_drop_prob; 1: the conditional model)"),
    click.option("--null-ms1", default=0.0, type=float, help="Raw MS1 value of the null condition (the training run's model.null_ms1)"),
    click.option("--guidance-rescale", default=0.0, type=float,
                 help="Rescaled guidance PHI in [0, 1]: scale each window's guided output towards the conditional output's spread (needs --guidance-scale)"),
    click.option("--threshold-quantile", default=None, type=float,
                 help="Dynamic thresholding: clamp every step's x0 estimate to the window's Q-quantile of |x0| (never below --clip-x0, or 1) and "
                      "scale it back to that floor (ddim / dpmpp_2m, eta 0)"),
    click.option("--threshold-max", default=None, type=float, help="Upper bound of the dynamic threshold (needs --threshold-quantile)"),
    click.option("--consistency", default=None, type=click.Choice(["bound", "sum"]),
                 help="Mixture consistency over the members of a group (deconvolve --joint): their positive parts never exceed the observed "
                      "window (bound), or add up to it (sum)"),
    click.option("--consistency-strength", default=1.0, type=float, help="Blend L in (0, 1] between each step's estimate and its projection"),
    click.option("--seed", default=0, type=int, help="Seed of x_T, of the sampling noise and of the evaluation noise"),
)


def sampling_options(command):
    """Declares ``_SAMPLING_OPTIONS`` on ``command`` and hands it ``eta``, ``seed`` and, in place of the options of ``JointSampleOptions``
    (taken by name; one that is not declared, as ``group_size``, stays at its default), ``sample_kw``: the ones that are not at their
    defaults, as ``evaluate`` / ``deconvolve_run`` / ``deconvolve_run_joint`` / ``sample`` take them"""
    @functools.wraps(command)
    def with_sample_kw(**kw):
        fields = dataclasses.fields(JointSampleOptions)
        return command(sample_kw=JointSampleOptions(**{f.name: kw.pop(f.name, f.default) for f in fields}).non_default(), **kw)

    for option in reversed(_SAMPLING_OPTIONS):
        with_sample_kw = option(with_sample_kw)
    return with_sample_kw


@cli.command()
@click.argument("config-path", type=click.Path(exists=True), required=True)
@click.option("--checkpoint", required=True, type=click.Path(exists=True), help="Checkpoint written by train (model_state_dict; its EMA when it has one)")
@click.option("--num-steps", default=None, type=int, help="Also sample every window with this many DDIM steps and report reconstruction metrics")
@sampling_options
@click.option("--use-ema/--no-use-ema", default=None, help="Evaluate the averaged weights (default: when the checkpoint has an average)")
@click.option("--max-batches", default=None, type=int, help="Stop after this many batches")
@click.option("--out", "out_path", default=None, type=click.Path(), help="Write the full result, per-window metrics included, as JSON")
def evaluate(config_path, checkpoint, num_steps, eta, seed, sample_kw, use_ema, max_batches, out_path):
    """Held-out loss (and, with --num-steps, reconstruction metrics) of a checkpoint on the config's data.validation set.  The pairs of
    that set come from the block's own seed, not from --seed: runs that differ in --seed, --eta, --num-steps or --use-ema score the same
    pairs.  Without a validation block the config's data section is scored, with a notice.  Prints one JSON line."""
    if "consistency" in sample_kw or "consistency_strength" in sample_kw:
        raise click.ClickException("--consistency: groups inside evaluate are not implemented (follow-up: a mixture loader that carries every "
                                   "member's MS1); use deconvolve --joint")
    if not torch.cuda.is_available():
        raise click.ClickException("no GPU visible: this build runs the hot path on MI355X only (no CPU fallback)")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    config = load_train_config(config_path)
    m = config["model"]
    val = validation_config(config)
    if val is None:
        click.echo("Notice: the config has no data.validation block; evaluating pairs of the TRAINING data section -- the result is "
                   "not a held-out loss", err=True)
        val = {**config["data"], "n_pairs": None, "seed": 0, "mixture": mixture_config(config["data"].get("mixture"))}
    loader = build_validation_loader(val, m, max(1, int(m["batch_size"])))
    dm = build_model(m, device)
    load_inference_checkpoint(dm, m, checkpoint, device, use_ema)
    res = dm.evaluate(loader, n_t=4, seed=seed, num_steps=num_steps, eta=eta, use_ema=use_ema, max_batches=max_batches, **sample_kw)
    # the per-window arrays go to --out only; the printed line keeps the scalars and the buckets (val_loss_by_weight among them)
    arrays = {k: res.pop(k).tolist() for k in ("per_window", "target_weight") if k in res}
    click.echo(json.dumps(res))
    if out_path is not None:
        with open(out_path, "w") as f:
            json.dump({**res, **arrays}, f)


def build_group_loader(val, m, groups_per_batch, group_size, rank=0, world=1):
    """The held-out loader of ``evaluate-joint``: ``build_validation_loader``'s frozen mixtures of a completed ``data.validation`` block,
    served as groups whose first ``group_size`` components are the members (``ResidentGroupLoader``; group k is item k of the loader
    ``evaluate`` scores)."""
    from .utils.data_loader import ResidentGroupLoader

    dataset = build_dataset(val, m, rank, world)
    return ResidentGroupLoader(dataset, groups_per_batch, group_size, frozen_items=len(dataset) if val["n_pairs"] is None else val["n_pairs"],
                               device=torch.device("cuda", torch.cuda.current_device()), **val["mixture"])


@cli.command("evaluate-joint")
@click.argument("config-path", type=click.Path(exists=True), required=True)
@click.option("--checkpoint", required=True, type=click.Path(exists=True), help="Checkpoint written by train (model_state_dict; its EMA when it has one)")
@click.option("--num-steps", required=True, type=int, help="Sampling steps per member")
@click.option("--group-size", required=True, type=int, help="Members P of a group: the first P components of every held-out mixture (1 .. kmin)")
@sampling_options
@click.option("--independent/--no-independent", default=True, help="Also sample every group without consistency (P independent calls) and score it")
@click.option("--use-ema/--no-use-ema", default=None, help="Evaluate the averaged weights (default: when the checkpoint has an average)")
@click.option("--max-batches", default=None, type=int, help="Stop after this many batches")
@click.option("--out", "out_path", default=None, type=click.Path(), help="Write the full result, the per-member and per-group arrays included, as JSON")
def evaluate_joint(config_path, checkpoint, num_steps, eta, seed, sample_kw, independent, use_ema, max_batches, out_path):
    """Score joint sampling (sample(group_size=P, consistency=...); deconvolve --joint) on the mixtures of the config's data.validation
    block: every mixture's first P components are sampled as one group under --consistency (default: bound) and, unless
    --no-independent, as P independent calls.  Reports the window metrics over all members, how far the members together exceed (excess)
    or miss (unexplained) the mixture, and how often a member's prediction looks most like its own target (id_acc; leak: how much it
    looks like another member's).  This is the route for --consistency inside an evaluation; `evaluate` scores one target per mixture.
    Prints one JSON line."""
    from .model.model import _JOINT_WITH_OPTIONS

    group_size = sample_kw.pop("group_size")  # (--group-size is one of JointSampleOptions' names: sampling_options hands it over in sample_kw)
    refused = [k for k in ("guidance_scale", "guidance_rescale", "threshold_quantile", "threshold_max") if k in sample_kw]
    if refused:
        raise click.ClickException(_JOINT_WITH_OPTIONS)
    config = load_train_config(config_path)
    m = config["model"]
    val = validation_config(config)
    if val is None or val.get("mixture") is None:
        raise click.ClickException("evaluate-joint needs a data.validation block with a mixture (data.mixture or data.validation.mixture): "
                                   "groups are the first --group-size components of its mixtures")
    kmin = int(val["mixture"]["n_components"][0])
    if not 1 <= group_size <= kmin:
        raise click.ClickException(f"--group-size {group_size}: the validation mixtures hold kmin = {kmin} .. {int(val['mixture']['n_components'][1])} "
                                   f"components (mixture.n_components); every group needs its members, so 1 <= --group-size <= kmin")
    if m["use_model"] != "UNet1d":
        raise click.ClickException("evaluate-joint: groups are built for UNet1d (dq_ddim_sample); other networks are not implemented")
    sample_kw.setdefault("consistency", "bound")
    if not torch.cuda.is_available():
        raise click.ClickException("no GPU visible: this build runs the hot path on MI355X only (no CPU fallback)")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    loader = build_group_loader(val, m, max(1, int(m["batch_size"])), group_size)
    dm = build_model(m, device)
    load_inference_checkpoint(dm, m, checkpoint, device, use_ema)
    try:
        res = dm.evaluate_joint(loader, num_steps, independent=independent, eta=eta, seed=seed, use_ema=use_ema, max_batches=max_batches, **sample_kw)
    except (NotImplementedError, ValueError) as e:  # what sample refuses, in its own words
        raise click.ClickException(str(e))
    # the arrays go to --out only; the printed line keeps the scalars and the buckets
    arrays = {"member_weight": res.pop("member_weight").tolist()}
    for leg in ("joint", "independent"):
        if leg in res:
            arrays[leg] = {k: res[leg].pop(k).tolist() for k in ("per_window", "cross", "group")}
    click.echo(json.dumps(res))
    if out_path is not None:
        full = {**res, "member_weight": arrays["member_weight"]}
        for leg in ("joint", "independent"):
            if leg in res:
                full[leg] = {**res[leg], **arrays[leg]}
        with open(out_path, "w") as f:
            json.dump(full, f)


@cli.command()
@click.argument("config-path", type=click.Path(exists=True), required=True)
@click.option("--checkpoint", required=True, type=click.Path(exists=True), help="Checkpoint written by train (model_state_dict; its EMA when it has one)")
@click.option("--ms2", "ms2_path", required=True, type=click.Path(exists=True),
              help="The observed run(s) as .npy: (RT_total, MZ), or (R, RT_total, MZ) for R runs processed in turn")
@click.option("--ms1", "ms1_path", required=True, type=click.Path(exists=True),
              help="The MS1 trace(s) as .npy: (RT_total,) or (RT_total, M1); with R runs (R, RT_total) or (R, RT_total, M1)")
@click.option("--out", "out_path", required=True, type=click.Path(), help="Write pred, overlap_var, coverage, scales and starts as .npz")
@click.option("--window", required=True, type=int, help="Scans per window (the window length the network was trained on)")
@click.option("--step", default=5, type=int, help="Scans between the starts of consecutive windows (1 .. window)")
@click.option("--taper", default="hann", type=click.Choice(["hann", "uniform"]), help="Weight of a window's scans where windows overlap")
@click.option("--batch-size", default=32, type=int, help="Windows sampled per call (the result does not depend on it)")
@click.option("--num-steps", default=1000, type=int, help="Sampling steps per window")
@click.option("--joint", is_flag=True, default=False,
              help="One run (--ms2 (RT_total, MZ)) with the MS1 traces of its P co-eluting precursors (--ms1 (P, RT_total) or (P, RT_total, M1)), "
                   "sampled as groups under --consistency (default: bound); pred and overlap_var gain a leading P axis")
@sampling_options
@click.option("--use-ema/--no-use-ema", default=None, help="Sample from the averaged weights (default: when the checkpoint has an average)")
def deconvolve(config_path, checkpoint, ms2_path, ms1_path, out_path, window, step, taper, batch_size, num_steps, joint, eta, seed, sample_kw,
               use_ema):
    """Deconvolve whole chromatograms with a checkpoint: every run is cut into overlapping windows, each window normalised on its own and
    sampled, and the predictions stitched back in intensity units (``deconvolve_run``).  Window i of run r samples under the id
    (windows of the runs before it) + i.  With --joint the P precursors of one run are sampled together (``deconvolve_run_joint``; member
    p's window i under the id p * windows + i).  Prints one JSON line: runs (--joint: members), windows, windows per second."""
    import time

    import numpy as np

    ms2, ms1 = np.load(ms2_path), np.load(ms1_path)
    if joint:
        if ms2.ndim != 2:
            raise click.ClickException(f"--ms2: --joint expects one run (RT_total, MZ), got {ms2.shape}")
        if ms1.ndim not in (2, 3) or ms1.shape[1] != ms2.shape[0]:
            raise click.ClickException(f"--ms1: --joint expects (P, RT_total) or (P, RT_total, M1) with RT_total = {ms2.shape[0]}, got {ms1.shape}")
        if not 1 <= ms1.shape[0] <= 8:
            raise click.ClickException(f"--ms1: --joint takes 1 .. 8 members, got {ms1.shape[0]}")
        sample_kw.setdefault("consistency", "bound")
    elif "consistency" in sample_kw or "consistency_strength" in sample_kw:
        raise click.ClickException("--consistency and --consistency-strength need --joint")
    if ms2.ndim not in (2, 3):
        raise click.ClickException(f"--ms2: expected (RT_total, MZ) or (R, RT_total, MZ), got {ms2.shape}")
    stacked = ms2.ndim == 3
    if not stacked:
        ms2, ms1 = ms2[None], ms1[None]
    if not joint and (ms1.ndim not in (2, 3) or ms1.shape[:2] != ms2.shape[:2]):
        raise click.ClickException(f"--ms1: expected {'(R, RT_total)' if stacked else '(RT_total,)'} with or without a trailing channel "
                                   f"dimension to go with --ms2 {tuple(ms2.shape[1 - stacked:])}, got {tuple(ms1.shape[1 - stacked:])}")
    if not 1 <= step <= window <= ms2.shape[1]:
        raise click.ClickException(f"need 1 <= --step <= --window <= RT_total, got step {step}, window {window}, RT_total {ms2.shape[1]}")
    if not torch.cuda.is_available():
        raise click.ClickException("no GPU visible: this build runs the hot path on MI355X only (no CPU fallback)")
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    m = load_train_config(config_path)["model"]
    dm = build_model(m, device)
    load_inference_checkpoint(dm, m, checkpoint, device, use_ema)
    outs, first = [], 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run = dm.deconvolve_run_joint if joint else dm.deconvolve_run  # (--joint: ms2[None] is the one run, ms1[None] its (P, ...) traces)
    for r in range(ms2.shape[0]):
        res = run(torch.from_numpy(np.ascontiguousarray(ms2[r], dtype=np.float32)).to(device),
                  torch.from_numpy(np.ascontiguousarray(ms1[r], dtype=np.float32)).to(device), window=window, step=step, taper=taper,
                  batch_size=batch_size, id_offset=first, num_steps=num_steps, eta=eta, seed=seed, use_ema=use_ema, **sample_kw)
        first += res["n_windows"] * (ms1.shape[1] if joint else 1)
        outs.append({k: res[k].cpu().numpy() for k in ("pred", "overlap_var", "coverage", "scales")})
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    arrays = {k: np.stack([o[k] for o in outs]) if stacked else outs[0][k] for k in outs[0]}
    np.savez(out_path, starts=res["starts"], **arrays)
    click.echo(json.dumps({"runs": int(ms1.shape[1] if joint else ms2.shape[0]), "windows": int(first), "windows_per_s": round(first / seconds, 2)}))


@cli.command()
@click.argument("config-path", type=click.Path(), required=True)
def generate_config(config_path):
    """Write the default training configuration."""
    click.echo(f"Info: Generating config at {config_path}")
    generate_train_config(config_path)


@cli.command()
@click.argument("input-file", type=click.Path(), required=True)
@click.argument("output-file", type=click.Path(), required=True)
def generate_train_data(input_file, output_file):
    """(not built) sqMass -> parquet slice ETL."""
    raise click.ClickException("generate-train-data is the reference's offline ETL on instrument files; it is outside the "
                                "accelerated hot path (SURVEY section 2) -- use the reference tool to produce parquet/npy slices")


if __name__ == "__main__":
    cli()
