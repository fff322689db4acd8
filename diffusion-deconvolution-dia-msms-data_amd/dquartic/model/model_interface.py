"""Training / prediction harness -- drop-in for the reference's ``dquartic.model.model_interface``
(reference model_interface.py:64-236 schedulers/callbacks, :238-1150 ModelInterface).

Kept: the public method names, signatures, checkpoint dictionary (``epoch, model_state_dict, optimizer_state_dict,
scheduler_state_dict, best_loss``; reference :617-626), "latest" + "best" checkpoint cadence (:419-430), per-epoch
warm-up + cosine LambdaLR (:149-155, :400), the ``(ms2_1, ms1_1, ms2_2, ms1_2)`` batch contract with
``ms2_cond = 0.5*ms2_1 + 0.5*ms2_2`` (:1070-1075) and the step sequence of ``_train_one_batch`` (:1112-1123):
zero_grad -> train_step -> backward -> clip_grad_norm_(10) -> AdamW -> loss float.

Changed (DESIGN.md "deviations"): when the network is this package's ``UNet1d`` the step runs through two native
calls on flat buffers (``dq_train_step`` + ``dq_adamw_clip_step``) instead of autograd; with ``torch.distributed``
initialised the flat gradient is all-reduced (RCCL) between them; wandb / plotting are optional and imported lazily;
the "latest" checkpoint goes next to ``checkpoint_path`` ('.' when it has no directory, not the filesystem root).
"""
import contextlib
import math
import os
from collections import OrderedDict
from typing import List

import numpy as np
import torch

from .. import _native as N


# ----------------------------------------------------------------------------------------------------------------
# learning-rate schedule (reference model_interface.py:64-194)
# ----------------------------------------------------------------------------------------------------------------
class LR_SchedulerInterface(object):
    def __init__(self, optimizer: torch.optim.Optimizer, **kwargs):
        raise NotImplementedError

    def step(self, epoch: int, loss: float):
        raise NotImplementedError

    def get_last_lr(self) -> float:
        raise NotImplementedError


class WarmupLR_Scheduler(LR_SchedulerInterface):
    """Linear warm-up then cosine decay, stepped once per epoch."""

    def __init__(self, optimizer, num_warmup_steps: int, num_training_steps: int, num_cycles: float = 0.5, last_epoch: int = -1):
        self.optimizer = optimizer
        self.lambda_lr = self.get_cosine_schedule_with_warmup(optimizer, num_warmup_steps, num_training_steps, num_cycles, last_epoch)

    def step(self, epoch: int = None, loss=None):
        return self.lambda_lr.step()

    def get_last_lr(self) -> List[float]:
        return self.lambda_lr.get_last_lr()

    @staticmethod
    def _lr_lambda(current_step: int, *, num_warmup_steps: int, num_training_steps: int, num_cycles: float):
        if current_step < num_warmup_steps:
            return float(current_step + 1) / float(max(1, num_warmup_steps))
        progress = float(current_step - num_warmup_steps) / float(max(1, num_training_steps - num_warmup_steps))
        return max(1e-10, 0.5 * (1.0 + math.cos(math.pi * float(num_cycles) * 2.0 * progress)))

    def get_cosine_schedule_with_warmup(self, optimizer, num_warmup_steps, num_training_steps, num_cycles=0.5, last_epoch=-1):
        from functools import partial

        fn = partial(self._lr_lambda, num_warmup_steps=num_warmup_steps, num_training_steps=num_training_steps, num_cycles=num_cycles)
        return torch.optim.lr_scheduler.LambdaLR(optimizer, fn, last_epoch)


class CallbackHandler:
    """Hooks at epoch / batch end; ``epoch_callback`` returning False stops training (reference :196-236)."""

    def epoch_callback(self, epoch: int, epoch_loss: float) -> bool:
        return True

    def batch_callback(self, batch: int, batch_loss: float):
        pass


# ----------------------------------------------------------------------------------------------------------------
# AdamW over the flat parameter buffer (K11)
# ----------------------------------------------------------------------------------------------------------------
class FlatAdamW(torch.optim.Optimizer):
    """``torch.optim.AdamW`` semantics (torch defaults) executed by ``dq_adamw_clip_step`` on the network's flat
    parameter / gradient buffers, with the global-norm clip of ``clip_grad_norm_`` folded in.  ``state_dict()`` has the
    torch AdamW layout (per-parameter ``step, exp_avg, exp_avg_sq``), so checkpoints interchange with the reference.

    ``ema_decay`` (None: off) keeps an exponential moving average of the weights in a flat buffer with the layout of ``flat_params``, updated
    by the optimiser kernel itself from the parameter it has just formed (``dq_adamw_clip_ema_step`` / ``_dev``):
    after step t, ``e += w_t (p - e)`` with ``w_t = float32(1 - beta_t)``, ``beta_t = min(ema_decay, (1 + t) / (10 + t))`` under
    ``ema_warmup`` and ``ema_decay`` without.  The decay reaches the kernel as a float32.  The average is not part of ``state_dict()``
    (that stays torch's AdamW layout): ``ema_state_dict()`` / ``load_ema_state_dict()`` carry it."""

    def __init__(self, net, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, max_norm=10.0, ema_decay=None, ema_warmup=True):
        self.net = net
        params = [p for _, p in net.trainable_named()]
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))
        self.max_norm = max_norm
        self.grad_scale = 1.0
        self._m = self._v = self._scratch = self._gnorm = None
        self._step = 0
        self._step_dev = self._lr_dev = None   # device copies of the step count / learning rate (step_dev(): graph-replayable step)
        self._lr_dev_value = None
        self.ema_decay, self.ema_warmup, self._ema = None, True, None
        if ema_decay is not None:
            self.enable_ema(ema_decay, ema_warmup)

    # ---- exponential moving average of the weights
    def enable_ema(self, decay, warmup=True):
        """Start (or re-parametrise) the average.  A new average is a copy of the parameters at this moment; an existing one is kept."""
        if isinstance(decay, bool) or not isinstance(decay, (int, float, np.floating, np.integer)):
            raise TypeError(f"FlatAdamW: ema_decay must be a number, got {decay!r}")
        decay = float(decay)
        if not (0.0 <= decay < 1.0 and float(np.float32(decay)) < 1.0):  # (also false for NaN; the kernel takes the decay as a float32)
            raise ValueError(f"FlatAdamW: ema_decay must satisfy 0 <= ema_decay < 1 (as a float32), got {decay!r}")
        self.ema_decay, self.ema_warmup = decay, bool(warmup)
        if self._ema is None:
            self._ema = self.net.flat_params.detach().clone()
        return self

    def disable_ema(self):
        self.ema_decay, self._ema = None, None
        return self

    @property
    def ema_enabled(self) -> bool:
        return self.ema_decay is not None

    def ema_buffer(self) -> torch.Tensor:
        """The flat average, on the parameters' device (it follows them like the moments do)."""
        if self._ema is None:
            raise RuntimeError("FlatAdamW: EMA is not enabled (enable_ema(decay) or ema_decay=...)")
        flat = self.net.flat_params
        if self._ema.device != flat.device:
            self._ema = self._ema.to(flat.device)
        return self._ema

    @torch.no_grad()
    def reset_ema(self):
        """The average becomes a copy of the current parameters (after weights were loaded from a file that has no average)."""
        self.ema_buffer().copy_(self.net.flat_params)

    def ema_state_dict(self):
        """``{parameter name: view of the average}`` with the keys, order and shapes of the model's ``state_dict()``: it loads into the
        reference's module with ``load_state_dict``.  Entries the optimiser does not train (the U-Net's RoPE frequencies) are the model's own."""
        ema = self.ema_buffer()
        views = {name: ema[o:o + math.prod(shape)].view(shape) for name, o, shape in self.net._layout}
        return OrderedDict((k, views.get(k, v)) for k, v in self.net.state_dict().items())

    @torch.no_grad()
    def load_ema_state_dict(self, sd):
        ema = self.ema_buffer()
        missing = [name for name, _, _ in self.net._layout if name not in sd]
        if missing:
            raise KeyError(f"load_ema_state_dict: missing {missing[:3]}{' ...' if len(missing) > 3 else ''}")
        for name, o, shape in self.net._layout:
            src = torch.as_tensor(sd[name])
            if tuple(src.shape) != tuple(shape):
                raise ValueError(f"load_ema_state_dict: {name} has shape {tuple(src.shape)}, the network's is {tuple(shape)}")
            ema[o:o + math.prod(shape)].copy_(src.reshape(-1))

    def _native_step(self, flat, dev: bool):
        """One optimiser call: ``dq_adamw_clip[_ema]_step[_dev]``.  The four entries take the same arguments but for the step's scalars
        (``dev``: lr and step count from device memory, else the host's) and the average's three behind the norm."""
        g = self.param_groups[0]
        name = "dq_adamw_clip" + ("_ema" if self.ema_enabled else "") + "_step" + ("_dev" if dev else "")
        lr = N.ptr(self._lr_dev) if dev else float(g["lr"])
        step = N.ptr(self._step_dev) if dev else int(self._step)
        ema = (N.ptr(self.ema_buffer()), float(self.ema_decay), 1 if self.ema_warmup else 0) if self.ema_enabled else ()
        N.check(getattr(N.lib(), name)(N.ptr(flat), N.ptr(self.net.flat_grads()), N.ptr(self._m), N.ptr(self._v), flat.numel(), N.ptr(self._scratch),
                                       float(self.grad_scale), float(self.max_norm), lr, float(g["betas"][0]), float(g["betas"][1]),
                                       float(g["eps"]), float(g["weight_decay"]), step, N.ptr(self._gnorm), *ema, N.stream_ptr()), name)

    def _buffers(self):
        flat = self.net.flat_params
        if self._m is None or self._m.device != flat.device:
            old_m, old_v = self._m, self._v
            self._m = torch.zeros_like(flat) if old_m is None else old_m.to(flat.device)
            self._v = torch.zeros_like(flat) if old_v is None else old_v.to(flat.device)
            if self._ema is not None:
                self._ema = self._ema.to(flat.device)
            self._scratch = torch.empty(1024, dtype=torch.float32, device=flat.device)
            self._gnorm = torch.zeros((), dtype=torch.float32, device=flat.device)
            self._publish_state()
        return flat

    def _publish_state(self):
        for (name, o, shape), p in zip(self.net._layout, self.param_groups[0]["params"]):
            n = p.numel()
            self.state[p] = {"step": torch.tensor(float(self._step)), "exp_avg": self._m[o:o + n].view(shape),
                             "exp_avg_sq": self._v[o:o + n].view(shape)}

    @torch.no_grad()
    def step(self, closure=None):
        flat = self._buffers()
        self._step += 1
        self._native_step(flat, dev=False)
        return None  # (the per-parameter "step" entries are refreshed by state_dict(): 395 tensor constructions per step cost ~1 ms of host time)

    def state_dict(self):
        for st in self.state.values():
            st["step"] = torch.tensor(float(self._step))
        return super().state_dict()

    def _dev_state(self):
        """Device copies of the step count and the learning rate for ``step_dev``; the lr copy is refreshed when the scheduler changed it."""
        flat = self._buffers()
        if self._step_dev is None or self._step_dev.device != flat.device:
            self._step_dev = torch.tensor([self._step], dtype=torch.int32, device=flat.device)
            self._lr_dev = torch.zeros(2, dtype=torch.float32, device=flat.device)  # (hi, lo): the double lr as two floats
            self._lr_dev_value = None
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_dev_value:
            hi = float(np.float32(lr))
            self._lr_dev.copy_(torch.tensor([hi, float(np.float32(lr - hi))], dtype=torch.float32), non_blocking=False)
            self._lr_dev_value = lr
        return flat

    @torch.no_grad()
    def step_dev(self, count: bool = True):
        """The same update with the step count and lr read from device memory (``dq_adamw_clip_step_dev``): the call is identical from
        step to step, so it can sit in a captured graph.  ``count=False`` while a graph is being captured (the replay counts instead)."""
        flat = self._dev_state()
        if count:
            self._step += 1
        self._native_step(flat, dev=True)
        return None

    def sync_step_dev(self):
        """After the host-side step count changed outside step_dev (plain step(), load_state_dict): push it to the device copy."""
        if self._step_dev is not None:
            self._step_dev.fill_(self._step)

    def zero_grad(self, set_to_none: bool = False):
        self.net.flat_grads(zero=True)

    @property
    def last_grad_norm(self) -> torch.Tensor:
        """Pre-clip global gradient norm of the last step (0-dim device tensor)."""
        return self._gnorm

    def load_state_dict(self, state_dict):
        self._buffers()
        super().load_state_dict(state_dict)
        # copy the loaded moments back into the flat buffers and re-publish views
        step = 0
        for (name, o, shape), p in zip(self.net._layout, self.param_groups[0]["params"]):
            st = self.state.get(p)
            if st:
                n = p.numel()
                self._m[o:o + n].copy_(st["exp_avg"].reshape(-1))
                self._v[o:o + n].copy_(st["exp_avg_sq"].reshape(-1))
                step = int(float(st["step"]))
        self._step = step
        self._publish_state()
        self.sync_step_dev()


class BucketedAllReduce:
    """Gradient all-reduce overlapped with the backward that produces the gradients -- what DistributedDataParallel's reducer does
    for the reference (model_interface.py:953-957), driven here by the backward itself: ``on_bucket(i, offset, count)`` is called
    by CustomTransformer._run_bwd when the kernels writing ``grads[offset:offset+count]`` are on the compute stream; the slice's
    all-reduce (sum) is started at once on a communication stream that waits for exactly that point, so a layer's 50 MB of
    gradients (hidden 1024) cross xGMI while the layers below it are still being differentiated.  ``finish()`` makes the compute
    stream wait for every bucket.  One bucket per layer: at hidden 1024 a bucket is 12.6 M floats, well past the size where a
    ring all-reduce is link-bound rather than latency-bound, so layers are not merged further.

    On CPU tensors (gloo; tests/test_dp_gloo.py) the same calls run without streams."""

    def __init__(self, grads: torch.Tensor, group=None):
        self.grads = grads
        self.group = group
        self.works = []
        self.seen = []
        self.comm = torch.cuda.Stream(device=grads.device) if grads.is_cuda else None

    def on_bucket(self, i: int, offset: int, count: int):
        if offset < 0 or count <= 0 or offset + count > self.grads.numel():
            raise ValueError(f"bucket {i}: slice [{offset}, {offset + count}) outside the {self.grads.numel()}-float gradient buffer")
        piece = self.grads[offset:offset + count]
        self.seen.append((offset, count))
        if self.comm is None:
            self.works.append(torch.distributed.all_reduce(piece, group=self.group, async_op=True))
            return
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.grads.device))
        self.comm.wait_event(ready)
        with torch.cuda.stream(self.comm):
            self.works.append(torch.distributed.all_reduce(piece, group=self.group, async_op=True))

    def finish(self):
        """Wait for every bucket (on CUDA: the current stream waits, the host does not) and check the buckets covered the buffer."""
        for w in self.works:
            w.wait()
        if self.comm is not None:
            torch.cuda.current_stream(self.grads.device).wait_stream(self.comm)
        covered = sorted(self.seen)
        pos = 0
        for off, cnt in covered:
            if off != pos:
                raise RuntimeError(f"gradient buckets leave [{pos}, {off}) unreduced" if off > pos else f"gradient buckets overlap at {off}")
            pos = off + cnt
        if pos != self.grads.numel():
            raise RuntimeError(f"gradient buckets leave [{pos}, {self.grads.numel()}) unreduced")
        self.works, self.seen = [], []


class TrainStepGraph:
    """One optimiser step of ``_train_one_batch`` -- draw t and noise, q_sample, forward, loss, backward, clip, AdamW -- captured in a
    hipGraph (through ``torch.cuda.graph``: the library's launches go to the capture stream like every other caller's stream) and replayed
    with ONE host call per step.  Single-process training only (a gradient all-reduce is not captured).  The inputs are copied into fixed
    buffers before each replay; t and noise come from torch's graph-safe generator, so successive replays draw fresh values; the step
    count and lr are read from device memory by the optimiser kernel.  The backward's remaining weight-gradient launches run on the capture
    stream (``dq_plan_set_side_stream(plan, 0)``): a fork / join inside a graph was measured slower than the chain."""

    def __init__(self, dm, x_0, ms2_cond, ms1_cond, ms1_loss_weight=0.0, keep_side=False):
        self.dm, self.opt, self.net = dm, dm.optimizer, dm.model
        self.key = (tuple(x_0.shape), tuple(ms1_cond.shape), float(ms1_loss_weight or 0.0), float(dm.optimizer.grad_scale))
        self._ema_key = (dm.optimizer.ema_decay, dm.optimizer.ema_warmup)  # launch arguments of the captured optimiser step
        self.x0, self.c2, self.c1 = (torch.empty_like(v, dtype=torch.float32).copy_(v) for v in (x_0, ms2_cond, ms1_cond))
        self.w = float(ms1_loss_weight or 0.0)
        self.keep_side = bool(keep_side)  # keep the fork / join inside the captured step (measured slower than the single chain: off)
        N.check(N.lib().dq_plan_set_side_stream(self.net._plan, 1 if self.keep_side else 0), "dq_plan_set_side_stream")
        self.opt._dev_state()
        self.opt.sync_step_dev()
        # warm-up on a side stream (workspaces, occupancy queries, lazy stream creation: nothing may allocate during capture) -- on a
        # SNAPSHOT of the training state: parameters, moments, step count and the generator state are put back afterwards, so that
        # building the graph is not a training step
        snap = (self.net.flat_params.detach().clone(), self.opt._m.clone(), self.opt._v.clone(), self.opt._step, torch.cuda.get_rng_state(x_0.device),
                self.opt.ema_buffer().clone() if self.opt.ema_enabled else None)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                self._body(count=True)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        with torch.no_grad():
            self.net.flat_params.copy_(snap[0]); self.opt._m.copy_(snap[1]); self.opt._v.copy_(snap[2])
            if snap[5] is not None:
                self.opt.ema_buffer().copy_(snap[5])
        self.opt._step = snap[3]
        self.opt.sync_step_dev()
        torch.cuda.set_rng_state(snap[4], x_0.device)
        # the replay dereferences RAW device pointers: every buffer the captured launches touch is held here for the graph's lifetime (the
        # network's workspace cache may evict its entry when another training shape comes by -- this reference keeps the memory alive), and
        # the ones whose identity carries the training state are part of matches(): a `.to()` / storage-replacing load re-creates the flat
        # buffers, and a graph that still pointed at the old ones would train dead memory
        B, RT = int(x_0.shape[0]), int(x_0.shape[1])
        self._ws = self.net.workspace(B, RT, True)
        self._held = self._live_buffers() + (self._ws, self.opt._scratch, self.opt._gnorm, self.opt._lr_dev, self.opt._step_dev, dm.alpha_bars)
        self._ptrs = tuple(t.data_ptr() for t in self._live_buffers())
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = self._body(count=False)
        if tuple(t.data_ptr() for t in self._live_buffers()) != self._ptrs or self.net.workspace(B, RT, True) is not self._ws:
            raise RuntimeError("TrainStepGraph: a training buffer moved while the step was being captured")

    def _live_buffers(self):
        live = (self.net.flat_params, self.net.flat_grads(), self.opt._m, self.opt._v)
        return live + (self.opt.ema_buffer(),) if self.opt.ema_enabled else live  # (EMA switched on or off since the capture: no match)

    def _body(self, count):
        loss = self.dm.train_step_fused(self.x0, self.c2, self.c1, zero_grads=True, ms1_loss_weight=self.w)
        self.opt.step_dev(count=count)
        return loss

    def matches(self, x_0, ms1_cond, ms1_loss_weight, grad_scale):
        return (self.key == (tuple(x_0.shape), tuple(ms1_cond.shape), float(ms1_loss_weight or 0.0), float(grad_scale))
                and self._ema_key == (self.opt.ema_decay, self.opt.ema_warmup)
                and tuple(t.data_ptr() for t in self._live_buffers()) == self._ptrs)

    def step(self, x_0, ms2_cond, ms1_cond):
        self.x0.copy_(x_0); self.c2.copy_(ms2_cond)
        if self.dm.cond_dropout_enabled:  # conditioning dropout in place of the copy, outside the captured graph (the step itself is unchanged)
            self.dm._cond_drop_ms1(ms1_cond, out=self.c1)
        else:
            self.c1.copy_(ms1_cond)
        self.opt._dev_state()      # (a changed lr reaches its device copy here, outside the graph)
        self.opt._step += 1
        self.graph.replay()
        return self.loss.clone()   # a fresh tensor per step, as the eager path returns (the graph's own output is overwritten by the next replay)


# ----------------------------------------------------------------------------------------------------------------
# harness
# ----------------------------------------------------------------------------------------------------------------
class ModelInterface(object):
    def __init__(self, device: str = torch.device("cuda" if torch.cuda.is_available() else "cpu"), min_pred_value: float = 0.0, **kwargs):
        self.model: torch.nn.Module = None
        self.optimizer = None
        self.model_params: dict = {}
        self.min_pred_value = min_pred_value
        self.lr_scheduler_class = WarmupLR_Scheduler
        self.callback_handler = CallbackHandler()
        self.device = device
        self.ms1_loss_weight = None
        self.use_wandb = False
        self.last_grad_norm = None
        self._cond_drop = None  # set_cond_dropout

    def __repr__(self):
        return f"{self.__class__.__name__} with {self.model.__class__.__name__} model with {self.get_parameter_num()} parameters on {self.device}"

    # ---- public
    def build(self, model_class, **kwargs):
        self.model = model_class
        self._init_for_training()

    def get_parameter_num(self):
        return int(np.sum([p.numel() for p in self.model.parameters()]))

    def train_step(self, x_0, ms2_cond=None, ms1_cond=None, noise=None, ms1_loss_weight=0.0):
        raise NotImplementedError

    def sample(self, x_t, ms2_cond=None, ms1_cond=None, num_steps=1000, **kwargs):
        raise NotImplementedError

    def train(self, dataloader, batch_size, epochs, warmup_epochs: int = 5, learning_rate: float = 1e-4, use_wandb: bool = False,
              checkpoint_path: str = "best_model.ckpt", *, val_dataloader=None, val_every: int = 1, **kwargs):
        """Epoch loop (reference :453-559).  ``warmup_epochs > 0`` uses the warm-up/cosine schedule, else a constant lr.
        ``batch_size`` is accepted and unused, as in the reference (the dataloader carries it).  ``val_dataloader`` / ``val_every``: see
        ``train_with_warmup``."""
        if val_dataloader is not None:
            kwargs.update(val_dataloader=val_dataloader, val_every=val_every)
        if warmup_epochs > 0:
            self.train_with_warmup(dataloader, epochs, num_warmup_steps=int(warmup_epochs), learning_rate=learning_rate,
                                   use_wandb=use_wandb, checkpoint_path=checkpoint_path, **kwargs)
        else:
            self.train_with_warmup(dataloader, epochs, num_warmup_steps=0, learning_rate=learning_rate, use_wandb=use_wandb,
                                   checkpoint_path=checkpoint_path, constant_lr=True, **kwargs)

    def train_with_warmup(self, dataloader, num_epochs, num_warmup_steps=5, learning_rate=1e-4, use_wandb=True,
                          log_every_n_epochs=100, checkpoint_path="best_model.ckpt", *, constant_lr: bool = False, val_dataloader=None,
                          val_every: int = 1, **kwargs):
        """Reference :348-450, same positional order (dataloader, num_epochs, num_warmup_steps, learning_rate, use_wandb,
        log_every_n_epochs, checkpoint_path).  ``constant_lr`` (keyword-only, this build) is how ``train`` runs its
        ``warmup_epochs <= 0`` branch (reference :498-559) through the same loop.

        ``val_dataloader`` (keyword-only, this build; None: everything as it always was): after every ``val_every``-th epoch
        ``evaluate(val_dataloader)`` runs, its ``val_loss`` is printed and logged beside the epoch loss, the "best" checkpoint is chosen by
        it instead of the noisy training loss (``best_loss`` then holds a validation loss), and the checkpoints gain a ``val_loss``
        entry."""
        val_every = int(val_every)
        if val_dataloader is not None and val_every < 1:
            raise ValueError(f"val_every must be >= 1, got {val_every}")
        self.use_wandb_epoch = bool(use_wandb)
        wandb = _wandb() if use_wandb else None
        self._prepare_training(learning_rate)
        lr_scheduler = None if constant_lr else self._get_lr_schedule_with_warmup(num_warmup_steps, num_epochs)
        self.model.train()
        ckpt_dir = os.path.dirname(checkpoint_path) or "."
        latest = os.path.join(ckpt_dir, "dquartic_latest_checkpoint.ckpt")
        start_epoch, best_loss, lr_scheduler = self.load_checkpoint(lr_scheduler, latest, self.device)
        self._sync_replicas()  # data-parallel: every rank continues from rank 0's weights / moments (also after a resume)
        # ... and from rank 0's epoch counter, best loss, lr-schedule state and current lr: with the "latest" checkpoint visible to rank 0
        # only (node-local disks), the ranks would otherwise run epoch loops of different lengths and hang in the per-step all-reduce
        start_epoch, best_loss = self._sync_resume_state(start_epoch, best_loss, lr_scheduler)
        best_epoch = start_epoch
        val_loss = None  # the last held-out loss (val_dataloader)
        if val_dataloader is not None and not getattr(self, "_resumed_with_val_loss", True):
            # resumed from a checkpoint written without validation: its best_loss is a training loss, which a held-out loss is not compared with
            best_loss = float("inf")
        rank0 = _rank() == 0
        for epoch in range(start_epoch, num_epochs):
            if hasattr(getattr(dataloader, "sampler", None), "set_epoch"):
                dataloader.sampler.set_epoch(epoch)  # DistributedSampler: a different permutation every epoch
            if hasattr(dataloader.dataset, "reset_epoch"):
                dataloader.dataset.reset_epoch()
            batch_loss = self._train_one_epoch(epoch, dataloader)
            if lr_scheduler is not None:
                lr_scheduler.step(epoch, np.mean(batch_loss))
            avg = self._global_mean(float(np.mean(batch_loss)))  # DP: the mean over ranks (one float, logging only)
            lr_now = self.optimizer.param_groups[0]["lr"]
            # With a validation loader the epoch's score is the held-out loss (on every rank: evaluate() averages over the ranks, so the
            # "best" decision agrees); an epoch between two validations has no score and writes the "latest" checkpoint only.
            validated = val_dataloader is not None and (epoch + 1) % val_every == 0
            if validated:
                val_loss = self.evaluate(val_dataloader)["val_loss"]  # (hands the network back in training mode)
            score = avg if val_dataloader is None else (val_loss if validated else None)
            if wandb is not None and rank0:
                wandb.log({"epoch": epoch, "train/loss": avg, "learning_rate": lr_now, **({"val/loss": val_loss} if validated else {})})
            if rank0:
                print(f"[Training] Epoch={epoch + 1}, lr={lr_now}, loss={avg}" + (f", val_loss={val_loss}" if validated else ""))
                self.save_checkpoint(lr_scheduler, epoch, best_loss if score is None else score, latest, val_loss=val_loss)
            if score is not None and score < best_loss:
                best_loss, best_epoch = score, epoch + 1
                if rank0:
                    self.save_checkpoint(lr_scheduler, epoch, best_loss, checkpoint_path, val_loss=val_loss)
            if not self.callback_handler.epoch_callback(epoch=epoch, epoch_loss=avg):
                print(f"Training stopped at epoch {epoch}")
                break
        if rank0:
            print(f"Best model checkpoint saved at epoch {best_epoch} with loss: {best_loss:.6f}")

    # ---- data-parallel helpers (new work: the reference is single-process)
    def _sync_replicas(self, src: int = 0):
        """Make every rank's replica identical to rank ``src``'s: the flat parameter buffer and, when an optimiser exists, its
        AdamW moments and step count.  Each process builds its network from its own default-seeded RNG, and only gradients are
        exchanged per step, so without this the replicas would start (or resume) from different weights and never meet."""
        d = torch.distributed
        if not (d.is_available() and d.is_initialized()) or d.get_world_size() == 1:
            return
        if hasattr(self.model, "flat_params"):
            d.broadcast(self.model.flat_params, src=src)
            for b in self.model.buffers():
                d.broadcast(b, src=src)
            if isinstance(self.optimizer, FlatAdamW):
                self.optimizer._buffers()
                d.broadcast(self.optimizer._m, src=src)
                d.broadcast(self.optimizer._v, src=src)
                if self.optimizer.ema_enabled:
                    d.broadcast(self.optimizer.ema_buffer(), src=src)
                step = torch.tensor([float(self.optimizer._step)], device=self.optimizer._m.device)
                d.broadcast(step, src=src)
                self.optimizer._step = int(step.item())
        else:
            for t in list(self.model.parameters()) + list(self.model.buffers()):
                d.broadcast(t.data, src=src)

    def _sync_resume_state(self, start_epoch, best_loss, lr_scheduler, src: int = 0):
        """Rank ``src``'s (start_epoch, best_loss), LambdaLR state and per-group lr on every rank (no-op outside a process group)."""
        d = torch.distributed
        if not (d.is_available() and d.is_initialized()) or d.get_world_size() == 1:
            return start_epoch, best_loss
        mine = d.get_rank() == src
        box = [{"start_epoch": start_epoch, "best_loss": best_loss,
                "scheduler": lr_scheduler.lambda_lr.state_dict() if lr_scheduler is not None else None,
                "lrs": [g["lr"] for g in self.optimizer.param_groups] if self.optimizer is not None else None} if mine else None]
        dev = None
        if d.get_backend() == "nccl":  # (object collectives stage through the current device with RCCL)
            dev = self.model.flat_params.device if hasattr(self.model, "flat_params") else next(self.model.parameters()).device
        d.broadcast_object_list(box, src=src, device=dev)
        st = box[0]
        if not mine:
            if lr_scheduler is not None and st["scheduler"] is not None:
                lr_scheduler.lambda_lr.load_state_dict(st["scheduler"])
            if self.optimizer is not None and st["lrs"] is not None:
                for g, lr in zip(self.optimizer.param_groups, st["lrs"]):
                    g["lr"] = lr
        return st["start_epoch"], st["best_loss"]

    def _global_mean(self, value: float) -> float:
        """Mean over the ranks of a per-rank scalar (the epoch's mean loss): identical on every rank afterwards, so the
        "best" decision, the callback and the log line agree."""
        d = torch.distributed
        if not (d.is_available() and d.is_initialized()) or d.get_world_size() == 1:
            return value
        dev = self.model.flat_params.device if hasattr(self.model, "flat_params") else next(self.model.parameters()).device
        t = torch.tensor([value], dtype=torch.float64, device=dev)
        d.all_reduce(t)
        return float(t.item()) / d.get_world_size()

    def load_checkpoint(self, scheduler, checkpoint_path, device):
        if os.path.exists(checkpoint_path):
            print(f"Loading checkpoint from {checkpoint_path}...")
            ck = torch.load(checkpoint_path, map_location=device, weights_only=False)
            self.model.load_state_dict(ck["model_state_dict"])
            if self.optimizer is not None and ck.get("optimizer_state_dict") is not None:
                self.optimizer.load_state_dict(ck["optimizer_state_dict"])
            if self.ema_enabled:  # the file's average, or -- a file written without one -- a fresh average of the loaded weights
                if ck.get("ema_state_dict") is not None:
                    self.optimizer.load_ema_state_dict(ck["ema_state_dict"])
                else:
                    self.optimizer.reset_ema()
            if scheduler is not None and ck.get("scheduler_state_dict") is not None:
                scheduler.lambda_lr.load_state_dict(ck["scheduler_state_dict"])
            epoch, best_loss = ck["epoch"], ck["best_loss"]
            self._resumed_with_val_loss = "val_loss" in ck  # (train with a validation loader: is best_loss a held-out loss?)
            print(f"Resumed from ({checkpoint_path}) epoch {epoch}, best loss {best_loss:.6f}")
        else:
            print(f"No checkpoint ({checkpoint_path}) found. Starting from scratch.")
            epoch, best_loss = 0, float("inf")
            self._resumed_with_val_loss = True
        return epoch, best_loss, scheduler

    def save_checkpoint(self, scheduler, epoch, best_loss, checkpoint_path, val_loss=None):
        ck = {"epoch": epoch, "model_state_dict": self.model.state_dict(), "optimizer_state_dict": self.optimizer.state_dict(),
              "scheduler_state_dict": (scheduler.lambda_lr.state_dict() if scheduler is not None else None), "best_loss": best_loss}
        if self.ema_enabled:  # (only then: without EMA the file has the reference's keys and nothing else)
            ck.update(ema_state_dict=self.optimizer.ema_state_dict(), ema_decay=self.optimizer.ema_decay, ema_warmup=self.optimizer.ema_warmup)
        if val_loss is not None:  # (only when training validates: the held-out loss of evaluate() at this epoch)
            ck["val_loss"] = val_loss
        torch.save(ck, checkpoint_path)

    # ---- exponential moving average of the weights (new work: the reference has none)
    @property
    def ema_enabled(self) -> bool:
        return isinstance(self.optimizer, FlatAdamW) and self.optimizer.ema_enabled

    def enable_ema(self, decay: float = 0.999, warmup: bool = True):
        """Keep an exponential moving average of the weights, updated inside the fused optimiser step (``FlatAdamW``).  Valid once the
        optimiser exists (``_set_optimizer`` / ``_set_lr``); ``ema_scope()`` / ``predict`` then evaluate the averaged weights."""
        if not isinstance(self.optimizer, FlatAdamW):
            raise RuntimeError("enable_ema needs the FlatAdamW optimiser of a native network (call it after _set_optimizer / _set_lr); "
                               f"the optimiser is {type(self.optimizer).__name__}")
        self.optimizer.enable_ema(decay, warmup)

    def disable_ema(self):
        if isinstance(self.optimizer, FlatAdamW):
            self.optimizer.disable_ema()

    # ---- conditioning dropout for classifier-free guidance (new work: the reference has none)
    @property
    def cond_dropout_enabled(self) -> bool:
        return getattr(self, "_cond_drop", None) is not None

    def set_cond_dropout(self, p, seed=0, null_ms1=0.0):
        """Train with the MS1 condition of a window replaced as a whole by the constant ``null_ms1`` (a raw value, normalised like real MS1)
        with probability ``p``: what ``sample(..., guidance_scale=w, null_ms1=...)`` needs the network to have seen.  ``0 <= p < 1``;
        ``p = 0`` turns it off again (the default).  UNet1d only.

        ``_train_one_batch`` runs ``dq_ms1_cond_drop`` on the batch's MS1 in front of the step (under ``enable_train_graph`` in place of
        the copy into the captured step's input, outside the graph).  The decision of window b of a step is a pure function of
        (``seed`` + the data-parallel rank, b, the optimiser's step count before the step), so a run is reproducible; the validation
        loss stays conditional and nothing is written into checkpoints."""
        from .unet1d import UNet1d

        try:
            p = float(p)
        except (TypeError, ValueError):
            raise ValueError(f"cond_drop_prob must satisfy 0 <= p < 1, got {p!r}") from None
        if not 0.0 <= p < 1.0:  # (NaN fails both comparisons)
            raise ValueError(f"cond_drop_prob must satisfy 0 <= p < 1, got {p!r}")
        if p == 0.0:
            self._cond_drop = None
            return
        if not isinstance(self.model, UNet1d):
            raise NotImplementedError("set_cond_dropout: conditioning dropout is built for UNet1d (the CustomTransformer's guided sampler is "
                                      "the follow-up)")
        self._cond_drop = {"p": p, "seed": int(seed), "null_ms1": float(null_ms1), "seed_dev": None}

    def _cond_drop_ms1(self, ms1_cond, out=None):
        """``dq_ms1_cond_drop`` of the batch's MS1 at draw = the optimiser's step count, ids = batch positions, seed + rank; ``out``: where
        the result goes (a contiguous fp32 tensor of ``ms1_cond``'s shape; None: a new one)."""
        cd = self._cond_drop
        if not ms1_cond.is_cuda:
            raise RuntimeError("conditioning dropout runs in the native kernel: the MS1 condition must be a device tensor")
        src = ms1_cond.detach().to(torch.float32).contiguous()
        if out is not None and not (out.is_contiguous() and out.dtype == torch.float32 and out.shape == src.shape):
            return out.copy_(self._cond_drop_ms1(src))  # (a buffer the kernel cannot write in place: through a temporary)
        if out is None:
            out = torch.empty_like(src)
        if cd["seed_dev"] is None or cd["seed_dev"].device != src.device:
            cd["seed_dev"] = self._seed_tensor(cd["seed"] + _rank(), src.device)
        draw = int(getattr(self.optimizer, "_step", 0))
        N.check(N.lib().dq_ms1_cond_drop(N.ptr(src), N.ptr(out), None, N.ptr(cd["seed_dev"]), draw, cd["p"], cd["null_ms1"], int(src.shape[0]),
                                         int(src[0].numel()), N.stream_ptr()), "dq_ms1_cond_drop")
        return out

    def _flat_net(self):
        """The module that owns the flat buffers and makes the native calls (the transformer behind its adapter)."""
        return getattr(self.model, "transformer", self.model)

    @contextlib.contextmanager
    def ema_scope(self):
        """Inside the scope every native call of the network reads the EMA buffer in place of ``flat_params`` -- by pointer, nothing is
        copied: ``UNet1d.forward`` under ``no_grad``, ``sample()`` (``dq_ddim_sample``, eager and captured), the ``CustomTransformer``'s
        forward behind its adapter.  A forward that would record autograd history and a train step raise inside it (the average is not
        trained).  The training weights are never written, so on exit they are what they were.  The plan keeps ONE captured sampling
        graph, keyed by the parameter pointer among other things: alternating sampling inside and outside the scope recaptures it each
        time; sample from one side in a row."""
        if not self.ema_enabled:
            raise RuntimeError("ema_scope: EMA is not enabled (enable_ema)")
        net = self._flat_net()
        net.flat_params  # (a pending .to() / load re-creates the flat buffer here, outside the scope)
        prev = net._param_override
        net._param_override = self.optimizer.ema_buffer()
        try:
            yield self
        finally:
            net._param_override = prev

    def _ema_or_null_scope(self, use_ema):
        use = self.ema_enabled if use_ema is None else bool(use_ema)
        return self.ema_scope() if use else contextlib.nullcontext()

    def predict(self, dataloader, mixture_weights=(0.5, 0.5), num_steps=1000, use_ema=None, eta=0.0, seed=None, n_draws=1,
                sampler="reference", clip_x0=None, *, guidance_rescale=0.0, threshold_quantile=None, threshold_max=None,
                group_size=None, consistency=None, consistency_strength=1.0, guidance_scale=None, null_ms1=0.0):
        """Reference :630-668: one dict per batch with the first item's prediction (``_predict_one_batch`` returns item 0).
        ``use_ema``: sample from the averaged weights; None (default) = when EMA is enabled.

        Stochastic sampling (the defaults are the call as it always was, x_T from ``torch.randn_like``): with
        ``eta > 0``, a ``seed`` or ``n_draws > 1``, x_T and the per-step noise come from the sampler's counter-based generator under
        ``seed`` (None: drawn once from torch's generator), and the window id of item b of batch k is its running index in the dataloader
        -- a window's prediction does not depend on the batch size.  Draw j (0-based) samples under ``seed + j``, so it is what
        ``n_draws=1, seed=seed + j`` returns.  ``n_draws > 1`` adds ``"pred_mean"`` and ``"pred_std"`` (per element, over the draws,
        population form) to each dict; ``"pred"`` stays draw 0.  With ``n_draws == 1`` those two keys are absent.

        ``sampler`` / ``clip_x0``: passed to ``sample``; with the defaults nothing else changes.  ``guidance_scale``
        / ``null_ms1`` (keyword-only): classifier-free guidance, passed to ``sample`` too; so are
        ``guidance_rescale`` / ``threshold_quantile`` / ``threshold_max`` and ``group_size`` / ``consistency`` /
        ``consistency_strength`` (every batch of the loader is then read as member-major groups).

        Batches that carry their weights (``ResidentMixLoader``) add ``"weights"``, the batch's ``(B, K)`` array."""
        self.model.eval()
        sampler_kw = _sampler_kwargs(sampler, clip_x0, guidance_scale, null_ms1, guidance_rescale, threshold_quantile, threshold_max, group_size,
                                     consistency, consistency_strength)
        n_draws = int(n_draws)
        if n_draws < 1:
            raise ValueError(f"n_draws must be >= 1, got {n_draws}")
        stochastic = float(eta) > 0.0 or seed is not None or n_draws > 1
        if stochastic and seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())
        preds = []
        first = 0
        for batch in dataloader:
            x_0, ms2_cond, ms1_cond, weights = self._batch_inputs(batch, mixture_weights)
            d = {"ms2_1": x_0.cpu().numpy(), "ms1_1": ms1_cond.cpu().numpy(), "mixture": ms2_cond.cpu().numpy()}
            if weights is not None:
                d["weights"] = weights.cpu().numpy()
            if not stochastic:
                d["pred"], _ = self._predict_one_batch(x_0, ms2_cond=ms2_cond, ms1_cond=ms1_cond, num_steps=num_steps, use_ema=use_ema,
                                                       **sampler_kw)
            else:
                ids = torch.arange(first, first + x_0.shape[0], dtype=torch.int64)
                out = self._predict_one_batch(x_0, ms2_cond=ms2_cond, ms1_cond=ms1_cond, num_steps=num_steps, use_ema=use_ema, eta=eta,
                                              seed=seed, n_draws=n_draws, window_ids=ids, **sampler_kw)
                d["pred"] = out[0]
                if n_draws > 1:
                    d["pred_mean"], d["pred_std"] = out[2], out[3]
            first += x_0.shape[0]
            preds.append(d)
        return np.array(preds, dtype=object)

    def evaluate(self, dataloader, mixture_weights=(0.5, 0.5), n_t=4, seed=0, num_steps=None, eta=0.0, use_ema=None, max_batches=None,
                 sampler="reference", clip_x0=None, *, guidance_rescale=0.0, threshold_quantile=None, threshold_max=None,
                 guidance_scale=None, null_ms1=0.0):
        """Held-out evaluation (new work: the reference has none).  Returns a dict.

        Loss: every window of the loader is evaluated ``n_t`` times by ``eval_steps`` -- repeat k at the timestep
        ``evaluation.stratified_timesteps`` gives it (one in each of the ``n_t`` equal buckets of [0, T), no RNG) with the noise of
        ``dq_randn(seed, window id, draw = k)``, the window id being the window's running index in the loader as in ``predict``.  Given
        the loader's windows the numbers are therefore reproducible and, for UNet1d, do not depend on the batch size; for the
        CustomTransformer (all repeats of a batch in one stacked forward) they are reproducible bit for bit at a given
        batch size and agree across batch sizes to fp32 rounding only: its GEMM plans follow the row count.  ``val_loss`` is the mean of
        ``loss_weight[t] * MSE`` over all (window, repeat) pairs, ``val_loss_by_t`` = {"edges": the n_t + 1 bucket edges, "mse": per
        bucket the mean of the UNWEIGHTED per-window MSE}, ``n_windows`` the number of windows seen.  The MSE part of the training loss
        only (no MS1 term).

        ``num_steps`` (None: loss only): every window is also sampled, ``sample(None, ..., num_steps, eta=eta, seed=seed,
        window_ids=ids)``, and ``dq_recon_metrics(sample, x_0)`` gives nine numbers per window (``_native.METRIC_NAMES``): the dict gains
        their means over the windows (``scan_sa`` / ``xic_r`` weighted by ``scan_count`` / ``xic_count``) under those names and the
        ``(n_windows, 9)`` float32 array as ``per_window``.  ``sampler`` / ``clip_x0`` go to that ``sample`` call
        and appear in the dict only when they are not the defaults; so do ``guidance_scale`` / ``null_ms1`` (keyword-only; DESIGN.md
        section 32: the scale can be tuned against these metrics) and ``guidance_rescale`` / ``threshold_quantile`` / ``threshold_max``
        (DESIGN.md section 38).  The loss part is always the conditional one.

        ``use_ema`` as in ``predict``; ``max_batches``: stop after that many batches.  Under ``torch.distributed`` each rank evaluates
        its own loader and the scalars are averaged over the ranks (``_global_mean``); ``per_window`` and ``n_windows`` stay the rank's.

        Batches that carry their weights (``ResidentMixLoader``; ``mixture_weights`` does not apply to them) add
        ``target_weight``, the float32 ``(n_windows,)`` array of every window's w_0, and ``val_loss_by_weight`` = {"edges": [0, 1/16, 1/8,
        1/4, 1/2, 1], "mse": per bucket the mean of the unweighted per-window MSE (over its ``n_t`` repeats), "n": the bucket's windows},
        with ``num_steps`` also "sa", the bucket's mean spectral angle (``evaluation.by_target_weight``; an empty bucket reports 0 and
        None).  Both stay the rank's.  Without such batches the dict has exactly the keys above."""
        from . import evaluation as E

        n_t = int(n_t)
        if n_t < 1:
            raise ValueError(f"n_t must be >= 1, got {n_t}")
        was_training = self.model.training
        self.model.eval()
        sampler_kw = _sampler_kwargs(sampler, clip_x0, guidance_scale, null_ms1, guidance_rescale, threshold_quantile, threshold_max)
        T = int(self.num_timesteps)
        lw_host = self.loss_weight.detach().to("cpu", torch.float32).numpy().astype(np.float64)
        mse, ts, rows, target_w = [[] for _ in range(n_t)], [[] for _ in range(n_t)], [], []
        first = 0
        seed_dev = None
        try:
            with torch.no_grad(), self._ema_or_null_scope(use_ema):
                for batch_idx, batch in enumerate(dataloader):
                    if max_batches is not None and batch_idx >= int(max_batches):
                        break
                    x_0, ms2_cond, ms1_cond, weights = self._batch_inputs(batch, mixture_weights)
                    if weights is not None:
                        target_w.append(weights[:, 0])
                    ids = np.arange(first, first + x_0.shape[0], dtype=np.int64)
                    ids_dev = torch.from_numpy(ids).to(x_0.device)
                    if seed_dev is None:
                        seed_dev = self._seed_tensor(int(seed), x_0.device)
                    t = np.stack([E.stratified_timesteps(ids, k, n_t, T) for k in range(n_t)])  # (n_t, B): repeat k draws at index k
                    _, per_window = self.eval_steps(x_0, ms2_cond, ms1_cond, torch.from_numpy(t).to(x_0.device), seed_dev, ids_dev)
                    for k in range(n_t):
                        mse[k].append(per_window[k])
                        ts[k].append(t[k])
                    if num_steps is not None:
                        sample, _ = self.sample(None, ms2_cond=ms2_cond, ms1_cond=ms1_cond, num_steps=int(num_steps), eta=eta, seed=int(seed),
                                                window_ids=ids_dev, shape=tuple(x_0.shape), **sampler_kw)
                        rows.append(E.recon_metrics(sample, x_0))
                    first += x_0.shape[0]
        finally:
            self.model.train(was_training)
        if first == 0:
            raise ValueError("evaluate: the dataloader yielded no batch")
        # one host copy per repeat after the loop; the means are float64 sums over the windows in loader order (no batch in them)
        mse = np.stack([torch.cat(m).cpu().numpy().astype(np.float64) for m in mse])  # (n_t, n_windows)
        weights = np.stack([lw_host[np.concatenate(t)] for t in ts])
        out = {"val_loss": self._global_mean(float((weights * mse).mean())),
               "val_loss_by_t": {"edges": E.bucket_edges(n_t, T), "mse": [self._global_mean(float(m.mean())) for m in mse]},
               "n_windows": int(first), "n_t": n_t, "seed": int(seed)}
        if num_steps is not None:
            per_window = torch.cat(rows).cpu().numpy()
            out.update({k: self._global_mean(v) for k, v in E.aggregate_metrics(per_window).items()})
            out.update(num_steps=int(num_steps), eta=float(eta), per_window=per_window)
            out.update(_reported_options(sampler_kw))
        if target_w:  # batches that carry their weights (ResidentMixLoader): the loss by the target's share of its mixture
            tw = torch.cat(target_w).cpu().numpy().astype(np.float32)
            if len(tw) != first:
                raise ValueError("evaluate: some batches of the dataloader carry mixture weights and some do not")
            out["target_weight"] = tw
            out["val_loss_by_weight"] = E.by_target_weight(tw, mse.mean(axis=0), None if num_steps is None else out["per_window"])
        return out

    def evaluate_joint(self, loader, num_steps, consistency="bound", consistency_strength=1.0, independent=True, eta=0.0, seed=0,
                       sampler="reference", clip_x0=None, use_ema=None, max_batches=None):
        """Held-out evaluation of joint sampling: does sampling the P precursors of a mixture as one group under
        ``consistency`` beat P independent calls?  ``loader`` yields ``GroupBatch``es (``ResidentGroupLoader``: member-major, group size
        P, ``n_groups`` groups per pass).  Per batch of G groups there is one ``sample(None, ..., group_size=P, consistency=consistency,
        consistency_strength=consistency_strength, window_ids=ids)`` call and, with ``independent``, a second one with
        ``consistency=None`` on the same batch and ids -- bit for bit P plain calls.  Member p of running group k samples under the id
        ``p * n_groups + k`` (``joint_window_ids`` with ``n_windows = loader.n_groups``), so member 0 has the id ``evaluate`` gives the
        same window of a ``ResidentMixLoader`` with the same arguments.  Each result goes through ``dq_recon_metrics`` against the
        members' targets and ``dq_group_metrics`` against the targets and the mixture.

        Returns a dict with ``"joint"`` and, with ``independent``, ``"independent"``, each holding the nine window metrics over all members
        (``aggregate_metrics``), the means of ``excess`` and ``unexplained``, ``id_acc``, ``leak`` (absent for P = 1) and ``sa_by_weight``
        (``evaluation.aggregate_joint``), and the arrays ``per_window`` ``(P * n, 9)``, ``cross`` ``(n, P, P)`` and ``group`` ``(n, 3)`` over
        the n groups seen; ``per_window`` and the dict's ``member_weight`` ``(P * n,)`` are member-major over ALL groups (member p of group k
        in row ``p * n + k``), so nothing in the result depends on the batch size.  Also ``n_groups`` (= n), ``group_size``, ``num_steps``,
        ``eta``, ``seed``, ``consistency``, ``consistency_strength`` and, where they are not the defaults, ``sampler`` / ``clip_x0``.

        UNet1d on the device only; no loss part (``evaluate`` has the loss).  ``use_ema`` / ``max_batches`` as in ``evaluate``."""
        from . import evaluation as E
        from .unet1d import UNet1d

        if not isinstance(self.model, UNet1d):
            raise NotImplementedError("evaluate_joint: groups are built for UNet1d (dq_ddim_sample); other networks are not implemented")
        if consistency is None:
            raise ValueError("evaluate_joint: consistency must be 'bound' or 'sum' (independent=True adds the calls without it)")
        n_total = getattr(loader, "n_groups", None)
        if n_total is None:
            raise ValueError("evaluate_joint: the loader must say how many groups a pass holds (ResidentGroupLoader.n_groups)")
        sampler_kw = _sampler_kwargs(sampler, clip_x0)
        legs = {"joint": dict(consistency=consistency, consistency_strength=float(consistency_strength))}
        if independent:
            legs["independent"] = dict(consistency=None)
        rows = {k: ([], [], []) for k in legs}
        member_w, first, P = [], 0, None
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad(), self._ema_or_null_scope(use_ema):
                for batch_idx, batch in enumerate(loader):
                    if max_batches is not None and batch_idx >= int(max_batches):
                        break
                    if not hasattr(batch, "group_size") or (P is not None and batch.group_size != P):
                        raise ValueError("evaluate_joint: every batch must be a GroupBatch of one group size")
                    P = batch.group_size
                    x_0, ms2_cond, ms1_cond = batch[0], batch.ms2_cond, batch[1]
                    if not x_0.is_cuda:
                        raise NotImplementedError("evaluate_joint runs in the native library only (device tensors)")
                    G = x_0.shape[0] // P
                    ids = torch.from_numpy(self.joint_window_ids(0, n_total, P, first, G)).to(x_0.device)
                    for name, kw in legs.items():
                        sample, _ = self.sample(None, ms2_cond=ms2_cond, ms1_cond=ms1_cond, num_steps=int(num_steps), eta=eta, seed=int(seed),
                                                window_ids=ids, shape=tuple(x_0.shape), group_size=P, **kw, **sampler_kw)
                        cross, group = E.group_metrics(sample, x_0, ms2_cond, P)
                        rows[name][0].append(E.recon_metrics(sample, x_0).view(P, G, -1))
                        rows[name][1].append(cross)
                        rows[name][2].append(group)
                    member_w.append(batch.member_weights().view(P, G))
                    first += G
        finally:
            self.model.train(was_training)
        if first == 0:
            raise ValueError("evaluate_joint: the loader yielded no batch")
        # one host copy per array after the loop; member-major over all groups, float64 means in that order (no batch in them)
        mw = torch.cat(member_w, dim=1).reshape(-1).cpu().numpy().astype(np.float32)
        out = {"n_groups": int(first), "group_size": int(P), "num_steps": int(num_steps), "eta": float(eta), "seed": int(seed),
               "consistency": str(consistency), "consistency_strength": float(consistency_strength), "member_weight": mw}
        out.update(_reported_options(sampler_kw))
        for name, (pw, cross, group) in rows.items():
            pw = torch.cat(pw, dim=1).reshape(P * first, -1).cpu().numpy()
            cross, group = torch.cat(cross).cpu().numpy(), torch.cat(group).cpu().numpy()
            out[name] = {**E.aggregate_joint(pw, cross, group, mw), "per_window": pw, "cross": cross, "group": group}
        return out

    _RUN_SAMPLE_OPTIONS = ("num_steps", "eta", "seed", "sampler", "clip_x0", "guidance_scale", "null_ms1", "guidance_rescale",
                           "threshold_quantile", "threshold_max", "use_ema")

    def _run_inputs(self, who, ms2_run, ms1_run, members, window, step, batch_size, taper, sample_options):
        """What ``deconvolve_run`` and ``deconvolve_run_joint`` (``members``: ``ms1_run`` carries a leading axis, one trace per member) check
        and stage alike, refusing under ``who``: the option names, the shapes, the MS1 channels against the network's, ``window``, the
        tiling, ``batch_size``, the taper, device tensors, a seed (drawn once when None).  Returns ``(ms2_run, ms1_run`` -- contiguous
        fp32, the MS1 with its channel axis -- ``RT_total, MZ, M1, window, step, batch_size, starts, taper (device), the sample options
        without use_ema, use_ema)``."""
        from ..utils.run_tiles import run_window_starts, taper_table

        lead = 1 if members else 0
        ms1_name = "ms1_runs" if members else "ms1_run"
        ms1_shapes = "(P, RT_total) or (P, RT_total, M1)" if members else "(RT_total,) or (RT_total, M1)"
        unknown = sorted(set(sample_options) - set(self._RUN_SAMPLE_OPTIONS))
        if unknown:
            raise TypeError(f"{who}: unknown option(s) {unknown} (sample options: {list(self._RUN_SAMPLE_OPTIONS)})")
        if not (torch.is_tensor(ms2_run) and torch.is_tensor(ms1_run)):
            raise TypeError(f"{who}: ms2_run and {ms1_name} must be torch tensors")
        if ms2_run.dim() != 2:
            raise ValueError(f"{who}: ms2_run must be (RT_total, MZ), got {tuple(ms2_run.shape)}")
        RT_total, MZ = (int(v) for v in ms2_run.shape)
        if ms1_run.dim() == lead + 1:
            ms1_run = ms1_run[..., None]
        if ms1_run.dim() != lead + 2 or ms1_run.shape[lead] != RT_total:
            raise ValueError(f"{who}: {ms1_name} must be {ms1_shapes} with RT_total = {RT_total}, got "
                             f"{tuple(ms1_run.shape)}")
        M1 = int(ms1_run.shape[-1])
        net_m1 = int(getattr(self._flat_net(), "attn_cond_channels", 1))
        if M1 != net_m1:
            raise ValueError(f"{who}: {ms1_name} has {M1} channel(s), the network was built with attn_cond_channels={net_m1}")
        if window is None:
            raise ValueError(f"{who}: window (the scans per window, the length the network was trained on) must be given")
        W, step, batch_size = int(window), int(step), int(batch_size)
        starts = run_window_starts(RT_total, W, step)
        if batch_size < 1:
            raise ValueError(f"{who}: batch_size must be >= 1, got {batch_size}")
        taper_host = taper_table(taper, W)
        opts = dict(sample_options)
        use_ema = opts.pop("use_ema", None)
        if not (ms2_run.is_cuda and ms1_run.is_cuda):
            raise NotImplementedError(f"{who} runs in the native library only (device tensors)")
        if opts.get("seed") is None:
            opts["seed"] = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())
        dev = ms2_run.device
        run2, run1 = ms2_run.detach().to(torch.float32).contiguous(), ms1_run.detach().to(device=dev, dtype=torch.float32).contiguous()
        return run2, run1, RT_total, MZ, M1, W, step, batch_size, starts, torch.from_numpy(taper_host).to(dev), opts, use_ema

    def deconvolve_run(self, ms2_run, ms1_run, window=None, step=5, taper="hann", batch_size=32, id_offset=0, **sample_options):
        """Deconvolve one observed isolation-window chromatogram (new work: the reference has no such entry).

        ``ms2_run`` ``(RT_total, MZ)`` and ``ms1_run`` ``(RT_total,)`` or ``(RT_total, M1)`` (M1 = the network's ``attn_cond_channels``)
        are device tensors in raw intensity units.  The run is cut into ``n`` windows of ``window`` scans every ``step`` scans
        (``utils.run_tiles.run_window_starts``: the last window is pulled back to end on the last scan), as the training data was cut
        from such runs; ``window`` must be given, nothing is guessed.  For each batch of ``batch_size`` consecutive windows
        ``dq_run_windows`` min-max normalises every window by its own statistics (a constant window, an empty stretch of the run, gives
        zeros), ``sample(None, ms2_win, ms1_win, window_ids=ids)`` predicts them with x_T and any step noise drawn from the sampler's
        counter-based generator -- window ``i`` under the id ``id_offset + i`` -- and ``dq_run_stitch`` folds the predictions, each
        brought back to intensity units by its window's ``hi - lo``, into a weighted running mean and variance per scan.  The update is
        sequential in window order, so the result does not depend on ``batch_size`` as long as the sampler's window-alone property
        holds (it is tested at small batches).

        ``taper``: the weight of a window's scan k in the blend -- ``"hann"`` (sin^2(pi (k + 1) / (W + 1)), strictly positive),
        ``"uniform"``, or ``window`` positive numbers.  ``sample_options``: ``num_steps``, ``eta``, ``seed``, ``sampler``, ``clip_x0``,
        ``guidance_scale``, ``null_ms1``, ``guidance_rescale``, ``threshold_quantile``, ``threshold_max`` go to ``sample`` as they are;
        ``use_ema`` as in ``predict``.  ``seed=None``: drawn once from
        torch's generator (x_T needs one), and kept in ``last_seed``.

        Returns a dict: ``"pred"`` ``(RT_total, MZ)``, the deconvolved chromatogram in intensity units ABOVE each window's floor -- the
        blend of ``p (hi - lo)``, not of ``lo + p (hi - lo)``: with ``scale_target`` mixtures the prediction is the
        target's contribution to the mixture, and the share of the window's ``lo`` that belongs to it is not identifiable;
        ``"overlap_var"`` ``(RT_total, MZ)``, the weighted variance among the windows that cover a scan (their disagreement; 0 where one
        window covers it); ``"coverage"`` ``(RT_total,)``, the sum of the taper weights on a scan; ``"scales"`` ``(n, 4)`` = (MS2 lo, MS2
        hi, MS1 lo, MS1 hi) of every window; ``"starts"`` (int64 array) and ``"n_windows"``.  The tensors stay on the device."""
        run2, run1, RT_total, MZ, M1, W, step, batch_size, starts, taper_dev, opts, use_ema = self._run_inputs(
            "deconvolve_run", ms2_run, ms1_run, False, window, step, batch_size, taper, sample_options)
        n, id_offset, dev = len(starts), int(id_offset), run2.device
        mean, m2 = torch.zeros(RT_total, MZ, device=dev), torch.zeros(RT_total, MZ, device=dev)
        wsum, scales = torch.zeros(RT_total, device=dev), torch.empty(n, 4, device=dev)
        nb = min(batch_size, n)
        scratch = torch.empty(max(1, N.lib().dq_run_windows_scratch_bytes(nb) // 4), dtype=torch.float32, device=dev)
        win2, win1 = torch.empty(nb, W, MZ, device=dev), torch.empty(nb, W, M1, device=dev)
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad(), self._ema_or_null_scope(use_ema):
                for i0 in range(0, n, batch_size):
                    B = min(batch_size, n - i0)
                    c2, c1, sc = win2[:B], win1[:B], scales[i0:i0 + B]
                    N.check(N.lib().dq_run_windows(N.ptr(run2), N.ptr(run1), RT_total, MZ, M1, W, step, i0, B, N.ptr(c2), N.ptr(c1), N.ptr(sc),
                                                   N.ptr(scratch), scratch.numel() * 4, N.stream_ptr()), "dq_run_windows")
                    ids = torch.arange(id_offset + i0, id_offset + i0 + B, dtype=torch.int64, device=dev)
                    pred, _ = self.sample(None, ms2_cond=c2, ms1_cond=c1, window_ids=ids, **opts)
                    pred = pred.detach().to(torch.float32).contiguous()
                    N.check(N.lib().dq_run_stitch(N.ptr(pred), N.ptr(sc), N.ptr(taper_dev), RT_total, MZ, W, step, i0, B, N.ptr(mean), N.ptr(m2),
                                                  N.ptr(wsum), N.stream_ptr()), "dq_run_stitch")
        finally:
            self.model.train(was_training)
        return {"pred": mean, "overlap_var": m2 / wsum[:, None], "coverage": wsum, "scales": scales, "starts": starts, "n_windows": n}

    @staticmethod
    def joint_window_ids(id_offset, n_windows, members, i0, count):
        """The window ids of one batch of ``deconvolve_run_joint``, member-major: member p, window i samples under ``id_offset + p *
        n_windows + i`` (member 0: the ids of ``deconvolve_run``), here for windows ``i0 .. i0 + count - 1`` of every member.  int64, host."""
        i = np.arange(int(i0), int(i0) + int(count), dtype=np.int64)
        return (int(id_offset) + np.arange(int(members), dtype=np.int64)[:, None] * int(n_windows) + i[None, :]).reshape(-1)

    def deconvolve_run_joint(self, ms2_run, ms1_runs, window=None, step=5, taper="hann", batch_size=32, id_offset=0, consistency="bound",
                             consistency_strength=1.0, **sample_options):
        """``deconvolve_run`` for the P precursors that co-elute in one isolation window, sampled as groups under mixture consistency
        (DESIGN.md section 40).  ``ms2_run`` ``(RT_total, MZ)`` is the one observed run, ``ms1_runs`` ``(P, RT_total)`` or ``(P, RT_total,
        M1)`` the P MS1 traces, 1 <= P <= 8.  Per batch of ``batch_size`` = G consecutive windows ``dq_run_windows`` runs once per member
        (the same MS2 windows and MS2 scales each time, the member's own MS1), the P batches are concatenated member-major and sampled in
        one call, ``sample(None, ..., group_size=P, consistency=consistency, consistency_strength=consistency_strength)`` -- member p,
        window i under the id ``id_offset + p * n_windows + i`` (``joint_window_ids``) -- and ``dq_run_stitch`` folds each member's
        contiguous slice into that member's running mean.  ``consistency``: ``"bound"`` (default: the members never explain more than
        the observed window, scan by scan and m/z by m/z), ``"sum"`` (they explain all of it) or None -- then every member's result is,
        bit for bit, what ``deconvolve_run(ms2_run, ms1_runs[p], id_offset=id_offset + p * n_windows)`` returns.  The other arguments and
        ``sample_options`` are ``deconvolve_run``'s, minus the options a call over groups refuses (``sample``).

        Returns ``deconvolve_run``'s dict with a leading P axis on ``"pred"``, ``"overlap_var"`` and ``"scales"`` (``(P, n, 4)``: the MS2
        columns are the same for every member); ``"coverage"``, ``"starts"`` and ``"n_windows"`` (the windows of ONE member) as there."""
        run2, runs1, RT_total, MZ, M1, W, step, batch_size, starts, taper_dev, opts, use_ema = self._run_inputs(
            "deconvolve_run_joint", ms2_run, ms1_runs, True, window, step, batch_size, taper, sample_options)
        P, n, dev = int(runs1.shape[0]), len(starts), run2.device
        if not 1 <= P <= N.GROUP_MAX:
            raise ValueError(f"deconvolve_run_joint: ms1_runs must hold 1 .. {N.GROUP_MAX} members, got {P}")
        mean, m2 = torch.zeros(P, RT_total, MZ, device=dev), torch.zeros(P, RT_total, MZ, device=dev)
        wsum, scales = torch.zeros(P, RT_total, device=dev), torch.empty(P, n, 4, device=dev)
        nb = min(batch_size, n)
        scratch = torch.empty(max(1, N.lib().dq_run_windows_scratch_bytes(nb) // 4), dtype=torch.float32, device=dev)
        win2, win1 = torch.empty(P * nb, W, MZ, device=dev), torch.empty(P * nb, W, M1, device=dev)
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad(), self._ema_or_null_scope(use_ema):
                for i0 in range(0, n, batch_size):
                    G = min(batch_size, n - i0)
                    c2, c1 = win2[:P * G], win1[:P * G]
                    for p in range(P):
                        N.check(N.lib().dq_run_windows(N.ptr(run2), N.ptr(runs1[p]), RT_total, MZ, M1, W, step, i0, G, N.ptr(c2[p * G:]),
                                                       N.ptr(c1[p * G:]), N.ptr(scales[p, i0:]), N.ptr(scratch), scratch.numel() * 4,
                                                       N.stream_ptr()), "dq_run_windows")
                    ids = torch.from_numpy(self.joint_window_ids(id_offset, n, P, i0, G)).to(dev)
                    pred, _ = self.sample(None, ms2_cond=c2, ms1_cond=c1, window_ids=ids, group_size=P, consistency=consistency,
                                          consistency_strength=consistency_strength, **opts)
                    pred = pred.detach().to(torch.float32).contiguous()
                    for p in range(P):
                        N.check(N.lib().dq_run_stitch(N.ptr(pred[p * G:]), N.ptr(scales[p, i0:]), N.ptr(taper_dev), RT_total, MZ, W, step, i0, G,
                                                      N.ptr(mean[p]), N.ptr(m2[p]), N.ptr(wsum[p]), N.stream_ptr()), "dq_run_stitch")
        finally:
            self.model.train(was_training)
        # (every member's taper sums are the same numbers: the tiling is the members' own)
        return {"pred": mean, "overlap_var": m2 / wsum[:, :, None], "coverage": wsum[0], "scales": scales, "starts": starts, "n_windows": n}

    # ---- internals
    def _init_for_training(self):
        self.loss_func = torch.nn.MSELoss()

    def _prepare_training(self, lr: float, **kwargs):
        self.model.train()
        self._set_lr(lr)
        self._sync_replicas()

    def _native_net(self) -> bool:
        from .building_blocks import DDIMTransformerAdapter
        from .unet1d import UNet1d

        return isinstance(self.model, (UNet1d, DDIMTransformerAdapter))

    def _set_optimizer(self, lr):
        """Reference :1011: AdamW(model.parameters(), lr) with torch defaults."""
        if self._native_net():
            self.optimizer = FlatAdamW(self.model, lr=lr)
        else:
            self.optimizer = torch.optim.AdamW(self.model.parameters(), lr=lr)

    def _set_lr(self, lr: float):
        if self.optimizer is None:
            self._set_optimizer(lr)
        else:
            for g in self.optimizer.param_groups:
                g["lr"] = lr

    def _get_lr_schedule_with_warmup(self, warmup_epoch, epoch):
        if warmup_epoch > epoch:
            warmup_epoch = epoch // 2
        return self.lr_scheduler_class(self.optimizer, num_warmup_steps=warmup_epoch, num_training_steps=epoch)

    def _batch_inputs(self, batch, mixture_weights=(0.5, 0.5)):
        """What the train, predict and evaluate loops take from a batch: ``(x_0, ms2_cond, ms1_cond, weights or None)``.

        A batch whose mixture is final (``MixBatch`` of ``ResidentMixLoader``, DESIGN.md section 34: K components, per-window weights, the
        target already scaled) is used as it is and ``mixture_weights`` does not apply; ``weights`` is its ``(B, K)`` tensor.  Anything
        else is ``(ms2_1, ms1_1, ms2_2, ms1_2)``: the simulated mixed spectrum of the target window and the other window (reference
        :1073-1075), which a resident loader (``ResidentPairLoader``) has already formed on the GPU, with the same bits, in the kernel that
        normalised the pair."""
        ms2_1, ms1_1, ms2_2, ms1_2 = batch
        x_0, ms1_cond = ms2_1.to(self.device), ms1_1.to(self.device)
        if getattr(batch, "mixture_final", False):
            return x_0, batch.ms2_cond, ms1_cond, batch.weights
        if getattr(batch, "ms2_cond", None) is not None and batch.mixture_weights == tuple(float(w) for w in mixture_weights):
            ms2_cond = batch.ms2_cond
        else:
            ms2_cond = (ms2_1 * mixture_weights[0]).to(self.device) + (ms2_2 * mixture_weights[1]).to(self.device)
        return x_0, ms2_cond, ms1_cond, None

    def _train_one_epoch(self, epoch, dataloader, mixture_weights=(0.5, 0.5)):
        self.model.train()
        batch_loss = []
        for batch_idx, batch in enumerate(dataloader):
            x_0, ms2_cond, ms1_cond, _ = self._batch_inputs(batch, mixture_weights)
            loss = self._train_one_batch(x_0, ms2_cond=ms2_cond, ms1_cond=ms1_cond, noise=None, ms1_loss_weight=self.ms1_loss_weight)
            batch_loss.append(loss)
            self.callback_handler.batch_callback(batch_idx, loss)
        return batch_loss

    def enable_train_graph(self, on: bool = True, keep_side: bool = False):
        """Run ``_train_one_batch`` as one captured hipGraph replay per step (``TrainStepGraph``): the reference trains at batch_size 1
        (dquartic_train_config.json:12), where a step is a chain of ~250 short launches and the host's launch rate is the limit.  Same
        kernels in the same order as the eager step (bit-identical given the same t / noise); single-process runs with drawn t / noise."""
        self.train_graph = bool(on)
        if bool(keep_side) != getattr(self, "_train_graph_side", False):
            self._train_graphs = {}
        self._train_graph_side = bool(keep_side)  # capture the side-stream fork / join as a second branch of the graph
        if not on and getattr(self, "_train_graphs", None):
            self._train_graphs = {}
            N.check(N.lib().dq_plan_set_side_stream(self.model._plan, 1), "dq_plan_set_side_stream")  # eager steps fork their weight gradients again

    def _train_one_batch(self, x_0, ms2_cond=None, ms1_cond=None, noise=None, ms1_loss_weight=0.0, t=None, sync=True):
        """Reference :1090-1123.  Returns the loss as a float (``sync=False``: a 0-dim device tensor, no host sync)."""
        fused = self._native_net() and isinstance(self.optimizer, FlatAdamW) and x_0.is_cuda and hasattr(self, "train_step_fused")
        if (fused and getattr(self, "train_graph", False) and noise is None and t is None and _world() == 1 and hasattr(self.model, "_plan")
                and ms2_cond is not None and ms1_cond is not None):
            # the whole step as one captured graph (enable_train_graph): drawn t / noise, single process.  A few graphs are kept, keyed by
            # shape: an epoch's short last batch does not throw the full-batch graph away (a capture costs two warm-up steps + state copies)
            graphs = self.__dict__.setdefault("_train_graphs", {})
            key = (tuple(x_0.shape), tuple(ms1_cond.shape), float(ms1_loss_weight or 0.0))
            tg = graphs.get(key)
            if tg is None or not tg.matches(x_0, ms1_cond, ms1_loss_weight, 1.0):
                for k in [k for k, g in graphs.items() if not g.matches(g.x0, g.c1, g.w, 1.0)]:
                    del graphs[k]   # (its flat buffers were re-created since: it can never match again)
                while len(graphs) >= 4:
                    del graphs[next(iter(graphs))]
                self.optimizer.grad_scale = 1.0
                tg = graphs[key] = TrainStepGraph(self, x_0, ms2_cond, ms1_cond, ms1_loss_weight, keep_side=getattr(self, "_train_graph_side", False))
            loss = tg.step(x_0, ms2_cond, ms1_cond)  # (conditioning dropout, when on: inside step(), in place of its copy of ms1_cond)
            self.last_grad_norm = self.optimizer.last_grad_norm
            return loss.item() if sync else loss
        if self.cond_dropout_enabled and ms1_cond is not None:
            ms1_cond = self._cond_drop_ms1(ms1_cond)  # (draw = the step count before this step)
        if fused:
            if noise is not None:
                noise = self.normalize(noise)  # reference quirk: a passed noise is mapped 2n-1 (model.py:346)
            loss = self.train_step_fused(x_0, ms2_cond, ms1_cond, t=t, noise=noise, zero_grads=True, ms1_loss_weight=ms1_loss_weight or 0.0)
            world = _world()
            if getattr(self, "_grads_reduced", False):
                self._grads_reduced = False  # the transformer's backward already all-reduced its buckets (BucketedAllReduce)
            elif torch.distributed.is_available() and torch.distributed.is_initialized():
                torch.distributed.all_reduce(self.model.flat_grads())  # one flat RCCL all-reduce (sum) of 515 KB
            self.optimizer.grad_scale = 1.0 / world
            self.optimizer.step()
            self.optimizer.sync_step_dev() if self.optimizer._step_dev is not None else None
            self.last_grad_norm = self.optimizer.last_grad_norm
            return loss.item() if sync else loss
        self.optimizer.zero_grad()
        loss = self.train_step(x_0, ms2_cond=ms2_cond, ms1_cond=ms1_cond, noise=noise, ms1_loss_weight=ms1_loss_weight or 0.0)
        if loss.dim() > 0:
            loss = loss.mean()
        loss.backward()
        if isinstance(self.optimizer, FlatAdamW):
            self.optimizer.grad_scale = 1.0
            self.optimizer.step()  # clip folded in
            self.last_grad_norm = self.optimizer.last_grad_norm
        else:
            self.last_grad_norm = torch.nn.utils.clip_grad_norm_(self.model.parameters(), max_norm=10.0)
            self.optimizer.step()
        return loss.item() if sync else loss.detach()

    def _predict_one_batch(self, x_0, ms2_cond=None, ms1_cond=None, num_steps=1000, use_ema=None, eta=0.0, seed=None, n_draws=1,
                           window_ids=None, sampler="reference", clip_x0=None, *, guidance_rescale=0.0, threshold_quantile=None,
                           threshold_max=None, group_size=None, consistency=None, consistency_strength=1.0, guidance_scale=None,
                           null_ms1=0.0):
        """Reference :1125-1150: eval + no_grad + sample(randn_like(x_0)); returns item 0 of the batch as numpy.  ``use_ema`` as in
        ``predict``.  With ``eta > 0``, a ``seed`` or ``n_draws > 1`` (see ``predict``): x_T and the step noise from the sampler's
        generator, draw j under ``seed + j``; ``n_draws > 1`` returns (sample, pred_noise, mean, std) of item 0, sample / pred_noise
        being draw 0's and mean / std taken per element over the draws' samples (torch reductions: this is not the hot path)."""
        self.model.eval()
        sampler_kw = _sampler_kwargs(sampler, clip_x0, guidance_scale, null_ms1, guidance_rescale, threshold_quantile, threshold_max, group_size,
                                     consistency, consistency_strength)
        if not (float(eta) > 0.0 or seed is not None or int(n_draws) > 1):
            with torch.no_grad(), self._ema_or_null_scope(use_ema):
                sample, pred_noise = self.sample(torch.randn_like(x_0), ms2_cond=ms2_cond, ms1_cond=ms1_cond, num_steps=num_steps,
                                                 **sampler_kw)
            return sample[0].cpu().detach().numpy(), pred_noise[0].cpu().detach().numpy()
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())
        draws = []
        with torch.no_grad(), self._ema_or_null_scope(use_ema):
            for j in range(int(n_draws)):
                draws.append(self.sample(None, ms2_cond=ms2_cond, ms1_cond=ms1_cond, num_steps=num_steps, eta=eta, seed=int(seed) + j,
                                         window_ids=window_ids, shape=tuple(x_0.shape), **sampler_kw))
        first = (draws[0][0][0].cpu().numpy(), draws[0][1][0].cpu().numpy())
        if int(n_draws) == 1:
            return first
        stack = torch.stack([s[0] for s, _ in draws])
        return first + (stack.mean(dim=0).cpu().numpy(), stack.std(dim=0, unbiased=False).cpu().numpy())

    def log_single_prediction(self, *args, **kwargs):
        raise NotImplementedError("wandb prediction tables / pyopenms_viz plots are outside the hot path (SURVEY section 2)")

    plot_single_prediction = log_single_prediction


def _sampler_kwargs(sampler, clip_x0, guidance_scale=None, null_ms1=0.0, guidance_rescale=0.0, threshold_quantile=None, threshold_max=None,
                    group_size=None, consistency=None, consistency_strength=1.0):
    """The step-consistent-sampler, guidance, per-window and group options as keyword arguments of ``sample`` -- none at the defaults, so that
    a subclass whose ``sample`` predates them is still called as it always was (the rule is ``SampleOptions.non_default``, with
    ``JointSampleOptions``' three on top)."""
    from .model import JointSampleOptions  # (that module imports this one)
    return JointSampleOptions(sampler, clip_x0, guidance_scale, null_ms1, guidance_rescale, threshold_quantile, threshold_max, group_size,
                              consistency, consistency_strength).non_default()


def _reported_options(sampler_kw):
    """``_sampler_kwargs``' result as ``evaluate`` reports it: the same keys, plain str / float values"""
    return {k: str(v) if k in ("sampler", "consistency") else int(v) if k == "group_size" else float(v) for k, v in sampler_kw.items()}


def _wandb():
    try:
        import wandb

        return wandb
    except ImportError:
        print("wandb is not installed; continuing without it")
        return None


def _world() -> int:
    d = torch.distributed
    return d.get_world_size() if d.is_available() and d.is_initialized() else 1


def _rank() -> int:
    d = torch.distributed
    return d.get_rank() if d.is_available() and d.is_initialized() else 0
