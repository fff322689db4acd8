"""DDIM diffusion process -- drop-in for the reference's ``dquartic.model.model`` (reference model.py:14-406).

Same module-level helpers and the same ``DDIMDiffusionModel`` constructor, attributes and methods
(``q_sample``, ``p_sample``, ``sample``, ``train_step``).  When the wrapped network is this package's ``UNet1d`` the
arithmetic runs in libdq_hip.so: ``sample`` is one native call that walks all timesteps (network forward + DDIM update per
step, no host sync inside), ``train_step`` is one native call (normalise, q_sample, forward, MSE, backward into the flat
gradient buffer).  Any other ``nn.Module`` is driven with plain tensor ops exactly like the reference does, so the class
stays usable as a generic harness -- but that is the caller's network, not this package's hot path.

Documented deviations: batches are supported and ``train_step`` returns a 0-dim loss (the mean over
samples of the reference's B = 1 loss); both ``pred_type`` values are built; ``ms1_loss_weight > 0`` is built with chosen
semantics (the reference's branch raises TypeError).  A third objective the reference does not have,
``pred_type="v_prediction"`` (the network predicts v = sa eps - sb x0), is built for ``UNet1d``.
"""
import ctypes
import dataclasses
import math
import os
from typing import Optional

import torch
import torch.nn.functional as F

from .. import _native as N
from .model_interface import BucketedAllReduce, ModelInterface
from .unet1d import UNet1d


# beta schedules (reference model.py:14-54): fp64, cast by the caller
def get_linear_beta_schedule(num_timesteps, beta_start=0.0001, beta_end=0.02):
    return torch.linspace(beta_start, beta_end, num_timesteps, dtype=torch.float64)


def get_cosine_beta_schedule(num_timesteps, s=0.008):
    x = torch.linspace(0, num_timesteps, num_timesteps + 1, dtype=torch.float64)
    ac = torch.cos(((x / num_timesteps) + s) / (1 + s) * math.pi * 0.5) ** 2
    ac = ac / ac[0]
    return torch.clip(1 - (ac[1:] / ac[:-1]), 0, 0.999)


def get_alphas(betas):  # model.py:57-69
    return 1.0 - betas


def get_alpha_bars(alpha):  # model.py:72-84
    return torch.cumprod(alpha, dim=0)


def normalize_to_neg_one_to_one(img):  # model.py:89-99
    return img * 2 - 1


def unnormalize_to_zero_to_one(t):  # model.py:102-112
    return (t + 1) * 0.5


def identity(t, *args, **kwargs):  # model.py:115-125
    return t


def _f32(v):
    return v.detach().to(torch.float32).contiguous()


def extract(a, t, x_shape):  # model.py:131-148
    b, *_ = t.shape
    out = a.gather(-1, t)
    return out.reshape(b, *((1,) * (len(x_shape) - 1)))


# the MS1 term compares per-RT summaries of the prediction with a chromatogram: undefined for a (RT, M1) MS1
_MS1_TERM_MULTI = "ms1_loss_weight > 0 with attn_cond_channels > 1 is not implemented (the MS1 loss term is defined on a 1-D chromatogram)"


# the v objective is built through UNet1d's native paths; its follow-ups are named where they are refused
_V_OTHER_NETWORKS = ("pred_type 'v_prediction' is implemented for UNet1d only (follow-up: the CustomTransformer's train step, sampler and "
                     "evaluation under the v objective)")
_V_MS1_TERM = ("ms1_loss_weight > 0 with pred_type 'v_prediction' is not implemented (follow-up: the MS1 term under the v objective; DESIGN.md "
               "section 12 defines it for 'eps' and 'x0' only)")


@dataclasses.dataclass(frozen=True)
class SampleOptions:
    """The options of a sampling call beyond ``eta`` and the seed, at ``sample``'s public defaults (DESIGN.md sections 26, 32, 38): the one
    place that says which of them are live and what the library is handed for them."""
    sampler: str = "reference"
    clip_x0: Optional[float] = None
    guidance_scale: Optional[float] = None
    null_ms1: float = 0.0
    guidance_rescale: float = 0.0
    threshold_quantile: Optional[float] = None
    threshold_max: Optional[float] = None

    def non_default(self):
        """The options that are not at their defaults, as keyword arguments of ``sample`` -- none at the defaults, so that a subclass whose
        ``sample`` predates them is still called as it always was.  ``null_ms1`` goes with ``guidance_scale`` and never without it."""
        live = {"sampler": self.sampler != "reference", "clip_x0": self.clip_x0 is not None, "guidance_scale": self.guidance_scale is not None,
                "null_ms1": self.guidance_scale is not None, "guidance_rescale": bool(self.guidance_rescale),
                "threshold_quantile": self.threshold_quantile is not None, "threshold_max": self.threshold_max is not None}
        return {k: getattr(self, k) for k, on in live.items() if on}

    def resolve(self, eta, model):
        """What the library takes: ``(sampler id, clamp or 0.0, (w, null_ms1) or None, (phi, q, cap) or None)`` -- None where the call is
        the one without the option (a scale of 1.0; ``phi`` without guidance, where g = c and m = 1).  ValueError as the three checks of
        ``model`` (a ``DDIMDiffusionModel``, or a subclass with checks of its own) raise it, in their order."""
        sampler_id, clip = model._check_sampler(self.sampler, eta, self.clip_x0)
        w = model._check_guidance(self.guidance_scale)
        phi, q, cap = model._check_adaptive(self.guidance_rescale, self.threshold_quantile, self.threshold_max, self.sampler, eta, clip)
        phi = 0.0 if w is None else phi  # (g = c: m = 1)
        return sampler_id, clip, None if w is None else (w, float(self.null_ms1)), (phi, q, cap) if (phi > 0.0 or q > 0.0) else None


@dataclasses.dataclass(frozen=True)
class JointSampleOptions(SampleOptions):
    """``SampleOptions`` with the three options of a call over groups: the batch is ``B / group_size`` groups of
    ``group_size`` members, member-major, and every step's x0 estimates of a group are projected onto its mixture (``consistency``:
    "bound" or "sum") at ``consistency_strength``.  ``consistency`` without ``group_size`` means groups of one."""
    group_size: Optional[int] = None
    consistency: Optional[str] = None
    consistency_strength: float = 1.0

    def non_default(self):
        live = super().non_default()
        live.update({k: getattr(self, k) for k, on in (("group_size", self.group_size is not None), ("consistency", self.consistency is not None),
                                                       ("consistency_strength", self.consistency_strength != 1.0)) if on})
        return live

    def resolve_joint(self, model):
        """``(P, mode id, strength)`` as the library takes them, or None where the call is the one without the pass (no ``consistency``;
        ``group_size`` is then only checked).  ValueError as ``model._check_joint`` raises it."""
        return model._check_joint(self.group_size, self.consistency, self.consistency_strength)


# what sample() refuses together with a live consistency pass, by name
_JOINT_WITH_OPTIONS = ("sample: consistency together with guidance_scale, guidance_rescale or threshold_quantile is not implemented (follow-up: the "
                       "guided form of the group pass, which needs the mirror half written, and the per-window statistics over projected estimates)")

# the options only UNet1d's native sampler serves, as sample() refuses them: (on a CustomTransformer, on anything else)
_UNET_ONLY = {
    "joint": ("sample: group_size / consistency are built for UNet1d (dq_ddim_sample); the group pass for the CustomTransformer's sampler "
              "(dq_tfm_sample) is the follow-up",
              "sample: group_size / consistency need the native sampler (this package's UNet1d on the GPU with both conditions); the generic "
              "loop is the plain update only"),
    "adaptive": ("sample: guidance_rescale and threshold_quantile are built for UNet1d (dq_ddim_sample); the per-window statistics "
                 "step for the CustomTransformer's sampler (dq_tfm_sample) is the follow-up",
                 "sample: guidance_rescale and threshold_quantile need the native sampler (this package's UNet1d on the GPU with both "
                 "conditions); the generic loop is the plain update only"),
    "guidance": ("sample: guidance_scale is built for UNet1d (dq_ddim_sample); guidance for the CustomTransformer's sampler "
                 "(dq_tfm_sample) is the follow-up",
                 "sample: guidance_scale needs the native sampler (this package's UNet1d on the GPU with both conditions); the generic "
                 "loop is the unguided update only"),
}


class DDIMDiffusionModel(ModelInterface):
    def __init__(self, model_class, num_timesteps=1000, beta_schedule_type="cosine", pred_type="eps", auto_normalize=True,
                 ms1_loss_weight=0.0, device="cuda", **kwargs):
        super().__init__()
        self.model = None
        self.build(model_class, **kwargs)
        self.num_timesteps = num_timesteps
        self.device = device
        # schedule exactly as the reference forms it (model.py:196-202): fp64 betas -> device -> fp32, cumprod in fp32
        # The three tensors are formed on the HOST and then moved: a device cumprod (parallel scan) rounds differently
        # from the sequential CPU one, and parity is defined against the reference's CPU path.
        betas = (get_linear_beta_schedule(num_timesteps) if beta_schedule_type == "linear"
                 else get_cosine_beta_schedule(num_timesteps)).to(torch.float32)
        alphas = get_alphas(betas).to(torch.float32)
        alpha_bars = get_alpha_bars(alphas).to(torch.float32)
        self.betas, self.alphas, self.alpha_bars = betas.to(device), alphas.to(device), alpha_bars.to(device)
        snr = (alpha_bars / (1 - alpha_bars)).to(device)  # model.py:205
        if pred_type == "eps":
            self.loss_weight = torch.ones_like(snr)
        elif pred_type == "x0":
            self.loss_weight = snr
        elif pred_type == "v_prediction":
            # v = sa eps - sb x0 (Salimans & Ho 2022): the plain MSE on v is the x0 loss weighted by SNR + 1
            if not isinstance(self.model, UNet1d):
                raise NotImplementedError(_V_OTHER_NETWORKS)
            if ms1_loss_weight > 0:
                raise NotImplementedError(_V_MS1_TERM)
            self.loss_weight = torch.ones_like(snr)
        else:
            raise ValueError(f"Unknown pred_type: {pred_type}")
        self.normalize = normalize_to_neg_one_to_one if auto_normalize else identity
        self.unnormalize = unnormalize_to_zero_to_one if auto_normalize else identity
        self.auto_normalize = bool(auto_normalize)
        self.pred_type = pred_type
        self.ms1_loss_weight = ms1_loss_weight
        self._ab_host = None
        self.use_graph = True  # sample(): replay one hipGraph-captured step per timestep (an attribute, not an environment switch)
        # sample() on a CustomTransformer behind its adapter: True sends every call to the library's loop (dq_tfm_sample); False (default)
        # only the calls the generic loop cannot serve (eta > 0, seed, window_ids, x_t=None, another sampler, clip_x0, return_trajectory)
        self.native_tfm_sampler = False

    # ------------------------------------------------------------------ helpers
    @property
    def native(self) -> bool:
        return isinstance(self.model, UNet1d)

    def _alpha_bars_host(self):
        if self._ab_host is None:
            ab = self.alpha_bars.detach().to("cpu", torch.float32).contiguous()
            self._ab_host = (ab, (ctypes.c_float * ab.numel()).from_buffer_copy(ab.numpy().tobytes()))
        return self._ab_host[1]

    @staticmethod
    def sampler_timesteps(num_timesteps, num_steps):
        """model.py:313"""
        return torch.linspace(num_timesteps - 1, 0, num_steps, dtype=torch.long)

    # ------------------------------------------------------------------ forward process
    def q_sample(self, x_0, t, noise=None):
        """model.py:225-242; ``x_0`` is already normalised by the caller, as in the reference."""
        if noise is None:
            noise = torch.randn_like(x_0)
        # the native kernel when nothing upstream wants a gradient through the noising (the training paths of this package
        # draw x_0 / noise as leaves); otherwise the reference's tensor expressions, which keep the autograd history
        wants_grad = torch.is_grad_enabled() and (x_0.requires_grad or noise.requires_grad)
        if x_0.is_cuda and not wants_grad:
            x0c, nz = x_0.detach().float().contiguous(), noise.detach().float().contiguous()
            tt = t.reshape(-1).to(device=x_0.device, dtype=torch.int64).contiguous()
            ab = self.alpha_bars.to(x_0.device)
            out = torch.empty_like(x0c)
            B = x0c.shape[0]
            N.check(N.lib().dq_q_sample(N.ptr(ab), N.ptr(x0c), N.ptr(tt), N.ptr(nz), N.ptr(out), B, x0c[0].numel(), 0,
                                        N.stream_ptr()), "dq_q_sample")
            return out
        a = torch.sqrt(self.alpha_bars[t])[:, None, None]
        b = torch.sqrt(1.0 - self.alpha_bars[t])[:, None, None]
        return a * x_0 + b * noise

    # ------------------------------------------------------------------ stochastic sampling
    @staticmethod
    def _check_eta(eta):
        eta = float(eta)
        if not 0.0 <= eta <= 1.0:  # (NaN fails both comparisons)
            raise ValueError(f"eta must satisfy 0 <= eta <= 1, got {eta!r}")
        return eta

    @staticmethod
    def _seed_tensor(seed, device):
        """The 64-bit seed as the one device word the kernels read (an int64 tensor carrying the uint64 bit pattern).  None: one draw
        from torch's generator."""
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (1,)).item())
        seed = int(seed) & (2 ** 64 - 1)
        return torch.tensor([seed - 2 ** 64 if seed >= 2 ** 63 else seed], dtype=torch.int64, device=device)

    @staticmethod
    def _ids_tensor(window_ids, B, device):
        if window_ids is None:
            return None
        ids = torch.as_tensor(window_ids, dtype=torch.int64).reshape(-1).to(device).contiguous()
        if ids.numel() != B:
            raise ValueError(f"window_ids must have one id per window of the batch ({B}), got {ids.numel()}")
        return ids

    def ddim_coef_table(self, timesteps, eta=0.0):
        """``dq_ddim_coef_table`` (host only): per step the rows [sqrt(ab), sqrt(1-ab), sqrt(ab_prev), c] and sigma as two float32 CPU
        tensors (num_steps, 4) and (num_steps,)."""
        ts = [int(v) for v in timesteps]
        ts_c = (ctypes.c_int32 * len(ts))(*ts)
        coef, sigma = (ctypes.c_float * (4 * len(ts)))(), (ctypes.c_float * len(ts))()
        N.check(N.lib().dq_ddim_coef_table(self._alpha_bars_host(), int(self.num_timesteps), ts_c, len(ts), float(eta), coef, sigma),
                "dq_ddim_coef_table")
        return torch.tensor(list(coef), dtype=torch.float32).reshape(-1, 4), torch.tensor(list(sigma), dtype=torch.float32)

    # ------------------------------------------------------------------ step-consistent samplers
    @staticmethod
    def _check_sampler(sampler, eta, clip_x0):
        """(sampler id, clip value or 0.0).  Raises ValueError for an unknown name and for the combinations no kernel runs."""
        if sampler not in N.SAMPLERS:
            raise ValueError(f"Unknown sampler: {sampler!r} (one of {sorted(N.SAMPLERS)})")
        clip = 0.0 if clip_x0 is None else float(clip_x0)
        if clip_x0 is not None and not clip > 0.0:  # (NaN fails the comparison)
            raise ValueError(f"clip_x0 must be > 0 or None, got {clip_x0!r}")
        if sampler == "dpmpp_2m" and eta > 0.0:
            raise ValueError("sampler 'dpmpp_2m' is deterministic: eta must be 0")
        if clip > 0.0 and sampler == "reference":
            raise ValueError("clip_x0 needs sampler 'ddim' or 'dpmpp_2m'")
        if clip > 0.0 and eta > 0.0:
            raise ValueError("clip_x0 needs eta == 0")
        return N.SAMPLERS[sampler], clip

    @staticmethod
    def _check_decreasing(ts):
        if any(b >= a for a, b in zip(ts[:-1], ts[1:])):
            raise ValueError("the timesteps of the 'ddim' and 'dpmpp_2m' samplers must be strictly decreasing (num_steps <= num_timesteps)")

    def sampler_coef_table(self, timesteps, sampler="reference", eta=0.0):
        """``dq_sampler_coef_table`` (host only): two float32 CPU tensors (num_steps, 4) and (num_steps,).  'reference': what
        ``ddim_coef_table`` returns; 'ddim': the same rows landing on ``alpha_bars[timesteps[i + 1]]`` and sigma; 'dpmpp_2m': rows
        [sa, sb, cx, c0] and c1 of ``x_prev = cx x + c0 x0 + c1 x0_hist``.  The last row returns x0."""
        if sampler not in N.SAMPLERS:
            raise ValueError(f"Unknown sampler: {sampler!r} (one of {sorted(N.SAMPLERS)})")
        ts = [int(v) for v in timesteps]
        ts_c = (ctypes.c_int32 * len(ts))(*ts)
        coef, extra = (ctypes.c_float * (4 * len(ts)))(), (ctypes.c_float * len(ts))()
        rc = N.lib().dq_sampler_coef_table(self._alpha_bars_host(), int(self.num_timesteps), ts_c, len(ts), N.SAMPLERS[sampler], float(eta),
                                           coef, extra)
        if rc:
            raise ValueError(N.last_error())
        return torch.tensor(list(coef), dtype=torch.float32).reshape(-1, 4), torch.tensor(list(extra), dtype=torch.float32)

    # ------------------------------------------------------------------ reverse process
    def p_sample(self, x_t, t, init_cond=None, attn_cond=None, eta=0.0, seed=None, window_ids=None, draw=None):
        """model.py:244-291.  ``t`` is a python int; conditions are already normalised.  ``eta > 0`` (device tensors, no autograd through
        the step): the update of ``dq_ddim_step_sto`` with the noise of (``seed``, ``window_ids``, draw index ``draw``: step i of a loop
        draws at 1 + i)."""
        eta = self._check_eta(eta)
        batch_size = x_t.size(0)
        t_tensor = torch.full((batch_size,), int(t), device=x_t.device, dtype=torch.long)
        ab = self.alpha_bars[t]
        sa, sb = torch.sqrt(ab), torch.sqrt(1.0 - ab)
        if self.pred_type not in N.PRED_TYPES:
            raise ValueError(f"Unknown pred_type: {self.pred_type}")
        out = self.model(x_t, t_tensor, init_cond, attn_cond)  # eps_pred, x0_pred (model.py:271 / :276) or v_pred
        wants_grad = torch.is_grad_enabled() and (x_t.requires_grad or out.requires_grad)
        if eta > 0.0:
            if not x_t.is_cuda or wants_grad:
                raise NotImplementedError("p_sample: eta > 0 runs in the native update kernel only (device tensors, no autograd through the step)")
            if seed is None or draw is None:
                raise ValueError("p_sample: eta > 0 needs seed and draw (the step's draw index: 1 + i for step i of a loop)")
            cf, sg = self.ddim_coef_table([t], eta)
            coef = torch.cat([cf.reshape(-1), sg]).to(x_t.device)
            xt, o = x_t.detach().float().contiguous(), out.detach().float().contiguous()
            x_prev = torch.empty_like(xt)
            eps_pred = torch.empty_like(xt) if self.pred_type != "eps" else None
            ids_dev, seed_dev = self._ids_tensor(window_ids, batch_size, x_t.device), self._seed_tensor(seed, x_t.device)
            N.check(N.lib().dq_ddim_step_sto(N.ptr(xt), N.ptr(o), N.ptr(x_prev), N.ptr(eps_pred), N.ptr(coef), N.ptr(ids_dev), N.ptr(seed_dev),
                                             int(draw), N.PRED_TYPES[self.pred_type], batch_size, xt[0].numel(), N.stream_ptr()),
                    "dq_ddim_step_sto")
            return x_prev, (out if self.pred_type == "eps" else eps_pred)
        if x_t.is_cuda and not wants_grad:
            if t > 0:
                abp = self.alpha_bars[t - 1]
                coef = torch.stack([sa, sb, torch.sqrt(abp), torch.sqrt(1.0 - abp)]).to(x_t.device, torch.float32)
            else:
                coef = torch.stack([sa, sb, -torch.ones_like(sa), torch.zeros_like(sa)]).to(x_t.device, torch.float32)
            xt, o = x_t.detach().float().contiguous(), out.detach().float().contiguous()
            x_prev = torch.empty_like(xt)
            if self.pred_type == "eps":
                N.check(N.lib().dq_ddim_step(N.ptr(xt), N.ptr(o), N.ptr(x_prev), N.ptr(coef), xt.numel(), N.stream_ptr()), "dq_ddim_step")
                return x_prev, out
            eps_pred = torch.empty_like(xt)
            if self.pred_type == "v_prediction":
                N.check(N.lib().dq_ddim_step_v(N.ptr(xt), N.ptr(o), N.ptr(x_prev), N.ptr(eps_pred), N.ptr(coef), xt.numel(),
                                               N.stream_ptr()), "dq_ddim_step_v")
                return x_prev, eps_pred
            N.check(N.lib().dq_ddim_step_x0(N.ptr(xt), N.ptr(o), N.ptr(x_prev), N.ptr(eps_pred), N.ptr(coef), xt.numel(),
                                            N.stream_ptr()), "dq_ddim_step_x0")
            return x_prev, eps_pred
        # host tensors (only reachable with a non-native network) or a caller differentiating through the step: the reference's
        # arithmetic as is
        if self.pred_type == "eps":
            eps_pred, x0_pred = out, (x_t - sb * out) / sa
        elif self.pred_type == "v_prediction":
            x0_pred, eps_pred = sa * x_t - sb * out, sb * x_t + sa * out
        else:
            x0_pred, eps_pred = out, (x_t - sa * out) / sb
        if t > 0:
            abp = self.alpha_bars[t - 1]
            x_prev = torch.sqrt(abp) * x0_pred + torch.sqrt(1.0 - abp) * eps_pred
        else:
            x_prev = x0_pred
        return x_prev, eps_pred

    @staticmethod
    def _check_guidance(guidance_scale):
        """None for the call as it always was (``None`` and 1.0: the conditional model itself), else the scale as a float.  ValueError for
        anything that is not a finite number >= 0 (as the float32 the kernels take it as)."""
        if guidance_scale is None:
            return None
        try:
            w = float(guidance_scale)
        except (TypeError, ValueError):
            raise ValueError(f"guidance_scale must be a finite number >= 0 or None, got {guidance_scale!r}") from None
        if not (w >= 0.0 and w <= float(torch.finfo(torch.float32).max)):  # (NaN fails both comparisons)
            raise ValueError(f"guidance_scale must be a finite number >= 0 or None, got {guidance_scale!r}")
        return None if w == 1.0 else w

    @staticmethod
    def _check_adaptive(guidance_rescale, threshold_quantile, threshold_max, sampler, eta, clip):
        """(phi, q or 0.0, cap): the two per-window options as the library takes them.  ValueError for ``phi`` outside
        [0, 1], ``q`` outside (0, 1] (as the float32 the kernels take it as), a cap below the floor, NaN anywhere, and thresholding with
        the combinations ``clip_x0`` is refused with."""
        try:
            phi = float(guidance_rescale)
        except (TypeError, ValueError):
            raise ValueError(f"guidance_rescale must be a number in [0, 1], got {guidance_rescale!r}") from None
        if not (0.0 <= phi <= 1.0):  # (NaN fails the comparison)
            raise ValueError(f"guidance_rescale must be a number in [0, 1], got {guidance_rescale!r}")
        if threshold_quantile is None:
            if threshold_max is not None:
                raise ValueError("threshold_max needs threshold_quantile")
            return phi, 0.0, float("inf")
        try:
            q = float(torch.tensor(float(threshold_quantile), dtype=torch.float32))
        except (TypeError, ValueError):
            raise ValueError(f"threshold_quantile must be a number in (0, 1] or None, got {threshold_quantile!r}") from None
        if not (0.0 < q <= 1.0):
            raise ValueError(f"threshold_quantile must be a number in (0, 1] or None, got {threshold_quantile!r}")
        if sampler == "reference":
            raise ValueError("threshold_quantile needs sampler 'ddim' or 'dpmpp_2m'")
        if eta > 0.0:
            raise ValueError("threshold_quantile needs eta == 0")
        floor = clip if clip > 0.0 else 1.0
        cap = float("inf") if threshold_max is None else float(threshold_max)
        if not cap >= floor:
            raise ValueError(f"threshold_max must be >= the floor ({floor!r}: clip_x0, or 1 without it), got {threshold_max!r}")
        return phi, q, cap

    @staticmethod
    def _check_joint(group_size, consistency, consistency_strength):
        """``(P, mode id, strength)`` of a call over groups, or None without ``consistency`` (``group_size`` is then
        only checked).  ValueError for a ``group_size`` that is not an integer in [1, 8], an unknown ``consistency``, and a strength outside
        (0, 1] (as the float32 the kernel takes it as; NaN included)."""
        P = 1
        if group_size is not None:
            if isinstance(group_size, bool) or not isinstance(group_size, int) or not 1 <= group_size <= N.GROUP_MAX:
                raise ValueError(f"group_size must be an integer in [1, {N.GROUP_MAX}] or None, got {group_size!r}")
            P = int(group_size)
        if consistency is not None and consistency not in N.CONSISTENCY_MODES:
            raise ValueError(f"Unknown consistency: {consistency!r} (one of {sorted(N.CONSISTENCY_MODES)}, or None)")
        try:
            strength = float(torch.tensor(float(consistency_strength), dtype=torch.float32))
        except (TypeError, ValueError):
            raise ValueError(f"consistency_strength must be a number in (0, 1], got {consistency_strength!r}") from None
        if not (0.0 < strength <= 1.0):  # (NaN fails the comparison)
            raise ValueError(f"consistency_strength must be a number in (0, 1], got {consistency_strength!r}")
        return None if consistency is None else (P, N.CONSISTENCY_MODES[consistency], strength)

    def sample(self, x_t, ms2_cond=None, ms1_cond=None, num_steps=1000, return_trajectory=False, eta=0.0, seed=None, window_ids=None,
               shape=None, sampler="reference", clip_x0=None, guidance_rescale=0.0, threshold_quantile=None, threshold_max=None,
               group_size=None, consistency=None, consistency_strength=1.0, guidance_scale=None, null_ms1=0.0):
        """model.py:293-324: returns (denoised, mixture - denoised).  Native loop when the network is UNet1d; for a CustomTransformer behind
        ``DDIMTransformerAdapter`` the library's loop (``dq_tfm_sample``) serves every call when
        ``native_tfm_sampler`` is set, and otherwise exactly the calls the generic loop refuses (the options below, ``return_trajectory``).

        ``eta`` in [0, 1]: 0 is the deterministic DDIM update, 1 ancestral (DDPM-like) sampling; the per-step noise
        is a counter-based generator inside the update kernel, keyed by (``seed``, window id, element, step), so a window's result does
        not depend on its place in the batch.  ``seed``: a 64-bit int (None with ``eta > 0``: drawn once from torch's generator);
        ``window_ids``: one int64 id per window (None: 0 .. B-1).  ``x_t=None`` draws x_T from the same generator (needs ``seed``); the
        shape is ``shape`` or ``ms2_cond``'s.  Native path only.  The defaults are the call as it always was.

        ``sampler``: "reference" lands every step on ``alpha_bars[t - 1]`` as the reference does (exact only at
        ``num_steps == num_timesteps``); "ddim" lands step i on the list's next timestep; "dpmpp_2m" is DPM-Solver++(2M) over the same
        list (``eta`` must be 0).  The last step of either returns the x0 estimate.  ``clip_x0 = c > 0`` (those two samplers, ``eta == 0``)
        clamps every step's x0 estimate to [-c, c].  Native path only.

        ``guidance_scale = w``: classifier-free guidance on MS1, the one input that names the component to extract.
        Every step's update runs on ``g = u + w (c - u)``, c the network output under ``ms1_cond`` and u the output under the null
        condition -- MS1 equal to the raw value ``null_ms1`` in every element, what ``set_cond_dropout`` trains the network on.  ``None``
        and 1.0 are the call as it is without the option, bit for bit: 1.0 *is* the conditional model, no doubled batch is run for it.
        Any other finite ``w >= 0`` (0: the unconditional model; > 1 pushes towards the component MS1 names) runs one forward at twice
        the batch per step inside the library and combines with every option above.  UNet1d on the GPU
        only: the generic loop and the CustomTransformer raise NotImplementedError.

        ``guidance_rescale = phi`` in [0, 1] and ``threshold_quantile = q`` in (0, 1] look at each window as a
        whole.  Rescaled guidance (Lin et al. 2024): the guided output of a window is multiplied by ``phi * std(c) / std(g) + (1 - phi)``,
        which takes back the spread a scale well above 1 adds; it needs ``guidance_scale`` (with ``None`` or 1.0 it is a no-op, ``g = c``)
        and works with every sampler and ``eta``.  Dynamic thresholding (Saharia et al. 2022): every step's x0 estimate is clamped to the
        window's ``q``-quantile ``s`` of ``|x0|`` -- never below the floor ``f = clip_x0`` (1 without it), never above ``threshold_max`` --
        and scaled by ``f / s``, which keeps the shape of a peak the constant clamp would cut flat; it is allowed where ``clip_x0`` is
        ('ddim' or 'dpmpp_2m', ``eta == 0``).  The defaults are the call as it is without the options, bit for bit and launch for launch.
        UNet1d on the GPU only.

        ``group_size = P`` and ``consistency`` sample the P precursors of an isolation window as one group.  The
        batch is ``B / P`` groups of P members, member-major -- member p of group g is row ``p * G + g``, the concatenation of P ordinary
        batches that share their ``ms2_cond`` rows and differ in ``ms1_cond`` -- and the group's mixture is row g of ``ms2_cond``.  Between
        the network forward and the update every step's x0 estimates are projected in the mixture's units: ``"bound"`` scales a group's
        positive parts down wherever their sum exceeds the mixture (nothing is raised, negatives are not touched; with P = 1 a prediction
        never exceeds the observation), ``"sum"`` scales them so that they add up to the mixture (negatives go to 0).
        ``consistency_strength`` in (0, 1] blends between the estimate (towards 0) and its projection (1).  The update then runs on the
        projected x0 whatever the objective.  ``consistency=None`` is the call as it is without the option, bit for bit (``group_size``
        is only checked); ``consistency`` without ``group_size`` means P = 1.  Works with every sampler, ``eta``, ``clip_x0``, seeds, window
        ids and trajectories; not together with ``guidance_scale``, ``guidance_rescale`` or ``threshold_quantile``.  UNet1d on the GPU only."""
        eta = self._check_eta(eta)
        options = JointSampleOptions(sampler, clip_x0, guidance_scale, null_ms1, guidance_rescale, threshold_quantile, threshold_max, group_size,
                                     consistency, consistency_strength)
        sampler_id, clip, guidance, adaptive = options.resolve(eta, self)
        joint = options.resolve_joint(self)
        if group_size is not None:
            B = int((shape if x_t is None and shape is not None else (x_t if x_t is not None else ms2_cond).shape)[0])
            if B % int(group_size):
                raise ValueError(f"the batch ({B}) must be a whole number of groups of group_size = {group_size}")
        if joint is not None and (guidance is not None or adaptive is not None):
            raise NotImplementedError(_JOINT_WITH_OPTIONS)
        stochastic = eta > 0.0 or x_t is None or seed is not None or window_ids is not None
        if sampler_id != 0:
            self._check_decreasing(self.sampler_timesteps(self.num_timesteps, num_steps).tolist())
        on_gpu = ms2_cond is not None and ms1_cond is not None and (x_t.is_cuda if x_t is not None else ms2_cond.is_cuda)
        # the route, decided once: UNet1d's loop, the transformer's, or the generic one below
        unet_only = "adaptive" if adaptive is not None else "guidance" if guidance is not None else "joint" if joint is not None else None
        if unet_only and not (self.native and on_gpu):
            raise NotImplementedError(_UNET_ONLY[unet_only][0 if self._native_tfm else 1])
        call = dict(seed=seed, window_ids=window_ids, shape=shape, sampler=sampler_id, clip_x0=clip)
        if self.native and on_gpu:
            # (the default call passes eta=None: the call as it always was; ``adaptive`` and ``joint`` only when live)
            plain = not (unet_only or stochastic or sampler_id != 0)
            return self._sample_native(x_t, ms2_cond, ms1_cond, num_steps, return_trajectory, eta=None if plain else eta, guidance=guidance,
                                       **call, **({} if adaptive is None else {"adaptive": adaptive}), **({} if joint is None else {"joint": joint}))
        if on_gpu and self._native_tfm and (self.native_tfm_sampler or stochastic or sampler_id != 0 or return_trajectory):
            return self._sample_native_tfm(x_t, ms2_cond, ms1_cond, num_steps, return_trajectory, eta=eta, **call)
        if sampler_id != 0:
            raise NotImplementedError("sample: the 'ddim' and 'dpmpp_2m' samplers and clip_x0 need the native sampler (this package's "
                                      "UNet1d, or its CustomTransformer behind DDIMTransformerAdapter, on the GPU with both "
                                      "conditions); the generic loop is the reference update only")
        if stochastic:
            raise NotImplementedError("sample: eta > 0, seed, window_ids and x_t=None need the native sampler (this package's UNet1d, or "
                                      "its CustomTransformer behind DDIMTransformerAdapter, on the GPU with both conditions); the "
                                      "generic loop is the deterministic update only")
        ms2n = self.normalize(ms2_cond) if ms2_cond is not None else None
        ms1n = self.normalize(ms1_cond) if ms1_cond is not None else None
        pred_noise = None
        for t in self.sampler_timesteps(self.num_timesteps, num_steps):
            x_t, pred_noise = self.p_sample(x_t, int(t.item()), ms2n, ms1n)
        x_t, pred_noise = self.unnormalize(x_t), self.unnormalize(pred_noise)
        if ms2n is not None:
            pred_noise = self.unnormalize(ms2n) - x_t
        return x_t, pred_noise

    # what the native calls stage alike
    def _stage_step(self, x_0, t, noise, draw_noise=True):
        """A step's batch as the library reads it: ``(x_0, t, noise, alpha_bars, loss_weight)``, contiguous fp32 / int64 on ``x_0``'s device.
        What was not passed is drawn in the reference's order: ``randint`` for ``t`` first, then ``randn_like`` for the noise (not with
        ``draw_noise=False``: the noise stays None)."""
        x_0 = _f32(x_0)
        dev = x_0.device
        if t is None:
            t = torch.randint(0, self.num_timesteps, (x_0.shape[0],), device=dev).long()
        if noise is None and draw_noise:
            noise = torch.randn_like(x_0)
        return (x_0, t.to(device=dev, dtype=torch.int64).contiguous(), None if noise is None else _f32(noise), self.alpha_bars.to(dev),
                self.loss_weight.to(device=dev, dtype=torch.float32).contiguous())

    @staticmethod
    def _stage_tfm(tfm, ms1_cond, who, what, *shapes):
        """The transformer's inputs: every shape of ``shapes`` (``what`` in the refusal) must be the same (batch, seqlen1, input_dim);
        ``ms1_cond`` (B, S2) or (B, S2, 1) comes back as contiguous fp32 (B, S2).  Returns ``(c1, B, S1, S2, D)``."""
        c1 = _f32(ms1_cond)
        if c1.dim() == 3:
            c1 = c1[..., 0].contiguous()
        if len(shapes[0]) != 3 or shapes[0][-1] != tfm.input_dim or any(tuple(v) != tuple(shapes[0]) for v in shapes):
            raise ValueError(f"{who}: {what} must be (batch, seqlen1, input_dim={tfm.input_dim})")
        B, S1, D = shapes[0]
        if c1.dim() != 2 or c1.shape[0] != B:
            raise ValueError(f"{who}: ms1_cond must be (batch, seqlen2) or (batch, seqlen2, 1)")
        return c1, B, S1, c1.shape[1], D

    @staticmethod
    def _stage_x(x_T, ms2_cond, eta, seed, shape):
        """(x_T or None, ms2_cond) as contiguous fp32 and the call's (batch, rows, width): x_T's, else ``shape`` or ``ms2_cond``'s."""
        if x_T is None:
            if seed is None and not eta:
                raise ValueError("sample: x_t=None needs a seed (x_T is drawn from it)")
            B, S, D = tuple(shape) if shape is not None else tuple(ms2_cond.shape)
        else:
            B, S, D = x_T.shape
            x_T = _f32(x_T)
        return x_T, _f32(ms2_cond), B, S, D

    def _stage_noise(self, x_T, eta, seed, window_ids, B, device):
        """The seed and window-id tensors of a call (None where the loop reads none); records ``last_seed``."""
        seed_dev = self._seed_tensor(seed, device) if (seed is not None or eta > 0.0 or x_T is None) else None
        ids_dev = self._ids_tensor(window_ids, B, device)
        self.last_seed = None if seed_dev is None else int(seed_dev.item()) & (2 ** 64 - 1)  # (what a seed=None call drew)
        return seed_dev, ids_dev

    def _run_loop(self, entry, head, call, x_T, c2, c1, ws, num_steps, dims, return_trajectory):
        """What both native calls stage alike, and the call: the int32 timesteps, [out_x, out_noise, traj_x, traj_eps] (the trajectories
        (num_steps, *dims), or None), the graph flag (off with a trajectory) and the fields of the record (``N.sample_call``) that both
        networks fill alike -- the schedule, the tensors, the workspace, the batch, the stream -- then the caller's own by name (``call``);
        the entry takes the network's arguments (``head``) and the record.  Returns what ``sample`` returns."""
        ts_c = (ctypes.c_int32 * num_steps)(*self.sampler_timesteps(self.num_timesteps, num_steps).to(torch.int32).tolist())
        outs = [torch.empty_like(c2), torch.empty_like(c2)] + [
            torch.empty((num_steps, *dims), device=c2.device) if return_trajectory else None for _ in range(2)]
        q = N.sample_call(alpha_bars_host=ctypes.addressof(self._alpha_bars_host()), num_timesteps=int(self.num_timesteps), x_T=N.ptr(x_T),
                          ms2_cond=N.ptr(c2), ms1_cond=N.ptr(c1), auto_normalize=1 if self.auto_normalize else 0,
                          pred_type=N.PRED_TYPES[self.pred_type], timesteps_host=ctypes.addressof(ts_c), num_steps=num_steps,
                          out_x=N.ptr(outs[0]), out_noise=N.ptr(outs[1]), traj_x=N.ptr(outs[2]), traj_eps=N.ptr(outs[3]),
                          use_graph=1 if (self.use_graph and not return_trajectory) else 0, workspace=N.ptr(ws), workspace_bytes=ws.numel(),
                          B=dims[0], RT=dims[1], stream=N.stream_ptr(), **call)
        N.check(getattr(N.lib(), entry)(*head, ctypes.byref(q)), entry)
        return tuple(outs) if return_trajectory else tuple(outs[:2])

    def _sample_native(self, x_T, ms2_cond, ms1_cond, num_steps, return_trajectory=False, eta=None, seed=None, window_ids=None, shape=None,
                       sampler=0, clip_x0=0.0, guidance=None, adaptive=None, joint=None):
        """The U-Net's loop in the library (``dq_ddim_sample``); the record holds what is live and leaves every other option off.  ``eta``
        None: the call as it always was (eta 0, no seed, no ids; ``last_seed`` untouched); ``guidance`` = (scale, null_ms1): on the
        workspace of twice the batch; ``adaptive`` = (phi, q, cap): with the statistics scratch; ``joint`` = (P, mode, strength): never
        with ``adaptive`` or ``guidance``."""
        net: UNet1d = self.model
        x_T, c2, B, RT, MZ = self._stage_x(x_T, ms2_cond, eta, seed, shape)
        c1 = net._check_inputs(ms1_cond, B, RT).detach().to(torch.float32).contiguous()
        flat = net.read_params()  # (the averaged weights inside ModelInterface.ema_scope())
        ws = net.workspace(2 * B if guidance is not None else B, RT, False)
        call = {}
        if eta is not None:
            seed_dev, ids_dev = self._stage_noise(x_T, eta, seed, window_ids, B, c2.device)
            call.update(eta=float(eta), seed_dev=N.ptr(seed_dev), window_ids_dev=N.ptr(ids_dev), sampler=int(sampler), clip_x0=float(clip_x0))
        if guidance is not None:
            call.update(guided=1, guidance_scale=float(guidance[0]), null_ms1=float(guidance[1]))
        if adaptive is not None:
            stat = net.stat_scratch(B, RT * MZ)
            call.update(guidance_rescale=float(adaptive[0]), threshold_quantile=float(adaptive[1]), threshold_max=float(adaptive[2]),
                        stat_scratch=N.ptr(stat), stat_scratch_bytes=stat.numel())
        if joint is not None:
            call.update(group_size=int(joint[0]), consistency=int(joint[1]), consistency_strength=float(joint[2]))
        return self._run_loop("dq_ddim_sample", [net._plan, N.ptr(flat), N.ptr(net.rope_freqs())], call, x_T, c2, c1, ws, num_steps,
                              (B, RT, MZ), return_trajectory)

    @property
    def _native_tfm(self) -> bool:
        from .building_blocks import CustomTransformer, DDIMTransformerAdapter

        return isinstance(self.model, DDIMTransformerAdapter) and isinstance(self.model.transformer, CustomTransformer)

    def _sample_native_tfm(self, x_T, ms2_cond, ms1_cond, num_steps, return_trajectory=False, eta=0.0, seed=None, window_ids=None, shape=None,
                           sampler=0, clip_x0=0.0):
        """``dq_tfm_sample``: the whole loop in the library for the transformer behind its adapter (``ms1_cond`` (B, RT) or (B, RT, 1) is
        its conditional sequence; ``ms2_cond`` only enters ``mixture - denoised``)."""
        tfm = self.model.transformer
        x_T, c2, B, S1, D = self._stage_x(x_T, ms2_cond, eta, seed, shape)
        c1, _, _, S2, _ = self._stage_tfm(tfm, ms1_cond, "sample", "x_t and ms2_cond", (B, S1, D), c2.shape)
        flat = tfm.read_params(False)  # (the averaged weights inside ModelInterface.ema_scope())
        ws = tfm.sample_workspace(B, S1, S2, num_steps)
        sin, cos, freqs = tfm.tables(max(S1, S2), c2.device)
        seed_dev, ids_dev = self._stage_noise(x_T, eta, seed, window_ids, B, c2.device)
        call = dict(eta=float(eta), seed_dev=N.ptr(seed_dev), window_ids_dev=N.ptr(ids_dev), sampler=int(sampler), clip_x0=float(clip_x0))
        return self._run_loop("dq_tfm_sample", [tfm._tfm, N.ptr(flat), N.ptr(sin), N.ptr(cos), N.ptr(freqs), S2], call, x_T, c2, c1, ws,
                              num_steps, (B, S1, D), return_trajectory)

    # ------------------------------------------------------------------ training objective
    def train_step(self, x_0, ms2_cond=None, ms1_cond=None, noise=None, ms1_loss_weight=0.0, t=None):
        """model.py:326-406 (both pred types; ``ms1_loss_weight > 0`` with the semantics of DESIGN.md section 12: the reference's
        branch raises).  Draw order as in the reference: ``randint`` then
        ``randn_like``.  A passed ``noise`` is mapped 2*noise-1 like the reference does (model.py:346).  Returns a 0-dim loss
        (mean over samples of loss_weight[t_b] * MSE_b) that carries autograd history through the native network (generic
        path; the fused path is ``train_step_fused``)."""
        if self.pred_type not in N.PRED_TYPES:
            raise ValueError(f"Unknown pred_type: {self.pred_type}")
        if float(ms1_loss_weight or 0.0) > 0.0 and getattr(self.model, "attn_cond_channels", 1) > 1:
            raise NotImplementedError(_MS1_TERM_MULTI)
        if float(ms1_loss_weight or 0.0) > 0.0 and self.pred_type == "v_prediction":
            raise NotImplementedError(_V_MS1_TERM)
        batch_size = x_0.size(0)
        if t is None:
            t = torch.randint(0, self.num_timesteps, (batch_size,), device=x_0.device).long()
        noise = torch.randn_like(x_0) if noise is None else self.normalize(noise)
        x_0 = self.normalize(x_0)
        ms2n = self.normalize(ms2_cond) if ms2_cond is not None else None
        ms1n = self.normalize(ms1_cond) if ms1_cond is not None else None
        x_t = self.q_sample(x_0, t, noise=noise)
        out = self.model(x_t, t, ms2n, ms1n)
        w = float(ms1_loss_weight or 0.0)
        if self.pred_type == "eps" and w <= 0.0:
            return F.mse_loss(out, noise) * 1.0  # loss_weight is all-ones for the eps objective (model.py:208-209, 404)
        if self.pred_type == "v_prediction":  # v = sa eps - sb x0
            ab = self.alpha_bars.to(x_0.device)
            target = extract(torch.sqrt(ab), t, x_0.shape) * noise - extract(torch.sqrt(1.0 - ab), t, x_0.shape) * x_0
        else:
            target = noise if self.pred_type == "eps" else x_0
        per_sample = ((out - target) ** 2).flatten(1).mean(dim=1)  # model.py:361 / :376 at B = 1, per sample here
        if w > 0.0:  # model.py:364-371, 379-386, 398-402 with the chosen semantics (this generic path: plain tensor expressions)
            d = (x_t - out) if self.pred_type == "eps" else out
            m1 = ms1n if ms1n.dim() == 2 else ms1n[..., 0]
            tgt = m1 / m1.max(dim=-1, keepdim=True).values
            add = torch.zeros_like(per_sample)
            for sic in (d.sum(dim=-1), d.mean(dim=-1), d.max(dim=-1).values):
                add = add + ((sic / sic.max(dim=-1, keepdim=True).values - tgt) ** 2).mean(dim=-1)
            per_sample = (1 - w) * per_sample + w * add
        return (per_sample * self.loss_weight.to(per_sample.device)[t]).mean()  # model.py:404

    def train_step_fused(self, x_0, ms2_cond, ms1_cond, t=None, noise=None, zero_grads=True, ms1_loss_weight=0.0):
        """One native call: normalise, q_sample, U-Net forward, MSE, backward into ``model.flat_grads()`` (+=).
        Returns the loss as a 0-dim device tensor (no host sync)."""
        from .building_blocks import DDIMTransformerAdapter

        if isinstance(self.model, DDIMTransformerAdapter):
            return self._train_step_fused_tfm(x_0, ms1_cond, t, noise, zero_grads, float(ms1_loss_weight or 0.0))
        net: UNet1d = self.model
        if not self.native:
            raise RuntimeError("train_step_fused needs this package's UNet1d or a DDIMTransformerAdapter")
        B, RT, MZ = x_0.shape
        if float(ms1_loss_weight or 0.0) > 0.0 and net.attn_cond_channels > 1:
            raise NotImplementedError(_MS1_TERM_MULTI)
        if float(ms1_loss_weight or 0.0) > 0.0 and self.pred_type == "v_prediction":
            raise NotImplementedError(_V_MS1_TERM)
        c2, c1 = _f32(ms2_cond), _f32(net._check_inputs(ms1_cond, B, RT))
        x_0, t, noise, ab, lw = self._stage_step(x_0, t, noise)
        flat = net.read_params(training=True)  # (raises inside ema_scope(): the average is not trained)
        grads = net.flat_grads(zero=zero_grads)
        ws = net.workspace(B, RT, True)
        loss = torch.empty((), dtype=torch.float32, device=x_0.device)
        N.check(N.lib().dq_train_step(net._plan, N.ptr(flat), N.ptr(net.rope_freqs()), N.ptr(ab), N.ptr(x_0), N.ptr(c2), N.ptr(c1),
                                      N.ptr(t), N.ptr(noise), 1 if self.auto_normalize else 0, N.PRED_TYPES[self.pred_type], N.ptr(lw),
                                      float(ms1_loss_weight or 0.0), N.ptr(grads), N.ptr(loss), N.ptr(ws), ws.numel(), B, RT,
                                      N.stream_ptr()), "dq_train_step")
        return loss

    @torch.no_grad()
    def eval_step(self, x_0, ms2_cond, ms1_cond, t=None, noise=None):
        """Forward-only counterpart of ``train_step_fused`` (``dq_eval_step``): normalise, q_sample, U-Net forward
        without anything kept for a backward, per-window MSE.  Returns ``(loss, per_window)`` as device tensors: ``per_window`` (B) is the
        unweighted MSE of each window against its target (the noise for ``eps``, the normalised ``x_0`` for ``x0``, ``sa noise - sb x_0`` for ``v_prediction``), ``loss`` (0-dim) the
        mean over windows of ``loss_weight[t_b] * per_window[b]``.  The MSE part only: the MS1 term of the training loss is not evaluated.
        It sets no ``.grad``, needs no optimiser, uses the inference workspace and reads the averaged weights inside ``ema_scope()``.
        ``noise`` is used as passed.  Native network only: this package's UNet1d, or its CustomTransformer behind
        ``DDIMTransformerAdapter`` (``dq_tfm_eval_step`` at one repeat; ``ms1_cond`` (B, RT) or (B, RT, 1),
        ``ms2_cond`` unused: that network has no input for it)."""
        if self._native_tfm:
            x_0, t, noise, _, _ = self._stage_step(x_0, t, noise)
            loss, per_window = self._eval_steps_tfm(x_0, ms1_cond, t.reshape(1, -1), noise=noise)
            return loss[0], per_window[0]
        net: UNet1d = self.model
        if not self.native:
            raise NotImplementedError("eval_step runs in the native library only (this package's UNet1d, or its CustomTransformer behind "
                                      f"DDIMTransformerAdapter); the network is {type(self.model).__name__}")
        if self.pred_type not in N.PRED_TYPES:
            raise ValueError(f"Unknown pred_type: {self.pred_type}")
        B, RT, MZ = x_0.shape
        c2, c1 = _f32(ms2_cond), _f32(net._check_inputs(ms1_cond, B, RT))
        x_0, t, noise, ab, lw = self._stage_step(x_0, t, noise)
        flat = net.read_params()  # (the averaged weights inside ModelInterface.ema_scope())
        ws = net.workspace(B, RT, False)
        loss = torch.empty((), dtype=torch.float32, device=x_0.device)
        per_window = torch.empty(B, dtype=torch.float32, device=x_0.device)
        N.check(N.lib().dq_eval_step(net._plan, N.ptr(flat), N.ptr(net.rope_freqs()), N.ptr(ab), N.ptr(x_0), N.ptr(c2), N.ptr(c1), N.ptr(t),
                                     N.ptr(noise), 1 if self.auto_normalize else 0, N.PRED_TYPES[self.pred_type], N.ptr(lw), N.ptr(loss),
                                     N.ptr(per_window), N.ptr(ws), ws.numel(), B, RT, N.stream_ptr()), "dq_eval_step")
        return loss, per_window

    @torch.no_grad()
    def eval_steps(self, x_0, ms2_cond, ms1_cond, t, seed_dev, window_ids_dev, first_draw=0):
        """``eval_step`` for R repeats of one batch: ``t`` (R, B), repeat r under the noise ``dq_randn(seed, window id, draw = first_draw +
        r)``.  Returns ``(loss (R), per_window (R, B))`` as device tensors.  The CustomTransformer behind its adapter takes all repeats in
        one native call (``dq_tfm_eval_step``: one stacked forward, the noise drawn inside its kernels and never materialised); UNet1d one
        ``eval_step`` per repeat on ``evaluation.window_noise``.  Native network only."""
        from . import evaluation as E

        if not (self.native or self._native_tfm):
            raise NotImplementedError("eval_steps runs in the native library only (this package's UNet1d, or its CustomTransformer behind "
                                      f"DDIMTransformerAdapter); the network is {type(self.model).__name__}")
        t = torch.as_tensor(t)
        if t.dim() != 2 or t.shape[1] != x_0.shape[0]:
            raise ValueError(f"eval_steps: t must be (repeats, batch = {x_0.shape[0]}), got {tuple(t.shape)}")
        if self._native_tfm:
            return self._eval_steps_tfm(x_0, ms1_cond, t, seed_dev=seed_dev, window_ids_dev=window_ids_dev, first_draw=int(first_draw))
        losses, per_window = [], []
        for k in range(t.shape[0]):
            noise = E.window_noise(seed_dev, window_ids_dev, int(first_draw) + k, x_0.shape)
            loss, pw = self.eval_step(x_0, ms2_cond, ms1_cond, t=t[k].to(x_0.device), noise=noise)
            losses.append(loss)
            per_window.append(pw)
        return torch.stack(losses), torch.stack(per_window)

    def _eval_steps_tfm(self, x_0, ms1_cond, t, noise=None, seed_dev=None, window_ids_dev=None, first_draw=0):
        """``dq_tfm_eval_step``: ``t`` (R, B); ``noise`` (R, B, S1, D) as passed, or None: drawn in the kernels from ``seed_dev`` /
        ``window_ids_dev`` at draw index ``first_draw + r``."""
        if self.pred_type not in N.PRED_TYPES:
            raise ValueError(f"Unknown pred_type: {self.pred_type}")
        tfm = self.model.transformer
        if not x_0.is_cuda:
            raise RuntimeError("CustomTransformer (MI355X build): tensors must live on the GPU; there is no CPU fallback")
        c1, B, S1, S2, _ = self._stage_tfm(tfm, ms1_cond, "eval_step", "x_0", x_0.shape)
        if t.dim() != 2 or t.shape[1] != B:
            raise ValueError(f"eval_step: t must be (repeats, batch = {B}), got {tuple(t.shape)}")
        x_0, t, noise, ab, lw = self._stage_step(x_0, t, noise, draw_noise=False)
        dev, R = x_0.device, t.shape[0]
        if noise is not None:
            if noise.numel() != R * x_0.numel():
                raise ValueError("eval_step: noise must have the shape of x_0 per repeat")
        elif seed_dev is None:
            raise ValueError("eval_steps: the noise is drawn from seed_dev (an int64 device tensor, DDIMDiffusionModel._seed_tensor)")
        flat = tfm.read_params(False)  # (the averaged weights inside ModelInterface.ema_scope())
        ws = tfm.eval_workspace(B, S1, S2, R)
        sin, cos, freqs = tfm.tables(max(S1, S2), dev)
        loss = torch.empty(R, dtype=torch.float32, device=dev)
        per_window = torch.empty(R, B, dtype=torch.float32, device=dev)
        N.check(N.lib().dq_tfm_eval_step(tfm._tfm, N.ptr(flat), N.ptr(sin), N.ptr(cos), N.ptr(freqs), N.ptr(ab), N.ptr(x_0), N.ptr(c1), N.ptr(t),
                                         N.ptr(noise), N.ptr(seed_dev), N.ptr(window_ids_dev), int(first_draw), 1 if self.auto_normalize else 0,
                                         N.PRED_TYPES[self.pred_type], N.ptr(lw), N.ptr(loss), N.ptr(per_window), None, N.ptr(ws), ws.numel(),
                                         B, S1, S2, R, N.stream_ptr()), "dq_tfm_eval_step")
        return loss, per_window

    def _train_step_fused_tfm(self, x_0, ms1_cond, t=None, noise=None, zero_grads=True, ms1_loss_weight=0.0):
        """train_step for the CustomTransformer behind its adapter: the same sequence as the U-Net's dq_train_step (normalise +
        q_sample, network forward, MSE and its gradient, network backward into the flat gradient buffer), each stage one native
        call -- dq_q_sample, dq_tfm_fwd, dq_mse_loss(_weighted)_fwd_bwd, dq_tfm_bwd -- issued back to back on the current stream."""
        tfm = self.model.transformer
        c1, B, _, _, _ = self._stage_tfm(tfm, ms1_cond, "train_step_fused", "x_0", x_0.shape)
        x_0, t, noise, ab, lw = self._stage_step(x_0, t, noise)
        per, dev = x_0[0].numel(), x_0.device
        norm = 1 if self.auto_normalize else 0
        lib = N.lib()
        x_t = torch.empty_like(x_0)
        N.check(lib.dq_q_sample(N.ptr(ab), N.ptr(x_0), N.ptr(t), N.ptr(noise), N.ptr(x_t), B, per, norm, N.stream_ptr()),
                "dq_q_sample")
        c1n = self.normalize(c1).contiguous()  # (B, RT) values: the only torch op of the step
        tfm._ensure_flat()
        out = tfm._run_fwd(x_t, t, c1n, training=True)
        grads = tfm.flat_grads(zero=False)  # zero_grads: the backward below overwrites instead of accumulating
        loss = torch.empty((), dtype=torch.float32, device=dev)
        dout = torch.empty_like(out)
        if getattr(self, "_mse_scratch", None) is None or self._mse_scratch.device != dev:
            self._mse_scratch = torch.empty(4096, dtype=torch.float32, device=dev)
        if self.pred_type == "eps":
            N.check(lib.dq_mse_loss_fwd_bwd(N.ptr(out), N.ptr(noise), N.ptr(loss), N.ptr(dout), N.ptr(self._mse_scratch), out.numel(),
                                            N.stream_ptr()), "dq_mse_loss_fwd_bwd")
        else:
            N.check(lib.dq_mse_loss_weighted_fwd_bwd(N.ptr(out), N.ptr(x_0), 2.0 if norm else 1.0, -1.0 if norm else 0.0, N.ptr(lw), N.ptr(t),
                                                     N.ptr(loss), N.ptr(dout), N.ptr(self._mse_scratch), B, per, N.stream_ptr()),
                    "dq_mse_loss_weighted_fwd_bwd")
        if ms1_loss_weight > 0.0:  # the MS1 term on top of the MSE part (same kernels as the U-Net's train step)
            B_, RT_, MZ_ = x_0.shape
            sc = torch.empty(5 * B_ * RT_ + B_ + 64, dtype=torch.float32, device=dev)
            lwp = N.ptr(lw) if self.pred_type == "x0" else None
            N.check(lib.dq_ms1_loss_fwd_bwd(N.ptr(out), N.ptr(x_t) if self.pred_type == "eps" else None, N.ptr(c1), 2.0 if norm else 1.0,
                                            -1.0 if norm else 0.0, lwp, N.ptr(t), float(ms1_loss_weight), N.ptr(loss), N.ptr(dout), N.ptr(sc),
                                            B_, RT_, MZ_, N.stream_ptr()), "dq_ms1_loss_fwd_bwd")
        if zero_grads and torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            # data parallel: each layer's gradient slice is all-reduced while the layers below it are still in backward
            red = BucketedAllReduce(grads)
            tfm._run_bwd(x_t, c1n, dout, grads, False, False, accumulate=False, on_bucket=red.on_bucket)
            red.finish()
            self._grads_reduced = True  # tells _train_one_batch to skip its flat all-reduce
        else:
            tfm._run_bwd(x_t, c1n, dout, grads, False, False, accumulate=not zero_grads)
        return loss
