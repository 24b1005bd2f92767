"""Drop-in façade for the reference's sampling surface.

``ClassifierFreeDiffRoll`` keeps the constructor keywords, ``hparams`` attribute access, method
names, argument meaning, return conventions and error behaviour of the reference class
(model/diffwave.py:579-686 on top of task/diffusion.py:219-256, :513-538, :765-790, :831-853,
:943-1025), but every tensor operation runs in the HIP engine (diffroll_amd/csrc) through the
C-ABI.  The torch modules created in the constructor are only PARAMETER CONTAINERS, so that a
reference ``state_dict`` / Lightning checkpoint loads by name; they are never called.

What is deliberately different from the reference:
  * the mel front-end and the conditioner projections are computed once per clip, not twice per
    step; the step-embedding MLP is a table built at load time;
  * nothing is copied to the host inside the loop (task/diffusion.py:530) - ``predict_step`` /
    ``sampling`` return device tensors; figures / gif / MIDI side effects are not produced;
  * classifier-free guidance evaluates the conditional and unconditional branch as one 2B batch.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from .engine import Engine
from .ensemble import aggregate, check_draws
from .schedule import respaced_steps, sampling_options

_SAMPLERS = ("ddpm_x0", "cfdg_ddpm_x0", "generation_ddpm_x0", "inpainting_ddpm_x0",
             "ddim_x0", "cfdg_ddim_x0", "ddpm", "ddim", "ddim2ddpm")
_GUIDED = ("cfdg_ddpm_x0", "inpainting_ddpm_x0", "cfdg_ddim_x0")


def _trimmed_frames(sampler: str, condition: str, T: int, spec_frames: Optional[int]) -> int:
    """Frames left of a T-frame roll by trim_spec_roll (model/diffwave.py:30-39, :662): the spectrogram's length when that is
    shorter - the clip's spec_frames = L // hop + 1 (None: no waveform), or the 641 frames of the learned unconditional
    spectrogram that generation runs on under condition='trainable_spec' (model/diffwave.py:656-660)."""
    if sampler == "generation_ddpm_x0" and condition == "trainable_spec":
        return min(T, 641)
    return T if spec_frames is None else min(T, spec_frames)


class AttrDict(dict):
    """hparams-style attribute access (``self.hparams.sampling.w``)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


def _attr(obj):
    if isinstance(obj, dict):
        return AttrDict({k: _attr(v) for k, v in obj.items()})
    if hasattr(obj, "items") and not isinstance(obj, (str, bytes)):   # OmegaConf DictConfig & friends
        try:
            return AttrDict({k: _attr(v) for k, v in obj.items()})
        except Exception:
            return obj
    return obj


def _conv1d(cin, cout, k):
    layer = nn.Conv1d(cin, cout, k)
    nn.init.kaiming_normal_(layer.weight)        # model/diffwave.py:41-44
    return layer


class _DiffusionEmbedding(nn.Module):            # parameter container for model/diffwave.py:58-63
    def __init__(self):
        super().__init__()
        self.projection1 = nn.Linear(128, 512)
        self.projection2 = nn.Linear(512, 512)


class _ResidualBlock(nn.Module):                 # parameter container for model/diffwave.py:108-132
    def __init__(self, n_mels, residual_channels, kernel_size):
        super().__init__()
        self.dilated_conv = _conv1d(residual_channels, 2 * residual_channels, kernel_size)
        self.diffusion_projection = nn.Linear(512, residual_channels)
        self.conditioner_projection = _conv1d(n_mels, 2 * residual_channels, 1)
        self.output_projection = _conv1d(residual_channels, 2 * residual_channels, 1)


class ClassifierFreeDiffRoll(nn.Module):
    def __init__(self,
                 residual_channels,
                 unconditional,
                 condition,
                 n_mels,
                 norm_args,
                 residual_layers=30,
                 kernel_size=3,
                 dilation_base=1,
                 dilation_bound=4,
                 spec_args={},
                 spec_dropout=0.5,
                 inpainting_t=None,
                 inpainting_f=None,
                 # SpecRollDiffusion (task/diffusion.py:220-232)
                 lr=1e-4,
                 timesteps=200,
                 loss_type="l2",
                 loss_keys=("diffusion_loss",),
                 beta_start=1e-4,
                 beta_end=0.02,
                 frame_threshold=0.5,
                 training=None,
                 sampling=None,
                 debug=False,
                 generation_filter=0.0,
                 device=None,
                 precision="f32",
                 beta_schedule="linear",
                 accumulation="auto"):
        super().__init__()
        if condition not in ("fixed", "trainable_spec"):
            if condition == "trainable_z":
                raise NotImplementedError(
                    "condition='trainable_z' cannot be constructed in the reference either (model/diffwave.py:619 "
                    "passes kernel_size into ResidualBlockz's `uncond`; SURVEY.md Appendix B)")
            raise ValueError(f"unrecognized condition '{condition}'")        # model/diffwave.py:610
        if unconditional:
            raise NotImplementedError("unconditional=True cannot run in the reference either: forward() still passes the "
                                      "spectrogram to blocks built without a conditioner and trips the assertion at "
                                      "model/diffwave.py:135-136")
        if len(norm_args) < 3 or norm_args[2] not in ("imagewise", "framewise"):
            raise ValueError(f"norm_args[2] must be 'imagewise' or 'framewise' (model/utils.py:10-35), got {norm_args!r}")
        sampling = _attr(sampling if sampling is not None else {"type": "cfdg_ddpm_x0", "w": 0.0})
        training = _attr(training if training is not None else {"mode": "x_0"})
        spec_args = _attr(dict(spec_args))
        if sampling.type not in _SAMPLERS:
            raise AttributeError(sampling.type)                               # getattr at task/diffusion.py:255
        # extensions, absent / None in the reference's configs (each key, its validator and the engine option it becomes:
        # schedule.sampling_options): steps, draws, guidance_interval, solver_order, solver_noise, start_step / strength,
        # x0_clip, x0_threshold, cfg_rescale, cfg_project, cfg_norm, cfg_momentum, guidance_stride, exact_below
        sampling_options(sampling, timesteps, norm_args)
        self.hparams = AttrDict(
            residual_channels=residual_channels, unconditional=unconditional, condition=condition,
            n_mels=n_mels, norm_args=list(norm_args), residual_layers=residual_layers,
            kernel_size=kernel_size, dilation_base=dilation_base, dilation_bound=dilation_bound,
            spec_args=spec_args, spec_dropout=spec_dropout, inpainting_t=inpainting_t,
            inpainting_f=inpainting_f, lr=lr, timesteps=timesteps, loss_type=loss_type,
            loss_keys=list(loss_keys), beta_start=beta_start, beta_end=beta_end,
            frame_threshold=frame_threshold, training=training, sampling=sampling, debug=debug,
            generation_filter=generation_filter, beta_schedule=beta_schedule)
        if beta_schedule not in ("linear", "cosine", "quadratic", "sigmoid"):
            raise ValueError(f"unknown beta_schedule '{beta_schedule}'")
        self.spec_dropout = spec_dropout

        if condition == "trainable_spec":                                    # model/diffwave.py:600-604
            self.trainable_parameters = nn.Parameter(torch.full((int(spec_args.get("n_mels", n_mels)), 641), -1.0))
        # parameter containers, same names/shapes/initialisation as the reference
        self.input_projection = _conv1d(88, residual_channels, 1)
        self.diffusion_embedding = _DiffusionEmbedding()
        self.residual_layers = nn.ModuleList(
            [_ResidualBlock(n_mels, residual_channels, kernel_size) for _ in range(residual_layers)])
        self.skip_projection = _conv1d(residual_channels, residual_channels, 1)
        self.output_projection = _conv1d(residual_channels, 88, 1)
        nn.init.zeros_(self.output_projection.weight)                         # model/diffwave.py:630
        for p in self.parameters():
            p.requires_grad_(False)

        sa = spec_args
        self._engine_kwargs = dict(
            residual_channels=residual_channels, residual_layers=residual_layers,
            kernel_size=kernel_size, dilation_base=dilation_base, dilation_bound=dilation_bound,
            n_mels=n_mels, timesteps=timesteps, beta_start=beta_start, beta_end=beta_end,
            sample_rate=int(sa.get("sample_rate", 16000)), n_fft=int(sa.get("n_fft", 2048)),
            hop_length=int(sa.get("hop_length", 512)), f_min=float(sa.get("f_min", 0.0)),
            f_max=float(sa.get("f_max", 8000.0)))
        # The front-end kernels implement config/spec/mel.yaml: center=True and normalized=True.  torchaudio's own
        # default for `normalized` is False, so a spec_args without the key would build a DIFFERENT front-end in the
        # reference (log(x + 1e-6) then min-max does not cancel the window scale): the key must be present and true.
        if not sa.get("center", True):
            raise NotImplementedError("spec_args.center=False is not supported (config/spec/mel.yaml)")
        if "normalized" not in sa:
            raise NotImplementedError("spec_args.normalized is required and must be True (config/spec/mel.yaml:10): "
                                      "torchaudio's default is False, which this front-end does not implement")
        if not sa["normalized"]:
            raise NotImplementedError("spec_args.normalized=False is not supported (config/spec/mel.yaml)")
        # the remaining keys default to config/spec/mel.yaml's values (n_fft 2048, hop 512, f_max 8000, sr 16000),
        # NOT to torchaudio's (400 / 200 / sr/2): the engine is built for the released configuration
        if sa.get("pad_mode", "reflect") != "reflect":
            raise NotImplementedError("only pad_mode='reflect' is supported (config/spec/mel.yaml)")
        # every other torchaudio MelSpectrogram argument must be at the value the front-end kernels implement
        # (torchaudio 0.11 defaults) - nothing is silently ignored
        fixed = {"win_length": (None, int(sa.get("n_fft", 2048))), "power": (2.0, 2), "mel_scale": ("htk",),
                 "norm": (None,), "onesided": (True,), "pad": (0,), "window_fn": (torch.hann_window,),
                 "wkwargs": (None,)}
        known = {"sample_rate", "n_fft", "hop_length", "n_mels", "f_min", "f_max", "center", "normalized", "pad_mode"}
        for key, val in sa.items():
            if key in known:
                continue
            if key not in fixed:
                raise TypeError(f"spec_args: unknown MelSpectrogram argument '{key}'")
            if val not in fixed[key]:
                raise NotImplementedError(f"spec_args.{key}={val!r} is not supported (front-end implements {fixed[key][0]!r})")
        if int(sa.get("n_mels", n_mels)) != int(n_mels):
            raise ValueError(f"spec_args.n_mels={sa.get('n_mels')} differs from n_mels={n_mels} (the conditioner's input width)")
        self._device = device
        self.precision = precision          # 'f32' (exact, default) | 'bf16x3' (opt-in split precision) | 'bf16' | 'f16' (opt-in, one pass)
        # accumulation order of the dilated conv (an extension): 'auto' = 'blocked' = one fp32 chain per
        # 32-channel chunk, chunk sums added up separately - like a CPU library's K-blocked GEMM - in every flavour;
        # 'single_chain' = 128-frame blocks (16 guided clips per GPU) and the 96 / 160-frame flavours (640-frame rolls) contract
        # all of K as one chain, the rounds 1-3 numerics: 0.2-0.8 % faster, 2-3x the rounding error against float64
        if accumulation not in ("auto", "blocked", "single_chain"):
            raise ValueError("accumulation is 'auto', 'blocked' or 'single_chain'")
        self.accumulation = accumulation
        self._engine: Optional[Engine] = None
        self._dirty = True
        self._fe_key = None
        self._fe_spec = None
        self.reverse_diffusion = getattr(self, sampling.type)                  # task/diffusion.py:255

    # ------------------------------------------------------------------ plumbing
    def _betas(self):
        """None for the reference's linear schedule (task/diffusion.py:239), else one of the model/unet.py:558-579
        schedules (an extension: `beta_schedule=` is not a reference kwarg)."""
        from . import schedule as S
        kind = self.__dict__["hparams"].get("beta_schedule", "linear")
        if kind == "linear":
            return None
        return {"cosine": S.cosine_beta_schedule, "quadratic": S.quadratic_beta_schedule,
                "sigmoid": S.sigmoid_beta_schedule}[kind](self.__dict__["hparams"].timesteps)

    @property
    def engine(self) -> Engine:
        options = self.sampling_options()                 # (a bad value raises here: before any GPU work)
        if self._engine is None:
            self._engine = Engine(device=self._device, betas=self._betas(), norm_mode=str(self.hparams.norm_args[2]),
                                  fe_window=self.__dict__.get("_ckpt_window"), fe_fb=self.__dict__.get("_ckpt_fb"),
                                  **self._engine_kwargs)
            self._dirty = True
        if self._dirty:
            self._engine.load_params({k: v for k, v in self.state_dict().items()})
            self._dirty = False
            self._fe_key = None
        if self._engine.precision != self.precision:
            self._engine.set_precision(self.precision)
        want = 1 if self.accumulation == "single_chain" else 2
        if self._engine.blocked_accumulation != want:
            self._engine.set_option("blocked_accumulation", want)
        # (a change of "sampling_steps" drops the engine's captured chain; the others are part of its key: nothing is dropped)
        for name, value in options.items():
            if name == "draws" or getattr(self._engine, name) == value:      # ("draws" is set around the calls that sample them)
                continue
            if name == "guidance_interval":
                self._engine.set_guidance_interval(*value)
            else:
                self._engine.set_option(name, value)
        return self._engine

    def start_configured(self):
        """The hparams.sampling key that starts chains at an intermediate step - 'start_step' or 'strength' - or None."""
        sampling = self.__dict__["hparams"].sampling
        return next((k for k in ("start_step", "strength") if sampling.get(k) is not None), None)

    def sampling_options(self) -> Dict[str, Any]:
        """hparams.sampling as the engine's options take it, by option name (schedule.sampling_options).  Read at every use; a
        bad value raises ValueError before any GPU work.  While one of the reference's single-step methods runs, the options
        that shape the chain's steps and updates read as off; which steps guide, how many rolls a clip gets and which steps
        run in exact fp32 stay."""
        hp = self.__dict__["hparams"]
        options = sampling_options(hp.sampling, hp.timesteps, hp.norm_args)
        if self.__dict__.get("_stride1"):
            off = sampling_options({}, hp.timesteps)
            options = {k: v if k in ("guidance_interval", "draws", "exact_below") else off[k] for k, v in options.items()}
        return options

    def start_step(self) -> int:
        """hparams.sampling.start_step / .strength as option "start_step" takes them (-1: the chain's first step)."""
        return self.sampling_options()["start_step"]

    def solver_order(self) -> int:
        """hparams.sampling.solver_order as the engine's option takes it (0: the sampler's own update)."""
        return self.sampling_options()["solver_order"]

    def solver_noise(self) -> int:
        """hparams.sampling.solver_noise as the engine's option takes it (0: the deterministic solver)."""
        return self.sampling_options()["solver_noise"]

    def x0_clip(self) -> int:
        """hparams.sampling.x0_clip as the engine's option takes it (0: off, 1: the range (0, 1) of hparams.norm_args, 2: (-1, 1))."""
        return self.sampling_options()["x0_clip"]

    def x0_threshold(self) -> int:
        """hparams.sampling.x0_threshold as the engine's option takes it (0: off, else the percentile in units of 1 / 10000)."""
        return self.sampling_options()["x0_threshold"]

    def cfg_rescale(self) -> int:
        """hparams.sampling.cfg_rescale as the engine's option takes it (0: off, else phi in units of 1 / 10000)."""
        return self.sampling_options()["cfg_rescale"]

    def cfg_project(self) -> int:
        """hparams.sampling.cfg_project as the engine's option takes it (0: off, else rho in units of 1 / 10000)."""
        return self.sampling_options()["cfg_project"]

    def cfg_norm(self) -> int:
        """hparams.sampling.cfg_norm as the engine's option takes it (0: off, else the rms bound r in units of 1 / 10000)."""
        return self.sampling_options()["cfg_norm"]

    def cfg_momentum(self) -> int:
        """hparams.sampling.cfg_momentum as the engine's option takes it (0: off, else the momentum beta in units of 1 / 10000)."""
        return self.sampling_options()["cfg_momentum"]

    def guidance_stride(self) -> int:
        """hparams.sampling.guidance_stride as the engine's option takes it (0: off, else the stride n of the steps that refresh)."""
        return self.sampling_options()["guidance_stride"]

    def exact_below(self) -> int:
        """hparams.sampling.exact_below as the engine's option takes it (0: off, else v: the steps t < v run in exact fp32)."""
        return self.sampling_options()["exact_below"]

    def guidance_interval(self):
        """(lo, hi) of hparams.sampling.guidance_interval as the engine's options take them; (0, -1): the whole chain."""
        return self.sampling_options()["guidance_interval"]

    def sampling_steps(self) -> int:
        """n of hparams.sampling.steps (0: every step)."""
        return self.sampling_options()["sampling_steps"]

    def draws(self) -> int:
        """D of hparams.sampling.draws: the rolls predict_step / sampling / test_step sample per clip (1: one)."""
        return self.sampling_options()["draws"]

    def visited_steps(self):
        """The diffusion steps sample() visits, in chain order (timesteps-1 .. 0, or hparams.sampling.steps of them)."""
        return respaced_steps(int(self.hparams.timesteps), self.sampling_steps())

    # schedule vectors, exposed like the reference's attributes (task/diffusion.py:239-256)
    def __getattr__(self, name):
        if name in ("betas", "alphas", "sqrt_recip_alphas", "sqrt_alphas_cumprod",
                    "sqrt_one_minus_alphas_cumprod", "posterior_variance"):
            from .schedule import make_schedule
            hp = self.__dict__["hparams"]
            return make_schedule(hp.beta_start, hp.beta_end, hp.timesteps, self._betas())[name]
        return super().__getattr__(name)

    def load_state_dict(self, state_dict, strict: bool = True):
        own = {k: v for k, v in state_dict.items()
               if not k.startswith("mel_layer.") and k != "diffusion_embedding.embedding"}
        out = super().load_state_dict(own, strict=strict)
        # the MelSpectrogram buffers of a reference checkpoint (torchaudio 0.11 names) are the front-end tables
        # themselves: use them (they equal diffroll_amd.frontend_tables' output, which is what runs without them)
        win, fb = state_dict.get("mel_layer.spectrogram.window"), state_dict.get("mel_layer.mel_scale.fb")
        n_fft, n_mels = self._engine_kwargs["n_fft"], self._engine_kwargs["n_mels"]
        changed = False
        if win is not None and tuple(win.shape) == (n_fft,):
            self.__dict__["_ckpt_window"] = win.detach().float().cpu()
            changed = True
        if fb is not None and tuple(fb.shape) == (n_fft // 2 + 1, n_mels):
            self.__dict__["_ckpt_fb"] = fb.detach().float().cpu()
            changed = True
        if changed and self._engine is not None:          # tables are fixed at engine creation: rebuild lazily
            self._engine.close()
            self._engine = None
        self._dirty = True
        return out

    def to(self, *args, **kwargs):           # parameters stay on the host; the engine owns device copies
        for a in args:
            if isinstance(a, (str, torch.device)) and torch.device(a).type == "cuda":
                self._device = torch.device(a)
        if "device" in kwargs and torch.device(kwargs["device"]).type == "cuda":
            self._device = torch.device(kwargs["device"])
        return self

    def cuda(self, device=None):
        self._device = torch.device("cuda", device if device is not None else torch.cuda.current_device())
        return self

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, trust=False, **overrides):
        """Lightning-style: ``{'state_dict', 'hyper_parameters'}``; keyword overrides win
        (sampling.py:54-65).  OmegaConf containers inside a real reference checkpoint are read without
        omegaconf / pytorch_lightning installed, and without executing anything the file names: an allow-listing
        unpickler (diffroll_amd/checkpoint.py); ``trust=True`` = the full unpickle Lightning itself does."""
        from .checkpoint import constructor_kwargs, load_checkpoint
        ckpt = load_checkpoint(checkpoint_path, trust=trust)
        m = cls(**constructor_kwargs(cls, ckpt["hyper_parameters"], overrides))
        m.load_state_dict(ckpt["state_dict"], strict=False)
        return m

    # ------------------------------------------------------------------ forward
    def _frontend(self, waveform: torch.Tensor, T_roll: int, inpainting_t, inpainting_f) -> torch.Tensor:
        eng = self.engine
        try:
            version = waveform._version
        except Exception:                      # inference-mode tensors do not track a version: never cached
            version = None
        key = (waveform.data_ptr(), tuple(waveform.shape), version, T_roll,
               tuple(inpainting_t) if inpainting_t else None, tuple(inpainting_f) if inpainting_f else None)
        if version is None or key != self._fe_key:
            self._fe_spec = eng.frontend(waveform, T_roll, inpainting_t, inpainting_f)
            self._fe_key = key
            self._fe_wave = waveform    # keep alive so data_ptr cannot be recycled
        return self._fe_spec

    def forward(self, x_t, waveform, diffusion_step, sampling=False, inpainting_t=None, inpainting_f=None):
        """(x_t (B,1,T,88), waveform (B,L), diffusion_step (B,) int) -> (x0_pred (B,1,T,88), spec (B,n_mels,T'))
        with T' = min(T, L//hop + 1) (model/diffwave.py:637-686, eval mode)."""
        eng = self.engine
        if diffusion_step.dtype not in (torch.int32, torch.int64):
            raise NotImplementedError("fractional diffusion steps (lerp branch, model/diffwave.py:76-81) are off-path")
        steps = [int(v) for v in diffusion_step.flatten().tolist()]
        B, _, T, K = x_t.shape
        if len(steps) != B:
            raise ValueError(f"diffusion_step has {len(steps)} entries for a batch of {B}")
        t = steps[0]
        uniform = all(v == t for v in steps)      # the samplers' case (task/diffusion.py:947)
        if sampling is True:                       # the unconditional evaluation: what generation_ddpm_x0 runs on
            spec, Tm = self._conditioning("generation_ddpm_x0", T, waveform, B)
        else:
            spec = self._frontend(waveform, T, inpainting_t, inpainting_f)
            Tm = spec.shape[-1]
        x = x_t.to(eng.device, torch.float32).squeeze(1)[:, :Tm, :].contiguous()
        if uniform:
            x0 = self._verified(lambda: eng.forward(x, t, uncond=(sampling is True)))
        else:                                      # one step per sample, as the reference's step() calls forward
            x0 = self._verified(lambda: eng.forward_steps(x, steps, uncond=(sampling is True)))
        return x0.unsqueeze(1), spec

    def _verified(self, fn):
        """Run fn (engine launches returning a result tensor) and hand the result out only after engine.finish() has
        confirmed that no fused launch timed out; after a time-out (healed by finish(): per-phase launches from then
        on) it is recomputed once.  The reference's methods return finished tensors - never silently invalid ones."""
        from .engine import EngineTimeout
        eng = self.engine
        try:
            out = fn()
            eng.finish()
            return out
        except EngineTimeout:
            try:                   # (a time-out left pending by earlier unchecked calls is cleared here)
                eng.finish()
            except EngineTimeout:
                pass
            out = fn()
            eng.finish()
            return out

    # ------------------------------------------------------------------ samplers (one step)
    def _conditioning(self, sampler: str, T: int, waveform, n: int):
        """(spec, Tm): the spectrogram a call on n clips is conditioned on, and the frames its T-frame rolls are trimmed to.
        The conditional samplers run the front-end (cached per waveform; the inpainting masks for inpainting_ddpm_x0 only);
        generation_ddpm_x0 runs on the spectrogram of its sampling=True forward (task/diffusion.py:979-997): -1 everywhere,
        or the learned one - 2-D, 641 frames - under condition='trainable_spec' (model/diffwave.py:656-660)."""
        if sampler != "generation_ddpm_x0":
            masked = sampler == "inpainting_ddpm_x0"
            spec = self._frontend(waveform, T, self.hparams.inpainting_t if masked else None,
                                  self.hparams.inpainting_f if masked else None)
            return spec, spec.shape[-1]
        eng = self.engine
        Tm = _trimmed_frames(sampler, self.hparams.condition, T,
                             None if waveform is None else waveform.shape[-1] // eng.hop_length + 1)
        if self.hparams.condition == "trainable_spec":
            return self.trainable_parameters.detach()[:, :Tm].to(eng.device, torch.float32), Tm
        return torch.full((n, eng.n_mels, Tm), -1.0, device=eng.device), Tm

    def _guidance_weight(self, sampler: str) -> float:
        """hparams.sampling.w for the samplers that guide, 0 for the others."""
        return float(self.hparams.sampling.get("w", 0.0)) if sampler in _GUIDED else 0.0

    def _one_step(self, sampler: str, x, waveform, t_index: int, noise=None, respaced=False, philox=None):
        """One dr_step.  The reference's single-step methods keep their stride-1 meaning (t -> t - 1) whatever
        hparams.sampling.steps says (the option is off while they run: under a respaced config that costs the engine its
        captured chain); respaced=True (sample_trajectory) takes the respaced chain's step.
        The step's z is `noise` where that is a tensor; else the engine's Philox draws for philox = (seed, first_sample), keyed
        as sample() keys them; else drawn here from torch's global generator when t > 0, as the reference's randn_like."""
        prev = self.__dict__.get("_stride1", False)
        self.__dict__["_stride1"] = not respaced
        try:
            eng = self.engine
            B, _, T, _ = x.shape
            spec, Tm = self._conditioning(sampler, T, waveform, B)
            x_in = x.to(eng.device, torch.float32).squeeze(1)[:, :Tm, :].contiguous()
            z, key = None, (0, 0)
            if noise is not None:
                z = noise.to(eng.device, torch.float32).reshape(B, Tm, 88).contiguous()
            elif philox is not None:
                key = philox
            elif t_index > 0:
                z = torch.randn(B, Tm, 88, device=eng.device)
            w = self._guidance_weight(sampler)
            xx = self._verified(lambda: eng.step(sampler, x_in.clone(), z, t_index, w, *key))
            return xx.unsqueeze(1), spec
        finally:
            self.__dict__["_stride1"] = prev

    def ddpm_x0(self, x, waveform, t_index, noise=None):
        """task/diffusion.py:831-853."""
        return self._one_step("ddpm_x0", x, waveform, t_index, noise)

    def cfdg_ddpm_x0(self, x, waveform, t_index, noise=None):
        """task/diffusion.py:943-969."""
        return self._one_step("cfdg_ddpm_x0", x, waveform, t_index, noise)

    def generation_ddpm_x0(self, x, waveform, t_index, noise=None):
        """task/diffusion.py:971-997."""
        return self._one_step("generation_ddpm_x0", x, waveform, t_index, noise)

    def inpainting_ddpm_x0(self, x, waveform, t_index, noise=None):
        """task/diffusion.py:999-1025."""
        return self._one_step("inpainting_ddpm_x0", x, waveform, t_index, noise)

    # same kernels, other per-step coefficients
    def ddim_x0(self, x, waveform, t_index, noise=None):
        """task/diffusion.py:855-875 (sigma = 0; `noise` is accepted and ignored, as 0 * randn_like)."""
        return self._one_step("ddim_x0", x, waveform, t_index, noise)

    def cfdg_ddim_x0(self, x, waveform, t_index, noise=None):
        """task/diffusion.py:1027-1055 (second branch: spectrogram of a zero waveform = all 0, not -1)."""
        return self._one_step("cfdg_ddim_x0", x, waveform, t_index, noise)

    def ddpm(self, x, waveform, t_index, noise=None):
        """task/diffusion.py:804-829 (network output interpreted as epsilon)."""
        return self._one_step("ddpm", x, waveform, t_index, noise)

    def ddim(self, x, waveform, t_index, noise=None):
        """task/diffusion.py:877-892 (epsilon prediction, deterministic)."""
        return self._one_step("ddim", x, waveform, t_index, noise)

    def ddim2ddpm(self, x, waveform, t_index, noise=None):
        """task/diffusion.py:894-911 (epsilon prediction)."""
        return self._one_step("ddim2ddpm", x, waveform, t_index, noise)

    # ------------------------------------------------------------------ whole chain
    def output_frames(self, T: int, waveform_samples: Optional[int]) -> int:
        """Frames of the roll sample() returns for a T-frame x_T (trim_spec_roll, model/diffwave.py:30-39, :662): the
        spectrogram's length when that is shorter - the clip's L // hop + 1, or the 641 frames of the learned
        unconditional spectrogram under condition='trainable_spec' for generation."""
        hop = self._engine_kwargs["hop_length"]
        return _trimmed_frames(self.hparams.sampling.type, self.hparams.condition, T,
                               None if waveform_samples is None else waveform_samples // hop + 1)

    @torch.no_grad()
    def sample(self, x_T, waveform=None, noise=None, seed: int = 0, first_sample: int = 0,
               use_graph: bool = True, check: bool = True, draws: int = 1, draw_stride: int = 0,
               init=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """The reverse chain t = timesteps-1 .. 0 (task/diffusion.py:528-534) - or, with hparams.sampling.steps = n,
        the n respaced steps of visited_steps() - on the device with no host round trip.  x_T (B,1,T,88); noise: None
        (on-device Philox keyed by seed, global sample index and step) or (timesteps, B, 1, T, 88) injected z's (row t
        is used at step t >= 1, also in a respaced chain).  With hparams.sampling.solver_order = 1 / 2 (option
        "solver_order": DPM-Solver++ on the x0 prediction) the chain is deterministic: noise and seed are not used - unless
        hparams.sampling.solver_noise = 1 (option "solver_noise": the solver's stochastic form), which draws at every visited
        step t >= 1 the z the ddpm_x0 chain draws there: noise and seed mean what they mean without a solver.
        Returns (roll (B,1,T',88), spec (B,n_mels,T')).
        draws = D > 1 (option "draws" of include/diffroll_amd.h): x_T (D*n,1,T,88) holds D draws of the n clips of waveform
        (n, L), draw-major (row b = draw b // n of clip b % n); the front-end and the conditioner tensors exist once per
        clip.  Returns (rolls (D*n,1,T',88), spec (n,n_mels,T')) - bit for bit the rolls of the waveform tiled D times.
        Philox keys row b by first_sample + b % n + (b // n) * draw_stride (0 = n: the tiled batch's first_sample + b).
        With hparams.sampling.start_step = t_s or .strength = s (options "start_step" / "start_noise") only the visited steps
        t <= t_s run.  init (B,1,T,88): a clean roll in the model's roll space - x_T must then be None; the roll is trimmed
        like x_T and diffused to t_s by the chain's first node (z: row 0 of noise, or Philox keyed as the steps' draws with
        step word timesteps + t_s); without a start configured it is diffused to the chain's first step.  Without init and
        with a start configured, x_T is x AT step t_s (resume: a row of sample_trajectory).
        With hparams.sampling.cfg_project = rho and / or .cfg_norm = r (options "cfg_project" / "cfg_norm": adaptive projected
        guidance) every step that guides removes the share rho of the guidance update's component parallel to the conditional
        prediction and bounds the update's rms by r, per roll; not beside x0_threshold or cfg_rescale.
        With hparams.sampling.cfg_momentum = beta beside either (option "cfg_momentum": the method's momentum, -0.5 in the paper)
        the update a guided step projects and bounds is d + beta m_prev, m_prev the previous guided step's; the chain's first
        guided step starts the state.
        With hparams.sampling.guidance_stride = n (option "guidance_stride", 2 .. 64) only every n-th step that guides - and
        step 0 - runs both evaluations; the others run the conditional one alone and reuse the stored guidance update, y = c + d.
        Not beside x0_threshold, cfg_rescale, cfg_project, cfg_norm or cfg_momentum.
        With hparams.sampling.exact_below = v (option "exact_below", 0 .. timesteps) under a reduced precision ('bf16x3', 'bf16',
        'f16') the steps at diffusion step t < v run in exact fp32 and the others in that precision; v = timesteps is the
        'f32' roll bit for bit; inert under 'f32'.  It combines with every key above.
        check=True (default): the call returns with the FINISHED, verified roll, as task/diffusion.py:528-538 does
        (synchronous; a fused-kernel time-out caused by another tenant of the device is healed by re-running the chain
        on the per-phase kernels - Engine.sample).  check=False: asynchronous; call engine.finish() before use."""
        eng = self.engine
        sampler = self.hparams.sampling.type
        if (init is None) == (x_T is None):
            raise ValueError("pass either x_T (x at the chain's first - or configured start - step) or init= (a clean roll to "
                             "diffuse to it), not " + ("both" if init is not None else "neither"))
        start_noise = 0 if init is None else 1
        if init is not None:
            x_T = init
        B, _, T, _ = x_T.shape
        draws = check_draws(draws)
        if B % draws:
            raise ValueError(f"{'init' if start_noise else 'x_T'} holds {B} rolls: not a whole number of draws = {draws}")
        if draws > 1 and waveform is not None and waveform.shape[0] != B // draws:
            raise ValueError(f"{draws} draws of {B} rolls take the waveform of {B // draws} clips, got {waveform.shape[0]}")
        if sampler != "generation_ddpm_x0" and waveform is None:
            raise ValueError("waveform is required for conditional samplers")
        spec, Tm = self._conditioning(sampler, T, waveform, B // draws)
        # a fresh roll buffer per call: the engine's captured chain runs on its own work buffer, so caller
        # addresses never force a re-capture
        xb = x_T.to(eng.device, torch.float32).squeeze(1)[:, :Tm, :].clone(memory_format=torch.contiguous_format)
        z = None
        if noise is not None:
            S = self.hparams.timesteps
            z = noise.to(eng.device, torch.float32).reshape(S, B, T, 88)
            if Tm != T or not z.is_contiguous():
                z = z[:, :, :Tm, :].contiguous()
        with eng.holding(draws=draws, draw_stride=draw_stride, start_noise=start_noise):
            eng.sample(sampler, xb, z, self._guidance_weight(sampler), seed, first_sample, use_graph, check)
        return xb.unsqueeze(1), spec

    @torch.no_grad()
    def sample_long(self, waveform=None, frames: Optional[int] = None, overlap: int = 160, seed: int = 0,
                    recording: int = 0, x_T=None, noise=None, use_graph: bool = True, check: bool = True,
                    draws: int = 1, init=None, blend=None) -> torch.Tensor:
        """One recording of any length as jointly sampled 640-frame windows (diffroll_amd/longform.py; option
        "window_overlap" of include/diffroll_amd.h): returns the stitched roll (1, 1, T_out, 88) on the device.
        Conditional samplers take waveform (L,) (T_out = ceil(L / hop)); generation_ddpm_x0 takes frames = T_out.
        x_T: (1, 1, T_c, 88) canvas, or None: drawn from torch.Generator().manual_seed(seed) on the host; noise: None
        (Philox keyed by seed, first_sample = recording and the canvas element) or a canvas tensor
        (timesteps, 1, 1, T_c, 88).  Every window is one row of ONE Engine.sample chain (check=True heals).
        draws = D > 1: D draws of the recording in that one chain, as sample_long_batch([waveform], draws=D) - returns
        (D, 1, T_out, 88); x_T (D, 1, T_c, 88), noise (timesteps, D, 1, T_c, 88).
        init: a clean roll of the recording in the shape this method RETURNS, (1, 1, T_out, 88) (or (D, 1, T_out, 88)) - a
        roll it returned can be fed back - instead of x_T: zero-padded to the canvas, a single roll shared by all draws, and
        diffused to the start step of hparams.sampling.start_step / .strength by the chain's first node (sample()).
        blend: what a frame shared by two windows takes of their predictions at every step (option "window_blend",
        longform.check_window_blend): None / "mean" = their mean, "linear" = a cross-fade over the overlap, "nearest" = each
        frame from the window whose centre is nearer."""
        from . import longform
        blend = longform.check_window_blend(blend)
        if check_draws(draws) > 1:
            return self.sample_long_batch(None if waveform is None else [waveform], None if frames is None else [frames],
                                          overlap, seed, recording, None if x_T is None else [x_T],
                                          None if noise is None else [noise], use_graph, check, draws,
                                          None if init is None else [init], blend)[0]
        sampler = self.hparams.sampling.type
        if sampler == "inpainting_ddpm_x0":
            raise ValueError("sample_long does not support inpainting_ddpm_x0: its masks (inpainting_t / inpainting_f) are in "
                             "the coordinates of one 640-frame clip, not of a recording")
        eng = self.engine
        if sampler == "generation_ddpm_x0":
            if frames is None or waveform is not None:
                raise ValueError("generation_ddpm_x0: pass frames= (the roll length), not a waveform")
            batch = longform.plan_batch([int(frames)], None, longform.WINDOW_FRAMES, overlap)
        else:
            if waveform is None or frames is not None:
                raise ValueError(f"{sampler}: pass waveform= (L,), not frames")
            waveform = torch.as_tensor(waveform).to("cpu", torch.float32)
            if waveform.dim() != 1:
                raise ValueError(f"waveform must be one recording (L,), got {tuple(waveform.shape)}")
            batch = longform.plan_batch([waveform.shape[0]], eng.hop_length, longform.WINDOW_FRAMES, overlap)
        plan = batch.plans[0]
        if plan.n > longform.MAX_WINDOWS:
            raise ValueError(f"{plan.n} windows of {plan.T} frames: one chain holds at most {longform.MAX_WINDOWS} "
                             f"(longform.MAX_WINDOWS); split the recording")
        S = int(self.hparams.timesteps)
        if init is not None:
            x_T = self._init_canvases([init], x_T, batch, 1)[0]
        if x_T is None:
            x_T = torch.randn(1, 1, plan.T_c, 88, generator=torch.Generator().manual_seed(int(seed)))
        if tuple(x_T.shape) != (1, 1, plan.T_c, 88):
            raise ValueError(f"x_T must be the canvas (1, 1, {plan.T_c}, 88), got {tuple(x_T.shape)}")
        if noise is not None and noise.numel() != S * plan.T_c * 88:
            raise ValueError(f"noise must be the canvas ({S}, 1, 1, {plan.T_c}, 88), got {tuple(noise.shape)}")
        xb = self._sample_windows(batch, None if waveform is None else [waveform], [x_T], None if noise is None else [noise],
                                  1, seed, recording, use_graph, check, start_noise=0 if init is None else 1, blend=blend)
        return longform.stitch(xb, plan).reshape(1, 1, plan.T_out, 88)

    @staticmethod
    def _init_canvases(init, x_T, batch, D):
        """init= of sample_long / sample_long_batch -> the canvases that take x_T's place: one roll per recording in the shape
        those methods return, (D or 1, 1, T_out, 88), zero-padded to the canvas's T_c frames, a single roll repeated for
        every draw.  The windows gathered from a canvas agree on the frames they share - what the joint chain needs."""
        if x_T is not None:
            raise ValueError("pass either x_T (canvases at the chain's first - or configured start - step) or init= (clean "
                             "rolls to diffuse to it), not both")
        plans = batch.plans
        if len(init) != len(plans) or any(r.dim() != 4 or r.shape[0] not in (1, D) or tuple(r.shape[1:]) != (1, p.T_out, 88)
                                          for r, p in zip(init, plans)):
            raise ValueError(f"init must be one roll ({D} or 1, 1, T_out, 88) per recording, T_out = {[p.T_out for p in plans]}, "
                             f"got {[tuple(r.shape) for r in init]}")
        out = []
        for r, p in zip(init, plans):
            canvas = torch.zeros(D, 1, p.T_c, 88, dtype=torch.float32, device=r.device)
            canvas[:, :, :p.T_out] = r.to(torch.float32)       # (a single roll broadcasts over the draws)
            out.append(canvas)
        return out

    def _sample_windows(self, batch, waveforms, x_T, noise, D, seed, first_recording, use_graph, check, marks=None,
                        start_noise=0, blend=0):
        """The one long-form chain: the recordings of `batch` (longform.plan_batch) as D draws of its windows.  waveforms: one
        (L,) host tensor per recording, or None (generation); x_T / noise: one canvas per recording, (D, 1, T_c, 88) /
        (timesteps, D, 1, T_c, 88), or noise None (Philox); marks: the window_break marks, the plan's unless given.  Options
        "window_overlap", "window_blend" (blend), "window_break", "draws" hold for the chain only.  Returns the window batch (D * n, T, 88) after the
        chain: that of draw 0, then that of draw 1, ... (draw-major).  start_noise = 1: the canvases are clean rolls (option
        "start_noise": diffused to the chain's start step per recording and canvas element)."""
        from . import longform
        eng = self.engine
        sampler = self.hparams.sampling.type
        S = int(self.hparams.timesteps)
        xb = torch.cat([longform.gather_batch([x[d].reshape(p.T_c, 88).to(eng.device, torch.float32)
                                               for x, p in zip(x_T, batch.plans)], batch) for d in range(D)], 0)
        z = None
        if noise is not None:
            z = torch.cat([longform.gather_batch([zr.reshape(S, D, p.T_c, 88)[:, d].to(eng.device, torch.float32)
                                                  for zr, p in zip(noise, batch.plans)], batch) for d in range(D)], 1).contiguous()
        if waveforms is not None:
            eng.frontend(torch.cat([longform.window_audio(wv, p, eng.hop_length) for wv, p in zip(waveforms, batch.plans)]),
                         batch.plans[0].T)
            self._fe_key = None          # the engine's conditioner is the windows' now: sample() recomputes its own
        with eng.holding(window_overlap=batch.plans[0].overlap, window_blend=blend, window_breaks=batch.marks if marks is None else marks,
                         draws=D, draw_stride=0, start_noise=start_noise):
            eng.sample(sampler, xb, z, self._guidance_weight(sampler), seed, first_recording, use_graph, check)
        return xb

    @torch.no_grad()
    def sample_long_batch(self, waveforms=None, frames=None, overlap: int = 160, seed: int = 0, first_recording: int = 0,
                          x_T=None, noise=None, use_graph: bool = True, check: bool = True, draws: int = 1,
                          init=None, blend=None) -> List[torch.Tensor]:
        """Several recordings of any lengths in ONE chain (option "window_break" of include/diffroll_amd.h;
        longform.plan_batch): their windows fill one batch, a window shares frames only with windows of its own
        recording, and recording i draws the noise of first_sample = first_recording + i on its own canvas.  Returns one
        stitched roll (1, 1, T_out_i, 88) per recording; roll i is what sample_long(waveforms[i], seed=seed,
        recording=first_recording + i) returns (bit for bit where both chains take the same kernel flavours).
        waveforms: a sequence of (L_i,) tensors; generation_ddpm_x0 takes frames = a sequence of roll lengths instead.
        x_T / noise: None, or one canvas per recording in sample_long's shapes ((1, 1, T_c_i, 88) /
        (timesteps, 1, 1, T_c_i, 88)); the default x_T of every recording is sample_long's for this seed.
        draws = D > 1 (option "draws"): D draws of every recording in the one chain - the window batch repeats per draw
        over ONE set of conditioner tensors, and draw d is the chain of first_recording + d * (number of recordings) on
        its own canvases.  Returns per recording (D, 1, T_out_i, 88); x_T / noise carry the draws in the canvases' batch
        dimension ((D, 1, T_c_i, 88) / (timesteps, D, 1, T_c_i, 88)); the default x_T are the first D canvases of
        torch.Generator().manual_seed(seed) (draw 0 = the single-draw default).
        init: instead of x_T, one clean roll per recording in the shape this method returns ((D or 1, 1, T_out_i, 88));
        see sample_long.  blend: option "window_blend" for the chain, as in sample_long."""
        from . import longform
        D = check_draws(draws)
        blend = longform.check_window_blend(blend)
        sampler = self.hparams.sampling.type
        if sampler == "inpainting_ddpm_x0":
            raise ValueError("sample_long_batch does not support inpainting_ddpm_x0: its masks (inpainting_t / inpainting_f) "
                             "are in the coordinates of one 640-frame clip, not of a recording")
        eng = self.engine
        if sampler == "generation_ddpm_x0":
            if frames is None or waveforms is not None:
                raise ValueError("generation_ddpm_x0: pass frames= (the roll lengths), not waveforms")
            batch = longform.plan_batch([int(f) for f in frames], None, longform.WINDOW_FRAMES, overlap)
        else:
            if waveforms is None or frames is not None:
                raise ValueError(f"{sampler}: pass waveforms= (a sequence of (L,) recordings), not frames")
            waveforms = [torch.as_tensor(wv).to("cpu", torch.float32) for wv in waveforms]
            for wv in waveforms:
                if wv.dim() != 1:
                    raise ValueError(f"every waveform must be one recording (L,), got {tuple(wv.shape)}")
            batch = longform.plan_batch([wv.shape[0] for wv in waveforms], eng.hop_length, longform.WINDOW_FRAMES, overlap)
        if D * batch.n > longform.MAX_WINDOWS:
            raise ValueError(f"{D * batch.n} windows in {len(batch.plans)} recordings ({D} draw(s)): one chain holds at most "
                             f"{longform.MAX_WINDOWS} (longform.MAX_WINDOWS); use fewer recordings per chain (longform.pack_chains)")
        R, S = len(batch.plans), int(self.hparams.timesteps)
        if init is not None:
            x_T = self._init_canvases(list(init), x_T, batch, D)
        if x_T is None:
            x_T = [torch.randn(D, 1, p.T_c, 88, generator=torch.Generator().manual_seed(int(seed))) for p in batch.plans]
        if len(x_T) != R or any(tuple(x.shape) != (D, 1, p.T_c, 88) for x, p in zip(x_T, batch.plans)):
            raise ValueError(f"x_T must be one canvas ({D}, 1, T_c, 88) per recording, T_c = {[p.T_c for p in batch.plans]}")
        if noise is not None and (len(noise) != R or any(zr.numel() != S * D * p.T_c * 88 for zr, p in zip(noise, batch.plans))):
            raise ValueError(f"noise must be one canvas ({S}, {D}, 1, T_c, 88) per recording, T_c = {[p.T_c for p in batch.plans]}")
        xb = self._sample_windows(batch, waveforms, x_T, noise, D, seed, first_recording, use_graph, check,
                                  start_noise=0 if init is None else 1, blend=blend)
        rolls = longform.stitch_batch(xb.reshape(D, batch.n, longform.WINDOW_FRAMES, 88), batch)
        return [r.reshape(D, 1, p.T_out, 88) for r, p in zip(rolls, batch.plans)]

    def sample_trajectory(self, x_T, waveform=None, noise=None, seed: int = 0, first_sample: int = 0):
        """The same chain, keeping every intermediate roll on the device: returns (trajectory (n, B, 1, T', 88) with
        row i = x after the i-th visited step - n = timesteps (t = timesteps-1-i), or hparams.sampling.steps - and spec).
        This is what the reference's sampling() collects as `noise_list` - on the host, with one D2H copy per step
        (task/diffusion.py:779-788) - for its animation; here it is an opt-in eager loop over dr_step (one launch sequence
        per step, no graph), and the last row equals sample()'s result bit for bit.
        With hparams.sampling.start_step / .strength the rows are those of the visited steps t <= t_s, and x_T is x at t_s."""
        sampler = self.hparams.sampling.type
        x, rows, spec = x_T, [], None
        steps, start = self.visited_steps(), self.start_step()
        for t in steps[steps.index(start) if start >= 0 else 0:]:
            # no noise given: Philox keyed by (seed, global sample, step), the draws of sample(); step 0 takes none
            z = torch.zeros_like(x) if t == 0 else None if noise is None else noise[t]
            x, spec = self._one_step(sampler, x, waveform, t, z, respaced=True, philox=(seed, first_sample))
            rows.append(x)
        return torch.stack(rows, 0), spec

    def predict_step(self, batch, batch_idx=0):
        """batch = (x_T, waveform[, ...]) as built by sampling.py:27-46.  Returns the final roll
        (B,1,T,88) (the reference returns nothing and writes figures/MIDI instead)."""
        noise, waveform = batch[0], batch[1]
        D = self.draws()
        if self.start_configured():
            # a chain that starts at an intermediate step starts FROM a roll: the batch's third element, (B,1,T,88) (one per
            # clip, shared by the draws) - Gaussian x_T is never taken for x at the start step
            init = self._batch_init(batch[2] if len(batch) > 2 else None)
            rolls, _ = self.sample(None, waveform, seed=batch_idx, draws=D, init=init.repeat(D, 1, 1, 1))
            return self._ensemble(rolls, D) if D > 1 else rolls
        if D > 1:      # draw 0 starts from the batch's x_T, the others from host-seeded ones; the mean roll is returned
            more = torch.randn((D - 1) * noise.shape[0], *noise.shape[1:], generator=torch.Generator().manual_seed(int(batch_idx)))
            rolls, _ = self.sample(torch.cat([noise.to("cpu", torch.float32), more], 0), waveform, seed=batch_idx, draws=D)
            return self._ensemble(rolls, D)
        roll, _ = self.sample(noise, waveform, seed=batch_idx)
        return roll

    def _batch_init(self, init):
        if init is None:
            key = self.start_configured()
            raise ValueError(f"hparams.sampling.{key} starts the chain at an intermediate step: the batch must carry the roll to "
                             f"start from (a third element / the key 'init', (B, 1, T, 88)) - x_T is noise, not x at that step")
        return torch.as_tensor(init).to(torch.float32)

    def _ensemble(self, rolls, D):
        """Mean roll of D draws per clip; the per-cell votes and spread stay in self.last_ensemble = (votes, std)."""
        mean, votes, std = aggregate(rolls, D, float(self.hparams.frame_threshold))
        self.__dict__["last_ensemble"] = (votes, std)
        return mean.contiguous()

    @staticmethod
    def frame_metrics(tp: int, fp: int, fn: int) -> Tuple[float, float, float]:
        """precision / recall / F1 from the confusion counts with sklearn's average='binary'
        conventions (0 where a denominator is 0)."""
        p = tp / (tp + fp) if tp + fp > 0 else 0.0
        r = tp / (tp + fn) if tp + fn > 0 else 0.0
        f = 2 * p * r / (p + r) if p + r > 0 else 0.0
        return p, r, f

    def test_step(self, batch, batch_idx=0):
        """Frame-level part of task/diffusion.py:312-428: sample the batch, threshold the final roll at
        hparams.frame_threshold and score it against batch['frame'] exactly as
        sklearn.metrics.precision_recall_fscore_support(label.flatten(), pred.flatten() > thr,
        average='binary') does (:381-383); then the note-level score of :385-410 - notes extracted from the
        prediction and from the label roll (GPU run-length scan), onset-only matching as mir_eval's
        precision_recall_f1_overlap(offset_ratio=None) (diffroll_amd/metrics.py; parity unpinned: mir_eval is
        absent here).  Returns the metrics the reference logs; Test/Note_F1 is the mean over the batch (the
        reference logs it for the samples of batch 0 only, :426)."""
        from . import midi, metrics
        roll, _ = self.sampling(batch, batch_idx)
        label = batch["frame"]
        Tm = roll.shape[2]
        label_dev = label[:, :Tm].to(roll.device, torch.float32).contiguous()
        thr = float(self.hparams.frame_threshold)
        tp, fp, fn = self.engine.frame_counts(roll[:, 0], label_dev, thr)
        p, r, f = self.frame_metrics(tp, fp, fn)
        sa = self.hparams.spec_args
        est = midi.extract_notes_wo_velocity(self.engine, roll, thr)
        ref = midi.extract_notes_wo_velocity(self.engine, label_dev, thr)
        notes = metrics.note_scores(ref, est, int(sa.get("hop_length", 512)), int(sa.get("sample_rate", 16000)))
        note_f1 = float(sum(n[2] for n in notes) / max(len(notes), 1))
        return {"Test/Frame_F1": f, "Test/Frame_precision": p, "Test/Frame_recall": r, "tp": tp, "fp": fp, "fn": fn,
                "Test/Note_F1": note_f1, "note_scores": notes}

    def export_midi(self, roll, path_prefix="raw_midi_", threshold=0.5, reference_timing=False, clean_prefix=None):
        """Post-processing of predict_step (task/diffusion.py:598-618): threshold the final roll (the
        reference uses the function default 0.5 there, not hparams.frame_threshold), extract notes on the
        GPU and write per sample `<path_prefix><i>.mid` (all notes: the reference's raw_midi_{batch}_{i}.mid) and,
        with clean_prefix, `<clean_prefix><i>.mid` without the notes not longer than hparams.generation_filter
        seconds (its clean_midi_e{batch}_{i}.mid).  Note times use the model's hop (512 / 16000 s per frame);
        reference_timing=True reproduces the reference's predict_step instead, which scales by its stale module
        constant HOP_LENGTH = 160 (task/diffusion.py:19,604: every time 3.2x too short, and the duration filter
        applied on that scale)."""
        from . import midi
        sa = self.hparams.spec_args
        hop = 160 if reference_timing else int(sa.get("hop_length", 512))
        return midi.export_midi(self.engine, roll, path_prefix, threshold, hop, int(sa.get("sample_rate", 16000)),
                                float(self.hparams.generation_filter), clean_prefix)

    def sampling(self, batch, batch_idx=0):
        """task/diffusion.py:765-790 with x_T drawn on the device; returns (roll, spec).  Two optional batch entries
        (an extension; the reference draws both from torch's global generator, :775 and :967) make a run repeatable
        against the reference on identical inputs: 'x_T' (B, 1, T, 88) and 'noise' (timesteps, B, 1, T, 88)."""
        if self.hparams.debug:
            raise NotImplementedError("debug=True feeds the label roll where the waveform belongs "
                                      "(task/diffusion.py:780-781): a development switch of the reference, not a mode")
        frame = batch["frame"]
        x_T = batch.get("x_T")
        D = self.draws()
        if self.start_configured():      # (as predict_step: the roll to start from is batch['init'], never x_T)
            init = self._batch_init(batch.get("init"))
            rolls, spec = self.sample(None, batch["audio"], noise=batch.get("noise"), seed=batch_idx, draws=D,
                                      init=init.repeat(D, 1, 1, 1))
            return (self._ensemble(rolls, D) if D > 1 else rolls), spec
        if D > 1:
            # hparams.sampling.draws: D rolls per clip in one chain ('x_T' (D*B, 1, T, 88) / 'noise' (timesteps, D*B, 1, T, 88),
            # draw-major; x_T drawn on the host from a generator seeded with batch_idx when absent); the roll returned -
            # scored by test_step, exported by the CLI - is their mean
            if x_T is None:
                x_T = torch.randn(D * frame.shape[0], 1, frame.shape[1], frame.shape[2],
                                  generator=torch.Generator().manual_seed(int(batch_idx)))
            rolls, spec = self.sample(x_T, batch["audio"], noise=batch.get("noise"), seed=batch_idx, draws=D)
            return self._ensemble(rolls, D), spec
        if x_T is None:
            x_T = torch.randn(frame.shape[0], 1, frame.shape[1], frame.shape[2], device=self.engine.device)
        return self.sample(x_T, batch["audio"], noise=batch.get("noise"), seed=batch_idx)
