"""The recording stand-in for Engine and the small façade built on it (see tests/test_facade_cpu.py, which asserts every
entry point's conversation with it), the clips and the expected-call builders: what the CPU façade tests share - test
infrastructure, not collected."""
import torch

from diffroll_amd import ClassifierFreeDiffRoll
from diffroll_amd.engine import Engine

HOP, MELS = 512, 229
SAMPLERS = ("ddpm_x0", "cfdg_ddpm_x0", "generation_ddpm_x0", "inpainting_ddpm_x0", "ddim_x0", "cfdg_ddim_x0", "ddpm", "ddim",
            "ddim2ddpm")
GUIDED = ("cfdg_ddpm_x0", "inpainting_ddpm_x0", "cfdg_ddim_x0")
W = 0.5
DEFAULTS = dict(window_overlap=0, window_breaks=(), draws=1, draw_stride=0)


class Eq:
    """A tensor compared by shape, contiguity and content."""

    def __init__(self, t):
        self.contiguous = t.is_contiguous()
        self.t = t.detach().clone()

    def __eq__(self, o):
        return isinstance(o, Eq) and self.t.shape == o.t.shape and self.contiguous == o.contiguous and torch.equal(self.t, o.t)

    def __repr__(self):
        return f"Eq({tuple(self.t.shape)}, sum={float(self.t.double().sum()):.6g})"


def eq(t):
    return None if t is None else Eq(t)


class RecordingEngine(Engine):
    """Engine's surface as the façade uses it, with nothing behind it: every method that would reach the library records
    its call instead (what is left of Engine is plain Python over these methods)."""

    def __init__(self, timesteps):
        self.device = torch.device("cpu")
        self.precision, self.hop_length, self.n_mels, self.timesteps = "f32", HOP, MELS, timesteps
        self.window_overlap, self.window_breaks, self.sampling_steps = 0, (), 0
        self.draws, self.draw_stride, self.solver_order, self.guidance_interval = 1, 0, 0, (0, -1)
        self.blocked_accumulation = 2
        self.calls, self.fail = [], False

    def close(self):
        pass

    def load_params(self, params):
        self.calls.append(("load_params", len(params)))

    def set_precision(self, mode):
        self.calls.append(("set_precision", mode))
        self.precision = mode

    def set_option(self, name, value):
        value = int(value)
        if name == "window_break":        # b >= 1 adds a mark, 0 clears them all
            attr, new = "window_breaks", tuple(sorted(set(self.window_breaks) | {value})) if value else ()
        elif name == "guidance_t_min":
            attr, new = "guidance_interval", (value, self.guidance_interval[1])
        elif name == "guidance_t_max":
            attr, new = "guidance_interval", (self.guidance_interval[0], value)
        else:
            attr, new = name, value
        self.calls.append(("set_option", name, value, getattr(self, attr, None) != new))
        setattr(self, attr, new)

    def set_guidance_interval(self, lo=0, hi=-1):
        self.calls.append(("set_guidance_interval", lo, hi, self.guidance_interval != (lo, hi)))
        self.guidance_interval = (lo, hi)

    def set_window_breaks(self, marks):
        marks = tuple(sorted(set(int(b) for b in marks)))
        self.calls.append(("set_window_breaks", marks, self.window_breaks != marks))
        self.window_breaks = marks

    def frontend(self, waveform, T_roll, inpainting_t=None, inpainting_f=None, return_spec=True):
        self.calls.append(("frontend", eq(waveform), T_roll, inpainting_t, inpainting_f))
        B, L = waveform.shape
        return torch.zeros(B, self.n_mels, min(T_roll, L // self.hop_length + 1))

    def forward(self, x, t, uncond):
        self.calls.append(("forward", eq(x), t, uncond))
        return x

    def forward_steps(self, x, steps, uncond):
        self.calls.append(("forward_steps", eq(x), list(steps), uncond))
        return x

    def step(self, sampler, x, noise, t, w=0.0, seed=0, first_sample=0):
        self.calls.append(("step", sampler, eq(x), eq(noise), t, w, seed, first_sample))
        return x

    def sample(self, sampler, x, noise, w=0.0, seed=0, first_sample=0, use_graph=True, check=True):
        self.calls.append(("sample", sampler, eq(x), eq(noise), w, seed, first_sample, use_graph, check, self.options()))
        if self.fail:
            raise RuntimeError("the engine's sample failed")
        return x

    def finish(self):
        self.calls.append(("finish",))

    def options(self):
        return dict(window_overlap=self.window_overlap, window_breaks=self.window_breaks, draws=self.draws,
                    draw_stride=self.draw_stride)

    def talk(self):
        """The record since the last look, without the sets that changed nothing and with every run of consecutive option
        sets in one canonical order."""
        out, run = [], []
        for c in self.calls:
            if c[0].startswith("set_") and c[0] != "set_precision":
                if c[-1]:
                    run.append(c[:-1])
                continue
            out += sorted(run, key=repr) + [c]
            run = []
        self.calls = []
        return out + sorted(run, key=repr)


def facade(sampler="cfdg_ddpm_x0", timesteps=6, sampling=None, **kw):
    args = dict(residual_channels=64, unconditional=False, condition="fixed", n_mels=MELS, norm_args=[0, 1, "imagewise"],
                residual_layers=3, kernel_size=3, dilation_base=2, dilation_bound=4,
                spec_args=dict(sample_rate=16000, n_fft=2048, hop_length=HOP, n_mels=MELS, f_min=0, f_max=8000, center=True,
                               normalized=True, pad_mode="reflect"),
                timesteps=timesteps, sampling=dict({"type": sampler, "w": W}, **(sampling or {})))
    args.update(kw)
    m = ClassifierFreeDiffRoll(**args)
    eng = RecordingEngine(timesteps)
    m._engine = eng
    assert m.engine is eng and eng.calls[0][0] == "load_params"      # the first use uploads the parameters
    eng.calls = []
    return m, eng


def clip(B, T, frames=None, seed=0, S=6):
    """(waveform (B, frames * hop), x (B, 1, T, 88), one step's noise, the chain's noise)."""
    g = torch.Generator().manual_seed(seed)
    wav = torch.randn(B, (T if frames is None else frames) * HOP, generator=g)
    return wav, torch.randn(B, 1, T, 88, generator=g), torch.randn(B, 1, T, 88, generator=g), torch.randn(S, B, 1, T, 88, generator=g)


def weight(sampler):
    return W if sampler in GUIDED else 0.0


def sample_call(sampler, x, z, seed=0, first=0, use_graph=True, check=True, **options):
    return ("sample", sampler, eq(x), eq(z), weight(sampler), seed, first, use_graph, check, dict(DEFAULTS, **options))


L2, L1 = 700 * HOP - 100, 300 * HOP + 5                      # recordings of two windows and of one
