"""Spectrogram geometries of the mel front-end beyond the released one, and its float64 reference - test infrastructure
(CPU only; tests/test_frontend_geometry_cpu.py and tests/test_gpu_frontend_geometry.py share it).

dr_create takes any n_fft % 32 == 0 up to 65536, any hop_length % 4 == 0 and any n_mels > 0; dr_frontend any clip longer
than n_fft / 2.  CASES holds, per code path behind that surface, the smallest geometry that reaches it; paths() restates
from the launch conditions of csrc/frontend.hip, csrc/pack.hip, csrc/gemm.hip and csrc/abi.hip which path a geometry takes,
so that the table's coverage is an assertion and not a comment.

frontend64 is the reference: the front-end of oracle.diffroll_ref (torchaudio's MelSpectrogram, log, min-max, masks)
evaluated in float64 - with ONE fp32 ingredient, the filterbank, whose fp32 rounding is part of the contract
(tests/test_host_cpu.py: test_frontend_tables_carry_the_reference_rounding).
"""
from collections import namedtuple

import torch

from oracle import diffroll_ref as R

Case = namedtuple("Case", "n_fft hop n_mels sample_rate f_min f_max L")

CASES = [
    Case(32, 4, 8, 16000, 0, 8000, 81),            # smallest transform: H = 16 < the 256-thread block; L % 4 != 0: scalar reflect pad
    Case(64, 16, 20, 16000, 0, 8000, 700),         # H = 32: two radix-4 passes plus the radix-2 pass
    Case(256, 64, 40, 16000, 0, 8000, 4099),       # radix-2 pass; L % 4 = 3
    Case(512, 128, 64, 16000, 0, 8000, 8192),      # pure radix-4; one mel tile; n_mels % 4 = 0
    Case(1024, 256, 80, 22050, 20, 11025, 16384),  # the common alternative geometry; radix-2 pass
    Case(4096, 1024, 229, 16000, 0, 8000, 40000),  # radix-2 pass, H = 2048; min-max cut over two workgroups
    Case(16384, 4096, 229, 16000, 0, 8000, 20481),  # largest FFT: 128 KiB of LDS
    Case(96, 24, 16, 16000, 0, 8000, 1000),        # windowed-DFT GEMM; bins_p = 64
    Case(1536, 384, 128, 16000, 30, 7600, 9001),   # DFT GEMM; exactly one full mel tile; L odd
    Case(2400, 600, 229, 48000, 0, 8000, 12000),   # DFT GEMM; 3 empty mel filters (rows at the floor log 1e-6)
    Case(2048, 500, 229, 16000, 0, 8000, 10000),   # hop does not divide n_fft
    Case(256, 512, 130, 16000, 0, 8000, 6000),     # hop > n_fft; n_mels % 4 = 2; 15 empty filters; 33 mel planes (conditioner K guard)
    Case(2048, 512, 229, 16000, 0, 8000, 1025),    # L = n_fft / 2 + 1, the shortest clip accepted: TF = 3, both reflections overlap
    Case(1024, 256, 83, 16000, 0, 8000, 25603),    # n_mels % 4 = 3; 21 planes x 101 frames: min-max over two workgroups at a small n_mels
]
SILENT_CASE = Case(1024, 256, 80, 22050, 20, 11025, 16384)      # the one case that carries a silent clip (exact zeros out)
NOISE, SINE, IMPULSE, SILENCE = 0, 1, 2, 3
MODES = ("imagewise", "framewise")

# calls on ONE engine, in this order (B, L): buffers regrow, shrink and are re-split; 28162 samples are 111 frames = a
# two-workgroup min-max at 80 mel rows
REUSE_CASE = SILENT_CASE
REUSE_CALLS = [(3, 16384), (1, 28162), (2, 5001), (3, 28162)]
# the cases whose shortest accepted clip (L = n_fft / 2 + 1) is run besides the table's own: smallest FFT, smallest DFT
SHORTEST_CASES = [CASES[0], CASES[7], CASES[12]]

# the tiny network the GPU tests run behind the front-end
NET = dict(residual_channels=64, residual_layers=2, kernel_size=3, timesteps=4)


def case_id(c) -> str:
    return f"{c.n_fft}-{c.hop}-{c.n_mels}-L{c.L}"


def case_hp(c, mode: str = "imagewise") -> dict:
    hp = dict(R.DEFAULT_HP)
    hp.update(NET)
    hp.update(n_fft=c.n_fft, hop_length=c.hop, n_mels=c.n_mels, sample_rate=c.sample_rate, f_min=float(c.f_min),
              f_max=float(c.f_max), norm_mode=mode)
    return hp


def frames(c, L=None) -> int:
    return (c.L if L is None else L) // c.hop + 1


def clips(c, L=None, B=None) -> torch.Tensor:
    """(B, L) float32: noise, a 440 Hz sine in faint noise, a unit impulse (and silence at SILENT_CASE), from a
    generator seeded by the case."""
    L = c.L if L is None else L
    g = torch.Generator().manual_seed(c.n_fft * 1000003 + c.hop * 1009 + c.n_mels * 31 + L)
    n = torch.arange(L, dtype=torch.float64)
    wav = [0.1 * torch.randn(L, generator=g),
           (0.3 * torch.sin(2 * torch.pi * 440.0 * n / c.sample_rate)).float() + 0.001 * torch.randn(L, generator=g),
           torch.zeros(L).index_fill_(0, torch.tensor([L // 3]), 1.0)]
    if c == SILENT_CASE:
        wav.append(torch.zeros(L))
    wav = torch.stack(wav)
    return wav if B is None else wav[:B].contiguous()


def compared_clips(c, mode: str, B=None):
    """The clips of clips(c) a test compares under `mode`.  The ONE exclusion: the impulse under framewise
    normalisation, at every case.  Frames the impulse does not reach hold nothing but the rounding noise of the
    transform (1e-14 of the peak), and per-frame min-max stretches that noise to [0, 1]: there the fp32 reference itself
    is 6.6e-4 away from the float64 one (4096 / 1024 / 229), i.e. the comparison would measure the reference."""
    n = (4 if c == SILENT_CASE else 3) if B is None else B
    return [b for b in range(n) if not (mode == "framewise" and b == IMPULSE)]


def frontend64(wav, hp, framewise, inpainting_t=None, inpainting_f=None):
    """(power (B, TF, bins), normalised + masked + untrimmed spectrogram (B, n_mels, TF)) in float64."""
    n_fft, hop = int(hp["n_fft"]), int(hp["hop_length"])
    w = torch.hann_window(n_fft, dtype=torch.float64)
    z = torch.stft(wav.double(), n_fft=n_fft, hop_length=hop, win_length=n_fft, window=w, center=True, pad_mode="reflect",
                   normalized=False, onesided=True, return_complex=True)
    z = z / w.pow(2.0).sum().sqrt()
    power = z.abs().pow(2.0)                                                    # (B, bins, TF)
    fb = R.melscale_fbanks_htk(n_fft // 2 + 1, float(hp["f_min"]), float(hp["f_max"]), int(hp["n_mels"]),
                               int(hp["sample_rate"])).double()
    spec = torch.log(torch.matmul(power.transpose(-1, -2), fb).transpose(-1, -2) + 1e-6)
    if framewise:
        lo, hi = spec.min(1, keepdim=True)[0], spec.max(1, keepdim=True)[0]
    else:
        lo, hi = spec.flatten(1).min(1)[0][:, None, None], spec.flatten(1).max(1)[0][:, None, None]
    spec = (spec - lo) / (hi - lo)
    spec[torch.isnan(spec)] = 0.0
    ft = slice(None) if not inpainting_t else slice(int(inpainting_t[0]), int(inpainting_t[1]))
    ff = slice(None) if not inpainting_f else slice(int(inpainting_f[0]), int(inpainting_f[1]))
    if inpainting_t or inpainting_f:
        spec[:, ff, ft] = -1.0
    return power.transpose(1, 2).contiguous(), spec


def dft32_frontend(wav, hp, framewise):
    """The windowed-DFT GEMM's sum restated in fp32 on the CPU: frames x (window * cos | window * sin) / ||w|| as ONE fp32
    matmul over the n_fft samples of a frame, then the later stages of the front-end in fp32.  Its distance to frontend64
    is the rounding an fp32 n_fft-term sum per bin costs at a geometry - what a bound for the DFT path may be derived from
    (twice that: another accumulation order), never the engine's own output."""
    n_fft, hop = int(hp["n_fft"]), int(hp["hop_length"])
    w = torch.hann_window(n_fft, dtype=torch.float64)
    k = torch.arange(n_fft, dtype=torch.int64)
    ph = (k[:, None] * torch.arange(n_fft // 2 + 1, dtype=torch.int64)[None, :]) % n_fft       # exact phase index
    ang = 2 * torch.pi * ph.double() / n_fft
    scale = (w / w.pow(2.0).sum().sqrt())[:, None]
    mat = torch.cat([scale * torch.cos(ang), scale * torch.sin(ang)], dim=1).float()            # (n_fft, 2 bins)
    pad = torch.nn.functional.pad(wav.float()[:, None], (n_fft // 2, n_fft // 2), mode="reflect")[:, 0]
    fr = pad.unfold(1, n_fft, hop)                                                              # (B, TF, n_fft)
    z = fr @ mat
    re, im = z[..., :n_fft // 2 + 1], z[..., n_fft // 2 + 1:]
    power = (re * re + im * im).transpose(1, 2)                                                 # (B, bins, TF)
    fb = R.melscale_fbanks_htk(n_fft // 2 + 1, float(hp["f_min"]), float(hp["f_max"]), int(hp["n_mels"]), int(hp["sample_rate"]))
    spec = torch.log(torch.matmul(power.transpose(-1, -2), fb).transpose(-1, -2) + 1e-6)
    return R.normalize_framewise(spec) if framewise else R.normalize_imagewise(spec)


# ---------------------------------------------------------------------------------------------
# which code path a geometry takes
# ---------------------------------------------------------------------------------------------
MINMAX_CHUNK_BYTES, MINMAX_CHUNKS = 32768, 32


def minmax_chunks(n_mels: int, TF: int) -> int:
    """launch_minmax: workgroups per clip of the imagewise min-max."""
    nbytes = ((n_mels + 3) // 4) * TF * 16
    return max(1, min(MINMAX_CHUNKS, (nbytes + MINMAX_CHUNK_BYTES - 1) // MINMAX_CHUNK_BYTES))


def gemm_ks(kchunks: int) -> int:
    """launch_gemm: 32-channel chunks staged per hand-over by a 1-tap GEMM."""
    return 4 if kchunks % 4 == 0 else 2 if kchunks % 2 == 0 else 1


def paths(c) -> dict:
    N, H = c.n_fft, c.n_fft // 2
    fft = 8 <= N <= 16384 and N & (N - 1) == 0                      # pack.hip: use_fft
    log2h = H.bit_length() - 1
    planes = (c.n_mels + 3) // 4                                    # abi.hip: mel_planes
    return dict(
        spectrum="fft" if fft else "dft",
        radix2=(log2h % 2 == 1) if fft else None,                   # stft_power_kernel: one radix-2 pass when log2 H is odd
        sub_block=(H < 256) if fft else None,                       # fewer complex points than the block has threads
        max_lds=(N == 16384) if fft else None,                      # n_fft * 8 bytes of dynamic LDS: 128 KiB
        reflect="quad" if c.L % 4 == 0 and (N // 2) % 4 == 0 else "scalar",      # launch_reflect_pad
        hop="divides" if N % c.hop == 0 else "beyond" if c.hop > N else "ragged",
        bins_p=-(-(H + 1) // 64) * 64,                              # dr_create: bins padded to 64
        mel_tiles=(c.n_mels + 127) // 128,                          # dr_frontend: M tiles of the filterbank GEMM
        mel_mod4=c.n_mels % 4,                                      # valid rows of the last mel plane (0: all four)
        minmax="many" if minmax_chunks(c.n_mels, frames(c)) > 1 else "one",
        cond_ks=gemm_ks((planes + 7) // 8),                         # conditioner GEMM: K = 4 planes, kchunks = ceil(planes / 8)
        cond_guard=planes % 8 != 0,                                 # its last chunk reads past x_planes: the producer's clamp
        shortest=c.L == H + 1,
    )


# every value of each path the table must reach
REQUIRED = dict(spectrum={"fft", "dft"}, radix2={True, False, None}, sub_block={True, False, None}, max_lds={True, False, None},
                reflect={"quad", "scalar"}, hop={"divides", "ragged", "beyond"}, mel_tiles={1, 2}, mel_mod4={0, 1, 2, 3},
                minmax={"one", "many"}, cond_ks={1, 2, 4}, cond_guard={True, False}, shortest={True, False})
