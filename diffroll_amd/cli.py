"""Command-line drivers with the reference's command surface (sampling.py:22-73, infer.py:19-45).

    python sampling.py task=generation dataset.num_samples=8 dataloader.batch_size=4 model.args.kernel_size=9
    python sampling.py task=transcription dataset=Custom dataset.args.audio_path=my_audio dataset.args.audio_ext=wav \
        checkpoint_path=weights/Pretrain_MAESTRO-retrain_MAESTRO-k=9.ckpt
    python sampling.py task=inpainting task.inpainting_t=[500,650] dataset=Custom ...
    python sampling.py task=transcription dataset=Custom dataset.args.max_segment_samples=null task.window_overlap=160 ...
    python sampling.py task=transcription task.sampling.steps=50 ...      # 50 respaced steps instead of 200
    python sampling.py task=transcription task.sampling.guidance_interval=[60,140] ...      # guide steps 60..140 only
    python sampling.py task=transcription dataset=Custom dataset.args.max_segment_samples=null task.sampling.strength=0.5 \
        task.sampling.init_dir=outputs ...      # refine the rolls of an earlier run: the last half of the chain, from them
    torchrun --nproc-per-node 8 sampling.py task=generation gpus=8 dataset.num_samples=128 dataloader.batch_size=128

Hydra is not a dependency: the same ``group=name`` / ``dotted.key=value`` override syntax is parsed here over
defaults that restate config/sampling.yaml, config/task/{generation,transcription,inpainting}.yaml,
config/model/ClassifierFreeDiffRoll.yaml and config/spec/mel.yaml.  Differences from the reference driver:
no Lightning Trainer / TensorBoard; rolls are written as ``rolls_batch<i>.npy`` plus ``raw_midi_<batch>_<i>.mid`` / ``clean_midi_e<batch>_<i>.mid``;
audio ingestion (utils/custom_dataset.py:55-91) reads .wav only (no mp3 codec in this image); resampling restates
torchaudio 0.11's windowed-sinc kernel (diffroll_amd/audio.py).

Long-form: ``dataset=Custom dataset.args.max_segment_samples=null`` transcribes every file whole (the reference
documents None as "get the full audio", utils/custom_dataset.py:21, but crashes on it): each recording is one chain of
jointly sampled 640-frame windows overlapping by ``task.window_overlap`` frames (default 160; diffroll_amd/longform.py;
``task.window_blend=linear`` / ``nearest`` cross-fades the windows over those frames or hands over in their middle),
written as ``roll_<stem>.npy`` (1, 1, ceil(L / hop), 88), ``raw_midi_<stem>.mid`` and ``clean_midi_<stem>.mid``.  With
``gpus=N`` every rank takes the files round-robin and writes its own outputs.

``task.recordings_per_chain=N`` (long-form only, default 1) puts up to N consecutive files into ONE chain
(ClassifierFreeDiffRoll.sample_long_batch; longform.pack_chains closes a chain early at longform.MAX_WINDOWS windows):
short recordings then fill the device together.  The chains are dealt round-robin to the ranks; a chain whose first
file is file j runs with seed = seed + j, and the roll of file i equals ``sample_long(wav, seed=<that chain's seed>,
recording=i)``.  It does NOT equal the N = 1 run, which seeds every file with seed + i.  The output files are the same.

``task.sampling.strength=S`` (0 < S <= 1) or ``task.sampling.start_step=T`` with ``task.sampling.init_dir=DIR`` (long-form
only) starts every chain from a given roll (options "start_step" / "start_noise"): for each input file,
``DIR/roll_<stem>.npy`` - the file this path itself writes - is diffused to the start step and only the remaining steps run.
"""
from __future__ import annotations

import ast
import copy
import glob
import os
import sys
import time
import warnings
from typing import Any, Dict, List

import numpy as np
import torch

TASKS: Dict[str, Dict[str, Any]] = {
    # config/task/generation.yaml, inpainting.yaml (Custom variant: inpainting_t null), transcription.yaml
    "generation": dict(timesteps=200, beta_start=1e-4, beta_end=0.02, frame_threshold=0.5, generation_filter=0.02,
                       sampling=dict(type="generation_ddpm_x0"), inpainting_t=None, inpainting_f=None),
    "inpainting": dict(timesteps=200, beta_start=1e-4, beta_end=0.02, frame_threshold=0.5, generation_filter=0.02,
                       sampling=dict(type="inpainting_ddpm_x0", w=0.5), inpainting_t=[500, 650], inpainting_f=None),
    "transcription": dict(timesteps=200, beta_start=1e-4, beta_end=0.02, frame_threshold=0.5, generation_filter=0.02,
                          sampling=dict(type="cfdg_ddpm_x0", w=0.5), inpainting_t=None, inpainting_f=None),
}
DATASETS: Dict[str, Dict[str, Any]] = {
    "Sampling": dict(name="Sampling", num_samples=4, args=dict()),                     # noise only (generation)
    "Custom": dict(name="Custom", num_samples=4,                                         # config/dataset/Custom.yaml
                   args=dict(audio_path="my_audio", audio_ext="wav", max_segment_samples=327680, sample_rate=16000)),
    "Synthetic": dict(name="Synthetic", num_samples=4, args=dict(seed=0)),              # 0.1 * randn waveforms
}
DEFAULTS: Dict[str, Any] = dict(
    gpus=1, hop_length=512, sequence_length=327680, sampling_rate=16000, checkpoint_path=None, seed=0,
    output_dir="outputs", precision="f32",
    dataloader=dict(batch_size=4),
    model=dict(name="ClassifierFreeDiffRoll",
               args=dict(residual_channels=512, unconditional=False, condition="fixed", n_mels=229,
                         residual_layers=15, kernel_size=3, dilation_base=2, dilation_bound=4, spec_dropout=0.1,
                         norm_args=[0, 1, "imagewise"])),
    spec=dict(args=dict(sample_rate=16000, n_fft=2048, hop_length=512, n_mels=229, f_min=0, f_max=8000, center=True,
                        normalized=True, pad_mode="reflect")),
)


def _parse_value(text: str):
    if text.lower() in ("null", "none"):
        return None
    if text.lower() in ("true", "false"):
        return text.lower() == "true"
    try:
        return ast.literal_eval(text)
    except Exception:
        return text


def build_config(argv: List[str], default_task: str = "generation") -> Dict[str, Any]:
    cfg = copy.deepcopy(DEFAULTS)
    groups = {"task": default_task, "dataset": None}
    rest = []
    for arg in argv:
        if "=" not in arg:
            raise SystemExit(f"expected key=value, got '{arg}'")
        k, v = arg.split("=", 1)
        if k in groups:
            groups[k] = v
        else:
            rest.append((k, v))
    if groups["task"] not in TASKS:
        raise SystemExit(f"unknown task '{groups['task']}' (choose from {sorted(TASKS)})")
    cfg["task"] = copy.deepcopy(TASKS[groups["task"]])
    cfg["task"]["name"] = groups["task"]
    ds = groups["dataset"] or ("Sampling" if groups["task"] == "generation" else "Synthetic")
    if ds not in DATASETS:
        raise SystemExit(f"dataset '{ds}' is not available here (choose from {sorted(DATASETS)}); MAPS / MAESTRO "
                         "need the AudioLoader package and the datasets on disk")
    cfg["dataset"] = copy.deepcopy(DATASETS[ds])
    for k, v in rest:
        node = cfg
        parts = k.split(".")
        for part in parts[:-1]:
            node = node.setdefault(part, {})
        node[parts[-1]] = _parse_value(v)
    # precision=f32 | bf16x3 | bf16 | f16: the arithmetic of the two hot contractions (Engine.set_precision)
    from ._cabi import PRECISIONS
    if cfg.get("precision", "f32") not in PRECISIONS:
        raise SystemExit(f"precision must be one of {sorted(PRECISIONS)}, got {cfg.get('precision')!r}")
    # task.sampling.steps=N: the chain on N respaced steps (option "sampling_steps"); absent / null / 0 = every step
    steps, S = cfg["task"]["sampling"].get("steps"), cfg["task"].get("timesteps")
    if steps is not None and (isinstance(steps, bool) or not isinstance(steps, int) or not isinstance(S, int)
                              or not (steps == 0 or 2 <= steps <= S)):
        raise SystemExit(f"task.sampling.steps must be an integer in [2, task.timesteps = {S}] (or 0 / null: every "
                         f"step), got {steps!r}")
    # task.sampling.draws=D: D rolls per clip in one chain (option "draws"); their mean is exported; absent / null / 1 = one
    draws = cfg["task"]["sampling"].get("draws")
    if draws is not None and (isinstance(draws, bool) or not isinstance(draws, int) or draws < 1):
        raise SystemExit(f"task.sampling.draws must be an integer >= 1 (or null: one roll per clip), got {draws!r}")
    # the other task.sampling keys - guidance_interval=[lo,hi], solver_order=N, solver_noise=1, strength=S / start_step=T,
    # x0_clip=1 (to the roll's range model.args.norm_args), x0_threshold=0.995, cfg_rescale=0.7,
    # cfg_project=1.0, cfg_norm=0.05, cfg_momentum=-0.5, guidance_stride=2, exact_below=25 - are read as the model reads them
    # (schedule.sampling_options: each key's validator and the engine option it becomes); absent / null = off
    from .schedule import sampling_options
    samp = cfg["task"]["sampling"]
    start_key = next((k for k in ("strength", "start_step") if samp.get(k) is not None), None)
    try:
        needs_S = next((k for k in ("guidance_interval", start_key, "exact_below") if k and samp.get(k) is not None), None)
        if needs_S and not isinstance(S, int):      # (the keys that are read against the schedule's length)
            bad = ValueError(f"task.timesteps = {S!r}")
            bad.key = needs_S
            raise bad
        sampling_options(samp, S, cfg["model"]["args"].get("norm_args"))
    except ValueError as err:
        raise SystemExit(f"task.sampling.{err.key}: {err}")
    # strength / start_step with task.sampling.init_dir=DIR: start every chain from the roll DIR/roll_<stem>.npy (options
    # "start_step" / "start_noise"); long-form only - the path that writes that file
    if start_key is not None:
        if not isinstance(samp.get("init_dir"), str):
            raise SystemExit(f"task.sampling.{start_key} starts every chain from a given roll: task.sampling.init_dir=DIR (the "
                             f"folder holding roll_<stem>.npy for every input file) is required")
        if not is_long_form(cfg):
            raise SystemExit(f"task.sampling.{start_key} is supported where roll_<stem>.npy is written: dataset=Custom "
                             f"dataset.args.max_segment_samples=null (long-form)")
    elif samp.get("init_dir") is not None:
        raise SystemExit("task.sampling.init_dir needs task.sampling.strength=S or task.sampling.start_step=T")
    per_chain = cfg["task"].get("recordings_per_chain", 1)
    if isinstance(per_chain, bool) or not isinstance(per_chain, int) or per_chain < 1:
        raise SystemExit(f"task.recordings_per_chain must be an integer >= 1, got {per_chain!r}")
    if per_chain > 1 and not is_long_form(cfg):
        raise SystemExit("task.recordings_per_chain groups whole recordings: it needs dataset=Custom "
                         "dataset.args.max_segment_samples=null (long-form)")
    if is_long_form(cfg):
        sampler = cfg["task"]["sampling"]["type"]
        if sampler == "inpainting_ddpm_x0":
            raise SystemExit("max_segment_samples=null (long-form) cannot run inpainting_ddpm_x0: its masks are in the "
                             "coordinates of one 640-frame clip, not of a recording")
        overlap = cfg["task"].get("window_overlap", DEFAULT_WINDOW_OVERLAP)
        if not isinstance(overlap, int) or not 1 <= overlap <= 320:
            raise SystemExit(f"task.window_overlap must be an integer in [1, 320] (half the 640-frame window), got {overlap!r}")
        # task.window_blend=linear: what the frames two windows share take of their predictions (option "window_blend")
        from .longform import check_window_blend
        try:
            check_window_blend(cfg["task"].get("window_blend"))
        except ValueError as err:
            raise SystemExit(f"task.window_blend: {err}")
    return cfg


DEFAULT_WINDOW_OVERLAP = 160


def steps_label(cfg: Dict[str, Any]) -> str:
    S, n = int(cfg["task"]["timesteps"]), cfg["task"]["sampling"].get("steps")
    return f"{n} of {S} steps" if n and n != S else f"{S} steps"


def is_long_form(cfg: Dict[str, Any]) -> bool:
    """dataset=Custom with max_segment_samples=null: every file is transcribed whole (diffroll_amd/longform.py)."""
    return cfg["dataset"]["name"] == "Custom" and cfg["dataset"]["args"].get("max_segment_samples", 0) is None


def load_wav_folder(args: Dict[str, Any]) -> torch.Tensor:
    """utils/custom_dataset.py:55-91 over a folder: mono mix, torchaudio-0.11 windowed-sinc resampling, crop /
    zero-pad to max_segment_samples (diffroll_amd/audio.py)."""
    from .audio import ingest
    files = wav_files(args)
    return torch.stack([ingest(f, int(args["sample_rate"]), int(args["max_segment_samples"])) for f in files])


def wav_files(args: Dict[str, Any]) -> List[str]:
    if str(args["audio_ext"]).lower() != "wav":
        raise SystemExit("only .wav can be decoded in this environment (no mp3/flac codec)")
    files = sorted(glob.glob(os.path.join(args["audio_path"], f"*.{args['audio_ext']}")))
    if not files:
        raise SystemExit(f"no *.{args['audio_ext']} files under {args['audio_path']}")
    return files


def transcribe_long_form(cfg: Dict[str, Any], model, rank: int, world: int) -> List[str]:
    """Every file of the Custom folder whole (max_segment_samples=null): this rank's share, dealt round-robin, one
    sample_long chain per recording (file i: seed = seed + i, recording = i) - or, with task.recordings_per_chain > 1,
    one sample_long_batch chain per group of consecutive files; writes roll_<stem>.npy, raw_midi_<stem>.mid and
    clean_midi_<stem>.mid.  Returns the roll paths written."""
    from .audio import ingest
    from .longform import deal
    args = cfg["dataset"]["args"]
    files = wav_files(args)
    if cfg["dataset"].get("num_samples"):
        files = files[:int(cfg["dataset"]["num_samples"])]
    overlap = int(cfg["task"].get("window_overlap", DEFAULT_WINDOW_OVERLAP))
    generation = cfg["task"]["sampling"]["type"] == "generation_ddpm_x0"
    hop = int(cfg["hop_length"])
    out = cfg["output_dir"]
    written = []
    D = int(cfg["task"]["sampling"].get("draws") or 1)
    more = {"draws": D} if D > 1 else {}
    if cfg["task"].get("window_blend") is not None:
        more["blend"] = cfg["task"]["window_blend"]
    init_dir = cfg["task"]["sampling"].get("init_dir")

    def init_roll(path, wav):
        """task.sampling.init_dir: the roll this recording's chain starts from, (1, 1, ceil(L / hop), 88) (shared by the draws)"""
        stem = os.path.splitext(os.path.basename(path))[0]
        roll_path = os.path.join(init_dir, f"roll_{stem}.npy")
        if not os.path.exists(roll_path):
            raise SystemExit(f"task.sampling.init_dir: {roll_path} does not exist (the roll to start {os.path.basename(path)} from)")
        roll = np.load(roll_path)
        want = (1, 1, -(-wav.shape[0] // hop), 88)
        if tuple(roll.shape) != want:
            raise SystemExit(f"task.sampling.init_dir: {roll_path} has shape {tuple(roll.shape)}, the recording needs {want}")
        return torch.from_numpy(roll).to(torch.float32)

    def write(path, roll):
        stem = os.path.splitext(os.path.basename(path))[0]
        if D > 1:       # (D, 1, T_out, 88): the mean roll takes the single roll's place, the votes go next to it
            from .ensemble import aggregate
            roll, votes, _ = aggregate(roll, D, float(cfg["task"]["frame_threshold"]))
            np.save(os.path.join(out, f"votes_{stem}.npy"), votes.cpu().numpy())
        roll_path = os.path.join(out, f"roll_{stem}.npy")
        np.save(roll_path, roll.cpu().numpy())
        written.append(roll_path)
        # export_midi names files <prefix><index in the batch>: one recording = index 0
        tmp_raw, tmp_clean = os.path.join(out, f".raw_{stem}_"), os.path.join(out, f".clean_{stem}_")
        model.export_midi(roll, tmp_raw, clean_prefix=tmp_clean)
        os.replace(tmp_raw + "0.mid", os.path.join(out, f"raw_midi_{stem}.mid"))
        os.replace(tmp_clean + "0.mid", os.path.join(out, f"clean_midi_{stem}.mid"))

    per_chain = int(cfg["task"].get("recordings_per_chain", 1))
    if per_chain > 1:
        # task.recordings_per_chain: consecutive files share a chain (module docstring); every file is read up front,
        # since the window counts decide the grouping
        from .longform import deal_chains, pack_chains, plan_windows
        wavs = [ingest(path, int(args["sample_rate"]), None) for path in files]
        counts = [plan_windows(wv.shape[0], hop, overlap=overlap).n for wv in wavs]
        for chain in deal_chains(pack_chains(counts, per_chain), rank, world):
            j = chain[0]
            seed = int(cfg["seed"]) + j
            kw = dict(more, init=[init_roll(files[i], wavs[i]) for i in chain]) if init_dir else more
            if generation:
                rolls = model.sample_long_batch(frames=[-(-wavs[i].shape[0] // hop) for i in chain], overlap=overlap,
                                                seed=seed, first_recording=j, **kw)
            else:
                rolls = model.sample_long_batch([wavs[i] for i in chain], overlap=overlap, seed=seed, first_recording=j, **kw)
            for i, roll in zip(chain, rolls):
                write(files[i], roll)
        return written
    for i, path in deal(list(enumerate(files)), rank, world):
        wav = ingest(path, int(args["sample_rate"]), None)
        seed = int(cfg["seed"]) + i
        kw = dict(more, init=init_roll(path, wav)) if init_dir else more
        if generation:          # (the waveform is ignored, sampling.py:45: a roll of the recording's length)
            roll = model.sample_long(frames=-(-wav.shape[0] // hop), overlap=overlap, seed=seed, recording=i, **kw)
        else:
            roll = model.sample_long(wav, overlap=overlap, seed=seed, recording=i, **kw)
        write(path, roll)
    return written


def make_model(cfg: Dict[str, Any], device):
    from . import ClassifierFreeDiffRoll
    task = cfg["task"]
    kwargs = dict(spec_args=cfg["spec"]["args"], timesteps=task["timesteps"], beta_start=task["beta_start"],
                  beta_end=task["beta_end"], frame_threshold=task["frame_threshold"],
                  generation_filter=task["generation_filter"], sampling=task["sampling"],
                  inpainting_t=task["inpainting_t"], inpainting_f=task["inpainting_f"], training={"mode": "x_0"})
    path = cfg["checkpoint_path"]
    if path:
        # a named checkpoint must exist (the reference fails in load_from_checkpoint, sampling.py:54): random
        # weights are only ever used when NO checkpoint is named
        if not os.path.exists(path):
            raise SystemExit(f"checkpoint_path '{path}' does not exist")
        # keyword overrides win over the checkpoint's hyper_parameters (sampling.py:54-65)
        m = ClassifierFreeDiffRoll.load_from_checkpoint(path, **{k: kwargs[k] for k in (
            "sampling", "frame_threshold", "generation_filter", "inpainting_t", "inpainting_f")})
    else:
        m = ClassifierFreeDiffRoll(**cfg["model"]["args"], **kwargs)
        torch.nn.init.normal_(m.output_projection.weight, 0.0, 0.02)
    m.precision = cfg.get("precision", "f32")
    return m.to(device)


def main(argv: List[str] = None, default_task: str = "generation") -> None:
    cfg = build_config(list(sys.argv[1:] if argv is None else argv), default_task)
    if not torch.cuda.is_available():
        raise SystemExit("sampling needs an MI355X: diffroll_amd has no CPU fallback")
    from . import launch
    gpus = int(cfg.get("gpus") or 1)
    if gpus > 1 and not launch.under_launcher():
        # `gpus=N` is the reference's one flag for N devices (Trainer(gpus=cfg.gpus), sampling.py:70): start the
        # N ranks here, one process per GPU
        if argv is not None:      # called as a function: there is no command line to re-execute
            raise SystemExit(f"gpus={gpus}: start the {gpus} ranks with torch.distributed.run (or run the driver script)")
        # (`python -m diffroll_amd.cli ...`: sys.argv[0] is this file, which cannot run as a plain script - relative
        # imports - so the ranks are started as the same module)
        main_mod = sys.modules.get("__main__")
        spec = getattr(main_mod, "__spec__", None)
        if spec is not None and spec.name and spec.name.startswith("diffroll_amd."):
            raise SystemExit(launch.spawn_ranks(gpus, spec.name, list(sys.argv[1:]), module=True))
        raise SystemExit(launch.spawn_ranks(gpus, os.path.abspath(sys.argv[0]), list(sys.argv[1:])))
    rank, world, local_rank = launch.rank_env()
    if launch.under_launcher():
        # Trainer(gpus=N) counts devices PER NODE (sampling.py:70): compare with the launcher's ranks on THIS node, and
        # only when gpus= was given - an explicitly launched job is authoritative over the default gpus=1 (ADVICE r3:
        # `torchrun --nproc-per-node 8 sampling.py ...` and multi-node jobs must not be rejected)
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world))
        explicit = any(a.split("=", 1)[0] == "gpus" for a in (sys.argv[1:] if argv is None else argv))
        if explicit and local_world != gpus:
            raise SystemExit(f"gpus={gpus} but the launcher started {local_world} rank(s) on this node (WORLD_SIZE={world})")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = launch.init_process_group(device) if world > 1 else None
    from .distributed import sample_sharded

    if is_long_form(cfg):
        model = make_model(cfg, device)
        os.makedirs(cfg["output_dir"], exist_ok=True)
        t0 = time.perf_counter()
        rolls = transcribe_long_form(cfg, model, rank, world)
        frames = sum(int(np.load(p, mmap_mode="r").shape[2]) for p in rolls)
        dt = time.perf_counter() - t0
        print(f"rank {rank}: {len(rolls)} recording(s) whole, {frames} frames, {steps_label(cfg)}, sampler "
              f"{cfg['task']['sampling']['type']}: {dt:.2f} s -> {cfg['output_dir']}/")
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    S = int(cfg["dataset"]["num_samples"])
    hop = int(cfg["hop_length"])
    g = torch.Generator().manual_seed(int(cfg["seed"]))
    T = int(cfg["sequence_length"]) // hop                       # sampling.py:27 uses 640 = 327680 / 512
    name = cfg["dataset"]["name"]
    if name == "Custom":
        waveform = load_wav_folder(cfg["dataset"]["args"])
        S = min(S, waveform.shape[0]) if cfg["dataset"].get("num_samples") else waveform.shape[0]
        waveform = waveform[:S]
        T = waveform.shape[1] // hop
    elif name == "Synthetic":
        waveform = 0.1 * torch.randn(S, int(cfg["sequence_length"]), generator=g)
    else:                                                        # generation: waveform is ignored (sampling.py:45)
        waveform = torch.zeros(S, int(cfg["sequence_length"]))
    x = torch.randn(S, 1, T, 88, generator=g)                    # x_T drawn on the host like sampling.py:27
    # task.sampling.draws=D: draw 0 starts from that x_T, draws 1 .. D-1 from the next draws of the SAME generator (never the
    # x_T of a run with a neighbouring seed)
    D = int(cfg["task"]["sampling"].get("draws") or 1)
    x_more = [torch.randn(S, 1, T, 88, generator=g) for _ in range(1, D)]
    bs = int(cfg["dataloader"]["batch_size"])
    if S < bs:
        warnings.warn(f"Batch size is larger than total number of audio clips. Forcing batch size to {S}")
        bs = S
    t_model = time.perf_counter()
    model = make_model(cfg, device)
    t_engine = time.perf_counter()
    eng = model.engine                       # dr_create + dr_commit (weight packing, uploads, hoisted tables)
    torch.cuda.synchronize()
    t_ready = time.perf_counter()
    os.makedirs(cfg["output_dir"], exist_ok=True)
    t0 = time.perf_counter()
    batch_s = []
    for bi, lo in enumerate(range(0, S, bs)):
        hi = min(lo + bs, S)
        tb = time.perf_counter()
        if D > 1:
            from .ensemble import aggregate
            rolls = sample_sharded(model, torch.cat([x[lo:hi]] + [xm[lo:hi] for xm in x_more], 0), waveform[lo:hi],
                                   seed=int(cfg["seed"]) + bi, draws=D)
            roll, votes, _ = aggregate(rolls, D, float(cfg["task"]["frame_threshold"]))
            if rank == 0:
                np.save(os.path.join(cfg["output_dir"], f"votes_batch{bi}.npy"), votes.cpu().numpy())
        else:
            roll = sample_sharded(model, x[lo:hi], waveform[lo:hi], seed=int(cfg["seed"]) + bi)
        batch_s.append(time.perf_counter() - tb)
        if rank == 0:
            np.save(os.path.join(cfg["output_dir"], f"rolls_batch{bi}.npy"), roll.cpu().numpy())
            model.export_midi(roll, os.path.join(cfg["output_dir"], f"raw_midi_{bi}_"),       # names of predict_step
                              clean_prefix=os.path.join(cfg["output_dir"], f"clean_midi_e{bi}_"))
    torch.cuda.synchronize()
    if rank == 0:
        dt = time.perf_counter() - t0
        print(f"{cfg['task']['name']}: {S} clips x {T} frames, {steps_label(cfg)}, sampler "
              f"{cfg['task']['sampling']['type']}, {world} GPU(s): {dt:.2f} s ({S * T / dt:.1f} frames/s incl. load "
              f"and capture) -> {cfg['output_dir']}/")
        # the split a one-shot run pays once (sampling.py:53-73 is one process per batch of clips): see bench.py cold_start
        ct = eng.cold_times()
        steady = f", later batches {1e3 * min(batch_s[1:]):.1f} ms" if len(batch_s) > 1 else ""
        print(f"cold start: model (host) {t_engine - t_model:.2f} s, engine create + commit {t_ready - t_engine:.2f} s "
              f"(pack {ct[0]:.3f}, upload {ct[1]:.3f}, tables {ct[2]:.3f}), first batch {batch_s[0]:.3f} s "
              f"(graph capture + instantiate {ct[3]:.4f} s, {int(ct[4])} kernel nodes){steady}; "
              f"fused-kernel time-outs healed: {eng.fallbacks}")
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
