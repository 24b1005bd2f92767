/*
 * diffroll_amd.h - C-ABI of the MI355X-native DiffRoll sampling engine.
 *
 * The reference (sony/DiffRoll) has NO plugin / FFI layer: its sampling path sits behind the
 * Python methods of a LightningModule.  This header is therefore the boundary a maintainer
 * would bind UNDER those methods (ctypes stub: INTEGRATION.md).  Each entry point names the
 * reference interface it replaces (paths relative to the reference checkout):
 *
 *   dr_create / dr_set_param / dr_commit   ClassifierFreeDiffRoll.__init__ + load_from_checkpoint
 *                                          (model/diffwave.py:580-635, sampling.py:54-65) and the
 *                                          schedule of SpecRollDiffusion.__init__
 *                                          (task/diffusion.py:239-256)
 *   dr_frontend                            mel_layer -> log -> normalize_spec -> inpainting mask ->
 *                                          trim (model/diffwave.py:643-662, model/utils.py:21-32)
 *   dr_forward                             ClassifierFreeDiffRoll.forward after the front-end
 *                                          (model/diffwave.py:664-686, ResidualBlock :134-151)
 *   dr_step                                cfdg_ddpm_x0 / generation_ddpm_x0 / inpainting_ddpm_x0 /
 *                                          ddpm_x0 (task/diffusion.py:943-1025, :831-853)
 *   dr_sample / dr_sample_checked          the loop of predict_step / sampling
 *                                          (task/diffusion.py:528-534, :779-788)
 *
 * Conventions: plain C, no torch types.  All tensor arguments are BORROWED device pointers to
 * contiguous fp32 (hipMalloc'd / torch ROCm memory on the engine's device); outputs are written
 * into caller-allocated buffers.  `stream` is a hipStream_t passed as void* (e.g.
 * torch.cuda.current_stream().cuda_stream).  Every function returns 0 on success or a negative
 * DR_E* code and never throws; the message is available from dr_last_error().  An engine handle
 * is not re-entrant: one handle per (device, stream), one host thread at a time.
 *
 * This header is the WHOLE boundary (30 functions).  Measurement, checker and test entry points of the same library
 * (dr_profile_*, dr_bench_*, dr_debug_*, dr_stack_status, dr_cold_times, the A/B options "tune.*") are declared in
 * diffroll_amd_debug.h; nothing on the sampling path needs them.
 */
#ifndef DIFFROLL_AMD_H
#define DIFFROLL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DR_ABI_VERSION 11

enum {
    DR_OK = 0,
    DR_EINVAL = -1,   /* bad argument / shape */
    DR_ESTATE = -2,   /* call order (e.g. dr_forward before dr_commit / dr_frontend) */
    DR_EHIP = -3,     /* a HIP runtime call failed (message has the HIP error string) */
    DR_ENOMEM = -4,
    DR_ENAME = -5,    /* unknown parameter name / wrong shape in dr_set_param */
    DR_ETIMEOUT = -6  /* a group barrier of the fused residual-stack kernel ran into its spin bound: the results
                         computed since the last dr_finish are invalid (see dr_finish / dr_sample_checked) */
};

/* samplers: task/diffusion.py, bound at :255 by hparams.sampling.type */
enum {
    DR_SAMPLER_DDPM_X0 = 0,        /* :831-853  one conditional evaluation            */
    DR_SAMPLER_CFDG_DDPM_X0 = 1,   /* :943-969  conditional + unconditional, weight w */
    DR_SAMPLER_GENERATION_DDPM_X0 = 2, /* :971-997  one unconditional evaluation (spec = -1) */
    DR_SAMPLER_INPAINTING_DDPM_X0 = 3, /* :999-1025 as cfdg; spectrogram frames/bins masked by
                                          dr_frontend's mask arguments */
    /* the remaining samplers = the same kernels with other per-step coefficients */
    DR_SAMPLER_DDIM_X0 = 4,            /* :855-875   x0 update with sigma = 0                      */
    DR_SAMPLER_CFDG_DDIM_X0 = 5,       /* :1027-1055 as ddim_x0 with guidance; its second branch is
                                          forward(zero waveform) WITHOUT sampling=True: spec == 0  */
    DR_SAMPLER_DDPM_EPS = 6,           /* :804-829   network output is epsilon ("ddpm")            */
    DR_SAMPLER_DDIM_EPS = 7,           /* :877-892   ("ddim")                                      */
    DR_SAMPLER_DDIM2DDPM_EPS = 8       /* :894-911   ("ddim2ddpm")                                 */
};

/* coefficient families of dr_set_tables' `coef` argument */
enum {
    DR_COEF_DDPM_X0 = 0,   /* [sqrt_acp[t-1], sqrt(1 - sqrt_acp[t-1]^2 - sigma^2), sqrt_acp[t], sqrt_1m_acp[t], sigma] */
    DR_COEF_DDIM_X0 = 1,   /* same with sigma = 0                                                          */
    DR_COEF_DDPM_EPS = 2,  /* [sqrt_recip_alphas[t], betas[t], sqrt_1m_acp[t], sqrt(posterior_variance[t]), 0] */
    DR_COEF_DDIM_EPS = 3,  /* [sqrt_acp[t-1], sqrt_1m_acp[t-1], sqrt_acp[t], sqrt_1m_acp[t], 0]            */
    DR_COEF_DDIM2DDPM_EPS = 4, /* [sqrt_acp[t-1], sqrt(1 - sqrt_acp[t-1]^2 - sigma^2), sqrt_acp[t], sqrt_1m_acp[t], sigma] */
    DR_COEF_FAMILIES = 5
};

/* arithmetic of the two hot contractions (dilated conv, 1x1 output projection); everything else is fp32 */
enum {
    DR_PRECISION_F32 = 0,     /* exact fp32 MFMA (v_mfma_f32_32x32x2_f32): the default                     */
    DR_PRECISION_BF16X3 = 1,  /* opt-in: each fp32 operand is split EXACTLY into three bf16 pieces and a
                                 product is formed from the six piece products with i + j <= 2 on the bf16
                                 MFMA with fp32 accumulation (drops terms <= 2^-24 |ab|); fp32-level error
                                 at 2.67x the matrix rate                                                  */
    DR_PRECISION_BF16 = 2,    /* opt-in: ordinary one-pass bf16.  Rounding happens at exactly the operands
                                 BF16X3 splits - the input x + diffusion_projection and the weights of each
                                 layer's dilated conv, the gated activation sigmoid * tanh and the weights of
                                 each layer's output projection - each rounded ONCE to bf16, round to nearest
                                 even (piece 0 of that split); products are exact (one bf16 MFMA per K step),
                                 accumulation is fp32.  Biases, the conditioner term, the residual stream,
                                 the skip sum and everything outside the residual stack (front-end, embedding,
                                 input / skip / head projections, update) stay fp32 as in BF16X3; nothing is
                                 truncated and no bf16 value is stored where BF16X3 stores fp32.  One sixth
                                 of BF16X3's matrix work, one third of its operand bytes; about 1e-3 rms
                                 error per evaluation on unit-scale activations (README.md)                */
    /* 3 is reserved (a split-f16 near-exact mode would take it); dr_set_precision refuses it              */
    DR_PRECISION_F16 = 4      /* opt-in: ordinary one-pass fp16.  Rounding happens at exactly the four operands
                                 BF16 rounds - the input x + diffusion_projection and the weights of each
                                 layer's dilated conv, the gated activation sigmoid * tanh and the weights of
                                 each layer's output projection - each rounded ONCE to IEEE binary16, round to
                                 nearest even.  Subnormal binary16 values are kept in the conversion, in the
                                 packing and as MFMA operands (gradual underflow; verified on the MI355X by
                                 tests/test_gpu_f16.py); a magnitude of 65520 or more becomes an infinity - the
                                 mode does not saturate; NaN stays NaN; nothing is truncated.  Products of two
                                 binary16 values are exact in fp32 (one v_mfma_f32_32x32x16_f16 per K step) and
                                 accumulation is fp32, blocked as in BF16.  Biases, the conditioner term, the
                                 residual stream, the skip sum, the input / skip / head projections and every
                                 update, statistic and selection kernel stay fp32 as under BF16.  BF16's
                                 layouts, operand bytes and matrix work; 11 significant bits instead of 8:
                                 about 1e-4 rms error per evaluation on unit-scale activations (README.md) */
};

/* which spectrogram a dr_forward evaluation sees (model/diffwave.py:656-660) */
enum {
    DR_COND_SPEC = 0,    /* the spectrogram of the last dr_frontend call   */
    DR_COND_UNCOND = 1   /* sampling=True: spectrogram == -1 everywhere     */
};

/* hyper-parameters: config/model/ClassifierFreeDiffRoll.yaml:1-15, config/task/<task>.yaml,
 * config/spec/mel.yaml:1-10, config/sampling.yaml:1-4 */
typedef struct dr_config {
    int32_t abi_version;        /* DR_ABI_VERSION */
    int32_t device;             /* HIP device ordinal */
    int32_t residual_channels;  /* 512 (multiple of 64) */
    int32_t residual_layers;    /* 15 */
    int32_t kernel_size;        /* odd: 3 / 9 / 15 */
    int32_t dilation_base;      /* 2 */
    int32_t dilation_bound;     /* 4 */
    int32_t n_mels;             /* 229 */
    int32_t timesteps;          /* 200 */
    int32_t sample_rate;        /* 16000 */
    int32_t n_fft;              /* 2048 (multiple of 32) */
    int32_t hop_length;         /* 512  (multiple of 4) */
    float f_min;                /* 0 */
    float f_max;                /* 8000 */
    float beta_start;           /* 1e-4  (informational; the coefficient table is passed in) */
    float beta_end;             /* 0.02 */
} dr_config;

typedef struct dr_engine dr_engine;

/* version of the loaded library (== DR_ABI_VERSION of the header it was built with) */
int dr_abi_version(void);

int dr_create(dr_engine** out, const dr_config* cfg);
void dr_destroy(dr_engine* e);
const char* dr_last_error(const dr_engine* e);   /* e may be NULL: error of the last dr_create */

/*
 * Hand over one parameter tensor by its reference state_dict name, in the
 * reference's own layout, from HOST memory (copied):
 *   input_projection.{weight (C,88,1), bias (C)}
 *   diffusion_embedding.projection1.{weight (512,128), bias}, .projection2.{weight (512,512), bias}
 *   residual_layers.<i>.dilated_conv.{weight (2C,C,k), bias (2C)}
 *   residual_layers.<i>.diffusion_projection.{weight (C,512), bias (C)}
 *   residual_layers.<i>.conditioner_projection.{weight (2C,n_mels,1), bias (2C)}
 *   residual_layers.<i>.output_projection.{weight (2C,C,1), bias (2C)}
 *   skip_projection.{weight (C,C,1), bias (C)},  output_projection.{weight (88,C,1), bias (88)}
 * numel must match the shape implied by the config.  Unknown names -> DR_ENAME.
 */
int dr_set_param(dr_engine* e, const char* name, const float* host_data, size_t numel);

/*
 * Host-built tables (same torch expressions as the reference, so bit-equal):
 *   embedding  (timesteps, 128)  DiffusionEmbedding._build_embedding (model/diffwave.py:83-88)
 *   coef       (DR_COEF_FAMILIES, timesteps, 5)  per-step scalars of the samplers' updates
 *                                (task/diffusion.py:957-967 and :804-911), one table per coefficient
 *                                family, columns as listed at the DR_COEF_* enum; row 0 of the x0
 *                                families only uses column 2 (x = x0 / sqrt_acp[0]).
 */
int dr_set_tables(dr_engine* e, const float* host_embedding, const float* host_coef);

/*
 * Constants of the mel front-end built by the caller WITH THE REFERENCE'S ARITHMETIC (torchaudio 0.11
 * MelSpectrogram, model/diffwave.py:635): host_window (n_fft) = torch.hann_window(n_fft), window_norm =
 * window.pow(2).sum().sqrt() (normalized=True divides the spectrum by it), host_fb (n_fft/2+1, n_mels) row-major =
 * torchaudio.functional.melscale_fbanks(..., norm=None, mel_scale='htk').  torchaudio evaluates these in fp32 and
 * the rounding of the filterbank is visible (2e-5 in the normalised log-mel), so parity needs the same tables:
 * diffroll_amd/frontend_tables.py builds them with the same torch expressions.  Optional: without this call (or
 * with NULL tables) dr_commit evaluates the published formulas itself, in double precision.
 */
int dr_set_frontend_tables(dr_engine* e, const float* host_window, float window_norm, const float* host_fb);

/* Pack weights for the kernels, upload, and build the hoisted tables on the device (the
 * (timesteps, layers, C) step-embedding projections; the unconditional conditioner constants).
 * Requires every parameter and both tables.  Synchronises `stream`. */
int dr_commit(dr_engine* e, void* stream);

/*
 * Front-end, once per clip batch.  d_wav (B, L) -> d_spec_out (B, n_mels, T) with
 * T = min(T_roll, L / hop + 1); also builds the per-layer conditioner tensors the residual
 * blocks consume, for this batch.  Mask: spectrogram[f0:f1, t0:t1] = -1 after normalisation
 * (pass t0 = t1 = -1 / f0 = f1 = -1 for "no mask on that axis"; model/diffwave.py:649-654).
 * d_spec_out may be NULL.
 */
int dr_frontend(dr_engine* e, const float* d_wav, int B, int L, int T_roll,
                int mask_t0, int mask_t1, int mask_f0, int mask_f1,
                float* d_spec_out, void* stream);

/* One network evaluation at diffusion step t: d_x (B, T, 88) [the reference's (B,1,T,88)] ->
 * d_x0_out (B, T, 88).  cond = DR_COND_SPEC needs a preceding dr_frontend with the same B, T. */
int dr_forward(dr_engine* e, const float* d_x, int B, int T, int t, int cond,
               float* d_x0_out, void* stream);

/* The same with one diffusion step PER SAMPLE (host_t: B ints on the host), the general form of the reference's
 * forward(x_t, waveform, diffusion_step (B,)) as its training / validation step() calls it; the samplers always
 * pass one step for the whole batch.  Synchronises `stream` (the step vector is uploaded). */
int dr_forward_steps(dr_engine* e, const float* d_x, int B, int T, const int32_t* host_t, int cond,
                     float* d_x0_out, void* stream);

/* One reverse-diffusion step t (in place on d_x).  d_noise (B, T, 88) is the z of that step
 * (ignored at t == 0); NULL -> on-device Philox keyed by (seed, first_sample + b, t). */
int dr_step(dr_engine* e, int sampler, float* d_x, const float* d_noise, int B, int T, int t,
            float w, uint64_t seed, int first_sample, void* stream);

/*
 * The whole reverse chain t = timesteps-1 .. 0 (or the visited steps of option "sampling_steps"), in place on d_x, no
 * host synchronisation.
 * d_noise: (timesteps, B, T, 88) injected noise (row t used at step t >= 1) or NULL for Philox.
 * use_graph != 0: the chain is captured once into a hipGraph and replayed; the graph is cached per
 * (sampler, B, T, d_noise): the chain runs on an engine-owned copy of d_x, and w, seed and first_sample are
 * read from a device block at run time, so new buffers / values re-use the instantiated graph.  Needs dr_frontend first unless sampler == DR_SAMPLER_GENERATION_DDPM_X0.
 */
int dr_sample(dr_engine* e, int sampler, float* d_x, const float* d_noise, int B, int T,
              float w, uint64_t seed, int first_sample, int use_graph, void* stream);

/*
 * Consume point of asynchronous results.  The fused residual-stack kernel (option "fused_stack") assumes that all
 * its workgroups are resident on the device at once; when something else holds CUs while it runs (a second engine,
 * stream or process computing on the same device) a group barrier can run into its spin bound - the launch then
 * carries on with wrong data, raises a flag, and every later fused launch of the engine returns immediately.
 * (An engine avoids most of these BEFORE it launches.  Engines of one process take turns on a per-device slot: the one
 * that finds another engine's fused work still in flight orders its own launches behind it on the device (a stream
 * wait on an event: no host wait, nobody gives up fusing).  And dr_create / dr_sample look for another PROCESS computing
 * on the GPU in the kernel driver's process list (/sys/class/kfd/kfd/proc: csrc/tenants.h): if there is one the engine
 * YIELDS - one launch per phase from then on, same results, one line on stderr, counted in dr_launch_state - and goes
 * back to fused launches once two looks in a row, in front of later chains, find the GPU its own again.  The spin bound
 * remains the backstop for what those checks cannot see: a tenant that arrives in the middle of a chain.)
 * dr_finish synchronises `stream` and checks that flag:
 *   DR_OK        everything issued on this engine since the last check is valid;
 *   DR_ETIMEOUT  it is NOT: recompute it.  The condition has been cleared and the engine switched to one launch per
 *                phase (fused_stack = 0: bit-identical results, no residency assumption), so the recomputation
 *                cannot time out again; re-enable with dr_set_option when the device is the engine's own again.
 * Call it before a roll produced by dr_forward / dr_step / dr_sample is used (copied to the host, written as MIDI,
 * gathered).  While an unchecked time-out is pending every entry point that COMPUTES (dr_forward, dr_forward_steps,
 * dr_step, dr_sample) refuses to start, and every entry point that CONSUMES a roll given an engine handle
 * (dr_note_runs, dr_frame_counts, dr_q_sample / dr_extract_x0, dr_gather) first does what dr_pending_timeout does -
 * it synchronises the stream the fused launches ran on (and `stream`) if any have been issued since the last check - and
 * returns DR_ETIMEOUT instead of working on an invalid roll; dr_gather still takes part in the collective first (a time-out
 * is a per-rank event: a rank that stayed out would leave its peers blocked) and reports DR_ETIMEOUT afterwards - ON EVERY
 * RANK (a status word travels with the rolls): every rank must gather again after the invalid shard has been recomputed.
 * Only dr_finish clears the condition.
 */
int dr_finish(dr_engine* e, void* stream);
/* The check alone: DR_ETIMEOUT when a fused launch issued on this engine has timed out and dr_finish has not been called
 * since; DR_OK otherwise.  Synchronises `stream` only when fused launches have been issued since the last check (so that
 * the flag is final); does not heal, does not clear.  `e` may be NULL (DR_OK). */
int dr_pending_timeout(dr_engine* e, void* stream);
/* dr_sample + dr_finish + (on a time-out) the re-run of the chain from the same x_T on the per-phase kernels:
 * returns DR_OK only with the correct roll in d_x.  Synchronous.  *recovered (optional) = 1 when the re-run was
 * needed.  This is what a one-shot caller (sampling.py, predict_step) should use: task/diffusion.py:528-538 returns
 * a finished roll, never a silently invalid one. */
int dr_sample_checked(dr_engine* e, int sampler, float* d_x, const float* d_noise, int B, int T,
                      float w, uint64_t seed, int first_sample, int use_graph, int32_t* recovered, void* stream);
/*
 * How this engine launches the residual layers, and what has happened to that decision - the record a measurement
 * must check (bench.py refuses to print a line when `fallbacks` or `yields` moved during its timed region):
 *   mode          DR_MODE_* of the most recently planned network evaluation (a captured chain: at capture)
 *   fused_enabled the current value of option "fused_stack" (0 while the engine runs per-phase launches after a
 *                 time-out or a yield)
 *   fallbacks     time-outs dr_finish has detected and healed (each switched the engine to per-phase launches)
 *   yields        times the engine gave up fusing BEFORE launching because another process was found computing on
 *                 its GPU (csrc/tenants.h); same results, one launch per phase from then on
 *   rearms        times fused launches were switched back on (after "fused_rearm" clean chains behind a time-out, or
 *                 two clean looks behind a yield)
 *   stack_launches / tail_launches   persistent launches issued so far (a captured chain counts once, at capture)
 */
enum { DR_MODE_NONE = 0, DR_MODE_PER_PHASE = 1, DR_MODE_FUSED_STACK = 2, DR_MODE_FUSED_STACK_TAIL = 3 };
typedef struct dr_launch_info {
    int32_t mode;
    int32_t fused_enabled;
    int64_t fallbacks;
    int64_t yields;
    int64_t rearms;
    int64_t stack_launches;
    int64_t tail_launches;
} dr_launch_info;
int dr_launch_state(dr_engine* e, dr_launch_info* out);

/*
 * Roll -> notes, the scan of extract_notes_wo_velocity (task/diffusion.py:1185-1233) as the reference's
 * drivers call it (onsets == frames == the roll, one threshold, rule1): d_note_end (B, T, 88) int32
 * receives, at every (frame, pitch) where a note STARTS, the frame index at which it ends (exclusive),
 * and 0 elsewhere.  np.nonzero() of that tensor enumerates the notes in the reference's order.
 */
int dr_note_runs(dr_engine* e, const float* d_roll, int B, int T, float threshold, int32_t* d_note_end,
                 void* stream);

/*
 * Frame-level evaluation of test_step (task/diffusion.py:381-383): confusion counts of
 * (d_pred > threshold) against the binary label roll over n elements, the integers sklearn's
 * precision_recall_fscore_support(average='binary') is computed from.  host_counts = {TP, FP, FN}.
 * Synchronises `stream`.
 */
int dr_frame_counts(dr_engine* e, const float* d_pred, const float* d_label, size_t n, float threshold,
                    int64_t* host_counts, void* stream);

/*
 * The forward-process arithmetic of task/diffusion.py (free functions, used by step() around the network):
 *   dr_q_sample   (:31-46)  out = sqrt_alphas_cumprod[t_b] * x_start + sqrt_one_minus_alphas_cumprod[t_b] * noise
 *   dr_extract_x0 (:49-64)  out = (x_t - sqrt_one_minus_alphas_cumprod[t_b] * epsilon) / sqrt_alphas_cumprod[t_b]
 * d_t (B,) int64 per-sample step indices, d_sac / d_s1m the two schedule vectors (n_steps,) - all on the
 * device; tensors are (B, per_sample) contiguous fp32.  Same operation order and roundings as the reference's
 * broadcasted torch expression (bit-exact).  Step indices are clamped to [0, n_steps).  `e` may be NULL (no
 * engine state is involved: current device, error text via dr_last_error(NULL)).
 */
int dr_q_sample(dr_engine* e, const float* d_x_start, const float* d_noise, const int64_t* d_t,
                const float* d_sac, const float* d_s1m, int n_steps, int B, size_t per_sample, float* d_out,
                void* stream);
int dr_extract_x0(dr_engine* e, const float* d_x_t, const float* d_epsilon, const int64_t* d_t,
                  const float* d_sac, const float* d_s1m, int n_steps, int B, size_t per_sample, float* d_out,
                  void* stream);

/* Spectrogram normalisation of the following dr_frontend calls: the mode of Normalization(0, 1, norm_args[2])
 * (model/diffwave.py:632, model/utils.py:10-32) - min-max per clip ("imagewise", the default and the released
 * configs) or per frame over the frequency bins ("framewise"). */
#define DR_NORM_IMAGEWISE 0
#define DR_NORM_FRAMEWISE 1
int dr_set_spec_norm(dr_engine* e, int mode);

/* Select DR_PRECISION_* for subsequent dr_forward / dr_step / dr_sample calls (default F32).
 * Drops a captured chain.  BF16X3, BF16 and F16 each build their own weight packing the first time they are
 * selected (none builds another's); the mode changes only once that packing exists.  Any other value -
 * the reserved 3 included - is DR_EINVAL and leaves the engine as it was. */
int dr_set_precision(dr_engine* e, int mode);

/*
 * Integer options (defaults in brackets).  Changing one drops a captured chain.
 *   "blocked_accumulation" [2] accumulation order of the dilated conv's K = taps x channels contraction
 *                          (model/diffwave.py:144 as a CPU library executes it: K-blocked): 2 = one fp32 MFMA chain per
 *                          32-channel block, block sums added up in block order, in every fp32 kernel flavour (against
 *                          float64 the error is 1.0-1.6x the CPU fp32 reference's in the trained-weight regime);
 *                          1 = the 128-frame blocks and the 96 / 160-frame flavours contract all of K as ONE chain (the
 *                          numerics of ABI <= 7: 0.2-0.8 % faster, 3.0-3.9x; 1.0 % faster in the split-bf16 precision).
 *   "fused_rearm"      [0] n > 0: after a time-out has switched this engine to per-phase launches, go back to the fused
 *                          kernels once n chains in a row have finished cleanly (a time-out caused by a transient
 *                          tenant - a profiler, a second process that has left - then costs n chains at the per-phase
 *                          pace instead of the rest of the engine's life).  0 = stay on per-phase launches until
 *                          "fused_stack" is set again.  Seeded results after a recovery can differ from a healthy fused
 *                          run in the last bits (the per-phase launches split K where the fused kernel does not).
 *   "fused_stack"      [1] the residual layers of an evaluation (model/diffwave.py:678-681: 15 x ResidualBlock.forward,
 *                          :134-151) run as ONE persistent launch whenever samples x frame tiles x M tiles fits the
 *                          chip's CUs in one resident round (the BASELINE configurations 2-5 do: 64 / 128 / 160-frame blocks); 0 = one launch per
 *                          dilated conv and per 1x1 (bit-identical results, 2 x residual_layers launches); 2 = fuse
 *                          also launches that fill less than half the chip (tests).
 *   "fused_tail"       [1] where the evaluation is one fused launch, the REST of a reverse
 *                          step is fused too (model/diffwave.py:667-668, :682-686; task/diffusion.py:953-967): skip
 *                          projection, output projection, combine + posterior update, the NEXT step's input projection
 *                          and - under classifier-free guidance - the next step's first-layer dilated conv (the same
 *                          contraction for the conditional and the unconditional evaluation: done once per pair) run as
 *                          one persistent "tail" launch, and the following stack launch starts at that layer's 1x1:
 *                          2 launches per reverse step instead of 6 (the first step of a chain still runs its input
 *                          projection and first-layer conv as launches of their own).  0 = separate launches
 *                          (bit-identical without split-K).
 *   "window_overlap"   [0] O > 0: long-form transcription.  The B rolls of dr_step / dr_sample / dr_sample_checked are B
 *                          consecutive T-frame windows of ONE recording, window b starting at frame b * H (H = T - O) of
 *                          a canvas of (B - 1) * H + T frames; at every reverse step a frame shared by windows b and
 *                          b + 1 (frames [H, T) of b, [0, O) of b + 1) takes 0.5f * (y_b + y_b+1), the mean of the two
 *                          windows' guided x0 predictions, before the posterior update (MultiDiffusion, Bar-Tal et al.
 *                          2023), and Philox noise is keyed (seed, first_sample = the recording, t, canvas element / 4);
 *                          injected noise rows are used as given.  If x_T agrees on shared frames, every x_t does, bit for
 *                          bit: the stitched roll is a plain gather from the canvas.  O > T / 2 -> DR_EINVAL at the call
 *                          (at most two windows share a frame).  dr_forward / dr_forward_steps are unaffected; 0 = off
 *                          (every clip on its own, bit-identical to an engine that never set it).
 *   "window_break"    [-]  recording boundaries inside a window batch: SEVERAL recordings in one chain.  Value b >= 1 marks
 *                          window b of the next dr_step / dr_sample / dr_sample_checked batches as the FIRST window of a new
 *                          recording (marks accumulate; window 0 always starts one); value 0 clears all marks; a negative
 *                          value -> DR_EINVAL.  Marks are engine state like "window_overlap" and are ignored while that is
 *                          0.  With marks m_1 < m_2 < ... window b belongs to recording r(b) = the number of marks <= b
 *                          and is window i(b) = b - (first window of r(b)) of that recording's own canvas: windows b and
 *                          b + 1 share frames only if r(b) == r(b + 1), and Philox is keyed (seed, first_sample + r(b), t,
 *                          (i(b) * H * 88 + element within the window) / 4) - every recording gets exactly the roll of a
 *                          chain of its own with first_sample + r.  No marks = one recording, the definition above.  A mark
 *                          >= B -> DR_EINVAL at the call (and a batch with marks holds at most 512 windows).  The marks are
 *                          data of a captured chain, not part of it: setting them does NOT drop it, and a new
 *                          segmentation at the same (sampler, B, T) replays the same graph.  dr_sample_checked's re-run
 *                          uses the same marks; dr_forward / dr_forward_steps are unaffected.
 *   "window_blend"     [0] 0, 1 or 2: WHAT A SHARED FRAME TAKES of the two windows' predictions under "window_overlap"
 *                          (ignored while that is 0).  With O the overlap, H = T - O and j = 0 .. O - 1 the position within
 *                          the overlap, frame H + j of the lower window b is frame j of the upper window b + 1; y_lo and
 *                          y_up are the two windows' guided predictions of it.  0 = the mean 0.5f * (y_lo + y_up), the
 *                          definition above: not a bit changes.  1 = LINEAR CROSS-FADE: wu = (float)(j + 1) / (float)(O + 1),
 *                          y = y_lo + wu * (y_up - y_lo) - subtraction, product and sum each rounded once, in that order
 *                          (no FMA); where y_lo == y_up the result is that value exactly.  Each window's weight falls
 *                          towards its own edge, where its dilated convolutions see zero padding instead of context (the
 *                          tapered window weights of tiled diffusion).  2 = HAND-OVER: y = j < (O + 1) / 2 ? y_lo : y_up
 *                          (integer division), a select: every canvas frame from the window whose centre is nearer, the
 *                          lower window taking the odd frame.  Both windows evaluate the same expression on the same
 *                          operands, lower first, so the frames they share stay bit-identical in every mode and the
 *                          stitched roll stays a plain gather.  Whatever read the mean reads the blended value: both
 *                          terms of every update (the epsilon samplers blend their epsilon), the clamp of "x0_clip", the
 *                          selection and the update of "x0_threshold" (every canvas frame still counted once), the d and
 *                          the history of "solver_order", the last step.  "window_break" is respected - only windows of
 *                          one recording blend - and "draws" blends per draw; noise keys, the diffusion of "start_noise",
 *                          dr_forward and dr_forward_steps are untouched.  Modes 1 and 2 keep the tail kernel of
 *                          "fused_tail" (cost: profiles/blend_sweep.txt).  Any other value -> DR_EINVAL at the set.  While
 *                          "window_overlap" is set the value is part of a captured chain's key, like "x0_clip": setting
 *                          it drops nothing, and a chain captured under another value is never replayed; while the
 *                          overlap is 0 it is inert and makes no other chain.  A change of the value ends a dr_step
 *                          history of "solver_order" 2, as a change of "x0_clip" does.  Nothing is known about what the
 *                          modes do to quality with real weights.
 *   "sampling_steps"   [0] n, 2 <= n < timesteps (S): a RESPACED reverse chain of n network steps instead of S.  Visited
 *                          steps t_i = (2 i (S - 1) + (n - 1)) / (2 (n - 1)) in integer arithmetic (linspace rounded half
 *                          up), i = n-1 .. 0: strictly decreasing from S - 1 to 0; t' = the next visited step.  The row of
 *                          step t: the committed row t unchanged when t == 0 or t' == t - 1; otherwise one derived in double
 *                          precision from the committed fp32 A = sqrt_acp[t], Ap = sqrt_acp[t'], Sm = sqrt_1m_acp[t], Smp =
 *                          sqrt_1m_acp[t'] (columns 2 and 3 of DR_COEF_DDPM_X0) and rounded to fp32 once - with
 *                          sigma = (Smp / Sm) sqrt(1 - (A / Ap)^2) and beta' = 1 - (A / Ap)^2:
 *                            DR_COEF_DDPM_X0, DR_COEF_DDIM2DDPM_EPS  [Ap, sqrt(max(0, 1 - Ap^2 - sigma^2)), A, Sm, sigma]
 *                            DR_COEF_DDIM_X0                         [Ap, sqrt(1 - Ap^2), A, Sm, 0]
 *                            DR_COEF_DDPM_EPS                        [Ap / A, beta', Sm, sqrt(beta' Smp^2 / Sm^2), 0]
 *                            DR_COEF_DDIM_EPS                        [Ap, Smp, A, Sm, 0]
 *                          (the stride-1 rows of the same formulas, mathematically).  Noise stays keyed by the real t: Philox
 *                          by (seed, sample, t), injected noise keeps its (S, B, T, 88) shape and row t is used at visited
 *                          step t - a respaced chain draws exactly the z's the full chain draws at those steps.  Applies to
 *                          dr_sample / dr_sample_checked (whose re-run uses the same steps) and dr_step (a t that is not
 *                          visited -> DR_EINVAL); dr_forward, dr_forward_steps, dr_q_sample, dr_extract_x0 are unaffected.
 *                          Combines with "window_overlap", both precisions and sharding.  0 or S = the full chain, bit for
 *                          bit; any other value -> DR_EINVAL.
 *   "draws"            [1] D >= 1: SEVERAL draws per clip in one chain, sharing the conditioning.  The B rolls of dr_step /
 *                          dr_sample / dr_sample_checked (and dr_forward / dr_forward_steps) are D draws of n = B / D clips,
 *                          draw-major: row b is draw b / n of clip b % n.  The preceding dr_frontend was called with the n
 *                          clips (its outputs stay at n clips); conditional row b reads conditioner tensor b % n, and the
 *                          conditional / unconditional halves of a guided batch keep their meaning.  B % D != 0 ->
 *                          DR_EINVAL, a front-end batch other than B / D for a conditional sampler -> DR_ESTATE, at the
 *                          call.  The result is, bit for bit, that of the same rolls after a front-end run on the waveform
 *                          tiled D times - without D copies of the conditioner tensors.  Injected noise keeps its
 *                          (S, B, T, 88) shape, one row per roll.  With "window_overlap" the rows of ONE draw are the window
 *                          batch: a new draw always starts new recordings (no averaging across a draw boundary),
 *                          "window_break" marks are those of one draw (a mark >= n -> DR_EINVAL) and repeat per draw, draw
 *                          d of recording r is keyed first_sample + r + d * R (R = the recordings of one draw, or
 *                          "draw_stride") - exactly the chain of first_sample + d * R - and B, the whole batch, holds at
 *                          most 512 windows.  1 = every roll its own clip, bit-identical to an engine that never set it;
 *                          < 1 -> DR_EINVAL.  The value is part of a captured chain's key: a chain captured under another
 *                          value is never replayed (the next dr_sample captures anew), and setting the option back
 *                          before the next call costs nothing - nothing in flight is touched.
 *   "draw_stride"      [0] G >= 0: the Philox sample key of row b under "draws" is first_sample + (b % n) + (b / n) * G, with
 *                          0 = n (then the key is first_sample + b, that of the tiled batch).  A sharded run sets G to the
 *                          global clip count: draw d of global clip c gets the same noise on any world size.  Ignored
 *                          while "draws" is 1; < 0 -> DR_EINVAL.  Part of a captured chain's key, like "draws".
 *   "guidance_t_min"   [0] lo, 0 <= lo < timesteps, and
 *   "guidance_t_max"  [-1] hi, -1 (= timesteps - 1) or 0 <= hi < timesteps: the GUIDANCE INTERVAL (limited-interval
 *                          guidance).  A reverse step at the real diffusion step t of a sampler that guides
 *                          (DR_SAMPLER_CFDG_DDPM_X0, _INPAINTING_DDPM_X0, _CFDG_DDIM_X0) is guided iff lo <= t <= hi: it is
 *                          then exactly the step with the caller's w.  Every other step is exactly the step with w = 0:
 *                          only the conditional evaluation of the B rolls runs (B network evaluations instead of 2 B) and the
 *                          update consumes it unchanged - (1 + 0) c - 0 u == c, so no value changes by not computing u.  It
 *                          is the reference's own sampler run with a per-step weight, w inside [lo, hi] and 0 outside.  The
 *                          defaults guide the whole chain, bit-identical to an engine that never set the options; the other
 *                          six samplers ignore both; w == 0 stays what it is whatever the interval.  A value out of range
 *                          -> DR_EINVAL at the set; an effective lo > hi -> DR_EINVAL at the next dr_step / dr_sample /
 *                          dr_sample_checked with a guiding sampler, naming both values.  Under "sampling_steps" the test
 *                          uses the real t of each visited step (the derived rows are untouched); under "window_overlap" /
 *                          "window_break" a step is guided or not for all windows alike, and the shared-frame mean is taken
 *                          of whichever prediction the step uses; combines with "draws" / "draw_stride", both precisions and
 *                          sharding (every rank sets the same interval).  dr_step: step t alone follows the rule;
 *                          dr_sample_checked's re-run uses the same interval; dr_forward, dr_forward_steps, dr_q_sample,
 *                          dr_extract_x0 are unaffected.  Philox keys and injected-noise rows are unchanged.  The effective
 *                          pair is part of a captured chain's key, like "draws": setting the options drops nothing, and a
 *                          chain captured under another interval is never replayed.  Nothing is known about the quality
 *                          of a limited interval with this model.
 *   "solver_order"     [0] 0, 1 or 2: how the x0-prediction samplers (DR_SAMPLER_* 0-5) INTEGRATE their prediction - a
 *                          multistep ODE solver for few-step chains (Lu et al. 2022, DPM-Solver++), orthogonal to the
 *                          sampler: the sampler keeps deciding which evaluations run (conditional, guided, unconditional,
 *                          inpainting mask, zero-spectrogram branch).  0 = the sampler's own update, bit-identical to an
 *                          engine that never set the option.  1 = the first-order exponential integrator in
 *                          lambda_t = log(A_t / Sm_t), A = sqrt_acp, Sm = sqrt_1m_acp; 2 = DPM-Solver++ (2M).  For a
 *                          visited step t > 0 with successor t' and predecessor t'' in the chain (the full chain, or the
 *                          visited steps of "sampling_steps" - the intended use), h = lambda_t' - lambda_t, h_prev =
 *                          lambda_t - lambda_t'', the row is [Smp / Sm, -Ap expm1(-h), A, c, 0] with c = h / (2 h_prev)
 *                          when the order is 2, t is not the chain's first step and t' != 0, else c = 0 (the step into 0
 *                          is always first order); the row of step 0 is [0, 0, A_0, 0, 0].  Rows are derived in double
 *                          from the committed fp32 A and Sm (columns 2 and 3 of DR_COEF_DDPM_X0), rounded to fp32 once, and
 *                          kept in a table of their own: dr_set_tables' shape is unchanged.  With y the step's (guided)
 *                          prediction and p that of the previous step: d = c != 0 ? y + c (y - p) : y, x' = c0 x + c1 d,
 *                          one fp32 rounding per operation; at t == 0 x' = y / c2, the x0 samplers' own last step.  The
 *                          chain is DETERMINISTIC: no noise is drawn, d_noise is ignored, and "draws" differ through x_T
 *                          only - unless "solver_noise" is 1 (the stochastic form: see there).  An epsilon sampler (DR_SAMPLER_* 6-8) with a non-zero order -> DR_EINVAL at dr_step /
 *                          dr_sample / dr_sample_checked, naming both; any other value -> DR_EINVAL at the set.  Order 2
 *                          keeps p in two engine-owned (B, T, 88) buffers (allocated on first use).  dr_step: at the
 *                          chain's first visited step it starts a new history; at any other visited step the previous
 *                          dr_step must have been the preceding visited step of the same (sampler, B, T), else
 *                          DR_ESTATE naming the step expected; order 1 needs no history and runs any visited step.
 *                          dr_sample, a healed time-out, and a change of "sampling_steps", "window_overlap" or "draws" end
 *                          a dr_step history; dr_sample_checked's re-run starts its own.  Combines with
 *                          "sampling_steps"; with "window_overlap" / "window_break" (y and p are the shared-frame means,
 *                          so shared frames stay bit-identical in both windows); with "draws" / "draw_stride"; with
 *                          "guidance_t_min" / "guidance_t_max" (p is whichever prediction the previous step used); with
 *                          both precisions and with sharding (every rank sets the same order).  dr_forward,
 *                          dr_forward_steps, dr_q_sample, dr_extract_x0 are unaffected.  The value is part of a captured
 *                          chain's key, like "draws": setting it drops nothing, and a chain captured under another value
 *                          is never replayed.  Nothing is known about the quality of either order with this model
 *                          (INTEGRATION.md 3c).
 *   "solver_noise"     [0] 0 or 1: 1 makes the solver of "solver_order" 1 / 2 STOCHASTIC (SDE-DPM-Solver++ of the same paper,
 *                          first order and 2M) - the second-order companion of the ddpm_x0 update for few-step chains
 *                          ("sampling_steps").  Stored always; it takes effect only while "solver_order" is 1 or 2 (as
 *                          "draw_stride" is inert while "draws" is 1; the epsilon samplers are refused under a non-zero
 *                          order already).  In the notation of "solver_order" the row of a visited step t > 0 becomes
 *                          [(Smp / Sm) exp(-h), Ap (-expm1(-2h)), A, c, Smp sqrt(-expm1(-2h))], c by the same rule; row 0
 *                          stays [0, 0, A_0, 0, 0]; derived in double from the committed fp32 A and Sm and rounded to fp32
 *                          once, in the same table.  The update is d = c != 0 ? y + c (y - p) : y,
 *                          x' = (c0 x + c1 d) + c4 z at t > 0 and x' = y / c2 at t == 0, one fp32 rounding per operation.
 *                          z is the z the DDPM-family updates draw at that step: row t of d_noise when that is given, else
 *                          Philox keyed exactly as DR_SAMPLER_DDPM_X0 keys it - counter word 2 = the real t, sample key
 *                          and element by clip, "draws" / "draw_stride", or recording and canvas element under
 *                          "window_overlap" / "window_break".  So a stochastic solver chain draws exactly the z's the
 *                          ddpm_x0 chain draws at those steps; frames shared by two windows stay bit-identical; draw d of
 *                          clip c gets the same noise on any world size; dr_sample_checked's re-run reproduces the same
 *                          chain; "start_noise" keeps its own, independent draw (counter word timesteps + t_s).  With
 *                          A^2 + Sm^2 = 1 the first-order stochastic update IS the ddpm_x0 update of the derived
 *                          "sampling_steps" row by another arithmetic route: c4^2 = Smp^2 (1 - exp(-2h)) =
 *                          (Smp / Sm)^2 (1 - A^2 / Ap^2) = sigma^2 and c0 = sqrt(1 - Ap^2 - sigma^2) / Sm - as order 1
 *                          without noise is ddim_x0 by another route; what the option adds is the second order.  The
 *                          order-2 history rules of dr_step are unchanged; "start_step" resumes a first-order chain bit
 *                          for bit, as it does without noise.  Combines with "sampling_steps", "window_overlap" /
 *                          "window_break", "draws" / "draw_stride", "guidance_t_min" / "guidance_t_max", "start_step" /
 *                          "start_noise", both precisions and sharding (every rank sets the same value).  0 = the
 *                          deterministic solver, bit-identical to an engine that never set the option, in every mode.
 *                          Any other value -> DR_EINVAL at the set.  The value is part of a captured chain's key, like
 *                          "solver_order": setting it drops nothing, and a chain captured under another value is never
 *                          replayed.  Nothing is known about the quality of the stochastic solver with this model: the
 *                          one measurement is of the integrator on a Gaussian toy prior.
 *   "start_step"      [-1] t_s, -1 or 0 <= t_s < timesteps: START the reverse chain at an intermediate step.  dr_sample /
 *                          dr_sample_checked run the visited steps t <= t_s in chain order, and d_x on entry is x at step
 *                          t_s - a row of an earlier chain's trajectory (resume), or a roll diffused to t_s ("start_noise";
 *                          SDEdit, Meng et al. 2022).  -1 = the chain's first visited step: off, bit-identical to an engine
 *                          that never set the option.  Any other value -> DR_EINVAL at the set; a t_s that the chain does
 *                          not visit (the full chain, or the steps of "sampling_steps") -> DR_EINVAL at the call, naming t_s
 *                          and the visited steps on either side of it.  Nothing else moves: coefficient rows, the guidance
 *                          interval test, Philox keys and injected-noise rows stay keyed by the real t, so a started chain
 *                          draws exactly the z's the whole chain draws at those steps - a chain resumed from the whole
 *                          chain's x at t_s ends in the whole chain's roll, bit for bit (orders 0 and 1).  Under
 *                          "solver_order" 2 the started chain's first step is first order (c = 0) and starts a new
 *                          history, as the whole chain's first step does - it reads a copy of its row with c = 0, kept
 *                          beside the table, so no row that another captured chain reads is touched; the step into 0 stays
 *                          first order; dr_step at t == t_s starts a history too.  dr_step, dr_forward, dr_forward_steps,
 *                          dr_q_sample, dr_extract_x0 are otherwise unaffected.  Combines with "sampling_steps",
 *                          "window_overlap" / "window_break", "draws" / "draw_stride", "guidance_t_min" / "guidance_t_max",
 *                          both precisions and sharding (every rank sets the same step).  The effective start is part of
 *                          a captured chain's key, like "draws": setting it drops nothing, and a chain captured under
 *                          another start is never replayed.  Nothing is known about the quality of a started chain with
 *                          this model.
 *   "start_noise"      [0] 0 or 1.  1: d_x on entry to dr_sample / dr_sample_checked is a CLEAN roll x0 in the model's roll
 *                          space, and the chain's first node diffuses it to the start step t_s ("start_step"; -1: the
 *                          chain's first visited step) in place on the buffer the chain runs on: x = (A * x0) + (Sm * z),
 *                          A = sqrt_acp[t_s], Sm = sqrt_1m_acp[t_s], the committed fp32 values (columns 2 and 3 of
 *                          DR_COEF_DDPM_X0), rounded as dr_q_sample rounds - each product once, then the sum.  z is row 0
 *                          of d_noise when that is given (no reverse step reads it), else Philox with the chain's seed and
 *                          counter word 2 = timesteps + t_s (the steps use t < timesteps: the draws are independent of
 *                          every step's z), sample key and element as the steps' own draws take them under "draws" /
 *                          "draw_stride" / "window_overlap" / "window_break" - windows are keyed by recording and canvas
 *                          element: if x0 agrees on the frames two windows share, so does x at t_s, bit for bit.  Under
 *                          "solver_order" != 0 this is the one place that still draws (unless "solver_noise" is 1: the
 *                          steps then draw their own z's, independent of this one).  dr_sample_checked keeps what the
 *                          caller passed - x0 - so its re-run diffuses again with the same z.  dr_step ignores the
 *                          option: it takes x at its step.  Any other value -> DR_EINVAL.  Part of a captured chain's key,
 *                          like "draws".
 *   "x0_clip"          [0] 0, 1 or 2: CLAMP the x0 prediction every update consumes to the range the rolls were normalised
 *                          to - 1 = [0, 1] (every released config), 2 = [-1, 1] - the static "clip_denoised" of the DDPM
 *                          code bases and the static thresholding DPM-Solver++ was published with (Lu et al. 2022), the
 *                          companion of strong guidance and short chains: under guidance the prediction (1 + w) c - w u
 *                          is an extrapolation and leaves that range.  0 = off, bit-identical to an engine that never set
 *                          the option, on every path.  The clamp applies to exactly one value: the step's prediction y
 *                          after the classifier-free combine and after the shared-frame mean of "window_overlap",
 *                          y = y < lo ? lo : (y > hi ? hi : y) (a NaN stays a NaN).  Everything behind it reads the
 *                          clamped y: both terms of the x0 samplers' own update; the last step's x' = y / c2, so a
 *                          finished roll lies in [lo / c2, hi / c2]; under "solver_order" d = y + c (y - p) is formed
 *                          from the clamped y and the history p holds the clamped prediction, while d itself is not
 *                          clamped (the published thresholded 2M), with or without "solver_noise"; a step outside
 *                          "guidance_t_min" / "guidance_t_max" clamps the conditional prediction alone; two windows clamp
 *                          the same mean, so the frames they share stay bit-identical.  The diffusion of "start_noise",
 *                          dr_forward, dr_forward_steps, dr_q_sample and dr_extract_x0 are unaffected; dr_sample_checked's
 *                          re-run uses the same value.  A change of the value ends a dr_step history of "solver_order" 2
 *                          (p would be clamped by another rule than y): the next dr_step that is not a chain's first ->
 *                          DR_ESTATE.  An epsilon sampler (DR_SAMPLER_* 6-8) has no x0 prediction to
 *                          clamp: a non-zero value with one -> DR_EINVAL at dr_step / dr_sample / dr_sample_checked,
 *                          naming both; any other value -> DR_EINVAL at the set.  Combines with "sampling_steps",
 *                          "window_overlap" / "window_break", "draws" / "draw_stride", "guidance_t_min" / "guidance_t_max",
 *                          "solver_order" / "solver_noise", "start_step" / "start_noise", both precisions and sharding
 *                          (every rank sets the same value).  The value is part of a captured chain's key, like
 *                          "solver_order": setting it drops nothing, and a chain captured under another value is never
 *                          replayed.  The dynamic (percentile) form is "x0_threshold" below, which refines this
 *                          option.  Nothing is known about the quality of clamped chains with this model
 *                          (INTEGRATION.md 3c).
 *   "x0_threshold"     [0] 0, or 5000 .. 10000: DYNAMIC THRESHOLDING of the same prediction (Saharia et al. 2022, Imagen;
 *                          the thresholding DPM-Solver++ was published with) at the percentile value / 10000 - 9950 is
 *                          Imagen's 99.5 %, 10000 the maximum.  It refines "x0_clip", which keeps naming the range
 *                          [lo, hi]; m = (lo + hi) / 2, r = (hi - lo) / 2.  With y the value "x0_clip" clamps (guided,
 *                          after the shared-frame mean), every line rounded once in fp32:
 *                              u = y - m;  a = |u| of every element of the GROUP, ascending (as bit patterns with the sign
 *                              cleared: -0 == +0, inf above every finite value, NaN last)
 *                              num = value (N - 1) (64-bit; N = elements of the group), k = num / 10000, rem = num % 10000
 *                              q = rem == 0 ? a[k] : a[k] + f (a[k + 1] - a[k]),  f = (float)((double)rem / 10000.0)
 *                              s = q > r ? q : r      (a NaN q gives s = r)
 *                              y' = s > r ? m + (clamp(u, -s, s) r) / s : clamp(y, lo, hi)
 *                          clamp = the compare-and-select of "x0_clip" (a NaN stays a NaN).  q is the linear-interpolation
 *                          quantile (torch.quantile), selected EXACTLY - no sampling, no bins - and deterministically:
 *                          integer counts only, the same bits on every launch geometry and replay.  A step whose q does
 *                          not exceed r is bit-identical to the "x0_clip" step.  Everything behind y' reads y', exactly as
 *                          it reads the clamped y under "x0_clip".  THE GROUP one q is taken over: a clip's roll, T * 88
 *                          elements (every draw of "draws" is a roll of its own); under "window_overlap" the RECORDING'S
 *                          CANVAS, every canvas frame counted once - a recording's first window contributes all its
 *                          frames, every other one frames [O, T); "window_break" and draws delimit recordings as they do
 *                          for the noise keys; N = ((n_r - 1) H + T) * 88 - so all windows of a recording use the same s
 *                          on the same mean and the frames they share stay bit-identical.  A group never spans ranks: a
 *                          sharded run gives every roll the same result on any world size.  WHERE IT RUNS: the selection
 *                          sits between the network and the update, so a thresholded step does not use the tail kernel.
 *                          The evaluation keeps its fused stack launch where it has one; the head projections, the
 *                          threshold launches (one per roll-sized clip batch, five for windows and longer clips) and the
 *                          update are ordinary launches: dr_launch_state reports DR_MODE_FUSED_STACK for such a step and
 *                          tail_launches does not move (cost: profiles/thresh_sweep.txt).  A non-zero value with
 *                          "x0_clip" = 0 -> DR_EINVAL at dr_step / dr_sample / dr_sample_checked, naming both; an
 *                          epsilon sampler is refused by the rule of "x0_clip"; any value but 0 and 5000 .. 10000 ->
 *                          DR_EINVAL at the set, naming the value.  dr_forward, dr_forward_steps, dr_q_sample,
 *                          dr_extract_x0 and the diffusion of "start_noise" are unaffected; dr_sample_checked's re-run
 *                          uses the same value.  A change of the value ends a dr_step history of "solver_order" 2, as a
 *                          change of "x0_clip" does.  Combines with "sampling_steps", "window_overlap" / "window_break",
 *                          "draws" / "draw_stride", "guidance_t_min" / "guidance_t_max" (an unguided step thresholds the
 *                          conditional prediction alone), "solver_order" / "solver_noise", "start_step" / "start_noise",
 *                          both precisions and sharding.  Stored like "solver_noise": setting it drops nothing; the value
 *                          is part of a captured chain's key, and the chain replays with no host help (the kernels re-arm
 *                          their own work words).  0 = off: every path is byte-identical to an engine that never set it.
 *                          Nothing is known about quality with real weights.
 *   "cfg_rescale"      [0] 0, or 1 .. 10000: THE GUIDANCE RESCALE of Lin et al. 2024 ("Common Diffusion Noise Schedules and
 *                          Sample Steps are Flawed", section 3.4), phi = value / 10000 (7000 = the paper's 0.7).  The guided
 *                          prediction (1 + w) c - w u is an extrapolation whose spread exceeds the conditional
 *                          prediction's; the rescale scales the excess back - cell order and zeros preserved - in front
 *                          of "x0_clip" / "x0_threshold", which cut it off at the range's ends.  WHERE IT ACTS: at a reverse
 *                          step that guides - the sampler is DR_SAMPLER_CFDG_DDPM_X0, _INPAINTING_DDPM_X0 or
 *                          _CFDG_DDIM_X0 and the step runs the unconditional evaluation (inside "guidance_t_min" /
 *                          "guidance_t_max", not a w = 0 chain).  With y the guided prediction after the shared-frame
 *                          mean / blend of "window_overlap" / "window_blend" and c the conditional prediction put through
 *                          the same mean / blend alone, per GROUP and in double:
 *                              N = elements of the group;  S1c = sum c, S2c = sum c c, S1y = sum y, S2y = sum y y
 *                              Vc = S2c - S1c (S1c / N),  Vy = S2y - S1y (S1y / N)      (each operation rounded once)
 *                              rho = sqrt(Vc / Vy),  phid = (double)value / 10000.0
 *                              g = (float)(1.0 + phid (rho - 1.0))
 *                              g = 1.0f exactly when !(Vy > 0), !(Vc >= 0) or g is not finite (constant rolls, inf / NaN)
 *                          The step's prediction becomes y' = g y - one fp32 product, the identity where g == 1.0f -
 *                          and everything behind reads y': the clamp of "x0_clip"; the selection of "x0_threshold", which
 *                          ranks |g y - m|; both terms of every update; y / c2 of the last step; d and the history p of
 *                          "solver_order", with or without "solver_noise".  THE GROUP is exactly the group of
 *                          "x0_threshold": a clip's roll (every draw of "draws" its own); under "window_overlap" the
 *                          recording's canvas, every canvas frame counted once (a window that is not its recording's first
 *                          contributes frames [O, T)); "window_break" and draws delimit recordings; a group never spans
 *                          ranks.  All windows of a recording use the same g on the same blended value: the frames they
 *                          share stay bit-identical.  THE ORDER OF THE SUMS is part of the definition (a square of an fp32
 *                          value is exact in double: only the additions round), every level a sequential sum from 0.0:
 *                              a frame's 88 elements in pitch order;
 *                              the frames a row counts - all of a clip's, [O, T) of a window that is not its recording's
 *                              first - in blocks of 64 from its first counted frame, a block's frames in frame order;
 *                              a group's blocks in row, then block order.
 *                          g is a function of the inputs alone - no floating-point atomic, the same bits on every grid,
 *                          replay and launch form.  WHERE IT RUNS: the statistics sit between the network and the update,
 *                          so a guided step under the option does not use the tail kernel: fused stack, head
 *                          projections, one statistics launch (csrc/rescale.hip), the threshold launches where
 *                          "x0_threshold" is set, the update; dr_launch_state reports DR_MODE_FUSED_STACK for it (cost:
 *                          profiles/rescale_sweep.txt).  A step
 *                          that does not guide is untouched - no launch is added, it keeps its tail kernel, not a bit
 *                          changes - and the six samplers that do not guide ignore the option as they ignore the
 *                          guidance interval.  Any value outside 0 .. 10000 -> DR_EINVAL at the set, naming the value.
 *                          dr_step follows the rule for its one step; dr_forward, dr_forward_steps, dr_q_sample,
 *                          dr_extract_x0 and the diffusion of "start_noise" are unaffected; dr_sample_checked's re-run
 *                          uses the same value.  A change of the value ends a dr_step history of "solver_order" 2, as a
 *                          change of "x0_clip" does.  Combines with "sampling_steps", "window_overlap" / "window_break" /
 *                          "window_blend", "draws" / "draw_stride", "guidance_t_min" / "guidance_t_max", "solver_order" /
 *                          "solver_noise", "start_step" / "start_noise", "x0_clip" / "x0_threshold" (neither is required),
 *                          all three precisions and sharding.  Stored like "x0_threshold": setting it drops nothing; the
 *                          value is part of a captured chain's key where a step of the chain can read it - a sampler
 *                          that guides, at w != 0 - and of no other chain's; the chain replays with no host help.  0 = off:
 *                          every path is byte-identical to an engine that never set it.  Nothing is known about quality
 *                          with real weights.
 *   "cfg_project"      [0] 0, or 1 .. 10000, and
 *   "cfg_norm"         [0] 0, or 1 .. 100000: ADAPTIVE PROJECTED GUIDANCE of Sadat et al. 2024 ("Eliminating Oversaturation
 *                          and Artifacts of High Guidance Scales in Diffusion Models"), without its momentum, which is option
 *                          "cfg_momentum" below (that part needs a roll-sized state with validity rules like the solver
 *                          history's).  The guided
 *                          prediction y = (1 + w) c - w u moves the conditional prediction c by w (c - u).  The part of that
 *                          update parallel to c only scales c up - the saturation "x0_clip", "x0_threshold" and
 *                          "cfg_rescale" fight afterwards; the orthogonal part carries the conditioning.  rho = cfg_project /
 *                          10000 is the share of the parallel component that is removed (10000 = APG's eta = 0); r =
 *                          cfg_norm / 10000 is the bound on the per-element rms of c - u over the group (the rms, not
 *                          APG's absolute norm: one value means the same for a 125-frame clip and a long canvas).  The
 *                          projected form runs at a step that guides when either value is not 0.  WHERE IT ACTS: at a
 *                          reverse step that guides, as "cfg_rescale" defines it - the sampler is
 *                          DR_SAMPLER_CFDG_DDPM_X0, _INPAINTING_DDPM_X0 or _CFDG_DDIM_X0 and the step runs the
 *                          unconditional evaluation (inside "guidance_t_min" / "guidance_t_max", w != 0).  With y the
 *                          guided prediction after the shared-frame mean / blend of "window_overlap" / "window_blend", c
 *                          the conditional prediction put through the same mean / blend alone and w the step's weight,
 *                          per GROUP and in double:
 *                              d_i = (double)y_i - (double)c_i
 *                              Scc = sum c_i c_i,  Scd = sum c_i d_i,  Sdd = sum d_i d_i,  N = elements of the group
 *                                  (every product and every addition rounded once, no contraction)
 *                              k = Scd / Scc,  k = 0.0 when !(Scc > 0)
 *                              rho = (double)cfg_project / 10000.0
 *                              s = 1.0;  if cfg_norm != 0: r = (double)cfg_norm / 10000.0,
 *                                  q = sqrt(Sdd / N) / fabs((double)w),  if (q > r) s = r / q
 *                              a = (float)((1.0 - s) - s (rho k)),  b = (float)s
 *                              a = 0.0f, b = 1.0f exactly when a or b is not finite
 *                              y' = y where a == 0.0f and b == 1.0f (bit for bit)
 *                              y' = (a c) + (b y) otherwise, fp32, each operation rounded once
 *                          which is y' = c + s (d - rho k c): the update is bounded and its parallel component reduced
 *                          by rho.  Everything behind reads y': the clamp of "x0_clip"; both terms of every update; y /
 *                          c2 of the last step; d and the history p of "solver_order", with or without "solver_noise".
 *                          THE GROUP is exactly the group of "x0_threshold" / "cfg_rescale": a clip's roll (every draw
 *                          of "draws" its own); under "window_overlap" the recording's canvas, every canvas frame counted
 *                          once (a window that is not its recording's first contributes frames [O, T)); "window_break"
 *                          and draws delimit recordings; a group never spans ranks.  All windows of a recording use the
 *                          same (a, b) on the same blended values: the frames they share stay bit-identical.  THE ORDER
 *                          OF THE SUMS is part of the definition and is "cfg_rescale"'s, every level a sequential sum
 *                          from 0.0:
 *                              a frame's 88 elements in pitch order;
 *                              the frames a row counts - all of a clip's, [O, T) of a window that is not its recording's
 *                              first - in blocks of 64 from its first counted frame, a block's frames in frame order;
 *                              a group's blocks in row, then block order.
 *                          a and b are functions of the inputs alone - no floating-point atomic, the same bits on every
 *                          grid, replay and launch form.  WHERE IT RUNS: the statistics sit between the network and the
 *                          update, so a guided step under the options does not use the tail kernel: fused stack, head
 *                          projections, one statistics launch (csrc/project.hip), the update's projecting form;
 *                          dr_launch_state reports DR_MODE_FUSED_STACK for it (cost: profiles/project_sweep.txt).  A step
 *                          that does not guide is untouched - no launch is added, it keeps its tail kernel, not a bit
 *                          changes - and the six samplers that do not guide ignore both options as they ignore the
 *                          guidance interval.  REFUSED: beside "x0_threshold" (its selection would have to rank the
 *                          projected prediction) and beside "cfg_rescale" (the two are alternatives; a combined form
 *                          would need the spread of y') - DR_EINVAL naming both options from dr_sample / dr_step, for every
 *                          sampler.  A value outside its range -> DR_EINVAL at the set, naming the value.  dr_step follows
 *                          the rule for its one step; dr_forward, dr_forward_steps, dr_q_sample, dr_extract_x0 and the
 *                          diffusion of "start_noise" are unaffected; dr_sample_checked's re-run uses the same values.  A
 *                          change of either value ends a dr_step history of "solver_order" 2, as a change of "x0_clip"
 *                          does.  Combines with "sampling_steps", "window_overlap" / "window_break" / "window_blend",
 *                          "draws" / "draw_stride", "guidance_t_min" / "guidance_t_max", "solver_order" / "solver_noise",
 *                          "start_step" / "start_noise", "x0_clip", all three precisions and sharding.  Stored like
 *                          "cfg_rescale": setting them drops nothing; the values are part of a captured chain's key
 *                          where a step of the chain can read them - a sampler that guides, at w != 0 - and of no other
 *                          chain's; the chain replays with no host help.  Both 0 = off: every path is byte-identical to
 *                          an engine that never set them.  Nothing is known about quality with real weights
 *                          (INTEGRATION.md 3c).
 *   "cfg_momentum"     [0] 0, or -9999 .. 9999 except 0: THE MOMENTUM of adaptive projected guidance (Sadat et al. 2024), the
 *                          third part of the method beside "cfg_project" / "cfg_norm": beta = cfg_momentum / 10000 (the paper's values are -0.5
 *                          .. -0.75, i.e. -5000 .. -7500).  A reverse momentum (beta < 0) keeps the guidance update from
 *                          accumulating in one direction from step to step; the projection and the norm bound treat one
 *                          step at a time.  WHERE IT ACTS: at a step that guides, as "cfg_project" defines it, and only
 *                          beside "cfg_project" and / or "cfg_norm".  With y the guided prediction and c the conditional
 *                          one, both after the shared-frame mean / blend, per element, in fp32, no contraction, each
 *                          operation rounded once:
 *                              bf = (float)((double)cfg_momentum / 10000.0)
 *                              d  = y - c
 *                              m  = d                  at the step that STARTS the state (nothing is read)
 *                              m  = d + (bf * m_prev)  at every other guided step
 *                              yb = c + m
 *                          and everything "cfg_project" / "cfg_norm" define happens with yb in place of y: the three sums
 *                          use d_i = (double)yb_i - (double)c_i in the same fixed order, (a, b) and its |w| are unchanged, y'
 *                          = (a c) + (b yb), y' = yb where a == 0.0f and b == 1.0f, then the clamp of "x0_clip".  m is what
 *                          the next guided step reads as m_prev.  A non-finite m stays non-finite for that element for the
 *                          rest of the chain; its group then gets a = 0.0f, b = 1.0f, as under "cfg_project".  THE STATE is
 *                          one float per roll element, engine memory, updated in place; a frame two windows share holds
 *                          the same m in both rows (d is bit-identical there), and each rank holds the state of its rows.
 *                          WHICH STEP STARTS IT: the first guided step a chain runs - from the chain's start position
 *                          ("start_step"), the highest visited step that guides (a sampler that guides, w != 0, inside
 *                          "guidance_t_min" / "guidance_t_max").  Steps that do not guide neither read nor write the state;
 *                          a guided step after a gap continues from the last guided one.  A captured chain bakes "starts"
 *                          into the step's nodes: no memset, no host help, every replay restarts by itself.  WHERE IT RUNS:
 *                          the launches of a guided step under "cfg_project" in their momentum form (csrc/momentum.hip) -
 *                          fused stack, head projections, one statistics launch that reads the state, the update that
 *                          advances it; dr_launch_state reports DR_MODE_FUSED_STACK.  dr_step: the state is engine state
 *                          with the discipline of the history of "solver_order" 2 - a guided dr_step starts it (the first
 *                          guided step) or continues the previous guided dr_step of the same (sampler, B, T), which must be
 *                          the guided visited step before it; otherwise DR_ESTATE naming the step expected next.  The state
 *                          ends on dr_sample, dr_frontend with another shape, growth of the state, every option change that
 *                          ends a solver history, and a change of "cfg_momentum" itself.  REFUSED: a value that is not 0
 *                          while "cfg_project" and "cfg_norm" are both 0 - DR_EINVAL naming the three options from dr_sample /
 *                          dr_step; beside "x0_threshold" / "cfg_rescale" the refusals of "cfg_project" hold.  A value out of
 *                          range -> DR_EINVAL at the set, stating the range.  Combines with everything "cfg_project"
 *                          combines with.  Stored like "cfg_project": the value is part of a captured chain's key where a
 *                          step can read it.  0 = off: every path is byte-identical to an engine that never set it.
 *                          Nothing is known about quality with real weights.
 *   "guidance_stride"  [0] 0 or 1 (off), or 2 .. 64: THE GUIDANCE UPDATE COMPUTED EVERY n-th GUIDED STEP and reused in
 *                          between - the CFG cache of FasterCache (Lv et al. 2024), the observation of "Adaptive Guidance"
 *                          (Castillo et al. 2023): the difference between the guided and the conditional prediction changes
 *                          slowly along the chain.  n = guidance_stride.  ORDINAL: the steps that guide - a sampler that
 *                          guides, w != 0, inside "guidance_t_min" / "guidance_t_max" - are numbered k = 0, 1, 2, ... in the
 *                          order the chain visits them from its start position ("start_step").  A guided step REFRESHES when
 *                          k % n == 0 or when it is step t == 0; otherwise it REUSES.  The first guided step a chain runs
 *                          is k = 0 and always refreshes: under an interval the first step inside it, under "start_step"
 *                          the first guided step at or below the start.  Step 0 refreshes because the roll is the last
 *                          step's prediction.  A REFRESH STEP evaluates both branches exactly as without the option.  With
 *                          y the guided prediction and c the conditional one, both after the shared-frame mean / blend,
 *                          per element, in fp32, no contraction, one rounding:
 *                              d = y - c
 *                          is stored into the engine's state - one float per roll element, written by the element's own
 *                          thread - and y goes on unchanged: the roll a refresh step leaves is, bit for bit, the roll of
 *                          the same step with the option off.  A REUSE STEP evaluates the conditional branch alone - B
 *                          evaluations, the shape of a step outside the guidance interval - and its prediction is
 *                              y = c + d
 *                          in fp32 with one rounding, c behind the blend, d as the last refresh stored it.  Everything that
 *                          read the guided prediction reads this y: the clamp of "x0_clip", the sampler's own update, the
 *                          solver's extrapolation and its history ("solver_order"), the last step.  d CARRIES THE WEIGHT of
 *                          the step that stored it: a dr_step sequence that changes w between a refresh and its reuses
 *                          gets what it asked for - the stored update at the old weight.  WINDOWS: d is taken behind the
 *                          blend, so a frame two windows share holds the same d in both rows; windows read each other's
 *                          predictions as without the option and never each other's state, and shared frames stay
 *                          bit-identical.  There is one state per roll: per draw under "draws", per window row, per rank's
 *                          rows when sharded.  A CAPTURED CHAIN bakes refresh / reuse into the step's nodes; its first
 *                          guided step refreshes and overwrites the state: no memset, no host help, every replay restarts
 *                          by itself.  WHERE IT RUNS: a guided step under the option - refresh or reuse - runs the stack
 *                          launch, the head projections and update_stride_kernel (csrc/stride.hip); dr_launch_state
 *                          reports DR_MODE_FUSED_STACK where the stack is fused.  Steps that do not guide keep the tail
 *                          kernel and every bit.  dr_step: the state is engine state with the discipline of "cfg_momentum" -
 *                          a step that refreshes needs nothing; a step that reuses must be the guided visited step behind
 *                          the guided step the previous guided dr_step ran, in a chain of the same (sampler, B, T);
 *                          otherwise DR_ESTATE naming the step expected next.  The state ends on dr_sample, dr_frontend
 *                          with another shape, growth of the state, every option change that ends a solver history, and a
 *                          change of "guidance_stride" itself.  REFUSED: beside "x0_threshold", "cfg_rescale",
 *                          "cfg_project", "cfg_norm" or "cfg_momentum" - their statistics need the unconditional
 *                          prediction - and by a sampler that does not guide: DR_EINVAL from dr_sample / dr_step, naming
 *                          the two options.  A value outside 0 .. 64 -> DR_EINVAL at the set, stating the range.  Combines
 *                          with "sampling_steps", windows and "window_blend", "window_break", "draws", the guidance
 *                          interval, "solver_order" / "solver_noise", "start_step" / "start_noise", "x0_clip", every
 *                          precision and sharding.  The value is part of a captured chain's key where a step can read it -
 *                          a sampler that guides, w != 0 - and 0 and 1 are one value there.  0 or 1 = off: every path is
 *                          byte-identical to an engine that never set it and replays the same captured chain.  Nothing is
 *                          known about quality with real weights.
 *   "exact_below"      [0] 0 (off), or v in 1 .. timesteps: FINISH A REDUCED-PRECISION CHAIN IN FP32.  A reverse step at
 *                          diffusion step t < v runs in DR_PRECISION_F32 whatever dr_set_precision selected; a step with
 *                          t >= v runs in the selected mode.  The reverse chain forgets - each update takes most of its
 *                          weight from the current prediction - so the rounding of the high-noise steps is mostly gone a
 *                          few steps later and only the last steps decide the roll.  RANGE: 0 <= v <= timesteps; 0 = off,
 *                          v = timesteps = every step exact (the roll of the DR_PRECISION_F32 engine, bit for bit); any
 *                          other value -> DR_EINVAL at the set, stating the range, and the previous value stays in force.
 *                          KEY: the real diffusion step t, as "guidance_t_min" / "guidance_t_max" are - the option means
 *                          the same under "sampling_steps", where v may fall between two visited steps.  The visited t
 *                          decrease along a chain, so every exact step lies behind every reduced one.  APPLIES TO the
 *                          reverse steps of dr_step, dr_sample and dr_sample_checked, the per-phase recompute after a
 *                          healed time-out included.  dr_forward and dr_forward_steps are network evaluations, not chain
 *                          steps: they are EXEMPT and keep the engine's mode.  Under DR_PRECISION_F32 the option is
 *                          accepted and changes nothing.  WHERE IT RUNS: an exact step is planned as a step of an fp32
 *                          chain - fused stack + tail kernel (two launches, DR_MODE_FUSED_STACK_TAIL) where that chain
 *                          would take them; the first exact step computes its own input layer, as a chain's first step
 *                          does, and the last reduced step primes nothing.  The selected mode's packings stay resident
 *                          beside the fp32 ones (which always are); no state depends on the mode - the roll, the history
 *                          of "solver_order" 2, the states of "cfg_momentum" and "guidance_stride", the work words and
 *                          the noise are fp32 - so a dr_step sequence continues across the boundary and the option
 *                          combines with every sampling option, windows and their blend, "draws", every precision and
 *                          sharding; it has no refusals.  dr_launch_state reports the last step that ran.  A CAPTURED
 *                          CHAIN bakes each step's precision into its nodes: the value is part of the captured chain's
 *                          key (not under DR_PRECISION_F32, where no step reads it) - a chain captured under another
 *                          value is not replayed, one captured under this value still is.  0 = off: every path is
 *                          byte-identical to an engine that never set it and replays the same captured chain.  Nothing is
 *                          known about quality with real weights.
 * Unknown names -> DR_ENAME. (The A/B and test knobs - "tune.*", "fused_stack_xcd", "fused_stack_warm", "stack_ticks" -
 * are set with dr_debug_set_option, diffroll_amd_debug.h.)
 */
int dr_set_option(dr_engine* e, const char* name, int value);
/*
 * Multi-GPU: the path shards by clips - one process per GPU, every rank runs its contiguous shard of
 * the batch with dr_sample (first_sample = the shard's global offset, so Philox noise does not depend on the world
 * size) and the ONLY collective is one all-gather of the finished rolls over xGMI.  These entry points give a
 * caller without torch.distributed that collective: RCCL (librccl, looked up with dlopen at first use).
 * The reference reaches N GPUs through Lightning's Trainer(gpus=N) (sampling.py:70) and never gathers.
 *   dr_comm_unique_id   rank 0: 128 bytes (ncclUniqueId) to hand to every rank by any side channel
 *   dr_comm_create      every rank, collectively: ncclCommInitRank on `device`
 *   dr_comm_info        ranks / rank of a communicator and the version code of the loaded librccl (any pointer may be
 *                       NULL; c == NULL: the version alone)
 *   dr_gather           d_shard (B_local, T, 88) of every rank -> d_full (n_ranks * B_local, T, 88), rank-major, on
 *                       `stream` (ncclAllGather; equal B_local on all ranks - pad uneven shards, see
 *                       diffroll_amd/distributed.py).  `e` may be NULL.  SYNCHRONOUS, and the verdict is COLLECTIVE: behind the
 *                       rolls every rank also gathers one status word (0 = my shard is valid, 1 = it came out of a fused
 *                       launch that timed out: dr_pending_timeout), and EVERY rank returns DR_ETIMEOUT when any shard was
 *                       invalid - nobody is handed a d_full that holds a bad shard together with DR_OK.  After
 *                       DR_ETIMEOUT: the rank(s) whose dr_finish also reports it recompute their shard, then all ranks
 *                       gather again.
 * Errors of these functions: dr_comm_last_error().
 */
typedef struct dr_comm dr_comm;
int dr_comm_unique_id(char* id_out /* 128 bytes */);
int dr_comm_create(dr_comm** out, const char* id /* 128 bytes */, int n_ranks, int rank, int device);
void dr_comm_destroy(dr_comm* c);
int dr_comm_info(const dr_comm* c, int* n_ranks, int* rank, int* rccl_version);
const char* dr_comm_last_error(void);
int dr_gather(dr_engine* e, dr_comm* comm, const float* d_shard, float* d_full, int B_local, int T, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFFROLL_AMD_H */
