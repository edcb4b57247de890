/*
 * psg_hip.h — C ABI of libpsg_hip.so: the MI355X (gfx950) kernels behind the
 * U-Net denoising train step of GabrieleConte/pokemon-sprite-generator.
 *
 * The reference has NO native code, plugin registry or FFI: its hot path is
 * PyTorch ATen ops called from src/models/unet.py and
 * src/training/improved_diffusion_trainer.py.  Each entry point below replaces
 * the ATen call(s) made at the cited reference lines (paths relative to the
 * reference root).  The host side (the .py files of pokemon_sprite_generator_amd) binds
 * these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *  - Plain pointers and sizes only; no torch types.  All pointers are DEVICE
 *    pointers borrowed for the duration of the call.  Nothing is allocated or
 *    freed on behalf of the caller: scratch is a caller-provided workspace
 *    (query *_workspace_bytes first).
 *  - Every launch is asynchronous on `stream` (a hipStream_t); no hidden
 *    synchronisation, no host reads: graph-capture safe.
 *  - Return 0 on success, <0 on error (enum below); psg_last_error() returns a
 *    thread-local message.  NaN/Inf in data is reported as data (flags), never
 *    as an error.
 *  - Activations are channels-last: a [B, H, W, C] (or [B, L, C] token) tensor
 *    is a row-major matrix of B*H*W rows with an explicit row stride `ld`
 *    (in elements), so slices of wider buffers are addressable.  dtype selects
 *    the element type of activations and prepared weights (PSG_F32 / PSG_BF16);
 *    statistics, biases, accumulators, master weights and gradients of
 *    parameters are always fp32.
 */
#ifndef PSG_HIP_H
#define PSG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* psg_stream_t; /* hipStream_t */

enum psg_status {
    PSG_OK = 0,
    PSG_ERR_SHAPE = -1,
    PSG_ERR_DTYPE = -2,
    PSG_ERR_ALIGN = -3,
    PSG_ERR_WORKSPACE = -4,
    PSG_ERR_HIP = -5,
    PSG_ERR_ARG = -6
};
enum psg_dtype { PSG_F32 = 0, PSG_BF16 = 1 };
enum psg_act { PSG_ACT_NONE = 0, PSG_ACT_SILU = 1, PSG_ACT_GELU = 2, PSG_ACT_RELU = 3, PSG_ACT_TANH = 4,   /* RELU / TANH: the frozen VAE (vae_decoder.py:82-91,185) */
               PSG_ACT_QUICK_GELU = 5 };   /* x * sigmoid(1.702 x): both CLIP towers (transformers' `quick_gelu`, clip_loss.py:22); any other value is PSG_ERR_ARG */
/* What the U-Net's output means (opt-in v-prediction; every entry without this argument is eps-prediction):
 * PSG_PRED_EPS the noise, PSG_PRED_V  v = sqrt(abar_t) eps - sqrt(1 - abar_t) x0. */
enum psg_prediction { PSG_PRED_EPS = 0, PSG_PRED_V = 1 };
/* Bits of the device-side NaN/Inf flag word of one train step (the reference's five host-side
 * check_for_nans scans, improved_diffusion_trainer.py:353-393).  A step whose word has any bit of
 * PSG_FLAG_SKIP_MASK set is skipped like the reference's `continue`: no optimizer step, no scheduler
 * step.  PSG_FLAG_FALLBACK alone does NOT skip: add_noise replaced a non-finite result by
 * x0 + 0.1*noise (:61-63) and the batch trains on that. */
enum psg_flag {
    PSG_FLAG_NOISY_BAD = 1,   /* noisy latent still non-finite after the fallback (:376) */
    PSG_FLAG_T_RANGE = 2,     /* a timestep outside [0, num_t) (the reference raises an IndexError -> batch skipped) */
    PSG_FLAG_PRED_BAD = 4,    /* predicted noise non-finite (:383) */
    PSG_FLAG_LOSS_BAD = 8,    /* loss non-finite (:390) */
    PSG_FLAG_FALLBACK = 16,   /* add_noise took the fallback (informational) */
    PSG_FLAG_INPUT_BAD = 32,  /* text embedding / clean latent non-finite (:353,359; set by the host-side caller) */
    PSG_FLAG_SKIP_MASK = 47
};

const char* psg_last_error(void);
int psg_version(void);
/* Select device, raise LDS limits of the big kernels.  Idempotent. */
int psg_init(int device);

/* ---------------------------------------------------------------------------
 * Noise schedule / sampler elementwise ops (bit-exact fp32, contraction off)
 * ------------------------------------------------------------------------- */

/* NoiseScheduler.add_noise — improved_diffusion_trainer.py:50-65 (+ clamp :363).
 * out[b,i] = tabA[t[b]] * clamp?(x0[b,i]) + tabB[t[b]] * noise[b,i]; two rounded
 * multiplies and one rounded add, bit-identical to the CPU path.  *flag (int32,
 * device) is OR-ed with PSG_FLAG_FALLBACK if any output is NaN/Inf, with
 * PSG_FLAG_T_RANGE if any t[b] is outside [0,num_t); such a t[b] reads the nearest entry of the
 * tables (0 or num_t - 1).  Zero *flag before the call.  B == 0 is PSG_OK with nothing launched;
 * B < 0, chw <= 0 or num_t <= 0 is PSG_ERR_SHAPE; a null pointer is PSG_ERR_ARG. */
int psg_noise_add_f32(const float* x0, const float* noise, const int64_t* t, const float* tabA,
                      const float* tabB, float* out, int32_t* flag, int64_t B, int64_t chw,
                      int num_t, int do_clamp, psg_stream_t stream);
/* The reference's fallback (:61-63): if (*flag & PSG_FLAG_FALLBACK) out = clamp?(x0) + 0.1*noise, and
 * *flag |= PSG_FLAG_NOISY_BAD if that is still non-finite (the trainer's re-check, :376).  Device-side
 * test of the flag; no host sync: with the bit clear neither out nor *flag is written.  n <= 0 is
 * PSG_OK with nothing launched; a null pointer is PSG_ERR_ARG. */
int psg_noise_fallback_f32(const float* x0, const float* noise, float* out, int32_t* flag,
                           int64_t n, int do_clamp, psg_stream_t stream);
/* ddpm_sample update — improved_diffusion_trainer.py:543-567.  step tables hold the per-timestep
 * scalars c1=1/sqrt(alpha_t), c2=beta_t/sqrt(1-alphabar_t), sigma=sqrt(beta_t) (fp32, computed on
 * the host with the reference's torch ops); t_index selects the entry on the device so the launch
 * is graph-replayable: x <- c1*(x - c2*eps) [+ sigma*z if t>0].  t_dev: int32 device scalar.
 * n <= 0 is PSG_OK with nothing launched; a null pointer (z included, whatever t is) is PSG_ERR_ARG. */
int psg_ddpm_update_f32(float* x, const float* eps, const float* z, const float* c1, const float* c2,
                        const float* sigma, const int32_t* t_dev, int64_t n, psg_stream_t stream);

/* Update steps of the two other samplers that consume the trained U-Net, in place on x (fp32, the reference's operation
 * order, bit-exact):
 *   mode 1 — NoiseScheduler.sample_previous_timestep, src/training/final_trainer.py:52-71:
 *            x <- c0 * (x - (c1 * eps) / c2) [+ c3 * z]   with c0 = sqrt(1/alpha_t), c1 = beta_t, c2 = sqrt(1 - abar_t),
 *            c3 = sqrt(posterior_variance_t); z == NULL for t == 0
 *   mode 2 — the t == 0 step of FinalPokemonGenerator.forward, final_trainer.py:203:  x <- x - eps
 *   mode 3 — PokemonGradioGenerator.ddpm_sample, gradio_app.py:343-358:
 *            x <- (x - c0 * eps) / c1  with c0 = (1 - alpha_t)/sqrt(1 - abar_t), c1 = sqrt(alpha_t); then, when z != NULL
 *            (not the last step and next_t > 0), x <- c2 * x + c3 * z with c2 = sqrt(alpha_next), c3 = sqrt(1 - alpha_next)
 * The scalars are computed by the host with the reference's own torch expressions.  A mode outside 1..3 or a null x or eps
 * is PSG_ERR_ARG; n <= 0 is PSG_OK with nothing launched. */
int psg_sampler_update_f32(float* x, const float* eps, const float* z, int mode, float c0, float c1, float c2,
                           float c3, int64_t n, psg_stream_t stream);

/* Classifier-free guidance and the DDIM step (no counterpart in the reference; opt-in on the host side).  fp32, every
 * operation rounded on its own (no FMA), so a numpy-float32 restatement gives the same bits.
 *
 * Per-sample text drop for training: text, out [B, row] (row = S * text_dim), null_text [row].  Sample b takes null_text when
 * the library's stateless dropout hash drops element index b at rate p, else its own row of text.  The device word of
 * psg_set_seed_source is added to seed when the launch runs, so a captured train step draws a new mask on every replay.
 * dropped (int32 [B], may be NULL) receives 1 for a replaced sample and 0 otherwise.  16-byte loads and stores when row is a
 * multiple of 4 and text, null_text and out are 16-byte aligned, element by element otherwise.  B == 0 is PSG_OK with nothing
 * launched; B < 0 or row <= 0 is PSG_ERR_SHAPE; p outside [0, 1) (the hash's 16-bit threshold saturates: p = 1 would still keep
 * one sample in 65 536), a null text, null_text or out, or out == text is PSG_ERR_ARG. */
int psg_text_cond_drop_f32(const float* text, const float* null_text, float* out, int32_t* dropped, int64_t B, int64_t row,
                           float p, uint64_t seed, psg_stream_t stream);
/* out = eps_u + w * (eps_c - eps_u), three roundings; for the chains that keep their own update (psg_ddpm_update_f32,
 * psg_sampler_update_f32).  out may alias eps_c.  n <= 0 is PSG_OK with nothing launched; a null pointer is PSG_ERR_ARG. */
int psg_cfg_combine_f32(const float* eps_c, const float* eps_u, float w, float* out, int64_t n, psg_stream_t stream);
/* One DDIM step in place on x, one launch.  tab: device [5, k] fp32, rows S0 = sqrt(abar_t), S1 = sqrt(1 - abar_t),
 * P0 = sqrt(abar_prev), P1 = sqrt(1 - abar_prev - sigma^2), SG = sigma of step j (built by the host in fp64, rounded once).
 * step_dev: int32 device scalar j, read on the device (graph-replayable); a j outside 0..k-1 reads the nearest entry.
 *   e  = eps_c                                   when eps_u == NULL
 *   e  = eps_u + w * (eps_c - eps_u)             otherwise
 *   x0 = (x - S1[j] * e) / S0[j]
 *   if clip > 0:  c = clamp(x0, -clip, clip)     (NaN stays NaN, as numpy.clip)
 *                 where c != x0:  e = (x - S0[j] * c) / S1[j]
 *                 x0 = c
 *   x' = P0[j] * x0 + P1[j] * e  [+ SG[j] * z    when z != NULL]
 * x' is written to x and, when x_copy != NULL, to x_copy too (the unconditional half of a 2n input buffer: no copy runs
 * between steps).  16-byte accesses when n is a multiple of 4 and every pointer given is 16-byte aligned, element by element
 * otherwise.  clip < 0, k < 1, or a null x, eps_c, tab or step_dev is PSG_ERR_ARG; n <= 0 is PSG_OK with nothing launched. */
int psg_guided_update_f32(float* x, float* x_copy, const float* eps_c, const float* eps_u, const float* z, const float* tab, int k,
                          const int32_t* step_dev, float w, float clip, int64_t n, psg_stream_t stream);
/* psg_guided_update_f32 for a network that predicts `prediction` (enum psg_prediction), same table, x_copy, vector rule and
 * refusals; a prediction outside the enum is PSG_ERR_ARG.  PSG_PRED_EPS gives psg_guided_update_f32's bits.  PSG_PRED_V:
 *   p  = pred_c                                  when pred_u == NULL
 *   p  = pred_u + w * (pred_c - pred_u)          otherwise
 *   x0 = S0[j] * x - S1[j] * p                   (two rounded products, one rounded subtraction; no division)
 *   e  = S1[j] * x + S0[j] * p
 * and from there the clamp, the eps recompute where it acts and x' exactly as above. */
int psg_guided_update_pred_f32(float* x, float* x_copy, const float* pred_c, const float* pred_u, const float* z, const float* tab, int k,
                               const int32_t* step_dev, float w, float clip, int64_t n, int prediction, psg_stream_t stream);
/* The guided prediction as eps, for the chains that keep their own update (psg_ddpm_update_f32, psg_sampler_update_f32); under
 * guidance it takes psg_cfg_combine_f32's place, so those chains gain no launch:
 *   p   = pred_c, or pred_u + w * (pred_c - pred_u) when pred_u != NULL        (psg_cfg_combine_f32's three roundings)
 *   out = p                                      PSG_PRED_EPS (x, tabA, tabB are not read and may be NULL)
 *   out = tabB[t] * x + tabA[t] * p              PSG_PRED_V, tabA = sqrt(abar), tabB = sqrt(1 - abar): the tables of psg_noise_add_f32
 * t = *t_dev (int32 device scalar, read on the device: graph-replayable; outside 0..num_t-1 it reads the nearest entry).
 * out may alias pred_c.  16-byte accesses when n is a multiple of 4 and every pointer read or written is 16-byte aligned.
 * A prediction outside the enum, a null pred_c, out or t_dev, or PSG_PRED_V with a null x, tabA or tabB is PSG_ERR_ARG;
 * num_t <= 0 is PSG_ERR_SHAPE; n <= 0 is PSG_OK with nothing launched, as is PSG_PRED_EPS without pred_u and out == pred_c. */
int psg_pred_to_eps_f32(const float* x, const float* pred_c, const float* pred_u, float w, const float* tabA, const float* tabB, int num_t,
                        const int32_t* t_dev, int prediction, float* out, int64_t n, psg_stream_t stream);

/* VAE reparameterisation, src/models/vae_decoder.py:120-123: out = mu + eps * exp(0.5 * logvar) (fp32, separately rounded).
 * n <= 0 is PSG_OK with nothing launched; a null pointer is PSG_ERR_ARG. */
int psg_reparam_f32(const float* mu, const float* logvar, const float* eps, float* out, int64_t n, psg_stream_t stream);
/* Its backward (stage 1 trains the encoder through the sample, vae_decoder.py:120-123): dmu = dlatent,
 * dlogvar = dlatent * eps * 0.5 * exp(0.5 * logvar); either output may be NULL; accumulate != 0 adds into what dmu / dlogvar
 * hold.  logvar and eps are read only for dlogvar and may be NULL without it.  A null dlatent, both outputs NULL, or dlogvar
 * without logvar and eps is PSG_ERR_ARG; n <= 0 is PSG_OK with nothing launched. */
int psg_reparam_bwd_f32(const float* dlatent, const float* logvar, const float* eps, float* dmu, float* dlogvar, int accumulate,
                        int64_t n, psg_stream_t stream);

/* SmoothL1Loss(beta) mean + its gradient — improved_diffusion_trainer.py:300,388,396.
 * loss_out: fp32 device scalar; grad (may be NULL) = dL/dpred * grad_scale.  Deterministic
 * two-stage reduction.  ws: >= psg_reduce_workspace_bytes() bytes.  *nan_flag (may be NULL; never cleared here) is
 * OR-ed with PSG_FLAG_PRED_BAD if any pred is NaN/Inf and with PSG_FLAG_LOSS_BAD if the loss is.  n <= 0 or
 * beta <= 0 is PSG_ERR_SHAPE; a null pred, target, loss_out or ws is PSG_ERR_ARG. */
int psg_smooth_l1_f32(const float* pred, const float* target, float* grad, float* loss_out,
                      int32_t* nan_flag, float beta, float grad_scale, int64_t n, void* ws,
                      psg_stream_t stream);
int64_t psg_reduce_workspace_bytes(void);
/* The diffusion loss with its target built in registers and a per-timestep weight (opt-in: v-prediction, Min-SNR), one
 * fused launch in psg_smooth_l1_f32's place.  pred, noise, x0 [B, chw] fp32, t [B] int64, tabA / tabB / wtab [num_t] fp32
 * (tabA = sqrt(abar), tabB = sqrt(1 - abar), psg_noise_add_f32's tables).  For element i of sample b, tt = t[b] clamped to
 * 0..num_t-1:
 *   target = noise                                         PSG_PRED_EPS (x0, tabA, tabB are not read and may be NULL)
 *   target = tabA[tt] * noise - tabB[tt] * clamp?(x0)      PSG_PRED_V: two rounded products, one rounded subtraction;
 *                                                          do_clamp is psg_noise_add_f32's clamp to +-3 (NaN kept)
 *   w      = wtab ? wtab[tt] : 1
 *   loss   = (1 / n) sum_i w * smoothl1_beta(pred - target),  n = B * chw   (a mean over all elements, not divided by sum w)
 *   grad   (may be NULL) = w * smoothl1'(pred - target) / n * grad_scale
 *   target_out (may be NULL) = target
 * Deterministic two-stage reduction in a fixed order; ws: >= psg_reduce_workspace_bytes() bytes.  *nan_flag (may be NULL; never
 * cleared here) is OR-ed with PSG_FLAG_PRED_BAD if any pred is NaN/Inf, with PSG_FLAG_LOSS_BAD if the loss is, and with
 * PSG_FLAG_T_RANGE if any t[b] is outside the tables.  16-byte loads and stores when chw is a multiple of 4 and every pointer
 * given among pred, noise, x0 (PSG_PRED_V), grad and target_out is 16-byte aligned; element by element otherwise.
 * B < 0, chw <= 0, num_t <= 0 or beta <= 0 is PSG_ERR_SHAPE; a prediction outside the enum, a null pred, noise, t, loss_out or
 * ws, or PSG_PRED_V with a null x0, tabA or tabB is PSG_ERR_ARG; B == 0 is PSG_OK with nothing launched. */
int psg_diffusion_loss_f32(const float* pred, const float* x0, const float* noise, const int64_t* t, const float* tabA,
                           const float* tabB, const float* wtab, int prediction, float* grad, float* target_out, float* loss_out,
                           int32_t* nan_flag, float beta, float grad_scale, int64_t B, int64_t chw, int num_t, int do_clamp, void* ws,
                           psg_stream_t stream);

/* Stage 3's reconstruction loss and its gradient in one pass - compute_generation_loss, final_trainer.py:425-440
 * (F.l1_loss + 0.1 * F.mse_loss, both means over all n elements):
 *   out3 (3 fp32 device scalars) = { w_l1 * mean|d| + w_mse * mean d^2, mean|d|, mean d^2 },  d = pred - target
 *   grad (may be NULL) = (w_l1 * sign(d) + 2 * w_mse * d) / n
 * with sign(0) = 0; the three scalars do not depend on whether grad is given.
 * Deterministic two-stage reduction.  ws: >= psg_recon_loss_workspace_bytes() bytes.  n <= 0 is PSG_ERR_SHAPE; a null pred,
 * target, out3 or ws is PSG_ERR_ARG. */
int psg_recon_loss_f32(const float* pred, const float* target, float* grad, float* out3, int64_t n, float w_l1,
                       float w_mse, void* ws, psg_stream_t stream);
int64_t psg_recon_loss_workspace_bytes(void);

/* ---------------------------------------------------------------------------
 * Stage 1's loss around the VGG16 convolutions (perceptual.hip) - src/models/losses.py: CombinedLoss = L1 + 0.1 * VGG16
 * perceptual + beta * KL, used on every batch by vae_trainer.py:214,249-286.  The convolutions are psg_conv_fwd with the ReLU
 * epilogue; these are the passes between them.  Channels-last operands are rows of C channels with a row stride ld (elements):
 * C and ld are whole 16-byte chunks (multiples of 4 for fp32, 8 for bf16) and the base is 16-byte aligned (PSG_ERR_SHAPE /
 * PSG_ERR_ALIGN otherwise).  No atomics; the same inputs give the same bits.
 * ------------------------------------------------------------------------- */
/* nn.MaxPool2d(kernel_size=2, stride=2) of torchvision's vgg16().features (indices 4, 9, 16 under losses.py:56-57): x
 * [B,Hi,Wi,C] -> y [B,Hi/2,Wi/2,C], floor (the last row / column of an odd Hi / Wi is dropped); Hi, Wi >= 2.  tap (may be
 * NULL; uint8, contiguous [B,Hi/2,Wi/2,C], 8-byte aligned) receives the winning tap 0..3, row-major inside the window.  On
 * ties the FIRST tap wins (torch.max_pool2d on the CPU replaces the maximum only by a strictly greater value).  y holds the
 * bits of the winning input.  Inputs are assumed finite. */
int psg_maxpool2x2_fwd(const void* x, int64_t ldx, void* y, int64_t ldy, uint8_t* tap, int B, int Hi, int Wi, int C,
                       int dtype, psg_stream_t stream);
/* Its backward as a gather: every element of dx [B,Hi,Wi,C] is written exactly once - the dy of its cell if it is the
 * recorded tap, else 0; the row / column an odd Hi / Wi drops gets 0.  dx needs no zero-fill. */
int psg_maxpool2x2_bwd(const void* dy, int64_t lddy, const uint8_t* tap, void* dx, int64_t lddx, int B, int Hi, int Wi,
                       int C, int dtype, psg_stream_t stream);
/* losses.py:75-81 + :51-53 (+ :137 through a, b) in one pass: img fp32 NCHW [B,3,Hi,Wi] -> y [B,Ho,Wo,8] in `dtype`,
 *   v = clamp(a * img + b, 0, 1);  v = F.interpolate(v, (Ho,Wo), 'bilinear', align_corners=False) when (Ho,Wo) != (Hi,Wi)
 *   (no resampling arithmetic at all otherwise);  y[..c] = (v - mean[c]) * inv_std[c]
 * with the ImageNet mean (0.485, 0.456, 0.406) and inv_std = fp32(1 / std), std = (0.229, 0.224, 0.225).  The resize is PyTorch's:
 * source index (in / out) * (dst + 0.5) - 0.5 clamped at 0, two taps per axis, combined in fp32 as h0 (w0 v00 + w1 v01) +
 * h1 (w0 v10 + w1 v11).  Only the formula is PyTorch's: the source index is evaluated in fp64 (torch: fp32 for an fp32 image) and each
 * weight rounded once, so fp32 results of the resize are closer to the exact one than torch's and not bit-comparable with them.
 * Any (Ho,Wo), larger or smaller.
 * Channels 3..7 are zero (the first convolution's weight is padded alike). */
int psg_image_prep_fwd(const float* img, void* y, int64_t ldy, int B, int Hi, int Wi, int Ho, int Wo, float a, float b,
                       int dtype, psg_stream_t stream);
/* Its backward as a gather: dimg (fp32 NCHW [B,3,Hi,Wi], every element written once) = (the forward's resize weights applied to
 * dy [B,Ho,Wo,8], summed in a fixed order in fp64 and rounded once; the one dy[..c] without a resize) * inv_std[c] * a where 0 <= a * img + b <= 1
 * (inclusive, as torch.clamp's gradient; the mask is recomputed from img), else 0. */
int psg_image_prep_bwd(const float* img, const void* dy, int64_t lddy, float* dimg, int B, int Hi, int Wi, int Ho, int Wo,
                       float a, float b, int dtype, psg_stream_t stream);
/* F.l1_loss of two feature maps (losses.py:89-90) and its gradient in one pass: a, b [rows, cols] in `dtype`,
 *   out2 (2 fp32 device scalars) = { mean |a - b|, scale * mean |a - b| }   (fp32 accumulation, n = rows * cols)
 *   grad (may be NULL; `dtype`) = sign(a - b) * fp32(scale / n) rounded to `dtype`, with sign(0) = 0 (as torch: after ReLU both
 *   maps are zero in many places).
 * Deterministic two-stage reduction.  ws: >= psg_feat_l1_workspace_bytes() bytes (PSG_ERR_WORKSPACE otherwise). */
int psg_feat_l1(const void* a, int64_t lda, const void* b, int64_t ldb, void* grad, int64_t ldg, float* out2, int64_t rows,
                int cols, float scale, int dtype, void* ws, int64_t ws_bytes, psg_stream_t stream);
int64_t psg_feat_l1_workspace_bytes(void);
/* losses.py:147-148: out[0] = -0.5 * sum(1 + logvar - mu^2 - exp(logvar)) / n over n fp32 elements, and (either may be NULL)
 * dmu = mu / n, dlogvar = 0.5 * (exp(logvar) - 1) / n in fp32.  The sum is taken as 0.5 * sum(mu^2 + (expm1(logvar) - logvar)),
 * every term >= 0, in fp64 in a fixed two-stage order.  ws: 8-byte aligned, >= psg_kl_workspace_bytes() bytes. */
int psg_kl_f32(const float* mu, const float* logvar, float* dmu, float* dlogvar, float* out, int64_t n, void* ws,
               int64_t ws_bytes, psg_stream_t stream);
int64_t psg_kl_workspace_bytes(void);

/* ---------------------------------------------------------------------------
 * Layout / small ops at the boundary (NCHW fp32 <-> channels-last dtype)
 * ------------------------------------------------------------------------- */
/* [B,C,HW] fp32 -> [B,HW,C] dtype (UNet.forward input, unet.py:448) and back (:507-509).  ld_dst / ld_src: the row stride of
 * the channels-last side in elements, >= C; columns C..ld-1 are neither read nor written.  B, C or HW <= 0 or ld < C is
 * PSG_ERR_SHAPE; a null pointer is PSG_ERR_ARG. */
int psg_nchw_to_nhwc(const float* src, void* dst, int64_t ld_dst, int B, int C, int HW, int dtype,
                     psg_stream_t stream);
int psg_nhwc_to_nchw(const void* src, int64_t ld_src, float* dst, int B, int C, int HW, int dtype,
                     psg_stream_t stream);
/* AdaptiveAvgPool1d(1) over tokens — unet.py:322,445: text [B,S,D] fp32 -> out[B, :D] (dtype),
 * and the dtype copy of the token embeddings themselves (text_cast, may be NULL; contiguous [B,S,D]).  Columns D..ld_pooled-1
 * are not written.  B, S or D <= 0 or ld_pooled < D is PSG_ERR_SHAPE; a null text or pooled is PSG_ERR_ARG. */
int psg_text_pool(const float* text, void* pooled, int64_t ld_pooled, void* text_cast, int B, int S,
                  int D, int dtype, psg_stream_t stream);
/* Sinusoidal features — unet.py:47-50: out[b, :half]=sin(t*coeff), out[b, half:]=cos(t*coeff),
 * accurate sinf/cosf (arguments reach 999 rad).  Columns 2*half..ld_out-1 are not written.  B or half <= 0 or
 * ld_out < 2*half is PSG_ERR_SHAPE; a null pointer is PSG_ERR_ARG. */
int psg_timestep_sinusoid(const int64_t* t, const float* coeff, void* out, int64_t ld_out, int B,
                          int half, int dtype, psg_stream_t stream);
/* nn.Upsample(size, bilinear, align_corners=False) — unet.py:365,375,385, channels-last. */
int psg_upsample_bilinear_fwd(const void* x, int64_t ldx, void* y, int64_t ldy, int B, int Hi, int Wi,
                              int Ho, int Wo, int C, int dtype, psg_stream_t stream);
int psg_upsample_bilinear_bwd(const void* dy, int64_t lddy, void* dx, int64_t lddx, int B, int Hi,
                              int Wi, int Ho, int Wo, int C, int dtype, psg_stream_t stream);
/* Which kernel pair takes an upsample launch, from the launches' own predicate and with their argument checks and error
 * codes; host only, no device is touched.  rd / ldrd: the operand a lane gathers from (forward x, backward dy), wr / ldwr:
 * the one it writes (forward y, backward dx).  out[0] = 1: the 8-channel bf16 kernel (bf16, C and both row strides
 * multiples of 8, both pointers 16-byte aligned, 32-bit offsets; backward also Wo <= 3 Wi), 0: the 4-channel kernel. */
int psg_upsample_route(int backward, int dtype, const void* rd, int64_t ldrd, const void* wr, int64_t ldwr, int B, int Hi,
                       int Wi, int Ho, int Wo, int C, int32_t* out);
/* Dropout under hipGraph replay.  Every mask in this library is a stateless hash of (seed, element index); the seeds are
 * launch arguments, so a captured train step would replay the SAME masks forever.  After psg_set_seed_source(p) every launch
 * that draws a mask adds the 64-bit word at device address p to its seed when it RUNS (conv / Linear epilogues, attention,
 * psg_dropout_apply, psg_epilogue_bwd - forward and backward of a step read the same value, so they still agree); the caller
 * advances the word on the device between steps.  NULL (default) restores the plain seeds.  Process-wide (one process per
 * GPU).  Reference: nn.Dropout / MultiheadAttention(dropout=) draw fresh masks every step (unet.py:160-187). */
int psg_set_seed_source(const uint64_t* seed_dev);

/* y = a (+ b (+ c)), b / c may be NULL (c needs b): row-strided [rows][cols] operands, 16-byte chunks (cols and row strides
 * multiples of 8 bf16 / 4 fp32), the fp32 sum rounded once.  One source: the strided copy of a skip tensor into its half of
 * the decoder's concat buffer (reference unet.py:480-504 `torch.cat([x, skip], dim=1)`: the x half is written there by
 * its producer); three: the gradient fan-in of a skip tensor (its three consumers) in one pass. */
int psg_sum_rows(const void* a, int64_t lda, const void* b, int64_t ldb, const void* c, int64_t ldc, void* y, int64_t ldy,
                 int64_t rows, int cols, int dtype, psg_stream_t stream);

/* ---------------------------------------------------------------------------
 * GroupNorm (+ fused SiLU) — unet.py:79,89,115,127,397 (eps 1e-5) and
 * :156-157,214,231 (eps 1e-6 on [B,C,L]); channels-last [B, HW, C].
 * mean/rstd: fp32 [B*G].  Biased variance, eps inside the sqrt.
 * ------------------------------------------------------------------------- */
int psg_groupnorm_fwd(const void* x, int64_t ldx, void* y, int64_t ldy, const float* gamma,
                      const float* beta, float* mean, float* rstd, int B, int HW, int C, int G,
                      float eps, int silu, int dtype, void* ws, psg_stream_t stream);
int64_t psg_groupnorm_fwd_workspace_bytes(int B, int G);
/* dx (may alias dy), dgamma/dbeta fp32 [C] (overwritten, or accumulated if accumulate!=0).
 * ws: >= psg_groupnorm_bwd_workspace_bytes(B,C) bytes. */
int psg_groupnorm_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* gamma,
                      const float* beta, const float* mean, const float* rstd, void* dx, int64_t lddx,
                      float* dgamma, float* dbeta, int B, int HW, int C, int G, int silu, int accumulate,
                      int dtype, void* ws, psg_stream_t stream);
/* Same, with the gradient of the normalised tensor's OTHER consumer added in the same pass:
 * dx = groupnorm_bwd(dy) + dres.  Every GroupNorm input of the U-Net also feeds a path that bypasses the norm
 * (ResBlock skip, unet.py:132; the attention residuals :220,238), so autograd's separate accumulation pass over
 * the activation gradient disappears.  dres may be NULL (then identical to psg_groupnorm_bwd) and may alias dx. */
int psg_groupnorm_bwd_res(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* gamma,
                          const float* beta, const float* mean, const float* rstd, const void* dres,
                          int64_t lddres, void* dx, int64_t lddx, float* dgamma, float* dbeta, int B, int HW,
                          int C, int G, int silu, int accumulate, int dtype, void* ws, psg_stream_t stream);
int64_t psg_groupnorm_bwd_workspace_bytes(int B, int C);
/* What a forward (backward = 0) or backward launch of this shape runs, from the launches' own routing functions and with
 * their shape checks and error codes; host only, no device is touched.  has_dres: a backward launch with dres != NULL.
 * out[12] = fused (1: one register-resident kernel, 0: the split kernels), N (channels per chunk), R (chunks per lane of
 * the slab plan, 0 if none; fused = 0 with R != 0: a plan was found but its LDS did not fit), grid, threads, lds (bytes,
 * the fused or the first split kernel), lds2 (second split kernel), slabC, nslab, PP (pixel lanes), NS (pixel splits),
 * pps (pixels per split).  slabC / nslab are 0 on the split route, NS / pps / lds2 on the fused one. */
int psg_groupnorm_route(int backward, int dtype, int B, int HW, int C, int G, int has_dres, int32_t* out);

/* ---------------------------------------------------------------------------
 * Implicit-GEMM convolution / linear on MFMA — nn.Conv2d 3x3 s1/s2 p1 and 1x1
 * (unet.py:80,90,96,325,335,342,349,366,376,386,399) and every nn.Linear
 * (unet.py:28-34,83,86,176,181-187 and the MHA in/out projections :160-173).
 *
 *   y[m, n] = residual[m, n] + alpha * drop(act(acc[m, n] + bias[n] + rowadd[b(m), n])) * dact'(...)
 *   acc[m, n] = sum_{kh,kw,ci} x[pix(m,kh,kw), ci] * w[n, (kh,kw,ci)]
 *
 * m indexes output pixels (b, ho, wo) row-major; a Linear is ksize=1, H=W=1.
 * `w` is a PREPARED weight [N][Kpad] (psg_prep_weight), Kpad = K rounded up to
 * the kernel's K tile.  transposed=1 gathers as the data-gradient of a strided
 * conv (x is then dY on the [Hi,Wi] grid of the forward OUTPUT, the result lives
 * on the forward INPUT grid [Ho,Wo]); with a dgrad-prepared weight this is
 * conv2d's dgrad for any stride.
 * ------------------------------------------------------------------------- */
/* PSG_CONV_SAVE_DACT (forward form): `preact` receives the epilogue's DERIVATIVE d = act'(u) * mask/(1-p) instead of
 *   the pre-activation u, so that backward multiplies by a loaded value instead of re-evaluating erf/exp and the mask.
 * PSG_CONV_DACT_MUL (backward form): `dact_u` holds that saved derivative: value *= dact_u (no act', drop_p must be 0).
 * PSG_CONV_GENERIC_EPILOGUE: run the launch through the run-time (one-step) epilogue instead of its specialised copy -
 * same results bit for bit; exists so that tests can hold the two against each other in one process. */
enum psg_conv_flags { PSG_CONV_SAVE_DACT = 1, PSG_CONV_DACT_MUL = 2, PSG_CONV_GENERIC_EPILOGUE = 4 };
typedef struct psg_conv_desc {
    int32_t dtype;               /* psg_dtype of x, w, y, rowadd, residual, preact, dact_u */
    int32_t B, Hi, Wi, Cin;      /* gather source x: [B, Hi, Wi, Cin] */
    int32_t Ho, Wo, Cout;        /* result y: [B, Ho, Wo, Cout] */
    int32_t ksize, stride, pad;  /* 1 (pad 0), 3 (pad 1), or the VAE encoder's 4 (stride 2, pad 1 or 2: forward gather only); stride 1 or 2 */
    int32_t transposed;          /* 0 forward gather, 1 data-gradient gather */
    int32_t act;                 /* psg_act applied to (acc + bias + rowadd) */
    float alpha;                 /* scale of the activated value (gates 0.7/0.8/0.6: unet.py:220,238,250) */
    float drop_p;                /* dropout probability on the activated value (0 = off) */
    int32_t flags;               /* psg_conv_flags (0 = none) */
    uint64_t drop_seed;          /* mask = hash(seed, m*Cout+n) — regenerated in backward */
    int64_t ldx, ldy, ld_rowadd, ld_residual, ld_preact, ld_dact;
    int64_t ldw;                 /* row stride of w in elements; 0 = Kpad (a column slice of a wider prepared
                                    weight is addressed with w + offset and ldw = its Kpad) */
    const void* x;
    const void* w;
    void* y;
    const float* bias;           /* [Cout] fp32 or NULL */
    const void* rowadd;          /* [B, Cout] per-sample add (time/text proj, unet.py:119-124) or NULL */
    const void* residual;        /* [M, Cout] or NULL; may alias y (accumulate) */
    void* preact;                /* optional store of (acc+bias+rowadd) for backward, or NULL */
    const void* dact_u;          /* backward form: when non-NULL, `act` is NOT applied; the value is multiplied by
                                    act'(dact_u[m,n]) (saved pre-activation) and by the same dropout mask.  Used by
                                    the FFN backward: the data gradient of its second Linear comes out already
                                    multiplied by GELU'(u) * mask of the first.  Mutually exclusive with residual. */
    void* ws;                    /* optional split-K workspace (16-byte aligned) of ws_bytes bytes, or NULL: with at least */
    int64_t ws_bytes;            /* psg_conv_fwd_workspace_bytes(d) bytes a launch whose tile grid would leave most of the
                                    chip idle (small M: the sampler of improved_diffusion_trainer.py:534-567 at 64 samples,
                                    training batches of 2-4) shares each tile's K axis among several workgroups - fp32
                                    partial tiles, summed in fixed order by a second kernel that applies the epilogue */
} psg_conv_desc;
int psg_conv_fwd(const psg_conv_desc* d, psg_stream_t stream);
int64_t psg_conv_fwd_workspace_bytes(const psg_conv_desc* d);   /* 0: the launch would not be split; < 0: bad descriptor */
/* Diagnostics: psg_conv_fwd runs pointwise layers (1x1 / Linear, bf16, whole 128 x 128 tiles, >= 1.5 tiles per resident
 * workgroup slot) on the persistent kernel of csrc/conv_pw.hip - same arithmetic, same bits.  psg_conv_set_pw(0) sends them
 * to the per-tile kernel instead (A/B runs, the bitwise test); psg_conv_pw_launches counts launches the persistent kernel took. */
int psg_conv_set_pw(int on);
int64_t psg_conv_pw_launches(void);
/* Stride-1 3x3 pad-1 bf16 launches (forward and data gradient) may run in border-class order: the output positions go class
 * by class (first / interior / last row x column), and each tile walks only the filter taps its class can reach (4, 6 or 9)
 * - the skipped taps read only padding, so the results are the same bits.  psg_conv_set_tapclass(0) turns it off (A/B runs,
 * the bitwise test), 1 (default) lets the tile plan decide per launch, 2 uses it on every launch it applies to;
 * psg_conv_tapclass_launches counts the launches that ran in class order. */
int psg_conv_set_tapclass(int on);
int64_t psg_conv_tapclass_launches(void);
/* Tile pin: c = 0..4 makes every psg_conv_fwd launch use the candidate tile 128x128, 128x64, 64x64, 128x160 or 64x160
 * instead of the plan's choice (kernel A/B runs, the route tests); -1 (any other value) gives the choice back to the plan.
 * The initial value is the environment variable PSG_CONV_TILE.  A pinned launch is never split along K (workspace or
 * not); the 160-wide tiles exist only for bf16 and not for the parity-class launches of a stride-2 3x3 data gradient:
 * pinned there, psg_conv_fwd (and psg_conv_route) return PSG_ERR_ARG and launch nothing. */
int psg_conv_set_tile(int c);
/* Host-only: which kernels psg_conv_fwd(d) would launch, and how.  Runs the descriptor checks of psg_conv_fwd (same error
 * codes) and the same planning code - honouring d->ws / ws_bytes, psg_conv_set_tile / _set_tapclass / _set_pw,
 * psg_set_available_cus and psg_set_reserve_rounds - but reads no operand, launches nothing and leaves the launch
 * counters alone (the pointers of d must only be non-NULL and aligned as psg_conv_fwd asks).
 * out[0] = number of launches (1; up to 4, one per non-empty parity class, for the data gradient of a stride-2 3x3 conv),
 * then PSG_CONV_ROUTE_FIELDS values per launch, the unused launches zero:
 *   BM, BN       tile (pixels x channels)
 *   mode         gather: 0 fast forward, 1 fast stride-1 data gradient, 2 generic per-thread decode, 3 parity class
 *   splits, kt_per_split   split-K: workgroups per tile (1 = unsplit) and K steps of each but the last
 *   tapcls       1: border-class order        pw: 1: the persistent pointwise kernel (csrc/conv_pw.hip)
 *   epi_lds      1: stores staged through LDS (bf16, unsplit, every row stride a multiple of 8); 0: direct / fp32 / split-K finish
 *   mtiles, ntiles, grid   tile counts (mtiles in class order with tapcls) and workgroups launched
 *   M, KT        GEMM rows and K steps of this launch (a parity class has its own)
 *   sub_h0, sub_w0, sub_nH, sub_nW, ntap   mode 3: first result row / column of the class, its grid, its filter taps */
#define PSG_CONV_ROUTE_FIELDS 18
#define PSG_CONV_ROUTE_MAX_LAUNCHES 4
int psg_conv_route(const psg_conv_desc* d, int32_t* out);   /* out: 1 + 4 * PSG_CONV_ROUTE_FIELDS values */

/* Weight gradient — convolution_backward's wgrad for the same layers.
 * dw (fp32) = sum_m dy[m,co] * x[pix(m,kh,kw), ci], stored in the parameter's own memory order:
 * PSG_W_OIHW dw[co][ci][kh][kw] (torch contiguous) or PSG_W_OHWI dw[co][kh][kw][ci]
 * (torch channels_last — the kernel's native order: no permute pass, and when the plan has a
 * single K split the tiles are written straight into dw).  Overwritten, or accumulated if
 * accumulate != 0.  Split-K over pixels with a deterministic fixed-order second pass.
 * ws: >= psg_conv_wgrad_workspace_bytes(...) (0 bytes / NULL allowed when that returns 0). */
enum psg_w_layout { PSG_W_OIHW = 0, PSG_W_OHWI = 1 };
typedef struct psg_wgrad_desc {
    int32_t dtype;
    int32_t B, Hi, Wi, Cin, Ho, Wo, Cout, ksize, stride, pad;
    int32_t accumulate;
    int32_t dw_layout;  /* psg_w_layout of dw */
    int32_t accumulate_bias;   /* like accumulate, for dbias */
    float scale;               /* dw, dbias = scale * (...) — 0 is read as 1 (folds a constant output gate, e.g. the
                                  0.7 / 0.8 attention gates of unet.py:220,238, into the gradient instead of a pass over dy) */
    int32_t reserved1;
    int64_t ldx, lddy;
    const void* x;    /* forward input  [B,Hi,Wi,Cin] */
    const void* dy;   /* output grad    [B,Ho,Wo,Cout] */
    float* dw;        /* Cout*Cin*k*k fp32 in dw_layout order */
    float* dbias;     /* optional [Cout] fp32: the layer's bias gradient sum_m dy[m,co], produced by the SAME launch
                         (the dY tiles are already in LDS: one extra MFMA against a ones operand per tile row) */
    void* ws;
    int64_t ws_bytes;
} psg_wgrad_desc;
int psg_conv_wgrad(const psg_wgrad_desc* d, psg_stream_t stream);
int64_t psg_conv_wgrad_workspace_bytes(const psg_wgrad_desc* d);
/* Family pin: v = 0..3 makes every psg_conv_wgrad launch run the kernel family narrow-128, narrow-160, wide or pipe (the
 * `family` values of psg_conv_wgrad_route) instead of the plan's choice (kernel A/B runs, the route tests); -1 (any other
 * value) gives the choice back to the plan.  A pin skips the plan's profitability thresholds (column waste, minimum tile
 * counts, "only where 128 does not divide Cout") and keeps what the kernels need: narrow-160, wide and pipe exist for bf16 and
 * the stride-1 same-size geometries only, narrow-160 needs Cout % 160 == 0, pipe Cout % 320 == 0, a dY extent below 2 GiB less
 * 64 rows and - with dbias - at least 10 column tiles.  Pinned where it cannot run, psg_conv_wgrad and psg_conv_wgrad_route
 * return PSG_ERR_ARG, psg_conv_wgrad_workspace_bytes -1, and nothing is launched. */
int psg_conv_wgrad_set_variant(int v);
/* Split pin: n > 0 makes every launch ask for n K splits (the environment variable PSG_WGRAD_SPLITS is the initial value; the
 * launch gets ceil(steps / ceil(steps / n)) of them); 0 returns the choice to the makespan model. */
int psg_conv_wgrad_set_splits(int n);

/* Slim weight gradient: the VAE decoder's high-resolution layers under stage 1 (src/training/vae_trainer.py) - blocks 4 and 5
 * of src/models/vae_decoder.py:163-175 (108 x 108 x 64 and 215 x 215 x 32 channels) and the 32 -> 3 image convolution - where
 * psg_conv_wgrad's 128-row tiles are three quarters padding.  Same descriptor, same result as psg_conv_wgrad, under a narrower
 * contract: dtype PSG_BF16 (PSG_ERR_DTYPE otherwise: fp32 keeps going to psg_conv_wgrad); ksize 1 (pad 0) or 3 (pad 1), stride
 * 1, Ho = Hi, Wo = Wi; Cout one of 8, 16, 32, 64; Cin a multiple of 8, at most 128; ldx >= Cin, lddy >= Cout, both multiples of
 * 8 (PSG_ERR_SHAPE); x, dy and ws 16-byte aligned (PSG_ERR_ALIGN); dw_layout, null pointers (PSG_ERR_ARG).  Everything is
 * checked on the host before any launch.  One workgroup owns all Cout rows, a 32-channel column block with all its taps and a
 * slab of 8 x 16-pixel tiles (the nine taps share one LDS image of the input tile with its halo); the slabs - their count
 * follows the pixel count and the CUs - are fp32 partials in ws (>= psg_conv_wgrad_slim_workspace_bytes, -1 for a descriptor
 * outside the contract) that a second kernel adds in a fixed order: no atomics, the same bits every run.  dbias, accumulate,
 * accumulate_bias and scale as in psg_conv_wgrad. */
int psg_conv_wgrad_slim(const psg_wgrad_desc* d, psg_stream_t stream);
int64_t psg_conv_wgrad_slim_workspace_bytes(const psg_wgrad_desc* d);
/* Split pin of psg_conv_wgrad_slim (a test hook like psg_conv4s2_wgrad_set_splits): n > 0 asks for n slabs of whole tiles (the
 * launch gets ceil(tiles / ceil(tiles / n)) of them, at most one per tile); 0 returns the choice to the plan. */
int psg_conv_wgrad_slim_set_splits(int n);
/* Host-only: which kernels psg_conv_wgrad(d) would launch, and how.  Runs the descriptor checks of
 * psg_conv_wgrad_workspace_bytes and the same plan - honouring psg_conv_wgrad_set_variant / _set_splits, the PSG_WGRAD_*
 * environment, psg_set_available_cus and psg_set_reserve_rounds - but reads no operand, initialises no device and launches
 * nothing (the pointers of d are only tested against NULL: dbias decides whether the bias gradient rides along).
 * out receives PSG_WGRAD_ROUTE_FIELDS values:
 *   family       0 narrow-128 (wgrad_kernel<T, GEOM, 128>), 1 narrow-160 (<bf16, GEOM, 160>), 2 wide (wgrad_wide_kernel),
 *                3 pipe (wgrad_pipe_kernel)
 *   dtype, geom  psg_dtype; 0 general (strided / resizing), 1 stride-1 same-size 3x3, 2 pointwise
 *   bias         1: the bias gradient rides in the kernel (dbias != NULL)
 *   BR, BQ, BKP  tile: rows (co) x columns (q = tap * Cin + ci), and the K step in pixels
 *   lds, wg_per_cu   dynamic LDS bytes of a workgroup, resident workgroups per CU
 *   rtiles, qtiles, splits, steps_per_split, grid   tile counts, K splits, K steps of each split but the last, workgroups
 *   finish       0: tiles written straight into dw, 1: wgrad_sum_kernel, 2: wgrad_reduce_kernel (OIHW 3x3)
 *   bias_finish  0: no bias gradient, 1: written directly, 2: folded into wgrad_sum_kernel, 3: wgrad_bias_sum_kernel
 *   launches     kernels launched (1..3) */
#define PSG_WGRAD_ROUTE_FIELDS 17
int psg_conv_wgrad_route(const psg_wgrad_desc* d, int32_t* out);

/* Master weight (w_dtype PSG_F32, or PSG_BF16 for the AdamW shadow copy; w_layout PSG_W_OIHW or PSG_W_OHWI memory
 * order; a bf16 source must be OHWI or 1x1) -> prepared forward weight wf [O][Kpad] with k=(kh,kw,ci) and prepared
 * data-gradient weight wd [I][Kpad'] with k=(kh,kw,co) (either may be NULL); zero K padding.  Kpad: psg_kpad(). */
/* 4x4 weights (ksize 4) must be OHWI with O and I multiples of 4 and w, wf and wd 16-byte aligned (PSG_ERR_ARG otherwise). */
int psg_prep_weight(const void* w, int w_dtype, int w_layout, void* wf, void* wd, int O, int I, int ksize, int dtype,
                    psg_stream_t stream);
/* Which kernel a psg_prep_weight launch with these arguments runs, from the launcher's own decision and with its argument
 * checks and error codes; host only, no device is touched.  out[0] = a psg_prep_kernel value: the generic kernel (fp32
 * source, any layout and channel counts, LDS transpose), the OHWI kernel on an fp32 or on a bf16 source (OHWI or 1x1, O and
 * I multiples of 4, all pointers 16-byte aligned), or the bf16 transposition that writes wd alone (no wf, O and I multiples
 * of 8). */
enum psg_prep_kernel { PSG_PREP_GENERIC = 0, PSG_PREP_OHWI_F32 = 1, PSG_PREP_OHWI_BF16 = 2, PSG_PREP_WD_BF16 = 3 };
int psg_prep_weight_route(const void* w, int w_dtype, int w_layout, const void* wf, const void* wd, int O, int I, int ksize,
                          int dtype, int32_t* out);
int64_t psg_kpad(int64_t K, int dtype);

/* ---------------------------------------------------------------------------
 * Gradients of nn.Conv2d(kernel 4, stride 2, padding 1 or 2) - the three downsampling convolutions of the VAE encoder
 * (src/models/vae_decoder.py:78-89), which stage 1 trains.  Channels-last row-strided operands in `dtype` (bf16 or fp32),
 * fp32 accumulation; Cin and Cout multiples of 8, every pointer and row 16-byte aligned, Ho = (Hi + 2 pad - 4) / 2 + 1 (Wo
 * alike).  Everything is validated on the host before a launch (PSG_ERR_ARG: null pointer, pad, cin_real, layout;
 * PSG_ERR_DTYPE; PSG_ERR_SHAPE: geometry, channel counts, a leading dimension below the channel count; PSG_ERR_ALIGN;
 * PSG_ERR_WORKSPACE).  The forward of these layers is psg_conv_fwd (ksize 4), unchanged.
 * ------------------------------------------------------------------------- */
/* Data gradient (src/models/vae_decoder.py:78-89).  g [B,Ho,Wo,Cout]: the gradient at the pre-activation; wd: the
 * data-gradient weight of psg_prep_weight(..., ksize = 4), [Cin][psg_kpad(16 Cout)] with k = (kh, kw, co); dx [B,Hi,Wi,Cin]:
 * every element is written, nothing is pre-zeroed.  Per parity class ((h+pad)&1, (w+pad)&1) of the input pixel a dense GEMM
 * of K = 4 Cout (bf16: v_mfma_f32_16x16x32_bf16; fp32: v_mfma_f32_16x16x4_f32 on fp32 operands). */
int psg_conv4s2_dgrad(const void* g, int64_t ldg, const void* wd, void* dx, int64_t lddx, int B, int Hi, int Wi, int Cin,
                      int Ho, int Wo, int Cout, int pad, int dtype, psg_stream_t stream);
/* Weight gradient (src/models/vae_decoder.py:78-89): dw[co,ci,kh,kw] = sum_{b,oh,ow} g[b,oh,ow,co] x[b,2oh-pad+kh,2ow-pad+kw,ci]
 * into an fp32 master in psg_w_layout order, of which only the first cin_real <= Cin input channels exist (the image conv
 * runs 3 channels padded to 8; its master is [32,3,4,4]); dbias (may be NULL) = column sums of g, from the same pass.
 * accumulate / accumulate_bias != 0 add into what dw / dbias hold.  M = B Ho Wo is split into fp32 partial slabs in ws
 * (>= psg_conv4s2_wgrad_workspace_bytes, 16-byte aligned), added in a fixed order by a second kernel: no atomics, bitwise
 * reproducible.  The workspace query returns -1 (and sets psg_last_error) for arguments the launch would refuse. */
int64_t psg_conv4s2_wgrad_workspace_bytes(int B, int Ho, int Wo, int Cin, int Cout, int dtype);
int psg_conv4s2_wgrad(const void* x, int64_t ldx, const void* g, int64_t ldg, float* dw, int dw_layout, int cin_real,
                      float* dbias, int B, int Hi, int Wi, int Cin, int Ho, int Wo, int Cout, int pad, int accumulate,
                      int accumulate_bias, int dtype, void* ws, int64_t ws_bytes, psg_stream_t stream);
/* Split pin of psg_conv4s2_wgrad (src/models/vae_decoder.py:78-89 has no counterpart: a test hook like
 * psg_conv_wgrad_set_splits): n > 0 asks for n slabs of whole 16-row steps (the launch gets ceil(M / rows per slab) of
 * them); 0 returns the choice to the plan. */
int psg_conv4s2_wgrad_set_splits(int n);

/* Column sums: out[g, c] = sum_{r<R} a[(g*R + r), c] for g<groups.  groups=1 gives a bias
 * gradient (fp32 out); groups=B, R=HW gives the gradient of the per-sample rowadd.  out_dtype
 * selects fp32 or bf16 output; accumulate adds into out (fp32 only).  Deterministic. */
int psg_colsum(const void* a, int64_t lda, void* out, int64_t ld_out, int64_t R, int groups, int cols,
               int dtype, int out_dtype, int accumulate, void* ws, int64_t ws_bytes, psg_stream_t stream);
int64_t psg_colsum_workspace_bytes(int64_t R, int groups, int cols);

/* Backward of the psg_conv_fwd epilogue: g[m,n] = dy[m,n] * alpha * mask(seed, m*cols+n)/(1-p) * act'(u[m,n])
 * (u = saved pre-activation, may be NULL when act == PSG_ACT_NONE). */
int psg_epilogue_bwd(const void* dy, int64_t lddy, const void* u, int64_t ldu, void* g, int64_t ldg, int64_t rows,
                     int cols, int act, float alpha, float drop_p, uint64_t seed, int dtype, psg_stream_t stream);
/* dropout backward helper: y = x * mask(seed, idx) * scale (same hash as psg_conv_fwd). */
int psg_dropout_apply(const void* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int cols,
                      float p, uint64_t seed, float scale, int dtype, psg_stream_t stream);

/* ---------------------------------------------------------------------------
 * Multi-head attention core — the scaled-dot-product inside
 * nn.MultiheadAttention (unet.py:160-173,217,235; torch/nn/functional.py
 * multi_head_attention_forward): P = softmax((q/sqrt(d)) k^T), o = drop(P) v.
 * q rows: token (b,l) at q + (b*L+l)*ldq + h*d; k, v: (b,s) at + (b*S+s)*ldk.
 * lse: fp32 [B, heads, L] (log-sum-exp of the scaled scores) saved for backward.
 * ------------------------------------------------------------------------- */
int psg_attn_fwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                 void* o, int64_t ldo, float* lse, int B, int heads, int L, int S, int d, float scale,
                 float drop_p, uint64_t seed, int dtype, psg_stream_t stream);
/* Forward with a key length per sample (the key-padding mask of a right-padded token batch, transformers'
 * BertModel attention_mask): key s of sample b takes part in the softmax only when s < kv_len[b] (int32 [B] on the
 * device, read by the kernels: no host synchronisation; values are clamped to [1, S]).  Key tiles past kv_len[b] are
 * neither loaded nor computed; queries are not masked (every l < L is computed, padded ones included).  With
 * kv_len[b] == S for every b the result is bit-identical to psg_attn_fwd.  Forward only: drop_p must be 0
 * (PSG_ERR_ARG otherwise); lse may be NULL.  Same kernel families as psg_attn_fwd (bf16 MFMA, exact-fp32 MFMA, VALU),
 * chosen by the forward's LDS need alone. */
int psg_attn_fwd_varlen(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                        void* o, int64_t ldo, float* lse, int B, int heads, int L, int S, int d, float scale,
                        float drop_p, uint64_t seed, int dtype, const int32_t* kv_len, psg_stream_t stream);
/* Training forward with a key length per sample: psg_attn_fwd_varlen's masking (kv_len int32 [B] on the device, clamped to
 * [1, S]; queries are not masked) with lse required and drop_p in [0, 1) drawing psg_attn_fwd's hash mask (same element
 * index, so the mask of a key does not depend on kv_len).  The family is chosen as psg_attn_fwd chooses it (forward and
 * backward kernels must fit LDS), so the pair with psg_attn_bwd_varlen stays on one family.  With kv_len[b] == S for every
 * b the result is bit-identical to psg_attn_fwd. */
int psg_attn_fwd_varlen_train(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                              void* o, int64_t ldo, float* lse, int B, int heads, int L, int S, int d, float scale,
                              float drop_p, uint64_t seed, int dtype, const int32_t* kv_len, psg_stream_t stream);
/* Diagnostic: launches of psg_attn_fwd / psg_attn_bwd served so far by the bf16 MFMA kernels (head_dim 16 / 32 / 64 / 80 /
 * 160 / 320, 16-byte aligned rows), by the VALU kernels (other shapes) and by the exact-fp32 MFMA kernels (fp32, head_dim
 * 16 / 32 / 64 / 80 / 160 while K/V - and Q/dO for backward - fit LDS).  All paths draw the same dropout mask. */
int psg_attn_path_counts(int64_t* mfma, int64_t* valu, int64_t* mfma_f32);
/* Diagnostic: which kernel families later psg_attn_fwd / psg_attn_bwd calls may take: bit 0 the bf16 MFMA kernels, bit 1
 * the exact-fp32 MFMA kernels; a cleared bit sends those launches to the VALU kernels (default 3).  The parity tests pin
 * each family against the same reference this way (a process-wide switch: not for concurrent use). */
int psg_attn_set_paths(int allow_mask);
/* Diagnostic, host only: what a call of this shape launches.  Initialises no device, launches nothing and leaves the
 * counters of psg_attn_path_counts alone; honours psg_attn_set_paths and PSG_ATTN_F32_MFMA.  pass: 0 psg_attn_fwd,
 * 1 psg_attn_fwd_varlen, 2 psg_attn_bwd, 3 psg_attn_fwd_varlen_train, 4 psg_attn_bwd_varlen.  ld_grads: the OR of the four
 * gradient row strides lddo | lddq | lddk | lddv (ignored for a forward); ptrs_aligned16: whether every pointer of the call
 * is 16-byte aligned (when not, the call runs on the VALU kernels).  Applies the shape, stride and dtype checks of the
 * pass's own entry point and returns its error codes (the gradient strides are checked on their OR).  out: int32
 * [PSG_ATTN_ROUTE_FIELDS] =
 *   family (0 bf16 MFMA, 1 VALU, 2 fp32 MFMA), ND (16-column slices of head_dim), waves per workgroup of the forward / dQ
 *   kernel, KW, QW (key-tile x query-group waves of the MFMA dK/dV kernels; 0 on the VALU kernels), waves of the dK/dV
 *   launch, QW reduced by the partial-sum fit, waves reduced by the private-tile fit, NH (passes over head_dim), KV_REG
 *   (K/V operands in registers), dynamic LDS bytes of the forward, dQ and dK/dV launches, grid x, y of the forward, dQ and
 *   dK/dV launches, VARLEN.  A forward pass leaves the backward fields 0 and a backward pass the forward fields. */
#define PSG_ATTN_ROUTE_FIELDS 20
int psg_attn_route(int pass, int dtype, int B, int heads, int L, int S, int d, int64_t ldq, int64_t ldk, int64_t ldv,
                   int64_t ldo, int64_t ld_grads, int ptrs_aligned16, int32_t* out);
/* delta: fp32 [B, heads, L] scratch.  dq/dk/dv have the strides of q/k/v. */
int psg_attn_bwd(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                 const void* o, int64_t ldo, const void* dout, int64_t lddo, const float* lse,
                 float* delta, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv,
                 int B, int heads, int L, int S, int d, float scale, float drop_p, uint64_t seed,
                 int dtype, psg_stream_t stream);

/* psg_attn_bwd for FEW keys and VERY MANY queries: the backward of the VAE decoder's text cross-attention
 * (src/models/vae_decoder.py:49-65: S = 32 tokens against L = 27^2 ... 215^2 pixels, head_dim 64 ... 4), which stage 3
 * differentiates to train the text encoder through the frozen decoder (final_trainer.py:215-236, :444-485).
 * Arguments as psg_attn_bwd (same layouts and strides, fp32 and bf16; q, k, v, o, dout and dq start on a 4-element
 * boundary).  head_dim is one of 4, 8, 16, 32, 64, 1 <= S <= 256, any L >= 1; drop_p must be 0 (PSG_ERR_ARG otherwise).
 * The grid is over query slabs x (b, head): each workgroup stages K / V once, recomputes P from lse for its slab, writes
 * its dq rows and one fp32 partial [2][S][d] of dk / dv into ws; a second kernel sums the partials in slab order.  No
 * atomics: the same inputs give the same bits.  ws: 16-byte aligned, at least
 * psg_attn_bwd_longq_workspace_bytes(B, heads, L, S, d) bytes (PSG_ERR_WORKSPACE otherwise).  Its own entry: psg_attn_bwd
 * never routes here, and psg_attn_path_counts does not count it. */
int psg_attn_bwd_longq(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                       const void* o, int64_t ldo, const void* dout, int64_t lddo, const float* lse,
                       float* delta, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv,
                       int B, int heads, int L, int S, int d, float scale, float drop_p, uint64_t seed,
                       int dtype, void* ws, int64_t ws_bytes, psg_stream_t stream);
int64_t psg_attn_bwd_longq_workspace_bytes(int B, int heads, int L, int S, int d);

/* psg_attn_bwd with psg_attn_fwd_varlen_train's key lengths: key tiles at or past kv_len[b] are neither staged nor
 * computed, and dk / dv rows kv_len[b] <= s < S are written as zeros (a Linear's weight gradient sums over every row).
 * Nothing stored in k or v past kv_len[b] can reach an output.  With kv_len[b] == S for every b: the bits of psg_attn_bwd.
 * For a sample with kv_len[b] < S, delta is computed in fp32 as sum_s drop(P)[l,s] dP[l,s] from the recomputed
 * probabilities rather than as rowsum(dO * O): few live keys concentrate P, dS = P (dP' - delta) then cancels (exactly at
 * kv_len = 1), and the rounding of a bf16 O inside delta would otherwise be all that is left of dk. */
int psg_attn_bwd_varlen(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                        const void* o, int64_t ldo, const void* dout, int64_t lddo, const float* lse,
                        float* delta, void* dq, int64_t lddq, void* dk, int64_t lddk, void* dv, int64_t lddv,
                        int B, int heads, int L, int S, int d, float scale, float drop_p, uint64_t seed,
                        int dtype, const int32_t* kv_len, psg_stream_t stream);

/* ---------------------------------------------------------------------------
 * BERT text encoder (src/models/text_encoder.py: transformers BertModel + projection + LayerNorm).
 * The GEMMs are psg_conv_fwd Linears, the attention is psg_attn_fwd_varlen; these are the row kernels.
 * Rows: 16-byte aligned starts (row strides multiples of 8 elements); gamma / beta / tables fp32.
 * ------------------------------------------------------------------------- */
/* y = LayerNorm(x [+ r]) * gamma + beta over each of `rows` rows of width N (multiple of 8, 8..4096): biased variance,
 * eps inside the square root, fp32 statistics in a fixed reduction order.  x and r (may be NULL) have x_dtype, y has
 * y_dtype (e.g. bf16 in, fp32 out for the encoder's final nn.LayerNorm). */
int psg_layernorm(const void* x, int64_t ldx, const void* r, int64_t ldr, void* y, int64_t ldy, const float* gamma,
                  const float* beta, int64_t rows, int N, float eps, int x_dtype, int y_dtype, psg_stream_t stream);
/* Backward of psg_layernorm.  x, r (may be NULL), N, eps: the forward's operands (the statistics are recomputed from them in
 * the forward's reduction order, nothing else is saved); dy has dy_dtype.  dz (x_dtype) is the gradient of z = x + r - the
 * one tensor serves both operands.  dgamma / dbeta: fp32 [N], either may be NULL; accumulate != 0 adds to what is there.
 * They are summed without atomics in an order fixed by (rows, N): workgroup partials go through ws (16-byte aligned, at
 * least psg_layernorm_bwd_workspace_bytes(rows, N) bytes - PSG_ERR_WORKSPACE otherwise; unused when both are NULL). */
int psg_layernorm_bwd(const void* x, int64_t ldx, const void* r, int64_t ldr, const void* dy, int64_t lddy,
                      const float* gamma, void* dz, int64_t lddz, float* dgamma, float* dbeta, int accumulate,
                      int64_t rows, int N, float eps, int x_dtype, int dy_dtype, void* ws, int64_t ws_bytes,
                      psg_stream_t stream);
int64_t psg_layernorm_bwd_workspace_bytes(int64_t rows, int N);
/* BertEmbeddings in eval mode: row b*S+s of y = LayerNorm(word_emb[ids] + type_emb[type_ids] + pos_emb[s]) (transformers'
 * summation order), y in `dtype`.  ids / type_ids: int64 [B*S] (type_ids NULL = all 0); tables fp32 row-major
 * [vocab|max_pos|type_vocab][N].  An id outside [0, vocab) or type id outside [0, type_vocab) reads nothing and yields a
 * row of NaN (the trainer's input check then skips the batch).  S > max_pos is PSG_ERR_SHAPE. */
int psg_bert_embed_ln(const int64_t* ids, const int64_t* type_ids, const float* word_emb, const float* pos_emb,
                      const float* type_emb, const float* gamma, const float* beta, void* y, int64_t ldy, int B, int S,
                      int N, int vocab, int max_pos, int type_vocab, float eps, int dtype, psg_stream_t stream);
/* Backward of psg_bert_embed_ln up to the tables.  z = (word_emb[id] + type_emb[type]) + pos_emb[s] is rebuilt from the fp32
 * tables in the forward's association and its statistics in the forward's reduction order (nothing is saved).  dy has
 * dy_dtype (row stride lddy); dz is fp32 [B*S][N] contiguous whatever dy_dtype - it is what psg_embed_scatter sums, never
 * rounded.  dgamma / dbeta / accumulate / ws: as psg_layernorm_bwd (psg_bert_embed_ln_bwd_workspace_bytes(B*S, N) bytes).  A
 * row whose id or type id is outside its table reads no table, gets a zero dz row and adds nothing to dgamma / dbeta. */
int psg_bert_embed_ln_bwd(const int64_t* ids, const int64_t* type_ids, const float* word_emb, const float* pos_emb,
                          const float* type_emb, const float* gamma, const void* dy, int64_t lddy, float* dz, float* dgamma,
                          float* dbeta, int accumulate, int B, int S, int N, int vocab, int max_pos, int type_vocab, float eps,
                          int dy_dtype, void* ws, int64_t ws_bytes, psg_stream_t stream);
int64_t psg_bert_embed_ln_bwd_workspace_bytes(int64_t rows, int N);
/* Embedding-table gradient: table_grad[k] (+)= sum of dz[perm[j]] over the run of sorted positions j with key[j] == k.
 * key: int64 [rows], ascending; perm: int64 [rows], the dz row of each sorted position (values below rows, trusted); dz fp32
 * rows of stride lddz; table_grad fp32 [V][N].  Keys outside [0, V) and key == skip_key (the padding index; -1: none)
 * contribute nothing.  No float atomics: a run's rows are added in ascending j, runs are cut at every multiple of
 * psg_embed_scatter_chunk_rows() sorted positions (at most 512), the chunks' sums go through ws and are added in chunk order,
 * so the bits depend on (key, perm, dz) alone.  accumulate == 0 writes every row of table_grad (rows no key names and row
 * skip_key: exact zeros); accumulate != 0 leaves those rows alone and stores old + (run sum), the add last.  ws: 16-byte
 * aligned, at least psg_embed_scatter_workspace_bytes(rows, N) bytes (PSG_ERR_WORKSPACE otherwise). */
int psg_embed_scatter(const float* dz, int64_t lddz, const int64_t* key, const int64_t* perm, float* table_grad, int64_t rows,
                      int N, int64_t V, int64_t skip_key, int accumulate, void* ws, int64_t ws_bytes, psg_stream_t stream);
int64_t psg_embed_scatter_workspace_bytes(int64_t rows, int N);
int psg_embed_scatter_chunk_rows(void);

/* ---------------------------------------------------------------------------
 * CLIP text-image alignment loss (clip.hip) - src/models/clip_loss.py: CLIPLoss.forward = CLIPProcessor + CLIPModel
 * (openai/clip-vit-base-patch32, frozen) + -mean(cosine), the third term of stage 3's loss (final_trainer.py:469-473).
 * The towers' GEMMs are psg_conv_fwd Linears (PSG_ACT_QUICK_GELU in the MLP), their norms psg_layernorm, the vision
 * tower's attention psg_attn_fwd / psg_attn_bwd; these are the parts CLIP alone has.  No atomics; the same inputs give the
 * same bits.
 * ------------------------------------------------------------------------- */
/* clip_loss.py:52,55 - `(image + 1) / 2` and CLIPProcessor(images=..., do_rescale=False) (transformers' CLIPImageProcessor:
 * resize to `S` bicubically, centre crop, normalise) in one pass: img fp32 NCHW [B,3,Hi,Wi] -> y, the patch rows
 * [B * (S/P)^2, 3*P*P] in `dtype` (row stride ldy >= 3*P*P): pixel (oy, ox) of channel c lands in row
 * (b * S/P + oy/P) * S/P + ox/P, column c*P*P + (oy%P)*P + ox%P - the flattening of the patch embedding's
 * Conv2d(3, width, P, stride=P, bias=False) weight (CLIPVisionEmbeddings.patch_embedding), so that embedding is one Linear.
 *   v = a * img + b;  v = resize(v) when Hi != S (no resampling arithmetic at all otherwise);  y = (v - mean[c]) * inv_std[c]
 * with CLIP's mean (0.48145466, 0.4578275, 0.40821073) and inv_std = fp32(1 / std), std = (0.26862954, 0.26130258, 0.27577711).
 * The resize is the processor's FLOAT path, F.interpolate(mode='bicubic', align_corners=False, antialias=True): per axis the
 * Keys cubic with a = -0.5 at (sample + 0.5 - centre), centre = (Hi/S)(o + 0.5), over the window
 * [trunc(centre - 1.5), trunc(centre + 2.5)) clipped to the image (at most 4 samples), the weights renormalised to sum 1;
 * no clamp, no quantisation.  Centre and weights are evaluated in fp64 and each weight rounded once (as psg_image_prep_fwd
 * takes its source index), the taps are combined in fp32, rows first.  The processor's PIL path (through uint8, overshoot
 * clipped; up to 0.41 away in normalised units on noise, not differentiable) is NOT reproduced.
 * Only Hi == Wi <= S and S % P == 0: a non-square image needs the centre crop and a larger one the widened antialias window -
 * PSG_ERR_SHAPE. */
int psg_clip_prep_fwd(const float* img, void* y, int64_t ldy, int B, int Hi, int Wi, int S, int P, float a, float b,
                      int dtype, psg_stream_t stream);
/* Its backward as a gather: dimg (fp32 NCHW [B,3,Hi,Wi], every element written once) = (the forward's weights applied to the
 * dy elements whose windows hold the pixel - a bounded set, about (4 S/Hi + 2)^2 outputs - summed in a fixed order (columns in
 * chunks of 8, rows, columns of the chunk) in fp64 and rounded once; the one dy element when Hi == S) * inv_std[c] * a.  Nothing is clamped, so there is no mask and the
 * image is not an operand. */
int psg_clip_prep_bwd(const void* dy, int64_t lddy, float* dimg, int B, int Hi, int Wi, int S, int P, float a, int dtype,
                      psg_stream_t stream);
/* CLIPTextTransformer's causal self-attention (transformers modeling_clip.py: the causal mask of CLIPTextTransformer.forward
 * inside CLIPAttention): psg_attn_fwd's operands and argument order, key s takes part for query l iff s <= l.  Padding
 * follows the pooled EOS position, so no key lengths are needed.  Forward only: L == S <= 128, head_dim 16 / 32 / 64
 * (PSG_ERR_SHAPE otherwise), drop_p must be 0 (PSG_ERR_ARG), seed is ignored, lse may be NULL.  q, k, v, o start on a
 * 4-element boundary with row strides that are multiples of 4.  One workgroup per (sample, head): K / V staged once in LDS
 * as fp32, one query row per lane, fp32 arithmetic with a running maximum; row 0 is v[0] itself.  Its own entry:
 * psg_attn_fwd never routes here, psg_attn_route and psg_attn_path_counts do not know it. */
int psg_attn_fwd_causal(const void* q, int64_t ldq, const void* k, int64_t ldk, const void* v, int64_t ldv,
                        void* o, int64_t ldo, float* lse, int B, int heads, int L, int S, int d, float scale,
                        float drop_p, uint64_t seed, int dtype, psg_stream_t stream);
/* clip_loss.py:60-67: out[0] (fp32 device scalar) = -mean_b( normalize(u[b]) . normalize(v[b]) ) for u, v [B, D] in `dtype`
 * (D and the row strides multiples of 4), F.normalize's x / max(||x||, 1e-12).  du (may be NULL; `dtype`, row stride lddu)
 * = d out / d u = -(v^ / max(||u||, eps) - [||u|| > eps] cos u / ||u||^2) / B; v gets no gradient (the text side is a
 * constant).  One pass in one workgroup, fp32 accumulation in a fixed order. */
int psg_cosine_loss(const void* u, int64_t ldu, const void* v, int64_t ldv, void* du, int64_t lddu, float* out, int B,
                    int D, int dtype, psg_stream_t stream);

/* ---------------------------------------------------------------------------
 * Optimizer side — improved_diffusion_trainer.py:399-413
 * ------------------------------------------------------------------------- */
/* out[0] (+)= sum(g^2) over n fp32 values; deterministic.  Replaces the 478 .item() syncs (:399-404).  Any n >= 1 (n need
 * not be a multiple of 4); g must be 16-byte aligned (PSG_ERR_ALIGN otherwise); ws: >= psg_reduce_workspace_bytes() bytes.
 * n <= 0 is PSG_ERR_SHAPE; a null pointer is PSG_ERR_ARG. */
int psg_sumsq_f32(const float* g, int64_t n, float* out, int accumulate, void* ws, psg_stream_t stream);
/* clip_grad_norm_ (:410) fused with AdamW (:277-283,412): coef = min(1, max_norm/(sqrt(*normsq)+1e-6))
 * read on the device (normsq may be NULL = no clipping); decoupled weight decay; step is 1-based.
 * skip_flag (may be NULL): when (*skip_flag & PSG_FLAG_SKIP_MASK) != 0 the update is skipped (NaN batch, :353-393).
 * shadow_bf16 (may be NULL): bf16 copy of the updated parameters written in the same pass, element i at
 * shadow_bf16[i] — with OHWI master weights this IS the prepared forward weight of the next step.
 * n % 4 == 0 with p, g, m, v 16-byte aligned runs a float4 kernel, anything else a scalar one with the same bits per
 * element.  The shadow exists on the float4 path only (and must itself be 8-byte aligned): PSG_ERR_ALIGN otherwise, with
 * nothing written.  n <= 0 or step < 1 is PSG_ERR_SHAPE; a null p, g, m or v is PSG_ERR_ARG. */
int psg_adamw_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, const float* normsq,
                  float max_norm, const int32_t* skip_flag, void* shadow_bf16, psg_stream_t stream);
/* The same update with the step count and the learning-rate schedule ON THE DEVICE, so that a skipped batch
 * advances neither (the reference `continue`s before optimizer.step() / scheduler.step() / global_step += 1,
 * :353-393,412-418) without a host read of the flag: step = *step_dev + 1 (1-based, bias correction computed in
 * the kernel), lr = lr_table[k], beta1 = beta1_table[k] with k = min(step - 1, sched_len - 1) (entry k = the values
 * the reference's scheduler holds after k scheduler.step() calls; OneCycleLR (:313-319) cycles Adam's beta1 along
 * with the lr; beta1_table may be NULL = constant beta1), and *step_dev += 1 after the update unless skipped.
 * n <= 0 or sched_len < 1 is PSG_ERR_SHAPE; a null p, g, m, v, lr_table or step_dev is PSG_ERR_ARG; the shadow as above. */
int psg_adamw_dev_f32(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_table,
                      const float* beta1_table, int sched_len, float beta1, float beta2, float eps,
                      float weight_decay, int32_t* step_dev, const float* normsq, float max_norm,
                      const int32_t* skip_flag, void* shadow_bf16, psg_stream_t stream);
/* psg_adamw_dev_f32 with an exponential moving average of the parameters kept IN THE SAME PASS (the reference has none: an
 * opt-in of this project).  p, m, v, the optional bf16 shadow and *step_dev get psg_adamw_dev_f32's bits; and with p' the
 * parameter value just computed, still in registers,
 *     ema[i] = fl( fl(d * ema[i]) + fl(fl(1 - d) * p'[i]) )
 * - two products and one sum, each rounded to nearest on its own (__fmul_rn / __fadd_rn / __fsub_rn: no FMA).
 * d = ema_decay when ema_warmup == 0, else d = min(ema_decay, fl(fl(1 + k) / fl(10 + k))) with k = (float)(*step_dev + 1), the
 * 1-based step the bias correction uses: formed once per thread, in fp32, from the device's own step count, so that a
 * captured graph warms up without host arithmetic.  A skipped step ((*skip_flag & PSG_FLAG_SKIP_MASK) != 0) writes nothing
 * at all, ema included.  ema: n fp32 values, not overlapping the other operands; 16-byte aligned it keeps the float4
 * kernel (10 x 16-byte loads in flight per lane, 38 instead of 30 bytes per parameter with the shadow), otherwise the
 * scalar kernel runs with the same bits per element (and the shadow is refused as above).  Checked on the host before
 * anything is launched: a null ema is PSG_ERR_ARG, ema_decay outside [0, 1) (NaN included) is PSG_ERR_SHAPE, everything else
 * as psg_adamw_dev_f32. */
int psg_adamw_dev_ema_f32(float* p, const float* g, float* m, float* v, int64_t n, const float* lr_table,
                          const float* beta1_table, int sched_len, float beta1, float beta2, float eps,
                          float weight_decay, int32_t* step_dev, const float* normsq, float max_norm,
                          const int32_t* skip_flag, void* shadow_bf16, float* ema, float ema_decay, int ema_warmup,
                          psg_stream_t stream);
/* a[i] <-> b[i] for n fp32 values, in place (the masters and their EMA change places: contents move, pointers do not).
 * float4 where n % 4 == 0 and both are 16-byte aligned, scalar otherwise.  A null pointer is PSG_ERR_ARG; n <= 0 or a == b
 * is PSG_OK with nothing launched; ranges that overlap without being equal are PSG_ERR_ARG. */
int psg_swap_f32(float* a, float* b, int64_t n, psg_stream_t stream);
/* Grouped forms (stage 1, src/training/vae_trainer.py:164-187,341-342: the VAE and the text encoder under one optimizer with
 * their own learning rate, and one clip_grad_norm_ each).  One flat fp32 arena of n floats is split into G consecutive
 * groups, 1 <= G <= PSG_OPT_MAX_GROUPS: group i covers the floats [bounds[i], bounds[i+1]).  bounds is a HOST array of G+1
 * values with bounds[0] == 0, bounds[G] == n, non-decreasing (PSG_ERR_SHAPE otherwise, as for G out of range or n <= 0), each
 * a multiple of 8 floats (PSG_ERR_ALIGN, as for a buffer that is not 16-byte aligned); null pointers are PSG_ERR_ARG.  All of
 * it is checked on the host before anything is launched.  An empty group (bounds[i] == bounds[i+1]) is legal.  Whole
 * workgroups are assigned to groups on the host, in proportion to the groups' sizes and at least one per non-empty group.
 *
 * psg_sumsq_groups_f32: out[i] (device, G floats) = sum(g^2) over group i (0 for an empty one), every group in one pass over
 * the arena plus one finishing launch; fixed reduction order, no atomics - the same input gives the same bits.  ws: at least
 * psg_reduce_workspace_bytes() bytes. */
#define PSG_OPT_MAX_GROUPS 8
int psg_sumsq_groups_f32(const float* g, int64_t n, const int64_t* bounds, int G, float* out, void* ws, psg_stream_t stream);
/* psg_adamw_dev_f32's update (the same arithmetic per element; no bf16 shadow, constant beta1) in ONE launch over all
 * groups, group i with lr[i], weight_decay[i] (HOST arrays of G floats) and
 * coef_i = min(1, max_norm[i] / (sqrt(normsq[i]) + 1e-6)): normsq is a device array of G floats (psg_sumsq_groups_f32's
 * out) or NULL = no clipping in any group (max_norm, a host array of G floats, may then be NULL too).  Bias correction from
 * *step_dev + 1; *step_dev += 1 once per call unless (*skip_flag & PSG_FLAG_SKIP_MASK) != 0 (skip_flag may be NULL), in
 * which case nothing is written at all. */
int psg_adamw_groups_f32(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* bounds, int G,
                         const float* lr, const float* weight_decay, const float* max_norm, float beta1, float beta2,
                         float eps, int32_t* step_dev, const float* normsq, const int32_t* skip_flag, psg_stream_t stream);
/* psg_adamw_groups_f32 with CLIP SETS (stage 3's joint phase, src/training/final_trainer.py:480-483: ONE clip_grad_norm_ over
 * groups that keep their own learning rates).  clip_set is a HOST array of G values in 0..G-1; groups with the same value are
 * clipped together: coef_i = min(1, max_norm[i] / (sqrt(sum_{j ascending, clip_set[j] == clip_set[i]} normsq[j]) + 1e-6)).
 * Every workgroup forms its set's sum itself, in ascending group order: no extra launch, no atomics, the same bits on every
 * run.  clip_set == NULL = every group its own set, and that or the identity map gives psg_adamw_groups_f32's bits (which is
 * this entry with NULL).  An empty group inside a set contributes 0.  Checked on the host before anything is launched:
 * clip_set[i] outside 0..G-1, or two groups of one set with different max_norm (one clip_grad_norm_ call has one max norm):
 * PSG_ERR_SHAPE; clip_set non-NULL while normsq or max_norm is NULL: PSG_ERR_ARG. */
int psg_adamw_groups_sets_f32(float* p, const float* g, float* m, float* v, int64_t n, const int64_t* bounds, int G,
                              const float* lr, const float* weight_decay, const float* max_norm, const int32_t* clip_set,
                              float beta1, float beta2, float eps, int32_t* step_dev, const float* normsq,
                              const int32_t* skip_flag, psg_stream_t stream);
/* g *= min(1, max_norm/(sqrt(*normsq)+1e-6)) — plain clip for callers that keep torch.optim.  A coefficient >= 1 writes
 * nothing.  n <= 0 is PSG_OK with nothing launched; a null g or normsq is PSG_ERR_ARG. */
int psg_clip_scale_f32(float* g, int64_t n, const float* normsq, float max_norm, psg_stream_t stream);

/* ---------------------------------------------------------------------------
 * Sprite batches from a device-resident dataset (sprites.hip): the train pipeline of the reference's loader
 * (src/data/dataset_improved.py:150-158 + :144-148: RandomHorizontalFlip, RandomRotation(10), ColorJitter,
 * RandomResizedCrop, ToTensor, Normalize) as one gather per output pixel, with the intermediate uint8 roundings of
 * the PIL chain removed and its clipping kept.
 *
 * src: uint8 [N, S, S, 4] (R, G, B, unused: one dword per pixel), composited on the background colour.
 * idx: int64 [B], the row of src each sample reads; a value outside [0, N) yields NaN for that sample, never an
 *      out-of-bounds read.
 * params: fp32 [B, PSG_SPRITE_PARAMS], per sample
 *   [0]      flip (0 or 1)
 *   [1..6]   a b c d e f of the inverse rotation: xin = a(u+.5) + b(v+.5) + c, yin = d(u+.5) + e(v+.5) + f; the rotated
 *            image's pixel (u, v) is the flipped image's pixel (floor xin, floor yin), black outside
 *   [7]      order of the four colour ops: index 0..23 of the lexicographic permutations of (0 brightness, 1 contrast,
 *            2 saturation, 3 hue); the k-th entry of the permutation is the k-th op applied
 *   [8..11]  brightness, contrast, saturation factors and the hue shift in turns; factor 1 (hue 0) skips the op
 *   [12..15] crop box top i, left j, height h, width w (integers; 1 <= h, w and i + h, j + w <= S)
 * The identity row (0, 1,0,0,0,1,0, 0, 1,1,1,0, 0,0,S,S) gives ((p / 255) - 0.5) / 0.5 of the stored pixel, bitwise.
 * ------------------------------------------------------------------------- */
#define PSG_SPRITE_PARAMS 16
/* mean[b]: mean luma ((19595 R + 38470 G + 7471 B) / 65536) over the S*S pixels of sample b's image as the contrast
 * op meets it: flipped, rotated (black corners included), the colour ops in front of contrast applied.  Fixed-order
 * reduction (lane, wave, block): bitwise reproducible.  A sample whose contrast factor is 1 gets 0. */
int psg_sprite_contrast_mean(const uint8_t* src, int64_t N, const int64_t* idx, const float* params, float* mean,
                             int B, int S, psg_stream_t stream);
/* out: fp32 [B, 3, S, S] in [-1, 1].  Output pixel (y, x): 2-tap bilinear up-scale of the crop box (taps clamped to the
 * box), each of the four taps fetched through rotation and flip and run through the colour ops (contrast blends with
 * mean[b]), then combined and normalised. */
int psg_sprite_augment(const uint8_t* src, int64_t N, const int64_t* idx, const float* params, const float* mean,
                       float* out, int B, int S, psg_stream_t stream);
/* The text inputs of a batch from the resident token table (data.TokenTable): table int32 [N, L], the tokenizer's ids of
 * every dataset row, right-padded; lens int32 [N], each row's token count; idx int64 [B] as above.  With
 * n = min(lens[idx[b]], S):  ids[b, s] = s < n ? table[idx[b], s] : pad_id,  mask[b, s] = s < n  (both int64 [B, S], what
 * the tokenizer's padding=True call returns when S is the longest row of the batch),  kv_len[b] = n (int32 [B]).  An idx[b]
 * outside [0, N) yields a row of pad_id, a zero mask and kv_len 0, never an out-of-bounds read.  Asynchronous on `stream`,
 * no allocation, any B and any S up to L.  PSG_ERR_ARG: null pointer; PSG_ERR_SHAPE: non-positive N, L, B or S, S > L, B above
 * 65535. */
int psg_token_batch(const int32_t* table, const int32_t* lens, int64_t N, int L, const int64_t* idx, int B, int S,
                    int32_t pad_id, int64_t* ids, int64_t* mask, int32_t* kv_len, psg_stream_t stream);

/* ---------------------------------------------------------------------------
 * The two ends of the demo's generation path (imaging.hip) - PokemonGradioGenerator, gradio_app.py:394-465: an uploaded
 * image in (pil_to_tensor), the latent / noise blend, uint8 sprites out (tensor_to_pil).
 * ------------------------------------------------------------------------- */
/* gradio_app.py:443-452 - `image.resize((215, 215), Image.Resampling.LANCZOS)`, then ToTensor and `(t - 0.5) * 2`.  PIL's
 * 8-bit separable resample (Resample.c) driven by integer coefficient tables, any filter, any sizes:
 *   src  uint8 [B, Hin, Win, C], interleaved channels, C in 1..4, every channel on its own
 *   per axis: bounds int32 [out, 2] = (first input index, tap count) and coef int32 [out, k] (22-bit fixed point, zero-padded
 *        rows of the table width k).  k == 0: PIL skips the pass (then the sizes must be equal and the tables are not read);
 *        both 0: a copy.  bounds is passed twice: *bounds_host is a HOST copy, checked here before anything is launched, and
 *        *bounds the DEVICE copy the kernels read (they cut every row to the input as well, so even a device copy that
 *        differs never reads outside src)
 *   the horizontal pass runs first: acc = 1 << 21; acc += pixel * coef per tap (int32); (acc >> 22) clamped to 0..255 and
 *        stored as uint8 [B, Hin, Wout, C] in ws (>= B * Hin * Wout * C bytes, when both passes run) before the vertical
 *        pass reads it - PIL's arithmetic, so the bytes are PIL's
 *   out_u8  uint8 [B, Hout, Wout, C], and / or
 *   out_f32 fp32 NCHW [B, 3, Hout, Wout] = lut[byte] of the first three channels (needs C >= 3): lut is the caller's 256-entry
 *        fp32 table of the reference's own expression, which fuses ToTensor + normalise into the last pass bit-exactly
 * The kernels loop over taps (tap counts are unbounded) and touch pixels one byte at a time (any row alignment).  Checked on
 * the host before any launch: null pointers (src, both outputs, a table of a pass that runs, lut with out_f32: PSG_ERR_ARG),
 * non-positive sizes, C outside 1..4, a side above 131072 or B above 65535, k < 0, a skipped pass between different sizes, a
 * bounds row with first < 0, taps > k or first + taps past the input (PSG_ERR_SHAPE), ws too small (PSG_ERR_WORKSPACE). */
int psg_resample_u8(const uint8_t* src, uint8_t* out_u8, float* out_f32, const float* lut, int B, int Hin, int Win, int C,
                    int Hout, int Wout, const int32_t* xbounds_host, const int32_t* xbounds, const int32_t* xcoef, int kx,
                    const int32_t* ybounds_host, const int32_t* ybounds, const int32_t* ycoef, int ky, void* ws,
                    int64_t ws_bytes, psg_stream_t stream);
/* tensor_to_pil's arithmetic, gradio_app.py:456-465 (and improved_diffusion_trainer.py generate_samples): fp32 image
 * [B, 3, H, W] addressed by element strides (a contiguous NCHW tensor and a channels_last one both go in as they are) ->
 * uint8 [B, H, W, 3] contiguous; per element, in fp32 and in the reference's order: (t + 1.0) / 2.0, clamp to [0, 1], * 255,
 * truncate toward zero.  NaN gives 0.  PSG_ERR_ARG: null pointer; PSG_ERR_SHAPE: non-positive size, B or H above 65535, W
 * above 131072, a negative stride. */
int psg_image_to_u8(const float* img, int64_t stride_b, int64_t stride_c, int64_t stride_h, int64_t stride_w, uint8_t* out,
                    int B, int H, int W, psg_stream_t stream);
/* gradio_app.py:426 - `latent * (1 - noise_strength) + noise * noise_strength`: out = fl(fl(a * c0) + fl(b * c1)) per
 * element with c0 = fp32(1 - s), c1 = fp32(s), which is how torch applies a Python scalar to an fp32 tensor.  out may not
 * alias a or b.  PSG_ERR_ARG: null pointer; PSG_ERR_SHAPE: n <= 0 or above 2^31. */
int psg_latent_mix_f32(const float* a, const float* b, float c0, float c1, float* out, int64_t n, psg_stream_t stream);

/* ---------------------------------------------------------------------------
 * Measurement hooks (bench.py): between begin and end every launch of the matrix / attention /
 * GroupNorm kernel families is bracketed by hipEvents on its stream.  end() drains once and
 * returns, per family k < nkinds (0 conv fwd gather, 1 conv data-gradient gather, 2 wgrad,
 * 3 attention, 4 GroupNorm): summed kernel milliseconds, summed algorithmic work (FLOPs for
 * 0-3, bytes for 4) and launch count.  Off by default: no cost on the product path.
 * ------------------------------------------------------------------------- */
/* Planning input: the number of CUs the tile / split-K choosers of psg_conv_fwd and psg_conv_wgrad may count on (default
 * 256 = the whole MI355X; 0 restores it).  A data-parallel step that overlaps the RCCL all-reduce with backward sets it to
 * 256 minus the CUs the collective's channels occupy, so a launch planned as ONE round of workgroups does not become two. */
int psg_set_available_cus(int n);
/* ... r > 0: only launches that would take at most r rounds of workgroups on the whole chip plan around the reserve (a
 * one-round grid doubles when CUs are taken; a many-round grid loses the CU share either way); 0: every launch (default). */
int psg_set_reserve_rounds(int r);
/* Measurement helpers (tools/contention.py): a HIP stream restricted to n_cus CUs (hipExtStreamCreateWithCUMask; the CUs
 * taken out are spread evenly over the 8 XCDs), to rehearse the step with part of the chip occupied by a collective. */
int psg_stream_create_cu_mask(int n_cus, psg_stream_t* stream);
int psg_stream_destroy(psg_stream_t stream);
int psg_profile_begin(void);
int psg_profile_end(double* ms, double* work, int64_t* launches, int nkinds);
/* Algorithmic operand bytes (each input / output / weight element once) summed per family over the launches the last
 * psg_profile_end() accounted for: printed beside the PMC traffic so the re-read ratio needs no derivation. */
int psg_profile_bytes(double* bytes, int nkinds);

#ifdef __cplusplus
}
#endif
#endif /* PSG_HIP_H */
