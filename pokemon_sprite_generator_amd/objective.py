"""The training objective beyond uniform eps regression: v-prediction and Min-SNR-gamma loss weighting.  Neither
exists in the reference; both are opt-in, and without them every launch of the step and of the samplers is what it was.

  * `min_snr_weights` - the host side: the [T] fp32 weight table (fp64 arithmetic on the fp32 `alphas_cumprod`, rounded once).
  * `diffusion_loss` - psg_diffusion_loss_f32: the weighted SmoothL1 and its gradient in ONE launch that builds its target
    (eps, or v = sqrt(abar) eps - sqrt(1 - abar) x0) in registers from (x0, noise, t); `v_target` returns that target.
  * `pred_to_eps` - psg_pred_to_eps_f32: the guidance combine and v -> eps for the chains that keep their reference update.
The DDIM step of a v-predicting network is psg_guided_update_pred_f32 (guidance.DdimRun).
"""
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

EPSILON, V_PREDICTION = "epsilon", "v_prediction"
PRED_EPS, PRED_V = (_lib.ABI.constants[n] for n in ("PSG_PRED_EPS", "PSG_PRED_V"))
_CODES = {EPSILON: PRED_EPS, "eps": PRED_EPS, V_PREDICTION: PRED_V, "v": PRED_V}


def prediction_code(prediction) -> int:
    """enum psg_prediction of "epsilon" / "v_prediction" (or of the code itself); None is "epsilon"."""
    if prediction is None:
        return PRED_EPS
    if isinstance(prediction, str):
        if prediction not in _CODES:
            raise ValueError(f'prediction type {prediction!r} ("{EPSILON}" or "{V_PREDICTION}")')
        return _CODES[prediction]
    if int(prediction) not in (PRED_EPS, PRED_V):
        raise ValueError(f"prediction code {prediction} (PSG_PRED_EPS = {PRED_EPS}, PSG_PRED_V = {PRED_V})")
    return int(prediction)


def prediction_name(prediction) -> str:
    return V_PREDICTION if prediction_code(prediction) == PRED_V else EPSILON


def min_snr_weights(alphas_cumprod, gamma: float, prediction=EPSILON) -> torch.Tensor:
    """[T] fp32 (CPU): the Min-SNR-gamma weight of every timestep, fp64 from the fp32 table values, one rounding.

    With snr = abar / (1 - abar):   epsilon       w = min(snr, gamma) / snr       = min(1, gamma (1 - abar) / abar)
                                    v_prediction  w = min(snr, gamma) / (snr + 1) = min(abar, gamma (1 - abar))
    evaluated in the right-hand forms, which need no snr: abar is first clipped to [0, 1], and the two ends are the limits
      abar -> 1 (snr -> inf):  both weights -> 0, and are exactly 0 at abar = 1;
      abar -> 0 (snr -> 0):    epsilon -> 1 (min(snr, gamma) = snr: the ratio is 1 on the whole untruncated side, and is
                               defined as 1 at abar = 0), v_prediction -> 0.
    No entry is NaN or infinite.  gamma <= 0 (or NaN) raises."""
    gamma = float(gamma)
    if not gamma > 0:
        raise ValueError(f"min_snr_weights: gamma={gamma} must be > 0")
    abar = np.asarray(torch.as_tensor(alphas_cumprod).detach().cpu().to(torch.float32).numpy(), dtype=np.float64).reshape(-1)
    if np.isnan(abar).any():
        raise ValueError("min_snr_weights: alphas_cumprod holds a NaN")
    abar = np.clip(abar, 0.0, 1.0)
    cap = gamma * (1.0 - abar)
    if prediction_code(prediction) == PRED_V:
        w = np.minimum(abar, cap)
    else:
        w = np.where(cap >= abar, 1.0, cap / np.where(abar > 0, abar, 1.0))
    return torch.from_numpy(w.astype(np.float32))


def _lib_for(t):
    if not t.is_cuda:
        raise _lib.PsgError("the diffusion objective needs GPU tensors (HIP path only; no CPU fallback)")
    return _lib.init(t.device.index if t.device.index is not None else torch.cuda.current_device())


def _f32c(t, what):
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous fp32")
    return t


def diffusion_loss(pred, x0, noise, t, scheduler, prediction=EPSILON, wtab: Optional[torch.Tensor] = None, beta: float = 0.1,
                   clamp: bool = True, want_grad: bool = True, flag: Optional[torch.Tensor] = None, loss_out=None, target_out=None,
                   grad_scale: float = 1.0):
    """psg_diffusion_loss_f32 -> (loss [1] fp32 on the device, dL/dpred or None).

    pred, noise (and x0 for v_prediction; None is allowed for epsilon) [B, ...], t [B]; `scheduler`: the NoiseScheduler whose
    sqrt tables built the noisy latent; `clamp`: whether add_noise clamped x0 to +-3 (the target must use the same x0);
    wtab: [T] fp32 on the device (min_snr_weights) or None for weight 1; flag: int32 [1] device word, OR-ed (never cleared).
    loss = mean over ALL elements of w_t smoothl1_beta(pred - target).  target_out: an fp32 tensor like pred that receives
    the target."""
    lib = _lib_for(pred)
    code = prediction_code(prediction)
    dev = pred.device
    scheduler.to(dev)
    pred_c = pred.detach().contiguous()
    if pred_c.dtype != torch.float32:
        pred_c = pred_c.float()
    nz = noise.detach().to(dev).contiguous().float()
    B = pred_c.shape[0]
    chw = pred_c.numel() // max(B, 1)
    tt = t.detach().to(device=dev, dtype=torch.int64).contiguous()
    if nz.shape != pred_c.shape or tt.numel() != B:
        raise ValueError(f"diffusion_loss: shapes pred {tuple(pred_c.shape)}, noise {tuple(nz.shape)}, t {tuple(tt.shape)}")
    x0c = None
    if code == PRED_V:
        if x0 is None:
            raise ValueError("diffusion_loss: v_prediction needs x0")
        x0c = x0.detach().to(dev).contiguous().float()
        if x0c.shape != pred_c.shape:
            raise ValueError(f"diffusion_loss: shapes pred {tuple(pred_c.shape)}, x0 {tuple(x0c.shape)}")
    if wtab is not None:
        _f32c(wtab, "diffusion_loss: wtab")
        if wtab.device != dev or wtab.numel() != scheduler.num_timesteps:
            raise ValueError(f"diffusion_loss: wtab needs {scheduler.num_timesteps} entries on {dev}")
    if target_out is not None and (_f32c(target_out, "diffusion_loss: target_out").shape != pred_c.shape or target_out.device != dev):
        raise ValueError("diffusion_loss: target_out must be like pred")
    loss = loss_out if loss_out is not None else torch.zeros(1, dtype=torch.float32, device=dev)
    grad = torch.empty_like(pred_c) if want_grad else None
    if B == 0:
        return loss, grad
    ws = _lib.workspace(lib.psg_reduce_workspace_bytes(), dev)
    check(lib.psg_diffusion_loss_f32(ptr(pred_c), ptr(x0c), ptr(nz), ptr(tt), ptr(scheduler.sqrt_alphas_cumprod),
                                     ptr(scheduler.sqrt_one_minus_alphas_cumprod), ptr(wtab), code, ptr(grad), ptr(target_out), ptr(loss),
                                     ptr(flag), float(beta), float(grad_scale), B, chw, scheduler.num_timesteps, int(bool(clamp)), ptr(ws),
                                     stream_ptr()), "psg_diffusion_loss_f32")
    return loss, grad


def v_target(x0, noise, t, scheduler, clamp: bool = True, prediction=V_PREDICTION) -> torch.Tensor:
    """The regression target of `prediction` as the loss kernel builds it: sqrt(abar_t) noise - sqrt(1 - abar_t) clamp?(x0)
    (fp32, two rounded products and one rounded subtraction), or `noise` itself for epsilon."""
    nz = noise.detach().contiguous().float()
    out = torch.empty_like(nz)
    diffusion_loss(nz, x0, nz, t, scheduler, prediction, None, 0.1, clamp, want_grad=False, target_out=out)
    return out


def pred_to_eps(x, pred_c, pred_u, w: float, scheduler, t_dev, prediction=EPSILON, out=None) -> torch.Tensor:
    """psg_pred_to_eps_f32: the guided prediction (pred_u + w (pred_c - pred_u), or pred_c when pred_u is None) as eps; for
    v_prediction eps = sqrt(1 - abar_t) x + sqrt(abar_t) p with t read from `t_dev` (int32 [1] on the device).  Contiguous
    fp32 operands of one size; `out` may be pred_c.  `scheduler`: a NoiseScheduler, or the pair (sqrt(abar), sqrt(1 - abar))
    of fp32 [T] device tables of any other schedule."""
    lib = _lib_for(pred_c)
    code = prediction_code(prediction)
    if isinstance(scheduler, (tuple, list)):
        tabA, tabB = (_f32c(v, "pred_to_eps: table") for v in scheduler)
        if tabA.device != pred_c.device or tabB.device != pred_c.device or tabA.numel() != tabB.numel() or tabA.numel() < 1:
            raise ValueError("pred_to_eps: the two tables must be on the operands' device and of one length")
        num_t = tabA.numel()
    else:
        scheduler.to(pred_c.device)
        tabA, tabB, num_t = scheduler.sqrt_alphas_cumprod, scheduler.sqrt_one_minus_alphas_cumprod, scheduler.num_timesteps
    if out is None:
        out = torch.empty_like(pred_c)
    for v in (pred_c, out) + ((pred_u,) if pred_u is not None else ()) + ((x,) if code == PRED_V else ()):
        if v is None or v.dtype != torch.float32 or not v.is_contiguous() or v.numel() != pred_c.numel():
            raise ValueError("pred_to_eps: operands must be contiguous fp32 of one size")
    if t_dev.dtype != torch.int32 or t_dev.device != pred_c.device:
        raise ValueError("pred_to_eps: t_dev must be an int32 device scalar")
    check(lib.psg_pred_to_eps_f32(ptr(x if code == PRED_V else None), ptr(pred_c), ptr(pred_u), float(w), ptr(tabA), ptr(tabB), num_t,
                                  ptr(t_dev), code, ptr(out), pred_c.numel(), stream_ptr()), "psg_pred_to_eps_f32")
    return out
