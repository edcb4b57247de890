"""Classifier-free guidance and a DDIM sampler on the HIP kernels.  Neither exists in the reference; both are
opt-in, and without them every launch of the step and of the existing samplers is what it was.

  * `ddim_timesteps`, `ddim_tables` - the host side of the schedule: k strictly descending timesteps and the [5, k] fp32
    table `psg_guided_update_f32` reads (fp64 arithmetic on the fp32 `alphas_cumprod`, rounded once).  Schedule-agnostic.
  * `text_cond_drop`, `cfg_combine` - the two small launches: the per-sample text drop of training and
    eps_u + w (eps_c - eps_u) for the chains that keep their own reference update (a v-predicting network goes through
    objective.pred_to_eps instead, one launch as well).
  * `DdimRun` / `ddim_sample` - the chain.  Guided, ONE U-Net forward runs at batch 2n on [x; x] with the text
    [text; null_text], and ONE launch combines the two halves of its output, takes the DDIM step in place on the first half of
    the input and writes the same values to the second half; nothing is copied or concatenated between steps.

Guidance on a checkpoint trained without `cond_drop_prob` runs, but the U-Net has never seen the null text: the
"unconditional" half is then an arbitrary prediction and the guided sample means nothing.
"""
import logging
import os
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .objective import PRED_EPS, pred_to_eps, prediction_code


def _lib_for(t):
    if not t.is_cuda:
        raise _lib.PsgError("guidance and the DDIM sampler need GPU tensors (HIP path only; no CPU fallback)")
    return _lib.init(t.device.index if t.device.index is not None else torch.cuda.current_device())


# ------------------------------------------------------------------------------------------------------- schedule side
def ddim_timesteps(T: int, k: int) -> np.ndarray:
    """k strictly descending integer timesteps from T - 1 to 0 (int64): t_j = round-half-up((T - 1) (k - 1 - j) / (k - 1)) in
    integers; k = 1 gives [T - 1]."""
    T, k = int(T), int(k)
    if not 1 <= k <= T:
        raise ValueError(f"ddim_timesteps: need 1 <= k <= T, got k={k} T={T}")
    if k == 1:
        return np.array([T - 1], dtype=np.int64)
    return np.array([((T - 1) * (k - 1 - j) * 2 + (k - 1)) // (2 * (k - 1)) for j in range(k)], dtype=np.int64)


def ddim_tables(alphas_cumprod, timesteps, eta: float = 0.0) -> torch.Tensor:
    """[5, k] fp32 (CPU), rows S0 = sqrt(a_t), S1 = sqrt(1 - a_t), P0 = sqrt(a_p), P1 = sqrt(max(1 - a_p - sigma^2, 0)),
    SG = sigma, with a_t = abar[t_j], a_p = abar[t_{j+1}] (1 after the last step) and
    sigma = eta sqrt((1 - a_p) / (1 - a_t)) sqrt(max(1 - a_t / a_p, 0)).  fp64 from the fp32 table values, one rounding."""
    abar = np.asarray(torch.as_tensor(alphas_cumprod).detach().cpu().to(torch.float32).numpy(), dtype=np.float64)
    ts = np.asarray(timesteps, dtype=np.int64).reshape(-1)
    if ts.size < 1 or int(ts.min()) < 0 or int(ts.max()) >= abar.size:
        raise ValueError("ddim_tables: timesteps outside the schedule")
    eta = float(eta)
    if eta < 0:
        raise ValueError(f"ddim_tables: eta={eta} < 0")
    a_t = abar[ts]
    a_p = np.concatenate([abar[ts[1:]], [1.0]])
    sigma = eta * np.sqrt((1.0 - a_p) / (1.0 - a_t)) * np.sqrt(np.maximum(1.0 - a_t / a_p, 0.0))
    rows = [np.sqrt(a_t), np.sqrt(1.0 - a_t), np.sqrt(a_p), np.sqrt(np.maximum(1.0 - a_p - sigma * sigma, 0.0)), sigma]
    return torch.from_numpy(np.stack(rows).astype(np.float32))


# ------------------------------------------------------------------------------------------------------ the two launches
def text_cond_drop(text: torch.Tensor, null_text: torch.Tensor, p: float, seed: int, dropped: Optional[torch.Tensor] = None):
    """psg_text_cond_drop_f32: (out [B, S, D] fp32, dropped int32 [B]).  null_text: [S, D] (or [1, S, D])."""
    lib = _lib_for(text)
    txt = text.detach().contiguous().float()
    B = txt.shape[0]
    row = txt.numel() // max(B, 1)
    null = null_text.detach().to(device=txt.device, dtype=torch.float32).contiguous()
    if null.numel() != row:
        raise ValueError(f"text_cond_drop: null_text has {null.numel()} elements, one sample of text has {row}")
    out = torch.empty_like(txt)
    if dropped is None:
        dropped = torch.zeros((B,), dtype=torch.int32, device=txt.device)
    if B:
        check(lib.psg_text_cond_drop_f32(ptr(txt), ptr(null), ptr(out), ptr(dropped), B, row, float(p), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                         stream_ptr()), "psg_text_cond_drop_f32")
    return out, dropped


def cfg_combine(eps_c: torch.Tensor, eps_u: torch.Tensor, w: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """psg_cfg_combine_f32: eps_u + w (eps_c - eps_u); fp32 contiguous operands; `out` may be eps_c."""
    lib = _lib_for(eps_c)
    if out is None:
        out = torch.empty_like(eps_c)
    for t in (eps_c, eps_u, out):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != eps_c.numel():
            raise ValueError("cfg_combine: operands must be contiguous fp32 of one size")
    check(lib.psg_cfg_combine_f32(ptr(eps_c), ptr(eps_u), float(w), ptr(out), eps_c.numel(), stream_ptr()), "psg_cfg_combine_f32")
    return out


def expand_null_text(null_text: torch.Tensor, text: torch.Tensor) -> torch.Tensor:
    """null_text [S, D] / [1, S, D] -> [n, S, D] like `text`."""
    null = null_text.detach().to(device=text.device, dtype=text.dtype)
    if null.dim() == text.dim() - 1:
        null = null.unsqueeze(0)
    if tuple(null.shape[1:]) != tuple(text.shape[1:]) or null.shape[0] not in (1, text.shape[0]):
        raise ValueError(f"null_text of shape {tuple(null_text.shape)} does not fit text of shape {tuple(text.shape)}")
    return null.expand(text.shape[0], *null.shape[1:])


def null_text_tokens(text_encoder, S: int, like=None):
    """(input_ids, attention_mask) int64 [1, S] of the empty description at token length S: [CLS] [SEP] [PAD]... with mask
    1, 1, 0, ...  The special ids are the tokenizer's; an encoder built without one takes them from `like` = (input_ids,
    attention_mask) of a tokenised batch: the first token of row 0 and its last attended one."""
    S = int(S)
    if S < 2:
        raise ValueError(f"null text: token length {S} has no room for [CLS] [SEP]")
    tok = getattr(text_encoder, "tokenizer", None)
    pad = int(getattr(text_encoder, "pad_token_id", 0))
    if tok is not None and getattr(tok, "cls_token_id", None) is not None:
        cls_id, sep_id = int(tok.cls_token_id), int(tok.sep_token_id)
        if getattr(tok, "pad_token_id", None) is not None:
            pad = int(tok.pad_token_id)
    elif like is not None:
        ids0, m0 = like[0][0].detach().cpu(), like[1][0].detach().cpu()
        cls_id, sep_id = int(ids0[0]), int(ids0[int(m0.sum()) - 1])
    else:
        raise _lib.PsgError("null text: the text encoder has no tokenizer; pass null_text, or token ids to take [CLS] / [SEP] from")
    ids = torch.full((1, S), pad, dtype=torch.int64)
    ids[0, 0], ids[0, 1] = cls_id, sep_id
    mask = torch.zeros((1, S), dtype=torch.int64)
    mask[0, :2] = 1
    return ids, mask


def encode_null_text(text_encoder, S: int, like=None) -> torch.Tensor:
    """[S, text_dim]: `encode_ids` of null_text_tokens; an injected encoder without encode_ids embeds [""] itself and must
    return S tokens."""
    with torch.no_grad():
        if hasattr(text_encoder, "encode_ids"):
            return text_encoder.encode_ids(*null_text_tokens(text_encoder, S, like))[0].detach().float()
        null = text_encoder([""])[0].detach().float()
    if null.shape[0] != S:
        raise _lib.PsgError(f"null text: the text encoder gave {null.shape[0]} tokens for the empty description, the batch has {S}")
    return null


def guided_eps(unet, xin, tv, text2, w, n, prediction=None, tables=None, t_dev=None):
    """The 2n forward and the combine, for the chains that keep their own update: xin [2n, ...] whose second half the caller
    keeps equal to the first; returns eps [n, ...] (a view of the forward's output, overwritten in place).  A v-predicting
    network (`prediction`) needs `tables` (a NoiseScheduler or the pair of sqrt tables) and `t_dev` (the timestep, int32 on the
    device): psg_pred_to_eps_f32 then stands where psg_cfg_combine_f32 stood."""
    out = unet(xin, tv, text2).detach().contiguous().float()
    if prediction_code(prediction) == PRED_EPS:
        return cfg_combine(out[:n], out[n:], w, out=out[:n])
    return pred_to_eps(xin[:n], out[:n], out[n:], w, tables, t_dev, prediction, out=out[:n])


# ------------------------------------------------------------------------------------------------------------- the chain
class DdimRun:
    """One DDIM chain, advanced step by step (`step()`, `remaining()`, `close()`; `x` is the latent [n, C, hw, hw]).

    use_graph=True (or PSG_GRAPH=1) captures the step body - the U-Net forward and `psg_guided_update_f32` - once and replays
    it, under SamplerRun's rules: step 0 runs eagerly (it sizes the workspace and fills the prepared-weight cache), eager step,
    capture and replays share ONE stream of ours, the workspace pool is frozen during the capture and the capture stream's
    buffer pinned afterwards, and a capture failure falls back to the eager loop with a warning.  The step index and the
    timestep live in device memory, so the captured work is the same for every step; with eta > 0 the last step (which draws
    no z) runs eagerly.  Bit-identical to the eager loop."""

    @torch.no_grad()
    def __init__(self, unet, text_emb, alphas_cumprod, num_steps=50, eta=0.0, guidance_scale=None, null_text=None, clip=3.0,
                 initial_latent=None, noise_fn=None, use_graph=None, latent_dim=8, hw=27, prediction=None):
        self.unet = unet
        self.prediction = prediction_code(prediction)
        unet.eval()
        dev = next(unet.parameters()).device
        self.dev = dev
        self.lib = _lib_for(torch.empty(0, device=dev))
        if clip < 0:
            raise ValueError(f"ddim_sample: clip={clip} < 0 (0 switches the clamp off)")
        self.guided = guidance_scale is not None
        if self.guided and null_text is None:
            raise ValueError("ddim_sample: guidance_scale needs null_text (the text the model was trained to see when the description is dropped)")
        self.w = float(guidance_scale) if self.guided else 0.0
        self.clip, self.eta = float(clip), float(eta)
        abar = torch.as_tensor(alphas_cumprod).detach().cpu().float()
        self.timesteps = ddim_timesteps(abar.numel(), num_steps)
        self.k = len(self.timesteps)
        self.tab = ddim_tables(abar, self.timesteps, eta).to(dev).contiguous()
        text = text_emb.to(dev)
        n = text.shape[0]
        self.n = n
        self.rnd = noise_fn if noise_fn is not None else (lambda i, shape: torch.randn(shape, device=dev))
        if initial_latent is None:
            x_T = self.rnd(-1, (n, latent_dim, hw, hw))
        else:
            x_T = initial_latent
        x_T = x_T.to(device=dev, dtype=torch.float32)
        if x_T.shape[0] != n:
            raise ValueError(f"ddim_sample: {x_T.shape[0]} latents for {n} texts")
        # guided: one input buffer [2n, ...]; x is its first half, the update writes the second half too
        self.xin = torch.empty((2 * n if self.guided else n,) + tuple(x_T.shape[1:]), dtype=torch.float32, device=dev)
        self.x = self.xin[:n]
        self.x.copy_(x_T)
        self.x_copy = None
        self.text = text
        if self.guided:
            self.x_copy = self.xin[n:]
            self.x_copy.copy_(x_T)
            self.text = torch.cat([text, expand_null_text(null_text, text)], dim=0).contiguous()
        self.tv = torch.zeros((self.xin.shape[0],), device=dev, dtype=torch.long)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.z = torch.zeros_like(self.x) if self.eta > 0 else None
        self.draws = 0
        if use_graph is None:
            use_graph = bool(os.environ.get("PSG_GRAPH"))
        self.use_graph = bool(use_graph) and self.k > 2
        self.graph = None
        self.i = 0
        self._stream = torch.cuda.Stream(device=dev) if self.use_graph else None
        self._ws_hold = None

    def close(self):
        """Drop the graph and the scratch buffer it pinned (also runs when the chain completes and on garbage collection)."""
        self.graph = None
        if self._ws_hold is not None:
            _lib.drop_workspace(self._ws_hold)
            self._ws_hold = None

    def __del__(self):
        try:
            self.close()
        except Exception:                            # noqa: BLE001 - interpreter shutdown
            pass

    def remaining(self):
        return self.k - self.i

    def _body(self, with_z):
        out = self.unet(self.xin, self.tv, self.text).contiguous()
        if out.dtype != torch.float32:
            out = out.float()
        n = self.n
        eps_c, eps_u = (out[:n], out[n:]) if self.guided else (out, None)
        if self.prediction == PRED_EPS:
            check(self.lib.psg_guided_update_f32(ptr(self.x), ptr(self.x_copy), ptr(eps_c), ptr(eps_u), ptr(self.z if with_z else None),
                                                 ptr(self.tab), self.k, ptr(self.step_dev), self.w, self.clip, self.x.numel(),
                                                 stream_ptr()), "psg_guided_update_f32")
        else:                                        # a v-predicting network: x0 = S0 x - S1 v, no division
            check(self.lib.psg_guided_update_pred_f32(ptr(self.x), ptr(self.x_copy), ptr(eps_c), ptr(eps_u), ptr(self.z if with_z else None),
                                                      ptr(self.tab), self.k, ptr(self.step_dev), self.w, self.clip, self.x.numel(),
                                                      self.prediction, stream_ptr()), "psg_guided_update_pred_f32")

    @torch.no_grad()
    def step(self):
        if self.i >= self.k:
            raise StopIteration("sampler chain is complete")
        self.unet.eval()
        self.tv.fill_(int(self.timesteps[self.i]))
        self.step_dev.fill_(self.i)
        with_z = self.z is not None and self.i < self.k - 1
        if with_z:
            self.z.copy_(self.rnd(self.draws, tuple(self.x.shape)).to(device=self.dev, dtype=torch.float32))
            self.draws += 1
        if self._stream is None:
            self._body(with_z)
        else:
            cur = torch.cuda.current_stream(self.dev)
            self._stream.wait_stream(cur)
            with torch.cuda.stream(self._stream):
                self._graph_step(with_z)
            cur.wait_stream(self._stream)
        self.i += 1
        if self.i >= self.k:
            self.close()
        return self.x

    def _graph_step(self, with_z):
        # the captured body is the one of the middle steps: z present exactly when eta > 0
        replayable = with_z == (self.z is not None)
        if self.use_graph and self.i >= 1 and self.graph is None and replayable:
            try:
                torch.cuda.synchronize(self.dev)
                graph = torch.cuda.CUDAGraph()
                xin_before = self.xin.clone()
                _lib.freeze_workspaces(True)
                try:
                    with torch.cuda.graph(graph, stream=self._stream):
                        self._body(with_z)
                finally:
                    _lib.freeze_workspaces(False)
                self.xin.copy_(xin_before)              # capture does not execute: the replay below runs this step
                self.graph = graph
                self._ws_hold = _lib.hold_workspace(self.dev)
            except Exception as e:                      # noqa: BLE001
                logging.getLogger(__name__).warning(f"hipGraph capture of the DDIM step failed ({e!r}); running eagerly")
                self.use_graph = False
        if self.graph is not None and replayable:
            self.graph.replay()
        else:
            self._body(with_z)


@torch.no_grad()
def ddim_sample(unet, text_emb, alphas_cumprod, num_steps=50, eta=0.0, guidance_scale=None, null_text=None, clip=3.0,
                initial_latent=None, noise_fn=None, trace=None, use_graph=None, latent_dim=8, hw=27, prediction=None) -> torch.Tensor:
    """DDIM chain of `num_steps` U-Net forwards over `alphas_cumprod` (any schedule), optionally guided.

    unet: any module with parameters on the device, called as unet(x, t, text) -> eps.  text_emb [n, S, text_dim].
    prediction: what the network returns - "epsilon" (default) or "v_prediction" (objective.py): guidance then combines the
      two v, and the step takes x0 = S0 x - S1 v, eps = S1 x + S0 v before the same clamp and update.
    eta: 0 the deterministic chain, 1 the posterior-variance noise of DDPM on consecutive timesteps.
    guidance_scale: None runs at batch n; a float w runs one forward at batch 2n with [text; null_text] and steps with
      eps_u + w (eps_c - eps_u); it needs null_text ([S, text_dim]).
    clip: the trainer's latent clamp (3.0) on the predicted x0, eps recomputed where it clamps; 0 switches it off.
    noise_fn(i, shape): i = -1 is x_T (unless initial_latent is given), i >= 0 the i-th z; z is drawn only when eta > 0
      and not on the last step.  trace: a list that receives a copy of the latent after every step."""
    run = DdimRun(unet, text_emb, alphas_cumprod, num_steps, eta, guidance_scale, null_text, clip, initial_latent, noise_fn,
                  use_graph, latent_dim, hw, prediction)
    while run.remaining():
        run.step()
        if trace is not None:
            trace.append(run.x.clone())
    return run.x.clone() if run.guided else run.x
