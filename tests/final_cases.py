"""Cases of the stage-3 fixture (tests/golden/final_grad.npz, made by tools/make_golden_final.py from the reference
VAEDecoder's own forward + backward): decoder weights, latents, text embeddings and images - all rebuilt here from
oracle.hashgen - the reconstruction loss of final_trainer.py:425-440, and a CPU restatement of the BERT text encoder for the
end-to-end check (pinned to the reference's fixture by tests/test_final_cpu.py)."""
import math

import torch
import torch.nn.functional as F

from oracle import hashgen

SEED_W, SEED_IN = 12, 1212
CASES = {"b2": (2, 32), "s20": (1, 20)}          # name -> (batch, text tokens)


def decoder_state(shapes):
    """'stress' weights for a VAEDecoder state dict given as {key: shape}."""
    return hashgen.fill_unet_state({k: tuple(s) for k, s in shapes.items()}, SEED_W, "stress")


def inputs(case):
    """(latent [B,8,27,27], text [B,S,256], images [B,3,215,215] uniform in [-1, 1))."""
    B, S = CASES[case]
    lat = hashgen.uniform((B, 8, 27, 27), SEED_IN, hashgen.name_id(f"final.{case}.lat")) * math.sqrt(3.0)
    text = hashgen.uniform((B, S, 256), SEED_IN, hashgen.name_id(f"final.{case}.text")) * math.sqrt(3.0)
    img = hashgen.uniform((B, 3, 215, 215), SEED_IN, hashgen.name_id(f"final.{case}.img"))
    return lat, text, img


def recon_loss(recon, img):
    """compute_generation_loss: (l1 + 0.1 * mse, l1, mse)."""
    l1, mse = F.l1_loss(recon, img), F.mse_loss(recon, img)
    return l1 + 0.1 * mse, l1, mse


def bert_encode(sd, cfg, ids, mask, tt, hidden_dim):
    """transformers' BertModel (eval) + TextEncoder's projection and LayerNorm (src/models/text_encoder.py forward) as plain
    torch functional ops on a state dict: [B,S] ids -> [B,S,hidden_dim]."""
    H, heads, eps = cfg["hidden_size"], cfg["num_attention_heads"], cfg["layer_norm_eps"]
    B, S = ids.shape
    d = H // heads
    e = "bert.embeddings."
    x = sd[e + "word_embeddings.weight"][ids] + sd[e + "position_embeddings.weight"][:S][None] + sd[e + "token_type_embeddings.weight"][tt]
    x = F.layer_norm(x, (H,), sd[e + "LayerNorm.weight"], sd[e + "LayerNorm.bias"], eps)
    bias = (1.0 - mask[:, None, None, :].to(x.dtype)) * torch.finfo(x.dtype).min
    for i in range(cfg["num_hidden_layers"]):
        p = f"bert.encoder.layer.{i}."
        lin = lambda t, n: F.linear(t, sd[p + n + ".weight"], sd[p + n + ".bias"])
        split = lambda t: t.view(B, S, heads, d).transpose(1, 2)
        q, k, v = split(lin(x, "attention.self.query")), split(lin(x, "attention.self.key")), split(lin(x, "attention.self.value"))
        pr = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d) + bias, dim=-1)
        ctx = (pr @ v).transpose(1, 2).reshape(B, S, H)
        h = F.layer_norm(lin(ctx, "attention.output.dense") + x, (H,), sd[p + "attention.output.LayerNorm.weight"],
                         sd[p + "attention.output.LayerNorm.bias"], eps)
        u = F.gelu(lin(h, "intermediate.dense"))
        x = F.layer_norm(lin(u, "output.dense") + h, (H,), sd[p + "output.LayerNorm.weight"], sd[p + "output.LayerNorm.bias"], eps)
    if "projection.weight" in sd:
        x = F.linear(x, sd["projection.weight"], sd["projection.bias"])
    return F.layer_norm(x, (hidden_dim,), sd["layer_norm.weight"], sd["layer_norm.bias"], 1e-5)
