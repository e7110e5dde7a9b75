"""Drop-in ``model`` module: ``from model import MatchaTTS`` (main.py:8) on MI355X.

Call surface and state_dict keys are those of the reference ``model.py``
(Lounes78/matcha-tts): ``MatchaTTS(n_vocab, n_spks, spk_emb_dim, encoder_params,
decoder_params, cfm_params, duration_predictor_params)``, ``.synthesize(...) ->
(mel, y_lengths, attn)`` (model.py:1264-1300), plus the upstream-style
``synthesise(...) -> dict`` used by the notebooks.

Everything on the synthesis path runs as hand-written HIP kernels behind the C ABI
(include/matcha_hip.h, ``matcha_hip.runtime``):
  * text encoder + duration predictor (model.py:148-535): ``TextEncoder.forward`` is one
    ``mt_encoder_forward`` call;
  * duration -> alignment index path, CFM Euler/midpoint solver over the U-Net estimator,
    denormalize/crop: ``mt_durations``, ``mt_alignment``, ``mt_cfm_solve``, ``mt_denorm_crop``.
The submodules below only hold parameters under the reference names and shapes (so reference
checkpoints load unchanged); calling one of them directly raises. There is no CPU fallback.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from matcha_hip import runtime as rt


# ======================================================================================
# utilities (model.py:42-125)
# ======================================================================================

def sequence_mask(length: torch.Tensor, max_length: Optional[int] = None) -> torch.Tensor:
    if max_length is None:
        max_length = int(length.max())
    ar = torch.arange(int(max_length), dtype=length.dtype, device=length.device)
    return ar[None, :] < length[:, None]


def fix_len_compatibility(length, num_downsamplings_in_unet: int = 2) -> int:
    """Round up to a multiple of 2**n (host int; model.py:49-55 ends in .item())."""
    f = 2 ** num_downsamplings_in_unet
    return int(math.ceil(int(length) / f) * f)


def denormalize(data, mu, std):
    mu = torch.as_tensor(mu, dtype=data.dtype, device=data.device)
    std = torch.as_tensor(std, dtype=data.dtype, device=data.device)
    return data * std.reshape(-1, 1) + mu.reshape(-1, 1)


def normalize(data, mu, std):
    mu = torch.as_tensor(mu, dtype=data.dtype, device=data.device)
    std = torch.as_tensor(std, dtype=data.dtype, device=data.device)
    return (data - mu.reshape(-1, 1)) / std.reshape(-1, 1)


def _get(p, k, default=None):
    if isinstance(p, dict):
        return p.get(k, default)
    return getattr(p, k, default)


# ======================================================================================
# text encoder parameter containers (state_dict keys of model.py:148-535); TextEncoder.forward is mt_encoder
# ======================================================================================

class _Params(nn.Module):
    """Parameter container of a reference submodule; its arithmetic is a HIP kernel of the owning module."""

    def forward(self, *a, **k):
        raise RuntimeError(f"{type(self).__name__} is evaluated by the HIP path of its owning module "
                           "(TextEncoder.forward / Decoder.forward); it has no forward of its own")


class LayerNorm(_Params):
    """Channel LayerNorm over dim 1 of [B,C,T] (model.py:148-166): gamma, beta."""

    def __init__(self, channels: int, eps: float = 1e-4):
        super().__init__()
        self.channels, self.eps = channels, eps
        self.gamma = nn.Parameter(torch.ones(channels))
        self.beta = nn.Parameter(torch.zeros(channels))


class ConvReluNorm(_Params):
    """Prenet (model.py:171-208): n x (conv(x*mask) -> LayerNorm -> ReLU), zero-init 1x1 proj, residual."""

    def __init__(self, in_channels, hidden_channels, out_channels, kernel_size, n_layers, p_dropout):
        super().__init__()
        self.n_layers = n_layers
        self.conv_layers = nn.ModuleList(
            [nn.Conv1d(in_channels if i == 0 else hidden_channels, hidden_channels, kernel_size,
                       padding=kernel_size // 2) for i in range(n_layers)])
        self.norm_layers = nn.ModuleList([LayerNorm(hidden_channels) for _ in range(n_layers)])
        self.relu_drop = nn.Sequential(nn.ReLU(), nn.Dropout(p_dropout))
        self.proj = nn.Conv1d(hidden_channels, out_channels, 1)
        nn.init.zeros_(self.proj.weight)
        nn.init.zeros_(self.proj.bias)


class DurationPredictor(_Params):
    """model.py:210-235: conv -> relu -> LayerNorm (x2) -> 1x1 -> log-durations."""

    def __init__(self, in_channels, filter_channels, kernel_size, p_dropout):
        super().__init__()
        self.drop = nn.Dropout(p_dropout)
        self.conv_1 = nn.Conv1d(in_channels, filter_channels, kernel_size, padding=kernel_size // 2)
        self.norm_1 = LayerNorm(filter_channels)
        self.conv_2 = nn.Conv1d(filter_channels, filter_channels, kernel_size, padding=kernel_size // 2)
        self.norm_2 = LayerNorm(filter_channels)
        self.proj = nn.Conv1d(filter_channels, 1, 1)


class RotaryPositionalEmebeddings(_Params):
    """RoPE on the first d features (model.py:244-292; name kept for compatibility). No parameters: the
    HIP encoder applies it (rope_kernel) with the theta table of runtime.rope_theta."""

    def __init__(self, d, base: int = 10_000):
        super().__init__()
        self.d, self.base = int(d), base


class MultiHeadAttention(_Params):
    """RoPE multi-head attention with 1x1-conv projections (model.py:294-372)."""

    def __init__(self, channels, out_channels, n_heads, heads_share=True, p_dropout=0.0,
                 proximal_bias=False, proximal_init=False):
        super().__init__()
        assert channels % n_heads == 0, "channels must be divisible by n_heads"
        if proximal_bias:
            raise NotImplementedError("proximal_bias is not used by the reference encoder (model.py:437)")
        self.channels, self.n_heads = channels, n_heads
        self.k_channels = channels // n_heads
        self.conv_q = nn.Conv1d(channels, channels, 1)
        self.conv_k = nn.Conv1d(channels, channels, 1)
        self.conv_v = nn.Conv1d(channels, channels, 1)
        self.query_rotary_pe = RotaryPositionalEmebeddings(self.k_channels * 0.5)
        self.key_rotary_pe = RotaryPositionalEmebeddings(self.k_channels * 0.5)
        self.conv_o = nn.Conv1d(channels, out_channels, 1)
        self.drop = nn.Dropout(p_dropout)
        nn.init.xavier_uniform_(self.conv_q.weight)
        nn.init.xavier_uniform_(self.conv_k.weight)
        if proximal_init:
            with torch.no_grad():
                self.conv_k.weight.copy_(self.conv_q.weight)
                self.conv_k.bias.copy_(self.conv_q.bias)
        nn.init.xavier_uniform_(self.conv_v.weight)


class FFN(_Params):
    """model.py:375-393: conv(x*mask) -> ReLU -> conv(.*mask) * mask."""

    def __init__(self, in_channels, out_channels, filter_channels, kernel_size, p_dropout=0.0):
        super().__init__()
        self.conv_1 = nn.Conv1d(in_channels, filter_channels, kernel_size, padding=kernel_size // 2)
        self.conv_2 = nn.Conv1d(filter_channels, out_channels, kernel_size, padding=kernel_size // 2)
        self.drop = nn.Dropout(p_dropout)


class Encoder(_Params):
    """model.py:396-444: n_layers x (x + MHA -> LayerNorm, x + FFN -> LayerNorm)."""

    def __init__(self, hidden_channels, filter_channels, n_heads, n_layers, kernel_size=1, p_dropout=0.0):
        super().__init__()
        self.n_layers = n_layers
        self.drop = nn.Dropout(p_dropout)
        self.attn_layers = nn.ModuleList(
            [MultiHeadAttention(hidden_channels, hidden_channels, n_heads, p_dropout=p_dropout)
             for _ in range(n_layers)])
        self.norm_layers_1 = nn.ModuleList([LayerNorm(hidden_channels) for _ in range(n_layers)])
        self.ffn_layers = nn.ModuleList(
            [FFN(hidden_channels, hidden_channels, filter_channels, kernel_size, p_dropout=p_dropout)
             for _ in range(n_layers)])
        self.norm_layers_2 = nn.ModuleList([LayerNorm(hidden_channels) for _ in range(n_layers)])


class TextEncoder(nn.Module):
    """model.py:452-535 -> (mu [B,n_feats,Tx], logw [B,1,Tx], x_mask [B,1,Tx])."""

    def __init__(self, encoder_type, encoder_params, duration_predictor_params, n_vocab, n_spks=1,
                 spk_emb_dim=128, precision: str = "fp32"):
        super().__init__()
        self.precision = precision
        self._engines = {}
        self._pk = rt.PackCache()
        self.encoder_type = encoder_type
        self.n_vocab = n_vocab
        self.n_feats = _get(encoder_params, "n_feats")
        self.n_channels = _get(encoder_params, "n_channels")
        self.spk_emb_dim, self.n_spks = spk_emb_dim, n_spks
        self.emb = nn.Embedding(n_vocab, self.n_channels)
        nn.init.normal_(self.emb.weight, 0.0, self.n_channels ** -0.5)
        if _get(encoder_params, "prenet"):
            self.prenet = ConvReluNorm(self.n_channels, self.n_channels, self.n_channels, kernel_size=5,
                                       n_layers=3, p_dropout=0.5)
        else:
            self.prenet = None  # no prenet parameters (the HIP encoder skips the stage)
        width = self.n_channels + (spk_emb_dim if n_spks > 1 else 0)
        self.encoder = Encoder(width, _get(encoder_params, "filter_channels"), _get(encoder_params, "n_heads"),
                               _get(encoder_params, "n_layers"), _get(encoder_params, "kernel_size"),
                               _get(encoder_params, "p_dropout"))
        self.proj_m = nn.Conv1d(width, self.n_feats, 1)
        self.proj_w = DurationPredictor(width, _get(duration_predictor_params, "filter_channels_dp"),
                                        _get(duration_predictor_params, "kernel_size"),
                                        _get(duration_predictor_params, "p_dropout"))

    # ---- HIP plumbing (mt_encoder: the whole forward below is one C-ABI call) ----
    def set_precision(self, precision: str):
        rt.dtype_code(precision)
        self.precision = precision
        return self

    def engine(self) -> rt.EncoderEngine:
        if self.precision not in self._engines:
            enc = self.encoder
            self._engines[self.precision] = rt.EncoderEngine(
                self.n_vocab, self.n_channels, enc.ffn_layers[0].conv_1.out_channels, enc.attn_layers[0].n_heads,
                enc.n_layers, enc.ffn_layers[0].conv_1.kernel_size[0], self.n_spks, self.spk_emb_dim,
                self.proj_w.conv_1.out_channels, self.proj_w.conv_1.kernel_size[0], self.prenet is not None,
                self.precision)
        return self._engines[self.precision]

    def forward(self, x, x_lengths, spks=None):
        """model.py:503-535 on the GPU -> (mu [B,80,Tx], logw [B,1,Tx], x_mask [B,1,Tx]) fp32. An id outside
        [0, n_vocab) raises IndexError, as ``self.emb(x)`` does (model.py:522)."""
        mu, logw, x_mask, oov = self.forward_unchecked(x, x_lengths, spks)
        rt.check_ids(oov)
        return mu, logw, x_mask

    def forward_unchecked(self, x, x_lengths, spks=None):
        """forward without the host sync of the id check: also returns the device flag for ``rt.check_ids``"""
        rt.require_gpu(x, x_lengths, spks, what="TextEncoder.forward")
        if self.n_spks > 1 and spks is None:
            raise ValueError("multi-speaker TextEncoder needs spks [B, spk_emb_dim]")
        eng = self.engine()
        key = (self.precision, str(x.device))
        packed = self._pk.get(key)
        if packed is None:
            sd = self.state_dict(keep_vars=True)
            packed = self._pk.put(key, list(sd.values()), eng.pack(dict(sd), x.device))
        return eng.forward(packed, x, x_lengths, rt.f32c(spks))


# ======================================================================================
# U-Net estimator parameter containers (state_dict keys of model.py:576-962).
# Their arithmetic is the HIP estimator; they have no torch forward of their own.
# ======================================================================================

class LoRACompatibleLinear(nn.Linear):
    pass


class SnakeBeta(_Params):
    def __init__(self, in_features, out_features, alpha=1.0, alpha_trainable=True, alpha_logscale=True):
        super().__init__()
        n = out_features if isinstance(out_features, int) else out_features[0]
        self.proj = nn.Linear(in_features, n)
        self.alpha_logscale = alpha_logscale
        init = torch.zeros(n) if alpha_logscale else torch.ones(n) * alpha
        self.alpha = nn.Parameter(init.clone(), requires_grad=alpha_trainable)
        self.beta = nn.Parameter(init.clone(), requires_grad=alpha_trainable)
        self.no_div_by_zero = 1e-9


class FeedForward(_Params):
    def __init__(self, dim, dim_out=None, mult=4, dropout=0.0, activation_fn="snakebeta", final_dropout=False):
        super().__init__()
        if activation_fn != "snakebeta":
            raise NotImplementedError("the HIP estimator implements the SnakeBeta feed-forward (main.py:74)")
        inner = int(dim * mult)
        self.net = nn.ModuleList([SnakeBeta(dim, inner), nn.Dropout(dropout), nn.Linear(inner, dim_out or dim)])
        if final_dropout:
            self.net.append(nn.Dropout(dropout))


class Attention(_Params):
    def __init__(self, query_dim, heads=8, dim_head=64, dropout=0.0, bias=False, cross_attention_dim=None,
                 upcast_attention=False):
        super().__init__()
        if cross_attention_dim is not None:
            raise NotImplementedError("the reference decoder uses self-attention only (model.py:721-736)")
        if dim_head != 64:
            raise NotImplementedError("the HIP attention kernel is built for head dim 64")
        inner = heads * dim_head
        self.heads, self.scale = heads, dim_head ** -0.5
        self.to_q = nn.Linear(query_dim, inner, bias=bias)
        self.to_k = nn.Linear(query_dim, inner, bias=bias)
        self.to_v = nn.Linear(query_dim, inner, bias=bias)
        self.to_out = nn.ModuleList([nn.Linear(inner, query_dim), nn.Dropout(dropout)])


class BasicTransformerBlock(_Params):
    def __init__(self, dim, num_attention_heads, attention_head_dim, dropout=0.0, activation_fn="snakebeta",
                 attention_bias=False):
        super().__init__()
        if attention_bias:
            raise NotImplementedError("attention_bias=True is not used by the reference decoder")
        self.norm1 = nn.LayerNorm(dim)
        self.attn1 = Attention(dim, num_attention_heads, attention_head_dim, dropout, attention_bias)
        self.norm3 = nn.LayerNorm(dim)
        self.ff = FeedForward(dim, dropout=dropout, activation_fn=activation_fn)


class SinusoidalPosEmb(nn.Module):
    def __init__(self, dim):
        super().__init__()
        assert dim % 2 == 0, "SinusoidalPosEmb requires dim to be even"
        self.dim = dim

    def forward(self, x, scale=1000):   # host helper (model.py:753-762); the HIP path has its own
        x = x.reshape(-1)
        emb = scale * x.unsqueeze(1) * rt.sinus_freq(self.dim).to(x.device).unsqueeze(0)
        return torch.cat((emb.sin(), emb.cos()), dim=-1)


class Block1D(_Params):
    def __init__(self, dim, dim_out, groups=8):
        super().__init__()
        self.block = nn.Sequential(nn.Conv1d(dim, dim_out, 3, padding=1), nn.GroupNorm(groups, dim_out), nn.Mish())


class ResnetBlock1D(_Params):
    def __init__(self, dim, dim_out, time_emb_dim, groups=8):
        super().__init__()
        self.mlp = nn.Sequential(nn.Mish(), nn.Linear(time_emb_dim, dim_out))
        self.block1 = Block1D(dim, dim_out, groups=groups)
        self.block2 = Block1D(dim_out, dim_out, groups=groups)
        self.res_conv = nn.Conv1d(dim, dim_out, 1)


class Downsample1D(_Params):
    def __init__(self, dim):
        super().__init__()
        self.conv = nn.Conv1d(dim, dim, 3, 2, 1)


class Upsample1D(_Params):
    def __init__(self, channels, use_conv_transpose=True, out_channels=None):
        super().__init__()
        if not use_conv_transpose:
            raise NotImplementedError("the reference decoder uses the ConvTranspose1d upsampler")
        self.conv = nn.ConvTranspose1d(channels, out_channels or channels, 4, 2, 1)


class TimestepEmbedding(_Params):
    def __init__(self, in_channels, time_embed_dim, act_fn="silu", out_dim=None):
        super().__init__()
        self.linear_1 = nn.Linear(in_channels, time_embed_dim)
        self.act = nn.SiLU() if act_fn == "silu" else nn.Mish()
        self.linear_2 = nn.Linear(time_embed_dim, out_dim or time_embed_dim)


class Decoder(nn.Module):
    """U-Net velocity estimator (model.py:834-1048). ``forward`` = one HIP estimator evaluation."""

    def __init__(self, in_channels, out_channels, channels=(256, 256), dropout=0.05, attention_head_dim=64,
                 n_blocks=1, num_mid_blocks=2, num_heads=4, time_emb_dim=None, time_mlp_dim=None, ffn_mult=4,
                 precision: str = "fp32", **kwargs):
        super().__init__()
        channels = tuple(channels)
        if channels != (256, 256) or out_channels != 80:
            raise NotImplementedError("the HIP estimator is built for channels=(256,256), n_feats=80 (main.py:68)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.n_blocks, self.num_mid_blocks, self.num_heads = n_blocks, num_mid_blocks, num_heads
        self.time_embeddings = SinusoidalPosEmb(in_channels)
        tdim = channels[0] * 4
        self.time_mlp = TimestepEmbedding(in_channels, tdim, act_fn="silu")

        def tblocks(dim):
            return nn.ModuleList([BasicTransformerBlock(dim, num_heads, attention_head_dim, dropout, "snakebeta")
                                  for _ in range(n_blocks)])

        self.down_blocks = nn.ModuleList([
            nn.ModuleList([ResnetBlock1D(in_channels, 256, tdim), tblocks(256), Downsample1D(256)]),
            nn.ModuleList([ResnetBlock1D(256, 256, tdim), tblocks(256), nn.Conv1d(256, 256, 3, padding=1)]),
        ])
        self.mid_blocks = nn.ModuleList([nn.ModuleList([ResnetBlock1D(256, 256, tdim), tblocks(256)])
                                         for _ in range(num_mid_blocks)])
        self.up_blocks = nn.ModuleList([
            nn.ModuleList([ResnetBlock1D(512, 256, tdim), tblocks(256), Upsample1D(256, use_conv_transpose=True)]),
            nn.ModuleList([ResnetBlock1D(512, 256, tdim), tblocks(256), nn.Conv1d(256, 256, 3, padding=1)]),
        ])
        self.final_block = Block1D(256, 256)
        self.final_proj = nn.Conv1d(256, out_channels, 1)
        self.precision = precision
        self._engines = {}
        self._pk = rt.PackCache()

    # ---- HIP plumbing ----
    def set_precision(self, precision: str):
        rt.dtype_code(precision)
        self.precision = precision
        return self

    def engine(self) -> rt.DecoderEngine:
        key = self.precision
        if key not in self._engines:
            self._engines[key] = rt.DecoderEngine(self.in_channels, self.num_mid_blocks, self.n_blocks,
                                                  self.num_heads, self.precision)
        return self._engines[key]

    def packed(self, device):
        key = (self.precision, str(device))
        packed = self._pk.get(key)
        if packed is None:
            sd = self.state_dict(keep_vars=True)
            packed = self._pk.put(key, list(sd.values()), self.engine().pack(dict(sd), device))
        return packed

    def forward(self, x, mask, mu, t, spks=None, cond=None):
        """model.py:964-1048 — x, mu [B,80,T], mask [B,1,T], t [B] (or scalar) -> [B,80,T]."""
        rt.require_gpu(x, mask, mu, spks, what="Decoder.forward")
        x, mu, mask, spks = rt.f32c(x), rt.f32c(mu), rt.f32c(mask), rt.f32c(spks)
        t = torch.as_tensor(t, dtype=torch.float32).reshape(-1)
        eng, packed = self.engine(), self.packed(x.device)
        if t.numel() == 1:
            return eng.step(packed, x, mu, mask, spks, float(t[0]))
        # one time per utterance (CFM.compute_loss): one batched call, the times stay on the device
        return eng.step_times(packed, x, mu, mask, spks, t.to(x.device))


# ======================================================================================
# Conditional flow matching (model.py:1063-1162)
# ======================================================================================

class BASECFM(nn.Module):
    def __init__(self, n_feats, cfm_params, n_spks=1, spk_emb_dim=64):
        super().__init__()
        self.n_feats, self.n_spks, self.spk_emb_dim = n_feats, n_spks, spk_emb_dim
        self.solver = _get(cfm_params, "solver", "euler")
        self.sigma_min = _get(cfm_params, "sigma_min", 1e-4)
        self.estimator = None

    @torch.inference_mode()
    def forward(self, mu, mask, n_timesteps, temperature=1.0, spks=None, cond=None, max_valid=None, seeds=None,
                t_span=None, x1=None, keep=None):
        """z = randn_like(mu)*temperature, then the Euler/midpoint loop — one HIP call. max_valid (extension, not
        in the reference signature): the most valid frames of any utterance when the caller knows it (synthesize's
        y_max); it lets the solver prove every utterance padded and use the query-independent attention.
        temperature (extension): a number, or one value per utterance ([B] tensor or sequence). seeds (extension):
        int64 [B] tensor or B ints; utterance b then starts from the seeded stream of seeds[b] (rt.seeded_noise),
        which depends on neither the batch nor the padded length, drawn inside the solve. n_timesteps (extension):
        also one count per utterance ([B] ints); t_span (extension): a time grid of n + 1 times in [0, 1] shared by
        the batch, or one per utterance (rt.step_plan; rt.cosine_grid), instead of the reference's i / n.
        x1, keep (extension, mel infill): x1 a normalized mel [B,80,T] and keep [B,T] (or [B,1,T]), non-zero = kept;
        the kept valid frames follow compute_loss's y_t = (1 - (1 - sigma_min) t) z + t x1 with the utterance's own
        noise z and come back as x1, the others are integrated as usual and see them through the estimator."""
        rt.infill_args(x1, keep, mu.shape[0], mu.shape[1], mu.shape[2], self.sigma_min)
        rt.require_gpu(mu, mask, spks, what="CFM.forward")
        mu, mask, spks = rt.f32c(mu), rt.f32c(mask), rt.f32c(spks)
        est = self.estimator
        kw = dict(max_valid=int(max_valid or 0), t_span=t_span)
        if x1 is not None:
            kw.update(x1=x1, keep=keep, sigma_min=self.sigma_min)
        if seeds is not None:
            return est.engine().solve(est.packed(mu.device), None, temperature, mu, mask, spks, n_timesteps,
                                      self.solver, seeds=seeds, **kw)
        if not rt.is_scalar(temperature):
            # unseeded, one temperature per utterance: the same draw, scaled per row here
            z = torch.randn_like(mu) * rt.per_row(temperature, mu.shape[0], mu.device, "temperature")[:, None, None]
            return est.engine().solve(est.packed(mu.device), z, 1.0, mu, mask, spks, n_timesteps, self.solver,
                                      out=z, **kw)
        z = torch.randn_like(mu)
        # out=z: a per-utterance solve gathers its rows first and scatters the result into z afterwards
        return est.engine().solve(est.packed(mu.device), z, temperature, mu, mask, spks, n_timesteps,
                                  self.solver, out=z, **kw)

    def compute_loss(self, x1, mask, mu, spks=None, cond=None):
        """model.py:1147-1162 -> (loss, y_t, pred, u_t): t ~ U(0,1) and z ~ N(0,1) per utterance on the
        device, one batched estimator evaluation with a time per utterance (mt_decoder_step_times).
        Forward only (bf16 / fp32 inference estimator, no autograd graph): the training step with its
        hand-written backward is matcha_hip.train.MatchaTrainer (train_standalone.MatchaLightningModule)."""
        b = mu.shape[0]
        t = torch.rand([b, 1, 1], device=mu.device, dtype=mu.dtype)
        z = torch.randn_like(x1)
        y_t = (1 - (1 - self.sigma_min) * t) * z + t * x1
        u_t = x1 - (1 - self.sigma_min) * z
        pred = self.estimator(y_t, mask, mu, t.squeeze(), spks, cond)
        loss = F.mse_loss(pred, u_t, reduction="sum") / (torch.sum(mask) * u_t.shape[1])
        return loss, y_t, pred, u_t


class CFM(BASECFM):
    def __init__(self, n_feats, cfm_params, n_spks=1, spk_emb_dim=64, estimator=None):
        super().__init__(n_feats, cfm_params, n_spks=n_spks, spk_emb_dim=spk_emb_dim)
        if estimator is None:
            raise ValueError("estimator must be provided")
        self.estimator = estimator


# ======================================================================================
# MatchaTTS (model.py:1173-1300)
# ======================================================================================

class MatchaTTS(nn.Module):
    """``precision`` sets the CFM estimator ("fp32" parity mode, "bf16" performance mode). The text encoder and
    duration predictor run in ``encoder_precision``, fp32 by default in BOTH modes: ``ceil(exp(logw))``
    (model.py:1273-1275) flips on a 1-ulp change of logw, so the index path is only bit-exact when logw is the
    reference's fp32 arithmetic; the encoder is < 1 % of the FLOPs."""

    def __init__(self, n_vocab, n_spks, spk_emb_dim, encoder_params, decoder_params, cfm_params,
                 duration_predictor_params, precision: str = "fp32", encoder_precision: str = "fp32"):
        super().__init__()
        self.n_vocab, self.n_spks, self.spk_emb_dim = n_vocab, n_spks, spk_emb_dim
        if n_spks > 1:
            self.spk_emb = nn.Embedding(n_spks, spk_emb_dim)
        self.register_buffer("mel_mean", torch.tensor(0.0))
        self.register_buffer("mel_std", torch.tensor(1.0))
        self.encoder = TextEncoder(_get(encoder_params, "encoder_type"), encoder_params, duration_predictor_params,
                                   n_vocab, n_spks, spk_emb_dim, precision=encoder_precision)
        n_feats = _get(encoder_params, "n_feats")
        dec_in = 2 * n_feats + (spk_emb_dim if n_spks > 1 else 0)
        est = Decoder(in_channels=dec_in, out_channels=n_feats, channels=_get(decoder_params, "channels"),
                      dropout=_get(decoder_params, "dropout"),
                      attention_head_dim=_get(decoder_params, "attention_head_dim"),
                      n_blocks=_get(decoder_params, "n_blocks"), num_mid_blocks=_get(decoder_params, "num_mid_blocks"),
                      num_heads=_get(decoder_params, "num_heads"), act_fn=_get(decoder_params, "act_fn"),
                      precision=precision)
        self.decoder = CFM(n_feats=n_feats, cfm_params=cfm_params, n_spks=n_spks, spk_emb_dim=spk_emb_dim,
                           estimator=est)

    def set_precision(self, precision: str, encoder_precision: str = "fp32"):
        """Estimator: 'fp32' (parity mode, default) or 'bf16' (bf16 MFMA, fp32 accumulate). The text encoder keeps
        fp32 unless ``encoder_precision`` says otherwise (see the class docstring)."""
        self.decoder.estimator.set_precision(precision)
        self.encoder.set_precision(encoder_precision)
        return self

    def forward(self, x, x_lengths, y, y_lengths, spks=None):
        # The reference's MatchaTTS.forward (model.py:1234-1262) is a placeholder: it feeds text-length mu and the
        # text mask to CFM.compute_loss against mel-length y (model.py:1254-1260). The reference trains through
        # MatchaLightningModule.forward (train_standalone.py:623-667) instead, whose drop-in runs on the GPU.
        raise NotImplementedError("train through train_standalone.MatchaLightningModule (the reference's training "
                                  "path, train_standalone.py:580-707); MatchaTTS.forward is a placeholder upstream")

    @torch.inference_mode()
    def synthesize(self, x, x_lengths, n_timesteps, temperature=1.0, spks=None, length_scale=1.0, seeds=None,
                   t_span=None, token_scale=None, durations=None, infill_mel=None, infill_keep=None):
        """model.py:1264-1300 -> (mel [B,80,y_max], y_lengths int64 [B], attn [B,1,Tx,T_pad]).
        Extensions for mixed batches: temperature and length_scale each take a number or one value per utterance
        ([B] tensor or sequence); seeds (int64 [B] tensor or B ints) gives utterance b the noise of seeds[b], the
        same whatever its position, the batch, the padded length or the device (rt.seeded_noise; None: randn_like).
        n_timesteps takes an int or one step count per utterance, and t_span a time grid in [0, 1] shared by the
        batch or one per utterance (n_timesteps may then be None): an utterance costs only its own steps.
        Duration control: token_scale (fp32 [B,Tx] or B lists) multiplies each token's predicted length before the
        ceil; durations (integer [B,Tx] frames per token, zeros allowed) replaces the predictor, e.g. an edited
        predict_durations() or the timing align() took from a recording. durations excludes a length_scale other
        than 1 and token_scale; a negative count raises ValueError.
        Mel infill: infill_mel ([B,80,Tk], denormalized, what synthesize returns) with infill_keep ([B,Tk], non-zero =
        kept) pins those frames: they come back as given (to the rounding of normalize / denormalize) while the
        solve fills the others around them. Frames at or past Tk are free, frames at or past y_lengths[b] ignored."""
        B, Tx = x.shape[0], x.shape[1]
        token_scale, durations = rt.duration_args(B, Tx, length_scale, token_scale, durations)
        n_feats = self.decoder.n_feats
        if infill_mel is not None and isinstance(infill_mel, torch.Tensor) and infill_mel.dim() == 3:
            infill_mel, infill_keep = rt.infill_args(infill_mel, infill_keep, B, n_feats, infill_mel.shape[2])
        elif infill_mel is not None or infill_keep is not None:
            infill_mel, infill_keep = rt.infill_args(infill_mel, infill_keep, B, n_feats, 0)
        rt.require_gpu(x, x_lengths, spks, what="MatchaTTS.synthesize")
        rt.step_plan(n_timesteps, t_span, B)  # argument errors before any launch
        if seeds is not None:
            seeds = rt.seed_tensor(seeds, B, x.device)
        if not rt.is_scalar(temperature):
            temperature = rt.per_row(temperature, B, x.device, "temperature")
        if not rt.is_scalar(length_scale):
            length_scale = rt.per_row(length_scale, B, x.device, "length_scale")
        mu, logw, x_mask, oov = self.encoder.forward_unchecked(x, x_lengths, spks)
        flags = [oov[0].to(torch.int64)]
        if token_scale is None and durations is None:
            w_ceil, cum, y_lengths = rt.durations(logw, x_mask, length_scale)
        else:
            w_ceil, cum, y_lengths, bad_w = rt.durations(logw, x_mask, length_scale, token_scale, durations)
            flags.append(bad_w[0].to(torch.int64))
        # validate the estimator's packed weights now, while the GPU runs the encoder, instead of after the
        # host sync below (nothing between here and the solve can change them)
        est = self.decoder.estimator
        est.packed(x.device)
        est._pk.trust_next((est.precision, str(x.device)))
        try:
            # the reference's host sync (model.py:1278-1281), which also brings back the encoder's out-of-vocabulary
            # flag and the duration flag (one device->host copy for all)
            y_max, bad, *bad_w = rt.fetch_ints(torch.stack([y_lengths.max()] + flags))
            if bad:
                raise IndexError("index out of range in self (a token id of x lies outside [0, n_vocab))")
            if bad_w and bad_w[0]:
                raise ValueError("durations / token_scale: every token needs a whole, finite frame count >= 0 and "
                                 "an utterance fewer than 2^24 frames")
            t_pad = fix_len_compatibility(y_max)
            attn, mu_y, y_mask = rt.alignment(cum, y_lengths, t_pad, mu)
            x1 = keep = None
            if infill_mel is not None:  # normalized, then zero-padded or cropped to t_pad (frames past Tk are free)
                tk = min(infill_mel.shape[2], t_pad)
                x1 = torch.zeros((B, n_feats, t_pad), dtype=torch.float32, device=x.device)
                x1[:, :, :tk] = normalize(infill_mel[:, :, :tk].to(device=x.device, dtype=torch.float32),
                                          self.mel_mean, self.mel_std)
                keep = torch.zeros((B, t_pad), dtype=torch.uint8, device=x.device)
                keep[:, :tk] = infill_keep[:, :tk].to(x.device)
            z = self.decoder(mu_y, y_mask, n_timesteps, temperature, spks, cond=None, max_valid=y_max, seeds=seeds,
                             t_span=t_span, x1=x1, keep=keep)
        finally:
            est._pk.untrust()
        mel = rt.denorm_crop(z, self.mel_mean, self.mel_std, y_max)
        return mel, y_lengths, attn

    @torch.inference_mode()
    def synthesise(self, x, x_lengths, n_timesteps, temperature=1.0, spks=None, length_scale=1.0, seeds=None,
                   t_span=None, token_scale=None, durations=None, infill_mel=None, infill_keep=None):
        """Upstream-Matcha-style alias (notebooks: MOS_audiou_generator.ipynb:294) -> dict."""
        import time
        t0 = time.perf_counter()
        mel, y_lengths, attn = self.synthesize(x, x_lengths, n_timesteps, temperature, spks, length_scale, seeds,
                                               t_span, token_scale, durations, infill_mel, infill_keep)
        y_max = mel.shape[-1]
        dt = time.perf_counter() - t0
        return {"mel": mel, "mel_lengths": y_lengths, "attn": attn[:, :, :, :y_max],
                "decoder_outputs": normalize(mel, self.mel_mean, self.mel_std),
                "rtf": dt * 22050 / (y_max * 256)}

    @torch.inference_mode()
    def predict_durations(self, x, x_lengths, spks=None, length_scale=1.0, token_scale=None):
        """The frames per token synthesize would use with these arguments -> int64 [B,Tx] (zero at padded tokens):
        edit them and pass them back as synthesize(durations=...)."""
        B, Tx = x.shape[0], x.shape[1]
        token_scale, _ = rt.duration_args(B, Tx, length_scale, token_scale, None)
        rt.require_gpu(x, x_lengths, spks, what="MatchaTTS.predict_durations")
        _, logw, x_mask, oov = self.encoder.forward_unchecked(x, x_lengths, spks)
        out = rt.durations(logw, x_mask, length_scale, token_scale)
        rt.check_ids(oov)
        if len(out) == 4 and rt.fetch_ints(out[3])[0]:
            raise ValueError("token_scale: every token needs a finite frame count >= 0")
        return out[0][:, 0].to(torch.int64)

    @torch.inference_mode()
    def align(self, x, x_lengths, mel, mel_lengths, spks=None, normalized=False, return_attn=False):
        """Forced alignment of a mel to a text: the frames each token spans under the textbook Monotonic Alignment
        Search on the encoder's mu (rt.align) -> durations int64 [B,Tx], with return_attn also the one-hot attn
        [B,1,Tx,Ty]. mel [B,80,Ty] is denormalized, what synthesize returns (normalized=True: already normalized);
        mel_lengths[b] >= x_lengths[b] (every token takes at least one frame). synthesize(durations=...) then speaks
        the text with the recording's timing."""
        rt.require_gpu(x, x_lengths, mel, spks, what="MatchaTTS.align")
        xl = torch.as_tensor(x_lengths).detach().cpu().to(torch.int64)
        yl = torch.as_tensor(mel_lengths).detach().cpu().to(torch.int64)
        if xl.shape != (x.shape[0],) or yl.shape != xl.shape:
            raise ValueError(f"align: x_lengths {tuple(xl.shape)} / mel_lengths {tuple(yl.shape)}: one per utterance")
        if bool((yl < xl).any()) or int(yl.max()) > mel.shape[-1]:
            raise ValueError(f"align: mel_lengths {yl.tolist()} must cover x_lengths {xl.tolist()} (a frame per "
                             f"token) and fit the mel's {mel.shape[-1]} frames")
        mu, _, _, oov = self.encoder.forward_unchecked(x, x_lengths, spks)
        mean, std = (None, None) if normalized else (self.mel_mean, self.mel_std)
        dur, attn, _ = rt.align(mu, mel, xl, yl, mean, std, want_attn=return_attn)
        rt.check_ids(oov)
        return (dur, attn.unsqueeze(1)) if return_attn else dur

    @torch.inference_mode()
    def edit(self, x_old, x_old_lengths, mel, mel_lengths, x_new, x_new_lengths, spans, n_timesteps, *,
             durations_old=None, margin=0, **synthesize_kwargs):
        """Change a few tokens of a recording and leave every other frame as it was -> (mel_new [B,80,y_max],
        y_lengths int64 [B], keep bool [B,y_max]: the frames taken from `mel`).
        mel [B,80,Ty] (denormalized, mel_lengths frames per row) speaks x_old; spans[b] = (a, b_old, b_new): old tokens
        [a, b_old) are replaced by new tokens [a, b_new). The tokens before a and after the spans must be the same
        ids and the same count in x_old and x_new (ValueError otherwise). Kept tokens keep their old durations
        (durations_old int [B,Tx_old], or align(x_old, ..., mel, ...)), the new span gets predict_durations(x_new, ...)
        (length_scale applies to it only). The recording's frames move to the new layout, the prefix in place and the
        tail shifted by the span's change in frames, and are pinned there by synthesize(x_new, durations=d_new,
        infill_mel=, infill_keep=), minus `margin` frames on each side of the span, which are generated with it.
        synthesize_kwargs: synthesize's other arguments (temperature, spks, seeds, t_span, length_scale); durations
        and token_scale are not accepted. Plain index operations and two host reads: not a hot path."""
        for k in ("durations", "token_scale", "infill_mel", "infill_keep"):
            if k in synthesize_kwargs:
                raise ValueError(f"edit: {k} is formed here (kept tokens keep their recorded durations)")
        if not isinstance(mel, torch.Tensor) or mel.dim() != 3 or mel.shape[1] != self.decoder.n_feats:
            raise ValueError(f"edit: mel [B,{self.decoder.n_feats},Ty] expected")
        B = x_old.shape[0]
        margin = int(margin)
        if x_new.shape[0] != B or mel.shape[0] != B or len(spans) != B or margin < 0:
            raise ValueError(f"edit: one utterance, mel and span per row of x_old ({B}) and margin >= 0 expected")
        xo, xn = x_old.detach().cpu(), x_new.detach().cpu()
        lo = torch.as_tensor(x_old_lengths).detach().cpu().to(torch.int64).tolist()
        ln = torch.as_tensor(x_new_lengths).detach().cpu().to(torch.int64).tolist()
        ml = torch.as_tensor(mel_lengths).detach().cpu().to(torch.int64)
        if len(lo) != B or len(ln) != B or ml.shape != (B,):
            raise ValueError("edit: one length per utterance expected")
        Txo, Txn = x_old.shape[1], x_new.shape[1]
        src_tok = torch.full((B, Txn), -1, dtype=torch.int64)  # the old token a new token keeps the duration of
        for b, sp in enumerate(spans):
            a, b_old, b_new = (int(v) for v in sp)
            if not (0 <= a <= b_old <= lo[b] <= Txo and a <= b_new <= ln[b] <= Txn):
                raise ValueError(f"edit: spans[{b}] = {(a, b_old, b_new)} outside the texts ({lo[b]}, {ln[b]} tokens)")
            if lo[b] - b_old != ln[b] - b_new:
                raise ValueError(f"edit: row {b}: {lo[b] - b_old} tokens after the old span, {ln[b] - b_new} after the "
                                 "new one (the tails must be the same tokens)")
            if not (torch.equal(xo[b, :a], xn[b, :a]) and torch.equal(xo[b, b_old:lo[b]], xn[b, b_new:ln[b]])):
                raise ValueError(f"edit: row {b}: the tokens outside the spans differ between x_old and x_new")
            src_tok[b, :a] = torch.arange(a)
            src_tok[b, b_new:ln[b]] = torch.arange(b_old, lo[b])
        rt.require_gpu(x_old, x_new, mel, what="MatchaTTS.edit")
        dev = x_new.device
        spks = synthesize_kwargs.get("spks")
        if durations_old is None:
            d_old = self.align(x_old, x_old_lengths, mel, mel_lengths, spks=spks)
        else:
            d_old = torch.as_tensor(durations_old).detach()
            if d_old.dtype.is_floating_point or d_old.dtype == torch.bool or d_old.shape != (B, Txo):
                raise ValueError(f"edit: durations_old: integer frame counts [{B}, {Txo}] expected")
            d_old = d_old.to(device=dev, dtype=torch.int64)
        d_pred = self.predict_durations(x_new, x_new_lengths, spks, synthesize_kwargs.pop("length_scale", 1.0))
        src_tok = src_tok.to(dev)
        d_new = torch.where(src_tok >= 0, d_old.gather(1, src_tok.clamp(min=0)), d_pred)
        # frame layout: [0, f_a) the prefix, [f_a, g_b) the new span, [g_b, y_new) the tail = old frames [f_b, y_old)
        a_t = torch.tensor([int(sp[0]) for sp in spans], device=dev)
        bo_t = torch.tensor([int(sp[1]) for sp in spans], device=dev)
        bn_t = torch.tensor([int(sp[2]) for sp in spans], device=dev)
        zero = torch.zeros((B, 1), dtype=torch.int64, device=dev)
        cum_o = torch.cat([zero, d_old.cumsum(1)], 1)
        cum_n = torch.cat([zero, d_new.cumsum(1)], 1)
        f_a = cum_o.gather(1, a_t[:, None])
        f_b = cum_o.gather(1, bo_t[:, None])
        g_b = cum_n.gather(1, bn_t[:, None])
        y_old, y_new = cum_o[:, -1:], cum_n[:, -1:]
        if not torch.equal(y_old[:, 0].cpu(), ml) or int(ml.max()) > mel.shape[2]:
            raise ValueError(f"edit: the old durations sum to {y_old[:, 0].tolist()} frames, mel_lengths are "
                             f"{ml.tolist()} (mel has {mel.shape[2]} frames)")
        y_max = int(y_new.max())
        j = torch.arange(y_max, device=dev)[None]
        tail = (j >= g_b) & (j < y_new)
        src = torch.where(j < f_a, j, torch.where(tail, j - (g_b - f_b), torch.full_like(j, -1)))
        keep = (j < f_a - margin) | (tail & (j >= g_b + margin))
        x1 = mel.to(device=dev, dtype=torch.float32).gather(
            2, src.clamp(0, mel.shape[2] - 1)[:, None, :].expand(B, mel.shape[1], y_max))
        mel_new, y_lengths, _ = self.synthesize(x_new, x_new_lengths, n_timesteps, durations=d_new, infill_mel=x1,
                                                infill_keep=keep, **synthesize_kwargs)
        return mel_new, y_lengths, keep[:, :mel_new.shape[-1]]
