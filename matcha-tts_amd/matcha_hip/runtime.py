"""Host runtime over the C ABI: handles, packed-weight caches and workspaces.

PyTorch owns every device buffer (inputs, outputs, packed weights, workspaces); the
library only enqueues kernels on the current stream. All entry points require CUDA
(ROCm) tensors and raise ``HipPathError`` otherwise — there is no CPU fallback.
"""
from __future__ import annotations

import math
import numbers
import time
from ctypes import byref, c_char_p, c_double, c_int, c_int32, c_int64, c_void_p, create_string_buffer
from typing import Dict, List, Optional, Tuple

import torch

from ._lib import (DTYPE_BF16, DTYPE_F32, SOLVER_EULER, SOLVER_MIDPOINT, HipPathError, check, lib,
                   ptr, stream_handle)

_DTYPES = {"fp32": DTYPE_F32, "float32": DTYPE_F32, "f32": DTYPE_F32,
           "bf16": DTYPE_BF16, "bfloat16": DTYPE_BF16,
           # text encoder only: fp32 storage and arithmetic, the FFN convs' products as six bf16 MFMA products of
           # 3-way bf16 splits (mt_encoder_set_split)
           "fp32x3": DTYPE_F32}


def dtype_code(precision: str) -> int:
    try:
        return _DTYPES[precision]
    except KeyError:
        raise ValueError(f"precision must be one of {sorted(set(_DTYPES))}, got {precision!r}")


def require_gpu(*tensors, what: str = "matcha_hip") -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise HipPathError(
                f"{what}: the synthesis path runs on the MI355X (ROCm) device only; got a tensor on "
                f"{t.device}. Move the model and inputs to 'cuda'.")


def f32c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    return t.detach().to(torch.float32).contiguous()


class _Workspace:
    """Grow-only device scratch per (device, stream)."""

    _bufs: Dict[Tuple[int, int], torch.Tensor] = {}

    @classmethod
    def get(cls, nbytes: int, device: torch.device) -> torch.Tensor:
        key = (device.index if device.index is not None else torch.cuda.current_device(),
               stream_handle(device))
        buf = cls._bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            cls._bufs.pop(key, None)
            buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
            cls._bufs[key] = buf
        return buf


def _param_list(h, num_fn, name_fn, shape_fn) -> List[Tuple[str, Tuple[int, ...]]]:
    L = lib()
    n = getattr(L, num_fn)(h)
    out = []
    buf = create_string_buffer(256)
    shp = (c_int64 * 8)()
    for i in range(n):
        check(getattr(L, name_fn)(h, i, buf, 256), name_fn)
        nd = getattr(L, shape_fn)(h, i, shp, 8)
        if nd < 0:
            check(nd, shape_fn)
        out.append((buf.value.decode(), tuple(int(shp[k]) for k in range(nd))))
    return out


# Every parameter / buffer / submodule (re)registration anywhere bumps this counter (torch's global
# module registration hooks), so PackCache reuses a packed buffer only while no registration happened
# and the module's state tensors are the same tensors at the same addresses and version counters.
_REG = [0]


def _bump_registration(*_args):
    _REG[0] += 1


for _hook in (torch.nn.modules.module.register_module_parameter_registration_hook,
              torch.nn.modules.module.register_module_buffer_registration_hook,
              torch.nn.modules.module.register_module_module_registration_hook):
    _hook(_bump_registration)


class PackCache:
    """Per-module cache of packed weight buffers, keyed by (precision, device).

    A hit costs one pass over the module's state tensors (address + version counter); a miss (first call,
    in-place weight update, `param.data = ...`, a registration such as remove_weight_norm, .to()) makes
    the caller rebuild state_dict() and repack. `trust_next` lets one internal call sequence (synthesize)
    validate early, while the GPU is still busy, and skip the check at the point of use."""

    def __init__(self):
        self.entries = {}
        self.trusted = set()

    def get(self, key):
        e = self.entries.get(key)
        if e is None:
            return None
        if key in self.trusted:
            self.trusted.discard(key)
            return e[3]
        reg, tensors, state, packed = e
        if reg != _REG[0] or [(t.data_ptr(), t._version) for t in tensors] != state:
            return None
        return packed

    def put(self, key, tensors, packed):
        self.entries[key] = (_REG[0], tensors, [(t.data_ptr(), t._version) for t in tensors], packed)
        return packed

    def trust_next(self, key):
        if key in self.entries:
            self.trusted.add(key)

    def untrust(self):
        self.trusted.clear()


def fingerprint(tensors: List[torch.Tensor]) -> Tuple:
    return tuple((t.data_ptr(), t._version, tuple(t.shape), str(t.device)) for t in tensors)


def sinus_freq(c_cond: int) -> torch.Tensor:
    """model.py:757-759 frequency table, formed exactly as the reference does (fp32, CPU)."""
    half = c_cond // 2
    e = math.log(10000) / (half - 1)
    return torch.exp(torch.arange(half).float() * -e)


def rope_theta(head_dim: int) -> torch.Tensor:
    """model.py:258-265 theta table, formed exactly as the reference does (fp32, CPU)."""
    d = int(head_dim * 0.5)
    return 1.0 / (10_000 ** (torch.arange(0, d, 2).float() / d))


class EncoderEngine:
    """mt_encoder handle: text encoder + duration predictor (model.py:452-535) for one config/dtype."""

    def __init__(self, n_vocab: int, n_channels: int, filter_channels: int, n_heads: int, n_layers: int,
                 kernel_size: int, n_spks: int, spk_emb_dim: int, dp_filter: int, dp_kernel: int, prenet: bool,
                 precision: str):
        self.dtype = dtype_code(precision)
        self.width = n_channels + (spk_emb_dim if n_spks > 1 else 0)
        self.head_dim = self.width // n_heads
        h = c_void_p()
        check(lib().mt_encoder_create(n_vocab, n_channels, filter_channels, n_heads, n_layers, kernel_size, n_spks,
                                      spk_emb_dim, dp_filter, dp_kernel, int(bool(prenet)), self.dtype, byref(h)),
              "encoder_create")
        self.h = h
        self.specs = _param_list(h, "mt_encoder_num_params", "mt_encoder_param_name", "mt_encoder_param_shape")
        self.packed_bytes = lib().mt_encoder_packed_bytes(h)
        self._packed = None
        self._fp = None
        if precision == "fp32x3":
            self.set_split(True)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().mt_encoder_destroy(self.h)
        except Exception:
            pass

    def set_mfma_attention(self, enable) -> None:
        """bf16, 96-dim heads: attention core on MFMA (1, default) or on the fp32-VALU kernel (0)."""
        check(lib().mt_encoder_set_mfma_attention(self.h, int(bool(enable))), "encoder_set_mfma_attention")

    def set_vconv(self, enable) -> None:
        """fp32: convs on mt_vconv's fp32 mode (1, default) or on the generic conv kernel (0)."""
        check(lib().mt_encoder_set_vconv(self.h, int(bool(enable))), "encoder_set_vconv")

    def set_split(self, enable) -> None:
        """fp32: the FFN convs on mt_vconv's split-bf16 mode (1; precision "fp32x3") or exact fp32 MFMA (0)."""
        check(lib().mt_encoder_set_split(self.h, int(bool(enable))), "encoder_set_split")

    def set_store_policy(self, mode) -> None:
        """the mt_vconv launches' 16-byte output stores: 0 plain (default), 1 write-through (sc1); same bits. Any
        other mode raises."""
        check(lib().mt_encoder_set_store_policy(self.h, int(mode)), "encoder_set_store_policy")

    def pack(self, params: Dict[str, torch.Tensor], device: torch.device) -> torch.Tensor:
        """params: TextEncoder-relative reference keys -> tensors."""
        tensors = []
        for name, shape in self.specs:
            t = rope_theta(self.head_dim) if name == "_rope_theta" else params.get(name)
            if t is None:
                raise KeyError(f"text encoder parameter {name!r} missing")
            if tuple(t.shape) != shape:
                raise ValueError(f"{name}: shape {tuple(t.shape)} != expected {shape}")
            tensors.append(t)
        fp = fingerprint([t for (n, _), t in zip(self.specs, tensors) if n != "_rope_theta"]) + (str(device),)
        if self._packed is not None and fp == self._fp:
            return self._packed
        dev = [t.detach().to(device=device, dtype=torch.float32).contiguous() for t in tensors]
        packed = torch.empty(self.packed_bytes, dtype=torch.uint8, device=device)
        arr = (c_void_p * len(dev))(*[t.data_ptr() for t in dev])
        check(lib().mt_encoder_pack(self.h, arr, packed.data_ptr(), stream_handle(device)), "encoder_pack")
        torch.cuda.current_stream(device).synchronize()  # staging copies die with `dev`
        self._packed, self._fp = packed, fp
        return packed

    def forward(self, packed, x: torch.Tensor, x_lengths: torch.Tensor, spks: Optional[torch.Tensor] = None):
        """x int64 [B,Tx], x_lengths int64 [B] -> mu [B,80,Tx], logw [B,1,Tx], x_mask [B,1,Tx] (fp32), oov int32 [1]
        (1 when an id of x lies outside [0, n_vocab): see ``check_ids``)."""
        x = x.to(torch.int64).contiguous()
        xl = x_lengths.to(torch.int64).contiguous()
        B, Tx = x.shape
        dev = x.device
        mu = torch.empty(B, 80, Tx, dtype=torch.float32, device=dev)
        logw = torch.empty(B, 1, Tx, dtype=torch.float32, device=dev)
        x_mask = torch.empty(B, 1, Tx, dtype=torch.float32, device=dev)
        L = lib()
        oov = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _Workspace.get(L.mt_encoder_workspace_bytes(self.h, B, Tx), dev)
        check(L.mt_encoder_forward(self.h, packed.data_ptr(), ptr(x), ptr(xl), ptr(spks), B, Tx, ptr(mu), ptr(logw),
                                   ptr(x_mask), ptr(oov), ws.data_ptr(), ws.numel(), stream_handle(dev)),
              "encoder_forward")
        return mu, logw, x_mask, oov


def check_ids(oov: torch.Tensor) -> None:
    """nn.Embedding's error for an out-of-vocabulary token id (model.py:471, 522: ``self.emb(x)`` raises
    IndexError on the CPU; on a GPU torch reports it at the next sync). Reads the encoder's device flag, i.e. one
    host sync: ``MatchaTTS.synthesize`` calls it right after the reference's own sync on max(y_lengths)."""
    if int(oov.item()) != 0:
        raise IndexError("index out of range in self (a token id of x lies outside [0, n_vocab))")


class DecoderEngine:
    """mt_decoder handle: U-Net estimator + CFM solver for one (c_cond, dtype)."""

    def __init__(self, c_cond: int, n_mid: int, n_blocks: int, heads: int, precision: str):
        self.c_cond, self.dtype = c_cond, dtype_code(precision)
        h = c_void_p()
        check(lib().mt_decoder_create(c_cond, n_mid, n_blocks, heads, self.dtype, byref(h)),
              "decoder_create")
        self.h = h
        self.specs = _param_list(h, "mt_decoder_num_params", "mt_decoder_param_name",
                                 "mt_decoder_param_shape")
        self.packed_bytes = lib().mt_decoder_packed_bytes(h)
        self._packed = None
        self._fp = None

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().mt_decoder_destroy(self.h)
        except Exception:
            pass

    def pack(self, params: Dict[str, torch.Tensor], device: torch.device) -> torch.Tensor:
        """params: estimator-relative reference keys -> tensors (any device/dtype)."""
        tensors = []
        for name, shape in self.specs:
            if name == "_sinus_freq":
                t = sinus_freq(self.c_cond)
            else:
                if name not in params:
                    raise KeyError(f"estimator parameter {name!r} missing")
                t = params[name]
            if tuple(t.shape) != shape:
                raise ValueError(f"{name}: shape {tuple(t.shape)} != expected {shape}")
            tensors.append(t)
        fp = fingerprint([t for (n, _), t in zip(self.specs, tensors) if n != "_sinus_freq"]) + (str(device),)
        if self._packed is not None and fp == self._fp:
            return self._packed
        dev = [t.detach().to(device=device, dtype=torch.float32).contiguous() for t in tensors]
        packed = torch.empty(self.packed_bytes, dtype=torch.uint8, device=device)
        arr = (c_void_p * len(dev))(*[t.data_ptr() for t in dev])
        check(lib().mt_decoder_pack(self.h, arr, packed.data_ptr(), stream_handle(device)), "decoder_pack")
        torch.cuda.current_stream(device).synchronize()  # staging copies die with `dev`
        self._packed, self._fp = packed, fp
        return packed

    def set_vconv(self, mode) -> None:
        """bf16: 1 (default) ResnetBlock / down / up / final convs on mt_vconv with block 2's GroupNorm + Mish
        in the res conv's epilogue; 2 the same with that GroupNorm as a separate pass; 0 generic conv kernel.
        True / False map to 1 / 0."""
        check(lib().mt_decoder_set_vconv(self.h, int(mode)), "decoder_set_vconv")

    def set_uniform_attention(self, enable) -> None:
        """1 (default): query-independent attention where the caller's max_valid proves every utterance padded."""
        check(lib().mt_decoder_set_uniform_attention(self.h, int(bool(enable))), "decoder_set_uniform_attention")

    def set_graphs(self, enable) -> None:
        """1 (default): solve() replays its evaluation chain as a cached hipGraph; 0: direct launches."""
        check(lib().mt_decoder_set_graphs(self.h, int(bool(enable))), "decoder_set_graphs")

    def solve(self, packed, z_noise, temperature, mu_y, mask, spks, n_timesteps, solver="euler",
              out=None, max_valid: int = 0, seeds=None, t_span=None, x1=None, keep=None, sigma_min: float = 1e-4):
        """max_valid: the most valid frames of any utterance (synthesize's y_max), 0 when unknown. seeds (int64 [B]
        or B ints): utterance b starts from the seeded stream of seeds[b] (``seeded_noise``) drawn inside the solve,
        z_noise is not read (pass None) and temperature is a number or one value per utterance.
        n_timesteps: an int, or one count per utterance ([B] ints); t_span: a 1-D grid of n + 1 times shared by the
        batch or B such grids (``step_plan``). An int (or B equal ints) without t_span is the graph-replayed solve;
        anything else is one mt_cfm_solve_rows call on the rows sorted by count, in which an utterance is left out
        of every launch after its last step.
        Mel infill: x1 (fp32 [B,80,T], normalized) with keep ([B,T] or [B,1,T], bool or numeric, non-zero = kept)
        holds the kept valid frames on the path (1 - (1 - sigma_min) t) z0 + t x1 while the others are integrated
        (``infill_args``); they come back as x1's bits. Every such call is one mt_cfm_solve_infill call on the sorted
        rows, also with one shared count: the graph path has no infill."""
        B, C, T = mu_y.shape
        x1, keep = infill_args(x1, keep, B, C, T, sigma_min)
        s = SOLVER_EULER if solver == "euler" else SOLVER_MIDPOINT if solver == "midpoint" else None
        if s is None:
            raise NotImplementedError(f"Solver {solver} not implemented")
        if seeds is None and not is_scalar(temperature):
            raise TypeError("solve: one temperature per utterance needs seeds (or scale z_noise per row and pass 1.0)")
        counts, grids = step_plan(n_timesteps, t_span, B)
        if x1 is not None:
            require_gpu(mu_y, x1, keep, what="DecoderEngine.solve")
            return self._solve_rows(packed, z_noise, temperature, mu_y, mask, spks, counts, grids, s, out,
                                    max_valid, seeds, (f32c(x1.to(mu_y.device)), keep.to(mu_y.device), float(sigma_min)))
        if grids is not None or len(set(counts)) > 1:
            return self._solve_rows(packed, z_noise, temperature, mu_y, mask, spks, counts, grids, s, out,
                                    max_valid, seeds)
        n_timesteps = counts[0]
        out = torch.empty_like(mu_y) if out is None else out
        L = lib()
        nbytes = L.mt_cfm_workspace_bytes(self.h, B, T, n_timesteps, s)
        ws = _Workspace.get(nbytes, mu_y.device)
        if seeds is not None:
            sd = seed_tensor(seeds, B, mu_y.device)
            temp = per_row(temperature, B, mu_y.device, "temperature")
            check(L.mt_cfm_solve_seeded(self.h, packed.data_ptr(), ptr(sd), ptr(temp), ptr(mu_y), ptr(mask),
                                        ptr(spks), B, T, int(max_valid), int(n_timesteps), s, ptr(out),
                                        ws.data_ptr(), ws.numel(), stream_handle(mu_y.device)), "cfm_solve_seeded")
            return out
        check(L.mt_cfm_solve_bounded(self.h, packed.data_ptr(), ptr(z_noise), float(temperature), ptr(mu_y),
                                     ptr(mask), ptr(spks), B, T, int(max_valid), int(n_timesteps), s, ptr(out),
                                     ws.data_ptr(), ws.numel(), stream_handle(mu_y.device)), "cfm_solve")
        return out

    def _solve_rows(self, packed, z_noise, temperature, mu_y, mask, spks, counts, grids, s, out, max_valid, seeds,
                    infill=None):
        """solve() with unequal step counts or explicit grids: the C entry point takes the rows sorted by count
        (descending, stable), so gather them, solve, and scatter the result back to the caller's order. infill:
        (x1 fp32 [B,80,T], keep uint8 [B,T], sigma_min) -> mt_cfm_solve_infill, which takes whole grids."""
        B, C, T = mu_y.shape
        dev = mu_y.device
        order = sorted(range(B), key=lambda b: -counts[b])
        perm = None
        if order != list(range(B)):  # from pinned memory: a pageable copy would make the host wait for the stream
            perm = torch.tensor(order, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        take = lambda v: v if v is None or perm is None else v.index_select(0, perm)  # noqa: E731
        sd = None if seeds is None else seed_tensor(seeds, B, dev)
        temp = per_row(temperature, B, dev, "temperature")
        n_max = counts[order[0]]
        n_host = (c_int32 * B)(*[counts[b] for b in order])
        t_host = dt_host = None
        if grids is not None:  # [B][n_max] row-major on the host; dt = t[i + 1] - t[i] in fp32
            t_host = torch.zeros((B, n_max), dtype=torch.float32)
            dt_host = torch.zeros((B, n_max), dtype=torch.float32)
            for r, b in enumerate(order):
                t_host[r, :counts[b]] = grids[b][:-1]
                dt_host[r, :counts[b]] = grids[b][1:] - grids[b][:-1]
        L = lib()
        zs = torch.empty_like(mu_y) if perm is not None or out is None else out
        if infill is not None:
            g_host = None
            if grids is not None:  # [B][n_max + 1]: the clamp after step i takes t[i + 1] itself
                g_host = torch.zeros((B, n_max + 1), dtype=torch.float32)
                for r, b in enumerate(order):
                    g_host[r, :counts[b] + 1] = grids[b]
            ws = _Workspace.get(L.mt_cfm_infill_workspace_bytes(self.h, B, T, n_max, s), dev)
            g = [take(v) for v in (z_noise, sd, temp, mu_y, mask, spks, infill[0], infill[1])]
            check(L.mt_cfm_solve_infill(self.h, packed.data_ptr(), ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]),
                                        ptr(g[4]), ptr(g[5]), ptr(g[6]), ptr(g[7]), infill[2], B, T, int(max_valid),
                                        n_host, ptr(g_host), s, ptr(zs), ws.data_ptr(), ws.numel(),
                                        stream_handle(dev)), "cfm_solve_infill")
            if perm is None:
                return zs
            out = torch.empty_like(mu_y) if out is None else out
            return out.index_copy_(0, perm, zs)
        ws = _Workspace.get(L.mt_cfm_rows_workspace_bytes(self.h, B, T, n_max, s), dev)
        # the gathered copies stay referenced until the launches are enqueued
        g = [take(v) for v in (z_noise, sd, temp, mu_y, mask, spks)]
        check(L.mt_cfm_solve_rows(self.h, packed.data_ptr(), ptr(g[0]), ptr(g[1]), ptr(g[2]), ptr(g[3]), ptr(g[4]),
                                  ptr(g[5]), B, T, int(max_valid), n_host, ptr(t_host), ptr(dt_host), s, ptr(zs),
                                  ws.data_ptr(), ws.numel(), stream_handle(dev)), "cfm_solve_rows")
        if perm is None:
            return zs
        # `out` may be the caller's z_noise: its gathered copy was consumed by the solve, which is ahead in the stream
        out = torch.empty_like(mu_y) if out is None else out
        return out.index_copy_(0, perm, zs)

    TAPS =("down0_res", "down0_tb", "mid1_tb", "up0_out", "up1_tb")

    def step_taps(self, packed, x, mu_y, mask, spks, t: float):
        """One evaluation plus the block outputs of DecoderEngine.TAPS as fp32 [B,256,T_l] (mt_decoder_set_taps)."""
        B, _, T = mu_y.shape
        taps = [torch.empty((B, 256, T // 2 if n == "mid1_tb" else T), dtype=torch.float32, device=mu_y.device)
                for n in self.TAPS]
        arr = (c_void_p * len(taps))(*[t_.data_ptr() for t_ in taps])
        check(lib().mt_decoder_set_taps(self.h, arr, len(taps)), "decoder_set_taps")
        try:
            out = self.step(packed, x, mu_y, mask, spks, t)
            torch.cuda.current_stream(mu_y.device).synchronize()
        finally:
            check(lib().mt_decoder_set_taps(self.h, None, 0), "decoder_set_taps")
        return out, dict(zip(self.TAPS, taps))

    def step(self, packed, x, mu_y, mask, spks, t: float, out=None):
        B, C, T = mu_y.shape
        out = torch.empty_like(mu_y) if out is None else out
        L = lib()
        nbytes = L.mt_decoder_step_workspace_bytes(self.h, B, T)
        ws = _Workspace.get(nbytes, mu_y.device)
        check(L.mt_decoder_step(self.h, packed.data_ptr(), ptr(x), ptr(mu_y), ptr(mask), ptr(spks), float(t),
                                B, T, ptr(out), ws.data_ptr(), ws.numel(), stream_handle(mu_y.device)),
              "decoder_step")
        return out


    def step_times(self, packed, x, mu_y, mask, spks, t: torch.Tensor, out=None):
        """One evaluation with a time per utterance: t [B] (device)."""
        B, C, T = mu_y.shape
        out = torch.empty_like(mu_y) if out is None else out
        tt = f32c(t.reshape(-1).to(mu_y.device))
        if tt.numel() != B:
            raise ValueError(f"t has {tt.numel()} values for a batch of {B}")
        L = lib()
        ws = _Workspace.get(L.mt_decoder_step_times_workspace_bytes(self.h, B, T), mu_y.device)
        check(L.mt_decoder_step_times(self.h, packed.data_ptr(), ptr(x), ptr(mu_y), ptr(mask), ptr(spks), ptr(tt),
                                      B, T, ptr(out), ws.data_ptr(), ws.numel(), stream_handle(mu_y.device)),
              "decoder_step_times")
        return out


class VocoderEngine:
    """mt_vocoder handle: HiFi-GAN Generator for one config and dtype."""

    def __init__(self, h: dict, precision: str):
        self.dtype = dtype_code(precision)
        ur, uk = list(h["upsample_rates"]), list(h["upsample_kernel_sizes"])
        rk = list(h["resblock_kernel_sizes"])
        rd = [list(d) for d in h["resblock_dilation_sizes"]]
        nd = len(rd[0])
        if any(len(d) != nd for d in rd):
            raise ValueError("resblock dilation lists must have equal length")
        flat = [x for d in rd for x in d]
        ci = lambda v: (c_int * len(v))(*v)  # noqa: E731
        hdl = c_void_p()
        check(lib().mt_vocoder_create(1 if str(h["resblock"]) == "1" else 2, len(ur), ci(ur), ci(uk),
                                      int(h["upsample_initial_channel"]), len(rk), ci(rk), nd, ci(flat),
                                      self.dtype, byref(hdl)), "vocoder_create")
        self.h = hdl
        self.hop = int(math.prod(ur))
        self.specs = _param_list(hdl, "mt_vocoder_num_params", "mt_vocoder_param_name",
                                 "mt_vocoder_param_shape")
        self.packed_bytes = lib().mt_vocoder_packed_bytes(hdl)
        self._packed = None
        self._fp = None

    def set_fusion(self, enable: bool) -> None:
        check(lib().mt_vocoder_set_fusion(self.h, int(bool(enable))), "vocoder_set_fusion")

    def set_pair(self, mode) -> None:
        """bf16 ResBlock pairs as one launch each: 1 (default) the 64- / 32-channel stages and the 128-channel
        stage's k = 3 resblock; 4 every 128-channel pair too; 2 none of the 128-channel stage; 0 all per layer."""
        check(lib().mt_vocoder_set_pair(self.h, int(mode)), "vocoder_set_pair")

    def set_store_policy(self, stage_mask) -> None:
        """bit i: stage i's launches store their 16-byte outputs write-through (sc1) instead of plain (0, the
        default, everywhere); same bits. A mask naming a missing stage raises."""
        check(lib().mt_vocoder_set_store_policy(self.h, int(stage_mask)), "vocoder_set_store_policy")

    def set_vconv(self, mode) -> None:
        """0 generic per-layer kernel, 1 vconv for the 128/256-channel stages, 2 (default) also for 64."""
        check(lib().mt_vocoder_set_vconv(self.h, int(mode)), "vocoder_set_vconv")

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib().mt_vocoder_destroy(self.h)
        except Exception:
            pass

    def pack(self, params_fn, src: List[torch.Tensor], device: torch.device) -> torch.Tensor:
        """params_fn() -> folded reference-keyed weights; repacked only when ``src`` changes."""
        fp = fingerprint(src) + (str(device),)
        if self._packed is not None and fp == self._fp:
            return self._packed
        params = params_fn()
        tensors = []
        for name, shape in self.specs:
            if name not in params:
                raise KeyError(f"vocoder parameter {name!r} missing")
            t = params[name]
            if tuple(t.shape) != shape:
                raise ValueError(f"{name}: shape {tuple(t.shape)} != expected {shape}")
            tensors.append(t)
        dev = [t.detach().to(device=device, dtype=torch.float32).contiguous() for t in tensors]
        packed = torch.empty(self.packed_bytes, dtype=torch.uint8, device=device)
        arr = (c_void_p * len(dev))(*[t.data_ptr() for t in dev])
        check(lib().mt_vocoder_pack(self.h, arr, packed.data_ptr(), stream_handle(device)), "vocoder_pack")
        torch.cuda.current_stream(device).synchronize()
        self._packed, self._fp = packed, fp
        return packed

    def ragged_supported(self) -> bool:
        return bool(lib().mt_vocoder_ragged_supported(self.h))

    def forward(self, packed, mel, out=None, lengths=None):
        """lengths (int [B], mel frames, or None): a ragged batch, utterance b vocoded at its own lengths[b]
        frames (mt_vocoder_forward_ragged); its samples past hop * lengths[b] are zero"""
        B, C, T = mel.shape
        out = torch.empty((B, 1, T * self.hop), dtype=torch.float32, device=mel.device) if out is None else out
        L = lib()
        ws = _Workspace.get(L.mt_vocoder_workspace_bytes(self.h, B, T), mel.device)
        if lengths is None:
            check(L.mt_vocoder_forward(self.h, packed.data_ptr(), ptr(mel), B, T, ptr(out), ws.data_ptr(),
                                       ws.numel(), stream_handle(mel.device)), "vocoder_forward")
            return out
        lens = lengths.to(device=mel.device, dtype=torch.int32).contiguous()
        if lens.shape != (B,):
            raise ValueError(f"lengths {tuple(lens.shape)}: expected ({B},)")
        check(L.mt_vocoder_forward_ragged(self.h, packed.data_ptr(), ptr(mel), B, T, ptr(lens), ptr(out),
                                          ws.data_ptr(), ws.numel(), stream_handle(mel.device)), "vocoder_forward")
        return out


# ---- index path / small ops ---------------------------------------------------------------

# utterances one ragged vocoder launch chain takes (mt_ragged.h RAG_MAXB: the per-utterance tile table lives in LDS);
# Generator.forward splits larger batches (tests/test_abi_host.py checks the two stay equal)
RAGGED_MAX_BATCH = 512

_HOST_BUFS: Dict[tuple, torch.Tensor] = {}


def fetch_ints(t: torch.Tensor) -> List[int]:
    """A few device int64 values -> Python ints (synthesize's one host sync, model.py:1278-1281): an async copy into
    a pinned buffer, then the host polls the copy's event. A blocking wait lets the host thread sleep, and its
    wake-up left the GPU idle ≈ 0.16 ms between the durations and the alignment kernels in the B = 32 bench trace
    (profiles/r06b_kernel_stats.csv's step)."""
    import threading
    n = t.numel()
    key = (str(t.device), n, threading.get_ident())
    buf = _HOST_BUFS.get(key)
    if buf is None:
        buf = _HOST_BUFS[key] = torch.empty(n, dtype=torch.int64, pin_memory=True)
    buf.copy_(t.reshape(-1).to(torch.int64), non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(t.device))
    polls = 0
    while not ev.query():
        polls += 1
        if polls > 256:  # past the first ~0.5 ms: yield the core between polls (a long encoder at large B)
            time.sleep(0)
    return buf.tolist()


def is_scalar(v) -> bool:
    """a Python / numpy number or a 0-d tensor: one value for the whole batch"""
    return isinstance(v, numbers.Real) or (isinstance(v, torch.Tensor) and v.dim() == 0)


def cosine_grid(n: int) -> torch.Tensor:
    """The n + 1 fp32 times 1 - cos(pi/2 * i/n), i = 0..n (CPU): a t_span with small steps near t = 0. Formed in
    fp64 and rounded once; the ends are exactly 0 and 1."""
    n = int(n)
    if n < 1:
        raise ValueError(f"cosine_grid: n = {n} must be >= 1")
    i = torch.arange(n + 1, dtype=torch.float64)
    g = (1.0 - torch.cos(i * (math.pi / 2 / n))).to(torch.float32)
    g[0], g[-1] = 0.0, 1.0
    return g


def _grid(g, what: str) -> torch.Tensor:
    """one time grid -> fp32 [n + 1] on the CPU, strictly increasing inside [0, 1]"""
    g = torch.as_tensor(g).detach().to(device="cpu", dtype=torch.float32).contiguous()
    if g.dim() != 1 or g.numel() < 2:
        raise ValueError(f"{what}: a 1-D grid of n + 1 >= 2 times expected, got shape {tuple(g.shape)}")
    if not bool(torch.isfinite(g).all()) or float(g[0]) < 0.0 or float(g[-1]) > 1.0:
        raise ValueError(f"{what}: the times must lie inside [0, 1]")
    if not bool((g[1:] > g[:-1]).all()):
        raise ValueError(f"{what}: the times must be strictly increasing")
    return g


def step_plan(n_timesteps, t_span, B: int):
    """solve()'s step arguments -> (counts, grids): counts a list of B ints >= 1, grids None (the reference's grid
    i / n per utterance) or a list of B fp32 CPU grids of counts[b] + 1 times. n_timesteps: an int or one per
    utterance ([B] tensor or sequence; None with t_span). t_span: one 1-D grid (tensor or sequence of numbers)
    shared by the batch, or B of them (a sequence of 1-D tensors / sequences, or a [B, n + 1] tensor). Raises
    ValueError for a wrong length, a count < 1, a grid that is not strictly increasing inside [0, 1], or counts
    that disagree with the grids."""
    counts = None
    if n_timesteps is not None:
        if is_scalar(n_timesteps):
            counts = [int(n_timesteps)] * B
        else:
            nt = torch.as_tensor(n_timesteps).detach().cpu()
            if nt.shape != (B,):
                raise ValueError(f"n_timesteps {tuple(nt.shape)}: expected an int or one count per utterance, ({B},)")
            if nt.dtype.is_floating_point and not bool((nt == nt.round()).all()):
                raise ValueError("n_timesteps: whole step counts expected")
            counts = [int(v) for v in nt.tolist()]
            if min(counts) < 1:
                raise ValueError(f"n_timesteps: every count must be >= 1, got {counts}")
    if t_span is None:
        if counts is None:
            raise ValueError("solve: n_timesteps or t_span is needed")
        return counts, None
    shared = (isinstance(t_span, torch.Tensor) and t_span.dim() == 1) or (
        not isinstance(t_span, torch.Tensor) and len(t_span) > 0 and all(is_scalar(v) for v in t_span))
    if shared:
        grids = [_grid(t_span, "t_span")] * B
    else:
        if len(t_span) != B:
            raise ValueError(f"t_span: {len(t_span)} grids for a batch of {B} (one shared 1-D grid, or one per "
                             "utterance)")
        grids = [_grid(g, f"t_span[{b}]") for b, g in enumerate(t_span)]
    steps = [g.numel() - 1 for g in grids]
    if counts is not None and counts != steps:
        raise ValueError(f"n_timesteps {counts} disagrees with t_span's {steps} steps")
    return steps, grids


def infill_args(x1, keep, B: int, C: int, T: int, sigma_min: float = 1e-4):
    """solve()'s infill arguments, checked on the host before any launch -> (x1, keep uint8 [B,T] contiguous) on the
    devices they came from, or (None, None). x1: a floating [B,C,T] tensor; keep: bool or numeric [B,T] or [B,1,T],
    non-zero = kept. One without the other, a wrong shape or a sigma_min outside [0, 1) raises ValueError, a
    non-tensor or a non-floating x1 / complex keep TypeError."""
    if x1 is None and keep is None:
        return None, None
    if x1 is None or keep is None:
        raise ValueError("infill: x1 and keep come together (%s is missing)" % ("x1" if x1 is None else "keep"))
    if not isinstance(x1, torch.Tensor) or not x1.dtype.is_floating_point:
        raise TypeError("infill: x1 is a floating-point [B,C,T] tensor")
    keep = torch.as_tensor(keep)
    if keep.dtype.is_complex:
        raise TypeError(f"infill: keep is bool or numeric, got {keep.dtype}")
    if tuple(x1.shape) != (B, C, T):
        raise ValueError(f"infill: x1 {tuple(x1.shape)}: expected ({B}, {C}, {T})")
    if tuple(keep.shape) not in ((B, T), (B, 1, T)):
        raise ValueError(f"infill: keep {tuple(keep.shape)}: expected ({B}, {T}) or ({B}, 1, {T})")
    if not (0.0 <= float(sigma_min) < 1.0):
        raise ValueError(f"infill: sigma_min {sigma_min} outside [0, 1)")
    return x1, (keep.detach().reshape(B, T) != 0).to(torch.uint8).contiguous()


def rows_plan(counts, solver: str = "euler") -> List[int]:
    """mt_cfm_rows_plan: the rows (a prefix of the batch sorted by count, descending) each estimator evaluation of a
    per-utterance solve runs on"""
    n = (c_int32 * len(counts))(*[int(c) for c in counts])
    cap = 2 * max([int(c) for c in counts] + [1])
    rows = (c_int32 * cap)()
    S = lib().mt_cfm_rows_plan(n, len(counts), SOLVER_MIDPOINT if solver == "midpoint" else SOLVER_EULER, rows, cap)
    if S < 0:
        check(S, "cfm_rows_plan")
    return list(rows[:S])


def per_row(v, B: int, device, name: str) -> torch.Tensor:
    """a number, or one value per utterance ([B] tensor or sequence) -> fp32 [B] on `device`"""
    if is_scalar(v):
        return torch.full((B,), float(v), dtype=torch.float32, device=device)
    t = torch.as_tensor(v).detach().to(device=device, dtype=torch.float32).contiguous()
    if t.shape != (B,):
        raise ValueError(f"{name} {tuple(t.shape)}: expected a number or one value per utterance, ({B},)")
    return t


def seed_tensor(seeds, B: int, device) -> torch.Tensor:
    """seeds: int64 [B] tensor or a sequence of B ints -> int64 [B] on `device`. A bare int is refused: it could
    mean one stream shared by every utterance or a base seed to derive B streams from."""
    if isinstance(seeds, numbers.Number) or (isinstance(seeds, torch.Tensor) and seeds.dim() == 0):
        raise TypeError("seeds: one int64 seed per utterance ([B] tensor or sequence), not a bare int")
    t = torch.as_tensor(seeds)
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise TypeError(f"seeds: integer seeds expected, got {t.dtype}")
    t = t.detach().to(device=device, dtype=torch.int64).contiguous()
    if t.shape != (B,):
        raise ValueError(f"seeds {tuple(t.shape)}: expected one seed per utterance, ({B},)")
    return t


def seeded_noise(seeds: torch.Tensor, T: int, temperature=None, C: int = 80) -> torch.Tensor:
    """The seeded noise stream (matcha_hip/noise.py is its CPU specification) -> fp32 [B,C,T] on the seeds' device:
    row b is a function of (seeds[b], channel, frame) only, times temperature (None: 1; a number or [B])."""
    if not isinstance(seeds, torch.Tensor):
        raise TypeError("seeded_noise: seeds is an int64 [B] tensor on the GPU (its device is the result's)")
    require_gpu(seeds, what="seeded_noise")
    if seeds.dim() != 1:
        raise ValueError(f"seeds {tuple(seeds.shape)}: expected [B]")
    B = seeds.shape[0]
    sd = seed_tensor(seeds, B, seeds.device)
    temp = None if temperature is None else per_row(temperature, B, seeds.device, "temperature")
    z = torch.empty((B, int(C), int(T)), dtype=torch.float32, device=seeds.device)
    check(lib().mt_noise_fill(ptr(sd), ptr(temp), B, int(C), int(T), ptr(z), stream_handle(seeds.device)),
          "noise_fill")
    return z


def _durations_exclude_scales(length_scale, token_scale) -> None:
    if token_scale is not None or not (is_scalar(length_scale) and float(length_scale) == 1.0):
        raise ValueError("durations replaces the duration predictor: length_scale / token_scale do not apply to it "
                         "(scale the durations instead)")


def duration_args(B: int, Tx: int, length_scale=1.0, token_scale=None, durations=None):
    """synthesize's duration-control arguments, checked on the host before any launch -> (token_scale fp32 [B,Tx] |
    None, durations fp32 [B,Tx] | None), on the devices they came from. token_scale: a [B,Tx] tensor or B sequences
    of Tx numbers. durations: whole frames per token, an integer [B,Tx] tensor or B sequences of Tx ints; they replace
    the predictor, so a length_scale other than the number 1 or a token_scale next to them raises ValueError."""
    if durations is not None:
        _durations_exclude_scales(length_scale, token_scale)
        d = torch.as_tensor(durations).detach()
        if d.dtype.is_floating_point or d.dtype.is_complex or d.dtype == torch.bool:
            raise TypeError(f"durations: whole frame counts of an integer dtype expected, got {d.dtype}")
        if d.shape != (B, Tx):
            raise ValueError(f"durations {tuple(d.shape)}: expected one frame count per token, ({B}, {Tx})")
        return None, d.to(torch.float32).contiguous()
    if token_scale is None:
        return None, None
    ts = torch.as_tensor(token_scale).detach().to(torch.float32).contiguous()
    if ts.shape != (B, Tx):
        raise ValueError(f"token_scale {tuple(ts.shape)}: expected one scale per token, ({B}, {Tx})")
    return ts, None


def durations(logw: Optional[torch.Tensor], x_mask: torch.Tensor, length_scale=1.0, token_scale=None,
              durations=None):
    """model.py:1273-1275 -> (w_ceil [B,1,Tx], cum [B,Tx], y_lengths int64 [B]). length_scale: a number, or one
    per utterance ([B] tensor or sequence; mt_durations_scaled).
    Duration control (mt_durations_tokens), taken only when one of the two is given, and then the result has a fourth
    entry, the device flag `bad` (int32 [1]: a frame count that is negative, not finite or fractional, or a row of
    2^24 frames or more): token_scale fp32 [B,Tx] multiplies each token's predicted length before the ceil;
    durations [B,Tx] are the frame counts themselves (logw may be None; zeros are legal)."""
    require_gpu(logw, x_mask, what="durations")
    logw, x_mask = f32c(logw), f32c(x_mask)
    B, _, Tx = x_mask.shape
    dev = x_mask.device
    w_ceil = torch.empty((B, 1, Tx), dtype=torch.float32, device=dev)
    cum = torch.empty((B, Tx), dtype=torch.float32, device=dev)
    yl = torch.empty((B,), dtype=torch.int64, device=dev)
    if token_scale is not None or durations is not None:
        ts = dur = ls = None
        if durations is not None:
            _durations_exclude_scales(length_scale, token_scale)
            dur = f32c(torch.as_tensor(durations).to(dev)).reshape(-1)
        else:
            ts = f32c(torch.as_tensor(token_scale).to(dev)).reshape(-1)
            ls = per_row(length_scale, B, dev, "length_scale")
        if (ts if dur is None else dur).numel() != B * Tx:
            raise ValueError(f"token_scale / durations: expected ({B}, {Tx}) values")
        bad = torch.empty((1,), dtype=torch.int32, device=dev)
        check(lib().mt_durations_tokens(ptr(logw), ptr(x_mask), ptr(ls), ptr(ts), ptr(dur), B, Tx, ptr(w_ceil),
                                        ptr(cum), ptr(yl), ptr(bad), stream_handle(dev)), "durations_tokens")
        return w_ceil, cum, yl, bad
    if not is_scalar(length_scale):
        ls = per_row(length_scale, B, logw.device, "length_scale")
        check(lib().mt_durations_scaled(ptr(logw), ptr(x_mask), ptr(ls), B, Tx, ptr(w_ceil), ptr(cum), ptr(yl),
                                        stream_handle(logw.device)), "durations_scaled")
        return w_ceil, cum, yl
    check(lib().mt_durations(ptr(logw), ptr(x_mask), float(length_scale), B, Tx, ptr(w_ceil), ptr(cum),
                             ptr(yl), stream_handle(logw.device)), "durations")
    return w_ceil, cum, yl


def alignment(cum: torch.Tensor, y_lengths: torch.Tensor, t_pad: int, mu: Optional[torch.Tensor],
              want_attn: bool = True):
    """model.py:1283-1289 -> (attn [B,1,Tx,T] | None, mu_y [B,C,T] | None, y_mask [B,1,T])."""
    B, Tx = cum.shape
    dev = cum.device
    attn = torch.empty((B, 1, Tx, t_pad), dtype=torch.float32, device=dev) if want_attn else None
    C = 0 if mu is None else mu.shape[1]
    mu = f32c(mu)
    mu_y = torch.empty((B, C, t_pad), dtype=torch.float32, device=dev) if mu is not None else None
    y_mask = torch.empty((B, 1, t_pad), dtype=torch.float32, device=dev)
    check(lib().mt_alignment(ptr(cum), ptr(y_lengths), B, Tx, t_pad, ptr(mu), C, ptr(attn), ptr(mu_y),
                             ptr(y_mask), stream_handle(dev)), "alignment")
    return attn, mu_y, y_mask


def denorm_crop(z: torch.Tensor, mean: torch.Tensor, std: torch.Tensor, t_y: int) -> torch.Tensor:
    B, C, T = z.shape
    mean = f32c(mean.to(z.device)).reshape(-1).expand(C).contiguous()
    std = f32c(std.to(z.device)).reshape(-1).expand(C).contiguous()
    out = torch.empty((B, C, t_y), dtype=torch.float32, device=z.device)
    check(lib().mt_denorm_crop(ptr(z), ptr(mean), ptr(std), B, C, T, t_y, ptr(out), stream_handle(z.device)),
          "denorm_crop")
    return out


def stft_magnitude(audio: torch.Tensor) -> torch.Tensor:
    require_gpu(audio, what="stft_magnitude")
    audio = f32c(audio)
    B, L = audio.shape
    nfr = 1 + L // 256
    mag = torch.empty((B, nfr, 513), dtype=torch.float32, device=audio.device)
    check(lib().mt_stft_magnitude(ptr(audio), B, L, ptr(mag), stream_handle(audio.device)), "stft_magnitude")
    return mag


def denoise(audio: torch.Tensor, bias_spec: torch.Tensor, strength: float, lengths=None,
            hop: int = 256) -> torch.Tensor:
    """lengths (int [B] in units of `hop` samples, or None): a ragged batch, row b denoised as an utterance of
    hop * lengths[b] samples (mt_denoise_ragged); its output past them is zero"""
    require_gpu(audio, what="denoise")
    audio = f32c(audio)
    B, L = audio.shape
    out = torch.empty((B, 256 * (L // 256)), dtype=torch.float32, device=audio.device)
    bias = f32c(bias_spec.reshape(-1).to(audio.device))
    L_ = lib()
    ws = _Workspace.get(L_.mt_denoise_workspace_bytes(B, L), audio.device)
    if lengths is None:
        check(L_.mt_denoise(ptr(audio), B, L, ptr(bias), float(strength), ptr(out), ws.data_ptr(), ws.numel(),
                            stream_handle(audio.device)), "denoise")
        return out
    lens = lengths.to(device=audio.device, dtype=torch.int32).contiguous()
    if lens.shape != (B,):
        raise ValueError(f"lengths {tuple(lens.shape)}: expected ({B},)")
    check(L_.mt_denoise_ragged(ptr(audio), B, L, ptr(lens), int(hop), ptr(bias), float(strength), ptr(out),
                               ws.data_ptr(), ws.numel(), stream_handle(audio.device)), "denoise")
    return out


# ---- audio output stage (audio_out.py is the specification) ------------------------------------

# outputs per workgroup of resample_kernel (mt_audio.hip RS_TN): tests put utterance ends around its multiples
RESAMPLE_TILE = 2048
NORMALIZE_CODES = {None: 0, "peak": 1, "rms": 2}
ENCODING_CODES = {"f32": (0, torch.float32), "pcm16": (1, torch.int16), "mulaw": (2, torch.uint8)}
DEFAULT_LEVEL = {None: 1.0, "peak": 0.95, "rms": 10 ** (-20 / 20)}  # 0.95: hifigan/meldataset.py's normalisation


class ResamplePlan:
    """One rate change: the factor, the filter (h fp64 on the host, specification) and its fp32 taps by phase
    [up][ceil((2 half + 1) / up)] on the device, as mt_resample reads them."""

    def __init__(self, src: int, dst: int, zeros: int, beta: float, device: torch.device):
        from . import audio_out
        self.src, self.dst = int(src), int(dst)
        self.up, self.down = audio_out.rates(src, dst)
        self.h, self.half = audio_out.design_filter(self.up, self.down, zeros, beta)
        self.taps_host = audio_out.polyphase(self.h, self.half, self.up).astype("float32")
        self.taps = torch.from_numpy(self.taps_host).to(device)
        self.device = device

    def out_length(self, n: int) -> int:
        return -((-int(n) * self.up) // self.down)


_PLANS: Dict[tuple, ResamplePlan] = {}


def resample_plan(src: int, dst: int, zeros: int = 10, beta: float = 5.0, device=None) -> ResamplePlan:
    """The plan of src -> dst Hz, cached per (src, dst, zeros, beta, device). ValueError for a factor above 1024."""
    from . import audio_out
    audio_out.rates(src, dst)  # refuse the factor before anything touches the device
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type != "cuda":
        raise HipPathError(f"resample_plan: the output stage runs on the MI355X (ROCm) device only; got {device}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(src), int(dst), int(zeros), float(beta), device.index)
    plan = _PLANS.get(key)
    if plan is None:
        plan = _PLANS[key] = ResamplePlan(src, dst, zeros, beta, device)
    return plan


def _lens32(lengths, B: int, device) -> Optional[torch.Tensor]:
    if lengths is None:
        return None
    lens = torch.as_tensor(lengths).to(device=device, dtype=torch.int32).contiguous()
    if lens.shape != (B,):
        raise ValueError(f"lengths {tuple(lens.shape)}: expected ({B},)")
    return lens


def resample(audio: torch.Tensor, plan: ResamplePlan, lengths=None, lmul: int = 1):
    """audio [B, L] -> (out fp32 [B, ceil(L up / down)], out_lens int32 [B]). lengths (int [B] in units of `lmul`
    samples, or None = L): row b is resampled as an utterance of that length alone, ceil(len up / down) samples,
    zero after them (mt_resample)."""
    require_gpu(audio, what="resample")
    audio = f32c(audio)
    B, L = audio.shape
    lens = _lens32(lengths, B, audio.device)
    Lout = plan.out_length(L)
    out = torch.empty((B, Lout), dtype=torch.float32, device=audio.device)
    out_lens = torch.empty((B,), dtype=torch.int32, device=audio.device)
    L_ = lib()
    taps = plan.taps if plan.taps.device == audio.device else plan.taps.to(audio.device)
    ws = _Workspace.get(L_.mt_resample_workspace_bytes(plan.half, plan.up, plan.down), audio.device)
    check(L_.mt_resample(ptr(audio), B, L, ptr(lens), int(lmul), ptr(taps), plan.half, plan.up, plan.down, ptr(out),
                         Lout, ptr(out_lens), ws.data_ptr(), ws.numel(), stream_handle(audio.device)), "resample")
    return out, out_lens


def audio_stats(audio: torch.Tensor, lengths=None):
    """audio [B, L], lengths in samples (int [B], or None = L) -> (peak fp32 [B] = max |x|, meansq fp64 [B] = mean
    x^2) over each row's valid samples (mt_audio_stats)"""
    require_gpu(audio, what="audio_stats")
    audio = f32c(audio)
    B, L = audio.shape
    lens = _lens32(lengths, B, audio.device)
    peak = torch.empty((B,), dtype=torch.float32, device=audio.device)
    meansq = torch.empty((B,), dtype=torch.float64, device=audio.device)
    L_ = lib()
    ws = _Workspace.get(L_.mt_audio_stats_workspace_bytes(B, L), audio.device)
    check(L_.mt_audio_stats(ptr(audio), B, L, ptr(lens), ptr(peak), ptr(meansq), ws.data_ptr(), ws.numel(),
                            stream_handle(audio.device)), "audio_stats")
    return peak, meansq


def encode_audio(audio: torch.Tensor, lengths=None, normalize=None, level=None, limit: bool = True,
                 encoding: str = "f32", stats=None):
    """audio [B, L], lengths in samples -> (out [B, L] fp32 / int16 / uint8, gain fp32 [B]): each row times its gain
    (audio_out.gain_ref of its peak and mean square: `stats`, or audio_stats of it), clamped to [-1, 1], encoded
    (mt_audio_encode); past a row's length 0, 0 and 0xFF."""
    require_gpu(audio, what="encode_audio")
    if normalize not in NORMALIZE_CODES:
        raise ValueError(f"normalize must be one of {list(NORMALIZE_CODES)}, got {normalize!r}")
    if encoding not in ENCODING_CODES:
        raise ValueError(f"encoding must be one of {list(ENCODING_CODES)}, got {encoding!r}")
    audio = f32c(audio)
    B, L = audio.shape
    lens = _lens32(lengths, B, audio.device)
    peak = meansq = None
    if normalize is not None:
        peak, meansq = audio_stats(audio, lens) if stats is None else stats
    code, dtype = ENCODING_CODES[encoding]
    out = torch.empty((B, L), dtype=dtype, device=audio.device)
    gain = torch.empty((B,), dtype=torch.float32, device=audio.device)
    level = DEFAULT_LEVEL[normalize] if level is None else float(level)
    check(lib().mt_audio_encode(ptr(audio), B, L, ptr(lens), ptr(peak), ptr(meansq), NORMALIZE_CODES[normalize],
                                level, int(bool(limit)), code, ptr(out), ptr(gain), stream_handle(audio.device)),
          "audio_encode")
    return out, gain


# ---- recording input stage (audio_in.py is the specification) ----------------------------------

# frames per workgroup of logmel_ragged_kernel (mt_audio_in.hip LMR_FPW): tests put row ends around its multiples
LOGMEL_FRAMES = 8


def decode_audio(raw: torch.Tensor, lengths=None, encoding: str = "f32", channels: int = 1) -> torch.Tensor:
    """raw [B, Lcap * channels] interleaved frames of the encoding's dtype (float32 / int16 / uint8), lengths in
    frames (int [B], or None = Lcap) -> mono fp32 [B, Lcap]: audio_in.decode_ref of every row, zero from its length
    on (mt_audio_decode). Nothing of raw at or past a row's length is read."""
    require_gpu(raw, what="decode_audio")
    if encoding not in ENCODING_CODES:
        raise ValueError(f"encoding must be one of {list(ENCODING_CODES)}, got {encoding!r}")
    channels = int(channels)
    if not 1 <= channels <= 8:
        raise ValueError(f"channels must be in 1..8, got {channels}")
    code, dtype = ENCODING_CODES[encoding]
    if raw.dtype != dtype:
        raise ValueError(f"decode_audio: {encoding} frames are {dtype}, got {raw.dtype}")
    if raw.dim() != 2 or raw.shape[1] == 0 or raw.shape[1] % channels:
        raise ValueError(f"decode_audio: raw {tuple(raw.shape)}, expected [B, Lcap * {channels}] with Lcap >= 1")
    raw = raw.contiguous()
    B, Lcap = raw.shape[0], raw.shape[1] // channels
    lens = _lens32(lengths, B, raw.device)
    out = torch.empty((B, Lcap), dtype=torch.float32, device=raw.device)
    check(lib().mt_audio_decode(ptr(raw), B, Lcap, ptr(lens), code, channels, ptr(out), stream_handle(raw.device)),
          "audio_decode")
    return out


def log_mel_ragged(audio: torch.Tensor, basis: torch.Tensor, start=None, end=None, gain=None, mel_mean: float = 0.0,
                   mel_std: float = 1.0, fill: float = 0.0, Fcap: Optional[int] = None):
    """audio [B, L]; start / end int [B] in samples (None: 0 / L), gain fp32 [B] (None: 1); basis fp32 [80, 513] ->
    (mel fp32 [B, 80, Fcap], frames int32 [B]): row b's frames are mt_log_mel's bits for fl32(gain[b] audio[b][start[b]
    : end[b]]) held alone, reflected at its own ends; `fill` from frames[b] on (mt_log_mel_ragged). Fcap defaults to
    the frame count of a row of L samples. audio is read in place when it is contiguous fp32; nothing comes back to
    the host."""
    from . import audio_in
    require_gpu(audio, basis, what="log_mel_ragged")
    audio = f32c(audio)
    if audio.dim() != 2:
        raise ValueError(f"log_mel_ragged: audio {tuple(audio.shape)}, expected [B, L]")
    B, L = audio.shape
    if tuple(basis.shape) != (80, 513) or basis.dtype != torch.float32:
        raise ValueError(f"log_mel_ragged: basis {tuple(basis.shape)} {basis.dtype}, expected fp32 [80, 513]")
    if float(mel_std) == 0.0:
        raise ValueError("log_mel_ragged: mel_std must be non-zero")
    need = audio_in.frames_ref(L)
    Fcap = need if Fcap is None else int(Fcap)
    if Fcap < need:
        raise ValueError(f"log_mel_ragged: Fcap {Fcap} < {need}, the frames of a row of {L} samples")
    start, end = _lens32(start, B, audio.device), _lens32(end, B, audio.device)
    if gain is not None:
        gain = f32c(gain.to(audio.device))
        if gain.shape != (B,):
            raise ValueError(f"gain {tuple(gain.shape)}: expected ({B},)")
    mel = torch.empty((B, 80, Fcap), dtype=torch.float32, device=audio.device)
    frames = torch.empty((B,), dtype=torch.int32, device=audio.device)
    check(lib().mt_log_mel_ragged(ptr(audio), B, L, ptr(start), ptr(end), ptr(gain), ptr(basis.contiguous()),
                                  float(mel_mean), float(mel_std), float(fill), ptr(mel) if Fcap else None, Fcap,
                                  ptr(frames), stream_handle(audio.device)), "log_mel_ragged")
    return mel, frames


# ---- loudness and true peak (loudness.py is the specification) ---------------------------------

# samples per chunk and per tile of the K-weighting scan (mt_loudness.hip KW_CH, KW_TILE): tests put row ends around
# their multiples
LOUDNESS_CHUNK = 32
LOUDNESS_TILE = 8192


def loudness(audio: torch.Tensor, lengths, sample_rate: int, return_blocks: bool = False):
    """audio [B, L] at sample_rate, lengths in samples (int [B], or None = L) -> (energy fp64 [B], nblocks int32 [B])
    and, with return_blocks, z fp64 [B, J(L)]: the gated mean square of each row's K-weighted signal
    (loudness.gate_ref of its block energies z; LUFS = -0.691 + 10 log10 energy), its block count, its blocks, zero
    from nblocks[b] on (mt_loudness)."""
    from . import loudness as ld
    coef = ld.coefficients(sample_rate)  # ValueError below 8 kHz
    require_gpu(audio, what="loudness")
    hop = ld.hop_of(sample_rate)
    audio = f32c(audio)
    B, L = audio.shape
    lens = _lens32(lengths, B, audio.device)
    energy = torch.empty((B,), dtype=torch.float64, device=audio.device)
    nblocks = torch.empty((B,), dtype=torch.int32, device=audio.device)
    Jcap = max(ld.block_count(L, sample_rate), 1)
    z = torch.empty((B, Jcap), dtype=torch.float64, device=audio.device) if return_blocks else None
    L_ = lib()
    ws = _Workspace.get(L_.mt_loudness_workspace_bytes(B, L, hop), audio.device)
    check(L_.mt_loudness(ptr(audio), B, L, ptr(lens), (c_double * 10)(*coef.tolist()), hop, ld.ABS_GATE, ptr(z),
                         Jcap, ptr(nblocks), ptr(energy), ws.data_ptr(), ws.numel(), stream_handle(audio.device)),
          "loudness")
    return (energy, nblocks, z) if return_blocks else (energy, nblocks)


def true_peak(audio: torch.Tensor, lengths, plan4: ResamplePlan) -> torch.Tensor:
    """audio [B, L], lengths in samples (int [B], or None = L), plan4 = resample_plan(fs, 4 fs) -> fp32 [B]: the
    larger of each row's sample peak (mt_audio_stats) and of the peak of its 4x oversampled signal, which has the bits
    of resample(audio, plan4) and is never written (mt_true_peak)."""
    require_gpu(audio, what="true_peak")
    if (plan4.up, plan4.down) != (4, 1):
        raise ValueError(f"true_peak: the plan is {plan4.up}/{plan4.down}; the true peak is measured at 4/1")
    audio = f32c(audio)
    B, L = audio.shape
    lens = _lens32(lengths, B, audio.device)
    peak, _ = audio_stats(audio, lens)
    tpeak = torch.empty((B,), dtype=torch.float32, device=audio.device)
    L_ = lib()
    taps = plan4.taps if plan4.taps.device == audio.device else plan4.taps.to(audio.device)
    ws = _Workspace.get(L_.mt_true_peak_workspace_bytes(B, L), audio.device)
    check(L_.mt_true_peak(ptr(audio), B, L, ptr(lens), ptr(taps), plan4.half, ptr(peak), ptr(tpeak), ws.data_ptr(),
                          ws.numel(), stream_handle(audio.device)), "true_peak")
    return tpeak


# ---- look-ahead true-peak limiter (limiter.py is the specification) ------------------------------

# samples per workgroup of peak_envelope_kernel and of limit_kernel (mt_limiter.hip LM_ENV_T, LM_T) and the widest
# smoothing window (LM_MAX_W): tests put row ends and peaks around the tiles' edges
ENVELOPE_TILE = 512
LIMIT_TILE = 2048
LIMIT_MAX_WINDOW = 2048


def peak_envelope(audio: torch.Tensor, lengths, plan4: ResamplePlan) -> torch.Tensor:
    """audio [B, L], lengths in samples (int [B], or None = L), plan4 = resample_plan(fs, 4 fs) -> env fp32 [B, L]:
    limiter.envelope_ref of every row, zero from its length on (mt_peak_envelope). The 4x signal has the bits of
    true_peak's and is never written."""
    require_gpu(audio, what="peak_envelope")
    if (plan4.up, plan4.down) != (4, 1):
        raise ValueError(f"peak_envelope: the plan is {plan4.up}/{plan4.down}; the envelope is taken at 4/1")
    audio = f32c(audio)
    B, L = audio.shape
    lens = _lens32(lengths, B, audio.device)
    env = torch.empty((B, L), dtype=torch.float32, device=audio.device)
    L_ = lib()
    taps = plan4.taps if plan4.taps.device == audio.device else plan4.taps.to(audio.device)
    ws = _Workspace.get(L_.mt_peak_envelope_workspace_bytes(), audio.device)
    check(L_.mt_peak_envelope(ptr(audio), B, L, ptr(lens), ptr(taps), plan4.half, ptr(env), ws.data_ptr(), ws.numel(),
                              stream_handle(audio.device)), "peak_envelope")
    return env


def limit(audio: torch.Tensor, env: torch.Tensor, lengths, stats, level: float, ceiling: float, W: int,
          gain_in: Optional[torch.Tensor] = None):
    """audio, env [B, L] (env = peak_envelope(audio, ...)), lengths in samples, stats = (peak fp32 [B], meansq fp64
    [B]) on the device -> (y fp32 [B, L], gain fp32 [B], reduction fp32 [B]) (mt_limit): gain =
    float32(double(gain_in) level / sqrt(meansq)) (gain_in: fp32 [B], None = 1; unchanged where peak == 0 or meansq ==
    0), y = limiter.apply_ref(x, gain, limiter.gain_curve_ref(env, gain, float32(ceiling), W)), untouched rows (peak
    == 0) at s = 1, reduction = min s. ceiling: a linear amplitude, 10^(dBTP / 20); W: the window in samples."""
    require_gpu(audio, what="limit")
    level, ceiling, W = float(level), float(ceiling), int(W)
    if not (0.0 < level < float("inf")) or not (0.0 < ceiling < float("inf")):
        raise ValueError(f"limit: level {level} and ceiling {ceiling} must be finite and positive")
    if not 1 <= W <= LIMIT_MAX_WINDOW:
        raise ValueError(f"limit: window of {W} samples outside 1 .. {LIMIT_MAX_WINDOW}")
    audio, env = f32c(audio), f32c(env)
    if audio.dim() != 2 or env.shape != audio.shape:
        raise ValueError(f"limit: audio {tuple(audio.shape)} and env {tuple(env.shape)}, expected equal [B, L]")
    B, L = audio.shape
    lens = _lens32(lengths, B, audio.device)
    peak, meansq = stats
    if peak.shape != (B,) or peak.dtype != torch.float32 or meansq.shape != (B,) or meansq.dtype != torch.float64:
        raise ValueError(f"limit: stats are (peak fp32 [{B}], meansq fp64 [{B}])")
    if gain_in is not None and (gain_in.shape != (B,) or gain_in.dtype != torch.float32):
        raise ValueError(f"limit: gain_in is fp32 [{B}]")
    peak, meansq = peak.contiguous(), meansq.contiguous()
    gain_in = None if gain_in is None else gain_in.contiguous()
    y = torch.empty((B, L), dtype=torch.float32, device=audio.device)
    gain = torch.empty((B,), dtype=torch.float32, device=audio.device)
    reduction = torch.empty((B,), dtype=torch.float32, device=audio.device)
    L_ = lib()
    ws = _Workspace.get(L_.mt_limit_workspace_bytes(B, L, W), audio.device)
    check(L_.mt_limit(ptr(audio), ptr(env), B, L, ptr(lens), ptr(peak), ptr(meansq), ptr(gain_in), level, ceiling, W,
                      ptr(y), ptr(reduction), ptr(gain), ws.data_ptr(), ws.numel(), stream_handle(audio.device)),
          "limit")
    return y, gain, reduction


def _range_args(what: str, i_lo, cnt):
    i_lo, cnt = int(i_lo), int(cnt)
    if i_lo < 0 or cnt < 1 or i_lo + cnt >= (1 << 31) - 4 * LIMIT_TILE:
        raise ValueError(f"{what}: samples [{i_lo}, {i_lo} + {cnt})")
    return i_lo, cnt


def _inplace_rows(what: str, name: str, t: torch.Tensor, shape=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2 \
            or (shape is not None and t.shape != shape):
        raise ValueError(f"{what}: {name} is a contiguous fp32 [B, L] tensor" + (f" {tuple(shape)}" if shape else ""))
    return t


def peak_envelope_range(audio: torch.Tensor, lengths, plan4: ResamplePlan, i_lo: int, cnt: int,
                        env: torch.Tensor) -> torch.Tensor:
    """The samples [i_lo, i_lo + cnt) of ``peak_envelope``'s rows, written into `env` (fp32 [B, L], the same buffer
    across calls) where they lie inside the row, bit for bit; the rest of env keeps its contents
    (mt_peak_envelope_range). lengths: the rows' FINAL lengths in samples. Of a row it reads no sample past
    min(len - 1, i_lo + cnt - 1 + limiter.envelope_reach(plan4.half)): the rest of `audio` may still be unwritten
    (DESIGN.md §24). audio and env are fp32 and contiguous: read and written in place."""
    require_gpu(audio, what="peak_envelope_range")
    if (plan4.up, plan4.down) != (4, 1):
        raise ValueError(f"peak_envelope_range: the plan is {plan4.up}/{plan4.down}; the envelope is taken at 4/1")
    _inplace_rows("peak_envelope_range", "audio", audio)
    _inplace_rows("peak_envelope_range", "env", env, audio.shape)
    require_gpu(env, what="peak_envelope_range")
    i_lo, cnt = _range_args("peak_envelope_range", i_lo, cnt)
    B, L = audio.shape
    lens = _lens32(lengths, B, audio.device)
    L_ = lib()
    taps = plan4.taps if plan4.taps.device == audio.device else plan4.taps.to(audio.device)
    ws = _Workspace.get(L_.mt_peak_envelope_workspace_bytes(), audio.device)
    check(L_.mt_peak_envelope_range(ptr(audio), B, L, ptr(lens), ptr(taps), plan4.half, i_lo, cnt, ptr(env),
                                    ws.data_ptr(), ws.numel(), stream_handle(audio.device)), "peak_envelope_range")
    return env


def limit_range(audio: torch.Tensor, env: torch.Tensor, lengths, gain: torch.Tensor, ceiling: float, W: int,
                i_lo: int, cnt: int, reduction: torch.Tensor, out: Optional[torch.Tensor] = None):
    """The samples [i_lo, i_lo + cnt) of the limiter at a fixed gain -> (out fp32 [B, cnt], out_cnt int32 [B]): the
    bits of ``limit(audio, env, lengths, (ones, ones), 1.0, ceiling, W, gain_in=gain)``'s columns, i.e. of
    limiter.apply_ref(x, gain, limiter.gain_curve_ref(env, gain, float32(ceiling), W)), zero past a row's end
    (mt_limit_range). gain: fp32 [B] on the device, used as it is. Of env it reads [i_lo - (W - 1), i_lo + cnt + W -
    2] inside the row, of audio the range: the rest of both may still be unwritten. reduction (fp32 [B], device) is
    updated in place to min(reduction, min s over the range); start it at 1."""
    require_gpu(audio, what="limit_range")
    ceiling, W = float(ceiling), int(W)
    if not (0.0 < ceiling < float("inf")):
        raise ValueError(f"limit_range: ceiling {ceiling} must be finite and positive")
    if not 1 <= W <= LIMIT_MAX_WINDOW:
        raise ValueError(f"limit_range: window of {W} samples outside 1 .. {LIMIT_MAX_WINDOW}")
    _inplace_rows("limit_range", "audio", audio)
    _inplace_rows("limit_range", "env", env, audio.shape)
    i_lo, cnt = _range_args("limit_range", i_lo, cnt)
    B, L = audio.shape
    dev = audio.device
    for name, t in (("gain", gain), ("reduction", reduction)):
        if not isinstance(t, torch.Tensor) or t.shape != (B,) or t.dtype != torch.float32 or t.device != dev \
                or not t.is_contiguous():
            raise ValueError(f"limit_range: {name} is a contiguous fp32 [{B}] tensor on {dev}")
    if env.device != dev:
        raise ValueError(f"limit_range: env is on {env.device}, audio on {dev}")
    lens = _lens32(lengths, B, dev)
    if out is None:
        out = torch.empty((B, cnt), dtype=torch.float32, device=dev)
    elif out.shape != (B, cnt) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"limit_range: out {tuple(out.shape)}: expected contiguous fp32 ({B}, {cnt}) on {dev}")
    out_cnt = torch.empty((B,), dtype=torch.int32, device=dev)
    L_ = lib()
    ws = _Workspace.get(L_.mt_limit_range_workspace_bytes(B, cnt, W), dev)
    check(L_.mt_limit_range(ptr(audio), ptr(env), B, L, ptr(lens), ptr(gain), ceiling, W, i_lo, cnt, ptr(out),
                            ptr(out_cnt), ptr(reduction), ws.data_ptr(), ws.numel(), stream_handle(dev)),
          "limit_range")
    return out, out_cnt


def resample_range(audio: torch.Tensor, plan: ResamplePlan, lengths, lmul: int, m_lo: int, cnt: int,
                   out: Optional[torch.Tensor] = None):
    """The outputs [m_lo, m_lo + cnt) of ``resample``'s rows -> (out fp32 [B, cnt], out_cnt int32 [B]), bit for bit,
    zero past a row's own output count (mt_resample_range). Of a row it reads no sample past the one the chain of its
    last requested output starts at, so the rest of `audio` may still be unwritten (streaming delivery, DESIGN.md
    §20). audio must be fp32 and contiguous: it is read in place."""
    require_gpu(audio, what="resample_range")
    if audio.dtype != torch.float32 or not audio.is_contiguous() or audio.dim() != 2:
        raise ValueError("resample_range: audio is a contiguous fp32 [B, L] tensor")
    B, L = audio.shape
    m_lo, cnt = int(m_lo), int(cnt)
    if m_lo < 0 or cnt < 1:
        raise ValueError(f"resample_range: outputs [{m_lo}, {m_lo} + {cnt})")
    lens = _lens32(lengths, B, audio.device)
    if out is None:
        out = torch.empty((B, cnt), dtype=torch.float32, device=audio.device)
    elif out.shape != (B, cnt) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"resample_range: out {tuple(out.shape)}: expected contiguous fp32 ({B}, {cnt})")
    out_cnt = torch.empty((B,), dtype=torch.int32, device=audio.device)
    L_ = lib()
    taps = plan.taps if plan.taps.device == audio.device else plan.taps.to(audio.device)
    ws = _Workspace.get(L_.mt_resample_workspace_bytes(plan.half, plan.up, plan.down), audio.device)
    check(L_.mt_resample_range(ptr(audio), B, L, ptr(lens), int(lmul), ptr(taps), plan.half, plan.up, plan.down, m_lo,
                               cnt, ptr(out), ptr(out_cnt), ws.data_ptr(), ws.numel(), stream_handle(audio.device)),
          "resample_range")
    return out, out_cnt


def _table(t: torch.Tensor, R: int, device, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.device != device or t.shape != (R,) \
            or not t.is_contiguous():
        raise ValueError(f"{name}: a contiguous int32 [{R}] tensor on {device} expected")
    return t


def window_gather(src: torch.Tensor, row_src: torch.Tensor, row_start: torch.Tensor, row_len: torch.Tensor, W: int,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """src fp32 [Bs, C, Ls] or [Bs, Ls] -> rows [R, C, W] / [R, W]: rows[r, c, w] = src[row_src[r], c, row_start[r] +
    w] for w < row_len[r], else 0 (mt_window_gather). The tables are int32 [R] on src's device; src is read in
    place (contiguous fp32). R <= RAGGED_MAX_BATCH."""
    require_gpu(src, what="window_gather")
    if src.dtype != torch.float32 or not src.is_contiguous() or src.dim() not in (2, 3):
        raise ValueError("window_gather: src is a contiguous fp32 [B, C, L] or [B, L] tensor")
    Bs, Ls = src.shape[0], src.shape[-1]
    C = src.shape[1] if src.dim() == 3 else 1
    R, W = int(row_src.shape[0]), int(W)
    if not (1 <= R <= RAGGED_MAX_BATCH) or W < 1:
        raise ValueError(f"window_gather: {R} rows (1..{RAGGED_MAX_BATCH}) of {W}")
    tabs = [_table(t, R, src.device, "window_gather") for t in (row_src, row_start, row_len)]
    shape = (R, C, W) if src.dim() == 3 else (R, W)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=src.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError(f"window_gather: out {tuple(out.shape)}: expected contiguous fp32 {shape}")
    check(lib().mt_window_gather(ptr(src), Bs, C, Ls, ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), R, W, ptr(out),
                                 stream_handle(src.device)), "window_gather")
    return out


def window_scatter(rows: torch.Tensor, row_dst: torch.Tensor, crop_from: torch.Tensor, dst_start: torch.Tensor,
                   crop_len: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    """dst[row_dst[r], dst_start[r] + i] = rows[r, crop_from[r] + i] for i < crop_len[r] (mt_window_scatter): rows
    fp32 [R, W] (or [R, 1, W]), dst fp32 [Bd, Ld], both contiguous; the tables int32 [R] on their device."""
    require_gpu(rows, dst, what="window_scatter")
    if rows.dim() == 3 and rows.shape[1] == 1:
        rows = rows[:, 0]
    for t, name in ((rows, "rows"), (dst, "dst")):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2:
            raise ValueError(f"window_scatter: {name} is a contiguous fp32 2-D tensor")
    R, W = rows.shape
    if not (1 <= R <= RAGGED_MAX_BATCH):
        raise ValueError(f"window_scatter: {R} rows (1..{RAGGED_MAX_BATCH})")
    tabs = [_table(t, R, dst.device, "window_scatter") for t in (row_dst, crop_from, dst_start, crop_len)]
    check(lib().mt_window_scatter(ptr(rows), R, W, ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), ptr(tabs[3]), ptr(dst),
                                  dst.shape[0], dst.shape[1], stream_handle(dst.device)), "window_scatter")
    return dst


# ---- long-form synthesis: trim edges, placement, join (join.py is the specification) ------------

# samples per workgroup of edges_tile_kernel (ED_TILE), segments per scan step of join_plan_kernel (JP_CHUNK) and
# document samples per workgroup of join_kernel (JN_TILE), all in mt_join.hip: tests put lengths around their multiples
EDGES_TILE = 4096
JOIN_PLAN_CHUNK = 256
JOIN_TILE = 1024
JOIN_MAX_ROWS = 65535

_RAMPS: Dict[tuple, torch.Tensor] = {}


def _ramp_table(fade: int, device) -> Optional[torch.Tensor]:
    """join.ramp(fade) on the device, cached per (fade, device): built on the host, as the resampler's taps are"""
    from . import join as jn
    table = jn.ramp(fade)  # ValueError for a fade the kernel does not take
    if fade == 0:
        return None
    key = (int(fade), device.index)
    t = _RAMPS.get(key)
    if t is None:
        t = _RAMPS[key] = torch.from_numpy(table).to(device)
    return t


def audio_edges(audio: torch.Tensor, lengths, thr: float, pad: int):
    """audio [S, L], lengths in samples (int [S], or None = L) -> (start, end) int32 [S]: join.edges_ref of every
    row (mt_audio_edges). audio is read in place when it is contiguous fp32."""
    require_gpu(audio, what="audio_edges")
    thr, pad = float(thr), int(pad)
    if not (math.isfinite(thr) and thr >= 0.0) or pad < 0:
        raise ValueError(f"audio_edges: thr {thr} (finite, >= 0), pad {pad} (>= 0)")
    audio = f32c(audio)
    if audio.dim() != 2:
        raise ValueError(f"audio_edges: audio {tuple(audio.shape)}, expected [S, L]")
    S, L = audio.shape
    lens = _lens32(lengths, S, audio.device)
    start = torch.empty((S,), dtype=torch.int32, device=audio.device)
    end = torch.empty((S,), dtype=torch.int32, device=audio.device)
    L_ = lib()
    ws = _Workspace.get(L_.mt_audio_edges_workspace_bytes(S, L), audio.device)
    check(L_.mt_audio_edges(ptr(audio), S, L, ptr(lens), thr, pad, ptr(start), ptr(end), ws.data_ptr(), ws.numel(),
                            stream_handle(audio.device)), "audio_edges")
    return start, end


def join_plan(doc_first: torch.Tensor, start: torch.Tensor, end: torch.Tensor, gap: torch.Tensor, head: int,
              tail: int, L: int, Lcap: int = 1 << 30):
    """doc_first int32 [D + 1] (CSR), start / end / gap int32 [S], all on the device -> (dst int32 [S], doc_len
    int32 [D], bad int32 [1]): join.plan_ref (mt_join_plan). Nothing comes back to the host."""
    require_gpu(doc_first, start, end, gap, what="join_plan")
    head, tail, L, Lcap = int(head), int(tail), int(L), int(Lcap)
    if head < 0 or tail < 0:
        raise ValueError(f"join_plan: head {head} and tail {tail} are sample counts >= 0")
    S, D = int(start.shape[0]), int(doc_first.shape[0]) - 1
    if not (1 <= S <= JOIN_MAX_ROWS and 1 <= D <= JOIN_MAX_ROWS):
        raise ValueError(f"join_plan: {S} segments in {D} documents (1..{JOIN_MAX_ROWS} each)")
    dev = start.device
    _table(doc_first, D + 1, dev, "join_plan: doc_first")
    for t in (start, end, gap):
        _table(t, S, dev, "join_plan")
    dst = torch.zeros((S,), dtype=torch.int32, device=dev)
    doc_len = torch.empty((max(D, 0),), dtype=torch.int32, device=dev)
    bad = torch.empty((1,), dtype=torch.int32, device=dev)
    check(lib().mt_join_plan(ptr(doc_first), D, ptr(start), ptr(end), ptr(gap), S, L, head, tail, Lcap, ptr(dst),
                             ptr(doc_len), ptr(bad), stream_handle(dev)), "join_plan")
    return dst, doc_len, bad


def join(seg: torch.Tensor, start: torch.Tensor, end: torch.Tensor, doc_first: torch.Tensor, dst: torch.Tensor,
         doc_len: torch.Tensor, fade: int, bad: Optional[torch.Tensor] = None, Ld: Optional[int] = None):
    """seg fp32 [S, L] (read in place), the tables of audio_edges / join_plan -> out fp32 [D, Ld]: join.join_ref
    (mt_join). Ld = max(doc_len) (at least 1) unless given; it and join_plan's `bad` flag come to the host in one
    device -> host copy, the one synchronisation of the chain. ValueError when `bad` is set (a document longer than
    join_plan's Lcap)."""
    require_gpu(seg, what="join")
    if seg.dtype != torch.float32 or not seg.is_contiguous() or seg.dim() != 2:
        raise ValueError("join: seg is a contiguous fp32 [S, L] tensor")
    S, L = seg.shape
    D = int(doc_first.shape[0]) - 1
    if not (1 <= S <= JOIN_MAX_ROWS and 1 <= D <= JOIN_MAX_ROWS):
        raise ValueError(f"join: {S} segments in {D} documents (1..{JOIN_MAX_ROWS} each)")
    dev = seg.device
    fade = int(fade)
    table = _ramp_table(fade, dev)
    _table(doc_first, D + 1, dev, "join: doc_first")
    for t in (start, end, dst):
        _table(t, S, dev, "join")
    _table(doc_len, D, dev, "join: doc_len")
    if bad is not None or Ld is None:
        flag = torch.zeros((1,), dtype=torch.int32, device=dev) if bad is None else bad.reshape(1)
        longest, is_bad = torch.cat([doc_len.max().reshape(1), flag]).cpu().tolist()
        if is_bad:
            raise ValueError("join: a document is longer than the plan's Lcap samples")
        Ld = max(int(longest), 1) if Ld is None else int(Ld)
    out = torch.empty((D, int(Ld)), dtype=torch.float32, device=dev)
    check(lib().mt_join(ptr(seg), S, L, ptr(start), ptr(end), ptr(doc_first), D, ptr(dst), ptr(doc_len), ptr(table),
                        fade, ptr(out), int(Ld), stream_handle(dev)), "join")
    return out


def maximum_path(neg_cent: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """train_standalone.py:280-325 on the GPU: neg_cent [B,Tx,Ty], attention mask [B,Tx,Ty] (x_mask x
    y_mask) -> one-hot monotonic path [B,Tx,Ty] in neg_cent's dtype. The lengths are the mask's row /
    column counts at index 0, as the reference takes them."""
    require_gpu(neg_cent, mask, what="maximum_path")
    B, Tx, Ty = neg_cent.shape
    value = f32c(neg_cent.detach())
    t_xs = mask.detach().sum(dim=1)[:, 0].to(torch.int32).contiguous()
    t_ys = mask.detach().sum(dim=2)[:, 0].to(torch.int32).contiguous()
    out = torch.empty((B, Tx, Ty), dtype=torch.float32, device=neg_cent.device)
    L_ = lib()
    ws = _Workspace.get(L_.mt_maximum_path_workspace_bytes(B, Tx, Ty), neg_cent.device)
    check(L_.mt_maximum_path(ptr(value), ptr(t_xs), ptr(t_ys), B, Tx, Ty, ptr(out), ws.data_ptr(), ws.numel(),
                             stream_handle(neg_cent.device)), "maximum_path")
    return out.to(neg_cent.dtype)


def align(mu: torch.Tensor, y: torch.Tensor, x_lengths, y_lengths, mean=None, std=None, want_attn: bool = False,
          want_log_prior: bool = False):
    """Forced aligner (mt_align): mu [B,C,Tx] (the text encoder's), y [B,C,Ty] (a mel), token / frame counts [B] ->
    (durations int64 [B,Tx], attn [B,Tx,Ty] | None, log_prior [B,Tx,Ty] | None). mean / std (a number or [C]): y is
    a denormalized mel and is normalized first; None: y is normalized already. The log-prior is the direct form
    -0.5 sum_c (y - mu)^2 - 0.5 C log(2 pi) in fp32 and the search the textbook MAS (Glow-TTS), not the trainer's
    `maximum_path`. A row with y_lengths < x_lengths or no tokens gets all-zero durations."""
    require_gpu(mu, y, what="align")
    mu, y = f32c(mu), f32c(y)
    B, C, Tx = mu.shape
    if y.dim() != 3 or y.shape[0] != B or y.shape[1] != C:
        raise ValueError(f"align: y {tuple(y.shape)} does not match mu {tuple(mu.shape)}")
    Ty = y.shape[2]
    dev = mu.device
    t_xs = torch.as_tensor(x_lengths).detach().to(device=dev, dtype=torch.int32).contiguous()
    t_ys = torch.as_tensor(y_lengths).detach().to(device=dev, dtype=torch.int32).contiguous()
    if t_xs.shape != (B,) or t_ys.shape != (B,):
        raise ValueError(f"align: x_lengths {tuple(t_xs.shape)} / y_lengths {tuple(t_ys.shape)}: expected ({B},)")
    if (mean is None) != (std is None):
        raise ValueError("align: mean and std go together")
    if mean is not None:
        mean = f32c(torch.as_tensor(mean).to(dev)).reshape(-1).expand(C).contiguous()
        std = f32c(torch.as_tensor(std).to(dev)).reshape(-1).expand(C).contiguous()
    dur = torch.empty((B, Tx), dtype=torch.int64, device=dev)
    attn = torch.empty((B, Tx, Ty), dtype=torch.float32, device=dev) if want_attn else None
    lp = torch.empty((B, Tx, Ty), dtype=torch.float32, device=dev) if want_log_prior else None
    L_ = lib()
    ws = _Workspace.get(L_.mt_align_workspace_bytes(B, C, Tx, Ty), dev)
    check(L_.mt_align(ptr(mu), ptr(y), ptr(mean), ptr(std), ptr(t_xs), ptr(t_ys), B, C, Tx, Ty, ptr(dur), ptr(lp),
                      ptr(attn), ws.data_ptr(), ws.numel(), stream_handle(dev)), "align")
    return dur, attn, lp


def op_conv1d(x_btc: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], stride=1, pad=0, dil=1,
              transposed=False, slope: Optional[float] = None, precision="fp32", variant: int = -1,
              out: Optional[torch.Tensor] = None, ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Op-level test entry: y = conv(lrelu(x)) on [B,T,C] activations (dtype by precision)."""
    require_gpu(x_btc, what="op_conv1d")
    dt = dtype_code(precision)
    et = torch.bfloat16 if dt == DTYPE_BF16 else torch.float32
    x = x_btc.to(et).contiguous()
    B, Tin, cin = x.shape
    if transposed:
        cout, k = W.shape[1], W.shape[2]
        tout = (Tin - 1) * stride - 2 * pad + k
    else:
        cout, k = W.shape[0], W.shape[2]
        tout = (Tin + 2 * pad - dil * (k - 1) - 1) // stride + 1
    y = torch.empty((B, tout, cout), dtype=et, device=x.device) if out is None else out
    L = lib()
    nb = L.mt_op_conv1d_workspace_bytes(dt, cin, cout, k, stride, int(transposed))
    if ws is None or ws.numel() < nb:
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    W, bias = f32c(W), f32c(bias)
    check(L.mt_op_conv1d_tile(int(variant), dt, ptr(x), B, Tin, cin, ptr(W), ptr(bias), cout, k, stride, pad, dil,
                              int(transposed), -1.0 if slope is None else float(slope), ptr(y), tout, ws.data_ptr(),
                              ws.numel(), stream_handle(x.device)), "op_conv1d")
    return y


def op_vconv(x_btc: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, dil: int = 1, ef: int = 0,
             resid: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None, y2: Optional[torch.Tensor] = None,
             slope: float = 0.1, div: float = 1.0, ws: Optional[torch.Tensor] = None, pack: bool = True,
             lens: Optional[torch.Tensor] = None):
    """Op-level test entry of mt_vconv: one "same"-padded bf16 Conv1d on an already activated
    [B,L,C] input with the ResBlock epilogues (ef bits: 1 resid, 2 accumulate into y, 4 /div,
    8 y=lrelu(v), 16 also y2=lrelu(v)); lens (int32 [B] on the device): a ragged batch. Returns (y, y2)."""
    require_gpu(x_btc, what="op_vconv")
    x = x_btc.to(torch.bfloat16).contiguous()
    B, L, cin = x.shape
    cout, k = W.shape[0], W.shape[2]
    if y is None:
        y = torch.empty((B, L, cout), dtype=torch.bfloat16, device=x.device)
    if (ef & 16) and y2 is None:
        y2 = torch.empty((B, L, cout), dtype=torch.bfloat16, device=x.device)
    if resid is not None:
        resid = resid.to(torch.bfloat16).contiguous()
    L_ = lib()
    nb = L_.mt_op_vconv_workspace_bytes(cin, cout, k)
    if ws is None or ws.numel() < nb:
        if not pack:
            raise ValueError("op_vconv: pack=False needs the workspace a packing call filled")
        ws = torch.empty(nb, dtype=torch.uint8, device=x.device)
    W, bias = f32c(W), f32c(bias)
    if lens is not None:
        lens = lens.to(device=x.device, dtype=torch.int32).contiguous()
    check(L_.mt_op_vconv(ptr(x), B, L, cin, ptr(W), ptr(bias), cout, k, dil, int(ef), ptr(resid), ptr(y), ptr(y2),
                         float(slope), float(div), ptr(lens), int(bool(pack)), ws.data_ptr(), ws.numel(),
                         stream_handle(x.device)), "op_vconv")
    return y, y2


def set_vconv_ct(enable: bool) -> bool:
    """mt_vconv's compile-time K loop for the decoder's / upsamplers' convs (True, default) or the runtime-cursor
    loop; returns the previous setting (process-wide)"""
    return bool(lib().mt_vconv_set_ct(int(bool(enable))))


def set_vpair_kernels(mask: int) -> int:
    """the round-5 ResBlock pair kernels (bit 0: the 64-channel k = 7 / 11 compile-time K loop; default 1), each
    bit-identical to the kernel it replaces; returns the previous mask (process-wide)"""
    return int(lib().mt_vpair_set_kernels(int(mask)))


def set_post_fold(enable) -> int:
    """conv_post in the last ResBlock pair's epilogue (1, default) or its own launch (0); bit-identical; returns the
    previous setting (process-wide)"""
    return int(lib().mt_vocoder_set_post_fold(int(bool(enable))))


def set_ffn(mode) -> int:
    """the bf16 decoder's transformer FeedForward as one fused launch (mt_ffn; 3, the default: serial schedule with the
    frame fragments prefetched; 1: serial, weight and frame fragments prefetched; 2: FF1 epilogues overlapped with FF2
    steps) or as two mt_vconv GEMMs (False / 0); returns the previous setting (process-wide)"""
    return int(lib().mt_ffn_set(int(mode)))


def set_ffn_min_frames(frames: int) -> int:
    """the fused FeedForward only on decoder levels of at least `frames` frames (B x T; default 16384); returns the
    previous value (process-wide)"""
    return int(lib().mt_ffn_set_min_frames(int(frames)))


def set_decoder_kernels(mask: int) -> int:
    """the decoder kernel variants (bit 0: the dedicated final projection + ODE update kernel; bit 1: the
    query-independent attention's o_b computed once per solve instead of once per evaluation; bits 2 / 3, values
    4 / 8: write-through output stores at level 0 / level 1; default 15), each bit-identical to what it replaces;
    returns the previous mask (process-wide)"""
    return int(lib().mt_decoder_set_kernels(int(mask)))


def set_rbconv_actin(enable: bool) -> bool:
    """the stage 1-2 ResBlock conv1s activate the raw chain state in LDS (True, default: no activated copies stored)
    or read the activated copies their producers store; returns the previous setting (process-wide)"""
    return bool(lib().mt_vconv_set_actin(int(bool(enable))))


def set_rbconv(enable: bool) -> bool:
    """the HiFi-GAN wide-stage ResBlock convs on mt_rbconv (True, default) or the generic mt_vconv kernel; returns
    the previous setting (process-wide)"""
    return bool(lib().mt_vconv_set_rbconv(int(bool(enable))))


def op_attention(qkv: torch.Tensor, mask: torch.Tensor, heads: int, precision="fp32") -> torch.Tensor:
    require_gpu(qkv, mask, what="op_attention")
    dt = dtype_code(precision)
    et = torch.bfloat16 if dt == DTYPE_BF16 else torch.float32
    qkv = qkv.to(et).contiguous()
    B, T, _ = qkv.shape
    out = torch.empty((B, T, heads * 64), dtype=et, device=qkv.device)
    mask = f32c(mask.reshape(B, T))
    check(lib().mt_op_attention(dt, ptr(qkv), ptr(mask), ptr(out), B, T, heads, stream_handle(qkv.device)),
          "op_attention")
    return out


# ---------------------------------------------------------------------------------- launch probe
PROBE_RBFUSE_C64, PROBE_RBFUSE_C32, PROBE_VCONV, PROBE_VCONV_DEC = 1, 2, 3, 4


def probe_start(site: int, max_launches: int) -> None:
    """Arm HIP events around every launch of one kernel site (see mt_probe_start)."""
    check(lib().mt_probe_start(int(site), int(max_launches)), "probe_start")


def probe_pause(paused: bool) -> None:
    """Stop (True) / resume (False) recording without disarming (see mt_probe_pause)."""
    check(lib().mt_probe_pause(int(bool(paused))), "probe_pause")


PROBE_TAGS = ("vconv", "vpair", "vpair32", "rbfuse", "vpair128", "rbconv")


def probe_detail(cap: int = 4096) -> List[Dict[str, float]]:
    """Per recorded launch (before probe_stop): ms, algorithmic flops / bytes and the kernel kind."""
    from ctypes import c_double
    ms, fl, by, tg = (c_double * cap)(), (c_double * cap)(), (c_double * cap)(), (c_int * cap)()
    n = lib().mt_probe_detail(int(cap), ms, fl, by, tg)
    if n < 0:
        check(n, "probe_detail")
    return [{"ms": ms[i], "flops": fl[i], "bytes": by[i], "kind": PROBE_TAGS[tg[i]]} for i in range(n)]


def probe_stop(peak_flops: float = 2.5e15, peak_bw: float = 8.0e12) -> Dict[str, float]:
    """Synchronize the probe's events: launches, summed kernel ms, algorithmic FLOPs and layer-boundary
    bytes, and the summed per-launch roofline time max(F / peak_flops, B / peak_bw) in ms (defaults: the
    MI355X dense bf16 MFMA and HBM peaks of MI355X_MICROARCH.md)."""
    from ctypes import c_double
    n, ms, fl, by, roof = c_int(0), c_double(0), c_double(0), c_double(0), c_double(0)
    check(lib().mt_probe_stop(byref(n), byref(ms), byref(fl), byref(by), float(peak_flops), float(peak_bw),
                              byref(roof)), "probe_stop")
    return {"launches": n.value, "ms": ms.value, "flops": fl.value, "bytes": by.value, "roof_ms": roof.value}


VCONV_LOG_FIELDS = ("ef", "bm", "bn", "k1", "ntiles", "grid", "taps", "M", "cin", "B", "L")
# "ef" of the launches that are not mt_vconv's: a tag instead of epilogue flags. PROJ_LOG proj_euler_kernel. Only
# after vconv_log_select(LOG_CONV | LOG_AUX): the query-independent attention's three launches (attn_uni_part_kernel,
# attn_uni_vec_kernel, attn_uni_apply_kernel; grid in "grid", utterances in "B", frames per utterance in "L") and
# FFN_LOG the fused FeedForward (k1 = 1: it adds o_b itself)
PROJ_LOG = 0x20000
INFILL_LOG = 0x1000000  # infill_clamp_kernel (mt_cfm_solve_infill): "B" the rows it ran on, "L" the frames per row
UNI_LOG_PART, UNI_LOG_VEC, UNI_LOG_APPLY = 0x40000, 0x80000, 0xC0000
FFN_LOG = 0x400000
LOG_CONV, LOG_AUX = 1, 2


def vconv_log_select(families: int) -> int:
    """which launches the log records: LOG_CONV the conv launches (always), LOG_AUX also the decoder's uniform-attention
    and fused-FeedForward launches (off by default); returns the previous selection (process-wide)"""
    return int(lib().mt_vconv_log_select(int(families)))


def vconv_log_start(capacity: int = 65536) -> None:
    """Record the variant and grid of every mt_vconv launch from now on (test coverage)."""
    check(lib().mt_vconv_log_start(int(capacity)), "vconv_log_start")


def vconv_log_stop(capacity: int = 65536) -> List[Dict[str, int]]:
    """Disarm the launch log; one dict per launch (fields VCONV_LOG_FIELDS)."""
    buf = (c_int * (capacity * len(VCONV_LOG_FIELDS)))()
    n = lib().mt_vconv_log_stop(buf, int(capacity))
    k = len(VCONV_LOG_FIELDS)
    return [dict(zip(VCONV_LOG_FIELDS, buf[i * k:(i + 1) * k])) for i in range(n)]
