"""Transformer ops (LayerNorm, BERT embeddings, fused attention, ViT tokens): packed-parameter
types, native launch-parameter builders, eager wrappers and fp32 PyTorch oracles."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from .. import _native as N

K_LAYERNORM, K_EMBED, K_ATTENTION, K_VIT_TOKENS = N.HZ_K_LAYERNORM, N.HZ_K_EMBED, N.HZ_K_ATTENTION, N.HZ_K_VIT_TOKENS
K_SOFTMAX, K_QKVATT = N.HZ_K_SOFTMAX, N.HZ_K_QKVATT


@N.params_of("HZ_K_SOFTMAX")
class SoftmaxParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("mask", C.c_void_p), ("out", C.c_void_p), ("rows", C.c_int), ("D", C.c_int),
                ("ldx", C.c_int), ("ldo", C.c_int), ("x_bf16", C.c_int), ("scale", C.c_float)]


@N.params_of("HZ_K_LAYERNORM")
class LayerNormParams(C.Structure):
    _fields_ = [("x", C.c_void_p), ("res", C.c_void_p), ("out", C.c_void_p), ("gamma", C.c_void_p),
                ("beta", C.c_void_p), ("rows", C.c_int), ("D", C.c_int), ("ldx", C.c_int), ("ldr", C.c_int),
                ("ldo", C.c_int), ("eps", C.c_float), ("out8", C.c_void_p), ("scale8", C.c_void_p)]


@N.params_of("HZ_K_EMBED")
class EmbedParams(C.Structure):
    _fields_ = [("ids", C.c_void_p), ("types", C.c_void_p), ("word", C.c_void_p), ("pos", C.c_void_p),
                ("type", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p), ("out", C.c_void_p),
                ("rows", C.c_int), ("L", C.c_int), ("D", C.c_int), ("eps", C.c_float),
                ("vocab", C.c_int), ("ntypes", C.c_int)]


@N.params_of("HZ_K_ATTENTION")
class AttentionParams(C.Structure):
    _fields_ = [("qkv", C.c_void_p), ("mask", C.c_void_p), ("out", C.c_void_p), ("B", C.c_int), ("L", C.c_int),
                ("heads", C.c_int), ("head_dim", C.c_int), ("ldqkv", C.c_int), ("k_off", C.c_int),
                ("v_off", C.c_int), ("ldo", C.c_int), ("scale", C.c_float), ("out8", C.c_void_p),
                ("os8", C.c_void_p)]


@N.params_of("HZ_K_QKVATT")
class QkvAttParams(C.Structure):  # HzQkvAttParams: QKV projection + attention in one launch
    _fields_ = [("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("mask", C.c_void_p), ("out", C.c_void_p),
                ("B", C.c_int), ("L", C.c_int), ("heads", C.c_int), ("D", C.c_int), ("ksteps", C.c_int),
                ("ldx", C.c_int), ("ldo", C.c_int), ("scale", C.c_float)]


@N.params_of("HZ_K_VIT_TOKENS")
class VitTokensParams(C.Structure):
    _fields_ = [("patches", C.c_void_p), ("cls", C.c_void_p), ("pos", C.c_void_p), ("out", C.c_void_p),
                ("B", C.c_int), ("np", C.c_int), ("D", C.c_int)]


@N.params_of("HZ_K_POOL_EMBED")
class PoolEmbedParams(C.Structure):  # HzPoolEmbedParams: CLS row / masked token mean (+ L2 norm) per sequence
    _fields_ = [("x", C.c_void_p), ("mask", C.c_void_p), ("out", C.c_void_p), ("B", C.c_int), ("L", C.c_int),
                ("D", C.c_int), ("ldx", C.c_int), ("ldo", C.c_int), ("first", C.c_int), ("mode", C.c_int),
                ("normalize", C.c_int)]


POOL_MODES = {"cls": 0, "mean": 1}  # HzPoolEmbedParams.mode


def launch(kind: int, prm, stream=None):
    N.check(N.lib().hz_launch_kernel(kind, C.byref(prm), N.stream_ptr(stream)), f"kernel {kind}")


@dataclass
class NormParams:
    gamma: torch.Tensor  # fp32 [D]
    beta: torch.Tensor   # fp32 [D]
    eps: float = 1e-12

    def to(self, device):
        return NormParams(self.gamma.to(device), self.beta.to(device), self.eps)


@dataclass
class EmbedTables:
    word: torch.Tensor   # bf16 [V, D]
    pos: torch.Tensor    # bf16 [Lmax, D]
    type: torch.Tensor   # bf16 [T, D]


def norm_from(sd, prefix, eps) -> NormParams:
    return NormParams(sd[f"{prefix}.weight"].float().contiguous(), sd[f"{prefix}.bias"].float().contiguous(), eps)


# ----------------------------------------------------------------------------- eager
def layernorm(x: torch.Tensor, np_: NormParams, residual: torch.Tensor | None = None, out=None) -> torch.Tensor:
    rows, D = x.shape
    out = out if out is not None else torch.empty_like(x)
    prm = LayerNormParams(x.data_ptr(), N.ptr(residual), out.data_ptr(), np_.gamma.data_ptr(), np_.beta.data_ptr(),
                          rows, D, x.stride(0), residual.stride(0) if residual is not None else 0, out.stride(0),
                          np_.eps)
    launch(K_LAYERNORM, prm)
    return out


def layernorm_q8(x: torch.Tensor, np_: NormParams, residual: torch.Tensor | None = None, keep_bf16: bool = False):
    """LayerNorm with the per-row fp8 quantisation of its output fused in:
    returns (x8 uint8 [rows, D], row scales fp32 [rows]) and, with ``keep_bf16``, the bf16 output."""
    rows, D = x.shape
    out = torch.empty_like(x) if keep_bf16 else None
    x8 = torch.empty(rows, D, dtype=torch.uint8, device=x.device)
    sx = torch.empty(rows, dtype=torch.float32, device=x.device)
    prm = LayerNormParams(x.data_ptr(), N.ptr(residual), N.ptr(out), np_.gamma.data_ptr(), np_.beta.data_ptr(),
                          rows, D, x.stride(0), residual.stride(0) if residual is not None else 0, D, np_.eps,
                          x8.data_ptr(), sx.data_ptr())
    launch(K_LAYERNORM, prm)
    return (x8, sx, out) if keep_bf16 else (x8, sx)


def softmax(x: torch.Tensor, cols: int | None = None, scale: float = 1.0, mask: torch.Tensor | None = None,
            out: torch.Tensor | None = None) -> torch.Tensor:
    """Row softmax over the first ``cols`` columns of a 2-D fp32/bf16 tensor -> fp32."""
    rows, ld = x.shape
    D = cols or ld
    assert x.dtype in (torch.float32, torch.bfloat16) and x.stride(1) == 1
    out = out if out is not None else torch.empty(rows, D, device=x.device, dtype=torch.float32)
    prm = SoftmaxParams(x.data_ptr(), N.ptr(mask), out.data_ptr(), rows, D, x.stride(0), out.stride(0),
                        int(x.dtype == torch.bfloat16), scale)
    launch(K_SOFTMAX, prm)
    return out


def softmax_ref(x: torch.Tensor, cols: int | None = None, scale: float = 1.0, mask=None,
                dtype=torch.float32) -> torch.Tensor:
    D = cols or x.shape[-1]
    v = x[..., :D].to(dtype) * scale
    if mask is not None:
        v = v + mask.to(dtype)
    return torch.softmax(v, dim=-1)


def attention(qkv: torch.Tensor, B: int, L: int, heads: int, mask: torch.Tensor | None = None,
              out: torch.Tensor | None = None) -> torch.Tensor:
    """softmax(Q K^T / 8 + mask) V for any L >= 1: the one-pass kernel up to L = 256, the streamed
    (online-softmax) kernel beyond, or for every L with ``HIPZAP_ATT_STREAM=1``."""
    D = heads * 64
    out = out if out is not None else torch.empty(B * L, D, dtype=torch.bfloat16, device=qkv.device)
    prm = AttentionParams(qkv.data_ptr(), N.ptr(mask), out.data_ptr(), B, L, heads, 64, qkv.stride(0), D, 2 * D,
                          out.stride(0), 1.0 / 8.0)
    launch(K_ATTENTION, prm)
    return out


def pool_embed(x: torch.Tensor, B: int, L: int, mask: torch.Tensor | None = None, mode: str = "mean",
               first: int = 0, normalize: bool = True, D: int | None = None,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """One fp32 vector per sequence from the hidden states ``x`` (bf16 ``[B*L, ldx]``, ``D`` columns
    used): the CLS row (``mode="cls"``) or the mean of the tokens of ``[first, L)`` whose additive
    ``mask`` value is 0, optionally divided by its L2 norm. ``out``: fp32 ``[B, ldo]``, columns past
    ``D`` are zeroed. A shape the kernel does not take raises."""
    assert x.dtype == torch.bfloat16 and x.stride(1) == 1
    D = D if D is not None else x.shape[1]
    out = out if out is not None else torch.empty(B, D, dtype=torch.float32, device=x.device)
    prm = PoolEmbedParams(x.data_ptr(), N.ptr(mask), out.data_ptr(), B, L, D, x.stride(0), out.stride(0),
                          first, POOL_MODES[mode], int(bool(normalize)))
    launch(N.HZ_K_POOL_EMBED, prm)
    return out


# ----------------------------------------------------------------------------- oracles
def pool_embed_ref(x, B: int, L: int, mask=None, mode: str = "mean", first: int = 0,
                   normalize: bool = True) -> torch.Tensor:
    """fp64 on the CPU: ``x`` ``[B*L, D]`` (any float dtype) -> ``[B, D]``. ``mean``: the sum of
    the counted tokens over their number (a token of ``[first, L)`` counts iff its additive mask
    value is 0; no counted token: zeros); ``cls``: row 0 of each sequence. ``normalize``: divided
    by ``max(||v||_2, 1e-12)`` (``F.normalize``)."""
    x = x.detach().to("cpu", torch.float64).reshape(B, L, -1)
    if POOL_MODES[mode] == 0:
        v = x[:, 0]
    else:
        on = torch.ones(B, L, dtype=torch.float64) if mask is None else \
            (mask.detach().to("cpu", torch.float64).reshape(B, L) == 0).double()
        on[:, :first] = 0
        cnt = on.sum(1, keepdim=True)
        v = (x * on[:, :, None]).sum(1) / cnt.clamp(min=1.0)
    if normalize:
        v = v / v.norm(dim=1, keepdim=True).clamp(min=1e-12)
    return v


def layernorm_ref(x, np_: NormParams, residual=None):
    x = x.float() + (residual.float() if residual is not None else 0)
    return F.layer_norm(x, (x.shape[-1],), np_.gamma.float(), np_.beta.float(), np_.eps)


def attention_ref(qkv, B, L, heads, mask=None):
    D = heads * 64
    q, k, v = qkv.float().reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0
    if mask is not None:
        s = s + mask.float().reshape(B, 1, 1, L)
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * L, D)


def attention_stream_ref(qkv, B, L, heads, mask=None, tile: int = 64):
    """CPU emulation of ``attention_stream_kernel``'s arithmetic (csrc/transformer.hip), not an
    oracle: the keys are walked in tiles of ``tile`` with a running max ``m`` and running sum ``l``
    per query; each tile's ``p = exp(s - m)`` is summed into ``l`` in fp32 and rounded to bf16
    UNNORMALISED for the fp32-accumulated P.V; the accumulators are rescaled by
    ``exp(m_old - m_new)`` and divided by ``l`` once at the end. Padding keys of the last tile are
    ``-inf``; while no finite score has been seen the tile contributes 0 and nothing is rescaled.

    Returns ``(out fp32 [B*L, heads*64], raised int32 [B, heads, L, tiles], growth fp32 [same])``:
    ``raised`` marks the tiles that raised a query's running max and ``growth`` is by how much, in
    score units (tile 0 always raises it, from ``-inf``: growth ``inf``)."""
    D = heads * 64
    q, k, v = qkv.float().reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)  # bf16-exact operands
    nt = (L + tile - 1) // tile
    madd = torch.zeros(B, L) if mask is None else mask.float().reshape(B, L)
    m = torch.full((B, heads, L), float("-inf"))
    l = torch.zeros(B, heads, L)
    o = torch.zeros(B, heads, L, 64)
    raised = torch.zeros(B, heads, L, nt, dtype=torch.int32)
    growth = torch.zeros(B, heads, L, nt)
    for t in range(nt):
        ks = slice(t * tile, min((t + 1) * tile, L))
        s = (q @ k[:, :, ks].transpose(-1, -2)) * 0.125 + madd[:, None, None, ks]
        mn = torch.maximum(m, s.amax(-1))
        none = torch.isinf(mn) & (mn < 0)
        msub = torch.where(none, torch.zeros_like(mn), mn)
        alpha = torch.where(none, torch.ones_like(mn), torch.exp(m - msub))
        p = torch.exp(s - msub[..., None])
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + p.to(torch.bfloat16).float() @ v[:, :, ks]
        raised[..., t] = (mn > m).int()
        growth[..., t] = torch.where(mn > m, mn - m, torch.zeros_like(mn))
        m = mn
    out = (o / l[..., None]).permute(0, 2, 1, 3).reshape(B * L, D)
    return out, raised, growth


def embed_ref(ids, types, tab: EmbedTables, np_: NormParams, L):
    pos = torch.arange(ids.numel(), device=ids.device) % L
    x = tab.word.float()[ids.long().reshape(-1)] + tab.pos.float()[pos] + tab.type.float()[types.long().reshape(-1)]
    return F.layer_norm(x, (x.shape[-1],), np_.gamma, np_.beta, np_.eps)
