"""Inputs shared by tests/test_att_stream_cpu.py and tests/test_att_stream_gpu.py: every
(qkv, mask) the GPU tests of the streamed attention kernel run, built deterministically on the
CPU, so the CPU test can pin them with the kernel's emulation (ops/transformer.py
attention_stream_ref) and the GPU tests run exactly those. Not a test module."""
import functools

import torch

TILE = 64  # csrc/transformer.hip ATS_T

# (B, L, heads): every edge of the 64-key tiling and of the 128-query blocks beyond the one-pass
# kernel's L <= 256; B * heads <= 4
LONG = [(2, 257, 2), (2, 288, 2), (2, 300, 2), (2, 320, 2), (2, 384, 2), (2, 512, 2), (2, 577, 2), (1, 1024, 1)]
# the one-pass kernel's ground, run through the streamed kernel with HIPZAP_ATT_STREAM=1
SHORT = [(2, L, 2) for L in (1, 7, 33, 64, 65, 197, 256)]
SPIKE_L, SPIKE_HEADS, SPIKE_AT = 320, 2, {"spike_last": 300, "spike_first": 5}


def half_mask(B, L):
    """The last sequence's second half at -1e9 (what bert.encode_inputs gives a padded sequence)."""
    m = torch.zeros(B, L)
    m[-1, L // 2:] = -1e9
    return m


@functools.lru_cache(maxsize=None)
def random_qkv(B, L, heads):
    g = torch.Generator().manual_seed(1000 * L + 10 * heads + B)
    return torch.randn(B * L, 3 * heads * 64, generator=g).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def spike(name):
    """Forced rescale (a rare data-dependent branch needs an input that takes it): scores sit near
    0 except one key, which every query meets at about +30. Every query carries the same vector u
    (|u|^2 = 16) plus small noise, the spike key is 15 u: q . k / 8 = 15 * 16 / 8 = 30; the other
    keys are small noise. ``spike_last``: the key is in the last tile, so every query's running max
    jumps there and everything accumulated before is rescaled by exp(-30). ``spike_first``: the
    key is in tile 0, so the max never grows after the first tile."""
    L, heads, at = SPIKE_L, SPIKE_HEADS, SPIKE_AT[name]
    g = torch.Generator().manual_seed(77)
    x = torch.randn(L, 3, heads, 64, generator=g)
    x[:, 0] = 0.05 * x[:, 0] + 0.5   # Q = noise + u, u = 0.5 in every head dim
    x[:, 1] = 0.05 * x[:, 1]         # K = noise ...
    x[at, 1] = 7.5                   # ... except the spike key = 15 u
    return x.reshape(L, 3 * heads * 64).to(torch.bfloat16)


def tile_mask(value, B=2, L=320):
    """The whole first tile of the last sequence masked with ``value`` (-1e9 or -inf)."""
    m = torch.zeros(B, L)
    m[-1, :TILE] = value
    return m


def cases():
    """(id, qkv, B, L, heads, mask) of every kernel-level GPU case."""
    out = []
    for B, L, H in LONG:
        out.append((f"long-L{L}-masked", random_qkv(B, L, H), B, L, H, half_mask(B, L)))
        out.append((f"long-L{L}-nomask", random_qkv(B, L, H), B, L, H, None))
    for B, L, H in SHORT:
        out.append((f"short-L{L}", random_qkv(B, L, H), B, L, H, half_mask(B, L)))
    for name in SPIKE_AT:
        out.append((name, spike(name), 1, SPIKE_L, SPIKE_HEADS, None))
    out.append(("tile0-1e9", random_qkv(2, 320, 2), 2, 320, 2, tile_mask(-1e9)))
    out.append(("tile0-inf", random_qkv(2, 320, 2), 2, 320, 2, tile_mask(float("-inf"))))
    return out


def attention_ref64(qkv, B, L, heads, mask=None):
    """ops.transformer.attention_ref in fp64 over the full tensor."""
    D = heads * 64
    q, k, v = qkv.double().reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) / 8.0
    if mask is not None:
        s = s + mask.double().reshape(B, 1, 1, L)
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B * L, D)


def rel(a, b):
    """tests/test_transformers_gpu.py _rel: max |a - b| / max |b|."""
    return ((a.float().cpu() - b.float().cpu()).abs().max() / (b.float().abs().max() + 1e-6)).item()
