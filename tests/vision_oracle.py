"""fp64 oracles of the helper kernels of csrc/vision.hip (max-pool, average pool, pool + FC, image
pre-processing, patchify, the two casts) and bit-exact oracles of the packing kernels of csrc/pack.hip
(``pack_conv_kernel``, ``frag_pack_kernel``), an element-wise comparator with a derived bound, output buffers
with guard regions, and the deterministic inputs of every per-kernel GPU case, so that
tests/test_vision_oracle_cpu.py judges the oracle on exactly what tests/test_vision_kernels_gpu.py and
tests/test_pack_kernels_gpu.py run. Torch and numpy, CPU only. Not a test module.

The operations, as the kernels define them:

* ``maxpool_kernel`` (vision.hip lines 16-67): the maximum over the taps of a k x k window that lie inside
  the image; a tap outside contributes nothing (K = 0: skipped, lines 54 and 57; K = 3: clamped to the
  nearest border pixel, which is a tap of the same window, lines 37 and 40). The maximum of bf16 values is a
  bf16 value: exact. ``fmaxf`` does not order -0 and +0, so the two compare equal here.
* ``avgpool_kernel`` (lines 72-98): ``bf16(sum_hw x / HW)``, the sum and the division in fp32 (lines 87, 95,
  96), the input NHWC or channel-blocked [N][C/32][HW][32] (line 81).
* ``pool_fc_kernel`` (lines 116-205): ``mean[c] = (sum_hw x) * (1.f / HW)`` in fp32 (lines 166, 171), NOT
  rounded to bf16; ``pooled``: the fp32 means are the input (line 135). ``out[b][n] = sum_c w[n][c] mean[c]
  + bias[n]`` with bf16 weights widened to fp32, fp32 products and sums (lines 192-204); no bias pointer: + 0.
  Columns N .. ldo - 1 are not written (line 203).
* ``preprocess_kernel`` / ``preprocess_u8c3_kernel`` (lines 281-366): ``v`` = the fp32 source value (mode 0,
  NCHW) or ``fp32(u8) * fp32(1 / 255)`` (mode 1, NHWC; lines 309, 360); with a mean ``(v - mean[c]) *
  inv_std[c]`` in fp32, where a byte's ``u / 255 - mean`` is ONE fused multiply-add in both kernels (lines
  306, 360: the same bits for the same pixel); one bf16 rounding at the store; channels Cin .. Cpad - 1 zero.
* ``patchify_kernel`` (lines 548-580): the mode 0 arithmetic on fp32 NCHW, stored as patch rows
  [N * (H/16) * (W/16)][Cin * 256], column (c, ky, kx).
* the casts (lines 582-594): RNE (a NaN stays a NaN) and the widening shift.
* ``pack_conv_kernel`` (pack.hip lines 33-71) and ``frag_pack_kernel`` (lines 81-115): fp contraction is off,
  so every fp32 operation rounds once and in the order written: ``scale = float32(float64(gamma) /
  sqrt(float64(var) + eps))``, ``w * scale``, ``(b - mean) * scale + beta``; bf16 by integer RNE with
  NaN -> 0x7FC0; K order (r, s, c) with channels padded to ``cin_p``; fragment-major
  [rows/16][ksteps][64 lanes][8], lane = 16 * (k chunk of 8) + row.

An element of a rounded operation passes iff

    |got - ref| <= r_out + c * 2**-24 * A

with ``r_out = ulp_bf16(ref) / 2`` for a bf16 output, ``2**-24 |ref|`` for an fp32 one, and ``A`` the sum of
the absolute values the operation adds: ``mean|x|`` (avgpool), ``|w| . mean|x| + |b|`` (pool_fc),
``(|v| + |mean|) |inv_std|`` (preprocess, patchify). No whole-tensor scale, no element left out; a NaN where
the reference has none fails; every guard element must keep its fill, bit for bit.

The constants ``c`` come from a measurement, as ``C_ACC`` of tests/gemm_oracle.py did: torch's fp32 evaluation
of the same operation against fp64 over every case of the tables below, times four, up to a power of two,
never above the operation count (``HW + 1`` additions and one division for pooling, ``HW + C + 3`` for
pool_fc, 4 for preprocess: the u8 product, the subtraction, the product, and one more for a fused form). The
measured figures are in profiles/vision_oracle/README.md; tests/test_vision_oracle_cpu.py measures again.

Exact cases need no bound and are compared bit for bit: maxpool; mode 0 and patchify without a mean (one RNE);
u8 without a mean (one fp32 product, then RNE); both casts; the packers; and ``kind="exact"``: small integers
whose sums stay below 2**24 with a power-of-two ``HW`` (avgpool, pool_fc) or power-of-two ``inv_std``
(preprocess), where every fp32 intermediate is exact whatever the order.
"""
import functools
import zlib
from collections import namedtuple

import numpy as np
import torch

U32 = 2.0 ** -24     # half an fp32 ulp, relative: one fp32 rounding
C_POOL = 4.0         # avgpool: 4 x the worst measured fp32-against-fp64 figure, to a power of two
C_POOLFC = 8.0       # pool_fc
C_PRE = 4.0          # preprocess / patchify with a mean (the operation count: 4)
NAN16 = 0x7FC0       # the fill of a bf16 / uint16 output buffer; fp32: NAN16 << 16
GUARD_TAIL = 96      # elements after the last row
BF16_MAX = 0x7F7F    # the largest finite bf16

Ref = namedtuple("Ref", "y A")
Report = namedtuple("Report", "ok ratio index got ref bound bad")


# ------------------------------------------------------------------------------------------------
# number formats
def bf16_bits(a):
    """fp32 array -> bf16 bit patterns (uint16): integer round-to-nearest-even, NaN -> 0x7FC0."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)
    return np.where(nan, np.uint16(NAN16), r)


def bf16_trunc_bits(a):
    """Not the kernels' rounding: truncation (a planted fault)."""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bits_to_f32(b):
    """bf16 bit patterns -> the fp32 values they stand for."""
    return (np.asarray(b).astype(np.uint32) << 16).view(np.float32)


def t_bits(t):
    """Bit pattern of a bf16 / fp32 / integer tensor as an int64 tensor (non-negative)."""
    t = t.contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).long() & 0xFFFF
    if t.dtype == torch.float32:
        return t.view(torch.int32).long() & 0xFFFFFFFF
    return t.long() & (0xFFFF if t.element_size() == 2 else 0xFFFFFFFF)


def bf16_tensor(bits):
    """uint16 numpy bit patterns -> a torch bf16 tensor."""
    return torch.from_numpy(np.ascontiguousarray(bits).astype(np.uint16).view(np.int16)).view(torch.bfloat16)


def ulp_bf16(t):
    """The spacing of bf16 numbers in the binade of ``|t|`` (float64)."""
    _, e = torch.frexp(t.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - 8)


def round_bf16(y):
    """float64 / fp32 tensor -> the bf16 bit patterns (int64) of RNE(fp32(y)), for exact cases."""
    f = y.float()
    assert torch.equal(f.double(), y.double()), "an exact case must be exact in fp32"
    return torch.from_numpy(bf16_bits(f.numpy()).astype(np.int64))


# ------------------------------------------------------------------------------------------------
# the comparator
def bound(ref: Ref, out_f32, c):
    y = ref.y.double()
    r_out = U32 * y.abs() if out_f32 else ulp_bf16(y) / 2
    return r_out + c * U32 * ref.A.double()


def compare(got, ref: Ref, out_f32, c) -> Report:
    """``got`` (the stored values) against ``ref``, element by element; the worst element by error / bound."""
    assert tuple(got.shape) == tuple(ref.y.shape), (tuple(got.shape), tuple(ref.y.shape))
    g, y = got.double().reshape(-1), ref.y.double().reshape(-1)
    bd = bound(ref, out_f32, c).reshape(-1)
    err = (g - y).abs()
    ratio = err / bd.clamp_min(2.0 ** -149)
    ratio = torch.where(torch.isfinite(g) & torch.isfinite(ratio), ratio, torch.full_like(ratio, float("inf")))
    ratio = torch.where((err == 0) & torch.isfinite(g), torch.zeros_like(ratio), ratio)
    bad = int((ratio > 1.0).sum())
    i = int(ratio.argmax())
    return Report(bad == 0, float(ratio[i]), i, float(g[i]), float(y[i]), float(bd[i]), bad)


def compare_bits(got_bits, want_bits, zero_sign=True, nan_payload=True, width=16) -> Report:
    """Bit patterns (int64 tensors) against bit patterns. ``zero_sign`` False: -0 and +0 compare equal
    (maxpool); ``nan_payload`` False: any NaN matches a NaN."""
    assert got_bits.numel() == want_bits.numel(), (tuple(got_bits.shape), tuple(want_bits.shape))
    g, w = got_bits.reshape(-1).long(), want_bits.reshape(-1).long()   # (compared in storage order)
    sign = 1 << (width - 1)
    if not zero_sign:
        g, w = torch.where(g == sign, 0, g), torch.where(w == sign, 0, w)
    ne = g != w
    if not nan_payload:
        emask, mmask = (0x7F80, 0x007F) if width == 16 else (0x7F800000, 0x007FFFFF)
        isnan = lambda b: ((b & emask) == emask) & ((b & mmask) != 0)  # noqa: E731
        ne = ne & ~(isnan(g) & isnan(w))
    bad = int(ne.sum())
    i = int(ne.long().argmax()) if bad else 0
    return Report(bad == 0, float("inf") if bad else 0.0, i, int(g[i]) if g.numel() else 0,
                  int(w[i]) if w.numel() else 0, 0.0, bad)


def describe(rep: Report) -> str:
    return (f"worst ratio {rep.ratio:.3g} at element {rep.index}: got {rep.got!r} ref {rep.ref!r} "
            f"bound {rep.bound:.3g}; {rep.bad} elements differ")


def check(got, ref: Ref, out_f32, c, label=""):
    rep = compare(got, ref, out_f32, c)
    assert rep.ok, f"{label}: {describe(rep)}"
    return rep


def check_bits(got_bits, want_bits, label="", **kw):
    rep = compare_bits(got_bits, want_bits, **kw)
    assert rep.ok, f"{label}: {describe(rep)} (bit patterns)"
    return rep


def old_metric(got, ref_y) -> float:
    """What the whole-tensor tests assert (< 1e-2): max|got - ref| / max|ref|."""
    return float((got.double() - ref_y.double()).abs().max() / ref_y.double().abs().max().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------
# output buffers with guards: [rows][ld] with ``cols`` live columns, GUARD_TAIL elements behind the last row
def new_out(rows, cols, ld=None, dtype=torch.bfloat16, device="cpu"):
    """The filled output buffer (flat): every element holds the fill, NaN 0x7FC0 (fp32: 0x7FC00000)."""
    ld = cols if ld is None else ld
    n = rows * ld + GUARD_TAIL
    if dtype == torch.float32:
        return torch.full((n,), NAN16 << 16, dtype=torch.int64).to(torch.int32).view(torch.float32).to(device)
    return torch.full((n,), NAN16, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).to(device)


def split_out(buf, rows, cols, ld=None):
    """-> (the live [rows, cols] part, the number of guard elements that lost their fill)."""
    ld = cols if ld is None else ld
    buf = buf.cpu()
    assert buf.numel() == rows * ld + GUARD_TAIL, (buf.numel(), rows, ld)
    fill = NAN16 << 16 if buf.dtype == torch.float32 else NAN16
    b = t_bits(buf)
    v = b[:rows * ld].reshape(rows, ld)
    lost = int((b[rows * ld:] != fill).sum()) + int((v[:, cols:] != fill).sum())
    return buf[:rows * ld].reshape(rows, ld)[:, :cols], lost


def untouched(buf):
    """Every element of a filled buffer still holds the fill (a refused launch wrote nothing)."""
    fill = NAN16 << 16 if buf.dtype == torch.float32 else NAN16
    return bool((t_bits(buf.cpu()) == fill).all())


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32("/".join(str(k) for k in key).encode()))


def blocked(x):
    """Logical [N, HW, C] -> channel-blocked [N][C/32][HW][32] (the kernels' layout; C % 32 == 0)."""
    n, hw, c = x.shape
    out = x.new_zeros(n, c // 32, hw, 32)
    for cb in range(c // 32):
        out[:, cb] = x[:, :, cb * 32:(cb + 1) * 32]
    return out.contiguous()


# ------------------------------------------------------------------------------------------------
# maxpool
MAXPOOL_CLAMPED = [(2, 9, 11, 64, 3, 2, 1), (1, 1, 1, 8, 3, 2, 1), (1, 2, 3, 8, 3, 1, 1), (1, 7, 5, 24, 3, 1, 2),
                   (1, 6, 6, 8, 3, 3, 0)]   # k == 3: maxpool_kernel<3>
MAXPOOL_LOOP = [(1, 6, 8, 16, 2, 2, 0), (2, 5, 7, 8, 1, 2, 0), (1, 8, 6, 16, 4, 2, 1), (1, 7, 7, 8, 7, 1, 3),
                (1, 9, 9, 8, 5, 2, 2)]      # maxpool_kernel<0>
MAXPOOL_CASES = MAXPOOL_CLAMPED + MAXPOOL_LOOP
MAXPOOL_KINDS = ("distinct", "negative")


def pool_out(h, w, k, s, p):
    return (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1


@functools.lru_cache(maxsize=None)
def maxpool_input(case, kind):
    """[N, H, W, C] bf16, every value different from every other. "distinct": both signs, with -inf, +0, -0
    and the largest finite bf16 among them; "negative": every value below zero (so a zero-padded window is
    wrong), with -inf and the most negative finite bf16."""
    n, h, w, c = case[:4]
    g = _gen("maxpool", case, kind)
    numel = n * h * w * c
    mag = torch.randperm(0x7F7F - 0x0080, generator=g)[:numel] + 0x0080   # finite, normal, below BF16_MAX
    sign = torch.randint(0, 2, (numel,), generator=g) if kind == "distinct" else torch.ones(numel, dtype=torch.long)
    b = (mag | (sign << 15)).numpy().astype(np.uint16)
    special = [0xFF80, 0x0000, 0x8000, BF16_MAX] if kind == "distinct" else [0xFF80, 0xFF7F]
    pos = torch.randperm(numel, generator=g)[:len(special)].numpy()
    b[pos] = special
    return bf16_tensor(b).reshape(n, h, w, c)


def maxpool_ref(x, k, s, p, drop=None, pad_value=float("-inf")):
    """[N, H, W, C] -> float64 [N, P, Q, C]. ``drop`` = (r, s): that tap is left out; ``pad_value`` 0: zero
    padding (planted faults)."""
    n, h, w, c = x.shape
    P, Q = pool_out(h, w, k, s, p)
    xp = torch.full((n, h + 2 * p + k, w + 2 * p + k, c), pad_value, dtype=torch.float64)
    xp[:, p:p + h, p:p + w] = x.double()
    out = torch.full((n, P, Q, c), float("-inf"), dtype=torch.float64)
    for r in range(k):
        for q in range(k):
            if drop == (r, q):
                continue
            out = torch.maximum(out, xp[:, r:r + s * (P - 1) + 1:s, q:q + s * (Q - 1) + 1:s])
    return out


# ------------------------------------------------------------------------------------------------
# avgpool and pool_fc
AVGPOOL_CASES = [(1, 1, 64), (2, 31, 64), (2, 33, 128), (3, 49, 192)]      # (N, HW, C)
KINDS = ("rand", "exact")


def is_pow2(v):
    return v >= 1 and v & (v - 1) == 0


@functools.lru_cache(maxsize=None)
def pool_input(n, hw, c, kind, tag="avgpool"):
    """Logical [N, HW, C] bf16. "rand": normal values with a per-channel offset (so a channel's mean is not
    near zero against its mean |x|); "exact": integers in [-8, 8] that depend on image, pixel and channel."""
    g = _gen(tag, n, hw, c, kind)
    if kind == "exact":
        ni, pi, ci = torch.meshgrid(torch.arange(n), torch.arange(hw), torch.arange(c), indexing="ij")
        x = ((ni * 7 + pi * 3 + ci * 5 + (pi * ci) % 11 + torch.randint(0, 17, (n, hw, c), generator=g)) % 17 - 8).float()
    else:
        x = torch.randn(n, hw, c, generator=g) + 0.75 * torch.randn(n, 1, c, generator=g)
    return x.bfloat16()


def avgpool_ref(x, dtype=torch.float64, divisor=None):
    """[N, HW, C] -> Ref([N, C]); ``divisor``: a planted fault."""
    v = x.to(dtype)
    d = x.shape[1] if divisor is None else divisor
    return Ref(v.sum(1) / d, v.abs().sum(1) / x.shape[1])


def avgpool_c(hw):
    return min(C_POOL, hw + 1.0)


# pool_fc: (B, HW, C, N, ldo - N, bias, pooled)
def _pfc(B=2, HW=4, C=64, N=17, ldo_pad=0, bias=True, pooled=False):
    return (B, HW, C, N, ldo_pad, bias, pooled)


POOLFC_CASES = ([_pfc(C=c) for c in (32, 96, 160, 512, 2048, 2112)]     # waves without a channel block; 2112: 2nd weight batch
                + [_pfc(HW=hw) for hw in (1, 15, 16, 17, 49)]           # around the 16-load batch
                + [_pfc(N=n) for n in (1, 16, 33)]                      # one row, a full group, three groups
                + [_pfc(ldo_pad=3), _pfc(bias=False), _pfc(B=3, HW=16, N=33)]
                + [_pfc(C=c, HW=49, pooled=True) for c in (32, 160, 2112)])
POOLFC_CASES = list(dict.fromkeys(POOLFC_CASES))


def poolfc_name(case):
    B, HW, C, N, lp, bias, pooled = case
    return f"B{B}-HW{HW}-C{C}-N{N}" + (f"-ldo+{lp}" if lp else "") + ("" if bias else "-nobias") + ("-pooled" if pooled else "")


def poolfc_exact_ok(case):
    return is_pow2(case[1]) or case[6]


@functools.lru_cache(maxsize=None)
def poolfc_inputs(case, kind):
    """-> (x, w, b): ``x`` logical [B, HW, C] bf16, or fp32 [B, C] channel means for ``pooled`` ("rand": not
    bf16-representable); ``w`` [N, C] fp32 holding bf16 values; ``b`` [N] fp32 (zeros when the launch passes
    no bias). "exact": integers, x in [-8, 8], w in [-2, 2], b in [-8, 8]."""
    B, HW, C, N, _, bias, pooled = case
    g = _gen("poolfc", case, kind)
    if kind == "exact":
        o, k = torch.arange(N)[:, None], torch.arange(C)[None, :]
        w = ((o * 3 + k * 5 + (o * k) % 7 + torch.randint(0, 5, (N, C), generator=g)) % 5 - 2).float()
        b = ((torch.arange(N) * 5) % 17 - 8).float()
        x = pool_input(B, HW, C, "exact", "poolfc")
        if pooled:
            x = pool_input(B, 1, C, "exact", "poolfc")[:, 0].float()
    else:
        w = (torch.randn(N, C, generator=g) / C ** 0.5).bfloat16().float()
        b = torch.rand(N, generator=g) - 0.5
        b[::4] /= 64
        x = pool_input(B, HW, C, "rand", "poolfc")
        if pooled:
            x = torch.randn(B, C, generator=g) + 0.5
            assert not torch.equal(x, x.bfloat16().float())
    if not bias:
        b = torch.zeros(N)
    return x, w, b


def poolfc_ref(x, w, b, dtype=torch.float64, divisor=None, mean_bf16=False):
    """-> Ref([B, N]). ``divisor`` and ``mean_bf16`` (the means rounded to bf16 before the FC) plant faults."""
    if x.dim() == 2:
        m, ma = x.to(dtype), x.to(dtype).abs()
    else:
        v = x.to(dtype)
        m, ma = v.sum(1) / (x.shape[1] if divisor is None else divisor), v.abs().sum(1) / x.shape[1]
    if mean_bf16:
        m = m.float().bfloat16().to(dtype)
    W, bb = w.to(dtype), b.to(dtype)
    return Ref(m @ W.T + bb, ma @ W.abs().T + bb.abs())


def poolfc_c(case):
    return min(C_POOLFC, case[1] + case[2] + 3.0)


# ------------------------------------------------------------------------------------------------
# preprocess: (name, mode, N, H, W, Cin, Cpad, path)   path: "generic" / "u8c3" / "unaligned"
PRE_CASES = ([(f"f32-c{ci}-p{cp}", 0, 2, 5, 7, ci, cp, "generic") for ci in (1, 3, 4, 8) for cp in (8, 16, 24)]
             + [("f32-257px", 0, 1, 257, 1, 3, 8, "generic")]          # a second workgroup with one live thread
             + [(f"u8-c{ci}", 1, 2, 5, 7, ci, 8, "generic") for ci in (1, 4)]
             + [("u8-c3-35px", 1, 1, 5, 7, 3, 8, "generic"),            # npix % 4 != 0
                ("u8-c3-unaligned", 1, 1, 4, 8, 3, 16, "unaligned")]    # npix % 4 == 0, src + 4 bytes
             + [(f"u8c3-{npx}px", 1, 1, 1, npx, 3, 8 + 8 * (i % 2), "u8c3") for i, npx in enumerate((4, 1020, 1024, 1028, 2040))]
             + [("u8c3-allbytes", 1, 1, 32, 32, 3, 8, "u8c3")])
PRE_BY_NAME = {c[0]: c for c in PRE_CASES}
INV255 = np.float32(1.0) / np.float32(255.0)   # the kernels' constant 1.0f / 255.0f


def pre_kinds(case):
    """(kind, with mean): "rand" with and without a mean; "exact" with one (small integers, power-of-two
    inv_std) where the source is fp32 (a u8 source times 1 / 255 is no integer)."""
    return [("rand", False), ("rand", True)] + ([("exact", True)] if case[1] == 0 else [])


@functools.lru_cache(maxsize=None)
def pre_inputs(case, kind, with_mean):
    """-> (src, mean, inv_std): src fp32 [N, Cin, H, W] or uint8 [N, H, W, Cin]; mean, inv_std fp32 [Cin] or
    None."""
    name, mode, n, h, w, cin, cpad, path = case
    g = _gen("pre", name, kind)
    if mode == 1:
        src = torch.randint(0, 256, (n, h, w, cin), dtype=torch.uint8, generator=g)
        if name == "u8c3-allbytes":   # thread t owns bytes 12 t .. 12 t + 11: slot s takes every value once
            t, s = torch.arange(256)[:, None], torch.arange(12)[None, :]
            src = ((t * (2 * s + 1) + 21 * s) % 256).to(torch.uint8).reshape(1, 32, 32, 3)
    elif kind == "exact":
        src = torch.randint(-64, 65, (n, cin, h, w), generator=g).float()
    else:
        src = torch.randn(n, cin, h, w, generator=g)
    if not with_mean:
        return src, None, None
    if kind == "exact":
        mean = (torch.arange(cin) % 5 - 2).float()
        inv = 2.0 ** ((torch.arange(cin) % 4).float() - 2)
    else:   # every channel its own constants, so a neighbour's are wrong; both signs of the mean
        mean = (0.3 + 0.05 * torch.arange(cin).float()) * (1 - 2 * (torch.arange(cin) % 3 == 2).float())
        inv = 1.0 / (0.2 + 0.011 * torch.arange(cin).float())
    return src, mean.float(), inv.float()


def pre_ref(src, mode, cpad, mean, inv_std, dtype=torch.float64, channel_shift=0, bgr=False):
    """-> Ref([N*H*W, Cpad]) in NHWC order; columns Cin .. Cpad - 1 are zero. ``channel_shift``: the
    constants of channel c + shift; ``bgr``: the channels reversed (planted faults)."""
    if mode == 1:
        v = src.to(dtype) * torch.tensor(float(INV255), dtype=dtype)   # (the constant is an fp32 value)
    else:
        n, cin, h, w = src.shape
        v = torch.stack([src[:, c] for c in range(cin)], dim=-1).to(dtype)   # NCHW -> NHWC
    cin = v.shape[-1]
    if bgr:
        v = torch.stack([v[..., cin - 1 - c] for c in range(cin)], dim=-1)
    A = v.abs()
    if mean is not None:
        idx = (torch.arange(cin) + channel_shift) % cin
        mu, inv = mean[idx].to(dtype), inv_std[idx].to(dtype)
        v, A = (v - mu) * inv, (A + mu.abs()) * inv.abs()
    y = torch.zeros(*v.shape[:-1], cpad, dtype=dtype)
    a = torch.zeros_like(y)
    y[..., :cin], a[..., :cin] = v, A
    return Ref(y.reshape(-1, cpad), a.reshape(-1, cpad))


def pre_exact_bits(src, mode, cpad, mean, inv_std):
    """The bit patterns of a case that is exact: no mean (one RNE; u8: one fp32 product first), or integer
    values with power-of-two inv_std. -> int64 [N*H*W, Cpad]."""
    r32 = pre_ref(src, mode, cpad, mean, inv_std, torch.float32)
    if mean is not None:
        r64 = pre_ref(src, mode, cpad, mean, inv_std)
        assert torch.equal(r32.y.double(), r64.y), "not an exact case"
    return torch.from_numpy(bf16_bits(r32.y.numpy()).astype(np.int64))


# patchify: (Cin, H, W), N = 2
PATCH_CASES = [(ci, h, w) for ci in (1, 3, 8) for h, w in ((16, 32), (32, 16), (48, 48))]
PATCH_N = 2
F32_SPECIALS = [0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x00010000, 0x3F808000, 0x3F818000, 0x3F807FFF,
                0x3F808001, 0xBF808000, 0x80000000, 0x7F7FFFFF, 0x7F7F8000, 0x00008000, 0x00018000]
# +-Inf, fp32 subnormals, the smallest bf16 subnormal, ties to even (down, up), either side of a tie, a negative
# tie, -0, the carries into Inf, ties among the bf16 subnormals


@functools.lru_cache(maxsize=None)
def patch_inputs(case, with_mean):
    """-> (src fp32 [2, Cin, H, W], mean, inv_std). Without a mean the specials above are planted."""
    cin, h, w = case
    g = _gen("patch", case, with_mean)
    src = torch.randn(PATCH_N, cin, h, w, generator=g)
    if with_mean:
        _, mean, inv = pre_inputs(("patch", 0, 1, 1, 1, cin, 8, "generic"), "rand", True)
        return src, mean, inv
    flat = src.reshape(-1)
    pos = torch.randperm(flat.numel(), generator=g)[:len(F32_SPECIALS)]
    flat[pos] = torch.from_numpy(np.array(F32_SPECIALS, dtype=np.uint32).view(np.float32).copy())
    return src, None, None


def patch_ref(src, mean, inv_std, dtype=torch.float64, channel_shift=0):
    """fp32 [N, Cin, H, W] -> Ref([N * (H/16) * (W/16), Cin * 256]), column (c, ky, kx)."""
    n, cin, h, w = src.shape
    py, px = h // 16, w // 16
    v = src.to(dtype)
    A = v.abs()
    if mean is not None:
        idx = (torch.arange(cin) + channel_shift) % cin
        mu, inv = mean[idx].to(dtype).view(1, cin, 1, 1), inv_std[idx].to(dtype).view(1, cin, 1, 1)
        v, A = (v - mu) * inv, (A + mu.abs()) * inv.abs()
    out = [torch.zeros(n * py * px, cin * 256, dtype=dtype) for _ in range(2)]
    for t, o in zip((v, A), out):
        for i in range(n):
            for a in range(py):
                for b in range(px):
                    o[(i * py + a) * px + b] = t[i, :, a * 16:a * 16 + 16, b * 16:b * 16 + 16].reshape(-1)
    return Ref(*out)


# casts
def cast_f32_patterns():
    """Every upper half-word crossed with the lower halves that decide a rounding: 327680 fp32 patterns."""
    hi = np.arange(65536, dtype=np.uint32)[:, None] << 16
    lo = np.array([0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=np.uint32)[None, :]
    return (hi | lo).reshape(-1)


CAST_TAILS = (1, 3, 4, 5, 1023, 1027)   # around the 4-wide vector body of cast_f32_bf16_kernel


# ------------------------------------------------------------------------------------------------
# csrc/pack.hip
def fragment(dense_bits, lane_fault=False):
    """[rows, K] uint16 -> [rows/16, K/32, 64, 8]: lane l holds row l & 15, k = 8 (l >> 4) .. + 7 of the step.
    ``lane_fault``: lane = row * 4 + kc (planted)."""
    rows, K = dense_bits.shape
    tile, ks, lane, j = np.meshgrid(np.arange(rows // 16), np.arange(K // 32), np.arange(64), np.arange(8),
                                    indexing="ij", sparse=True)
    row, kc = (lane >> 2, lane & 3) if lane_fault else (lane & 15, lane >> 4)
    return dense_bits[tile * 16 + row, ks * 32 + kc * 8 + j]


def bn_scale(gamma, var, eps, sqrt32=False):
    if sqrt32:   # a planted fault: the scale in fp32 throughout
        return (gamma / np.sqrt(var + np.float32(eps))).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + eps)).astype(np.float32)


def pack_conv_ref(w, bn=None, bias_in=None, eps=1e-5, cin_p=None, rows=None, ksteps=None, korder="rsc",
                  lane_fault=False, sqrt32=False, fma_bias=False, trunc=False):
    """``w`` fp32 [cout, cin, r, s] (numpy); ``bn`` = (gamma, beta, mean, var) or None -> (wf uint16
    [rows/16, ksteps, 64, 8], bias fp32 [cout]); one fp32 operation at a time, in the kernel's order."""
    w = np.asarray(w, dtype=np.float32)
    cout, cin, r, s = w.shape
    scale = None
    with np.errstate(invalid="ignore", over="ignore"):
        if bn is not None:
            gamma, beta, mean, var = (np.asarray(t, dtype=np.float32) for t in bn)
            scale = bn_scale(gamma, var, eps, sqrt32)
            w = w * scale[:, None, None, None]
        dense = np.zeros((rows, ksteps * 32), dtype=np.float32)
        for rr in range(r):
            for ss in range(s):
                k0 = ((rr * s + ss) if korder == "rsc" else (ss * r + rr)) * cin_p
                dense[:cout, k0:k0 + cin] = w[:, :, rr, ss]
        b = np.zeros(cout, dtype=np.float32) if bias_in is None else np.asarray(bias_in, dtype=np.float32)
        if bn is not None:
            t = b - mean
            if fma_bias:   # a planted fault: one rounding for the product and the sum
                b = (t.astype(np.float64) * scale.astype(np.float64) + beta.astype(np.float64)).astype(np.float32)
            else:
                b = t * scale + beta
    bits = bf16_trunc_bits(dense) if trunc else bf16_bits(dense)
    return fragment(bits, lane_fault), b.astype(np.float32)


W_SPECIALS = [0x7FC00001, 0x7F800000, 0xFF800000, 0x00000001, 0x00010000, 0x3F808000, 0x3F818000, 0x3F807FFF,
              0x3F808001, 0x80000000, 0xBF818000, 0x7F7FFFFF]
# NaN, +-Inf, subnormals, ties both ways, either side of a tie, -0, a negative tie, a carry into Inf

# name -> (cout, cin, r, s, cin_p, rows, ksteps, bn, bias_in)
PACK_CASES = {
    "stem-like": (5, 3, 7, 7, 8, 16, 13, True, False),       # K = 392 ends inside step 13 of 13
    "small-k": (17, 8, 1, 1, 8, 32, 1, False, False),
    "bias-only": (16, 32, 3, 3, 32, 64, 9, False, True),
    "bn-bias": (10, 5, 3, 3, 8, 64, 3, True, True),
    "wide-pad": (4, 3, 1, 1, 16, 64, 1, False, False),
    "linear": (10, 64, 1, 1, 64, 128, 4, False, True),        # two steps of padding behind K = 64
    "grid-stride": (2048, 256, 3, 3, 256, 2048, 72, True, False),   # 589824 chunks > 2048 blocks x 256
}


def pack_chunks(name):
    return PACK_CASES[name][5] // 16 * PACK_CASES[name][6] * 64


@functools.lru_cache(maxsize=None)
def pack_inputs(name):
    """-> (w, bn, bias_in) numpy fp32. Weights: normal values with W_SPECIALS planted; BN: channel 0 has
    var = 0, channel 1 a (gamma, var) whose fp32-sqrt scale differs from the fp64 one, channel 2 gamma = 0,
    channel 3 a negative gamma, channel 4 a (bias, mean, beta) whose fused multiply-add differs."""
    cout, cin, r, s, cin_p, rows, ksteps, has_bn, has_bias = PACK_CASES[name]
    rng = np.random.default_rng(zlib.crc32(f"pack/{name}".encode()))
    w = (rng.standard_normal((cout, cin, r, s)) * 0.1).astype(np.float32)
    flat = w.reshape(-1)
    pos = rng.permutation(flat.size)[:len(W_SPECIALS)]
    flat[pos] = np.array(W_SPECIALS, dtype=np.uint32).view(np.float32)
    bias_in = rng.standard_normal(cout).astype(np.float32) if has_bias else None
    bn = None
    if has_bn:
        gamma = (0.5 + rng.random(cout)).astype(np.float32)
        beta = (0.1 * rng.standard_normal(cout)).astype(np.float32)
        mean = (0.1 * rng.standard_normal(cout)).astype(np.float32)
        var = (0.5 + rng.random(cout)).astype(np.float32)
        cg, cv = (0.5 + rng.random(4096)).astype(np.float32), (0.5 + rng.random(4096)).astype(np.float32)
        i = int(np.flatnonzero(bn_scale(cg, cv, 1e-5) != bn_scale(cg, cv, 1e-5, True))[0])
        var[0], gamma[1], var[1], gamma[2], gamma[3] = 0.0, cg[i], cv[i], 0.0, -abs(gamma[3])
        sc = bn_scale(gamma, var, 1e-5)[4]
        cm, cb = (0.1 * rng.standard_normal(4096)).astype(np.float32), (0.1 * rng.standard_normal(4096)).astype(np.float32)
        b4 = np.float32(0.0) if bias_in is None else bias_in[4]
        t = b4 - cm
        two = t * sc + cb
        one = (t.astype(np.float64) * np.float64(sc) + cb.astype(np.float64)).astype(np.float32)
        i = int(np.flatnonzero(two != one)[0])
        mean[4], beta[4] = cm[i], cb[i]
        bn = (gamma, beta, mean, var)
    return w, bn, bias_in


def pack_ref(name, **faults):
    cout, cin, r, s, cin_p, rows, ksteps, _, _ = PACK_CASES[name]
    w, bn, bias_in = pack_inputs(name)
    return pack_conv_ref(w, bn, bias_in, 1e-5, cin_p, rows, ksteps, **faults)


# frag_pack: name -> dict(R, K, nrows, ih, ka, acols, lda, bcols, ldb, a, b, out, bias_out, bias_a, bias_b)
def _fp(R, K, nrows=0, ih=0, ka=None, acols=None, lda=None, bcols=0, ldb=0, a=True, b=False, out=True,
        bias_out=True, bias_a=True, bias_b=False):
    ka = K if ka is None else ka
    acols = ka if acols is None else acols
    return dict(R=R, K=K, nrows=nrows, ih=ih, ka=ka, acols=acols, lda=acols if lda is None else lda, bcols=bcols,
                ldb=ldb or bcols, a=a, b=b, out=out, bias_out=bias_out, bias_a=bias_a, bias_b=bias_b)


FRAG_CASES = {
    "interleave-h5": _fp(32, 32, ih=5, bias_b=True),                       # rows 20 .. 31 zero
    "rows-21": _fp(32, 64, nrows=21),
    "a-only": _fp(16, 32, nrows=16, ka=20, acols=18),
    "b-only": _fp(16, 32, nrows=16, ka=20, acols=0, a=False, b=True, bcols=5),
    "a-b-seam": _fp(32, 32, nrows=30, ka=20, acols=18, b=True, bcols=5, bias_b=True),   # the seam inside k 16 .. 23
    "ld-wide": _fp(16, 64, nrows=16, ka=40, acols=33, lda=37, b=True, bcols=20, ldb=29),
    "bias-only": _fp(32, 32, nrows=32, out=False, bias_b=True),
    "no-bias-out": _fp(16, 32, nrows=16, bias_out=False),
    "no-bias-a": _fp(16, 32, nrows=16, bias_a=False),
    "grid-stride": _fp(4112, 2048, nrows=4112),                            # 1052672 chunks > 4096 blocks x 256
}


@functools.lru_cache(maxsize=None)
def frag_inputs(name):
    """-> (a, b, bias_a, bias_b) numpy fp32 or None; the columns behind acols / bcols hold 777 (never read)."""
    c = FRAG_CASES[name]
    rng = np.random.default_rng(zlib.crc32(f"frag/{name}".encode()))
    nsrc = 4 * c["ih"] if c["ih"] else max(c["nrows"], 1)

    def mat(cols, ld):
        m = np.full((nsrc, max(ld, 1)), 777.0, dtype=np.float32)
        m[:, :cols] = rng.standard_normal((nsrc, cols)).astype(np.float32)
        flat = m[:, :cols]
        k = min(len(W_SPECIALS), flat.size)
        pos = rng.permutation(flat.size)[:k]
        flat[np.unravel_index(pos, flat.shape)] = np.array(W_SPECIALS[:k], dtype=np.uint32).view(np.float32)
        return m
    a = mat(c["acols"], c["lda"]) if c["a"] else None
    b = mat(c["bcols"], c["ldb"]) if c["b"] else None
    ba = rng.standard_normal(nsrc).astype(np.float32) if c["bias_a"] else None
    bb = rng.standard_normal(nsrc).astype(np.float32) if c["bias_b"] else None
    return a, b, ba, bb


def frag_pack_ref(name, lane_fault=False):
    """-> (out uint16 [R/16, K/32, 64, 8] or None, bias fp32 [R] or None)."""
    c = FRAG_CASES[name]
    a, b, ba, bb = frag_inputs(name)
    R, K = c["R"], c["K"]
    r = np.arange(R)
    if c["ih"] > 0:
        src = np.where(r < 4 * c["ih"], (r & 3) * c["ih"] + (r >> 2), -1)
    else:
        src = np.where(r < c["nrows"], r, -1)
    live = src >= 0
    out = None
    if c["out"]:
        dense = np.zeros((R, K), dtype=np.float32)
        if a is not None:
            dense[live, :c["acols"]] = a[src[live], :c["acols"]]
        if b is not None:
            dense[live, c["ka"]:c["ka"] + c["bcols"]] = b[src[live], :c["bcols"]]
        out = fragment(bf16_bits(dense), lane_fault)
    bias = None
    if c["bias_out"]:
        bias = np.zeros(R, dtype=np.float32)
        if ba is not None:
            bias[live] = ba[src[live]] + bb[src[live]] if bb is not None else ba[src[live]]
    return out, bias
