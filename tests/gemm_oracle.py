"""fp64 oracles of the implicit-GEMM kernels of csrc/conv.hip (``conv_kernel``, ``conv2_kernel``: the
register-ring kernel) and csrc/gemm.hip (``gemm_lds_kernel``: the LDS-tiled GEMM and its CV conv mode), an
element-wise comparator with a derived bound, and the inputs of every per-kernel GPU case, built
deterministically on the CPU so that tests/test_gemm_oracle_cpu.py judges the oracle on exactly what
tests/test_conv_kernels_gpu.py and tests/test_gemm_kernels_gpu.py run. Torch only, CPU only. Not a test
module.

The operation, as the kernels define it (``conv_ref``):

* operands are bf16: the packed weights (``PackedConv.dense()``) and the activations; an fp32 activation
  (``HzConvParams.x_f32``) is ``bf16(relu(x))`` first (``f32relu_bf16``, conv.hip lines 68-72, applied at
  line 285);
* a tap outside the image contributes zero (conv.hip lines 206, 232: the load is skipped and the fragment
  zeroed; gemm.hip line 161: an offset past the buffer descriptor's range);
* ``acc = sum_k W[n][k] im2col(x)[m][k]`` in fp32 (the MFMA, conv.hip line 291, gemm.hip line 233; the
  K-split partials are summed in fp32 through LDS, conv.hip line 358), ``+ bias[n]`` in fp32 (conv.hip
  line 304, gemm.hip line 266), ``+ res[m][n]`` widened from bf16, in fp32 (conv.hip lines 310-313, gemm.hip
  line 279);
* ``y = act(acc)`` in fp32: ``fmaxf``, ``gelu_erf`` (common.h line 167: the erf form), ``tanhf`` (conv.hip
  lines 315-324, gemm.hip lines 281-290);
* ONE rounding at the store: ``pack2`` to bf16 (conv.hip line 328, gemm.hip line 294), or none for an fp32
  output (conv.hip line 326, gemm.hip line 292).

An element passes iff

    |got - ref| <= r_out + L * C_ACC * 2**-24 * A + C_FN * 2**-24 * |ref|

with ``A = |W| |im2col(x)| + |b| + |res|``, ``r_out = ulp_bf16(ref) / 2`` for a bf16 output and
``2**-24 |ref|`` for an fp32 one, ``L`` = 1 for none, relu and tanh (slope <= 1) and 1.13 for GELU (the
largest slope of ``gelu_erf``, 1.129 at x = 1.41), ``C_FN`` = 0 for none and relu (exact in fp32). No
whole-tensor scale, no share of elements that may fail; a NaN fails; every element of a guard region must
still hold its fill, bit for bit.

``C_ACC`` from the operation count (u = 2**-24). Every product of two bf16 values has 16 significant bits and
is exact in fp32, so only additions round. Whatever the order (the MFMA's inside a 32-deep step is not
documented for bf16 inputs; the K-split adds ``kw`` partials; the LDS tile adds two 32-deep steps per stage)
a sum of K terms takes K - 1 additions, plus the zero accumulator: K; the K-split reduction starts from zero
too: ``kw``; bias and residual: 2; one for an fused-multiply inside ``act`` counted with the sum: 1. Each
rounds a partial sum no larger than A, by at most u A: |d acc| <= (K + kw + 3) u A, all roundings at
their largest and of one sign. That ceiling (``c_ops``; 1171 at K = 1152) is no bound to test
against. What fp32 really differs from fp64 by is measured in tests/test_gemm_oracle_cpu.py over every
case of the table below (torch's fp32 matmul, blocked and vectorised as the host likes): worst 2.62 u A
(gemm-577x128x132; profiles/gemm_oracle/README.md). ``C_ACC`` = 16 is 4 x that (10.5) rounded up to a power of two, the rule
that gave ``C_LN`` = 8 in tests/tx_oracle.py. With integer-valued operands (``kind="exact"``) every partial
sum is an integer below 2**24: the output is predictable to the bit and needs no ``C_ACC``.

``C_FN`` the same way: torch's fp32 ``erf`` and ``tanh`` against fp64 on the pre-activations of the table's
GELU and tanh cases, relative to the function value: worst 1.04 u (erf), 1.06 u (tanh); 4 x (4.24), to a power
of two: ``C_FN`` = 8. (GELU's own error on its negative tail, where ``1 + erf`` cancels, is
``|x| / 2 * d erf <= C_FN u A / 2``: it falls under the A term, A >= |x|.)
"""
import functools
import math
import zlib
from collections import namedtuple
from dataclasses import dataclass

import torch

from hipzap.ops import conv as CV

U32 = 2.0 ** -24   # half an fp32 ulp, relative: one fp32 rounding
C_ACC = 16.0       # 4 x the worst measured fp32-against-fp64 figure (2.62), to a power of two
C_FN = 8.0         # 4 x the worst measured torch fp32 erf / tanh figure (1.06), to a power of two
L_ACT = {"none": 1.0, "relu": 1.0, "tanh": 1.0, "gelu": 1.13}
NAN16 = 0x7FC0     # the fill of a bf16 output buffer (torch's NaN); fp32: NAN16 << 16
GUARD_ROWS = 2     # row-major outputs: rows M, M + 1 of [M + 2][ldo]
GUARD_TAIL = 96    # channel-blocked outputs: elements behind the last block

Ref = namedtuple("Ref", "y A acc")   # [M, Cout]; y unrounded, A = |W||x| + |b| + |res|, acc before act
Report = namedtuple("Report", "ok ratio row column got ref bound bad")


def _bf16(t):
    """Round to bf16 (nearest even) and back."""
    return t.to(torch.bfloat16).to(t.dtype)


def ulp_bf16(t):
    """The spacing of bf16 numbers in the binade of ``|t|`` (float64)."""
    _, e = torch.frexp(t.double().abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - 8)


def c_ops(K, kw=16):
    """The operation-count ceiling of C_ACC (module docstring)."""
    return K + kw + 3


def out_hw(pc, h, w):
    return (h + 2 * pc.pad - pc.r) // pc.stride + 1, (w + 2 * pc.pad - pc.s) // pc.stride + 1


def gelu_tanh(a):
    """Not the kernels' GELU: the tanh approximation (a planted fault)."""
    return 0.5 * a * (1.0 + torch.tanh(0.7978845608028654 * (a + 0.044715 * a ** 3)))


def activation(acc, act):
    if act == "relu":
        return torch.relu(acc)
    if act == "gelu":
        return 0.5 * acc * (1.0 + torch.erf(acc * 0.70710678118654752))
    if act == "tanh":
        return torch.tanh(acc)
    assert act == "none", act
    return acc


def im2col(x, pc, padding="zeros"):
    """[n, h, w, C] -> [n * P * Q, R * S * C], K ordered (r, s, c) as ``pack_conv`` orders the weights."""
    n, h, w, c = x.shape
    P, Q = out_hw(pc, h, w)
    xp = x
    if pc.pad:
        xp = x.new_zeros(n, h + 2 * pc.pad, w + 2 * pc.pad, c)
        xp[:, pc.pad:pc.pad + h, pc.pad:pc.pad + w] = x
        if padding == "replicate":  # a planted fault
            ih = (torch.arange(h + 2 * pc.pad) - pc.pad).clamp(0, h - 1)
            iw = (torch.arange(w + 2 * pc.pad) - pc.pad).clamp(0, w - 1)
            xp = x[:, ih][:, :, iw]
    cols = [xp[:, r:r + pc.stride * (P - 1) + 1:pc.stride, s:s + pc.stride * (Q - 1) + 1:pc.stride]
            for r in range(pc.r) for s in range(pc.s)]
    return torch.cat(cols, -1).reshape(n * P * Q, pc.r * pc.s * c)


def conv_ref(x, pc, n, h, w, residual=None, act="relu", x_f32=False, dtype=torch.float64, hooks=None):
    """``conv_kernel`` / ``gemm_lds_kernel`` (CV) on ``pc.dense()`` and ``pc.bias``. ``x``: logical NHWC
    [n, h, w, pc.cin], bf16 values, or fp32 with ``x_f32`` (then ``bf16(relu(x))`` is the operand);
    ``residual``: logical [n, P, Q, cout] bf16 or None. Everything is widened to ``dtype`` and nothing is
    rounded after that. Returns ``Ref(y, A, acc)``, each [n * P * Q, cout]. ``hooks`` plants faults:
    ``padding`` = "replicate", ``k_keep`` = a bool mask over K of the products that are summed."""
    hk = hooks or {}
    assert tuple(x.shape) == (n, h, w, pc.cin), (tuple(x.shape), (n, h, w, pc.cin))
    xo = _bf16(torch.relu(x.float())) if x_f32 else x.float()
    assert torch.equal(xo, _bf16(xo)), "activations must hold bf16 values"
    cols = im2col(xo.to(dtype), pc, hk.get("padding", "zeros"))
    W = pc.dense().to(dtype)
    if "k_keep" in hk:
        W = W * hk["k_keep"].to(dtype)[None, :]
    b = pc.bias.to(dtype)
    acc = cols @ W.T + b
    A = cols.abs() @ W.abs().T + b.abs()
    if residual is not None:
        r = residual.reshape(-1, pc.cout).to(dtype)
        acc = acc + r
        A = A + r.abs()
    return Ref(activation(acc, act), A, acc)


def linear_ref(x, pc, rows, residual=None, act="none", dtype=torch.float64, hooks=None):
    """The 1x1 / ``x_rowmajor`` case: ``x`` [>= rows, ldx >= K] bf16, row stride ``ldx``; only [:rows, :K]
    is an operand (conv.hip line 172: ``kk < p.K``; gemm.hip stages K / 64 steps). ``residual`` [rows, cout]."""
    xx = x[:rows, :pc.K].reshape(rows, 1, 1, pc.K)
    return conv_ref(xx, pc, rows, 1, 1, residual, act, False, dtype, hooks)


# ------------------------------------------------------------------------------------------------
# the comparator
def bound(ref: Ref, act, out_f32, c_acc=C_ACC, c_fn=C_FN):
    y = ref.y.double()
    r_out = U32 * y.abs() if out_f32 else ulp_bf16(y) / 2
    fn = 0.0 if act in ("none", "relu") else c_fn
    return r_out + L_ACT[act] * c_acc * U32 * ref.A.double() + fn * U32 * y.abs()


def compare(got, ref: Ref, act, out_f32, c_acc=C_ACC, c_fn=C_FN) -> Report:
    """``got`` [M, cout] (the stored values, widened) against ``ref``; the worst element by error / bound."""
    assert tuple(got.shape) == tuple(ref.y.shape), (tuple(got.shape), tuple(ref.y.shape))
    bd = bound(ref, act, out_f32, c_acc, c_fn)
    err = (got.double() - ref.y.double()).abs()
    ratio = err / bd.clamp_min(2.0 ** -149)
    ratio = torch.where(torch.isfinite(got.double()) & torch.isfinite(ratio), ratio,
                        torch.full_like(ratio, float("inf")))
    ratio = torch.where((err == 0) & torch.isfinite(got.double()), torch.zeros_like(ratio), ratio)
    bad = int((ratio > 1.0).sum())
    i = int(ratio.argmax())
    m, c = divmod(i, ratio.shape[1])
    return Report(bad == 0, float(ratio.reshape(-1)[i]), m, c, float(got.reshape(-1)[i]),
                  float(ref.y.reshape(-1)[i]), float(bd.reshape(-1)[i]), bad)


def describe(rep: Report) -> str:
    return (f"worst ratio {rep.ratio:.3g} at row {rep.row} column {rep.column}: got {rep.got!r} ref {rep.ref!r} "
            f"bound {rep.bound:.3g}; {rep.bad} elements over the bound")


def check(got, ref: Ref, act, out_f32, label="") -> Report:
    rep = compare(got, ref, act, out_f32)
    assert rep.ok, f"{label}: {describe(rep)}"
    return rep


def old_metric(got, ref_y) -> float:
    """What the whole-tensor tests assert (< 2e-2, 1e-2 for fp32 outputs): max|got - ref| / max|ref|."""
    return float((got.double() - ref_y.double()).abs().max() / ref_y.double().abs().max())


def expected_exact(ref: Ref, out_f32):
    """The stored value of an integer-exact case: the exact fp32, or its bf16 (nearest even)."""
    y = ref.y.float()
    assert torch.equal(y.double(), ref.y.double())
    return y if out_f32 else _bf16(y)


def bits(t):
    """Bit pattern of a bf16 / fp32 tensor (for bitwise comparison: NaN payloads and the sign of zero count)."""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


# ------------------------------------------------------------------------------------------------
# output buffers with guards
def out_layout(case, ldo=None):
    """-> (rowmajor, ldo, live elements, total elements) of the output buffer of ``case``."""
    rowmajor = case.xrow or case.out_rowmajor or not CV.is_blocked(case.cout)
    M = case.M
    if rowmajor:
        ld = case.cout + case.ldo_pad if ldo is None else ldo
        return True, ld, M * ld, (M + GUARD_ROWS) * ld
    return False, case.cout, M * case.cout, M * case.cout + GUARD_TAIL


def new_out(case, device="cpu"):
    """The NaN-filled output buffer (flat), guards included."""
    _, _, _, total = out_layout(case)
    return torch.full((total,), float("nan"), dtype=torch.float32 if case.out_f32 else torch.bfloat16, device=device)


def split_out(buf, case):
    """-> (the live [M, cout] part in logical order, the number of guard elements that lost their fill)."""
    rowmajor, ld, live, total = out_layout(case)
    assert buf.numel() == total
    fill = NAN16 << 16 if case.out_f32 else NAN16
    b = bits(buf).long() & (0xFFFFFFFF if case.out_f32 else 0xFFFF)
    M, co = case.M, case.cout
    if rowmajor:
        v = b.reshape(M + GUARD_ROWS, ld)
        lost = int((v[M:] != fill).sum()) + int((v[:M, co:] != fill).sum())
        got = buf.reshape(M + GUARD_ROWS, ld)[:M, :co]
    else:
        lost = int((b[live:] != fill).sum())
        n, P, Q = case.n, *case.PQ
        got = CV.from_blocked(buf[:live], (n, P, Q, co)).reshape(M, co)
    return got, lost


def res_buffer(case, res):
    """The residual in the OUTPUT's layout (the kernels read it at the output offset); NaN in pad columns."""
    if res is None:
        return None
    rowmajor, ld, _, _ = out_layout(case)
    if rowmajor:
        buf = torch.full((case.M, ld), float("nan"), dtype=torch.bfloat16)
        buf[:, :case.cout] = res.reshape(case.M, case.cout)
        return buf
    return CV.to_blocked(res).contiguous()


def x_buffer(case, x):
    """The activations in the device layout: row-major [M][ldx] (NaN in the pad columns: they are never
    read), channel-blocked [N][C/32][H][W][32], or NHWC for C < 32."""
    if case.xrow:
        buf = torch.full((case.M, case.cin + case.ldx_pad), float("nan"), dtype=torch.bfloat16)
        buf[:, :case.cin] = x
        return buf
    return CV.to_blocked(x).contiguous()


# ------------------------------------------------------------------------------------------------
# the case table
@dataclass(frozen=True)
class Case:
    name: str
    inst: str                # kernel instantiation / family
    n: int
    h: int
    w: int
    cin: int
    cout: int
    r: int = 1
    s: int = 1
    stride: int = 1
    pad: int = 0
    act: str = "relu"
    res: bool = False
    out_f32: bool = False
    x_f32: bool = False
    xrow: bool = False       # x_rowmajor: n = rows, h = w = 1
    ldx_pad: int = 0
    ldo_pad: int = 0
    bias: bool = True        # False: the launch passes bias = NULL
    out_rowmajor: bool = False
    row_pad: int = CV.ROW_PAD

    @property
    def PQ(self):
        return ((self.h + 2 * self.pad - self.r) // self.stride + 1,
                (self.w + 2 * self.pad - self.s) // self.stride + 1)

    @property
    def M(self):
        return self.n * self.PQ[0] * self.PQ[1]

    @property
    def K(self):
        return self.r * self.s * self.cin

    @property
    def ksteps(self):
        return (self.K + 31) // 32


def _gen(case, kind):
    return torch.Generator().manual_seed(zlib.crc32(f"{case.name}/{kind}".encode()))


@functools.lru_cache(maxsize=128)
def case_weights(case, kind):
    """The packed weights of ``case`` (CPU). ``kind``: "rand" (normal weights of unit output variance, bias
    in [-0.5, 0.5] with every fourth channel's 1 / 64 of that) or "exact" (integers in [-2, 2], integer
    bias in [-8, 8]); both depend on the position (o, k)."""
    g = _gen(case, kind + "/w")
    co, K = case.cout, case.K
    if kind == "exact":
        o, k = torch.arange(co)[:, None], torch.arange(K)[None, :]
        w = ((o * 3 + k * 5 + (o * k) % 7 + torch.randint(0, 5, (co, K), generator=g)) % 5 - 2).float()
        b = ((torch.arange(co) * 5) % 17 - 8).float()
    else:
        w = torch.randn(co, K, generator=g) / math.sqrt(K)
        b = torch.rand(co, generator=g) - 0.5
        b[::4] /= 64
    if not case.bias:
        b = torch.zeros(co)
    return CV.pack_matrix(w, b, case.cin, case.r, case.s, case.stride, case.pad, case.row_pad)


@functools.lru_cache(maxsize=128)
def case_inputs(case, kind):
    """-> (x, res): ``x`` logical NHWC (``[M, K]`` for ``xrow``), bf16 or fp32 (``x_f32``: negative and not
    bf16-representable values); ``res`` logical [n, P, Q, cout] bf16 or None. "exact": x in [-3, 3] with the
    position (image, row, column, channel) encoded asymmetrically, res integer in [-4, 4]."""
    g = _gen(case, kind + "/x")
    n, h, w, c = case.n, case.h, case.w, case.cin
    P, Q = case.PQ
    if kind == "exact":
        ni, hi, wi, ci = torch.meshgrid(torch.arange(n), torch.arange(h), torch.arange(w), torch.arange(c),
                                        indexing="ij")
        x = ((ni * 5 + hi * 3 + wi + ci * 2 + (hi * wi) % 5 + (ci * wi) % 3
              + torch.randint(0, 7, (n, h, w, c), generator=g)) % 7 - 3).float()
        if case.x_f32:  # negative values are live operands of relu-at-load: keep them, exactly
            x = x.clone()
        res = torch.randint(-4, 5, (n, P, Q, case.cout), generator=g).float().bfloat16() if case.res else None
    else:
        x = torch.randn(n, h, w, c, generator=g)
        res = torch.randn(n, P, Q, case.cout, generator=g).bfloat16() if case.res else None
    if case.x_f32:
        x = x.float()  # fp32: not rounded ("rand" values are not bf16-representable, about half negative)
    else:
        x = x.bfloat16()
    if case.xrow:
        x = x.reshape(n, c)
    return x, res


@functools.lru_cache(maxsize=128)
def case_ref(case, kind, dtype=torch.float64):
    x, res = case_inputs(case, kind)
    pc = case_weights(case, kind)
    if case.xrow:
        return linear_ref(x, pc, case.n, None if res is None else res.reshape(case.n, case.cout), case.act, dtype)
    return conv_ref(x, pc, case.n, case.h, case.w, res, case.act, case.x_f32, dtype)


# --- csrc/conv.hip: the register-ring kernel. cfg -> (FC, FP) = CV.TILES; ring depth per tile
def ring_depth(cfg):
    fc, fp = CV.TILES[cfg]
    return 6 if fc + fp <= 2 else 4 if fc + fp <= 3 else 3 if fc + fp <= 4 else 2


def ring_configs():
    """Every (cfg, kw) that ``CV.legal`` allows over the 9 tiles."""
    return [(cfg, kw) for cfg in range(9) for kw in (1, 2, 4, 8, 16) if CV.legal(cfg, kw)]


def ksteps_of_interest(cfg, kw):
    d = ring_depth(cfg)
    return sorted({1, 2, kw - 1, kw, kw + 1, d, d + 1, 2 * d + 3} - {0})


KSTEPS_ALL = sorted({k for cfg, kw in ring_configs() for k in ksteps_of_interest(cfg, kw)})

CONV_CASES = [
    # FAST 1x1
    Case("pix1", "fast1x1", 1, 1, 1, 64, 64),                                     # M = 1
    Case("pix1-res-f32", "fast1x1", 1, 1, 1, 32, 96, res=True, out_f32=True, act="none"),
    Case("c40-rowmajor", "fast1x1", 3, 5, 7, 64, 40, res=True),                   # N tail, groups of 4
    Case("c4-rowmajor", "fast1x1", 1, 7, 5, 32, 4, act="none", out_f32=True),
    Case("c96-blocked", "fast1x1", 3, 5, 7, 64, 96, res=True, act="gelu"),        # Cout % 64 != 0
    # FAST general: 3x3 pad 1 on 5x7 / 7x5, stride 1 and 2, one and three images (M = 105: an image
    # boundary inside a 16-pixel fragment, the last tile partial); C = 64: 18 K-steps, a K-split slice
    # starts in the middle of a filter tap at kw = 4 and 8
    Case("3x3-5x7-n3", "fast", 3, 5, 7, 64, 64, 3, 3, 1, 1, res=True),
    Case("3x3-7x5-n3", "fast", 3, 7, 5, 64, 96, 3, 3, 1, 1, act="none", out_f32=True),
    Case("3x3-5x7-n1", "fast", 1, 5, 7, 32, 40, 3, 3, 1, 1, act="tanh"),
    Case("3x3-7x5-n1", "fast", 1, 7, 5, 64, 64, 3, 3, 1, 1, res=True, out_f32=True),
    Case("3x3s2-5x7-n3", "fast", 3, 5, 7, 64, 64, 3, 3, 2, 1),
    Case("3x3s2-7x5-n3", "fast", 3, 7, 5, 32, 96, 3, 3, 2, 1, res=True, act="none"),
    Case("3x3s2-5x7-n1", "fast", 1, 5, 7, 64, 4, 3, 3, 2, 1, res=True),
    Case("3x3s2-7x5-n1", "fast", 1, 7, 5, 64, 64, 3, 3, 2, 1, out_f32=True),
    Case("1x1s2-6x9", "fast", 3, 6, 9, 64, 96, 1, 1, 2, 0, res=True),             # downsample
    Case("1x3-5x7", "fast", 3, 5, 7, 32, 64, 1, 3, 1, 1, res=True),               # R != S
    Case("3x1-7x5", "fast", 3, 7, 5, 32, 64, 3, 1, 1, 1, act="none", out_f32=True),
    Case("1x3s2-7x5", "fast", 1, 7, 5, 64, 40, 1, 3, 2, 1),
    # generic (plain NHWC, C = 8 and 16)
    Case("7x7s2-c8", "generic", 3, 9, 11, 8, 64, 7, 7, 2, 3),                     # the stem's geometry
    Case("3x3-c16", "generic", 3, 5, 7, 16, 40, 3, 3, 1, 1, res=True, out_f32=True),
    Case("1x3-c8", "generic", 3, 5, 7, 8, 64, 1, 3, 1, 1, act="none"),
    Case("3x1-c16", "generic", 1, 7, 5, 16, 96, 3, 1, 2, 1, res=True),
    Case("1x1-c8", "generic", 1, 7, 5, 8, 4, act="tanh"),
    # F32IN: fp32 input, ReLU and the bf16 rounding at the load
    Case("f32in-1x1", "f32in1x1", 3, 5, 7, 64, 64, x_f32=True, res=True),
    Case("f32in-1x1-pix1", "f32in1x1", 1, 1, 1, 32, 96, x_f32=True, act="none", out_f32=True),
    Case("f32in-3x3", "f32in3x3", 3, 5, 7, 64, 64, 3, 3, 1, 1, x_f32=True, res=True),
    Case("f32in-3x3s2", "f32in3x3", 1, 7, 5, 32, 96, 3, 3, 2, 1, x_f32=True, act="none", out_f32=True),
]
# XROW: K = 40 (% 8, not % 32), ldx = K + 8, ldo = Cout + 8, bias = NULL, the four activations
XROW_CASES = [
    Case(f"xrow-{act}", "xrow", 37, 1, 1, 40, 40, act=act, xrow=True, ldx_pad=8, ldo_pad=8, res=i % 2 == 0,
         out_f32=i >= 2, bias=i != 1, row_pad=CV.GEMM_ROW_PAD)
    for i, act in enumerate(CV.ACT)
] + [Case("xrow-k96-n4", "xrow", 105, 1, 1, 96, 4, act="none", xrow=True, ldx_pad=8, row_pad=CV.GEMM_ROW_PAD),
     Case("xrow-m1", "xrow", 1, 1, 1, 64, 132, act="gelu", xrow=True, ldo_pad=8, res=True, row_pad=CV.GEMM_ROW_PAD)]
# K-step counts around the ring depth and kw: a 1x1 conv of C = 32 * ksteps on a 5x7 image
KSTEP_CASES = {k: Case(f"ksteps-{k}", "fast1x1", 1, 5, 7, 32 * k, 64, res=k % 2 == 1, out_f32=k % 3 == 0,
                       act=("relu", "none")[k % 2]) for k in KSTEPS_ALL}
RING_CASES = CONV_CASES + XROW_CASES + list(KSTEP_CASES.values())
KINDS = ("rand", "exact")


def exact_ok(case):
    """Integer-valued operands predict the output to the bit for none and relu only."""
    return case.act in ("none", "relu")


# --- csrc/gemm.hip, GEMM mode: every cfg of CV.LDS_TILES
GEMM_K = (64, 128, 192, 256, 320)    # nst = 1 .. 5, around NS - 1 for 2, 3 and 4 stages
GEMM_VARIANTS = [  # (act, res, out_f32, ldx_pad, ldo_pad), rotated over the (M, K, N) grid
    ("none", False, False, 8, 8), ("relu", True, False, 8, 8), ("gelu", False, True, 8, 8),
    ("tanh", True, False, 8, 8), ("relu", False, True, 0, 8), ("none", True, True, 8, 0),
    ("gelu", True, False, 0, 0),
]


def gemm_widths(cfg):
    """N in {4, 132, one full plus one partial tile}, and what else ``lds_fits`` needs for two widths."""
    bn = CV.LDS_TILES[cfg][1]
    out = [nn for nn in (4, 132, bn + 36) if CV.lds_fits(cfg, nn)]
    hi = [nn for nn in range(bn + 4, 2 * bn + 1, 4) if CV.lds_fits(cfg, nn)]   # one full plus one partial tile
    lo = [nn for nn in range(bn - 28, bn + 1, 4) if CV.lds_fits(cfg, nn)]       # one partial tile
    more = hi[:1] + lo[:1] + hi[1:]
    while len(set(out)) < 2:
        out.append(more.pop(0))
    return sorted(set(out))


def gemm_ms(cfg):
    return (64, CV.LDS_TILES[cfg][0] + 9, 577)


def gemm_case(M, K, N, v):
    act, res, f32, lx, lo = GEMM_VARIANTS[v % len(GEMM_VARIANTS)]
    return Case(f"gemm-{M}x{K}x{N}-v{v % len(GEMM_VARIANTS)}", "gemm", M, 1, 1, K, N, act=act, res=res, out_f32=f32,
                xrow=True, ldx_pad=lx, ldo_pad=lo, row_pad=CV.GEMM_ROW_PAD)


def gemm_cases(cfg):
    """Every (M, K, N) of ``cfg``; the variant rotates with the position in the grid."""
    out = []
    for im, M in enumerate(gemm_ms(cfg)):
        for ik, K in enumerate(GEMM_K):
            for iw, N in enumerate(gemm_widths(cfg)):
                out.append(gemm_case(M, K, N, im * 3 + ik + iw * 2))
    return out


@functools.lru_cache(maxsize=None)
def all_gemm_cases():
    seen = {}
    for cfg in CV.LDS_TILES:
        for c in gemm_cases(cfg):
            seen[c.name] = c
    return list(seen.values())


# --- csrc/gemm.hip, CV mode: LDS_CONV_CFGS
_CV_GEOM = [  # name, n, h, w, cin, r, s, stride, pad, act, res, out_f32
    ("3x3-5x7-n3", 3, 5, 7, 64, 3, 3, 1, 1, "relu", True, False),
    ("3x3s2-7x5-n1", 1, 7, 5, 128, 3, 3, 2, 1, "none", False, True),     # M = 12 < BM
    ("3x3s2-5x7-n3", 3, 5, 7, 64, 3, 3, 2, 1, "relu", False, False),
    ("3x3-7x5-n1", 1, 7, 5, 128, 3, 3, 1, 1, "relu", True, True),
    ("1x1-5x7-n3", 3, 5, 7, 64, 1, 1, 1, 0, "relu", True, False),        # K = 64: nst = 1
    ("1x1s2-7x5-n3", 3, 7, 5, 128, 1, 1, 2, 0, "none", True, False),
    ("1x3-5x7-n1", 1, 5, 7, 64, 1, 3, 1, 1, "relu", False, True),
    ("3x1-7x5-n3", 3, 7, 5, 64, 3, 1, 1, 1, "none", True, False),
]
CV_CASES = [Case(f"cv-{g[0]}-co{co}", "cv", g[1], g[2], g[3], g[4], co, g[5], g[6], g[7], g[8], g[9], g[10], g[11])
            for g in _CV_GEOM for co in (64, 128, 256)]


def cv_cases(cfg):
    bn = CV.LDS_TILES[cfg][1]
    return [c for c in CV_CASES if c.cout in (bn, 2 * bn)]


def all_cases():
    return RING_CASES + all_gemm_cases() + CV_CASES
