"""fp32 / fp64 oracles of the fused ResNet kernels of csrc/block.hip (``bneck_kernel``,
``bneck2_kernel``, ``bneck2d_kernel``, ``stem_kernel``), an element-wise comparator with a derived
bound, and the inputs of every per-kernel GPU case, built deterministically on the CPU so that
tests/test_block_oracle_cpu.py can judge the oracle on exactly what tests/test_block_kernels_gpu.py
runs. Torch only, CPU only. Not a test module.

The comparator: an element passes iff ``|got - ref| <= 2**-7 * |ref| + 2**-7 * A`` where ``A`` is the
absolute-value companion of the last conv at that element (every product and the bias replaced by
its magnitude). 2**-7 is one bf16 ulp (relative, at the bottom of a binade), so the bound allows one
ulp on the stored output plus one ulp on every operand of the last conv: the intermediate the last
conv reads is itself a bf16 rounding of a sum whose fp32 order differs between kernel and oracle.
fp32 accumulation order is orders of magnitude below it (K <= 1152 terms at 2**-24 each). There is
no share of elements that may fail and no whole-tensor scale in it.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from hipzap.ops import conv as CV

ULP = 2.0 ** -7  # one bf16 ulp, relative

Ref = namedtuple("Ref", "y A t1 t2 r")              # NHWC; y unrounded, A the magnitude companion
StemRef = namedtuple("StemRef", "y A image so")     # image: the bf16 NHWC8 tensor stem mode 2 reads
Report = namedtuple("Report", "ok ratio n tile pixel channel got ref bound bad")


def _bf16(t):
    """Round to bf16 (nearest even) and back. (A float64 goes through float32 first: double rounding
    can move a value that sits within 2**-24 of a bf16 tie by one ulp, which the bound covers.)"""
    return t.to(torch.bfloat16).to(t.dtype)


def _ident(t):
    return t


def _w(pc, dtype):
    """[cout, r, s, cin] bf16-dense packed weights and [cout] bias in ``dtype``."""
    return pc.dense().reshape(pc.cout, pc.r, pc.s, pc.cin).to(dtype), pc.bias.to(dtype)


def bneck_ref(x, p1, p2, p3, pd=None, stride=1, dtype=torch.float32, hooks=None):
    """One bottleneck block as the fused kernels compute it, on the bf16-dense packed weights
    (``pc.dense()``, ``pc.bias``), in ``dtype`` (float32 or float64). ``x``: [N, H, W, Cin] NHWC holding
    bf16 values.

        t1  = bf16(relu(W1 x + b1))
        t2  = bf16(relu(conv3x3(t1, zero padded, stride) + b2))
        acc = W3 t2 + b3 + r        r = x (identity), or Wd x(::stride) + bd (downsample), fp32, unrounded
        y   = relu(acc)             (the kernel then stores bf16(y): the comparator's first term)

    Rounding points, read in csrc/block.hip:
    * t1 is bf16 in LDS: ``pack2`` at line 397 (bneck_kernel), 668 (bneck2_kernel), 870-871
      (bneck2d_kernel); halo pixels outside the image are written as zero there (lines 393-396, 664-667,
      866-869), which is conv2's zero padding -- zero, not relu(b1).
    * t2 is bf16 in LDS: ``pack2`` at line 452, 696-697, 899-900.
    * the identity residual is the bf16 input, widened and added to the fp32 accumulator: 523-528,
      740-743.
    * the downsample is NOT rounded: its MFMAs run into conv3's accumulators (503-511; 929-944) and its
      bias is added to conv3's in fp32 (356; 810-811). The per-conv program stores it as bf16 first.
    * y is rounded once, at the store: 532, 747, 956.
    * bneck2d_kernel reads the downsample input at halo position (2jy + 1, 2jx + 1) with the halo
      origin at (2 y0 - 1, 2 x0 - 1), i.e. input pixel (2y, 2x): line 907.

    ``A = |W3| t2 + |b3| + |r|``, with ``|Wd| |x| + |bd|`` for ``|r|`` in a downsample block.

    ``hooks`` edits the computation (planted faults, the per-conv rounding of r): ``t1_padded`` gets the
    zero-padded NCHW t1 that conv2 reads, ``t2`` the NHWC t2, ``xd`` the input and returns what the
    downsample samples, ``r`` the NHWC residual."""
    h = hooks or {}
    xs = x.to(dtype)
    (w1, b1), (w2, b2), (w3, b3) = _w(p1, dtype), _w(p2, dtype), _w(p3, dtype)
    t1 = _bf16(torch.relu(xs @ w1.reshape(p1.cout, -1).t() + b1))
    t1p = h.get("t1_padded", _ident)(F.pad(t1.permute(0, 3, 1, 2), (1, 1, 1, 1)))
    t2 = _bf16(torch.relu(F.conv2d(t1p, w2.permute(0, 3, 1, 2), b2, stride=stride))).permute(0, 2, 3, 1)
    t2 = h.get("t2", _ident)(t2)
    if pd is None:
        assert stride == 1
        r, absr = xs, xs.abs()
    else:
        wd, bd = _w(pd, dtype)
        wd = wd.reshape(pd.cout, -1)
        xd = h.get("xd", lambda t: t[:, ::stride, ::stride])(xs)
        r, absr = xd @ wd.t() + bd, xd.abs() @ wd.abs().t() + bd.abs()
    r = h.get("r", _ident)(r)
    w3 = w3.reshape(p3.cout, -1)
    acc = t2 @ w3.t() + b3 + r
    A = t2.abs() @ w3.abs().t() + b3.abs() + absr
    return Ref(torch.relu(acc), A, t1, t2, r)


def stem_ref(img, pc, mean, inv_std, mode, dtype=torch.float32, hooks=None):
    """``stem_kernel``: normalise, round to bf16 as the preprocess kernel does, 7x7/2 pad 3 conv + bias
    + ReLU, 3x3/2 pad 1 max-pool. ``img``: fp32 NCHW (mode 0) or uint8 NHWC (modes 1 and 2); ``mean`` /
    ``inv_std``: three float32 values each, or None for no normalisation.

    The normalisation is float32 whatever ``dtype`` is, operation by operation what the kernels do
    (csrc/vision.hip preprocess_kernel, csrc/block.hip lines 164-174: ``u8 * (1.0f / 255.0f)``, then
    ``(v - mean) * inv_std``, then ``pack8`` = bf16): it defines the conv's bf16 operand, so it is
    bit-exact, not approximate. The conv's outputs are rounded to bf16 in LDS before the pool (line
    235); rounding is monotonic, so the pooled value is the rounding of the pooled exact value and the
    oracle leaves it unrounded like every ``y`` here.

    ``A`` of a conv output is ``|W| |x| + |b|``; a pooled element takes the largest ``A`` of its window:
    |max_i got_i - max_i ref_i| <= max_i |got_i - ref_i| <= 2**-7 (max_i |ref_i| + max_i A_i), and
    max_i |ref_i| is the pooled reference itself (every ref_i >= 0).

    ``hooks['pool']`` gets the NCHW conv output and returns the pooled one (planted fault)."""
    h = hooks or {}
    if mode == 0:
        v = img.float().permute(0, 2, 3, 1)
    else:
        v = img.float() * torch.tensor(1.0 / 255.0, dtype=torch.float32)
    if mean is not None:
        v = (v - torch.tensor(mean, dtype=torch.float32)) * torch.tensor(inv_std, dtype=torch.float32)
    xb = v.to(torch.bfloat16)
    w, b = _w(pc, dtype)
    w = w[..., :3].permute(0, 3, 1, 2)  # (cin_pad 8: channels 3..7 of the image are zero)
    xs = xb.to(dtype).permute(0, 3, 1, 2)
    so = torch.relu(F.conv2d(xs, w, b, stride=2, padding=3))
    a_so = F.conv2d(xs.abs(), w.abs(), b.abs(), stride=2, padding=3)
    y = h.get("pool", lambda t: F.max_pool2d(t, 3, 2, 1))(so)
    A = F.max_pool2d(a_so, 3, 2, 1)
    return StemRef(y.permute(0, 2, 3, 1), A.permute(0, 2, 3, 1), F.pad(xb, (0, 5)), so.permute(0, 2, 3, 1))


def bound(ref, A):
    return ULP * ref.abs() + ULP * A


def compare(got, ref, A, tile=(8, 8)) -> Report:
    """Element-wise ``|got - ref| <= bound(ref, A)`` over NHWC tensors; the worst element (largest
    err / bound; a NaN counts as infinitely bad) as (image, (tile row, tile column), (row, column in
    the tile), channel) for ``tile`` = the kernel's output tile (rows, columns)."""
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    got, ref, A = got.double(), ref.double(), A.double()
    err, bnd = (got - ref).abs(), bound(ref, A)
    bad = ~(err <= bnd)  # (NaN: bad)
    ratio = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err / bnd.clamp_min(1e-300))
    k = int(ratio.reshape(-1).argmax())
    n, y, x, c = (int(v) for v in torch.unravel_index(torch.tensor(k), ratio.shape))
    th, tw = tile
    return Report(not bool(bad.any()), float(ratio.reshape(-1)[k]), n, (y // th, x // tw), (y % th, x % tw), c,
                  float(got[n, y, x, c]), float(ref[n, y, x, c]), float(bnd[n, y, x, c]), int(bad.sum()))


def describe(rep: Report) -> str:
    return (f"worst err/bound {rep.ratio:.3f} at image {rep.n} tile {rep.tile} pixel {rep.pixel} channel "
            f"{rep.channel}: got {rep.got:.6g}, ref {rep.ref:.6g}, bound {rep.bound:.3g}; {rep.bad} outside")


def check(got, ref, A, tile=(8, 8), label="") -> Report:
    rep = compare(got, ref, A, tile)
    print(f"[block_oracle] {label}: {describe(rep)}")
    assert rep.ok, f"{label}: {describe(rep)}"
    return rep


def old_metric(got, ref) -> float:
    """The whole-tensor metric of tests/test_fused_gpu.py (max |err| / max |ref|, passes below 2e-2)."""
    return (got.double() - ref.double()).abs().max().item() / max(ref.double().abs().max().item(), 1e-6)


# ------------------------------------------------------------------------------------------------
# the per-kernel GPU cases and their inputs
# kind -> (Cin, Cmid, Cout, downsample, stride, output tile)
KINDS = {"l1ds": (64, 64, 256, True, 1, (8, 8)), "l1id": (256, 64, 256, False, 1, (8, 8)),
         "l2id": (512, 128, 512, False, 1, (4, 4)), "l2ds": (256, 128, 512, True, 2, (4, 4))}
# bneck_kernel: (N, H, W) -- one tile whose whole halo is outside the image; non-square with interior
# tile borders both ways; more than one image. Each with 8- and 4-row tiles (at 8 x 8 the 4-row tiles
# share a row border).
BNECK_SHAPES = [(1, 8, 8), (1, 16, 24), (2, 8, 16)]
BNECK_TILE_H = [8, 4]
# bneck2_kernel / bneck2d_kernel: (N, H, W, imgs), H x W the block's OUTPUT size
BNECK2_CASES = [(1, 4, 4, 1), (1, 8, 12, 1), (2, 4, 8, 1), (2, 4, 8, 2), (4, 4, 4, 2)]
BNECK2D_CASES = [(1, 4, 4, 1), (1, 8, 12, 1), (2, 4, 4, 2), (2, 8, 4, 1)]
# stem_kernel: the launcher's minimum (one partial tile); W * 3 no multiple of 16 with odd SH / SW and
# partial last tiles both ways (30 x 36: stem 15 x 18, 34 x 44: 17 x 22); several whole tiles (32 x 40)
STEM_SIZES = [(8, 8), (30, 36), (34, 44), (32, 40)]
STEM_MODES = [0, 2]
STEM_BATCHES = [1, 2]
STEM_TILE = (4, 8)


def _pack(g, cout, cin, k, stride=1, pad=0, cin_pad=None):
    """He-scaled weights, biases of about +0.1 (none near zero: a missing bias, or relu(b1) in place of
    the zero padding, moves every element it touches)."""
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = 0.1 + 0.03 * torch.randn(cout, generator=g)
    return CV.pack_conv(w, b, None, stride, pad, cin_pad=cin_pad)


@functools.lru_cache(maxsize=None)
def bneck_weights(kind):
    """(p1, p2, p3, pd or None) of a block kind, CPU-packed."""
    cin, cm, co, ds, stride, _ = KINDS[kind]
    g = torch.Generator().manual_seed(1000 + sorted(KINDS).index(kind))
    p1, p2, p3 = _pack(g, cm, cin, 1), _pack(g, cm, cm, 3, stride, 1), _pack(g, co, cm, 1)
    return p1, p2, p3, (_pack(g, co, cin, 1, stride, 0) if ds else None)


@functools.lru_cache(maxsize=None)
def bneck_input(kind, n, h, w):
    """The block input for an ``h x w`` OUTPUT: [n, stride*h, stride*w, Cin] bf16, non-negative (a block
    input is a ReLU's or the max-pool's output)."""
    cin, _, _, _, stride, _ = KINDS[kind]
    g = torch.Generator().manual_seed(100000 * sorted(KINDS).index(kind) + 1000 * n + 10 * h + w)
    return torch.relu(torch.randn(n, stride * h, stride * w, cin, generator=g)).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def bneck_case(kind, n, h, w, dtype=torch.float64):
    """(x, weights, Ref in ``dtype``) of a GPU case; computed once and shared, never modified."""
    x, ws = bneck_input(kind, n, h, w), bneck_weights(kind)
    return x, ws, bneck_ref(x, *ws, stride=KINDS[kind][4], dtype=dtype)


@functools.lru_cache(maxsize=None)
def stem_weights():
    return _pack(torch.Generator().manual_seed(2000), 64, 3, 7, 2, 3, cin_pad=8)


def stem_norm():
    """(mean, inv_std) as engine/fusion.py stem_params hands them to the kernel: float32 constants,
    inv_std = 1 / std in float32."""
    import numpy as np

    from hipzap.ops.vision import IMAGENET_MEAN, IMAGENET_STD
    inv = (np.float32(1.0) / np.asarray(IMAGENET_STD, dtype=np.float32)).astype(np.float32)
    return [float(np.float32(m)) for m in IMAGENET_MEAN], [float(v) for v in inv]


@functools.lru_cache(maxsize=None)
def stem_input(mode, n, h, w):
    """mode 0: fp32 NCHW in [0, 1] (normalised in the kernel); mode 2: the uint8 HWC request whose
    preprocessed bf16 NHWC8 image (StemRef.image) the kernel reads."""
    g = torch.Generator().manual_seed(10000 * mode + 1000 * n + 10 * h + w)
    if mode == 0:
        return torch.rand(n, 3, h, w, generator=g)
    x = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=g)
    x.view(-1)[0], x.view(-1)[1], x.view(-1)[-1] = 0, 255, 255
    return x


@functools.lru_cache(maxsize=None)
def stem_case(mode, n, h, w, dtype=torch.float64):
    img = stem_input(mode, n, h, w)
    mean, inv_std = stem_norm()
    return img, stem_ref(img, stem_weights(), mean, inv_std, mode, dtype=dtype)
