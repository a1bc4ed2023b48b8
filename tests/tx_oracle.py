"""fp32 / fp64 oracles of the transformer kernels of csrc/transformer.hip (``layernorm_kernel``,
``embed_ln_kernel``, ``attention_kernel``, ``attention_stream_kernel``, ``qkvatt_kernel``,
``vit_tokens_kernel``, ``softmax_kernel``), element-wise comparators with derived bounds, and the inputs
of every per-kernel GPU case, built deterministically on the CPU so that tests/test_tx_oracle_cpu.py
judges the oracles on exactly what tests/test_tx_kernels_gpu.py runs. Torch only, CPU only. Not a test
module.

LayerNorm and the embeddings: an element passes iff

    |got - ref| <= ulp_bf16(ref) / 2 + C_LN * 2**-24 * (rstd |gamma| (|v - mean| + max_row |v|) + |beta|)

The first term is the one rounding, at the store (``pack8``: transformer.hip line 113, line 197 for the
embeddings); everything before it is fp32 on bf16 operands, which the second term covers. An error in
the mean is amplified by ``rstd |gamma|`` whatever the element's own size, so the term carries
``max_row |v|``. No whole-tensor scale, no share of elements that may fail.

``C_LN`` from the operation count (u = 2**-24; n_v roundings in ``v``: 1 for ``x + res`` at line 82, 2
for ``word + pos + type`` at line 170):

* the row sum (lines 85 and 88, 171 and 175): at most 32 serial adds per lane (four 8-element chunks),
  6 shuffle steps (``warp_sum``) and the division: |d mean| <= (n_v + 39) u max|v|;
* ``d = v - mean`` (lines 96, 110): |dd| <= (2 n_v + 39) u max|v| + u |d|;
* the variance (lines 97-101): a product, the same 38-deep sum, the division and ``+ eps``: 43 u
  relative; the common error of the mean cancels to first order (sum d = 0), the per-element rounding
  of ``v`` does not: 2 n_v u max|v| rstd relative;
* ``rsqrtf`` (line 101): 1 ulp = 2 u; so rstd carries 23.5 u + n_v u max|v| rstd relative;
* ``d * rstd * gamma + beta`` (lines 110-111, 196): two multiplies and an add (or a multiply and an
  FMA): 2 u relative on the product and u |y| on the sum.

Together |dy| <= u (rstd |gamma| ((2 n_v + 39 + n_v z) max|v| + 28.5 |d|) + |beta|) with z = |d| rstd
<= sqrt(D) <= 45.3: a worst case of ``C_OPS`` = 134 at n_v = 2, D = 2048. That is every rounding at
its largest and all of one sign; what fp32 really differs from fp64 by on the cases here is measured in
tests/test_tx_oracle_cpu.py (torch's own order, which depends on the host's vector width, and the
kernel's order, ``layernorm_emul``): worst 1.46 of ``2**-24 * S`` on one host and 1.59 on another
(embed-D2048-notypes both times). ``C_LN`` = 8 is the larger with a factor of 4 (6.36), rounded up to
a power of two, far inside the worst case.

Attention (``attention_kernel``, ``attention_stream_kernel``, ``qkvatt_kernel``): an element passes iff

    |got - ref| <= 2**-7 |ref| + 2**-7 A,      A = softmax(s) |V|

one bf16 ulp on the store (lines 386, 575, 785) and one on every ``p_k``: P is rounded to bf16 before
the P.V MFMA (lines 341-342 and 766-767 after the normalisation, lines 519-520 before it).
"""
import functools
from collections import namedtuple
from types import SimpleNamespace

import torch

import att_stream_inputs as I
from hipzap.ops import conv as CV

ULP = 2.0 ** -7    # one bf16 ulp, relative (at the bottom of a binade)
U32 = 2.0 ** -24   # half an fp32 ulp, relative: one fp32 rounding
C_OPS = 134.0      # worst case of the operation count (module docstring)
C_LN = 8.0         # 4 x the worst measured fp32-against-fp64 figure (1.59; tests/test_tx_oracle_cpu.py)

LNRef = namedtuple("LNRef", "y S")          # y unrounded; S the scale of the fp32 term
AttRef = namedtuple("AttRef", "y A")        # [B*L, heads*64]; y unrounded, A = softmax(s) |V|
Report = namedtuple("Report", "ok ratio row head column got ref bound bad")


def _bf16(t):
    """Round to bf16 (nearest even) and back. (A float64 goes through float32 first: double rounding
    can move a value that sits within 2**-24 of a bf16 tie by one ulp, which the bounds cover.)"""
    return t.to(torch.bfloat16).to(t.dtype)


def ulp_bf16(t):
    """The spacing of bf16 numbers in the binade of ``|t|`` (float64)."""
    _, e = torch.frexp(t.double().abs().clamp_min(2.0 ** -126))  # |t| = m 2**e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - 8)


# ------------------------------------------------------------------------------------------------
# LayerNorm, embeddings
def _ln(v, gamma, beta, eps, hooks=None):
    h = hooks or {}
    dtype = v.dtype
    g, b = gamma.to(dtype), beta.to(dtype)
    e = torch.tensor(eps, dtype=torch.float32).to(dtype)  # the kernel's operand: eps as a float
    mean = v.mean(-1, keepdim=True)
    d = v - mean
    var = h.get("var", lambda q, D: q / D)((d * d).sum(-1, keepdim=True), v.shape[-1])  # two-pass, biased
    rstd = 1.0 / torch.sqrt(var + h.get("eps", lambda t: t)(e))
    y = d * rstd * g + b
    S = rstd * g.abs() * (d.abs() + v.abs().amax(-1, keepdim=True)) + b.abs()
    return LNRef(y, S)


def layernorm_ref(x, gamma, beta, eps, residual=None, dtype=torch.float64, hooks=None):
    """``layernorm_kernel``: ``x`` [rows, D] (and ``residual``) hold bf16 values, widened to ``dtype``; the
    residual is added unrounded (the kernel: one fp32 add, line 82); two-pass biased variance (lines
    88-101); ``y = (v - mean) rstd gamma + beta`` unrounded (the kernel then stores bf16(y), line 113:
    the bound's first term). ``hooks`` plants faults: ``var`` gets (sum d^2, D), ``eps`` gets eps."""
    v = x.to(dtype)
    if residual is not None:
        v = v + residual.to(dtype)
    return _ln(v, gamma, beta, eps, hooks)


def embed_ln_ref(ids, types, tables, gamma, beta, eps, L, vocab, ntypes, dtype=torch.float64):
    """``embed_ln_kernel``: row r = word[clamp(ids[r], 0, vocab-1)] + pos[r % L] + type[clamp(types[r],
    0, ntypes-1)] (lines 151-153: the clamps are the contract; ``types`` None = type row 0), the three
    rows added unrounded (line 170: two fp32 adds), then LayerNorm as above (lines 175-196), unrounded.
    ``tables`` = (word, pos, type), bf16."""
    word, pos, typ = tables
    ids = ids.reshape(-1).long()
    rows = ids.numel()
    tok = ids.clamp(0, vocab - 1)
    tt = torch.zeros(rows, dtype=torch.long) if types is None else types.reshape(-1).long().clamp(0, ntypes - 1)
    v = word.to(dtype)[tok] + pos.to(dtype)[torch.arange(rows) % L] + typ.to(dtype)[tt]
    return _ln(v, gamma, beta, eps)


def layernorm_emul(v, gamma, beta, eps):
    """Not an oracle: ``layernorm_kernel`` / ``embed_ln_kernel``'s fp32 arithmetic in the kernel's own
    order, on the fp32 row ``v`` (= x + res, or the three table rows added left to right): lane l holds
    the 8-element chunks l, l + 64, ..., adds their elements serially (lines 85, 97), then the xor
    butterfly of ``warp_sum`` (common.h). Unrounded fp32 ``y``. (A product the compiler contracts into an
    FMA is one rounding fewer than here.)"""
    rows, D = v.shape
    nc = (D // 8 + 63) // 64
    vv = torch.zeros(rows, nc * 512, dtype=torch.float32)
    vv[:, :D] = v.float()
    live = (torch.arange(nc * 512) < D).reshape(1, nc, 64, 8)
    vv = vv.reshape(rows, nc, 64, 8)
    lanes = torch.arange(64)

    def warp_sum(fn):
        s = torch.zeros(rows, 64)
        for c in range(nc):
            for e in range(8):
                s = s + fn(vv[:, c, :, e], live[:, c, :, e])
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        return s[:, :1]

    mean = warp_sum(lambda t, on: t) / D
    q = warp_sum(lambda t, on: torch.where(on, (t - mean) * (t - mean), torch.zeros(())))
    rstd = torch.rsqrt(q / D + torch.tensor(eps, dtype=torch.float32))
    d = vv.reshape(rows, -1)[:, :D] - mean
    return d * rstd * gamma.float() + beta.float()


def ln_bound(ref: LNRef, c=C_LN):
    return ulp_bf16(ref.y) / 2 + c * U32 * ref.S.double()


def fp32_term(ref: LNRef, c=C_LN):
    return c * U32 * ref.S.double()


def ulp_e4m3(t):
    """The spacing of e4m3fn numbers in the binade of ``|t|`` (subnormals below 2**-6: 2**-9)."""
    _, e = torch.frexp(t.double().abs().clamp_min(2.0 ** -6))
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - 4)


# ------------------------------------------------------------------------------------------------
# attention
def attention_ref(qkv, B, L, heads, mask=None, scale=0.125, k_off=None, v_off=None, dtype=torch.float64,
                  hooks=None):
    """softmax(s) V per (sequence, head) over the L real keys (padding keys do not exist here), head dim
    64. ``qkv``: [B*L, ld] bf16 values, Q of head h at columns h*64, K at ``k_off`` + h*64, V at ``v_off``
    + h*64 (default: packed, k_off = D, v_off = 2D). ``mask``: additive, [B, L] over the keys, or None.

    ``s = fp32(q.k * scale) + mask`` with the mask add in float32 whatever ``dtype`` is (the kernels:
    ``s * p.scale + madd`` in fp32, lines 308, 490, 736): at -1e9 that add absorbs the score entirely,
    which DEFINES a fully masked sequence as the uniform mean of V -- part of the operand, not an
    approximation. -inf keys get probability 0; a row of nothing but -inf is undefined (line 409).

    Returns ``(y, A)``, both [B*L, heads*64] and unrounded: ``y = softmax(s) V``, ``A = softmax(s) |V|``.
    ``hooks`` plants faults: ``s`` gets the masked scores [B, heads, L, keys], ``p`` the probabilities,
    ``pad_keys`` = n counts n padding keys (copies of key L-1, as the kernels stage them) with mask 0."""
    h = hooks or {}
    D = heads * 64
    k_off = D if k_off is None else k_off
    v_off = 2 * D if v_off is None else v_off
    t = qkv.to(dtype)
    q, k, v = (t[:, o:o + D].reshape(B, L, heads, 64).permute(0, 2, 1, 3) for o in (0, k_off, v_off))
    madd = torch.zeros(B, L) if mask is None else mask.float().reshape(B, L)
    n = h.get("pad_keys", 0)
    if n:
        k = torch.cat([k] + [k[:, :, -1:]] * n, 2)
        v = torch.cat([v] + [v[:, :, -1:]] * n, 2)
        madd = torch.cat([madd, torch.zeros(B, n)], 1)
    s = ((q @ k.transpose(-1, -2)) * scale).float() + madd[:, None, None, :]
    s = h.get("s", lambda a: a)(s)
    p = h.get("p", lambda a: a)(torch.softmax(s.to(dtype), -1))
    flat = lambda a: a.permute(0, 2, 1, 3).reshape(B * L, D)  # noqa: E731
    return AttRef(flat(p @ v), flat(p @ v.abs()))


def qkvatt_ref(x, pc, mask, B, L, heads, dtype=torch.float64, hooks=None):
    """``qkvatt_kernel``: Q, K, V = bf16(x W^T + b) on the bf16-dense packed weights (``pc.dense()``,
    ``pc.bias``) in ``dtype`` (the kernel: fp32 MFMA accumulators + bias, ``pack_bf16x2`` into the LDS
    images, lines 698-700), then ``attention_ref`` at scale 1/8. ``x``: [B*L, >= D] bf16."""
    D = heads * 64
    qkv = _bf16(x[:, :D].to(dtype) @ pc.dense().to(dtype).t() + pc.bias.to(dtype))
    return attention_ref(qkv, B, L, heads, mask, 0.125, dtype=dtype, hooks=hooks)


def att_bound(ref: AttRef):
    return ULP * ref.y.double().abs() + ULP * ref.A.double()


def attention_onepass_emul(qkv, B, L, heads, mask=None):
    """Not an oracle: ``attention_kernel``'s arithmetic on packed ``qkv`` -- fp32 scores, softmax
    normalised in fp32, P rounded to bf16 AFTER the normalisation (lines 341-342), fp32-accumulated P.V,
    bf16 store."""
    D = heads * 64
    q, k, v = qkv.float().reshape(B, L, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    if mask is not None:
        s = s + mask.float().reshape(B, 1, 1, L)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    p = (e * (1.0 / e.sum(-1, keepdim=True))).to(torch.bfloat16).float()
    return (p @ v).permute(0, 2, 1, 3).reshape(B * L, D).to(torch.bfloat16)


def vit_tokens_ref(patches, cls, pos, B, npatch):
    """``vit_tokens_kernel``, bitwise: out[b][0] = bf16(cls + pos[0]), out[b][1+i] = bf16(patches[b*np+i] +
    pos[1+i]), one fp32 add of two bf16 values (line 805) and one rounding (line 806)."""
    D = patches.shape[-1]
    a = torch.cat([cls.reshape(1, 1, D).expand(B, 1, D), patches.reshape(B, npatch, D)], 1)
    return (a.float() + pos.float()[None]).to(torch.bfloat16).reshape(B * (npatch + 1), D)


# ------------------------------------------------------------------------------------------------
# the comparator
def compare(got, ref, bound, head_dim=None) -> Report:
    """Element-wise ``|got - ref| <= bound`` over [rows, columns] tensors; every ``got`` must be finite. The
    worst element (largest err / bound; a NaN or an infinity counts as infinitely bad) as (row, head,
    column in the head) for ``head_dim`` columns per head (None: one head)."""
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    got, ref, bound = got.double(), ref.double(), bound.double()
    err = (got - ref).abs()
    bad = ~(err <= bound) | ~torch.isfinite(got)
    ratio = torch.where(torch.isfinite(err), err / bound.clamp_min(1e-300), torch.full_like(err, float("inf")))
    k = int(ratio.reshape(-1).argmax())
    r, c = k // got.shape[1], k % got.shape[1]
    hd = head_dim or got.shape[1]
    return Report(not bool(bad.any()), float(ratio[r, c]), r, c // hd, c % hd, float(got[r, c]), float(ref[r, c]),
                  float(bound[r, c]), int(bad.sum()))


def describe(rep: Report) -> str:
    return (f"worst err/bound {rep.ratio:.3f} at row {rep.row} head {rep.head} column {rep.column}: got "
            f"{rep.got:.6g}, ref {rep.ref:.6g}, bound {rep.bound:.3g}; {rep.bad} outside")


def check(got, ref, bound, head_dim=None, label="") -> Report:
    rep = compare(got, ref, bound, head_dim)
    print(f"[tx_oracle] {label}: {describe(rep)}")
    assert rep.ok, f"{label}: {describe(rep)}"
    return rep


# ------------------------------------------------------------------------------------------------
# the per-kernel GPU cases and their inputs. Every builder is cached: computed once, shared, never
# modified.
# LayerNorm (rows, D): one chunk on one lane; one chunk per lane at most (64); two full chunks (768: NC
# 2); 520: nch = 65, the second chunk has one live lane; 1024: NC 2 full; 1032: the first NC 3 width;
# 1536: NC 3 full; 2048: NC 4 full
LN_SHAPES = [(1, 8), (5, 64), (5, 768), (9, 520), (7, 1024), (6, 1032), (5, 1536), (3, 2048)]


def _ln_rows(g, rows, ld, const):
    """Row 1: mean 100, std 1; row 2: constant; row 3: small; row 4: large; the rest N(0, 1)."""
    t = torch.randn(rows, ld, generator=g)
    if rows > 1:
        t[1] += 100.0
    if rows > 2:
        t[2] = const
    if rows > 3:
        t[3] *= 0.01
    if rows > 4:
        t[4] *= 30.0
    return t.to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _ln_inputs(rows, D, ldx, ldr):
    g = torch.Generator().manual_seed(1000 * rows + D)
    gamma, beta = torch.randn(D, generator=g), torch.randn(D, generator=g)
    return _ln_rows(g, rows, ldx, 3.0), _ln_rows(g, rows, ldr, -1.25), gamma, beta


def _ln_case(name, rows, D, res, eps, ldx=None, ldr=None, ldo=None, fp8=None):
    """``xs`` [rows, ldx] / ``rs`` [rows, ldr]: the storage the kernel strides over (columns past D are
    other data, which a wrong stride reads); ``fp8``: None, "only" (out == nullptr) or "both"."""
    ldx, ldr, ldo = ldx or D, ldr or D, ldo or D
    xs, rs, gamma, beta = _ln_inputs(rows, D, ldx, ldr)
    return SimpleNamespace(kernel="layernorm", id=name, rows=rows, D=D, ldx=ldx, ldr=ldr, ldo=ldo, eps=eps, xs=xs,
                           rs=rs if res else None, gamma=gamma, beta=beta, fp8=fp8)


@functools.lru_cache(maxsize=None)
def ln_cases():
    out = []
    for rows, D in LN_SHAPES:
        out.append(_ln_case(f"ln-{rows}x{D}", rows, D, False, 1e-12))
        out.append(_ln_case(f"ln-{rows}x{D}-res", rows, D, True, 1e-5))
    out.append(_ln_case("ln-5x768-eps5", 5, 768, False, 1e-5))       # the constant row at the other eps
    out.append(_ln_case("ln-5x768-res-eps12", 5, 768, True, 1e-12))
    out.append(_ln_case("ln-9x768-res", 9, 768, True, 1e-5))        # rows % (4 RPW) != 0 at RPW 2 and 4
    out.append(_ln_case("ln-17x768-res", 17, 768, True, 1e-5))
    out.append(_ln_case("ln-5x768-strided", 5, 768, True, 1e-5, ldx=776, ldr=784, ldo=776))
    out.append(_ln_case("ln-3x768-cls", 3, 768, False, 1e-12, ldx=4 * 768, ldo=4 * 768))  # ViT: CLS rows of T = 4
    out.append(_ln_case("ln-5x768-fp8only", 5, 768, False, 1e-12, fp8="only"))
    out.append(_ln_case("ln-5x768-res-fp8both", 5, 768, True, 1e-5, fp8="both"))     # = ln-5x768-res + out8
    return out


def ln_ref(c, dtype=torch.float64, hooks=None) -> LNRef:
    return layernorm_ref(c.xs[:, :c.D], c.gamma, c.beta, c.eps, None if c.rs is None else c.rs[:, :c.D], dtype, hooks)


EMBED_B, EMBED_L, EMBED_VOCAB, EMBED_NTYPES = 3, 5, 50, 2


@functools.lru_cache(maxsize=None)
def embed_cases():
    out = []
    for D in (8, 520, 768, 2048):
        g = torch.Generator().manual_seed(7000 + D)
        rows = EMBED_B * EMBED_L
        ids = torch.randint(0, EMBED_VOCAB, (rows,), generator=g, dtype=torch.int32)
        ids[:4] = torch.tensor([0, 49, -3, 57], dtype=torch.int32)
        types = None
        if D in (8, 768):
            types = torch.randint(0, EMBED_NTYPES, (rows,), generator=g, dtype=torch.int32)
            types[1:5] = torch.tensor([2, -1, 1, 0], dtype=torch.int32)
        tables = tuple(torch.randn(n, D, generator=g).to(torch.bfloat16) for n in (EMBED_VOCAB, EMBED_L + 2, EMBED_NTYPES))
        out.append(SimpleNamespace(kernel="embed_ln", id=f"embed-D{D}-{'types' if types is not None else 'notypes'}",
                                   D=D, rows=rows, L=EMBED_L, ids=ids, types=types, tables=tables,
                                   gamma=torch.randn(D, generator=g), beta=torch.randn(D, generator=g), eps=1e-12))
    return out


def embed_ref_of(c, dtype=torch.float64) -> LNRef:
    return embed_ln_ref(c.ids, c.types, c.tables, c.gamma, c.beta, c.eps, c.L, EMBED_VOCAB, EMBED_NTYPES, dtype)


@functools.lru_cache(maxsize=None)
def vit_cases():
    out = []
    for B, npatch, D in [(1, 1, 8), (3, 5, 768), (2, 4, 520)]:
        g = torch.Generator().manual_seed(100 * B + 10 * npatch + D)
        mk = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)  # noqa: E731
        out.append(SimpleNamespace(kernel="vit_tokens", id=f"vit-{B}x{npatch}x{D}", B=B, np=npatch, D=D,
                                   patches=mk(B * npatch, D), cls=mk(D), pos=mk(npatch + 1, D)))
    return out


# attention: the edges of the 32-key padding (31, 32, 33), of the 16-query waves (16), of the 64- and
# 128-query blocks (64, 65, 127, 128, 129), ViT (197), the one-pass limit (256) and the first streamed L
ATT_L = [1, 16, 31, 32, 33, 64, 65, 127, 128, 129, 197, 256, 257]
ATT_B, ATT_HEADS = 2, 2
MASKS = ["none", "half", "seq", "inf"]


def make_mask(kind, B, L):
    """none; half: the last sequence's second half at -1e9; seq: the whole of sequence 0 at -1e9; inf:
    -inf on the 16-aligned block of keys 16..31 and on every 7th key from 3 -- never a whole row (key 0
    stays), so there is none at L = 1."""
    if kind == "none":
        return None
    if kind == "half":
        return I.half_mask(B, L)
    m = torch.zeros(B, L)
    if kind == "seq":
        m[0] = -1e9
        return m
    assert kind == "inf" and L > 1
    m[:, 16:32] = float("-inf")
    m[-1, 3::7] = float("-inf")
    m[0, 1:2] = float("-inf")
    return m


def _att_case(name, qkv, B, L, heads, mask, ldo=None, k_off=None, v_off=None):
    D = heads * 64
    return SimpleNamespace(kernel="attention", id=name, qkv=qkv, B=B, L=L, heads=heads, mask=mask, ldo=ldo or D,
                           k_off=D if k_off is None else k_off, v_off=2 * D if v_off is None else v_off)


@functools.lru_cache(maxsize=None)
def _layout_qkv(B, L, heads):
    g = torch.Generator().manual_seed(5000 + L)
    return torch.randn(B * L, 3 * heads * 64 + 8, generator=g).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def att_cases():
    """Own cases, then every input of tests/att_stream_inputs.py (``stream-*``: the default process runs
    its SHORT ones through the one-pass kernel and the rest through the streamed one)."""
    out = []
    B, H = ATT_B, ATT_HEADS
    for L in ATT_L:
        for kind in MASKS:
            if kind == "inf" and L == 1:
                continue
            out.append(_att_case(f"att-L{L}-{kind}", I.random_qkv(B, L, H), B, L, H, make_mask(kind, B, L)))
    for L in (65, 257):  # K and V swapped in a row of 3D + 8, output rows of D + 4: one-pass and streamed
        out.append(_att_case(f"att-L{L}-layout", _layout_qkv(B, L, H), B, L, H, I.half_mask(B, L), ldo=H * 64 + 4,
                             k_off=2 * H * 64, v_off=H * 64))
    for name, qkv, b, L, h, mask in I.cases():
        out.append(_att_case(f"stream-{name}", qkv, b, L, h, mask))
    return out


@functools.lru_cache(maxsize=None)
def att_ref_of(name, dtype=torch.float64) -> AttRef:
    c = case(name)
    return attention_ref(c.qkv, c.B, c.L, c.heads, c.mask, 0.125, c.k_off, c.v_off, dtype)


def packed_qkv(c):
    """The case's Q, K, V in the packed default layout [B*L, 3D] (for the emulations)."""
    D = c.heads * 64
    return torch.cat([c.qkv[:, o:o + D] for o in (0, c.k_off, c.v_off)], 1).contiguous()


# qkvatt: L = 1; exactly one 32-key step; a partial wave; 33 with 4 heads; 100 (BERT-like, 7 waves,
# the last one partial); the full 128-token tile; one head (D = 64: one GEMM stage, nst = 1)
QKVATT_SHAPES = [(1, 1, 2), (1, 32, 2), (3, 7, 2), (1, 33, 4), (2, 100, 2), (2, 128, 2), (1, 17, 1)]
QKVATT_SEED = 0


@functools.lru_cache(maxsize=None)
def qkvatt_weights(heads):
    D = heads * 64
    g = torch.Generator().manual_seed(300 + heads + QKVATT_SEED)
    return CV.pack_linear(torch.randn(3 * D, D, generator=g) * D ** -0.5, 0.1 * torch.randn(3 * D, generator=g))


@functools.lru_cache(maxsize=None)
def _qkvatt_x(B, L, heads, ldx):
    g = torch.Generator().manual_seed(10000 * B + 10 * L + heads + QKVATT_SEED)
    return torch.randn(B * L, ldx, generator=g).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def qkvatt_cases():
    out = []

    def add(name, B, L, H, kind, ld=None):
        D = H * 64
        out.append(SimpleNamespace(kernel="qkvatt", id=name, B=B, L=L, heads=H, D=D, ldx=ld or D, ldo=ld or D,
                                   xs=_qkvatt_x(B, L, H, ld or D), mask=make_mask(kind, B, L)))

    for B, L, H in QKVATT_SHAPES:
        for kind in MASKS:
            if not (kind == "inf" and L == 1):
                add(f"qkvatt-{B}x{L}x{H}-{kind}", B, L, H, kind)
    add("qkvatt-2x100x2-ld", 2, 100, 2, "half", ld=2 * 64 + 8)
    return out


@functools.lru_cache(maxsize=None)
def qkvatt_ref_of(name, dtype=torch.float64) -> AttRef:
    c = case(name)
    return qkvatt_ref(c.xs, qkvatt_weights(c.heads), c.mask, c.B, c.L, c.heads, dtype)


@functools.lru_cache(maxsize=None)
def softmax_cases():
    """(rows, D, ldx, ldo, input type, masked): D = 1, D = 65 (one element on the second trip of a lane),
    fp32 and bf16, ld > D, the [D] additive mask with some entries at -inf (never all)."""
    out = []
    for rows, D, ldx, ldo, dt, masked in [(4, 1, 8, 4, torch.float32, False), (4, 1, 8, 1, torch.bfloat16, True),
                                          (5, 65, 72, 65, torch.float32, True), (5, 65, 72, 80, torch.bfloat16, True),
                                          (5, 65, 65, 65, torch.bfloat16, False), (37, 197, 200, 197, torch.bfloat16, True),
                                          (3, 1000, 1000, 1000, torch.float32, True)]:
        g = torch.Generator().manual_seed(10 * D + rows)
        x = (torch.randn(rows, ldx, generator=g) * 4).to(dt)
        mask = None
        if masked:
            mask = torch.randn(D, generator=g)
            mask[2::5] = float("-inf")  # (D = 1: nothing)
        name = f"softmax-{rows}x{D}-ld{ldx}-{'bf16' if dt == torch.bfloat16 else 'fp32'}{'-mask' if masked else ''}"
        out.append(SimpleNamespace(kernel="softmax", id=name, rows=rows, D=D, ldx=ldx, ldo=ldo, x=x, mask=mask, scale=0.5))
    return out


def cases():
    """Every per-kernel GPU case."""
    return ln_cases() + embed_cases() + vit_cases() + att_cases() + qkvatt_cases() + softmax_cases()


@functools.lru_cache(maxsize=None)
def _by_id():
    d = {c.id: c for c in cases()}
    assert len(d) == len(cases())
    return d


def case(name):
    return _by_id()[name]


def ids(cs):
    return [c.id for c in cs]
