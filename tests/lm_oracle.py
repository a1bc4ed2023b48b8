"""fp64 oracles of the single-request AWD-LSTM decode kernels of csrc/lstm.hip (``lstm_cell_kernel``,
``lstm_x_kernel`` with and without the folded layer 0, ``hh_rows``, ``decoder_kernel`` and its keys
epilogue, the two samplers), element-wise comparators with derived bounds, the host copy of the Gumbel
noise, and the seeded inputs of every per-kernel GPU case, so that tests/test_lm_oracle_cpu.py judges the
oracles on exactly what tests/test_lm_kernels_gpu.py runs. Torch and numpy, CPU only. Not a test module.

Every ``*_ref`` takes exactly what its kernel reads -- the bf16 weights widened, the fp32 state, bias,
``pre`` and ``xtab`` as they are -- so weight rounding is no part of the error: what remains is the
kernel's fp32 arithmetic. u = 2**-24 is one fp32 rounding, relative.

GEMV rows (line numbers: csrc/lstm.hip). A row's dot product is computed as

* the 8 products and 7 adds of one lane's 16-B chunk, added to the lane's accumulator (lines 212-213,
  382-383, 664-665, 727-728): 1 + 7 + 1 roundings on the deepest path, the last once per 512-chunk the
  wave owns (``NC`` chunks: ``ceil(NCH / 2)`` in the two LSTM kernels where two waves split K, ``NCH``
  in the decoder, 3 in ``hh_rows``);
* the 6 xor-shuffle steps of ``warp_sum`` (common.h);
* in the LSTM kernels one add of the other wave's partial (KW = 2; lines 227, 396);
* one add of the bias (lines 230-233, 675, 739) or of ``pre`` (lines 397-400).

so every term passes through at most ``c = 8 + NC + 6 + KW - 1 + 1`` roundings and

    |pre_got - pre_ref| <= c u S,    S = sum_k |w_k x_k| + |b|

(first order in u; the second-order terms are below 2**-19 of this). c per kernel, with
NCH = ceil(ldk / 512):

    lstm_cell_kernel<NCH, 2>   c = 16 + ceil(NCH / 2)   (17 .. 19)
    lstm_x_kernel<NCH, *>      c = 16 + ceil(NCH / 2)   (17 .. 19; the last add is ``+ pre``)
    layer 0 folded             c = 1                    (``xtab[tok] + pre0``, line 348: S = |xtab| + |pre0|)
    hh_rows<3>                 c = 18                   (8 + 3 + 6 + 1)
    decoder_kernel<NCH, 4, *>  c = 15 + NCH             (16 .. 19)

A fused multiply-add has one rounding fewer than counted. Columns past K are zero on one side (the
weight pad, the LDS pad or ``wmask``) and add exact zeros.

The cell (lines 234-240, 349-357, 397-403), from gate pre-activations a_i, a_f, a_g, a_o with errors d:

    s = 1 / (1 + __expf(-a))      |ds| <= s (1 - s) d + u min(E_SIG_ABS, E_SIG s)
    t = tanhf(a)                  |dt| <= (1 - t^2) d + E_TANH u |t|
    c' = s_f c + s_i t_g          |dc'| <= |c| ds_f + |t_g| ds_i + s_i dt_g + u (|s_f c| + |s_i t_g| + |c'|)
    h' = s_o tanhf(c')            |dh'| <= |tanh c'| ds_o + s_o ((1 - tanh^2 c') dc' + E_TANH u |tanh c'|) + u |h'|

the derivative terms carry the pre-activation error through the gates; ``E_SIG`` (relative) and
``E_SIG_ABS`` (absolute) cover ``__expf``, the add and the division together and ``E_TANH`` is ``tanhf``'s
relative error, all in units of u. The
single-request kernels keep h and c in fp32, so nothing else is rounded. In the folded kernel layer 1's
GEMV runs on the kernel's own h0, so its pre-activations carry ``sum_k |w_k| dh0_k`` as well.

No accuracy of ``__expf``, ``tanhf`` or ``__logf`` on gfx950 is documented in anything this repository can
cite, so the terms are measured: on an MI355X, 2026-10-20, scripts/native/ulp_probe.hip (built with the
library's compiler flags) evaluated each expression in fp32 and in fp64 at 2**24 arguments, argument i of
n = 2**24 as given below, and kept the largest difference; every constant is twice the measured figure,
for arguments between grid points.

    1 / (1 + __expf(-x)), x = -16 + 32 i / n:         abs 1.564 u, relative 16.06 u (at x = -16; ``__expf``
                                                      alone: 15.91 u)      -> E_SIG_ABS 3.2, E_SIG 32.2
    tanhf(x), x = -8 + 16 i / n:                      relative 2.427 u (abs 1.363 u)        -> E_TANH 4.9
    __logf(u), u = (k + 0.5f) 2**-24, k < 2**24:      relative 3.157 u
    __logf(x), x = 2**(-26 + 31 i / 2**24):           relative 3.180 u                      -> E_LOG 6.4

The relative figure of ``__logf`` holds up to the arguments next to 1 (the last of 64 bins of u: 2.76 u),
so the logarithm needs no absolute term.

Sampler keys: ``key = logit + gumbel(seed, t, row)`` (line 742), ``gumbel_of`` in common.h:
``u = ((r >> 9) + 0.5f) * 2**-23``, ``g = -__logf(-__logf(u))``. With 23 random bits ``k + 0.5`` has 24
significant bits, so the fp32 u is exact, the same number ``gumbel_np`` forms in fp64, and lies in
[2**-24, 1 - 2**-24]: every key is finite (tests/test_lm_oracle_cpu.py checks both at the extreme k). Only
the two logarithms err; with L = -log u,

    |dL| <= E_LOG u L,     |dg| <= -log(1 - E_LOG u) + E_LOG u |log L|

and the key adds ``u |key|`` and the logit's own bound. (Until this oracle was written the kernel took 24
bits: ``k + 0.5f`` was then rounded to an integer for k >= 2**23, u differed from the exact value by
2**-25, up to 0.29 in g, and at k = 2**24 - 1 u was 1.0f and the key +inf -- one id in 2**24 per step won
the sampler whatever its logit. Found by sweeping every k on the GPU; fixed in common.h.)

Faults the ``hooks`` of the oracles plant, one each (tests/test_lm_oracle_cpu.py shows that every one
leaves the bound at every case): ``swap_fg`` gates f and g exchanged; ``bias_next`` the bias (or ``pre``)
of row r taken from row r + 1; ``drop_k8`` the last 8 columns of K dropped; ``x_parity`` the vector operand
from the wrong parity half; ``c_parity`` the previous cell state from the wrong half; ``stale_unit`` the
last unit's new cell state left at the previous one; ``h_layer_shift`` (``hh_ref``) layer l's h used for
layer l + 1; ``tie_high`` (sampler order) equal keys resolved to the higher row. Each case lists the hooks
that exist for it (``c.hooks``): ``x_parity`` is absent where the vector operand has no parity half (the
embedding row of the layer-0 forms, the h0 the folded kernel rebuilds itself), ``bias_next`` where the
decoder has no bias, and ``tie_high`` at V = 1, where one key cannot tie. Every other hook runs at every case.

The case tables hold ``Spec``s (an id and the arguments); ``build`` makes the tensors inside the test that
uses them, so nothing large lives past it.
"""
import zlib
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import torch

from hipzap.engine.lm import _bf16_rows, _interleave, _pad_to

U32 = 2.0 ** -24
E_SIG, E_SIG_ABS = 32.2, 3.2  # 2 x measured (module docstring), in units of u
E_TANH = 4.9
E_LOG = 6.4
F64, F32 = torch.float64, torch.float32
NONE_IDX = 0x7FFFFFFF

Report = namedtuple("Report", "ok ratio index got ref bound bad")
Bounded = namedtuple("Bounded", "ref bound")


# ------------------------------------------------------------------------------------------------
# comparators
def compare(got, ref: Bounded) -> Report:
    """Element-wise ``|got - ref| <= bound`` with every value finite; the worst element by err / bound."""
    g = torch.as_tensor(got).double().reshape(-1)
    r, b = ref.ref.double().reshape(-1), ref.bound.double().reshape(-1)
    assert g.shape == r.shape == b.shape, (g.shape, r.shape, b.shape)
    err = (g - r).abs()
    fail = ~(err <= b) | ~torch.isfinite(g)
    ratio = torch.where(torch.isfinite(err), err / b.clamp_min(1e-300), torch.full_like(err, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    i = int(ratio.argmax()) if ratio.numel() else 0
    idx = tuple(int(x) for x in np.unravel_index(i, tuple(ref.ref.shape))) if ratio.numel() else ()
    return Report(not bool(fail.any()), float(ratio[i]) if ratio.numel() else 0.0, idx,
                  float(g[i]) if g.numel() else 0.0, float(r[i]) if g.numel() else 0.0,
                  float(b[i]) if g.numel() else 0.0, int(fail.sum()))


def describe(what: str, rep: Report) -> str:
    return (f"{what}: worst err/bound {rep.ratio:.3g} at {rep.index}: got {rep.got!r} ref {rep.ref!r} "
            f"bound {rep.bound:.3g}; {rep.bad} element(s) outside")


def check(what: str, got, ref: Bounded) -> Report:
    rep = compare(got, ref)
    print(describe(what, rep))
    assert rep.ok, describe(what, rep)
    return rep


# ------------------------------------------------------------------------------------------------
# the math
def nch_of(ldk: int) -> int:
    return (ldk + 511) // 512


def c_lstm(ldk: int) -> int:
    return 16 + (nch_of(ldk) + 1) // 2


def c_decoder(ldk: int) -> int:
    return 15 + nch_of(ldk)


C_HH = 18


def _gemv(w, x, b, c, K, hooks, dx=None):
    """rows of ``w[:, :K] . x + b`` and the bound ``c u S`` (+ ``|w| . dx``)."""
    dt = x.dtype
    wk, xk = w[:, :K].to(dt), x
    if hooks.get("drop_k8"):
        wk, xk = wk[:, :max(K - 8, 0)], xk[:max(K - 8, 0)]
    if hooks.get("bias_next"):
        b = torch.roll(b, -1)
    pre = wk @ xk + b.to(dt)
    S = wk.abs().double() @ xk.abs().double() + b.abs().double()
    bound = c * U32 * S
    if dx is not None:
        bound = bound + w[:, :K].abs().double() @ dx
    return pre, bound


def _sig(a, da):
    s = torch.sigmoid(a)
    return s, s.double() * (1 - s.double()) * da + U32 * torch.clamp(E_SIG * s.double(), max=E_SIG_ABS)


def _tanh(a, da):
    t = torch.tanh(a)
    return t, (1 - t.double() ** 2) * da + E_TANH * U32 * t.double().abs()


def _cell(pre, dpre, c_prev, hooks):
    """rows 4j + q = gate q (i, f, g, o) of unit j -> (h', c', dh', dc')"""
    a, d = pre.reshape(-1, 4), dpre.reshape(-1, 4)
    qf, qg = (2, 1) if hooks.get("swap_fg") else (1, 2)
    si, dsi = _sig(a[:, 0], d[:, 0])
    sf, dsf = _sig(a[:, qf], d[:, qf])
    tg, dtg = _tanh(a[:, qg], d[:, qg])
    so, dso = _sig(a[:, 3], d[:, 3])
    c_new = sf * c_prev + si * tg
    D = lambda t: t.double().abs()  # noqa: E731
    dc = D(c_prev) * dsf + D(tg) * dsi + D(si) * dtg + U32 * (D(sf * c_prev) + D(si * tg) + D(c_new))
    if hooks.get("stale_unit"):
        c_new = c_new.clone()
        c_new[-1] = c_prev[-1]
    tc, dtc = _tanh(c_new, dc)
    h_new = so * tc
    dh = D(tc) * dso + D(so) * dtc + U32 * D(h_new)
    return h_new, c_new, dh, dc


def cell_ref(w, bias, h_state, c_state, par, In, H, x_state=None, x=None, dtype=F64, hooks=None):
    """``lstm_cell_kernel``: ``w`` [4H, ldk] bf16 rows 4j + q over [x ; h], ``bias`` [4H] fp32, the state
    ``[2, H]`` fp32 read at parity ``par`` and written at ``par ^ 1``; the input is ``x`` (the embedding
    row of the token, layer 0) or ``x_state[par ^ 1]`` (the previous layer's output of this step).
    -> {"h": Bounded, "c": Bounded}, the halves the kernel writes."""
    hk = hooks or {}
    if x is None:
        x = x_state[par if hk.get("x_parity") else par ^ 1]
    v = torch.cat([x.to(dtype), h_state[par].to(dtype)])
    pre, dpre = _gemv(w, v, bias, c_lstm(w.shape[1]), In + H, hk)
    c_prev = c_state[par ^ 1 if hk.get("c_parity") else par].to(dtype)
    h, c, dh, dc = _cell(pre, dpre, c_prev, hk)
    return {"h": Bounded(h, dh), "c": Bounded(c, dc)}


def x_cell_ref(w, pre, h_state, c_state, par, In, H, x_state=None, fold=None, dtype=F64, hooks=None):
    """``lstm_x_kernel``: gates = ``w[:, :In] . x + pre`` (``pre`` [4H] fp32 = W_hh h + b of the step
    before), cell as above. ``fold`` (layer 0 folded: ``xrow`` [4 H0] fp32 = xtab[tok], ``pre0`` [4 H0],
    ``c0_state`` [2, H0]): x = h0' of this step from ``xrow + pre0`` and ``c0_state[par]``, also returned
    (workgroup 0 publishes it); else x = ``x_state[par ^ 1]``.
    -> {"h", "c"} and with ``fold`` {"h0", "c0"}."""
    hk = hooks or {}
    out = {}
    dx = None
    if fold is not None:
        g0 = fold["xrow"].to(dtype) + fold["pre0"].to(dtype)
        dg0 = U32 * (fold["xrow"].double().abs() + fold["pre0"].double().abs())
        c0 = fold["c0_state"][par ^ 1 if hk.get("c_parity") else par].to(dtype)
        h0, c0n, dh0, dc0 = _cell(g0, dg0, c0, hk)
        out["h0"], out["c0"] = Bounded(h0, dh0), Bounded(c0n, dc0)
        x, dx = h0, dh0
    else:
        x = x_state[par if hk.get("x_parity") else par ^ 1].to(dtype)
    p, dp = _gemv(w, x, pre, c_lstm(w.shape[1]), In, hk, dx)
    c_prev = c_state[par ^ 1 if hk.get("c_parity") else par].to(dtype)
    h, c, dh, dc = _cell(p, dp, c_prev, hk)
    out["h"], out["c"] = Bounded(h, dh), Bounded(c, dc)
    return out


def hh_ref(ws, biases, h_states, par, Hs, dtype=F64, hooks=None):
    """``hh_rows``: per layer l, ``out[l] = W_hh^l . h^l[par ^ 1] + b^l`` ([4 H_l], interleaved rows), the
    next step's recurrent partials. -> list of Bounded."""
    hk = hooks or {}
    out = []
    for l, (w, b, H) in enumerate(zip(ws, biases, Hs)):
        src = h_states[l]
        if hk.get("h_layer_shift") and l > 0:  # the previous layer's h, cut or zero-filled to H
            prev = h_states[l - 1]
            src = torch.zeros_like(h_states[l])
            n = min(H, prev.shape[1])
            src[:, :n] = prev[:, :n]
        h = src[par if hk.get("x_parity") else par ^ 1].to(dtype)
        out.append(Bounded(*_gemv(w, h, b, C_HH, H, hk)))
    return out


def decoder_ref(w, bias, h_state, par, V, H, dtype=F64, hooks=None):
    """``decoder_kernel``: ``logits = w[:V, :H] . h[par ^ 1] (+ bias)``. -> Bounded."""
    hk = hooks or {}
    h = h_state[par if hk.get("x_parity") else par ^ 1].to(dtype)
    b = torch.zeros(V, dtype=F32) if bias is None else bias
    return Bounded(*_gemv(w[:V], h, b, c_decoder(w.shape[1]), H, hk))


# ------------------------------------------------------------------------------------------------
# Gumbel keys and the sampler's order
def _philox_bits(seed: int, t: int, V: int) -> np.ndarray:
    """common.h gumbel(seed, t, j)'s 32 random bits for j = 0..V-1 (Philox4x32-10, one block per 4 ids)."""
    M = np.uint64(0xFFFFFFFF)
    j = np.arange(V, dtype=np.uint64)
    c0 = j >> np.uint64(2)
    c1 = np.full(V, t & 0xFFFFFFFF, np.uint64)
    c2 = np.full(V, 0x5EED, np.uint64)
    c3 = np.zeros(V, np.uint64)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        h0, l0 = p0 >> np.uint64(32), p0 & M
        h1, l1 = p1 >> np.uint64(32), p1 & M
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return np.choose((j & np.uint64(3)).astype(np.int64), [c0, c1, c2, c3])


def uniform_of(r, dtype=np.float64) -> np.ndarray:
    """common.h ``gumbel_of``'s u from 32 random bits, in ``dtype`` arithmetic: 23 bits, so ``k + 0.5`` has 24
    significant bits and float32 gives the very same number as float64, inside [2**-24, 1 - 2**-24]."""
    k = (np.asarray(r, dtype=np.uint64) >> np.uint64(9)).astype(dtype)
    return (k + dtype(0.5)) * dtype(1.0 / 8388608.0)


def gumbel_of(r) -> np.ndarray:
    return -np.log(-np.log(uniform_of(r)))


def gumbel_np(seed: int, t: int, V: int) -> np.ndarray:
    """Host copy of common.h gumbel(seed, t, j) for j = 0..V-1 (Philox4x32-10, one block per 4 ids)."""
    return gumbel_of(_philox_bits(seed, t, V))


def gumbel_bound_of(r) -> np.ndarray:
    """|device gumbel_of(r) - gumbel_of(r)| (module docstring)."""
    L = -np.log(uniform_of(r))
    return -np.log1p(-U32 * E_LOG) + U32 * E_LOG * np.abs(np.log(L))


def gumbel_bound(seed: int, t: int, V: int) -> np.ndarray:
    return gumbel_bound_of(_philox_bits(seed, t, V))


def keys_ref(logits: Bounded, seed: int, t: int) -> Bounded:
    """The decoder's keys epilogue: ``logit + gumbel(seed, t, row)``."""
    V = logits.ref.numel()
    key = logits.ref.double() + torch.from_numpy(gumbel_np(seed, t, V))
    return Bounded(key, logits.bound + torch.from_numpy(gumbel_bound(seed, t, V)) + U32 * key.abs())


def better(av, ai, bv, bi, tie_high=False):
    """csrc/lstm.hip ``better``: larger value first, ties to the lower row."""
    return av > bv or (av == bv and (ai > bi if tie_high else ai < bi))


def order(keys, tie_high=False) -> list:
    """All rows in descending ``better`` order."""
    k = [float(x) for x in keys]
    return sorted(range(len(k)), key=lambda r: (-k[r], -r if tie_high else r))


def top10(keys, tie_high=False) -> list:
    return order(keys, tie_high)[:10]


def decoder_geometry(V: int):
    """Host copy of ``hz_decoder_geometry`` -> (nblk, rpb)."""
    groups = (V + 7) // 8
    nb = min(2048, (groups + 3) // 4)
    gpb = (groups + nb - 1) // nb
    gpb = (gpb + 3) // 4 * 4
    return (groups + gpb - 1) // gpb, gpb * 8


def block_maxima(keys, nblk, rpb, exclude=(), tie_high=False):
    """What the decoder's epilogue leaves per workgroup: the best key (value, row) and the best over the
    acceptable rows (not 0, not excluded); (-inf, 0x7fffffff) where a workgroup has no such row.
    -> (bmax_val f32, bmax_idx i32, bacc_val, bacc_idx) numpy."""
    k = np.asarray(keys, dtype=np.float32)
    V = k.shape[0]
    ex = set(int(e) for e in exclude) | {0}
    bv = np.full(nblk, -np.inf, np.float32)
    bi = np.full(nblk, NONE_IDX, np.int32)
    av, ai = bv.copy(), bi.copy()
    for b in range(nblk):
        for r in range(b * rpb, min(V, (b + 1) * rpb)):
            if better(k[r], r, bv[b], bi[b], tie_high):
                bv[b], bi[b] = k[r], r
            if r not in ex and better(k[r], r, av[b], ai[b], tie_high):
                av[b], ai[b] = k[r], r
    return bv, bi, av, ai


def token_from_maxima(bv, bi, av, ai, V, tie_high=False) -> int:
    """``block_token`` and the fused samplers: the best acceptable maximum, else the best maximum."""
    def best(val, idx):
        v, i = -np.inf, NONE_IDX
        for a, b in zip(val, idx):
            if better(a, int(b), v, i, tie_high):
                v, i = a, int(b)
        return i
    i = best(av, ai)
    if i == NONE_IDX:
        i = best(bv, bi)
    return min(max(i, 0), V - 1)


def select_draw(draws, exclude) -> int:
    """The reference's rule: the first draw that is not 0 and not excluded, else the first draw."""
    ex = set(int(e) for e in exclude)
    for r in draws:
        if r != 0 and r not in ex:
            return int(r)
    return int(draws[0])


# ------------------------------------------------------------------------------------------------
# inputs of the cases (seeded; CPU tensors)
def _gen(cid: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(cid.encode()))


def _bf(t):
    return t.to(torch.bfloat16)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=F32) * scale


def _state(g, n):
    """[2, n] fp32 of order 1, both parity halves different."""
    return _randn(g, 2, n)


def pack_rows(w, ld):
    """gate-interleaved rows (already 4j + q) -> bf16 [rows, ld], pad columns zero."""
    return _bf16_rows(w, ld, "cpu")


Spec = namedtuple("Spec", "id fn args kw")


def _spec(fn, *args, **kw) -> Spec:
    return Spec(fn(*args, only_id=True, **kw), fn, args, kw)


def build(s: Spec):
    """The tensors of a case (a SimpleNamespace), made when asked for."""
    return s.fn(*s.args, **s.kw)


def _small_maxima(g, V, tok):
    """three decoder workgroups whose best acceptable maximum names ``tok``"""
    bmax_val, bmax_idx = _randn(g, 3).numpy(), np.array([3, 9, 17], np.int32) % V
    bacc_val, bacc_idx = _randn(g, 3).numpy(), np.array([4 % V, 10 % V, tok], np.int32)
    bacc_val[2] = 7.0
    assert token_from_maxima(bmax_val, bmax_idx, bacc_val, bacc_idx, V) == tok
    return bmax_val, bmax_idx, bacc_val, bacc_idx


CELL_SHAPES = [(37, 6), (300, 301), (500, 530), (1000, 552), (1000, 1150), (1500, 1150)]  # NCH 1..6
EMB_V, FUSED_V = 50, 2400


def cell_case(In, H, form="plain", tok=0, nblk=0, fallback=False, only_id=False):
    """Inputs of one ``lstm_cell_kernel`` case. form: plain (x from x_state), emb (layer 0, forced token
    ``tok`` of a V = 50 table, lde != In; decoder maxima that name another token are passed too, and must be
    ignored while t < n_forced), fused (layer 0, the token from ``nblk`` decoder maxima)."""
    cid = f"cell-{In}x{H}-{form}" + (f"-tok{tok}" if form == "emb" else "") + \
        (f"-nblk{nblk}" + ("-fallback" if fallback else "") if form == "fused" else "")
    if only_id:
        return cid
    g = _gen(f"cell-{In}x{H}")  # the same weights and state for every form of a shape
    ldk = _pad_to(In + H, 64)
    s = (In + H) ** -0.5
    c = SimpleNamespace(id=cid, In=In, H=H, ldk=ldk, form=form, nch=nch_of(ldk))
    c.w_ih, c.w_hh = _bf(_randn(g, 4 * H, In, scale=s)).float(), _bf(_randn(g, 4 * H, H, scale=s)).float()
    c.b = _randn(g, 4 * H, scale=0.5)                                  # gate-major, b_ih + b_hh
    c.w = pack_rows(_interleave(torch.cat([c.w_ih, c.w_hh], 1), H), ldk)
    c.bias = c.b.reshape(4, H).t().reshape(4 * H).contiguous()
    c.h_state, c.c_state, c.x_state = _state(g, H), _state(g, H), _state(g, In)
    c.hooks = ["swap_fg", "bias_next", "drop_k8", "c_parity", "stale_unit"] + (["x_parity"] if form == "plain" else [])
    if form != "plain":
        c.V = EMB_V if form == "emb" else FUSED_V
        c.lde = _pad_to(In, 8) + 8
        ge = _gen(f"emb-{In}-{c.V}")
        c.emb = torch.zeros(c.V, c.lde, dtype=torch.bfloat16)
        c.emb[:, :In] = _bf(_randn(ge, c.V, In))
        c.tok = tok
    if form == "emb":
        c.nblk = 3
        c.bmax_val, c.bmax_idx, c.bacc_val, c.bacc_idx = _small_maxima(_gen(cid), c.V, c.V - 1 - tok)
    if form == "fused":
        gm = _gen(cid)
        c.nblk, c.fallback = nblk, fallback
        c.bmax_val = _randn(gm, nblk).numpy()
        c.bmax_idx = torch.randint(0, c.V, (nblk,), generator=gm, dtype=torch.int32).numpy()
        c.bacc_val = _randn(gm, nblk).numpy()
        c.bacc_idx = torch.randint(1, c.V, (nblk,), generator=gm, dtype=torch.int32).numpy()
        if nblk > 256:  # the two best acceptable maxima equal, in different per-thread slots: the lower row wins
            c.bacc_val[[7, 263]] = 9.0
            c.bacc_idx[7], c.bacc_idx[263] = 1900, 1200
        if fallback:
            c.bacc_val[:] = -np.inf
            c.bacc_idx[:] = NONE_IDX
        c.tok = token_from_maxima(c.bmax_val, c.bmax_idx, c.bacc_val, c.bacc_idx, c.V)
    return c


def cell_cases():
    out = [_spec(cell_case, In, H) for In, H in CELL_SHAPES]
    for In, H in (CELL_SHAPES[0], CELL_SHAPES[4]):
        out += [_spec(cell_case, In, H, "emb", tok=0), _spec(cell_case, In, H, "emb", tok=EMB_V - 1)]
    In, H = CELL_SHAPES[0]
    out += [_spec(cell_case, In, H, "fused", nblk=1), _spec(cell_case, In, H, "fused", nblk=300),
            _spec(cell_case, In, H, "fused", nblk=300, fallback=True)]
    return out


def cell_oracle(c, par, dtype=F64, hooks=None):
    x = None if c.form == "plain" else c.emb[c.tok, :c.In].to(dtype)
    return cell_ref(c.w, c.bias, c.h_state, c.c_state, par, c.In, c.H, x_state=c.x_state, x=x, dtype=dtype,
                    hooks=hooks)


X_SHAPES = [(40, 7), (600, 10), (1100, 10), (1600, 10), (2100, 1150), (2600, 10)]        # NCH 1..6
X0_SHAPES = [(10, 7), (514, 10), (600, 10), (1150, 10), (1536, 10)]                     # H0 = In; NCH 1, 2, 2, 3, 3
XTAB_V = 20


def x_case(In, H, fold=False, tok=0, fused=False, only_id=False):
    """Inputs of one ``lstm_x_kernel`` case; ``fold``: layer 0 folded (H0 = In, a V = 20 ``xtab``), the token
    forced (``tok``; the decoder maxima passed with it name another token) or, with ``fused``, taken from
    the decoder maxima (nblk 3)."""
    cid = f"x{'0' if fold else ''}-{In}x{H}" + (f"-tok{tok}" + ("-fused" if fused else "") if fold else "")
    if only_id:
        return cid
    g = _gen(f"x{'0' if fold else ''}-{In}x{H}")
    ldk = _pad_to(In, 64)
    c = SimpleNamespace(id=cid, In=In, H=H, ldk=ldk, fold=fold, nch=nch_of(ldk), fused=fused)
    c.w = pack_rows(_bf(_randn(g, 4 * H, In, scale=In ** -0.5)).float(), ldk)
    c.pre = _randn(g, 4 * H)
    c.h_state, c.c_state, c.x_state = _state(g, H), _state(g, H), _state(g, In)
    c.hooks = ["swap_fg", "bias_next", "drop_k8", "c_parity", "stale_unit"] + ([] if fold else ["x_parity"])
    if fold:
        c.V = XTAB_V
        c.xtab = _randn(g, XTAB_V, 4 * In)
        c.pre0 = _randn(g, 4 * In)
        c.h0_state, c.c0_state = _state(g, In), _state(g, In)
        c.tok = tok
        c.nblk = 3
        c.bmax_val, c.bmax_idx, c.bacc_val, c.bacc_idx = _small_maxima(_gen(cid), c.V, tok if fused else c.V - 1 - tok)
    return c


def x_cases():
    out = [_spec(x_case, In, H) for In, H in X_SHAPES]
    for In, H in X0_SHAPES:
        out += [_spec(x_case, In, H, True, tok=0), _spec(x_case, In, H, True, tok=XTAB_V - 1, fused=True)]
    return out


def x_oracle(c, par, dtype=F64, hooks=None):
    fold = dict(xrow=c.xtab[c.tok], pre0=c.pre0, c0_state=c.c0_state) if c.fold else None
    return x_cell_ref(c.w, c.pre, c.h_state, c.c_state, par, c.In, c.H, x_state=c.x_state, fold=fold, dtype=dtype,
                      hooks=hooks)


DEC_SHAPES = [(7, 6, 8), (33, 96, 96), (257, 600, 600), (100, 1100, 1152), (100, 2000, 2048), (8193, 64, 64)]
DEC_SEED = 0x1234567811


def dec_case(V, H, ldk, bias=True, exact=False, only_id=False):
    cid = f"dec-{V}x{H}x{ldk}" + ("" if bias else "-nobias") + ("-exact" if exact else "")
    if only_id:
        return cid
    g = _gen(f"dec-{V}x{H}x{ldk}" + ("-exact" if exact else ""))
    c = SimpleNamespace(id=cid, V=V, H=H, ldk=ldk, exact=exact, nch=nch_of(ldk))
    if exact:  # small integers: every partial sum is an integer below 2**24, exact in fp32 in any order
        w = torch.randint(-4, 5, (V, H), generator=g).float()
        c.h_state = torch.randint(-8, 9, (2, H), generator=g).float()
        c.bias = torch.randint(-100, 101, (V,), generator=g).float() if bias else None
    else:
        w = _bf(_randn(g, V, H, scale=H ** -0.5)).float()
        c.h_state = _state(g, H)
        b = _randn(g, V)
        c.bias = b if bias else None
    c.w = pack_rows(w, ldk)
    c.nblk, c.rpb = decoder_geometry(V)
    c.hooks = ["drop_k8", "x_parity"] + (["bias_next"] if bias else [])
    return c


def dec_cases():
    out = []
    for s in DEC_SHAPES:
        out += [_spec(dec_case, *s), _spec(dec_case, *s, bias=False)]
    return out + [_spec(dec_case, 33, 96, 96, exact=True)]


def dec_oracle(c, par, dtype=F64, hooks=None):
    return decoder_ref(c.w, c.bias, c.h_state, par, c.V, c.H, dtype=dtype, hooks=hooks)


HH_H = (6, 10, 130, 1150)


def hh_case(n, exact=False, only_id=False):
    """``hh_rows`` for ``n`` layers of different H (ldh padded to 64) riding in a V = 33 decoder launch."""
    cid = f"hh-{n}" + ("-exact" if exact else "")
    if only_id:
        return cid
    g = _gen(cid)
    c = SimpleNamespace(id=cid, n=n, Hs=HH_H[:n], exact=exact, dec=dec_case(33, 96, 96, exact=exact))
    c.lds = [_pad_to(H, 64) for H in c.Hs]
    c.ws, c.biases, c.h_states = [], [], []
    for H, ld in zip(c.Hs, c.lds):
        if exact:
            w = torch.randint(-4, 5, (4 * H, H), generator=g).float()
            c.h_states.append(torch.randint(-8, 9, (2, H), generator=g).float())
            c.biases.append(torch.randint(-100, 101, (4 * H,), generator=g).float())
        else:
            w = _bf(_randn(g, 4 * H, H, scale=H ** -0.5)).float()
            c.h_states.append(_state(g, H))
            c.biases.append(_randn(g, 4 * H))
        c.ws.append(pack_rows(w, ld))
    c.blk = [0]
    for H in c.Hs:
        c.blk.append(c.blk[-1] + -(-4 * H // 16))
    c.hooks = ["drop_k8", "x_parity", "bias_next", "h_layer_shift"]
    return c


def hh_cases():
    return [_spec(hh_case, 2), _spec(hh_case, 4), _spec(hh_case, 4, exact=True)]


def hh_oracle(c, par, dtype=F64, hooks=None):
    return hh_ref(c.ws, c.biases, c.h_states, par, c.Hs, dtype=dtype, hooks=hooks)


SAMPLER_V = (1, 7, 9, 10, 11, 3000)
SAMPLER_PATTERNS = ("equal", "two-max", "max-excluded", "neg-inf", "row0", "exclude8")


def sampler_case(V, pattern, only_id=False):
    """Host-made keys: a coarse grid of values (so the 10 best always hold ties when V > 1), then the
    pattern. -> keys f32 [V], exclude list, and the decoder's maxima computed from the keys."""
    cid = f"sampler-V{V}-{pattern}"
    if only_id:
        return cid
    g = _gen(cid)
    nblk, rpb = decoder_geometry(V)
    keys = torch.randint(0, max(2, V // 3), (V,), generator=g).float().numpy() * 0.5
    exclude = []
    last = V - 1
    if pattern == "equal":
        keys[:] = 1.25
    elif pattern == "two-max":      # equal maxima in the first and the last workgroup
        keys[[min(1, last), last]] = 1e4
    elif pattern == "max-excluded":  # equal maxima, the lower one excluded
        keys[[min(1, last), last]] = 1e4
        exclude = [min(1, last)]
    elif pattern == "neg-inf":
        keys[::2] = -np.inf
        if V > 4:
            keys[V // 2:] = -np.inf
    elif pattern == "row0":
        keys[0] = 1e4
    elif pattern == "exclude8":     # at V <= 9 no row is acceptable: the fallback
        exclude = list(range(1, 9))
    c = SimpleNamespace(id=cid, V=V, pattern=pattern, keys=keys.astype(np.float32), exclude=exclude, nblk=nblk, rpb=rpb)
    c.hooks = ["tie_high"] if V > 1 else []  # one key cannot tie
    return c


def sampler_cases():
    return [_spec(sampler_case, V, p) for V in SAMPLER_V for p in SAMPLER_PATTERNS]


def sampler_oracle(c, hooks=None):
    """-> (draws: the min(10, V) best rows in order, token, the four maxima arrays)."""
    th = bool((hooks or {}).get("tie_high"))
    draws = top10(c.keys, th)
    mx = block_maxima(c.keys, c.nblk, c.rpb, c.exclude, th)
    return draws, select_draw(draws, c.exclude), mx
