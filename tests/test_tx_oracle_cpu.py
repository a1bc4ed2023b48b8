"""tests/tx_oracle.py on the CPU: the oracles of the transformer kernels agree with the project's
existing fp32 / fp64 references, their own fp32 and fp64 evaluations agree within the stated share of
the comparator's bound on the exact inputs of tests/test_tx_kernels_gpu.py, the CPU emulations of the
attention kernels pass the bound, and the comparator rejects every planted fault. Every element is
judged: no share of them may fail.

What the bounds cannot see (measured here, on ``att-L197-half``):
* P truncated to bf16 instead of rounded: worst 0.41 of the attention bound (the bound grants a whole
  ulp on every p_k, truncation uses one, rounding half);
* the unbiased variance at D = 768: rstd changes by 1 / (2 D) = 6.5e-4 relative, under half a bf16
  ulp (2**-9 .. 2**-8 relative), so only elements near a rounding tie move: the comparator rejects it
  at D = 8 and D = 64, not reliably at D = 768."""
import pytest
import torch

import att_stream_inputs as I
import tx_oracle as X
from hipzap.ops import transformer as T

F32, F64 = torch.float32, torch.float64


def _bf16(t):
    return t.to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------
# the oracles against the project's existing references, on the unmasked cases
@pytest.mark.parametrize("c", X.ln_cases(), ids=X.ids(X.ln_cases()))
def test_layernorm_ref_agrees_with_ops(c):
    ref = X.ln_ref(c, F32)
    old = T.layernorm_ref(c.xs[:, :c.D], T.NormParams(c.gamma, c.beta, c.eps), None if c.rs is None else c.rs[:, :c.D])
    X.check(old, ref.y, X.fp32_term(ref), label=f"ops.layernorm_ref vs layernorm_ref fp32, {c.id}")


@pytest.mark.parametrize("c", X.embed_cases(), ids=X.ids(X.embed_cases()))
def test_embed_ln_ref_agrees_with_ops(c):
    """ops.embed_ref neither clamps nor takes ``types=None``: it gets the clamped ids."""
    ref = X.embed_ref_of(c, F32)
    ids = c.ids.clamp(0, X.EMBED_VOCAB - 1)
    types = torch.zeros_like(ids) if c.types is None else c.types.clamp(0, X.EMBED_NTYPES - 1)
    old = T.embed_ref(ids, types, T.EmbedTables(*c.tables), T.NormParams(c.gamma, c.beta, c.eps), c.L)
    X.check(old, ref.y, X.fp32_term(ref), label=f"ops.embed_ref vs embed_ln_ref fp32, {c.id}")
    # the clamp is the contract: row 2 (id -3) reads word row 0, row 3 (id 57) word row 49
    w = c.tables[0].double()
    v = lambda r, tok, tt: w[tok] + c.tables[1].double()[r % c.L] + c.tables[2].double()[tt]  # noqa: E731
    tt = lambda r: 0 if c.types is None else min(max(int(c.types[r]), 0), 1)  # noqa: E731
    for r, tok in ((2, 0), (3, 49)):
        one = X._ln(v(r, tok, tt(r))[None], c.gamma, c.beta, c.eps)
        assert torch.equal(one.y[0], X.embed_ref_of(c).y[r])


_PACKED = [c for c in X.att_cases() if c.k_off == c.heads * 64 and c.ldo == c.heads * 64]
_UNMASKED = [c for c in _PACKED if c.mask is None]


@pytest.mark.parametrize("c", _UNMASKED, ids=X.ids(_UNMASKED))
def test_attention_ref_agrees_with_ops_and_ref64(c):
    bound = X.att_bound(X.att_ref_of(c.id)) / 4
    X.check(T.attention_ref(c.qkv, c.B, c.L, c.heads), X.att_ref_of(c.id, F32).y, bound, 64, f"ops.attention_ref, {c.id}")
    r = X.check(I.attention_ref64(c.qkv, c.B, c.L, c.heads), X.att_ref_of(c.id).y, bound, 64, f"attention_ref64, {c.id}")
    assert r.ratio < 1e-3  # fp64 both: apart by the float32 rounding of the scores alone


def test_vit_tokens_ref_is_the_rounded_sum():
    for c in X.vit_cases():
        ref = X.vit_tokens_ref(c.patches, c.cls, c.pos, c.B, c.np).reshape(c.B, c.np + 1, c.D)
        assert torch.equal(ref[:, 0], _bf16(c.cls.double() + c.pos[0].double()).expand(c.B, c.D))
        assert torch.equal(ref[:, 1:], _bf16(c.patches.double().reshape(c.B, c.np, c.D) + c.pos[1:].double()))


def test_softmax_ref_in_fp64():
    for c in X.softmax_cases():
        r64, r32 = T.softmax_ref(c.x, c.D, c.scale, c.mask, dtype=F64), T.softmax_ref(c.x, c.D, c.scale, c.mask)
        assert r64.dtype == F64 and r32.dtype == F32 and torch.isfinite(r64).all()
        assert (r64 - r32).abs().max() < 1e-6 and (r64.sum(-1) - 1).abs().max() < 1e-12
        if c.mask is not None:
            assert (r64[:, torch.isinf(c.mask)] == 0).all()


# ------------------------------------------------------------------------------------------------
# the reference alone: fp32 against fp64 on the GPU cases' inputs
def _ln_v(c):
    if c.kernel == "layernorm":
        return c.xs[:, :c.D].float() + (0 if c.rs is None else c.rs[:, :c.D].float())
    word, pos, typ = c.tables
    tok = c.ids.long().clamp(0, X.EMBED_VOCAB - 1)
    tt = torch.zeros_like(tok) if c.types is None else c.types.long().clamp(0, X.EMBED_NTYPES - 1)
    return word.float()[tok] + pos.float()[torch.arange(c.rows) % c.L] + typ.float()[tt]


def test_c_ln_is_four_times_the_worst_fp32_against_fp64():
    """The fp32 oracle (torch's order) and the kernel-order fp32 emulation against the fp64 oracle, in
    units of 2**-24 * S, over every LayerNorm and embedding case: the measured figure C_LN stands on."""
    worst = {}
    for c in X.ln_cases() + X.embed_cases():
        of = X.ln_ref if c.kernel == "layernorm" else X.embed_ref_of
        r64, r32 = of(c), of(c, F32)
        emul = X.layernorm_emul(_ln_v(c), c.gamma, c.beta, c.eps)
        unit = X.U32 * r64.S
        a, b = ((r32.y.double() - r64.y).abs() / unit).max().item(), ((emul.double() - r64.y).abs() / unit).max().item()
        worst[c.id] = max(a, b)
        print(f"[tx_oracle] {c.id}: fp32 oracle {a:.3f}, kernel-order fp32 {b:.3f} of 2**-24 S")
        assert torch.isfinite(emul).all()
    w = max(worst.values())
    print(f"[tx_oracle] worst fp32 vs fp64: {w:.3f} ({max(worst, key=worst.get)}); C_LN = {X.C_LN}, C_OPS = {X.C_OPS}")
    assert 4 * w <= X.C_LN <= X.C_OPS


@pytest.mark.parametrize("c", X.ln_cases(), ids=X.ids(X.ln_cases()))
def test_constant_row_is_beta(c):
    if c.rows > 2:
        for dt in (F32, F64):
            assert torch.equal(X.ln_ref(c, dt).y[2], c.beta.to(dt))


@pytest.mark.parametrize("c", X.att_cases(), ids=X.ids(X.att_cases()))
def test_attention_ref_fp32_within_a_quarter_of_the_bound_of_fp64(c):
    r64, r32 = X.att_ref_of(c.id), X.att_ref_of(c.id, F32)
    assert torch.isfinite(r64.y).all() and torch.isfinite(r64.A).all()
    X.check(r32.y, r64.y, X.att_bound(r64) / 4, 64, f"attention_ref fp32 vs fp64, {c.id}")
    assert X.compare(r32.A, r64.A, X.att_bound(r64) / 4, 64).ok


@pytest.mark.parametrize("c", X.qkvatt_cases(), ids=X.ids(X.qkvatt_cases()))
def test_qkvatt_ref_fp32_within_a_quarter_of_the_bound_of_fp64(c):
    r64, r32 = X.qkvatt_ref_of(c.id), X.qkvatt_ref_of(c.id, F32)
    assert torch.isfinite(r64.y).all()
    X.check(r32.y, r64.y, X.att_bound(r64) / 4, 64, f"qkvatt_ref fp32 vs fp64, {c.id}")


def test_fully_masked_sequence_is_the_mean_of_v():
    c = X.case("att-L33-seq")
    D = c.heads * 64
    v = c.qkv[:c.L, 2 * D:].double()
    assert torch.allclose(X.att_ref_of(c.id).y[:c.L], v.mean(0).expand(c.L, D), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------
# the kernels' CPU emulations pass the bound
@pytest.mark.parametrize("c", X.att_cases(), ids=X.ids(X.att_cases()))
def test_kernel_emulations_pass_the_bound(c):
    ref = X.att_ref_of(c.id)
    qkv = X.packed_qkv(c)
    one = X.attention_onepass_emul(qkv, c.B, c.L, c.heads, c.mask)
    a = X.check(one, ref.y, X.att_bound(ref), 64, f"one-pass emulation, {c.id}")
    st = _bf16(T.attention_stream_ref(qkv, c.B, c.L, c.heads, c.mask)[0])
    b = X.check(st, ref.y, X.att_bound(ref), 64, f"streamed emulation, {c.id}")
    assert max(a.ratio, b.ratio) < 0.5


# ------------------------------------------------------------------------------------------------
# planted faults: attention
def _rejects(got, ref, bound, label):
    rep = X.compare(_bf16(got), ref.y if hasattr(ref, "y") else ref, bound, 64)
    print(f"[tx_oracle] planted {label}: {X.describe(rep)}")
    assert not rep.ok and rep.ratio > 1.0, label
    return rep


def _drop_last(s):
    s = s.clone()
    s[..., -1] = float("-inf")
    return s


def _drop_median(p):
    k = p.argsort(-1)[..., p.shape[-1] // 2]
    p = p.scatter(-1, k[..., None], 0.0)
    return p / p.sum(-1, keepdim=True)


def _att(c, mask="case", qkv=None, scale=0.125, hooks=None):
    return X.attention_ref(c.qkv if qkv is None else qkv, c.B, c.L, c.heads, c.mask if isinstance(mask, str) else mask,
                           scale, c.k_off, c.v_off, hooks=hooks).y


@pytest.mark.parametrize("name", ["att-L197-half", "att-L33-none", "att-L129-inf", "stream-long-L300-masked"])
def test_comparator_rejects_planted_attention_faults(name):
    c, ref = X.case(name), X.att_ref_of(name)
    bound = X.att_bound(ref)
    assert X.compare(_bf16(ref.y), ref.y, bound, 64).ratio <= 0.5  # the rounded oracle itself: the store's half ulp
    if c.mask is None or torch.isfinite(c.mask[:, -1]).all():
        _rejects(_att(c, hooks={"s": _drop_last}), ref, bound, f"last key dropped, {name}")
    _rejects(_att(c, hooks={"p": _drop_median}), ref, bound, f"each query's median key dropped, {name}")
    rep = _rejects(_att(c, scale=0.123), ref, bound, f"scale 0.123, {name}")
    _rejects(_att(c, hooks={"pad_keys": 1}), ref, bound, f"one padding key counted, {name}")
    if c.mask is not None and not torch.equal(c.mask[0], c.mask[1]):
        _rejects(_att(c, mask=c.mask.flip(0)), ref, bound, f"the other sequence's mask, {name}")
    D = c.heads * 64
    q = c.qkv.clone()  # V rows 0..7 <-> 8..15 in head dims 0..15 of head 0, sequence 0
    q[0:8, c.v_off:c.v_off + 16], q[8:16, c.v_off:c.v_off + 16] = c.qkv[8:16, c.v_off:c.v_off + 16], c.qkv[0:8, c.v_off:c.v_off + 16]
    assert D and not torch.equal(q, c.qkv)
    _rejects(_att(c, qkv=q), ref, bound, f"eight V rows swapped in 16 head dims, {name}")


def test_what_the_attention_bound_cannot_see():
    """P truncated to bf16 instead of rounded stays inside the bound (module docstring)."""
    c, ref = X.case("att-L197-half"), X.att_ref_of("att-L197-half")

    def trunc(p):
        return (p.float().view(torch.int32) & -65536).view(torch.float32).double()

    rep = X.compare(_bf16(_att(c, hooks={"p": trunc})), ref.y, X.att_bound(ref), 64)
    print(f"[tx_oracle] P truncated: {X.describe(rep)}")
    assert rep.ok and 0.2 < rep.ratio < 0.6


# ------------------------------------------------------------------------------------------------
# planted faults: LayerNorm
def _ln_rejects(got, ref, label):
    rep = X.compare(_bf16(got), ref.y, X.ln_bound(ref))
    print(f"[tx_oracle] planted {label}: {X.describe(rep)}")
    assert not rep.ok, label


@pytest.mark.parametrize("name", ["ln-1x8", "ln-5x64", "ln-5x64-res"])
def test_comparator_rejects_the_unbiased_variance(name):
    c = X.case(name)
    ref = X.ln_ref(c)
    assert X.compare(_bf16(ref.y), ref.y, X.ln_bound(ref)).ok
    _ln_rejects(X.ln_ref(c, hooks={"var": lambda q, D: q / (D - 1)}).y, ref, f"unbiased variance, {name}")


def test_comparator_rejects_planted_layernorm_faults():
    c = X.case("ln-5x768-strided")
    ref = X.ln_ref(c)
    assert X.compare(_bf16(ref.y), ref.y, X.ln_bound(ref)).ok
    # eps dropped: the constant row (2) is 0 * inf
    got = X.ln_ref(c, hooks={"eps": lambda e: 0 * e}).y
    rep = X.compare(_bf16(got), ref.y, X.ln_bound(ref))
    assert not rep.ok and rep.row == 2 and rep.ratio == float("inf")
    # the residual read with the row stride D instead of ldr
    wrong = c.rs.reshape(-1)[: c.rows * c.D].reshape(c.rows, c.D)
    _ln_rejects(X.layernorm_ref(c.xs[:, :c.D], c.gamma, c.beta, c.eps, wrong).y, ref, "residual stride")
    # gamma / beta one 8-element chunk off
    _ln_rejects(X.layernorm_ref(c.xs[:, :c.D], c.gamma.roll(8), c.beta, c.eps, c.rs[:, :c.D]).y, ref, "gamma chunk")
    _ln_rejects(X.layernorm_ref(c.xs[:, :c.D], c.gamma, c.beta.roll(8), c.eps, c.rs[:, :c.D]).y, ref, "beta chunk")
    # one ulp of bf16 on one element
    got = _bf16(ref.y).clone()
    got[4, 5] = (got[4, 5].view(torch.int16) + 1).view(torch.bfloat16)
    rep = X.compare(got, ref.y, X.ln_bound(ref))
    assert not rep.ok and (rep.row, rep.column, rep.bad) == (4, 5, 1)


def test_comparator_counts_nan_inf_and_reports_the_head():
    ref = torch.ones(3, 128, dtype=F64)
    got = ref.clone()
    got[2, 70] = float("nan")
    rep = X.compare(got, ref, 0.1 * ref, 64)
    assert not rep.ok and (rep.row, rep.head, rep.column, rep.bad) == (2, 1, 6, 1) and rep.ratio == float("inf")
    got[2, 70] = float("inf")
    assert not X.compare(got, ref, float("inf") * ref, 64).ok  # every output must be finite
    assert X.compare(ref + 0.05, ref, 0.1 * ref, 64).ok


def test_case_list():
    ids = X.ids(X.cases())
    assert len(set(ids)) == len(ids)
    by = {k: sum(c.kernel == k for c in X.cases()) for k in ("layernorm", "embed_ln", "vit_tokens", "attention", "qkvatt", "softmax")}
    print(f"[tx_oracle] cases: {by}")
    assert by == {"layernorm": 24, "embed_ln": 4, "vit_tokens": 3, "attention": 80, "qkvatt": 28, "softmax": 7}
    assert all(c.B * c.heads <= 4 for c in X.att_cases())
