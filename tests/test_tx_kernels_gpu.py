"""The transformer kernels of csrc/transformer.hip, each alone on MI355X against the fp64 oracle of the
same op (tests/tx_oracle.py), element by element under the derived bounds:

* ``layernorm_kernel`` (every NC, strided rows, the fp8 output) and ``embed_ln_kernel`` (id / type clamps,
  ``row % L``, ``types == nullptr``): ``|got - ref| <= ulp_bf16(ref) / 2 + C_LN 2**-24 S``;
* ``attention_kernel``, ``attention_stream_kernel`` and ``qkvatt_kernel`` (the edges of the 32-key padding
  and of the 16-, 64- and 128-query blocks; -1e9, whole-sequence and -inf masks; K / V offsets and row
  strides): ``|got - ref| <= 2**-7 |ref| + 2**-7 A``;
* ``vit_tokens_kernel``: bitwise; ``softmax_kernel`` (mask, D = 1, D = 65, ld > D): 1e-5 of the fp64 oracle;
* the variants a once-per-process switch selects (``HIPZAP_LN_RPW``, ``HIPZAP_QKVATT_NS``,
  ``HIPZAP_ATT_NW8_MINL``, ``HIPZAP_ATT_NW16``), each in a fresh child process: inside the bound, and bitwise
  the default process's outputs.

Every output goes into a NaN-filled buffer with a guard row after the last row and guard columns where
the row stride exceeds D: the guards must still be NaN, every real element finite and inside the bound.
The inputs and references are those tests/test_tx_oracle_cpu.py judges on the CPU."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import tx_oracle as X
from hipzap import _native as N
from hipzap.ops import transformer as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
BF16 = torch.bfloat16
E4M3_NAN = 0x7F  # the fp8 guard rows are filled with it


def _rc(kind, prm):
    return N.lib().hz_launch_kernel(kind, ctypes.byref(prm), N.stream_ptr())


def _launch(kind, prm, what):
    N.check(_rc(kind, prm), what)
    torch.cuda.synchronize()


def _nan(rows, ld, dtype=BF16):
    """[rows + 1, ld] of NaN: the kernel's output rows and a guard row."""
    return torch.full((rows + 1, ld), float("nan"), dtype=dtype, device=DEV)


def _take(buf, rows, D, what):
    """The real elements of a guarded output buffer; the guard row and the guard columns must be NaN."""
    b = buf.cpu()
    assert torch.isnan(b[rows].float()).all(), f"{what}: the row after the last row was written"
    assert torch.isnan(b[:rows, D:].float()).all(), f"{what}: columns past D were written"
    return b[:rows, :D].contiguous()


def _d(t):
    return None if t is None else t.contiguous().to(DEV)


# ------------------------------------------------------------------------------------------------
# one launch per case; -> dict of CPU tensors
def run_layernorm(c):
    xs, rs, g, b = _d(c.xs), _d(c.rs), _d(c.gamma), _d(c.beta)
    out = None if c.fp8 == "only" else _nan(c.rows, c.ldo)
    o8 = s8 = None
    if c.fp8:
        o8 = torch.full((c.rows + 1, c.D), E4M3_NAN, dtype=torch.uint8, device=DEV)
        s8 = torch.full((c.rows + 1,), float("nan"), dtype=torch.float32, device=DEV)
    prm = T.LayerNormParams(xs.data_ptr(), N.ptr(rs), N.ptr(out), g.data_ptr(), b.data_ptr(), c.rows, c.D, c.ldx,
                            c.ldr if rs is not None else 0, c.ldo, c.eps, N.ptr(o8), N.ptr(s8))
    _launch(T.K_LAYERNORM, prm, c.id)
    res = {}
    if out is not None:
        res["out"] = _take(out, c.rows, c.D, c.id)
    if c.fp8:
        o8, s8 = o8.cpu(), s8.cpu()
        assert (o8[c.rows] == E4M3_NAN).all() and torch.isnan(s8[c.rows]), f"{c.id}: fp8 guard row written"
        res["out8"], res["scale8"] = o8[:c.rows].contiguous(), s8[:c.rows].contiguous()
    return res


def run_embed_ln(c):
    ids, types, g, b = _d(c.ids), _d(c.types), _d(c.gamma), _d(c.beta)
    word, pos, typ = (_d(t) for t in c.tables)
    out = _nan(c.rows, c.D)
    prm = T.EmbedParams(ids.data_ptr(), N.ptr(types), word.data_ptr(), pos.data_ptr(), typ.data_ptr(), g.data_ptr(),
                        b.data_ptr(), out.data_ptr(), c.rows, c.L, c.D, c.eps, X.EMBED_VOCAB, X.EMBED_NTYPES)
    _launch(T.K_EMBED, prm, c.id)
    return {"out": _take(out, c.rows, c.D, c.id)}


def run_vit_tokens(c):
    patches, cls, pos = _d(c.patches), _d(c.cls), _d(c.pos)
    rows = c.B * (c.np + 1)
    out = _nan(rows, c.D)
    prm = T.VitTokensParams(patches.data_ptr(), cls.data_ptr(), pos.data_ptr(), out.data_ptr(), c.B, c.np, c.D)
    _launch(T.K_VIT_TOKENS, prm, c.id)
    return {"out": _take(out, rows, c.D, c.id)}


def run_attention(c):
    qkv, mask = _d(c.qkv), _d(c.mask)
    D, rows = c.heads * 64, c.B * c.L
    out = _nan(rows, c.ldo)
    prm = T.AttentionParams(qkv.data_ptr(), N.ptr(mask), out.data_ptr(), c.B, c.L, c.heads, 64, qkv.stride(0), c.k_off,
                            c.v_off, c.ldo, 0.125)
    _launch(T.K_ATTENTION, prm, c.id)
    return {"out": _take(out, rows, D, c.id)}


_WEIGHTS = {}


def run_qkvatt(c):
    if c.heads not in _WEIGHTS:
        _WEIGHTS[c.heads] = X.qkvatt_weights(c.heads).to(DEV)
    pc, xs, mask = _WEIGHTS[c.heads], _d(c.xs), _d(c.mask)
    rows = c.B * c.L
    out = _nan(rows, c.ldo)
    prm = T.QkvAttParams(xs.data_ptr(), pc.wf.data_ptr(), pc.bias.data_ptr(), N.ptr(mask), out.data_ptr(), c.B, c.L,
                         c.heads, c.D, pc.ksteps, c.ldx, c.ldo, 0.125)
    _launch(T.K_QKVATT, prm, c.id)
    return {"out": _take(out, rows, c.D, c.id)}


def run_softmax(c):
    out = _nan(c.rows, c.ldo, torch.float32)
    T.softmax(_d(c.x), cols=c.D, scale=c.scale, mask=_d(c.mask), out=out[:c.rows])
    torch.cuda.synchronize()
    return {"out": _take(out, c.rows, c.D, c.id)}


_RUN = {"layernorm": run_layernorm, "embed_ln": run_embed_ln, "vit_tokens": run_vit_tokens, "attention": run_attention,
        "qkvatt": run_qkvatt, "softmax": run_softmax}
_RESULTS = {}


def run(c):
    """The case's outputs in this process (launched once, shared by the bitwise comparisons)."""
    if c.id not in _RESULTS:
        _RESULTS[c.id] = _RUN[c.kernel](c)
    return _RESULTS[c.id]


# ------------------------------------------------------------------------------------------------
# the verdicts
def judge_ln(c, res):
    ref = X.ln_ref(c) if c.kernel == "layernorm" else X.embed_ref_of(c)
    ratio = 0.0
    if "out" in res:
        ratio = X.check(res["out"], ref.y, X.ln_bound(ref), label=c.id).ratio
        # (an element near a rounding tie sits at the bound by construction; what it uses of the fp32 term:)
        over = ((res["out"].double() - ref.y).abs() - X.ulp_bf16(ref.y) / 2) / X.fp32_term(ref)
        print(f"[tx_oracle] {c.id}: fp32 term used {max(over.max().item(), 0.0):.3f}")
    if "out8" in res:
        # the row scale is amax / 448 of the kernel's own unrounded y: the oracle's, to within the fp32 term
        # (|max |a| - max |b|| <= max |a - b|) and the roundings of the division
        amax = ref.y.abs().amax(-1).clamp_min(1e-12)
        s8 = res["scale8"].double()
        tol = (X.fp32_term(ref).amax(-1) + 4 * X.U32 * amax) / 448
        print(f"[tx_oracle] {c.id}: scale8 worst err/tol {((s8 - amax / 448).abs() / tol).max():.3f}")
        assert torch.isfinite(s8).all() and ((s8 - amax / 448).abs() <= tol).all(), (s8, amax / 448)
        # the dequantised values: within one e4m3 step (at the element's size in scale units) of the oracle
        deq = res["out8"].view(torch.float8_e4m3fn).float().double() * s8[:, None]
        step = X.ulp_e4m3(ref.y / s8[:, None]) * s8[:, None]
        r8 = X.check(deq, ref.y, step + X.fp32_term(ref), label=f"{c.id} fp8 dequantised")
        ratio = max(ratio, r8.ratio)
    return ratio


def judge_att(c, res):
    ref = X.att_ref_of(c.id) if c.kernel == "attention" else X.qkvatt_ref_of(c.id)
    return X.check(res["out"], ref.y, X.att_bound(ref), 64, c.id).ratio


def judge_vit(c, res):
    ref = X.vit_tokens_ref(c.patches, c.cls, c.pos, c.B, c.np)
    assert torch.equal(res["out"].view(torch.int16), ref.view(torch.int16)), c.id
    return 0.0


def judge_softmax(c, res):
    ref = T.softmax_ref(c.x, c.D, c.scale, c.mask, dtype=torch.float64)
    err = (res["out"].double() - ref).abs().max().item()
    print(f"[tx_oracle] {c.id}: max |err| {err:.3e}")
    assert torch.isfinite(res["out"]).all() and err < 1e-5, (c.id, err)
    if c.mask is not None:
        assert (res["out"][:, torch.isinf(c.mask)] == 0).all()
    return err


_JUDGE = {"layernorm": judge_ln, "embed_ln": judge_ln, "vit_tokens": judge_vit, "attention": judge_att,
          "qkvatt": judge_att, "softmax": judge_softmax}


def judge(c, res):
    return _JUDGE[c.kernel](c, res)


def _bitwise(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (what, k)
        same = torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)) if a[k].dtype == torch.uint8 else \
            torch.equal(a[k].contiguous().view(torch.int16 if a[k].dtype == BF16 else torch.int32),
                        b[k].contiguous().view(torch.int16 if b[k].dtype == BF16 else torch.int32))
        assert same, f"{what}: {k} differs in {(a[k].float() != b[k].float()).sum().item()} elements"


# ------------------------------------------------------------------------------------------------
# every kernel alone, in the default process
@pytest.mark.parametrize("c", X.ln_cases(), ids=X.ids(X.ln_cases()))
def test_layernorm_kernel_vs_fp64(c):
    res = run(c)
    judge(c, res)
    if c.rows > 2 and "out" in res:  # the constant row: d = 0 exactly, y = beta whatever eps is
        assert torch.equal(res["out"][2], c.beta.to(BF16)), c.id


def test_layernorm_bf16_output_is_the_same_with_and_without_fp8():
    plain, both = X.case("ln-5x768-res"), X.case("ln-5x768-res-fp8both")
    assert torch.equal(plain.xs, both.xs) and torch.equal(plain.rs, both.rs) and plain.eps == both.eps
    _bitwise({"out": run(plain)["out"]}, {"out": run(both)["out"]}, "layernorm with and without out8")


def test_layernorm_launcher_refuses():
    """D = 2056 (> 2048) and D = 12 (not a multiple of 8); the buffers would hold either."""
    x = torch.zeros(2, 2064, dtype=BF16, device=DEV)
    out, g = torch.zeros_like(x), torch.zeros(2064, device=DEV)
    for D in (2056, 12):
        prm = T.LayerNormParams(x.data_ptr(), 0, out.data_ptr(), g.data_ptr(), g.data_ptr(), 2, D, 2064, 0, 2064, 1e-5)
        assert _rc(T.K_LAYERNORM, prm) != 0, D
    prm.D = 2048
    assert _rc(T.K_LAYERNORM, prm) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", X.embed_cases(), ids=X.ids(X.embed_cases()))
def test_embed_ln_kernel_vs_fp64(c):
    judge(c, run(c))


def test_embed_ln_launcher_refuses():
    """D % 8 != 0, D > 2048, vocab < 1 (the clamp needs a non-empty table)."""
    tab = torch.zeros(4, 2064, dtype=BF16, device=DEV)
    ids, g = torch.ones(2, dtype=torch.int32, device=DEV), torch.zeros(2064, device=DEV)
    out = torch.zeros(2, 2064, dtype=BF16, device=DEV)

    def prm(D, vocab):  # (the word table starts at row 1 of ``tab``)
        return T.EmbedParams(ids.data_ptr(), 0, tab[1:].data_ptr(), tab.data_ptr(), tab.data_ptr(), g.data_ptr(),
                             g.data_ptr(), out.data_ptr(), 2, 2, D, 1e-12, vocab, 2)

    for D, vocab in ((12, 3), (2056, 3), (768, 0), (768, -1)):
        assert _rc(T.K_EMBED, prm(D, vocab)) != 0, (D, vocab)
    assert _rc(T.K_EMBED, prm(768, 3)) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", X.vit_cases(), ids=X.ids(X.vit_cases()))
def test_vit_tokens_kernel_bitwise(c):
    judge(c, run(c))


@pytest.mark.parametrize("c", X.att_cases(), ids=X.ids(X.att_cases()))
def test_attention_kernels_vs_fp64(c):
    """One-pass up to L = 256, streamed beyond (this process has no switch set)."""
    assert not any(os.environ.get(k) for k in ("HIPZAP_ATT_STREAM", "HIPZAP_ATT_NW16", "HIPZAP_ATT_NW8_MINL"))
    judge(c, run(c))


@pytest.mark.parametrize("c", X.qkvatt_cases(), ids=X.ids(X.qkvatt_cases()))
def test_qkvatt_kernel_vs_fp64(c):
    assert not os.environ.get("HIPZAP_QKVATT_NS")
    judge(c, run(c))


def test_qkvatt_launcher_refuses_more_than_one_tile():
    c = X.case("qkvatt-2x128x2-none")
    pc, xs = X.qkvatt_weights(c.heads).to(DEV), torch.zeros(2 * 129, c.D, dtype=BF16, device=DEV)
    out = torch.zeros_like(xs)
    prm = T.QkvAttParams(xs.data_ptr(), pc.wf.data_ptr(), pc.bias.data_ptr(), 0, out.data_ptr(), 2, 129, c.heads, c.D,
                         pc.ksteps, c.D, c.D, 0.125)
    assert _rc(T.K_QKVATT, prm) != 0


@pytest.mark.parametrize("c", X.softmax_cases(), ids=X.ids(X.softmax_cases()))
def test_softmax_kernel_vs_fp64(c):
    judge(c, run(c))


# ------------------------------------------------------------------------------------------------
# the variants a switch selects. Every switch is read once per process (a static in its launcher), so
# each setting gets a fresh child process, one after another; the child judges its own outputs against
# the bound and sends them back for the bitwise comparison with this process's.
_ONE_PASS = [c.id for c in X.att_cases() if c.L <= 256 and c.id.startswith("att-")]
VARIANTS = {
    # layernorm_kernel<NC, 2> / <NC, 4>: "same per-row math in the same order" (the kernel's comment)
    "HIPZAP_LN_RPW=2": X.ids(X.ln_cases()),
    "HIPZAP_LN_RPW=4": X.ids(X.ln_cases()),
    # qkvatt_kernel<3>: the MFMA order does not depend on the stage count (heads = 1: nst = 1 < NS - 1)
    "HIPZAP_QKVATT_NS=3": X.ids(X.qkvatt_cases()),
    # attention_kernel<4> above L = 64 and <16> above 128: a wave's 16 queries see the same keys in the
    # same order whatever the workgroup size
    "HIPZAP_ATT_NW8_MINL=256": _ONE_PASS,
    "HIPZAP_ATT_NW16=1": [i for i in _ONE_PASS if X.case(i).L in (129, 197, 256)],
}

CHILD = r"""
import sys
sys.path.insert(0, "tests")
import test_tx_kernels_gpu as G
G.child(sys.argv[1], sys.argv[2])
"""


def child(setting, path):
    """(In the child process.) Run and judge every case of ``setting``; save the outputs."""
    name, value = setting.split("=")
    assert os.environ.get(name) == value
    outs, ratios = {}, {}
    for i in VARIANTS[setting]:
        outs[i] = run(X.case(i))
        ratios[i] = judge(X.case(i), outs[i])
    torch.save({"outs": outs, "ratios": ratios}, path)


@pytest.mark.parametrize("setting", sorted(VARIANTS))
def test_switch_variant_is_inside_the_bound_and_bitwise_the_default(setting, tmp_path):
    name, value = setting.split("=")
    assert not os.environ.get(name), "this process must run the default kernels"
    res = str(tmp_path / "variant.pt")
    env = dict(os.environ, HIPZAP_NO_AUTOBUILD="1", **{name: value})
    r = subprocess.run([sys.executable, "-c", CHILD, setting, res], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-4000:])
    got = torch.load(res)
    assert sorted(got["outs"]) == sorted(VARIANTS[setting])
    print(f"[tx_oracle] {setting}: {len(got['outs'])} cases inside the bound, worst err/bound {max(got['ratios'].values()):.3f}")
    for i in VARIANTS[setting]:
        _bitwise(got["outs"][i], run(X.case(i)), f"{setting} vs the default, {i}")
