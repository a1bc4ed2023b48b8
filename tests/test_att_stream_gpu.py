"""Streamed (online-softmax) attention on MI355X: csrc/transformer.hip attention_stream_kernel
against the fp32 / fp64 oracles at every edge of its 64-key tiling and 128-query blocks, with a
forced rescale, whole masked tiles, the MX8 output, write bounds, the debug contracts, and BERT
L = 512 / ViT-384 engines and a --seq-len 512 text plan end to end. The inputs are
tests/att_stream_inputs.py's, pinned by the kernel's CPU emulation in test_att_stream_cpu.py."""
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import att_stream_inputs as I
from hipzap import _native as N
from hipzap.engine.engine import Engine
from hipzap.models import bert, vit
from hipzap.ops import fp8 as F8
from hipzap.ops import transformer as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent


def _dev(mask):
    return None if mask is None else mask.to(DEV)


@pytest.mark.parametrize("masked", [True, False], ids=["masked", "nomask"])
@pytest.mark.parametrize("B,L,heads", I.LONG)
def test_long_sequences(B, L, heads, masked):
    qkv = I.random_qkv(B, L, heads)
    mask = I.half_mask(B, L) if masked else None
    out = T.attention(qkv.to(DEV), B, L, heads, _dev(mask))
    err = I.rel(out, T.attention_ref(qkv, B, L, heads, mask))
    print(f"L={L} masked={masked}: {err:.3e}")
    assert err < 2e-2, err


# the child runs every SHORT input through the streamed kernel (the switch is read once per
# process) and checks it against the fp32 oracle; the outputs come back for the comparison with
# the one-pass kernel, which this process runs
FORCED_CHILD = r"""
import sys, torch
sys.path.insert(0, "tests")
import att_stream_inputs as I
from hipzap.ops import transformer as T
outs, errs = {}, {}
for B, L, H in I.SHORT:
    qkv, mask = I.random_qkv(B, L, H), I.half_mask(B, L)
    o = T.attention(qkv.to("cuda:0"), B, L, H, mask.to("cuda:0")).cpu()
    outs[L], errs[L] = o, I.rel(o, T.attention_ref(qkv, B, L, H, mask))
torch.save({"outs": outs, "errs": errs}, sys.argv[1])
"""


def test_forced_stream_on_the_one_pass_ground(tmp_path):
    res = str(tmp_path / "forced.pt")
    env = dict(os.environ, HIPZAP_ATT_STREAM="1", HIPZAP_NO_AUTOBUILD="1")
    r = subprocess.run([sys.executable, "-c", FORCED_CHILD, res], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    got = torch.load(res)
    assert not os.environ.get("HIPZAP_ATT_STREAM"), "this process must run the one-pass kernel"
    for B, L, H in I.SHORT:
        one = T.attention(I.random_qkv(B, L, H).to(DEV), B, L, H, I.half_mask(B, L).to(DEV))
        vs_one = I.rel(got["outs"][L], one)
        print(f"L={L}: streamed vs oracle {got['errs'][L]:.3e}, vs one-pass {vs_one:.3e}")
        assert torch.isfinite(got["outs"][L].float()).all()
        assert got["errs"][L] < 2e-2, (L, got["errs"][L])
        assert vs_one < 2e-2, (L, vs_one)


@pytest.mark.parametrize("name", sorted(I.SPIKE_AT))
def test_forced_rescale_against_fp64(name):
    """spike_last: every query's running max jumps by ~30 at the last tile, so everything
    accumulated before is rescaled by exp(-30) (a kernel that skipped it would return the mean of
    the earlier V rows, an O(1) error); spike_first: the max never grows after tile 0. Full-tensor
    fp64 host reference."""
    qkv = I.spike(name)
    out = T.attention(qkv.to(DEV), 1, I.SPIKE_L, I.SPIKE_HEADS, None)
    err = I.rel(out, I.attention_ref64(qkv, 1, I.SPIKE_L, I.SPIKE_HEADS))
    print(f"{name}: vs fp64 {err:.3e}")
    assert torch.isfinite(out.float()).all() and err < 2e-2, err


@pytest.mark.parametrize("value", [-1e9, float("-inf")], ids=["1e9", "inf"])
def test_whole_first_tile_masked(value):
    """A tile whose real keys are all masked must not poison the accumulators: with -inf the running
    max is still -inf after it (exp(-inf - -inf) is NaN unguarded); with -1e9 the tile's p = 1 must
    be rescaled away by the first real tile."""
    B, L, H = 2, 320, 2
    qkv, mask = I.random_qkv(B, L, H), I.tile_mask(value, B, L)
    out = T.attention(qkv.to(DEV), B, L, H, mask.to(DEV))
    assert torch.isfinite(out.float()).all()
    err = I.rel(out, T.attention_ref(qkv, B, L, H, mask))
    print(f"first tile at {value}: {err:.3e}")
    assert err < 2e-2, err


def test_mx8_output():
    """tests/test_fp8_gpu.py test_attention_mx8_output at L = 320: within one e4m3 step."""
    B, L, H = 2, 320, 2
    D = H * 64
    qkv = I.random_qkv(B, L, H)
    ref = T.attention_ref(qkv, B, L, H, None)
    o8 = torch.zeros(B * L, D, dtype=torch.uint8, device=DEV)
    os8 = torch.zeros(B * L, H * 2, dtype=torch.uint8, device=DEV)
    q = qkv.to(DEV)
    prm = T.AttentionParams(q.data_ptr(), 0, 0, B, L, H, 64, q.stride(0), D, 2 * D, D, 0.125, o8.data_ptr(),
                            os8.data_ptr())
    N.check(N.lib().hz_launch_kernel(T.K_ATTENTION, ctypes.byref(prm), N.stream_ptr()), "attention mx8")
    torch.cuda.synchronize()
    sc = torch.ldexp(torch.ones(os8.shape), os8.cpu().long() - 127).repeat_interleave(32, 1)
    got = o8.cpu().view(torch.float8_e4m3fn).float() * sc
    ref_q, _ = F8.quant_mx_ref(ref.float())
    err = ((got - ref_q).abs().max() / ref_q.abs().max()).item()
    print(f"mx8 L={L}: {err:.3e}")
    assert err < 0.1, err  # <= one e4m3 step


def test_write_bounds():
    """Every one of the B*L rows is written (the last 128-query block holds 44 real queries) and
    the row after them is not."""
    B, L, H = 2, 300, 2
    D = H * 64
    qkv = I.random_qkv(B, L, H)
    buf = torch.full((B * L + 1, D), float("nan"), dtype=torch.bfloat16, device=DEV)
    T.attention(qkv.to(DEV), B, L, H, None, out=buf[: B * L])
    torch.cuda.synchronize()
    assert not torch.isnan(buf[: B * L].float()).any()
    assert torch.isnan(buf[B * L].float()).all()
    assert I.rel(buf[: B * L], T.attention_ref(qkv, B, L, H, None)) < 2e-2


DEBUG_CHILD = r"""
import json, os, sys, torch
sys.path.insert(0, "tests")
import att_stream_inputs as I
from hipzap import _native as N
from hipzap.ops import transformer as T
from hipzap.utils import kcheck
assert N.DEBUG and os.path.basename(N._LIB_PATH) == "libhipzap_debug.so", N._LIB_PATH
B, L, H = 2, 300, 2
qkv, mask = I.random_qkv(B, L, H), I.half_mask(B, L)
o = T.attention(qkv.to("cuda:0"), B, L, H, mask.to("cuda:0"))
torch.cuda.synchronize()
print("RESULT " + json.dumps({"fails": kcheck.poll(), "err": I.rel(o, T.attention_ref(qkv, B, L, H, mask))}))
"""


def test_debug_contracts_hold():
    lib = ROOT / "hipzap" / "_lib" / "libhipzap_debug.so"
    assert lib.exists(), "build it first: python -m hipzap.build --debug"
    env = dict(os.environ, HIPZAP_DEBUG="1", HIPZAP_NO_AUTOBUILD="1")
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["fails"] == [] and res["err"] < 2e-2, res


# ----------------------------------------------------------------------------- engines
@pytest.fixture(scope="module")
def bert2():
    """A 2-layer BERT with randomised LayerNorm affine parameters (as test_bert_engine_matches_hf),
    B = 2 requests of L = 512, the second padded from token 300, and the HF fp32 logits."""
    torch.manual_seed(0)
    m = bert.make_model(num_labels=2, num_hidden_layers=2)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "LayerNorm" in name:
                p.add_(0.3 * torch.randn_like(p))
    B, L = 2, 512
    ids = torch.randint(0, 30000, (B, L))
    am = torch.ones(B, L, dtype=torch.long)
    am[1, 300:] = 0
    with torch.no_grad():
        ref = m(input_ids=ids, attention_mask=am).logits
    return {"model": m, "sd": m.state_dict(), "ids": ids, "am": am, "ref": ref, "B": B, "L": L}


def test_bert_512_engine_matches_hf(bert2):
    eng = Engine.from_state_dict("bert-base", bert2["sd"], DEV, batch=bert2["B"], arch_kw={"seq_len": bert2["L"]})
    assert [n.attrs["L"] for n in eng.graph.nodes if n.kind == "attention"] == [512, 512]
    out = eng.infer(bert.encode_inputs(bert2["ids"], None, bert2["am"])).float().cpu()
    ref = bert2["ref"]
    print(f"bert L=512: {I.rel(out, ref):.3e}", out, ref)
    assert out.shape == (2, 2)
    assert I.rel(out, ref) < 5e-2, (out, ref)
    assert torch.equal(out.argmax(1), ref.argmax(1))


def test_bert_512_fp8_engine(bert2):
    """test_bert_fp8_engine_matches_graph_oracle_and_hf's bounds: 0.15 against the fp32 graph oracle
    of the same quantisation, 0.25 against HF fp32 (no argmax there either: e4m3 noise may swap the
    near-tie of two small random-init logits)."""
    from hipzap.engine.reference import run_graph_reference
    from hipzap.models import registry
    eng = Engine.from_state_dict("bert-base-fp8", bert2["sd"], DEV, batch=bert2["B"], arch_kw={"seq_len": bert2["L"]})
    inputs = bert.encode_inputs(bert2["ids"], None, bert2["am"])
    out = eng.infer(inputs).float().cpu()
    P, _ = registry.get("bert-base-fp8").pack(bert2["sd"], "cpu")
    oracle = run_graph_reference(eng.graph, P, inputs)[eng.graph.outputs[0]].reshape(bert2["B"], -1)[:, :2]
    print(f"bert-fp8 L=512: vs oracle {I.rel(out, oracle):.3e}, vs HF {I.rel(out, bert2['ref']):.3e}")
    assert out.shape == (2, 2)
    assert I.rel(out, oracle) < 0.15, (out, oracle)
    assert I.rel(out, bert2["ref"]) < 0.25, (out, bert2["ref"])


def test_vit_384_engine_matches_hf():
    torch.manual_seed(0)
    m = vit.make_model(num_labels=1000, num_hidden_layers=2, image_size=384)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "layernorm" in name:
                p.add_(0.3 * torch.randn_like(p))
    eng = Engine.from_state_dict("vit-b16", m.state_dict(), DEV, batch=1)
    assert [n.attrs["L"] for n in eng.graph.nodes if n.kind == "attention"] == [577, 577]
    x = torch.randn(1, 3, 384, 384)
    out = eng.infer(x).float().cpu()
    with torch.no_grad():
        ref = m(pixel_values=x).logits
    print(f"vit-384: {I.rel(out, ref):.3e}")
    assert out.shape == (1, 1000)
    assert I.rel(out, ref) < 5e-2
    assert torch.equal(out.argmax(1), ref.argmax(1))


def test_text_plan_512_equals_engine(bert2, tmp_path):
    """``hipzap plan --model bert-base --seq-len 512`` through hipzap/lite.py (PlanTextBackend) and
    the torch-built engine run the same program: tests/test_text_plan_gpu.py's comparison."""
    from hipzap.engine.plan import export_from_checkpoint
    from hipzap.serve.server import PlanTextBackend
    from hipzap.serve.settings import ModelSpec
    ckpt = str(tmp_path / "bert2.pth")
    torch.save(bert2["sd"], ckpt)
    plan = export_from_checkpoint("bert-base", ckpt, str(tmp_path / "bert2.hzplan"), batch=2, seq_len=512)
    be = PlanTextBackend("bert-base", plan, 0, ModelSpec(name="bert-base", contexts=1))
    try:
        assert be.seq_len == 512
        got = be.infer_np(bert2["ids"].numpy(), None, bert2["am"].numpy())
        with pytest.raises(ValueError):
            be.infer_np(np.zeros((1, 513), np.int64))
    finally:
        be.engine.close()
    eng = Engine.from_state_dict("bert-base", bert2["sd"], DEV, batch=2, arch_kw={"seq_len": 512})
    ref = eng.infer(bert.encode_inputs(bert2["ids"], None, bert2["am"])).float().cpu().numpy()
    print("plan vs engine", np.abs(got - ref).max(), got, ref)
    assert np.abs(got - ref).max() <= 2e-2 * np.abs(ref).max() + 1e-3, (got, ref)
