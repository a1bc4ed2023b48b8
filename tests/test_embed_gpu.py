"""The embedding head on the GPU: ``pool_embed_kernel`` (csrc/transformer.hip, kind 29) against the
fp64 oracle, its independence of the batch around a sequence, the launcher's refusals, the BERT / ViT
embedding engines against HF fp32, the ``.emb.hzplan`` plan path, and the classification graphs unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

from hipzap import _native as N
from hipzap.engine import plan as P
from hipzap.engine.engine import Engine
from hipzap.models import bert, registry, vit
from hipzap.ops import transformer as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rel(a, b):
    return ((a.float().cpu() - b.float().cpu()).abs().max() / (b.float().abs().max() + 1e-6)).item()


def _mask(kind, B, L, seed=0):
    """Additive fp32 mask [B, L] (0 counts, -1e9 does not), or None."""
    if kind == "none":
        return None
    on = torch.ones(B, L)
    g = torch.Generator().manual_seed(seed)
    if kind == "prefix":
        for b in range(B):
            on[b, 1 + (7 * b + L // 2) % L:] = 0
    elif kind == "prefix300":
        on[:, 300:] = 0
    elif kind == "holes":
        on = (torch.rand(B, L, generator=g) < 0.6).float()
        on[:, 0] = 1
    elif kind == "row2":
        on[:, L // 2:] = 0
        on[2] = 0
    else:
        raise KeyError(kind)
    return (1.0 - on) * -1e9


def _bound(x, B, L, mask, mode, first):
    """Per element: L * 2^-23 * mean over the counted tokens of |x[t][d]| + 2^-24 * |ref| (the fp32
    recursive-sum bound for any order plus the final rounding), and the un-normalised fp64 reference."""
    ref = T.pool_embed_ref(x, B, L, mask, mode, first, normalize=False)
    mean_abs = T.pool_embed_ref(x.float().abs(), B, L, mask, mode, first, normalize=False)
    return L * 2.0 ** -23 * mean_abs + 2.0 ** -24 * ref.abs(), ref


CASES = [(1, 1, 64, 0, "none", "mean"), (3, 7, 64, 0, "prefix", "mean"), (2, 33, 768, 0, "holes", "mean"),
         (5, 197, 768, 1, "none", "mean"), (2, 128, 1024, 0, "prefix", "mean"), (1, 512, 768, 0, "prefix300", "mean"),
         (4, 40, 768, 0, "row2", "mean"), (3, 40, 768, 0, "holes", "cls"), (2, 16, 2048, 0, "none", "mean")]


def _check(out, x, B, L, D, mask, mode, first, normalize):
    out = out.double().cpu()
    bound, ref = _bound(x[:, :D], B, L, mask, mode, first)
    assert torch.isfinite(out).all()
    if not normalize:
        err = (out - ref).abs()
        print(f"max err/bound {float((err / bound.clamp(min=1e-300)).max()):.3f}")
        assert (err <= bound).all()
        return
    nrm = ref.norm(dim=1, keepdim=True)
    live = nrm[:, 0] > 0
    refn = ref / nrm.clamp(min=1e-12)
    err = (out - refn).abs()[live]
    lim = (3 * bound / nrm.clamp(min=1e-12))[live]
    print(f"normalised: max err/limit {float((err / lim.clamp(min=1e-300)).max()):.3f}, "
          f"max | ||out|| - 1 | {float((out[live].norm(dim=1) - 1).abs().max()):.3e}")
    assert ((out[live].norm(dim=1) - 1).abs() <= D * 2.0 ** -23).all()
    assert (err <= lim).all()
    assert (out[~live] == 0).all()


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("B,L,D,first,mk,mode", CASES)
def test_kernel_matches_the_fp64_oracle(B, L, D, first, mk, mode, normalize):
    g = torch.Generator().manual_seed(B * 1000 + L)
    x = (torch.randn(B * L, D, generator=g) + 0.25).to(torch.bfloat16)
    mask = _mask(mk, B, L)
    out = T.pool_embed(x.to(DEV), B, L, None if mask is None else mask.to(DEV), mode, first, normalize)
    torch.cuda.synchronize()
    assert out.shape == (B, D) and out.dtype == torch.float32
    _check(out, x, B, L, D, mask, mode, first, normalize)
    if mode == "cls" and not normalize:  # bitwise the bf16 row
        assert torch.equal(out.cpu().view(torch.int32), x.reshape(B, L, D)[:, 0].float().view(torch.int32))
    if mk == "row2":
        assert (out[2].cpu().view(torch.int32) == 0).all()  # no counted token: exactly zero


@pytest.mark.parametrize("normalize", [False, True])
def test_kernel_strided_rows_and_pad_columns(normalize):
    B, L, D = 3, 21, 768
    g = torch.Generator().manual_seed(5)
    xw = torch.randn(B * L, D + 64, generator=g).to(torch.bfloat16)
    mask = _mask("prefix", B, L)
    out = torch.full((B, D + 4), 7.0, device=DEV)
    T.pool_embed(xw.to(DEV), B, L, mask.to(DEV), "mean", 0, normalize, D=D, out=out)
    torch.cuda.synchronize()
    assert (out[:, D:].cpu().view(torch.int32) == 0).all()
    _check(out[:, :D], xw, B, L, D, mask, "mean", 0, normalize)


@pytest.mark.parametrize("D", [768, 2048])
def test_a_sequence_does_not_depend_on_its_batch(D):
    L = 53
    g = torch.Generator().manual_seed(9)
    seq = torch.randn(L, D, generator=g).to(torch.bfloat16)
    m1 = _mask("holes", 1, L, seed=3)
    x5 = torch.randn(5 * L, D, generator=g).to(torch.bfloat16)
    x5[4 * L:] = seq
    m5 = _mask("holes", 5, L, seed=4)
    m5[4] = m1[0]
    for normalize in (False, True):
        a = T.pool_embed(seq.to(DEV), 1, L, m1.to(DEV), "mean", 0, normalize)
        b = T.pool_embed(x5.to(DEV), 5, L, m5.to(DEV), "mean", 0, normalize)
        b2 = T.pool_embed(x5.to(DEV), 5, L, m5.to(DEV), "mean", 0, normalize)
        torch.cuda.synchronize()
        assert torch.equal(a[0].view(torch.int32), b[4].view(torch.int32))
        assert torch.equal(b.view(torch.int32), b2.view(torch.int32))


@pytest.mark.parametrize("what", ["D=100", "D=2056", "L=0", "first=L", "ldx<D"])
def test_launcher_refuses_and_touches_nothing(what):
    B, L, D = 2, 8, 64
    x = torch.full((B * L, 2056 + 8), 1.0, dtype=torch.bfloat16, device=DEV)
    mask = torch.zeros(B, L, device=DEV)
    out = torch.full((B, 2056 + 8), 7.0, device=DEV)
    prm = T.PoolEmbedParams(x.data_ptr(), mask.data_ptr(), out.data_ptr(), B, L, D, x.stride(0), out.stride(0), 0, 1, 1)
    if what == "D=100":
        prm.D = 100
    elif what == "D=2056":
        prm.D = 2056
    elif what == "L=0":
        prm.L = 0
    elif what == "first=L":
        prm.first = L
    else:
        prm.ldx = D - 8
    rc = N.lib().hz_launch_kernel(N.HZ_K_POOL_EMBED, C.byref(prm), N.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0
    assert (out == 7.0).all() and (x == 1.0).all() and (mask == 0).all()


# ---------------------------------------------------------------- engines against HF fp32
def _perturb_ln(m):
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "LayerNorm" in name or "layernorm" in name:
                p.add_(0.3 * torch.randn_like(p))
    return m


def _cos(a, b):
    return torch.nn.functional.cosine_similarity(a.double(), b.double(), dim=1)


@pytest.fixture(scope="module")
def bert2():
    """A 2-layer BertModel, its inputs (B=3, L=40: full, prefix 17, token 0 only) and the fp32 / bf16 HF
    hidden states on the CPU (the bf16 run is the yardstick for 1 - cos)."""
    from transformers import BertConfig, BertModel
    torch.manual_seed(0)
    m = _perturb_ln(BertModel(BertConfig(num_hidden_layers=2), add_pooling_layer=False).eval())
    B, L = 3, 40
    ids = torch.randint(0, 30000, (B, L))
    am = torch.ones(B, L, dtype=torch.long)
    am[1, 17:] = 0
    am[2, 1:] = 0
    with torch.no_grad():
        h32 = m(input_ids=ids, attention_mask=am).last_hidden_state
        mb = BertModel(m.config, add_pooling_layer=False).eval()
        mb.load_state_dict(m.state_dict())
        h16 = mb.to(torch.bfloat16)(input_ids=ids, attention_mask=am).last_hidden_state.float()
    return m.state_dict(), ids, am, h32, h16


@pytest.mark.parametrize("model,rel", [("bert-base", 5e-2), ("bert-base-fp8", 0.15)])
@pytest.mark.parametrize("pooling", ["mean", "cls"])
def test_bert_embedding_engine_matches_hf(bert2, pooling, model, rel):
    sd, ids, am, h32, h16 = bert2
    B, L = ids.shape
    eng = Engine.from_state_dict(model, sd, DEV, batch=B,
                                 arch_kw={"seq_len": L, "head": "embed", "pooling": pooling, "normalize": True})
    assert eng.embed == {"pooling": pooling, "normalize": True, "dim": 768}
    inputs = bert.encode_inputs(ids, None, am)
    out = eng.infer(inputs)
    assert out.shape == (B, 768) and out.dtype == torch.float32
    madd = inputs[2].reshape(B, L)
    ref = T.pool_embed_ref(h32.reshape(B * L, -1), B, L, madd, pooling, 0, True)
    yard = T.pool_embed_ref(h16.reshape(B * L, -1), B, L, madd, pooling, 0, True)
    for b in range(B):
        r = _rel(out[b], ref[b])
        d, d16 = float(1 - _cos(out[b:b + 1], ref[b:b + 1])), float(1 - _cos(yard[b:b + 1], ref[b:b + 1]))
        print(f"{model} {pooling} row {b}: rel {r:.3e}  1-cos {d:.3e}  (bf16 PyTorch {d16:.3e})")
        assert r < rel
        if model == "bert-base":
            assert d <= 4 * max(d16, 2e-5)


@pytest.mark.parametrize("pooling", ["cls", "mean"])
def test_vit_embedding_engine_matches_hf(pooling):
    from transformers import ViTConfig, ViTModel
    torch.manual_seed(0)
    m = _perturb_ln(ViTModel(ViTConfig(num_hidden_layers=2), add_pooling_layer=False).eval())
    B = 2
    x = torch.randn(B, 3, 224, 224)
    with torch.no_grad():
        h32 = m(pixel_values=x).last_hidden_state
        mb = ViTModel(m.config, add_pooling_layer=False).eval()
        mb.load_state_dict(m.state_dict())
        h16 = mb.to(torch.bfloat16)(pixel_values=x.to(torch.bfloat16)).last_hidden_state.float()
    Tn = h32.shape[1]
    eng = Engine.from_state_dict("vit-b16", m.state_dict(), DEV, batch=B,
                                 arch_kw={"head": "embed", "pooling": pooling, "normalize": True})
    out = eng.infer(x)
    assert out.shape == (B, 768)
    first = 1 if pooling == "mean" else 0
    ref = T.pool_embed_ref(h32.reshape(B * Tn, -1), B, Tn, None, pooling, first, True)
    yard = T.pool_embed_ref(h16.reshape(B * Tn, -1), B, Tn, None, pooling, first, True)
    for b in range(B):
        r = _rel(out[b], ref[b])
        d, d16 = float(1 - _cos(out[b:b + 1], ref[b:b + 1])), float(1 - _cos(yard[b:b + 1], ref[b:b + 1]))
        print(f"vit {pooling} row {b}: rel {r:.3e}  1-cos {d:.3e}  (bf16 PyTorch {d16:.3e})")
        assert r < 5e-2
        assert d <= 4 * max(d16, 2e-5)


# ---------------------------------------------------------------- the plan path
def test_embedding_plan_serves_the_engines_bits(bert2, tmp_path):
    """``.emb.hzplan`` at B=4, L=32 serving 2 sequences of length 20 (2 fully masked pad rows):
    bitwise the torch-built engine on the same padded inputs (both programs bind the same untuned
    default launch configs here, so no tolerance applies), eager and captured."""
    from hipzap.lite import PlanEngine
    from hipzap.serve.server import PlanTextBackend
    from hipzap.serve.settings import ModelSpec
    sd = bert2[0]
    ckpt = str(tmp_path / "bert2.pth")
    torch.save(sd, ckpt)
    path = P.export_from_checkpoint("bert-base", ckpt, batch=4, seq_len=32, embed={"pooling": "mean", "normalize": True})
    assert path == ckpt + ".emb.hzplan"
    B, Lc, n, L = 4, 32, 2, 20
    ids = np.random.default_rng(0).integers(0, 30000, (n, L))
    be = PlanTextBackend("bert-base", path, 0, ModelSpec(name="bert-base"))
    assert be.embed == {"pooling": "mean", "normalize": True, "dim": 768}
    eager = be.embed_np(ids)  # the first request of a lazily captured plan runs launch by launch
    be.engine.ensure_contexts()
    replay = be.embed_np(ids)
    assert eager.shape == (n, 768) and np.isfinite(eager).all()
    assert np.array_equal(eager.view(np.int32), replay.view(np.int32))
    with pytest.raises(ValueError, match="is an embedding plan: POST /embed"):
        be.infer_np(ids)
    # the torch-built engine on the same padded request
    ci, cm = torch.zeros(B, Lc, dtype=torch.long), torch.zeros(B, Lc, dtype=torch.long)
    ci[:n, :L], cm[:n, :L] = torch.from_numpy(ids), 1
    eng = Engine.from_state_dict("bert-base", sd, DEV, batch=B,
                                 arch_kw={"seq_len": Lc, "head": "embed", "pooling": "mean", "normalize": True})
    want = eng.infer(bert.encode_inputs(ci, None, cm))
    assert (want[n:] == 0).all()  # the fully masked pad rows
    assert np.array_equal(want[:n].numpy().view(np.int32), replay.view(np.int32))
    # PlanEngine alone: the raw output bytes are the [B, 768] vectors
    pe = PlanEngine(path, device=0)
    madd = ((1.0 - cm.float()) * -1e9).numpy().astype(np.float32)
    raw = np.frombuffer(pe.infer_raw([ci.numpy().astype(np.int32), np.zeros((B, Lc), np.int32), madd]), np.float32)
    assert np.array_equal(raw.reshape(B, 768).view(np.int32), want.numpy().view(np.int32))
    pe.close()


def test_classification_graph_is_unchanged():
    """The default engine and one built with an explicit head="cls" give the same logits, bitwise."""
    torch.manual_seed(0)
    sd = bert.make_model(2, num_hidden_layers=2).state_dict()
    B, L = 2, 24
    ids = torch.randint(0, 30000, (B, L))
    inputs = bert.encode_inputs(ids)
    a = Engine.from_state_dict("bert-base", sd, DEV, batch=B, arch_kw={"seq_len": L}).infer(inputs)
    b = Engine.from_state_dict("bert-base", sd, DEV, batch=B, arch_kw={"seq_len": L, "head": "cls"}).infer(inputs)
    assert a.shape == (B, 2) and torch.equal(a.view(torch.int32), b.view(torch.int32))
