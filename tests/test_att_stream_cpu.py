"""Streamed attention (csrc/transformer.hip attention_stream_kernel) without a GPU: the public
sequence-length interface (plan export, CLI, the serving backend), and the kernel's CPU emulation
(ops/transformer.py attention_stream_ref) against the fp32 oracle on every input the GPU tests
run -- the emulation is what pins those inputs."""
import json

import pytest
import torch

import att_stream_inputs as I
from hipzap.ops import transformer as T


@pytest.fixture(scope="module")
def bert_ckpt(tmp_path_factory):
    """A 2-layer random BERT checkpoint with the standard 512-row position table."""
    from hipzap.models import bert
    torch.manual_seed(0)
    m = bert.make_model(num_labels=2, num_hidden_layers=2)
    d = tmp_path_factory.mktemp("bert2")
    ckpt = str(d / "bert2.pth")
    torch.save(m.state_dict(), ckpt)
    return ckpt


def _attention_lengths(plan):
    """L of every attention launch record of a plan (a fused QKV + attention record included)."""
    from hipzap import _native as N
    from hipzap.engine import plan as P
    from hipzap.lite import read_meta
    meta = read_meta(plan)
    kinds = {N.HZ_K_ATTENTION: T.AttentionParams, N.HZ_K_QKVATT: T.QkvAttParams}
    raw = open(plan, "rb").read()
    f = P.HEADER.unpack_from(raw, 0)
    n_ops, p, out = f[3], f[6], []
    for _ in range(n_ops):  # OpHeader, the parameter bytes padded to 8, the relocations
        t, arg, _slot, plen, nrel, _pad = P.OPHDR.unpack_from(raw, p)
        p += P.OPHDR.size
        if t == P.OP_KERNEL and arg in kinds:
            out.append(kinds[arg].from_buffer_copy(raw, p).L)
        p += (plen + 7) // 8 * 8 + nrel * P.RELOC.size
    assert p == f[6] + f[7]
    return meta, out


def test_plan_seq_len(bert_ckpt, tmp_path):
    from hipzap.engine.plan import export_from_checkpoint
    p512 = export_from_checkpoint("bert-base", bert_ckpt, str(tmp_path / "l512.hzplan"), batch=2, seq_len=512)
    meta, Ls = _attention_lengths(p512)
    assert meta["seq_len"] == 512 and meta["arch_kw"]["seq_len"] == 512
    assert Ls == [512, 512], Ls
    p128 = export_from_checkpoint("bert-base", bert_ckpt, str(tmp_path / "l128.hzplan"), batch=2)
    meta, Ls = _attention_lengths(p128)
    assert meta["seq_len"] == 128 and Ls == [128, 128], (meta["seq_len"], Ls)


def test_plan_seq_len_beyond_the_position_table(bert_ckpt, tmp_path):
    from hipzap.engine.plan import export_from_checkpoint
    with pytest.raises(ValueError, match="513"):
        export_from_checkpoint("bert-base", bert_ckpt, str(tmp_path / "l513.hzplan"), batch=2, seq_len=513)
    with pytest.raises(ValueError):  # a vision model has no sequence length
        from hipzap.models import registry
        sd = registry.get("resnet18").make_model().state_dict()
        torch.save(sd, str(tmp_path / "r18.pth"))
        export_from_checkpoint("resnet18", str(tmp_path / "r18.pth"), str(tmp_path / "r18.hzplan"), seq_len=64)


def test_cli_plan_seq_len(bert_ckpt, tmp_path, capsys, monkeypatch):
    import sys
    from hipzap import __main__ as cli
    from hipzap.lite import read_meta
    out = str(tmp_path / "cli.hzplan")
    monkeypatch.setattr(sys, "argv", ["hipzap", "plan", "--model", "bert-base", "--ckpt", bert_ckpt, "--out", out,
                                      "--batch", "2", "--seq-len", "384"])
    cli.main()
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["out"] == out
    assert read_meta(out)["seq_len"] == 384


def test_text_backend_configured_length(bert_ckpt):
    from hipzap.serve.server import TextBackend
    from hipzap.serve.settings import ModelSpec
    sd = torch.load(bert_ckpt, map_location="cpu", weights_only=True)
    be = TextBackend("bert-base", sd, "cpu", "cpu", ModelSpec(name="bert-base", extra={"seq_len": 384}), False)
    assert be.seq_len == 384
    assert TextBackend("bert-base", sd, "cpu", "cpu", ModelSpec(name="bert-base"), False).seq_len == 128


def test_adapter_keeps_a_requested_length():
    """meta_params (what a data-parallel receiver builds its layout from) keeps the source's length."""
    from hipzap.models import registry
    a = registry.get("bert-base")
    kw = dict(layers=1, hidden=64, heads=1, ffn=128, max_pos=512)
    assert a.meta_params(seq_len=512, **kw)[1]["seq_len"] == 512
    assert a.meta_params(**kw)[1]["seq_len"] == 128
    g = a.build_graph(batch=1, seq_len=512, layers=1, max_pos=512)
    assert [n.attrs["L"] for n in g.nodes if n.kind == "attention"] == [512]
    with pytest.raises(ValueError):
        a.build_graph(batch=1, seq_len=513, layers=1, max_pos=512)


# max-normalised error of the emulation against the fp32 oracle, as seen (the bound is the
# project's 2e-2 for a bf16 kernel; the emulation holds only the bf16 rounding of P, so it sits two
# orders of magnitude inside it and far below half the bound):
#   long cases 6.2e-4 .. 1.4e-3, short cases 8.7e-4 .. 1.7e-3 (L = 1: exactly 0, a single key has
#   p = 1), tile0-1e9 / tile0-inf 8.3e-4, spike_last / spike_first exactly 0 (the spike key's
#   p = 1 and every other p is below exp(-29): the output is the spike key's V row)
@pytest.mark.parametrize("case", I.cases(), ids=lambda c: c[0])
def test_emulation_matches_the_oracle(case):
    name, qkv, B, L, heads, mask = case
    out, raised, growth = T.attention_stream_ref(qkv, B, L, heads, mask, tile=I.TILE)
    ref = T.attention_ref(qkv, B, L, heads, mask)
    assert torch.isfinite(out).all()
    err = I.rel(out, ref)
    print(f"{name}: emulation vs fp32 oracle {err:.3e}")
    assert err < 2e-2, err
    assert raised.shape[-1] == (L + I.TILE - 1) // I.TILE
    if name != "tile0-inf":  # the first tile always sets the max, unless every key of it is -inf
        assert bool((raised[..., 0] == 1).all())


def test_spike_inputs_do_what_they_are_for():
    qkv = I.spike("spike_last")
    _, raised, growth = T.attention_stream_ref(qkv, 1, I.SPIKE_L, I.SPIKE_HEADS, None, tile=I.TILE)
    last = (I.SPIKE_L - 1) // I.TILE
    assert I.SPIKE_AT["spike_last"] // I.TILE == last
    assert bool((raised[..., last] == 1).all()) and growth[..., last].min().item() >= 20.0, growth[..., last].min()
    qkv = I.spike("spike_first")
    _, raised, _ = T.attention_stream_ref(qkv, 1, I.SPIKE_L, I.SPIKE_HEADS, None, tile=I.TILE)
    assert bool((raised[..., 0] == 1).all()) and int(raised[..., 1:].sum()) == 0


def test_emulation_whole_tile_of_minus_inf_is_finite():
    """The guard the kernel needs: with the first tile at -inf the running max is still -inf after
    it; the unguarded exp(-inf - -inf) would be NaN."""
    qkv, mask = I.random_qkv(2, 320, 2), I.tile_mask(float("-inf"))
    out, raised, _ = T.attention_stream_ref(qkv, 2, 320, 2, mask, tile=I.TILE)
    assert torch.isfinite(out).all()
    assert int(raised[1, :, :, 0].sum()) == 0 and bool((raised[1, :, :, 1] == 1).all())
