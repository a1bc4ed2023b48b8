"""ResNet-50 at image sizes besides 224 on MI355X: the fusion planner binds the stem, the layer1 and
layer2 block kernels, the seams, the K-split 3x3 convs and the tail at 128, 160, 192 and 256 px
(tests/test_fusion_cpu.py plans them on the CPU); here those bindings run.

* 128: layer3 at 8 x 8 = 64 px (two seam tiles), layer4 at 4 x 4;
* 160 (batches 1 and 2): layer3 at 10 x 10 = 100 px (a partial seam tile), the 3x3 convs stay per
  conv (no K-split geometry), the tail at 5 x 5;
* 192: layer3 at 12 x 12 = 144 px, layer4 at 6 x 6 = 36 px;
* 256: layer1 at 64 x 64, the tail at exactly 8 x 8 = 64 px.

Each with the default fusion set and with ``fuse="all"``: the context binds exactly what
``fusion.plan`` plans; without arena reuse every tensor a fused launch writes matches the per-conv
program and the fp32 graph oracle (the whole-net thresholds of tests/test_fused_gpu.py and
tests/test_seam_gpu.py: 2e-2 and 3e-2 of the tensor's largest value), and so do the logits; with the
arena's default reuse the logits match again; a captured graph replayed over two images equals the
eager run."""
import pytest
import torch

from hipzap.engine import fusion
from hipzap.engine.program import ExecContext
from hipzap.engine.reference import run_graph_reference
from hipzap.models import registry
from hipzap.models.resnet import build_graph, randomize_bn
from hipzap.ops.conv import from_blocked

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(128, 1), (160, 1), (160, 2), (192, 1), (256, 1)]
# The request of each case. This random-weight network's two largest logits are nearly tied for every
# noise image (classes 440 and 697, mostly within 0.5 % of the largest logit), so "the same argmax as
# the per-conv program" holds only where the tie is clear of bf16-level differences between two correct
# programs. Each seed is one whose fp32 ORACLE keeps its top class at least MARGIN of the largest
# |logit| ahead in every row (found on the CPU from the oracle alone; asserted below).
SEEDS = {(128, 1): 27, (160, 1): 9, (160, 2): 24, (192, 1): 15, (256, 1): 1211}
MARGIN = 1e-2
FUSE = [None, "all"]  # None: the default set (engine/fusion.py DEFAULT)


@pytest.fixture(scope="module")
def r50():
    torch.manual_seed(0)
    a = registry.get("resnet50")
    sd = randomize_bn(a.make_model()).eval().state_dict()
    params, kw = a.pack({k: v.to(DEV) for k, v in sd.items()}, torch.device(DEV))
    params_cpu, _ = a.pack(sd, "cpu")
    return a, params, params_cpu, kw


@pytest.fixture(scope="module")
def baseline(r50):
    """(graph, request, fp32 graph oracle, the per-conv program after its run without arena reuse) per
    (image, batch): computed once, shared by the fusion sets, never modified."""
    _, params, params_cpu, _ = r50
    cache = {}

    def get(image, batch):
        if (image, batch) not in cache:
            g = build_graph("resnet50", batch, 1000, image, True)
            x = torch.randint(0, 256, (batch, image, image, 3), dtype=torch.uint8,
                              generator=torch.Generator().manual_seed(SEEDS[image, batch]))
            mp = pytest.MonkeyPatch()
            mp.setenv("HIPZAP_ARENA_NOREUSE", "1")
            try:
                plain = ExecContext(g, params, torch.device(DEV), fuse="none")
            finally:
                mp.undo()
            assert plain.fused == {}
            _run(plain, x)
            ref = run_graph_reference(g, params_cpu, [x])
            lr = ref[g.outputs[0]].reshape(batch, -1)
            top = lr.topk(2, dim=1).values
            assert ((top[:, 0] - top[:, 1]) >= MARGIN * lr.abs().max()).all(), (image, batch)
            cache[image, batch] = g, x, ref, plain
        return cache[image, batch]

    return get


def _run(ctx, x):
    ctx.input.copy_(x.to(ctx.input.device))
    ctx.run()
    torch.cuda.synchronize()


def _rel(a, b):
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-6)


def _kinds(fused):
    return sorted((i, f.kind) for i, f in fused.items())


def _f32(ctx, tid, shape):
    """A tensor the fused program keeps as fp32 in the bf16 tensor's arena slot (a seam's or a K-split
    conv's accumulator, engine/fusion.py planning_graph), as logical NHWC."""
    n = 1
    for d in shape:
        n *= d
    off = ctx.tensor_offsets[tid]
    return from_blocked(ctx.arena[off: off + 4 * n].view(torch.float32), shape).cpu()


def _bf16(ctx, tid):
    return from_blocked(ctx.view(tid).reshape(-1), ctx.graph.shape(tid)).float().cpu()


def _whole(t):
    return t


def _pooled(t):
    return t.mean(dim=(1, 2))


def _written(ctx):
    """(label, tensor id, value, view) of every tensor a fused launch writes: ``value`` is comparable
    with ``view`` of what the per-conv program and the oracle hold for that tensor id."""
    g = ctx.graph
    for f in ctx.fused.values():
        name = f.kind + ":" + "+".join(str(n.attrs.get("name", n.kind)) for n in f.nodes)
        if f.kind in ("stem", "convpool", "bneck", "bneck2"):
            tid = f.nodes[-1].outputs[0]
            yield name, tid, _bf16(ctx, tid), _whole
        elif f.kind == "seam":  # the block output y (bf16) and conv1's fp32 sum z (its ReLU at the reader)
            y, z = f.nodes[0].outputs[0], f.nodes[1].outputs[0]
            yield name + ":y", y, _bf16(ctx, y), _whole
            yield name + ":z", z, torch.relu(_f32(ctx, z, g.shape(z))), _whole
        elif f.kind == "kconv":  # the fp32 accumulator, its ReLU at the reader
            a = f.nodes[0].outputs[0]
            yield name, a, torch.relu(_f32(ctx, a, g.shape(a))), _whole
        elif f.kind == "tail":  # [N][2048] fp32 channel means where the block output would be
            tid = f.nodes[0].outputs[0]
            nb, _, _, c = g.shape(tid)
            yield name, tid, _f32(ctx, tid, (nb, 1, 1, c)).reshape(nb, c), _pooled
        else:
            assert f.kind == "skip", f.kind


def _logits(ctx, batch):
    return ctx.output.float().cpu().reshape(batch, -1)


@pytest.mark.parametrize("fuse", FUSE, ids=["default", "all"])
@pytest.mark.parametrize("image,batch", CASES)
def test_resnet50_at_other_sizes_matches_per_conv_and_oracle(r50, baseline, image, batch, fuse, monkeypatch):
    monkeypatch.delenv("HIPZAP_FUSE", raising=False)
    _, params, _, _ = r50
    g, x, ref, plain = baseline(image, batch)
    planned = fusion.plan(g, params, fusion.enabled_kinds(fuse))
    monkeypatch.setenv("HIPZAP_ARENA_NOREUSE", "1")
    ctx = ExecContext(g, params, torch.device(DEV), fuse=fuse)
    assert _kinds(ctx.fused) == _kinds(planned)
    kinds = [f.kind for f in ctx.fused.values()]
    assert kinds[0] in ("stem", "convpool") and kinds.count("bneck") == 3 and kinds.count("bneck2") == 4, kinds
    if fuse is None:  # the seams bind at every size; the K-split 3x3s where their geometry exists
        assert kinds.count("seam") >= 7 and kinds.count("tail") == 1, kinds
    _run(ctx, x)
    worst = {}
    for label, tid, got, view in _written(ctx):
        yp, yr = view(_bf16(plain, tid)), view(ref[tid].float())
        assert torch.isfinite(got).all(), label
        ep, er = _rel(got, yp), _rel(got, yr)
        k = label.split(":")[0]
        worst[k] = max(worst.get(k, (0.0, 0.0)), (ep, er))
        assert ep < 2e-2 and er < 3e-2, (label, ep, er)
    lf, lp, lr = _logits(ctx, batch), _logits(plain, batch), ref[g.outputs[0]].reshape(batch, -1)
    assert _rel(lf, lr) < 3e-2 and _rel(lf, lp) < 3e-2, (_rel(lf, lr), _rel(lf, lp))
    assert torch.equal(lf.argmax(1), lp.argmax(1))
    # once more with the arena's default reuse plan
    monkeypatch.delenv("HIPZAP_ARENA_NOREUSE")
    reuse = ExecContext(g, params, torch.device(DEV), fuse=fuse)
    assert _kinds(reuse.fused) == _kinds(planned) and reuse.arena_bytes < ctx.arena_bytes
    _run(reuse, x)
    lu = _logits(reuse, batch)
    print(f"[sizes] {image} px batch {batch} fuse {fuse or 'default'}: " +
          ", ".join(f"{k} {v[0]:.1e}/{v[1]:.1e}" for k, v in worst.items()) +
          f"; logits {_rel(lf, lp):.1e}/{_rel(lf, lr):.1e}, with arena reuse {_rel(lu, lp):.1e}/{_rel(lu, lr):.1e}"
          " (vs per-conv / vs oracle)")
    assert _rel(lu, lp) < 3e-2 and _rel(lu, lr) < 3e-2, (_rel(lu, lp), _rel(lu, lr))
    assert torch.equal(lu.argmax(1), lp.argmax(1))


@pytest.mark.parametrize("fuse", FUSE, ids=["default", "all"])
def test_resnet50_at_160_graph_replay_equals_eager(r50, fuse, monkeypatch):
    monkeypatch.delenv("HIPZAP_FUSE", raising=False)
    monkeypatch.delenv("HIPZAP_ARENA_NOREUSE", raising=False)
    _, params, _, _ = r50
    g = build_graph("resnet50", 1, 1000, 160, True)
    eager = ExecContext(g, params, torch.device(DEV), fuse=fuse)
    ctx = ExecContext(g, params, torch.device(DEV), fuse=fuse)
    s = torch.cuda.Stream()
    ctx.capture(s)
    outs = []
    for seed in (9, 7):  # (oracle margins 1.8e-2 and 1.2e-2, as above)
        x = torch.randint(0, 256, (1, 160, 160, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
        _run(eager, x)
        with torch.cuda.stream(s):
            ctx.input.copy_(x.to(DEV))
            ctx.replay(s)
        torch.cuda.synchronize()
        le, lc = _logits(eager, 1), _logits(ctx, 1)
        assert torch.isfinite(lc).all() and _rel(lc, le) < 2e-2 and torch.equal(lc.argmax(1), le.argmax(1))
        outs.append(lc)
    assert not torch.equal(outs[0], outs[1])  # the replay served the second image
