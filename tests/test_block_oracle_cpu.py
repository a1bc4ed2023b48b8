"""tests/block_oracle.py on the CPU: the oracle of the fused ResNet kernels agrees with the project's
graph oracle, its own fp32 and fp64 evaluations agree within a quarter of the comparator's bound on
the exact inputs of tests/test_block_kernels_gpu.py, and the comparator rejects every planted fault
(each printed beside the verdict of the old whole-tensor metric, max |err| / max |ref| < 2e-2).
Every element is judged: no share of them may fail."""
import pytest
import torch
import torch.nn.functional as F

import block_oracle as B
from hipzap.engine.reference import run_graph_reference
from hipzap.models import registry
from hipzap.models.resnet import build_graph, randomize_bn


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


# ------------------------------------------------------------------------------------------------
# the oracle against the graph oracle (engine/reference.py) on slices of a ResNet-50 graph at 32 px:
# layer1 runs at 8 x 8 and layer2 at 4 x 4, the smallest shapes of the GPU cases
@pytest.fixture(scope="module")
def r50_at_32():
    torch.manual_seed(0)
    a = registry.get("resnet50")
    params, _ = a.pack(randomize_bn(a.make_model()).eval().state_dict(), "cpu")
    g = build_graph("resnet50", 1, 1000, 32, True)
    x = torch.randint(0, 256, (1, 32, 32, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    return g, params, run_graph_reference(g, params, [x])


@pytest.mark.parametrize("block,kind", [("layer1.0", "l1ds"), ("layer1.1", "l1id"), ("layer2.1", "l2id"),
                                        ("layer2.0", "l2ds")])
def test_oracle_agrees_with_the_graph_oracle(r50_at_32, block, kind):
    g, params, vals = r50_at_32
    cin, cm, co, ds, stride, tile = B.KINDS[kind]
    c1, c3 = (next(n for n in g.nodes if n.attrs.get("name") == f"{block}.conv{i}") for i in (1, 3))
    x = vals[c1.inputs[0]]
    hw = 8 if block.startswith("layer1") else 4  # the smallest shapes of the GPU cases
    assert x.shape == (1, stride * hw, stride * hw, cin) and g.shape(c3.outputs[0]) == (1, hw, hw, co)
    assert torch.equal(x, _bf16(x))
    ps = [params[f"{block}.{c}"] for c in ("conv1", "conv2", "conv3")]
    pd = params[f"{block}.downsample"] if ds else None
    assert (ps[1].stride, pd is not None and pd.stride) == (stride, ds and stride)
    # the graph oracle stores the downsample as bf16 (the per-conv program does); the fused kernels do
    # not: the one documented difference, so the comparison rounds r in a copy of the oracle
    ref = B.bneck_ref(x, *ps, pd, stride=stride, hooks={"r": _bf16} if ds else None)
    rep = B.check(vals[c3.outputs[0]].float(), ref.y, ref.A, tile, f"graph oracle vs bneck_ref, {block}")
    assert rep.ratio < 0.5  # the stored bf16 rounding of y alone: half an ulp of |y|, under half the bound
    if ds:  # and the unrounded residual is a different (closer) value, still inside the bound
        exact = B.bneck_ref(x, *ps, pd, stride=stride)
        assert not torch.equal(exact.y, ref.y)
        B.check(ref.y, exact.y, exact.A, tile, f"rounded vs unrounded downsample, {block}")


def test_stem_oracle_agrees_with_the_graph_oracle(r50_at_32):
    g, params, vals = r50_at_32
    pre, cv, mp = g.nodes[:3]
    assert (pre.kind, cv.kind, mp.kind) == ("preprocess", "conv", "maxpool")
    img = vals[g.inputs[0]]
    mean, inv_std = B.stem_norm()
    ref = B.stem_ref(img, params["conv1"], mean, inv_std, 2)
    # the graph oracle divides by std where the kernels multiply by 1 / std: an ulp of fp32 before the
    # bf16 rounding, so a few image values may sit one bf16 ulp apart (inside the bound: an operand ulp)
    gi = vals[pre.outputs[0]].float()
    assert ((gi - ref.image.float()).abs() <= 2.0 ** -7 * gi.abs()).all()
    B.check(vals[mp.outputs[0]].float(), ref.y, ref.A, B.STEM_TILE, "graph oracle vs stem_ref")


# ------------------------------------------------------------------------------------------------
# the reference alone: fp32 against fp64 on the GPU cases' inputs
def _bneck_cases():
    out = [(k, s) for k in ("l1ds", "l1id") for s in B.BNECK_SHAPES]
    out += [("l2id", s) for s in sorted({c[:3] for c in B.BNECK2_CASES})]
    return out + [("l2ds", s) for s in sorted({c[:3] for c in B.BNECK2D_CASES})]


@pytest.mark.parametrize("kind,shape", _bneck_cases())
def test_bneck_ref_fp32_within_a_quarter_of_the_bound_of_fp64(kind, shape):
    x, ws, r64 = B.bneck_case(kind, *shape)
    r32 = B.bneck_ref(x, *ws, stride=B.KINDS[kind][4], dtype=torch.float32)
    assert r64.y.dtype == torch.float64 and r32.y.dtype == torch.float32
    rep = B.check(r32.y, r64.y, r64.A, B.KINDS[kind][5], f"fp32 vs fp64 {kind} {shape}")
    print(f"[block_oracle] fp32-vs-fp64 {kind} {shape}: ratio {rep.ratio:.3e}")
    assert rep.ratio <= 0.25


@pytest.mark.parametrize("mode", B.STEM_MODES)
@pytest.mark.parametrize("n", B.STEM_BATCHES)
@pytest.mark.parametrize("hw", B.STEM_SIZES)
def test_stem_ref_fp32_within_a_quarter_of_the_bound_of_fp64(hw, n, mode):
    img, r64 = B.stem_case(mode, n, *hw)
    mean, inv_std = B.stem_norm()
    r32 = B.stem_ref(img, B.stem_weights(), mean, inv_std, mode)
    assert torch.equal(r32.image, r64.image)  # the normalisation does not depend on dtype
    rep = B.check(r32.y, r64.y, r64.A, B.STEM_TILE, f"fp32 vs fp64 stem mode {mode} n {n} {hw}")
    print(f"[block_oracle] fp32-vs-fp64 stem mode {mode} n {n} {hw}: ratio {rep.ratio:.3e}")
    assert rep.ratio <= 0.25


# ------------------------------------------------------------------------------------------------
# planted faults: each an edit of the oracle's own computation, each rejected by the comparator
def _verdict(name, got, ref, tile):
    rep = B.compare(got, ref.y, ref.A, tile)
    old = B.old_metric(got, ref.y)
    print(f"[block_oracle] fault {name}: new comparator {'REJECTS' if not rep.ok else 'accepts'} "
          f"({rep.bad} elements outside, {B.describe(rep)}); old metric {old:.3e} "
          f"{'rejects' if old >= 2e-2 else 'ACCEPTS'}")
    assert not rep.ok, name
    with pytest.raises(AssertionError):
        B.check(got, ref.y, ref.A, tile, name)
    return rep


def _faulty(kind, shape, hooks):
    x, ws, ref = B.bneck_case(kind, *shape)
    return ref, B.bneck_ref(x, *ws, stride=B.KINDS[kind][4], dtype=torch.float64, hooks=hooks).y


@pytest.mark.parametrize("kind,shape", [("l1ds", (1, 8, 8)), ("l1id", (1, 16, 24)), ("l2id", (1, 4, 4)),
                                        ("l2ds", (1, 4, 4))])
def test_fault_halo_outside_the_image_is_relu_b1(kind, shape):
    b1 = B.bneck_weights(kind)[0].bias.double()

    def halo(t1p):  # the padding ring holds bf16(relu(b1)), what conv1 gives a zero input pixel
        v = _bf16(torch.relu(b1)).view(1, -1, 1, 1).expand_as(t1p)
        out = v.clone()
        out[:, :, 1:-1, 1:-1] = t1p[:, :, 1:-1, 1:-1]
        return out

    ref, got = _faulty(kind, shape, {"t1_padded": halo})
    rep = _verdict(f"halo=relu(b1) {kind} {shape}", got, ref, B.KINDS[kind][5])
    th, tw = B.KINDS[kind][5]
    y, x = rep.tile[0] * th + rep.pixel[0], rep.tile[1] * tw + rep.pixel[1]
    assert y in (0, ref.y.shape[1] - 1) or x in (0, ref.y.shape[2] - 1)  # the worst element is on the image border


@pytest.mark.parametrize("kind,shape,col", [("l1ds", (1, 16, 24), 7), ("l1id", (1, 16, 24), 15), ("l2id", (1, 8, 12), 3)])
def test_fault_tile_border_column_of_t1_seen_as_zero(kind, shape, col):
    """The tile right of column ``col`` (its left halo column) reads zeros there, over one tile's rows."""
    th, tw = B.KINDS[kind][5]
    assert (col + 1) % tw == 0

    def zero_col(t1p):
        out = t1p.clone()
        out[:, :, 1:1 + th + 1, col + 1] = 0  # padded coordinates: rows 0 .. th of the image (tile row 0's halo)
        return out

    ref, zeroed = _faulty(kind, shape, {"t1_padded": zero_col})
    got = ref.y.clone()
    got[:, :th, col + 1:col + 1 + tw] = zeroed[:, :th, col + 1:col + 1 + tw]  # only the neighbouring tile sees it
    assert int((got != ref.y).any(-1).sum()) <= th  # one column of one tile
    rep = _verdict(f"t1 border column {col} zero {kind} {shape}", got, ref, (th, tw))
    assert rep.tile == (0, (col + 1) // tw) and rep.pixel[1] == 0


@pytest.mark.parametrize("kind,shape", [("l1id", (1, 8, 8)), ("l2id", (2, 4, 8)), ("l2ds", (1, 8, 12))])
def test_fault_two_8_channel_chunks_of_t2_swapped(kind, shape):
    def swap(t2):
        out = t2.clone()
        out[-1, 2, 3, 8:16], out[-1, 2, 3, 40:48] = t2[-1, 2, 3, 40:48], t2[-1, 2, 3, 8:16]
        return out

    ref, got = _faulty(kind, shape, {"t2": swap})
    assert int((got != ref.y).any(-1).sum()) == 1
    rep = _verdict(f"t2 chunks swapped {kind} {shape}", got, ref, B.KINDS[kind][5])
    th, tw = B.KINDS[kind][5]
    assert (rep.n, rep.tile[0] * th + rep.pixel[0], rep.tile[1] * tw + rep.pixel[1]) == (shape[0] - 1, 2, 3)


@pytest.mark.parametrize("kind,shape", [("l1id", (2, 8, 16)), ("l1ds", (1, 8, 8)), ("l2id", (1, 4, 4)),
                                        ("l2ds", (2, 4, 4))])
def test_fault_residual_dropped_at_one_pixel(kind, shape):
    def drop(r):
        out = r.clone()
        out[0, 1, 2] = 0
        return out

    ref, got = _faulty(kind, shape, {"r": drop})
    rep = _verdict(f"residual dropped at one pixel {kind} {shape}", got, ref, B.KINDS[kind][5])
    th, tw = B.KINDS[kind][5]
    assert (rep.n, rep.tile[0] * th + rep.pixel[0], rep.tile[1] * tw + rep.pixel[1]) == (0, 1, 2)


@pytest.mark.parametrize("shape", [(1, 4, 4), (2, 8, 4)])
def test_fault_downsample_read_at_odd_pixels(shape):
    ref, got = _faulty("l2ds", shape, {"xd": lambda x: x[:, 1::2, 1::2]})
    _verdict(f"downsample at (2y+1, 2x+1) l2ds {shape}", got, ref, (4, 4))


@pytest.mark.parametrize("mode,hw", [(2, (30, 36)), (0, (34, 44))])
def test_fault_stem_pool_window_shifted_at_the_far_edges(mode, hw):
    """Odd SH / SW: the last pooled row / column takes rows (2 py, 2 py + 2) in place of
    (2 py - 1, 2 py + 1), i.e. loses its first row of stem outputs."""
    img, ref = B.stem_case(mode, 1, *hw)
    SH, SW = ref.so.shape[1:3]
    assert SH % 2 == 1 or SW % 2 == 1

    def pool(so):
        good = F.max_pool2d(so, 3, 2, 1)
        shifted = F.max_pool2d(F.pad(so, (0, 2, 0, 2)), 3, 2, 0)[:, :, :good.shape[2], :good.shape[3]]
        out = good.clone()
        out[:, :, -1, :], out[:, :, :, -1] = shifted[:, :, -1, :], shifted[:, :, :, -1]
        return out

    mean, inv_std = B.stem_norm()
    got = B.stem_ref(img, B.stem_weights(), mean, inv_std, mode, dtype=torch.float64, hooks={"pool": pool}).y
    assert torch.equal(got[:, :-1, :-1], ref.y[:, :-1, :-1])
    _verdict(f"stem pool window shifted, mode {mode} {hw}", got, ref, B.STEM_TILE)


def test_comparator_rejects_nan_and_accepts_the_reference():
    _, _, ref = B.bneck_case("l1id", 1, 8, 8)
    assert B.compare(ref.y, ref.y, ref.A).ratio == 0.0
    assert B.check(_bf16(ref.y), ref.y, ref.A, label="bf16(ref)").ratio <= 0.5
    got = ref.y.clone()
    got[0, 5, 6, 77] = float("nan")
    rep = B.compare(got, ref.y, ref.A)
    assert not rep.ok and rep.bad == 1 and (rep.tile, rep.pixel, rep.channel) == ((0, 0), (5, 6), 77)
    got = ref.y.clone()
    got[0, 5, 6, 77] += 1.01 * float(B.bound(ref.y, ref.A)[0, 5, 6, 77])
    assert not B.compare(got, ref.y, ref.A).ok
