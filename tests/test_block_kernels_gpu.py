"""The fused ResNet kernels of csrc/block.hip, each alone on MI355X against the fp64 oracle of the same
op (tests/block_oracle.py), element by element under the derived bound
``|got - ref| <= 2**-7 |ref| + 2**-7 A``:

* ``bneck_kernel`` (layer1: Cin 64 with the downsample, Cin 256 identity; 8- and 4-row tiles),
* ``bneck2_kernel`` (layer2 identity blocks) and ``bneck2d_kernel`` (layer2's first block, stride 2 with
  the downsample), one and two images per workgroup, the two bitwise equal,
* ``stem_kernel`` modes 0 and 2 (mode 1 is tied bitwise to mode 2 by
  tests/test_stem_device_input_gpu.py),

at the smallest shapes where tiling can go wrong: one tile whose whole halo is outside the image,
interior tile borders in both directions, several images, partial stem tiles and odd stem maps.
Outputs are pre-filled with NaN, so an element no workgroup wrote fails. The inputs and references
are those tests/test_block_oracle_cpu.py judges on the CPU."""
import pytest
import torch

import block_oracle as B
from hipzap.engine import fusion
from hipzap.ops import conv as CV

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def dev_weights():
    """Packed weights of every block kind on the device, uploaded once."""
    cache = {}

    def get(kind):
        if kind not in cache:
            cache[kind] = [None if p is None else p.to(DEV) for p in B.bneck_weights(kind)]
        return cache[kind]

    return get


def _run_bneck(kind, n, h, w, dev_weights, tile_h=0, imgs=0):
    """Launch the block kernel of ``kind`` for an ``h x w`` output; -> the raw blocked bf16 output."""
    cin, cm, co, ds, stride, _ = B.KINDS[kind]
    x = B.bneck_input(kind, n, h, w)
    p1, p2, p3, pd = dev_weights(kind)
    xd = CV.to_blocked(x).to(DEV)
    out = torch.full((n, co // 32, h, w, 32), float("nan"), dtype=torch.bfloat16, device=DEV)
    p = fusion.BneckParams()
    p.x, p.out = xd.data_ptr(), out.data_ptr()
    p.w1, p.b1, p.w2, p.b2 = p1.wf.data_ptr(), p1.bias.data_ptr(), p2.wf.data_ptr(), p2.bias.data_ptr()
    p.w3, p.b3 = p3.wf.data_ptr(), p3.bias.data_ptr()
    if pd is not None:
        p.wd, p.bd = pd.wf.data_ptr(), pd.bias.data_ptr()
    # layer2 kernels take the block's OUTPUT size, layer1 (stride 1) the input's: the same here
    p.N, p.H, p.W, p.Cin, p.Cmid, p.Cout, p.tile_h, p.imgs = n, h, w, cin, cm, co, tile_h, imgs
    fusion.launch("bneck", p)
    torch.cuda.synchronize()
    return out.cpu()


def _judge(kind, n, h, w, out, label, tile=None):
    _, _, ref = B.bneck_case(kind, n, h, w)
    got = CV.from_blocked(out, tuple(ref.y.shape)).float()
    return B.check(got, ref.y, ref.A, tile or B.KINDS[kind][5], label)


@pytest.mark.parametrize("tile_h", B.BNECK_TILE_H)
@pytest.mark.parametrize("shape", B.BNECK_SHAPES)
@pytest.mark.parametrize("kind", ["l1ds", "l1id"])
def test_bneck_kernel_vs_fp64(dev_weights, kind, shape, tile_h):
    out = _run_bneck(kind, *shape, dev_weights, tile_h=tile_h)
    _judge(kind, *shape, out, f"bneck {kind} {shape} tile_h {tile_h}", tile=(tile_h, 8))


def test_bneck_kernel_default_tile_is_8_rows(dev_weights):
    """HzBneckParams.tile_h = 0 picks 8-row tiles: bitwise the tile_h = 8 launch."""
    a = _run_bneck("l1id", 1, 16, 24, dev_weights, tile_h=0)
    b = _run_bneck("l1id", 1, 16, 24, dev_weights, tile_h=8)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def _layer2(kind, n, h, w, imgs, dev_weights):
    out = _run_bneck(kind, n, h, w, dev_weights, imgs=imgs)
    _judge(kind, n, h, w, out, f"{'bneck2' if kind == 'l2id' else 'bneck2d'} {(n, h, w)} imgs {imgs}")
    if imgs == 2:  # per image the arithmetic and its order are the one-image kernel's (block.hip 563-566)
        one = _run_bneck(kind, n, h, w, dev_weights, imgs=1)
        assert not one.float().isnan().any()
        assert torch.equal(out.view(torch.int16), one.view(torch.int16))


@pytest.mark.parametrize("n,h,w,imgs", B.BNECK2_CASES)
def test_bneck2_kernel_vs_fp64(dev_weights, n, h, w, imgs):
    _layer2("l2id", n, h, w, imgs, dev_weights)


@pytest.mark.parametrize("n,h,w,imgs", B.BNECK2D_CASES)
def test_bneck2d_kernel_vs_fp64(dev_weights, n, h, w, imgs):
    _layer2("l2ds", n, h, w, imgs, dev_weights)


@pytest.mark.parametrize("mode", B.STEM_MODES)
@pytest.mark.parametrize("n", B.STEM_BATCHES)
@pytest.mark.parametrize("hw", B.STEM_SIZES)
def test_stem_kernel_vs_fp64(hw, n, mode):
    H, W = hw
    img, ref = B.stem_case(mode, n, H, W)
    pc = B.stem_weights().to(DEV)
    SH, SW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    PH, PW = (SH + 2 - 3) // 2 + 1, (SW + 2 - 3) // 2 + 1
    assert tuple(ref.y.shape) == (n, PH, PW, 64)
    # mode 0 normalises the fp32 NCHW image itself; mode 2 reads the preprocessed bf16 NHWC8 image
    src = (img if mode == 0 else ref.image).contiguous().to(DEV)
    out = torch.full((n, 2, PH, PW, 32), float("nan"), dtype=torch.bfloat16, device=DEV)
    p = fusion.StemParams()
    p.src, p.w, p.bias, p.out = src.data_ptr(), pc.wf.data_ptr(), pc.bias.data_ptr(), out.data_ptr()
    p.N, p.H, p.W, p.mode, p.SH, p.SW, p.PH, p.PW, p.norm = n, H, W, mode, SH, SW, PH, PW, int(mode == 0)
    mean, inv_std = B.stem_norm()
    for c in range(3):
        p.mean[c], p.inv_std[c] = mean[c], inv_std[c]
    fusion.launch("stem", p)
    torch.cuda.synchronize()
    got = CV.from_blocked(out.cpu(), (n, PH, PW, 64)).float()
    B.check(got, ref.y, ref.A, B.STEM_TILE, f"stem mode {mode} n {n} {hw}")
