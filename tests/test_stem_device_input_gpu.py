"""Device-resident request slots (csrc/runtime.cpp hz_reqslot_alloc, csrc/reqcopy.h) on MI355X: the
request bytes are written by the CPU into host-writable device memory, and the one-launch stem
(``stem_kernel`` mode 1) reads them there.

* the stem reading a device slot is bitwise preprocess + convpool, at the smallest images where
  the row arithmetic can go wrong: 8 x 8 (the launcher's minimum, one partial tile), 32 x 40 (several
  tiles, the image edge inside a patch on every side), 30 x 36 and 34 x 44 (W * 3 not a multiple of
  16, rows starting at every dword phase, partial last tiles both ways), batches 1 and 2;
* a ResNet-50 engine at 224 on device slots is 28 launches and returns the bits of the same engine
  on pinned slots (29 launches);
* two different images back to back on one context each equal a fresh context's answer;
* the executor's three submit paths (whole, sized with a length that is no multiple of 16, rows of a
  dynamic batch) return on device slots what they return on pinned ones.
"""
import ctypes as C

import pytest
import torch
from conftest import logits_match

from hipzap import _native as N
from hipzap.engine import fusion
from hipzap.engine.engine import Engine
from hipzap.models import registry
from hipzap.models.resnet import randomize_bn
from hipzap.ops import vision

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def r50():
    torch.manual_seed(0)
    a = registry.get("resnet50")
    sd = randomize_bn(a.make_model()).eval().state_dict()
    params, kw = a.pack({k: v.to(DEV) for k, v in sd.items()}, torch.device(DEV))
    return a, params, dict(kw, input_uint8=True)


def _image(shape, seed):
    x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    x.view(-1)[0], x.view(-1)[1], x.view(-1)[-1] = 0, 255, 255
    return x


class _Slot:
    """A device-resident request slot holding ``x`` (written the way the executor writes it)."""

    def __init__(self, x):
        n = x.numel()
        s = N.reqslot_alloc(n)
        assert s is not None and s[2] == N.REQSLOT_DEVICE, f"no host-writable device memory here: {s}"
        self.dev, self.host, self.kind = s
        N.lib().hz_reqslot_write(self.host, x.data_ptr(), n, (n + 15) // 16 * 16)

    def free(self):
        N.reqslot_free(self.dev, self.kind)


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("hw", [(8, 8), (32, 40), (30, 36), (34, 44)])
def test_stem_on_device_slot_is_bitwise_preprocess_convpool(r50, hw, batch):
    a, params, kw = r50
    g = a.build_graph(batch=1, **kw)
    pre, cv = g.nodes[0], g.nodes[1]
    assert pre.kind == "preprocess" and cv.kind == "conv"
    pc = params[cv.attrs["w"]]
    H, W = hw
    assert (H * W * 3) % 4 == 0
    SH, SW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    PH, PW = (SH + 2 - 3) // 2 + 1, (SW + 2 - 3) // 2 + 1
    x = _image((batch, H, W, 3), 100 * H + batch)
    mean = torch.tensor(pre.attrs["mean"], dtype=torch.float32, device=DEV)
    inv_std = 1.0 / torch.tensor(pre.attrs["std"], dtype=torch.float32, device=DEV)

    def stem(src, mode):
        out = torch.zeros(batch, 2, PH, PW, 32, dtype=torch.bfloat16, device=DEV)
        p = fusion.StemParams()
        p.src, p.w, p.bias, p.out = src, pc.wf.data_ptr(), pc.bias.data_ptr(), out.data_ptr()
        p.N, p.H, p.W, p.mode, p.SH, p.SW, p.PH, p.PW, p.norm = batch, H, W, mode, SH, SW, PH, PW, 1
        for c in range(3):
            p.mean[c], p.inv_std[c] = float(mean[c].item()), float(inv_std[c].item())
        fusion.launch("stem", p)
        torch.cuda.synchronize()
        return out

    # reference: the standalone preprocess kernel, then conv1 + max-pool from its bf16 NHWC8 image
    xd = x.to(DEV)
    img = torch.zeros(batch, H, W, 8, dtype=torch.bfloat16, device=DEV)
    args = vision.PreprocessArgs(xd.data_ptr(), img.data_ptr(), mean.data_ptr(), inv_std.data_ptr(), batch, 3, H, W,
                                 8, 1)
    N.check(N.lib().hz_launch_kernel(N.HZ_K_PREPROCESS, C.byref(args), N.stream_ptr()), "preprocess")
    want = stem(img.data_ptr(), 2)
    slot = _Slot(x)
    try:
        got = stem(slot.dev, 1)
    finally:
        slot.free()
    assert want.float().abs().sum().item() > 0
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


@pytest.fixture(scope="module")
def engines(r50):
    """(engine on device-resident slots, the same engine on pinned slots), one context each."""
    a, params, kw = r50
    dev = Engine("resnet50", params, DEV, batch=1, num_contexts=1, arch_kw=kw, host_io=True, zero_copy="dev")
    mp = pytest.MonkeyPatch()
    mp.setenv("HIPZAP_REQSLOT", "host")
    try:
        pin = Engine("resnet50", params, DEV, batch=1, num_contexts=1, arch_kw=kw, host_io=True, zero_copy="all")
    finally:
        mp.undo()
    return dev, pin


def test_engine_on_device_slots_matches_pinned_slots(engines):
    dev, pin = engines
    cd, cp = dev.contexts[0], pin.contexts[0]
    assert cd.input_kind == N.REQSLOT_DEVICE and cp.input_kind == N.REQSLOT_PINNED
    assert [f.kind for f in cd.fused.values()][0] == "stem" and [f.kind for f in cp.fused.values()][0] == "convpool"
    assert (cd.num_ops(), cp.num_ops()) == (28, 29)
    x = _image((1, 224, 224, 3), 5)
    yd, yp = dev.infer(x), pin.infer(x)
    assert torch.isfinite(yp).all() and logits_match(yd, yp)
    assert torch.equal(yd, yp)  # the arithmetic is unchanged


def test_context_reuse_serves_the_new_image(r50, engines):
    a, params, kw = r50
    dev, _ = engines
    x1, x2 = _image((1, 224, 224, 3), 11), _image((1, 224, 224, 3), 12)
    y1, y2 = dev.infer(x1).clone(), dev.infer(x2).clone()
    assert not torch.equal(y1, y2)
    for x, y in ((x1, y1), (x2, y2)):
        fresh = Engine("resnet50", params, DEV, batch=1, num_contexts=1, arch_kw=kw, host_io=True, zero_copy="dev")
        assert fresh.contexts[0].input_kind == N.REQSLOT_DEVICE
        assert torch.equal(fresh.infer(x), y)


def test_executor_sized_submit_on_device_slots(engines):
    """A sized request (a length that is no multiple of 16) replaces its own bytes only: the tail of the
    slot keeps the previous request's bytes, on either kind of slot."""
    dev, pin = engines
    x1, x2 = _image((1, 224, 224, 3), 21), _image((1, 224, 224, 3), 22)
    n = x2.numel() - 5 - 16 * 7
    outs = []
    for eng in (dev, pin):
        eng.infer(x1)
        out = torch.empty_like(eng.contexts[0].host_output)
        eng.executor().submit_sized([x2.data_ptr()], [n], out.data_ptr())
        outs.append(out)
    mixed = torch.cat([x2.view(-1)[:n], x1.view(-1)[n:]]).reshape(x1.shape)
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(dev._post(outs[0]), pin.infer(mixed))


def test_executor_rows_on_device_slots(r50):
    a, params, kw = r50
    x = _image((3, 224, 224, 3), 31)
    outs = []
    for zc in ("dev", "all"):
        mp = pytest.MonkeyPatch()
        mp.setenv("HIPZAP_REQSLOT", "host" if zc == "all" else "dev")
        try:
            eng = Engine("resnet50", params, DEV, batch=4, num_contexts=1, arch_kw=kw, host_io=True, zero_copy=zc)
        finally:
            mp.undo()
        assert eng.contexts[0].input_kind == (N.REQSLOT_DEVICE if zc == "dev" else N.REQSLOT_PINNED)
        ex = eng.batched_executor(max_wait_us=50.0)
        row_out = eng.contexts[0].host_output.numel() // 4
        out = torch.empty(3 * row_out, dtype=eng.contexts[0].host_output.dtype)
        ex.submit_rows([x.data_ptr()], 3, out.data_ptr())
        one, x1 = torch.empty(row_out, dtype=out.dtype), x[1].contiguous()
        ex.submit([x1.data_ptr()], one.data_ptr())
        assert torch.equal(one, out[row_out:2 * row_out])
        outs.append(out)
        ex.close()
    assert torch.isfinite(outs[0]).all() and torch.equal(outs[0], outs[1])
