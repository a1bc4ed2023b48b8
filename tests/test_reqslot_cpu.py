"""Device-resident request slots without a GPU: the fallback decision and the fusion matcher's choice
for both kinds of slot on recording contexts (engine/plan.py ``PlanRecorder``), and the streaming
copy helper (csrc/reqcopy.h) under host ASan + UBSan in a stand-alone program."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

from hipzap import _native as N
from hipzap.engine import fusion
from hipzap.engine import plan as P
from hipzap.engine.program import ExecContext
from hipzap.models import registry
from hipzap.models.resnet import randomize_bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", shutil.which("hipcc") or "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def r50():
    torch.manual_seed(0)
    a = registry.get("resnet50")
    sd = randomize_bn(a.make_model()).eval().state_dict()
    params, kw = a.pack(sd, "cpu")
    return a, params, dict(kw, input_uint8=True)


def _recorded(r50, zero_copy, **kw):
    a, params, arch = r50
    g = a.build_graph(batch=1, **dict(arch, **kw.pop("arch", {})))
    rec = P.PlanRecorder()
    ctx = ExecContext(g, params, torch.device("cpu"), None, host_io=True, zero_copy=zero_copy, lib=rec, **kw)
    return ctx, rec


def _kinds(ctx):
    return [f.kind for f in ctx.fused.values()]


@pytest.fixture
def fake_device_slots(monkeypatch):
    """Stands in for hz_reqslot_alloc on a host-writable device: heap blocks reported as device slots."""
    made = []

    def alloc(nbytes):
        buf = (C.c_uint8 * ((nbytes + 15) // 16 * 16))()
        made.append(buf)
        return C.addressof(buf), C.addressof(buf), N.REQSLOT_DEVICE

    monkeypatch.setattr(N, "reqslot_alloc", alloc)
    monkeypatch.setattr(N, "reqslot_free", lambda dev, kind: None)
    return made


def test_probe_says_no_gives_pinned_slot_and_convpool(r50, monkeypatch):
    """No host-writable device memory: the allocator hands back a pinned buffer and says so; the
    context keeps today's request path -- preprocess + convpool, 29 launches."""
    freed = []
    pinned = (C.c_uint8 * 150528)()
    monkeypatch.setattr(N, "reqslot_alloc", lambda n: (C.addressof(pinned), C.addressof(pinned), N.REQSLOT_PINNED))
    monkeypatch.setattr(N, "reqslot_free", lambda dev, kind: freed.append((dev, kind)))
    ctx, rec = _recorded(r50, "dev")
    assert ctx.input_kind == N.REQSLOT_PINNED and ctx._req_slots is None
    assert freed == [(C.addressof(pinned), N.REQSLOT_PINNED)]  # the context pins its own, as under "all"
    assert _kinds(ctx)[0] == "convpool" and "stem" not in _kinds(ctx)
    assert len(rec.ops) == 29 and ctx.zc_in and ctx.zc_out
    base, rec0 = _recorded(r50, "all")
    assert _kinds(base) == _kinds(ctx) and len(rec0.ops) == 29
    # no allocator at all (no HIP device): the same fallback
    monkeypatch.setattr(N, "reqslot_alloc", lambda n: None)
    ctx2, rec2 = _recorded(r50, "dev")
    assert ctx2.input_kind == N.REQSLOT_PINNED and _kinds(ctx2) == _kinds(base) and len(rec2.ops) == 29


def test_device_slot_binds_the_one_launch_stem(r50, fake_device_slots):
    ctx, rec = _recorded(r50, "dev")
    assert ctx.input_kind == N.REQSLOT_DEVICE and len(fake_device_slots) == 1
    assert _kinds(ctx)[0] == "stem" and "convpool" not in _kinds(ctx)
    assert len(rec.ops) == 28
    # the stem launch reads the slot's DEVICE address in mode 1; the host view is the slot's host address
    t, kind, slot, structs = rec.ops[0]
    assert kind == N.HZ_K_STEM and structs[0].mode == 1
    assert structs[0].src == C.addressof(fake_device_slots[0]) == ctx.host_input.data_ptr()
    assert ctx.host_input.shape == (1, 224, 224, 3) and ctx.host_input.dtype == torch.uint8
    # a staged write lands in the slot (and nothing is read back from it)
    x = torch.randint(0, 256, (1, 224, 224, 3), dtype=torch.uint8)
    ctx.write_input(0, x)
    assert bytes(fake_device_slots[0])[:x.numel()] == x.numpy().tobytes()
    # every later launch is the pinned program's
    base, rec0 = _recorded(r50, "all")
    assert _kinds(ctx)[1:] == _kinds(base)[1:]
    assert [(o[0], o[1]) for o in rec.ops[1:]] == [(o[0], o[1]) for o in rec0.ops[2:]]


def test_unchanged_programs(r50, fake_device_slots, monkeypatch):
    """fp32-input engines keep preprocess + convpool on either slot; an explicit fusion list or
    HIPZAP_FUSE is obeyed; "all" never takes device slots while recording a plan image."""
    ctx, rec = _recorded(r50, "dev", arch={"input_uint8": False})
    assert ctx.input_kind == N.REQSLOT_DEVICE and _kinds(ctx)[0] == "convpool" and len(rec.ops) == 29
    ctx, rec = _recorded(r50, "dev", fuse="convpool,bneck")
    assert _kinds(ctx)[0] == "convpool"
    monkeypatch.setenv("HIPZAP_FUSE", fusion.DEFAULT)
    ctx, rec = _recorded(r50, "dev")
    assert _kinds(ctx)[0] == "convpool" and len(rec.ops) == 29
    monkeypatch.delenv("HIPZAP_FUSE")
    monkeypatch.setenv("HIPZAP_REQSLOT", "dev")
    n0 = len(fake_device_slots)
    ctx, rec = _recorded(r50, "all")
    assert ctx.input_kind == N.REQSLOT_PINNED and len(fake_device_slots) == n0 and len(rec.ops) == 29
    with pytest.raises(ValueError):
        P.export_plan("resnet50", r50[1], r50[2], os.devnull, zero_copy="dev")


def test_default_kinds():
    assert fusion.default_kinds(False) == fusion.enabled_kinds(fusion.DEFAULT)
    assert fusion.default_kinds(True) == fusion.enabled_kinds(fusion.DEFAULT) | {"stem"}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_reqcopy_host_asan_ubsan(tmp_path):
    """csrc/reqcopy.h against exact-size heap buffers: sizes 0, 1, 15, 16, 17 and 150,528 bytes,
    unaligned sources, aligned and unaligned destinations, with and without room to complete the last
    16-byte unit -- a stand-alone program, on the CPU."""
    exe = tmp_path / "reqcopy_asan"
    san = []  # host code only, as every sanitizer build here (tests/test_native_asan_cpu.py)
    for f in ("-fsanitize=address", "-fsanitize=undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=all"):
        san += ["-Xarch_host", f]
    cmd = [HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", *san, "-I", os.path.join(ROOT, "hipzap", "csrc"),
           os.path.join(ROOT, "tests", "native", "reqcopy_host_sanitize.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert run.returncode == 0 and "reqcopy host sanitize: ok" in run.stdout, (run.stdout[-2000:], run.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in run.stderr and "runtime error" not in run.stderr
