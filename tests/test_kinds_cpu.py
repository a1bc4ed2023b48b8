"""The kernel table (csrc/hipzap.h HZ_KERNELS) against its Python side: the kind numbers and the
ctypes mirrors of the parameter structs (hipzap/_native.py KINDS / KIND_STRUCT), and the programs
the lowering builds from them (tests/golden/lowered_programs.json: the op sequences recorded before
the per-op ``hz_prog_add_*`` entry points were folded into the table)."""
import ctypes as C
import json
import os

import pytest
import torch

from hipzap import _native as N
from hipzap.engine import fusion, lmcore, plan as P  # noqa: F401  (importing registers their structs)
from hipzap.models import registry
from hipzap.models.resnet import randomize_bn
from hipzap.ops import fp8, transformer, vision  # noqa: F401

from test_plan_cpu import decode

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lowered_programs.json")


def test_python_mirrors_match_the_native_table():
    lib = N.lib()
    assert len(set(N.KINDS.values())) == len(N.KINDS)
    for name, kind in N.KINDS.items():
        assert lib.hz_kernel_name(kind) == name.encode()
        assert kind in N.KIND_STRUCT, f"no ctypes struct registered for {name}"
        assert C.sizeof(N.KIND_STRUCT[kind]) == lib.hz_kernel_param_size(kind), name
    named = {k for k in range(1, 65) if lib.hz_kernel_name(k) is not None}
    assert named == set(N.KINDS.values())  # a kind added on one side only shows up here
    assert lib.hz_kernel_name(17) is None and lib.hz_kernel_param_size(17) == 0  # retired, never reused


def _normalised(path):
    """[launcher, cfg, slot, parameter bytes with pointers zeroed, relocations] per op. A conv's
    bytes are its HzConvParams (two for a pair) and cfg its launch config, wherever the format keeps
    them; every other op's bytes are its whole record and cfg is -1."""
    names = {v: k for k, v in N.KINDS.items()}
    out = []
    for t, arg, slot, prm, rels in decode(path)[2]:
        prm, cfg = bytearray(prm), -1
        for off, _, _ in rels:
            prm[off: off + 8] = bytes(8)
        name = {P.OP_MEMCPY: "MEMCPY", P.OP_FORK: "FORK", P.OP_JOIN: "JOIN"}.get(t) or names[arg]
        if t == P.OP_KERNEL and arg in (N.HZ_K_CONV, N.HZ_K_CONV2):
            op = N.KIND_STRUCT[arg].from_buffer_copy(prm)
            assert len(prm) == C.sizeof(op) and op.pad_ == 0
            cfg, prm = op.cfg, prm[:type(op).cfg.offset]
        out.append([name, cfg, slot, bytes(prm).hex(), [list(r) for r in sorted(rels)]])
    return out


def _resnet18(path):
    torch.manual_seed(0)
    a = registry.get("resnet18")
    params, kw = a.pack(randomize_bn(a.make_model()).eval().state_dict(), "cpu")
    P.export_plan("resnet18", params, dict(kw, input_uint8=True), path, batch=1)


def _bert_2_layers(path):
    from hipzap.models.bert import make_model
    torch.manual_seed(0)
    a = registry.get("bert-base")
    params, kw = a.pack(make_model(2, num_hidden_layers=2).state_dict(), "cpu")
    P.export_plan("bert-base", params, dict(kw), path, batch=1)


@pytest.mark.parametrize("name,export", [("resnet18_b1", _resnet18), ("bert_l2_b1", _bert_2_layers)])
def test_lowered_program_is_unchanged(tmp_path, name, export):
    """Same launchers in the same order with the same parameter bytes, cfg, slot and relocations as
    the golden sequence."""
    path = str(tmp_path / "m.hzplan")
    export(path)
    got, want = _normalised(path), json.load(open(GOLDEN))[name]
    assert [o[0] for o in got] == [o[0] for o in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"op {i} ({w[0]})"
