"""Launches one case of tests/gemm_oracle.py on the GPU through ``make_params`` and the launchers themselves
(``hz_conv_launch``, ``hz_conv2_launch``, ``hz_gemm_lds_launch``), into NaN-filled outputs with guards, and
judges the result. Shared by tests/test_conv_kernels_gpu.py and tests/test_gemm_kernels_gpu.py. Not a test
module. Run as a program (``python tests/gemm_launch.py <set>``) it prints digests of the raw outputs of a
set of cases: what the child processes of the debug-library and HIPZAP_GEMM_GROUP tests return."""
import ctypes
import hashlib
import json
import sys

import torch

import gemm_oracle as G
from hipzap import _native as N
from hipzap.ops import conv as CV

DEV = "cuda:0"
WORST = {}  # family -> (ratio, label): the worst error / bound seen by judge()
_dev_cache = {}


def lds_launcher():
    fn = N.lib().hz_gemm_lds_launch
    fn.argtypes = [ctypes.POINTER(N.ConvParams), ctypes.c_int, ctypes.c_void_p]
    fn.restype = ctypes.c_int
    return fn


def device_case(case, kind):
    """(pc, x, res) of a case on the device, uploaded once (a small cache)."""
    key = (case, kind)
    if key not in _dev_cache:
        if len(_dev_cache) > 256:
            _dev_cache.clear()
        x, res = G.case_inputs(case, kind)
        rb = G.res_buffer(case, res)
        _dev_cache[key] = (G.case_weights(case, kind).to(DEV), G.x_buffer(case, x).to(DEV),
                           None if rb is None else rb.to(DEV))
    return _dev_cache[key]


def params(case, kind, cfg, kw, out):
    """-> (HzConvParams, what must stay alive)."""
    pc, x, res = device_case(case, kind)
    rowmajor, ld, _, _ = G.out_layout(case)
    prm, P, Q = CV.make_params(x.data_ptr(), pc, case.n, case.h, case.w, out.data_ptr(), N.ptr(res), case.act,
                               case.out_f32, cfg, kw, out_rowmajor=rowmajor, ldo=ld, x_rowmajor=case.xrow,
                               ldx=case.cin + case.ldx_pad)
    assert (P, Q) == case.PQ and prm.M == case.M and prm.K == case.K
    prm.x_f32 = int(case.x_f32)
    if not case.bias:
        prm.bias = 0
    return prm, (pc, x, res)


def run(case, kind, cfg, kw=1, direct_lds=False, tweak=None):
    """One launch -> the raw output buffer on the CPU (guards included)."""
    out = G.new_out(case, DEV)
    prm, keep = params(case, kind, cfg, kw, out)
    if tweak:
        tweak(prm)
    if direct_lds:
        rc = lds_launcher()(prm, cfg, N.stream_ptr())
    else:
        rc = N.lib().hz_conv_launch(prm, cfg, N.stream_ptr())
    assert rc == 0, f"{case.name} cfg {cfg} kw {kw}: launcher returned {rc}"
    torch.cuda.synchronize()
    del keep
    return out.cpu()


def run2(a, b, kind, cfg, kw, tweak=None):
    """``hz_conv2_launch`` of two cases -> their raw outputs."""
    oa, ob = G.new_out(a, DEV), G.new_out(b, DEV)
    pa, ka = params(a, kind, cfg, kw, oa)
    pb, kb = params(b, kind, cfg, kw, ob)
    if tweak:
        tweak(pa, pb)
    rc = N.lib().hz_conv2_launch(pa, pb, cfg, N.stream_ptr())
    assert rc == 0, f"{a.name} + {b.name} cfg {cfg} kw {kw}: launcher returned {rc}"
    torch.cuda.synchronize()
    del ka, kb
    return oa.cpu(), ob.cpu()


def judge(case, kind, raw, label, family=None):
    """Guards intact; exact cases bitwise, random ones element by element under the bound."""
    got, lost = G.split_out(raw, case)
    assert lost == 0, f"{label}: {lost} guard elements written"
    ref = G.case_ref(case, kind)
    if kind == "exact":
        want = G.expected_exact(ref, case.out_f32)
        same = G.bits(got.contiguous()) == G.bits(want.to(got.dtype))
        if not bool(same.all()):
            i = int((~same).reshape(-1).nonzero()[0])
            m, c = divmod(i, case.cout)
            raise AssertionError(f"{label}: {int((~same).sum())} elements differ from the exact value, first at row {m} "
                                 f"column {c}: got {float(got[m, c])!r} want {float(want[m, c])!r}")
        return 0.0
    rep = G.compare(got.float(), ref, case.act, case.out_f32)
    fam = (family or case.inst) + (" fp32 out" if case.out_f32 else " bf16 out")
    if rep.ratio > WORST.get(fam, (-1.0, ""))[0]:
        WORST[fam] = (rep.ratio, label)
    assert rep.ok, f"{label}: {G.describe(rep)}"
    return rep.ratio


def kinds_of(case):
    return [k for k in G.KINDS if k == "rand" or G.exact_ok(case)]


def digest(raw):
    return hashlib.sha1(G.bits(raw).numpy().tobytes()).hexdigest()[:16]


DEBUG_RING_CFGS = [(0, 1), (0, 16), (2, 4), (4, 2), (6, 4), (8, 1)]


def launch_set(name):
    """-> [(key, case, kind, cfg, kw)] of a named set of launches."""
    out = []
    if name == "ring-exact":
        for case in G.RING_CASES:
            if G.exact_ok(case):
                out += [(case, "exact", cfg, kw) for cfg, kw in DEBUG_RING_CFGS]
    elif name in ("gemm-exact", "gemm-rand", "gemm-tail"):
        for cfg in CV.LDS_TILES:
            for case in G.gemm_cases(cfg):
                if name == "gemm-exact" and G.exact_ok(case):
                    out.append((case, "exact", cfg, 1))
                elif name == "gemm-rand" or (name == "gemm-tail" and case.n == 577):
                    out.append((case, "rand", cfg, 1))
    elif name == "cv-exact":
        for cfg in CV.LDS_CONV_CFGS:
            out += [(case, "exact", cfg, 1) for case in G.cv_cases(cfg) if G.exact_ok(case)]
    else:
        raise ValueError(name)
    return [(f"{c.name}/{k}/{cfg}/{kw}", c, k, cfg, kw) for c, k, cfg, kw in out]


def digests(names):
    return {key: digest(run(c, k, cfg, kw)) for name in names for key, c, k, cfg, kw in launch_set(name)}


if __name__ == "__main__":
    from hipzap.utils import kcheck
    res = {"debug": bool(N.DEBUG), "digests": digests(sys.argv[1:])}
    res["kcheck"] = kcheck.poll() if N.DEBUG else []
    print("RESULT " + json.dumps(res))
