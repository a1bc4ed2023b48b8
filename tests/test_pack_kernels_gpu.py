"""The packing kernels of csrc/pack.hip, one launch each, against the bit-exact oracles of
tests/vision_oracle.py: every byte of the fragment-major weights and every bias bit, guards intact, every
condition the launchers list refused with -1 before anything is written (MI355X only). The cases are the
oracle module's tables; tests/test_vision_oracle_cpu.py holds them to the host packers on the CPU."""
import numpy as np
import pytest
import torch

import vision_oracle as O
from hipzap import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64))


def _refused(rc, *outs):
    assert rc == -1, rc
    torch.cuda.synchronize()
    for o in outs:
        assert O.untouched(o), "a refused launch wrote to its output"


# ------------------------------------------------------------------------------------------------ pack_conv
def _pack_conv(w, bn, bias_in, wf, bias_out, cout, cin, r, s, cin_p, rows, ksteps, eps=1e-5):
    g, b, m, v = bn if bn is not None else (None, None, None, None)
    prm = N.PackConvParams(N.ptr(w), N.ptr(g), N.ptr(b), N.ptr(m), N.ptr(v), N.ptr(bias_in), N.ptr(wf), N.ptr(bias_out),
                           cout, cin, r, s, cin_p, rows, ksteps, 0, eps)
    return N.lib().hz_pack_conv_launch(prm, N.stream_ptr())


@pytest.mark.parametrize("name", list(O.PACK_CASES))
def test_pack_conv(name):
    cout, cin, r, s, cin_p, rows, ksteps, _, _ = O.PACK_CASES[name]
    w, bn, bias_in = O.pack_inputs(name)
    nwf = rows * ksteps * 32
    wf = O.new_out(1, nwf, device=DEV)
    bias_out = O.new_out(1, cout, dtype=torch.float32, device=DEV)
    dbn = None if bn is None else tuple(_dev(t) for t in bn)
    assert _pack_conv(_dev(w), dbn, _dev(bias_in), wf, bias_out, cout, cin, r, s, cin_p, rows, ksteps) == 0
    torch.cuda.synchronize()
    got_wf, lost_w = O.split_out(wf, 1, nwf)
    got_b, lost_b = O.split_out(bias_out, 1, cout)
    assert lost_w == 0 and lost_b == 0
    want_wf, want_b = O.pack_ref(name)
    O.check_bits(O.t_bits(got_wf).reshape(-1), _i64(want_wf).reshape(-1), f"{name}: wf")
    O.check_bits(O.t_bits(got_b).reshape(-1), _i64(want_b.view(np.uint32)), f"{name}: bias", width=32)


def test_pack_conv_refusals():
    w = torch.zeros(16 * 8 * 9, device=DEV)
    vec = torch.zeros(16, device=DEV)
    wf = O.new_out(1, 32 * 96, device=DEV)
    bias_out = O.new_out(1, 16, dtype=torch.float32, device=DEV)
    good = dict(w=w, bn=None, bias_in=None, wf=wf, bias_out=bias_out, cout=10, cin=5, r=3, s=3, cin_p=8, rows=16, ksteps=3)
    bad = [dict(w=None), dict(wf=None), dict(bias_out=None), dict(cout=0), dict(cin=0), dict(r=0), dict(s=0), dict(cin_p=4),
           dict(rows=24), dict(rows=0), dict(cout=17), dict(ksteps=2),
           dict(bn=(vec, None, vec, vec)), dict(bn=(vec, vec, None, vec)), dict(bn=(vec, vec, vec, None))]
    for b in bad:
        _refused(_pack_conv(**{**good, **b}), wf, bias_out)
    assert _pack_conv(**good) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ frag_pack
def _frag(c, a, b, ba, bb, out, bias_out):
    prm = N.FragPackParams(N.ptr(a), N.ptr(b), N.ptr(out), N.ptr(ba), N.ptr(bb), N.ptr(bias_out), c["R"], c["K"],
                           c["nrows"], c["ih"], c["ka"], c["acols"], c["lda"], c["bcols"], c["ldb"], 0)
    return N.lib().hz_frag_pack_launch(prm, N.stream_ptr())


@pytest.mark.parametrize("name", list(O.FRAG_CASES))
def test_frag_pack(name):
    c = O.FRAG_CASES[name]
    a, b, ba, bb = O.frag_inputs(name)
    R, K = c["R"], c["K"]
    out = O.new_out(1, R * K, device=DEV)
    bias_out = O.new_out(1, R, dtype=torch.float32, device=DEV)
    assert _frag(c, _dev(a), _dev(b), _dev(ba), _dev(bb), out if c["out"] else None, bias_out if c["bias_out"] else None) == 0
    torch.cuda.synchronize()
    want_out, want_bias = O.frag_pack_ref(name)
    if c["out"]:
        got, lost = O.split_out(out, 1, R * K)
        assert lost == 0
        O.check_bits(O.t_bits(got).reshape(-1), _i64(want_out).reshape(-1), f"{name}: out")
    else:
        assert O.untouched(out)
    if c["bias_out"]:
        got, lost = O.split_out(bias_out, 1, R)
        assert lost == 0
        O.check_bits(O.t_bits(got).reshape(-1), _i64(want_bias.view(np.uint32)), f"{name}: bias", width=32)
    else:
        assert O.untouched(bias_out)


def test_frag_pack_refusals():
    a = torch.zeros(32 * 64, device=DEV)
    vec = torch.zeros(32, device=DEV)
    out = O.new_out(1, 32 * 64, device=DEV)
    bias_out = O.new_out(1, 32, dtype=torch.float32, device=DEV)
    good = O._fp(32, 64, nrows=30, ka=40, acols=33, lda=37, b=True, bcols=20, ldb=29)
    bad = [dict(R=24), dict(K=48), dict(R=0), dict(R=-16), dict(K=0), dict(K=-32), dict(ka=-1), dict(ka=96), dict(nrows=-1),
           dict(ih=-1), dict(acols=-1), dict(acols=41), dict(lda=32), dict(bcols=-1), dict(bcols=25), dict(ldb=19)]
    for d in bad:
        _refused(_frag({**good, **d}, a, a, vec, vec, out, bias_out), out, bias_out)
    _refused(_frag(good, a, a, vec, vec, None, None), out, bias_out)
    assert _frag(good, a, a, vec, vec, out, bias_out) == 0
    torch.cuda.synchronize()
