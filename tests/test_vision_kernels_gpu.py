"""The helper kernels of csrc/vision.hip, one launch each, against the fp64 oracles of tests/vision_oracle.py:
every element under its derived bound or equal bit for bit, every guard element intact, every refusal
answered with -1 before anything is written (MI355X only; the release library). The cases and their inputs
are the oracle module's tables, which tests/test_vision_oracle_cpu.py judges on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import vision_oracle as O
from hipzap import _native as N
from hipzap.ops import vision as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _sync():
    torch.cuda.synchronize()


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64))


def _refused(rc, *outs):
    assert rc == -1, rc
    _sync()
    for o in outs:
        assert O.untouched(o), "a refused launch wrote to its output"


# ------------------------------------------------------------------------------------------------ maxpool
def _maxpool(x, out, n, h, w, c, P, Q, k, s, p):
    prm = N.PoolParams(N.ptr(x), N.ptr(out), n, h, w, c, P, Q, k, s, p)
    return N.lib().hz_maxpool_launch(prm, N.stream_ptr())


@pytest.mark.parametrize("case", O.MAXPOOL_CASES, ids=str)
def test_maxpool(case):
    n, h, w, c, k, s, p = case
    P, Q = O.pool_out(h, w, k, s, p)
    for kind in O.MAXPOOL_KINDS:
        x = O.maxpool_input(case, kind)
        out = O.new_out(n * P * Q, c, device=DEV)
        assert _maxpool(x.to(DEV), out, n, h, w, c, P, Q, k, s, p) == 0
        _sync()
        got, lost = O.split_out(out, n * P * Q, c)
        assert lost == 0
        want = O.round_bf16(O.maxpool_ref(x, k, s, p)).reshape(-1, c)
        O.check_bits(O.t_bits(got), want, f"{case} {kind}", zero_sign=False)
    if case == O.MAXPOOL_CASES[0]:   # the wrapper computes the same P, Q
        assert torch.equal(O.t_bits(V.maxpool_nhwc(x.to(DEV), k, s, p).cpu()).reshape(-1, c), want)


def test_maxpool_refusals():
    n, h, w, c, k, s, p = 1, 6, 6, 8, 3, 2, 1
    P, Q = O.pool_out(h, w, k, s, p)
    x = torch.zeros(n, h, w, 16, dtype=torch.bfloat16, device=DEV)
    out = O.new_out(4 * n * P * Q, 16, device=DEV)
    good = dict(x=x, out=out, n=n, h=h, w=w, c=c, P=P, Q=Q, k=k, s=s, p=p)
    bad = [dict(c=12), dict(c=0), dict(k=0), dict(s=0), dict(p=-1), dict(p=3), dict(k=2, p=2), dict(n=0), dict(P=0),
           dict(Q=0), dict(P=P + 2), dict(Q=Q + 2), dict(x=None), dict(out=None)]
    for b in bad:
        _refused(_maxpool(**{**good, **b}), out)
    assert (P + 2 - 1) * s - p >= h   # P + 2: the last window lies wholly below the image
    assert _maxpool(**good) == 0
    _sync()


# ------------------------------------------------------------------------------------------------ avgpool
def _avgpool(x, out, n, hw, c, blocked):
    return N.lib().hz_avgpool_launch(N.ptr(x), N.ptr(out), n, hw, c, int(blocked), N.stream_ptr())


@pytest.mark.parametrize("blocked", [False, True], ids=["nhwc", "blocked"])
@pytest.mark.parametrize("case", O.AVGPOOL_CASES, ids=str)
def test_avgpool(case, blocked):
    n, hw, c = case
    for kind in O.KINDS:
        x = O.pool_input(n, hw, c, kind)
        src = (O.blocked(x) if blocked else x.contiguous()).to(DEV)
        out = O.new_out(n, c, device=DEV)
        assert _avgpool(src, out, n, hw, c, blocked) == 0
        _sync()
        got, lost = O.split_out(out, n, c)
        assert lost == 0
        ref = O.avgpool_ref(x)
        rep = O.compare(got, ref, False, O.avgpool_c(hw))
        print(f"avgpool {case} {kind} blocked={blocked}: {O.describe(rep)}")
        if kind == "exact" and O.is_pow2(hw):
            O.check_bits(O.t_bits(got), O.round_bf16(ref.y), f"{case} exact")
        assert rep.ok, O.describe(rep)


def test_avgpool_refusals():
    x = torch.zeros(2 * 4 * 128, dtype=torch.bfloat16, device=DEV)
    out = O.new_out(2, 128, device=DEV)
    for n, hw, c, xx, oo in [(2, 4, 32, x, out), (2, 4, 96, x, out), (0, 4, 64, x, out), (2, 0, 64, x, out),
                             (2, 4, 0, x, out), (2, 4, 64, None, out), (2, 4, 64, x, None)]:
        for blocked in (0, 1):
            _refused(_avgpool(xx, oo, n, hw, c, blocked), out)


# ------------------------------------------------------------------------------------------------ pool_fc
def _wf(w):
    """[N, C] bf16-valued fp32 -> the fragment-major weights on the device, rows padded to the 16-row group."""
    n, c = w.shape
    rows = (n + 15) // 16 * 16
    wf, _ = O.pack_conv_ref(w.numpy().reshape(n, c, 1, 1), cin_p=c, rows=rows, ksteps=c // 32)
    return O.bf16_tensor(wf).to(DEV)


def _poolfc(x, wf, bias, out, B, C, HW, Nn, ldo, pooled):
    prm = V.PoolFcParams(N.ptr(x), N.ptr(wf), N.ptr(bias), N.ptr(out), B, C, HW, Nn, ldo, int(pooled))
    return N.lib().hz_launch_kernel(V.K_POOL_FC, ctypes.byref(prm), N.stream_ptr())


@pytest.mark.parametrize("case", O.POOLFC_CASES, ids=O.poolfc_name)
def test_pool_fc(case):
    B, HW, C, Nn, ldo_pad, has_bias, pooled = case
    ldo = Nn + ldo_pad
    for kind in O.KINDS:
        x, w, b = O.poolfc_inputs(case, kind)
        src = (x if pooled else O.blocked(x)).contiguous().to(DEV)
        out = O.new_out(B, Nn, ldo, torch.float32, DEV)
        bias = b.to(DEV) if has_bias else None
        assert _poolfc(src, _wf(w), bias, out, B, C, HW, Nn, ldo, pooled) == 0
        _sync()
        got, lost = O.split_out(out, B, Nn, ldo)
        assert lost == 0
        for i in range(B):   # each image's row against that image alone
            ref = O.poolfc_ref(x[i:i + 1], w, b)
            rep = O.compare(got[i:i + 1], ref, True, O.poolfc_c(case))
            print(f"pool_fc {O.poolfc_name(case)} {kind} image {i}: {O.describe(rep)}")
            if kind == "exact" and O.poolfc_exact_ok(case):
                O.check_bits(O.t_bits(got[i:i + 1]), O.t_bits(ref.y.float()), "exact", width=32)
            assert rep.ok, O.describe(rep)


def test_pool_fc_refusals():
    B, HW, C, Nn = 2, 4, 64, 17
    x = torch.zeros(B * HW * 16448, dtype=torch.bfloat16, device=DEV)
    wf = torch.zeros(32 * 16448, dtype=torch.bfloat16, device=DEV)
    bias = torch.zeros(32, device=DEV)
    out = O.new_out(B, Nn + 3, dtype=torch.float32, device=DEV)
    good = dict(x=x, wf=wf, bias=bias, out=out, B=B, C=C, HW=HW, Nn=Nn, ldo=Nn, pooled=0)
    bad = [dict(C=48), dict(C=0), dict(C=16416), dict(HW=0), dict(Nn=0), dict(ldo=Nn - 1), dict(B=0), dict(x=None),
           dict(wf=None), dict(out=None)]
    for b in bad:
        for pooled in (0, 1):
            _refused(_poolfc(**{**good, **b, "pooled": pooled}), out)
    assert _poolfc(**good) == 0
    _sync()


# ------------------------------------------------------------------------------------------------ preprocess
def _pre(src, out, n, cin, h, w, cpad, mode, mean=None, inv=None):
    return N.lib().hz_preprocess_launch(src if isinstance(src, int) else N.ptr(src), N.ptr(out), n, cin, h, w, cpad, mode,
                                        N.ptr(mean), N.ptr(inv), N.stream_ptr())


def _offset_u8(src, off):
    """The same bytes at a device address that is ``off`` past a 16-byte boundary."""
    buf = torch.zeros(src.numel() + 32, dtype=torch.uint8, device=DEV)
    view = buf[off:off + src.numel()]
    view.copy_(src.reshape(-1))
    assert view.data_ptr() % 16 == off
    return buf, view


def _run_pre(case, src, mean, inv, offset=0):
    _, mode, n, h, w, cin, cpad, _ = case
    keep, dsrc = _offset_u8(src.to(DEV), offset) if mode == 1 else (None, src.contiguous().to(DEV))
    out = O.new_out(n * h * w, cpad, device=DEV)
    m, i = (None, None) if mean is None else (mean.to(DEV), inv.to(DEV))
    assert _pre(dsrc, out, n, cin, h, w, cpad, mode, m, i) == 0
    _sync()
    got, lost = O.split_out(out, n * h * w, cpad)
    assert lost == 0
    return got


@pytest.mark.parametrize("case", O.PRE_CASES, ids=[c[0] for c in O.PRE_CASES])
def test_preprocess(case):
    name, mode, n, h, w, cin, cpad, path = case
    for kind, wm in O.pre_kinds(case):
        src, mean, inv = O.pre_inputs(case, kind, wm)
        got = _run_pre(case, src, mean, inv, 4 if path == "unaligned" else 0)
        ref = O.pre_ref(src, mode, cpad, mean, inv)
        if kind == "exact" or not wm:
            O.check_bits(O.t_bits(got), O.pre_exact_bits(src, mode, cpad, mean, inv), f"{name} {kind} mean={wm}")
        else:
            rep = O.compare(got, ref, False, O.C_PRE)
            print(f"preprocess {name} {kind}: {O.describe(rep)}")
            assert rep.ok, O.describe(rep)
        if path == "u8c3":   # the same pixels through the generic kernel: the same bits
            other = _run_pre(case, src, mean, inv, 4)
            O.check_bits(O.t_bits(other), O.t_bits(got), f"{name} mean={wm}: generic against u8c3")


def test_preprocess_refusals():
    src = torch.zeros(2 * 8 * 5 * 7, device=DEV)
    out = O.new_out(2 * 5 * 7, 24, device=DEV)
    mean, inv = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    good = dict(src=src, out=out, n=2, cin=3, h=5, w=7, cpad=8, mode=0, mean=mean, inv=inv)
    bad = [dict(cpad=12), dict(cin=9), dict(cpad=0), dict(cpad=4), dict(cpad=-8), dict(cin=0), dict(cin=-1), dict(n=0),
           dict(h=0), dict(w=0), dict(src=None), dict(out=None), dict(inv=None)]
    for mode in (0, 1):
        for b in bad:
            _refused(_pre(**{**good, "mode": mode, **b}), out)
    for mode in (-1, 3):
        _refused(_pre(**{**good, "mode": mode}), out)
    assert _pre(**good) == 0
    _sync()


# ------------------------------------------------------------------------------------------------ patchify
@pytest.mark.parametrize("case", O.PATCH_CASES, ids=str)
def test_patchify(case):
    cin, h, w = case
    rows = O.PATCH_N * (h // 16) * (w // 16)
    for wm in (False, True):
        src, mean, inv = O.patch_inputs(case, wm)
        out = O.new_out(rows, cin * 256, device=DEV)
        m, i = (None, None) if not wm else (mean.to(DEV), inv.to(DEV))
        assert _pre(src.to(DEV), out, O.PATCH_N, cin, h, w, 16, 2, m, i) == 0
        _sync()
        got, lost = O.split_out(out, rows, cin * 256)
        assert lost == 0
        ref = O.patch_ref(src, mean, inv)
        if wm:
            rep = O.compare(got, ref, False, O.C_PRE)
            print(f"patchify {case}: {O.describe(rep)}")
            assert rep.ok, O.describe(rep)
        else:
            O.check_bits(O.t_bits(got), _i64(O.bf16_bits(ref.y.float().numpy())), f"patchify {case}", nan_payload=False)


def test_patchify_refusals():
    src = torch.zeros(2 * 8 * 48 * 48 + 8, device=DEV)
    out = O.new_out(2 * 9, 8 * 256, device=DEV)
    good = dict(src=src, out=out, n=2, cin=3, h=32, w=32, cpad=16, mode=2)
    bad = [dict(cpad=8), dict(cpad=32), dict(h=24), dict(w=40), dict(cin=0), dict(cin=9), dict(src=src.data_ptr() + 4),
           dict(src=None), dict(out=None), dict(n=0)]
    for b in bad:
        _refused(_pre(**{**good, **b}), out)
    # a misaligned destination: 8 bytes into the buffer
    rc = N.lib().hz_preprocess_launch(src.data_ptr(), out.data_ptr() + 8, 2, 3, 32, 32, 16, 2, 0, 0, N.stream_ptr())
    _refused(rc, out)
    assert _pre(**good) == 0
    _sync()


# ------------------------------------------------------------------------------------------------ casts
def test_cast_bf16_f32_every_pattern():
    allb = np.arange(65536, dtype=np.uint16)
    x = O.bf16_tensor(allb).to(DEV)
    out = O.new_out(1, 65536, dtype=torch.float32, device=DEV)
    assert N.lib().hz_cast_bf16_f32(x.data_ptr(), out.data_ptr(), 65536, N.stream_ptr()) == 0
    _sync()
    got, lost = O.split_out(out, 1, 65536)
    assert lost == 0
    O.check_bits(O.t_bits(got), _i64(allb.astype(np.uint32) << 16), "bf16 -> fp32", width=32)


def test_cast_f32_bf16_every_rounding():
    pat = O.cast_f32_patterns()
    x = torch.from_numpy(pat.view(np.float32).copy()).to(DEV)
    out = O.new_out(1, pat.size, device=DEV)
    assert N.lib().hz_cast_f32_bf16(x.data_ptr(), out.data_ptr(), pat.size, N.stream_ptr()) == 0
    _sync()
    got, lost = O.split_out(out, 1, pat.size)
    assert lost == 0
    O.check_bits(O.t_bits(got), _i64(O.bf16_bits(pat.view(np.float32))), "fp32 -> bf16", nan_payload=False)


@pytest.mark.parametrize("n", O.CAST_TAILS)
def test_cast_vector_and_tail(n):
    pat = O.cast_f32_patterns()
    sel = pat[np.random.default_rng(n).permutation(pat.size)[:n]]
    x = torch.from_numpy(sel.view(np.float32).copy()).to(DEV)
    out = O.new_out(1, n, device=DEV)
    assert N.lib().hz_cast_f32_bf16(x.data_ptr(), out.data_ptr(), n, N.stream_ptr()) == 0
    _sync()
    got, lost = O.split_out(out, 1, n)
    assert lost == 0
    O.check_bits(O.t_bits(got), _i64(O.bf16_bits(sel.view(np.float32))), f"n = {n}", nan_payload=False)
    xb = O.bf16_tensor((sel >> 16).astype(np.uint16)).to(DEV)
    out = O.new_out(1, n, dtype=torch.float32, device=DEV)
    assert N.lib().hz_cast_bf16_f32(xb.data_ptr(), out.data_ptr(), n, N.stream_ptr()) == 0
    _sync()
    got, lost = O.split_out(out, 1, n)
    assert lost == 0
    O.check_bits(O.t_bits(got), _i64((sel >> 16) << 16), f"n = {n}", width=32)


def test_cast_refusals():
    x32, x16 = torch.zeros(8, device=DEV), torch.zeros(8, dtype=torch.bfloat16, device=DEV)
    o16, o32 = O.new_out(1, 8, device=DEV), O.new_out(1, 8, dtype=torch.float32, device=DEV)
    L, st = N.lib(), N.stream_ptr()
    for n in (0, -1):   # nothing to do: 0, and no launch
        assert L.hz_cast_f32_bf16(x32.data_ptr(), o16.data_ptr(), n, st) == 0
        assert L.hz_cast_bf16_f32(x16.data_ptr(), o32.data_ptr(), n, st) == 0
    _refused(L.hz_cast_f32_bf16(0, o16.data_ptr(), 8, st), o16)
    _refused(L.hz_cast_f32_bf16(x32.data_ptr(), 0, 8, st), o16)
    _refused(L.hz_cast_bf16_f32(0, o32.data_ptr(), 8, st), o32)
    _refused(L.hz_cast_bf16_f32(x16.data_ptr(), 0, 8, st), o32)
    _sync()
