"""The oracle of tests/gemm_oracle.py judged on the CPU, on the inputs the GPU cases run: it is the
convolution torch computes, its fp32 evaluation stays inside the bound the GPU is held to (the measurement
``C_ACC`` and ``C_FN`` come from), the integer-valued cases are exact, and the comparator rejects every
planted fault. Figures: profiles/gemm_oracle/README.md."""
import math

import pytest
import torch

import gemm_oracle as G
from hipzap.ops import conv as CV

CASES = G.all_cases()
SMALL = G.RING_CASES + G.CV_CASES  # (the GEMM grid is large: its cases are sampled below where fp64 conv2d is slow)


def _ids(cases):
    return [c.name for c in cases]


def _torch_conv(case, kind):
    """fp64 ``conv2d`` / ``conv2d_reference`` on the same operands, [M, cout]."""
    x, res = G.case_inputs(case, kind)
    pc = G.case_weights(case, kind)
    if case.xrow:
        x = x.reshape(case.n, 1, 1, case.cin)
    xo = G._bf16(torch.relu(x.float())) if case.x_f32 else x.float()
    w4 = pc.dense().double().reshape(case.cout, case.r, case.s, case.cin).permute(0, 3, 1, 2).contiguous()
    xn = xo.double().permute(0, 3, 1, 2)
    rn = None if res is None else res.double().reshape(case.n, *case.PQ, case.cout).permute(0, 3, 1, 2)
    a = torch.nn.functional.conv2d(xn, w4, pc.bias.double(), stride=case.stride, padding=case.pad)
    if rn is not None:
        a = a + rn
    b = CV.conv2d_reference(xn, w4, pc.bias.double(), None, case.stride, case.pad, rn, case.act)
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(case.M, case.cout)  # noqa: E731
    return flat(G.activation(a, case.act)), flat(b)


@pytest.mark.parametrize("case", SMALL + G.all_gemm_cases()[::7], ids=_ids(SMALL + G.all_gemm_cases()[::7]))
def test_oracle_is_torch_conv2d_fp64(case):
    for kind in G.KINDS:
        ref = G.case_ref(case, kind)
        a, b = _torch_conv(case, kind)
        tol = 1e-12 * ref.A  # fp64 against fp64: summation order only
        assert ((ref.y - a).abs() <= tol).all(), (kind, float((ref.y - a).abs().max()))
        # conv2d_reference computes in the dtype it is given except where it calls .float(): fp32
        assert ((ref.y - b.double()).abs() <= 64 * G.U32 * ref.A).all(), (kind, float((ref.y - b).abs().max()))


def measure():
    """Worst |fp32 - fp64| of the accumulation in units of u A, and of erf / tanh in units of u |f|, over
    the case table -> (acc ratio, case, erf ratio, tanh ratio)."""
    worst, where, w_erf, w_tanh = 0.0, None, 0.0, 0.0
    for case in CASES:
        r64 = G.case_ref(case, "rand")
        r32 = G.case_ref(case, "rand", torch.float32)
        q = float(((r32.acc.double() - r64.acc).abs() / (G.U32 * r64.A)).max())
        if q > worst:
            worst, where = q, case.name
        a = r32.acc  # an fp32 argument: the function's own error, not the argument's
        if case.act == "gelu":
            t = a * 0.70710678118654752
            e64 = torch.erf(t.double())
            w_erf = max(w_erf, float(((torch.erf(t).double() - e64).abs() / (G.U32 * e64.abs().clamp_min(1e-300))).max()))
        if case.act == "tanh":
            e64 = torch.tanh(a.double())
            w_tanh = max(w_tanh, float(((torch.tanh(a).double() - e64).abs() / (G.U32 * e64.abs().clamp_min(1e-300))).max()))
    return worst, where, w_erf, w_tanh


def _pow2(v):
    return 2.0 ** math.ceil(math.log2(v))


def test_constants_follow_the_measurement():
    worst, where, w_erf, w_tanh = measure()
    print(f"\nfp32 against fp64: accumulation worst {worst:.3f} u A ({where}); erf {w_erf:.3f} u, tanh {w_tanh:.3f} u")
    # the rule: 4 x the worst figure, up to a power of two; torch's summation order depends on the host, so
    # the constants may sit above the rule's value here, never below it
    assert G.C_ACC >= _pow2(4 * worst), (worst, where)
    assert G.C_FN >= _pow2(4 * max(w_erf, w_tanh)), (w_erf, w_tanh)
    kmax = max(c.K for c in CASES)
    assert G.C_ACC < G.c_ops(kmax) == kmax + 19  # far inside the operation-count ceiling


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_fp32_oracle_inside_the_bound(case):
    """The fp32 evaluation, unrounded, against fp64 under the bound WITHOUT its store term."""
    r64 = G.case_ref(case, "rand")
    r32 = G.case_ref(case, "rand", torch.float32)
    bd = G.bound(r64, case.act, True)  # r_out = u |ref|: fp32's own last rounding
    err = (r32.y.double() - r64.y).abs()
    assert (err <= bd).all(), (float((err / bd).max()), case.name)
    # and stored as the kernel stores it, under the comparator
    stored = r32.y if case.out_f32 else G._bf16(r32.y)
    G.check(stored, r64, case.act, case.out_f32, case.name)


EXACT = [c for c in CASES if G.exact_ok(c)]


@pytest.mark.parametrize("case", EXACT, ids=_ids(EXACT))
def test_exact_cases_are_exact(case):
    r64 = G.case_ref(case, "exact")
    r32 = G.case_ref(case, "exact", torch.float32)
    assert float(r64.A.max()) < 2 ** 24          # |sum| + |bias| + |res| <= A: every partial sum is exact
    assert torch.equal(r64.acc, r64.acc.round())  # integers
    assert torch.equal(r32.y.double(), r64.y) and torch.equal(G.bits(r32.y), G.bits(r64.y.float()))
    x, _ = G.case_inputs(case, "exact")
    assert x.float().abs().max() <= 3 and G.case_weights(case, "exact").dense().abs().max() <= 2
    assert float(r64.y.abs().max()) > 0


def test_case_table_covers_what_it_claims():
    insts = {c.inst for c in G.RING_CASES}
    assert insts == {"fast1x1", "fast", "generic", "xrow", "f32in1x1", "f32in3x3"}
    assert {c.cin for c in G.RING_CASES if c.inst == "generic"} == {8, 16}
    assert any(c.r != c.s for c in G.RING_CASES if c.inst == "fast")
    assert any(c.r != c.s for c in G.RING_CASES if c.inst == "generic")
    assert any(c.M == 1 for c in G.RING_CASES) and any(c.M == 105 for c in G.RING_CASES)
    assert {c.act for c in G.XROW_CASES} == set(CV.ACT) and any(not c.bias for c in G.XROW_CASES)
    assert len(G.ring_configs()) == 41 and set(G.KSTEPS_ALL) >= {1, 2, 3, 6, 7, 15, 17}
    for cfg in CV.LDS_TILES:  # every cfg gets every M and K with at least two widths
        cs = G.gemm_cases(cfg)
        ws = G.gemm_widths(cfg)
        assert len(ws) >= 2 and all(CV.lds_fits(cfg, n) for n in ws), (cfg, ws)
        assert len(cs) == 3 * len(G.GEMM_K) * len(ws)
        assert {(c.n, c.cin) for c in cs} == {(m, k) for m in G.gemm_ms(cfg) for k in G.GEMM_K}
    acts = {(c.act, c.res, c.out_f32) for c in G.all_gemm_cases()}
    assert {a for a, _, _ in acts} == set(CV.ACT) and {r for _, r, _ in acts} == {True, False}
    for cfg in CV.LDS_CONV_CFGS:
        assert len(G.cv_cases(cfg)) == 2 * len(G._CV_GEOM)


# ------------------------------------------------------------------------------------------------
# planted faults: what a subtly wrong kernel would store, judged by the comparator and by the old metric
def _stored(y32, case):
    return y32.float() if case.out_f32 else G._bf16(y32.float())


def _with_weights(case, kind, fn):
    pc = G.case_weights(case, kind)
    wf, b = fn(pc.wf.clone(), pc.bias.clone())
    return CV.PackedConv(wf, b, pc.cin, pc.cout, pc.r, pc.s, pc.stride, pc.pad)


def _eval(case, kind="rand", pc=None, x=None, res="same", act=None, hooks=None):
    """The fp32 evaluation of a (faulty) variant of ``case``, as the kernel would store it."""
    x0, r0 = G.case_inputs(case, kind)
    x = x0 if x is None else x
    r = r0 if isinstance(res, str) else res
    pc = pc or G.case_weights(case, kind)
    act = act or case.act
    if case.xrow:
        ref = G.linear_ref(x, pc, case.n, None if r is None else r.reshape(case.n, case.cout), act, torch.float32, hooks)
    else:
        ref = G.conv_ref(x, pc, case.n, case.h, case.w, r, act, case.x_f32, torch.float32, hooks)
    return ref


def _by_name(name):
    return next(c for c in CASES if c.name == name)


def _fault_last_kstep(case):
    pc = _with_weights(case, "rand", lambda wf, b: (wf.index_fill(1, torch.tensor([wf.shape[1] - 1]), 0), b))
    return _stored(_eval(case, pc=pc).y, case)


def _fault_partial(case, kw=4, wave=1):
    ks = case.ksteps
    spw = -(-ks // kw)
    idx = torch.arange(wave * spw, min(ks, (wave + 1) * spw))
    pc = _with_weights(case, "rand", lambda wf, b: (wf.index_fill(1, idx, 0), b))
    return _stored(_eval(case, pc=pc).y, case)


def _fault_swap_hw(case):
    """The input indexed with H and W exchanged (``pih * H + piw``): the same memory read as a w x h image,
    the output written back in the same exchanged order."""
    x, res = G.case_inputs(case, "rand")
    pc = G.case_weights(case, "rand")
    P, Q = case.PQ
    y = G.conv_ref(x.reshape(case.n, case.w, case.h, case.cin), pc, case.n, case.w, case.h, None, "none", case.x_f32,
                   torch.float32).y  # [n * Q * P, cout], rows in (q, p) order of the exchanged image
    acc = y.reshape(case.n, P, Q, case.cout)
    if res is not None:
        acc = acc + res.float()
    return _stored(G.activation(acc, case.act).reshape(case.M, case.cout), case)


def _fault_res_neighbour(case):
    _, res = G.case_inputs(case, "rand")
    return _stored(_eval(case, res=torch.roll(res.reshape(case.M, case.cout), 1, 0).reshape(res.shape)).y, case)


def _fault_bias_shift(case):
    pc = _with_weights(case, "rand", lambda wf, b: (wf, torch.roll(b, 4)))
    return _stored(_eval(case, pc=pc).y, case)


def _fault_act_first(case):
    _, res = G.case_inputs(case, "rand")
    y = _eval(case, res=None).y + res.reshape(case.M, case.cout).float()
    return _stored(y, case)


def _fault_unwritten(case):
    y = _stored(_eval(case).y, case).clone()
    y[case.M - 1, case.cout - 1] = float("nan")
    return y


FAULTS = {  # name -> (case, what the faulty kernel stores)
    "last 32-deep K step dropped": ("3x3-5x7-n3", _fault_last_kstep),
    "one K-split partial dropped": ("3x3-7x5-n1", _fault_partial),
    "H and W exchanged": ("3x3-5x7-n3", _fault_swap_hw),
    "replicate padding": ("3x3-5x7-n3", lambda c: _stored(_eval(c, hooks={"padding": "replicate"}).y, c)),
    "residual of the neighbouring pixel": ("c40-rowmajor", _fault_res_neighbour),
    "bias shifted by 4 channels": ("c40-rowmajor", _fault_bias_shift),
    "fp32 output rounded through bf16": ("3x3-7x5-n3", lambda c: G._bf16(_eval(c).y)),
    "tanh-approximation GELU": ("c96-blocked", lambda c: _stored(G.gelu_tanh(_eval(c).acc), c)),
    "missing ReLU": ("3x3s2-5x7-n3", lambda c: _stored(_eval(c, act="none").y, c)),
    "activation before the residual": ("3x3-5x7-n3", _fault_act_first),
    "one element of a partial tile unwritten": ("3x3-5x7-n3", _fault_unwritten),
}


def fault_table():
    """-> [(fault, case, comparator's worst ratio, bad elements, old metric, old metric's verdict)]."""
    rows = []
    for name, (cname, fn) in FAULTS.items():
        case = _by_name(cname)
        got = fn(case)
        ref = G.case_ref(case, "rand")
        rep = G.compare(got, ref, case.act, case.out_f32)
        old = G.old_metric(torch.nan_to_num(got, nan=0.0), ref.y)  # (an unwritten torch.empty element: anything)
        rows.append((name, cname, rep.ratio, rep.bad, old, old < (1e-2 if case.out_f32 else 2e-2)))
    return rows


@pytest.mark.parametrize("fault", list(FAULTS))
def test_comparator_rejects_planted_fault(fault):
    cname, fn = FAULTS[fault]
    case = _by_name(cname)
    # the unfaulted evaluation passes ...
    G.check(_stored(_eval(case).y, case), G.case_ref(case, "rand"), case.act, case.out_f32, cname)
    # ... the faulted one does not
    rep = G.compare(fn(case), G.case_ref(case, "rand"), case.act, case.out_f32)
    assert not rep.ok and rep.bad >= 1, (fault, G.describe(rep))


def test_guard_element_written_is_seen():
    for case in (_by_name("c40-rowmajor"), _by_name("3x3-5x7-n3"), _by_name("xrow-gelu")):
        buf = G.new_out(case)
        got, lost = G.split_out(buf, case)
        assert lost == 0 and got.shape == (case.M, case.cout) and got.isnan().all()
        _, _, live, total = G.out_layout(case)
        for pos in (live, total - 1):
            b = buf.clone()
            b[pos] = 0.0
            assert G.split_out(b, case)[1] == 1
        if G.out_layout(case)[1] > case.cout:  # a guard column inside the live rows
            b = buf.clone()
            b[case.cout] = 1.0
            assert G.split_out(b, case)[1] == 1
        b = buf.clone()
        G.bits(b)[total - 1] += 1  # another NaN is not the fill
        assert b[total - 1].isnan()
        assert G.split_out(b, case)[1] == 1


def test_fault_table_prints():
    print()
    for row in fault_table():
        print("| %s | %s | %.3g | %d | %.2e | %s |" % (*row[:5], "passes" if row[5] else "fails"))
