"""The oracles of tests/vision_oracle.py judged on the CPU, on the inputs the GPU cases run: they are what
torch computes in fp64 where torch has the operation, the packing oracles are the host packers bit for bit,
the constants follow the fp32-against-fp64 measurement, the exact cases are exact, and the comparator rejects
every planted fault. Figures: profiles/vision_oracle/README.md."""
import math

import numpy as np
import pytest
import torch

import vision_oracle as O
from hipzap.engine import lmbatch as LB
from hipzap.ops import conv as CV
from hipzap.ops import vision as V


def _bf16(t):
    return t.bfloat16().to(t.dtype)


# ------------------------------------------------------------------------------------------------
# agreement with torch (fp64)
@pytest.mark.parametrize("case", O.MAXPOOL_CASES, ids=str)
def test_maxpool_is_torch_max_pool2d(case):
    n, h, w, c, k, s, p = case
    for kind in O.MAXPOOL_KINDS:
        x = O.maxpool_input(case, kind)
        bits = O.t_bits(x).reshape(-1)
        assert bits.unique().numel() == bits.numel()          # every value differs from every other
        have = set(bits.tolist())
        want = {0xFF80, 0x0000, 0x8000, O.BF16_MAX} if kind == "distinct" else {0xFF80, 0xFF7F}
        assert want <= have, (kind, want - have)
        if kind == "negative":
            assert bool((x.float() < 0).all())
        ref = O.maxpool_ref(x, k, s, p)
        assert ref.shape == (n, *O.pool_out(h, w, k, s, p), c)
        if p <= k // 2:
            t = torch.nn.functional.max_pool2d(x.double().permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1)
            assert torch.equal(ref, t)
        # a clamped tap changes nothing: replicate padding gives the same maximum (maxpool_kernel<3>)
        ih = (torch.arange(-p, h + p + k) ).clamp(0, h - 1)
        iw = (torch.arange(-p, w + p + k)).clamp(0, w - 1)
        P, Q = O.pool_out(h, w, k, s, p)
        xr = x.double()[:, ih][:, :, iw]
        rep = torch.stack([xr[:, r:r + s * (P - 1) + 1:s, q:q + s * (Q - 1) + 1:s] for r in range(k) for q in range(k)]).amax(0)
        assert torch.equal(ref, rep)


@pytest.mark.parametrize("case", O.AVGPOOL_CASES, ids=str)
def test_avgpool_is_torch_mean(case):
    for kind in O.KINDS:
        x = O.pool_input(*case, kind)
        ref = O.avgpool_ref(x)
        assert ((ref.y - x.double().mean(1)).abs() <= 1e-12 * ref.A).all()
        assert torch.equal(O.blocked(x), CV.to_blocked(x.reshape(case[0], case[1], 1, case[2])).reshape(O.blocked(x).shape))


@pytest.mark.parametrize("case", O.POOLFC_CASES, ids=O.poolfc_name)
def test_poolfc_is_torch_mean_matmul(case):
    for kind in O.KINDS:
        x, w, b = O.poolfc_inputs(case, kind)
        assert torch.equal(w, _bf16(w))
        ref = O.poolfc_ref(x, w, b)
        m = x.double() if case[6] else x.double().mean(1)
        t = m @ w.double().T + b.double()
        assert ((ref.y - t).abs() <= 1e-12 * ref.A.clamp_min(1e-300)).all()
        pc = CV.pack_linear(w, b)
        hx = x if case[6] else x.reshape(case[0], case[1], 1, case[2])
        host = (x.float() @ pc.dense().float().t() + pc.bias.float()) if case[6] else V.pool_fc_ref(hx, pc)
        assert ((ref.y - host.double()).abs() <= 64 * O.U32 * ref.A + 1e-30).all()


def test_preprocess_and_patchify_are_torch_permutes():
    for case in O.PRE_CASES:
        _, mode, n, h, w, cin, cpad, _ = case
        for kind, wm in O.pre_kinds(case):
            src, mean, inv = O.pre_inputs(case, kind, wm)
            ref = O.pre_ref(src, mode, cpad, mean, inv)
            v = src.double().permute(0, 2, 3, 1) if mode == 0 else src.double() * float(O.INV255)
            if wm:
                v = (v - mean.double()) * inv.double()
            t = torch.nn.functional.pad(v, (0, cpad - cin)).reshape(-1, cpad)
            assert torch.equal(ref.y, t), case[0]
            host = V.preprocess_reference(src, cpad, None if mean is None else mean.tolist(),
                                          None if mean is None else (1.0 / inv.double()).tolist())
            assert ((ref.y - host.double().reshape(-1, cpad)).abs() <= 64 * O.U32 * ref.A + 1e-30).all(), case[0]
    for case in O.PATCH_CASES:
        for wm in (False, True):
            src, mean, inv = O.patch_inputs(case, wm)
            ref = O.patch_ref(src, mean, inv)
            v = src.double()
            if wm:
                v = (v - mean.double().view(1, -1, 1, 1)) * inv.double().view(1, -1, 1, 1)
            n, c, h, w = v.shape
            t = v.reshape(n, c, h // 16, 16, w // 16, 16).permute(0, 2, 4, 1, 3, 5).reshape(-1, c * 256)
            assert torch.equal(torch.nan_to_num(ref.y, posinf=9e99, neginf=-9e99), torch.nan_to_num(t, posinf=9e99, neginf=-9e99))
            if not wm:
                assert torch.equal(O.t_bits(V.patchify_reference(src)), torch.from_numpy(O.bf16_bits(ref.y.float().numpy()).astype(np.int64)))


def test_bf16_rounding_is_torch_rounding():
    pat = O.cast_f32_patterns()
    assert pat.size == 327680
    f = torch.from_numpy(pat.view(np.float32).copy())
    want = O.t_bits(f.bfloat16())
    got = torch.from_numpy(O.bf16_bits(f.numpy()).astype(np.int64))
    assert O.compare_bits(got, want, nan_payload=False).ok
    nan = f.isnan()
    assert bool((got[nan] == O.NAN16).all())   # pack.hip's rule; the cast kernels keep some NaN
    allb = np.arange(65536, dtype=np.uint16)
    assert torch.equal(O.t_bits(O.bf16_tensor(allb).float()), torch.from_numpy(allb.astype(np.int64)) << 16)
    assert np.array_equal(O.bits_to_f32(allb).view(np.uint32), allb.astype(np.uint32) << 16)


# ------------------------------------------------------------------------------------------------
# agreement with the host packers, bit for bit
def _host_pack(name):
    cout, cin, r, s, cin_p, rows, ksteps, _, _ = O.PACK_CASES[name]
    w, bn, bias_in = O.pack_inputs(name)
    tw = torch.from_numpy(w)
    tb = None if bias_in is None else torch.from_numpy(bias_in)
    if name == "linear":
        return CV.pack_linear(tw.reshape(cout, cin), tb), None
    d = None if bn is None else dict(zip(("weight", "bias", "running_mean", "running_var"), map(torch.from_numpy, bn)))
    return CV.pack_conv(tw, tb, d, cin_pad=cin_p), None


@pytest.mark.parametrize("name", list(O.PACK_CASES))
def test_pack_oracle_is_the_host_packer(name):
    cout, cin, r, s, cin_p, rows, ksteps, _, _ = O.PACK_CASES[name]
    wf, bias = O.pack_ref(name)
    assert wf.shape == (rows // 16, ksteps, 64, 8) and wf.dtype == np.uint16
    pc, _ = _host_pack(name)
    host = O.t_bits(pc.wf).numpy().astype(np.uint16)    # rows padded to the host's row_pad, ksteps = ceil(K / 32)
    hk = host.shape[1]
    assert hk <= ksteps and host.shape[0] * 16 >= cout
    g = min(host.shape[0], rows // 16)
    nanfix = lambda a: np.where((a & 0x7FFF) > 0x7F80, O.NAN16, a)  # noqa: E731  (torch keeps a NaN's sign)
    assert np.array_equal(nanfix(host[:g]), wf[:g, :hk])
    assert not wf[:, hk:].any() and not wf[g:].any() and not host[g:].any()
    assert np.array_equal(pc.bias.numpy().view(np.uint32), bias.view(np.uint32))
    # the padding is zero: rows cout .., columns K .., channels cin .. cin_p - 1
    dense = np.zeros((rows, ksteps * 32), dtype=np.uint16)
    t, ks, lane, j = np.meshgrid(np.arange(rows // 16), np.arange(ksteps), np.arange(64), np.arange(8), indexing="ij")
    dense[t * 16 + (lane & 15), ks * 32 + 8 * (lane >> 4) + j] = wf
    assert not dense[cout:].any() and not dense[:, r * s * cin_p:].any()
    assert not dense[:, :r * s * cin_p].reshape(rows, r * s, cin_p)[:, :, cin:].any()


@pytest.mark.parametrize("name", list(O.FRAG_CASES))
def test_frag_oracle_is_the_host_packer(name):
    c = O.FRAG_CASES[name]
    a, b, ba, bb = O.frag_inputs(name)
    out, bias = O.frag_pack_ref(name)
    R, K = c["R"], c["K"]
    r = torch.arange(R)
    nsrc = 4 * c["ih"] if c["ih"] else c["nrows"]
    src = torch.arange(nsrc)
    if c["ih"]:   # engine/lmbatch.py pack_lmb: row 4 j + q = gate q of unit j
        src = src.reshape(4, c["ih"]).t().reshape(-1)
    w = torch.zeros(R, K)
    if a is not None:
        w[:nsrc, :c["acols"]] = torch.from_numpy(a)[src, :c["acols"]]
    if b is not None:
        w[:nsrc, c["ka"]:c["ka"] + c["bcols"]] = torch.from_numpy(b)[src, :c["bcols"]]
    if c["out"]:
        host = O.t_bits(LB.frag_pack(w)).numpy().astype(np.uint16)
        host = np.where((host & 0x7FFF) > 0x7F80, O.NAN16, host)
        assert np.array_equal(host, out)
    else:
        assert out is None
    if c["bias_out"]:
        want = torch.zeros(R)
        if ba is not None:
            want[:nsrc] = torch.from_numpy(ba)[src] + (torch.from_numpy(bb)[src] if bb is not None else 0)
        assert np.array_equal(want.numpy().view(np.uint32), bias.view(np.uint32))
    else:
        assert bias is None


# ------------------------------------------------------------------------------------------------
# the constants
def measure():
    """Worst |fp32 - fp64| in units of u A over the case tables -> {operation: (worst, case)}."""
    worst = {"avgpool": (0.0, None), "pool_fc": (0.0, None), "preprocess": (0.0, None)}

    def note(op, r32, r64, name):
        q = float(((r32.y.double() - r64.y).abs() / (O.U32 * r64.A).clamp_min(1e-300)).max())
        if q > worst[op][0]:
            worst[op] = (q, name)
    for case in O.AVGPOOL_CASES:
        x = O.pool_input(*case, "rand")
        note("avgpool", O.avgpool_ref(x, torch.float32), O.avgpool_ref(x), str(case))
    for case in O.POOLFC_CASES:
        x, w, b = O.poolfc_inputs(case, "rand")
        note("pool_fc", O.poolfc_ref(x, w, b, torch.float32), O.poolfc_ref(x, w, b), O.poolfc_name(case))
    for case in O.PRE_CASES:
        src, mean, inv = O.pre_inputs(case, "rand", True)
        note("preprocess", O.pre_ref(src, case[1], case[6], mean, inv, torch.float32),
             O.pre_ref(src, case[1], case[6], mean, inv), case[0])
    for case in O.PATCH_CASES:
        src, mean, inv = O.patch_inputs(case, True)
        note("preprocess", O.patch_ref(src, mean, inv, torch.float32), O.patch_ref(src, mean, inv), f"patchify {case}")
    return worst


def _pow2(v):
    return 2.0 ** math.ceil(math.log2(v))


def test_constants_follow_the_measurement():
    worst = measure()
    print()
    for op, (q, name) in worst.items():
        print(f"fp32 against fp64, {op}: worst {q:.3f} u A ({name})")
    # the rule: 4 x the worst figure, up to a power of two, never above the operation count; torch's
    # summation order depends on the host, so a constant may sit above the rule's value here, never below 4 x
    assert O.C_POOL >= 4 * worst["avgpool"][0] and O.C_POOL >= min(_pow2(4 * worst["avgpool"][0]), 50.0)
    assert O.C_POOLFC >= 4 * worst["pool_fc"][0] and O.C_POOLFC >= _pow2(4 * worst["pool_fc"][0])
    # preprocess: two roundings that can each reach u A (a mean of the other sign), so 4 x the figure passes
    # the operation count and the count is the constant: a ceiling no correct evaluation exceeds
    assert worst["preprocess"][0] <= 3.0 < O.C_PRE == 4.0 == min(_pow2(4 * worst["preprocess"][0]), 4.0)
    assert O.avgpool_c(1) == 2.0 and O.avgpool_c(49) == O.C_POOL < 50
    assert all(O.poolfc_c(c) == O.C_POOLFC < c[1] + c[2] + 3 for c in O.POOLFC_CASES)


def test_fp32_oracles_inside_the_bound():
    """The fp32 evaluation, stored as the kernel stores it, under the comparator."""
    for case in O.AVGPOOL_CASES:
        x = O.pool_input(*case, "rand")
        O.check(_bf16(O.avgpool_ref(x, torch.float32).y), O.avgpool_ref(x), False, O.avgpool_c(case[1]), str(case))
    for case in O.POOLFC_CASES:
        x, w, b = O.poolfc_inputs(case, "rand")
        O.check(O.poolfc_ref(x, w, b, torch.float32).y, O.poolfc_ref(x, w, b), True, O.poolfc_c(case), O.poolfc_name(case))
    for case in O.PRE_CASES:
        src, mean, inv = O.pre_inputs(case, "rand", True)
        O.check(_bf16(O.pre_ref(src, case[1], case[6], mean, inv, torch.float32).y),
                O.pre_ref(src, case[1], case[6], mean, inv), False, O.C_PRE, case[0])
    for case in O.PATCH_CASES:
        src, mean, inv = O.patch_inputs(case, True)
        O.check(_bf16(O.patch_ref(src, mean, inv, torch.float32).y), O.patch_ref(src, mean, inv), False, O.C_PRE, str(case))


def test_exact_cases_are_exact():
    for case in O.AVGPOOL_CASES:
        x = O.pool_input(*case, "exact")
        r64, r32 = O.avgpool_ref(x), O.avgpool_ref(x, torch.float32)
        assert x.float().abs().max() <= 8 and float(r64.A.max()) * case[1] < 2 ** 24
        if O.is_pow2(case[1]):
            assert torch.equal(r32.y.double(), r64.y)
    n_exact = 0
    for case in O.POOLFC_CASES:
        x, w, b = O.poolfc_inputs(case, "exact")
        assert torch.equal(x.float(), x.float().round()) and w.abs().max() <= 2
        if O.poolfc_exact_ok(case):
            r64, r32 = O.poolfc_ref(x, w, b), O.poolfc_ref(x, w, b, torch.float32)
            assert float(r64.A.max()) * case[1] < 2 ** 24      # every partial sum, scaled by HW, is an integer
            assert torch.equal(r32.y.double(), r64.y) and float(r64.y.abs().max()) > 0
            n_exact += 1
    assert n_exact >= 12
    for case in O.PRE_CASES:
        for kind, wm in O.pre_kinds(case):
            if kind == "exact" or not wm:
                src, mean, inv = O.pre_inputs(case, kind, wm)
                O.pre_exact_bits(src, case[1], case[6], mean, inv)   # asserts fp32 == fp64 with a mean


def test_case_table_covers_what_it_claims():
    assert {c[4] for c in O.MAXPOOL_CLAMPED} == {3} and 3 not in {c[4] for c in O.MAXPOOL_LOOP}
    assert {c[4] for c in O.MAXPOOL_LOOP} == {1, 2, 4, 5, 7}
    assert (1, 1, 1, 8, 3, 2, 1) in O.MAXPOOL_CLAMPED and any(c[6] == 2 for c in O.MAXPOOL_CLAMPED)
    assert [c for c in O.AVGPOOL_CASES] == [(1, 1, 64), (2, 31, 64), (2, 33, 128), (3, 49, 192)]
    pf = O.POOLFC_CASES
    assert {c[2] for c in pf if not c[6]} >= {32, 96, 160, 512, 2048, 2112}
    assert {c[1] for c in pf if c[2] == 64} >= {1, 15, 16, 17, 49} and {c[3] for c in pf if c[2] == 64} >= {1, 16, 33}
    assert any(c[4] == 3 for c in pf) and any(not c[5] for c in pf) and any(c[0] == 3 for c in pf)
    assert {c[2] for c in pf if c[6]} == {32, 160, 2112}
    # C = 2112: 17 channel blocks per wave, more than the 16 weight fragments of one batch
    assert ((2112 // 32) + 3) // 4 > 16 >= ((2048 // 32) + 3) // 4
    # C = 32, 96, 160: at least one of the four waves owns no channel block
    for c in (32, 96, 160):
        ncb = c // 32
        cpw = (ncb + 3) // 4
        assert any(w * cpw >= ncb for w in range(4))
    m0 = [c for c in O.PRE_CASES if c[1] == 0]
    assert {c[5] for c in m0} == {1, 3, 4, 8} and {c[6] for c in m0} == {8, 16, 24}
    assert any(c[2] * c[3] * c[4] == 257 for c in m0)
    u8 = [c for c in O.PRE_CASES if c[1] == 1]
    assert {c[5] for c in u8 if c[7] == "generic"} == {1, 3, 4}
    assert any(c[5] == 3 and (c[2] * c[3] * c[4]) % 4 for c in u8 if c[7] == "generic")
    assert any(c[7] == "unaligned" and (c[2] * c[3] * c[4]) % 4 == 0 for c in u8)
    assert {c[2] * c[3] * c[4] for c in u8 if c[7] == "u8c3"} == {4, 1020, 1024, 1028, 2040}
    src, _, _ = O.pre_inputs(O.PRE_BY_NAME["u8c3-allbytes"], "rand", False)
    slots = src.reshape(256, 12)       # thread t, byte slot s
    for s in range(12):
        assert sorted(slots[:, s].tolist()) == list(range(256))
    assert {c[0] for c in O.PATCH_CASES} == {1, 3, 8} and {c[1:] for c in O.PATCH_CASES} == {(16, 32), (32, 16), (48, 48)}
    for case in O.PATCH_CASES:
        src, _, _ = O.patch_inputs(case, False)
        have = set(O.t_bits(src).reshape(-1).tolist())
        assert set(O.F32_SPECIALS) <= have
    # packing
    for name, (cout, cin, r, s, cin_p, rows, ksteps, bn, bias) in O.PACK_CASES.items():
        assert rows % 16 == 0 and rows >= cout and ksteps * 32 >= r * s * cin_p and cin_p >= cin, name
        w, b, _ = O.pack_inputs(name)
        assert set(O.W_SPECIALS) <= set(w.view(np.uint32).reshape(-1).tolist()), name
        if bn:
            gamma, _, _, var = b
            assert var[0] == 0 and gamma[2] == 0 and gamma[3] < 0
    assert O.pack_chunks("grid-stride") == 589824 > 2048 * 256
    assert O.PACK_CASES["stem-like"][6] * 32 - 392 < 32 and O.PACK_CASES["linear"][6] * 32 - 64 == 64
    assert O.PACK_CASES["bn-bias"][7] and O.PACK_CASES["bn-bias"][8] and O.PACK_CASES["wide-pad"][4] == 16
    fc = O.FRAG_CASES
    assert fc["grid-stride"]["R"] // 16 * (fc["grid-stride"]["K"] // 32) * 64 == 1052672 > 4096 * 256
    assert fc["interleave-h5"]["ih"] == 5 and fc["rows-21"]["nrows"] == 21
    s = fc["a-b-seam"]
    # k 16 .. 23 is one lane's run: a (16, 17), zeros (18, 19: acols < ka), b (20 ..)
    assert s["ka"] % 8 and s["ka"] // 8 * 8 < s["acols"] < s["ka"] and s["b"] and s["bcols"] > 0
    assert fc["ld-wide"]["lda"] > fc["ld-wide"]["acols"] and fc["ld-wide"]["ldb"] > fc["ld-wide"]["bcols"]
    assert not fc["bias-only"]["out"] and not fc["no-bias-out"]["bias_out"]
    assert any(c["bias_b"] for c in fc.values()) and any(c["bias_a"] and not c["bias_b"] for c in fc.values())


# ------------------------------------------------------------------------------------------------
# planted faults: name -> () -> (comparator's report on the faulted output, old whole-tensor metric or None)
MP3, MPL = (2, 9, 11, 64, 3, 2, 1), (1, 8, 6, 16, 4, 2, 1)


def _mp(case, kind="distinct", **kw):
    n, h, w, c, k, s, p = case
    x = O.maxpool_input(case, kind)
    good, bad = O.maxpool_ref(x, k, s, p), O.maxpool_ref(x, k, s, p, **kw)
    assert O.compare_bits(O.round_bf16(good), O.round_bf16(good), zero_sign=False).ok
    return O.compare_bits(O.round_bf16(bad), O.round_bf16(good), zero_sign=False), None


def _avg(case, divisor):
    x = O.pool_input(*case, "rand")
    ref = O.avgpool_ref(x)
    O.check(_bf16(ref.y.float()), ref, False, O.avgpool_c(case[1]))
    got = _bf16(O.avgpool_ref(x, divisor=divisor).y.float())
    return O.compare(got, ref, False, O.avgpool_c(case[1])), O.old_metric(got, ref.y)


def _pfc(case, **kw):
    x, w, b = O.poolfc_inputs(case, "rand")
    ref = O.poolfc_ref(x, w, b)
    O.check(ref.y.float(), ref, True, O.poolfc_c(case))
    got = O.poolfc_ref(x, w, b, **kw).y.float()
    return O.compare(got, ref, True, O.poolfc_c(case)), O.old_metric(got, ref.y)


def _pre(name, **kw):
    case = O.PRE_BY_NAME[name]
    src, mean, inv = O.pre_inputs(case, "rand", True)
    ref = O.pre_ref(src, case[1], case[6], mean, inv)
    O.check(_bf16(ref.y.float()), ref, False, O.C_PRE)
    got = _bf16(O.pre_ref(src, case[1], case[6], mean, inv, **kw).y.float())
    return O.compare(got, ref, False, O.C_PRE), O.old_metric(got, ref.y)


def _trunc(name):
    case = O.PRE_BY_NAME[name]
    src, mean, inv = O.pre_inputs(case, "rand", False)
    want = O.pre_exact_bits(src, case[1], case[6], None, None)
    got = torch.from_numpy(O.bf16_trunc_bits(O.pre_ref(src, case[1], case[6], None, None, torch.float32).y.numpy()).astype(np.int64))
    return O.compare_bits(got, want), None


def _pack(name, **faults):
    wf, bias = O.pack_ref(name)
    fw, fb = O.pack_ref(name, **faults)
    got = torch.from_numpy(np.concatenate([fw.reshape(-1).astype(np.int64), fb.view(np.uint32).astype(np.int64)]))
    want = torch.from_numpy(np.concatenate([wf.reshape(-1).astype(np.int64), bias.view(np.uint32).astype(np.int64)]))
    return O.compare_bits(got, want, width=32), None


def _frag_lane():
    out, _ = O.frag_pack_ref("a-b-seam")
    bad, _ = O.frag_pack_ref("a-b-seam", lane_fault=True)
    return O.compare_bits(torch.from_numpy(bad.astype(np.int64)), torch.from_numpy(out.astype(np.int64))), None


def _guard():
    buf = O.new_out(5, 17, 20, torch.float32)
    assert O.split_out(buf, 5, 17, 20)[1] == 0 and O.untouched(buf)
    buf[17] = 1.0
    lost = O.split_out(buf, 5, 17, 20)[1]
    return O.Report(lost == 0, float("inf") if lost else 0.0, 17, 1.0, float("nan"), 0.0, lost), None


FAULTS = {
    **{f"maxpool 3x3: tap ({r},{q}) dropped": (lambda r=r, q=q: _mp(MP3, drop=(r, q))) for r in range(3) for q in range(3)},
    **{f"maxpool 4x4 loop: tap ({r},{q}) dropped": (lambda r=r, q=q: _mp(MPL, drop=(r, q))) for r in range(4) for q in range(4)},
    "maxpool 3x3: zero padding": lambda: _mp(MP3, "negative", pad_value=0.0),
    "maxpool 4x4 loop: zero padding": lambda: _mp(MPL, "negative", pad_value=0.0),
    "avgpool HW=31: divisor 32": lambda: _avg((2, 31, 64), 32),
    "avgpool HW=33: divisor 64 (padded HW)": lambda: _avg((2, 33, 128), 64),
    "pool_fc HW=15: divisor 16 (the load batch)": lambda: _pfc(O._pfc(HW=15), divisor=16),
    "pool_fc HW=49: divisor 32": lambda: _pfc(O._pfc(HW=49), divisor=32),
    "pool_fc: pooled mean rounded to bf16": lambda: _pfc(O._pfc(C=512), mean_bf16=True),
    "pool_fc pooled input: means rounded to bf16": lambda: _pfc(O._pfc(C=160, HW=49, pooled=True), mean_bf16=True),
    "preprocess: truncation instead of RNE": lambda: _trunc("f32-c3-p8"),
    "preprocess u8: truncation instead of RNE": lambda: _trunc("u8c3-allbytes"),
    "preprocess: constants of the neighbouring channel": lambda: _pre("f32-c3-p8", channel_shift=1),
    "preprocess u8: channels in BGR order": lambda: _pre("u8c3-1024px", bgr=True),
    "pack_conv: K order (s, r, c)": lambda: _pack("stem-like", korder="src"),
    "pack_conv: fragment lane row*4 + kc": lambda: _pack("bias-only", lane_fault=True),
    "pack_conv: truncation instead of RNE": lambda: _pack("small-k", trunc=True),
    "pack_conv: fp32 sqrt in the BN scale": lambda: _pack("bn-bias", sqrt32=True),
    "pack_conv: fused multiply-add in the bias": lambda: _pack("bn-bias", fma_bias=True),
    "frag_pack: fragment lane row*4 + kc": _frag_lane,
    "one guard element overwritten": _guard,
}


@pytest.mark.parametrize("fault", list(FAULTS))
def test_comparator_rejects_planted_fault(fault):
    rep, _ = FAULTS[fault]()
    assert not rep.ok and rep.bad >= 1, (fault, O.describe(rep))


def test_fold_faults_differ_where_claimed():
    for name, (_, _, _, _, _, _, _, bn, _) in O.PACK_CASES.items():
        if not bn:
            continue
        w, (gamma, beta, mean, var), bias_in = O.pack_inputs(name)
        assert O.bn_scale(gamma, var, 1e-5)[1] != O.bn_scale(gamma, var, 1e-5, True)[1], name
        _, b = O.pack_ref(name)
        _, bf = O.pack_ref(name, fma_bias=True)
        assert b[4] != bf[4] and np.isfinite(b).all(), name


def test_fault_table_prints():
    print()
    for name, fn in FAULTS.items():
        rep, old = fn()
        oldtxt = "-" if old is None else "%.2e %s" % (old, "passes" if old < 1e-2 else "fails")
        print("| %s | %.3g | %d | %s |" % (name, rep.ratio, rep.bad, oldtxt))
