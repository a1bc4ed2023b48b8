"""The register-ring implicit-GEMM kernel of csrc/conv.hip (``conv_kernel``, ``conv2_kernel``), launched
alone on MI355X through ``make_params`` and judged against the fp64 oracle of tests/gemm_oracle.py:

* with random operands element by element under the derived bound
  ``|got - ref| <= r_out + L C_ACC 2**-24 A + C_FN 2**-24 |ref|``,
* with integer-valued operands bit for bit (every partial sum is exact in fp32, whatever the order),

on every one of the 9 tiles with every ``kw`` that ``legal`` allows, over the six instantiations (FAST 1x1,
FAST general, generic C = 8 / 16, XROW, F32IN 1x1, F32IN 3x3). Outputs are NaN-filled with guard rows (and
guard columns where ``ldo > Cout``): an element nobody wrote fails, and so does a write outside the live part.
The inputs and references are those tests/test_gemm_oracle_cpu.py judges on the CPU."""
import pytest
import torch

import gemm_launch as GL
import gemm_oracle as G
from hipzap import _native as N
from hipzap.ops import conv as CV

pytestmark = pytest.mark.gpu
DEV = GL.DEV
CONFIGS = G.ring_configs()
_ID = [f"cfg{c}-kw{k}" for c, k in CONFIGS]


@pytest.mark.parametrize("cfg,kw", CONFIGS, ids=_ID)
def test_ring_kernel_case_table(cfg, kw):
    """Every case of the table (all six instantiations) on this tile and K-split."""
    seen = set()
    for case in G.CONV_CASES + G.XROW_CASES:
        for kind in GL.kinds_of(case):
            label = f"{case.name}/{kind} cfg {cfg} kw {kw}"
            GL.judge(case, kind, GL.run(case, kind, cfg, kw), label)
            seen.add(case.inst)
    assert seen == {"fast1x1", "fast", "generic", "xrow", "f32in1x1", "f32in3x3"}


@pytest.mark.parametrize("cfg,kw", CONFIGS, ids=_ID)
def test_ring_kernel_kstep_counts(cfg, kw):
    """ksteps in {1, 2, kw - 1, kw, kw + 1, DEPTH, DEPTH + 1, 2 DEPTH + 3}: waves with no K step at all, a
    ring that never fills, one that wraps."""
    ks = G.ksteps_of_interest(cfg, kw)
    assert len(ks) >= 4 and 2 * G.ring_depth(cfg) + 3 in ks
    for k in ks:
        case = G.KSTEP_CASES[k]
        assert case.ksteps == k
        for kind in GL.kinds_of(case):
            GL.judge(case, kind, GL.run(case, kind, cfg, kw), f"{case.name}/{kind} cfg {cfg} kw {kw}", "ksteps")


def _by_name(name):
    return next(c for c in G.RING_CASES if c.name == name)


# conv2: the pair takes the 1x1, the general and the generic kernel; unequal grids
PAIRS = [("c96-blocked", "pix1"), ("1x1s2-6x9", "3x3-7x5-n3"), ("pix1", "3x3s2-7x5-n3"), ("7x7s2-c8", "1x3-c8")]


@pytest.mark.parametrize("cfg,kw", [(0, 4), (4, 2), (8, 1)], ids=["cfg0-kw4", "cfg4-kw2", "cfg8-kw1"])
@pytest.mark.parametrize("pair", PAIRS, ids=["+".join(p) for p in PAIRS])
def test_conv2_halves_equal_single_launches(pair, cfg, kw):
    a, b = _by_name(pair[0]), _by_name(pair[1])
    fc, fp = CV.TILES[cfg]
    grid = lambda c: -(-c.cout // (16 * fc)) * -(-c.M // (16 * fp))  # noqa: E731
    assert grid(a) != grid(b)
    for kind in G.KINDS:
        oa, ob = GL.run2(a, b, kind, cfg, kw)
        for case, raw in ((a, oa), (b, ob)):
            label = f"conv2 {pair} {case.name}/{kind} cfg {cfg} kw {kw}"
            one = GL.run(case, kind, cfg, kw)
            assert torch.equal(G.bits(raw), G.bits(one)), label
            if kind in GL.kinds_of(case):
                GL.judge(case, kind, raw, label, "conv2")


def _zinit(n, z_c, z_hw):
    g = torch.Generator().manual_seed(7)
    zb = (torch.randn(z_c, generator=g) * 3).to(DEV)
    z = torch.full((n * z_c * z_hw + 64,), float("nan"), device=DEV)
    want = (torch.round(zb.cpu() * 1024.0) * (1.0 / 1024.0))  # hz_fixq (common.h line 88)
    want = want.reshape(1, z_c // 32, 1, 32).expand(n, z_c // 32, z_hw, 32).reshape(-1)
    return zb, z, want


def _check_z(z, want, label):
    z = z.cpu()
    assert torch.equal(G.bits(z[:want.numel()]), G.bits(want.contiguous())), label
    assert bool((G.bits(z[want.numel():]) == G.NAN16 << 16).all()), f"{label}: zinit guard written"


@pytest.mark.parametrize("cfg,kw", [(0, 1), (1, 8), (8, 1)], ids=["cfg0-kw1", "cfg1-kw8", "cfg8-kw1"])
def test_zinit_is_fixq_of_zbias(cfg, kw):
    """``HzConvParams.zinit``: after a conv, and after a conv2 pair, the preset accumulator holds
    ``hz_fixq(zbias[c])`` bit for bit, nothing behind it is written, and the conv's own output is unchanged."""
    case = _by_name("3x3-5x7-n3")
    z_c, z_hw = 64, 35
    zb, z, want = _zinit(case.n, z_c, z_hw)

    def tw(prm, *_):
        prm.zinit, prm.zbias, prm.z_C, prm.z_HW = z.data_ptr(), zb.data_ptr(), z_c, z_hw

    raw = GL.run(case, "exact", cfg, kw, tweak=tw)
    _check_z(z, want, f"zinit conv cfg {cfg} kw {kw}")
    assert torch.equal(G.bits(raw), G.bits(GL.run(case, "exact", cfg, kw)))
    GL.judge(case, "exact", raw, "zinit conv")
    z.fill_(float("nan"))
    other = _by_name("1x1s2-6x9")
    oa, ob = GL.run2(case, other, "exact", cfg, kw, tweak=tw)
    _check_z(z, want, f"zinit conv2 cfg {cfg} kw {kw}")
    GL.judge(case, "exact", oa, "zinit conv2 a")
    GL.judge(other, "exact", ob, "zinit conv2 b")


# ------------------------------------------------------------------------------------------------
# refusals: a return code, and nothing runs
def _base(case, cfg=0, kw=1):
    out = G.new_out(case, DEV)
    prm, keep = GL.params(case, "exact", cfg, kw, out)
    return prm, out, keep


def _refused(launch, prm_edit, case, code, cfg=0, kw=1):
    prm, out, keep = _base(case, cfg, kw)
    prm_edit(prm)
    rc = launch(prm, cfg)
    torch.cuda.synchronize()
    assert rc == code, (rc, code)
    assert bool(out.isnan().all()), "a refused launch wrote its output"
    del keep


def _set(**kv):
    def edit(prm):
        for k, v in kv.items():
            setattr(prm, k, v)
    return edit


def test_conv_launch_refusals():
    lib = N.lib()
    launch = lambda prm, cfg: lib.hz_conv_launch(prm, cfg, N.stream_ptr())  # noqa: E731
    blocked, rowm, xrow = _by_name("3x3-5x7-n3"), _by_name("c40-rowmajor"), _by_name("xrow-relu")
    prm, out, keep = _base(blocked)
    assert launch(prm, 0) == 0  # the unedited parameters are accepted
    torch.cuda.synchronize()
    for case, edit in [(rowm, _set(Cout=38)), (blocked, _set(C=60)), (blocked, _set(C=24)), (blocked, _set(C=40)),
                       (xrow, _set(R=3, S=3)), (xrow, _set(ldx=44)), (blocked, _set(Cout=40)),
                       (blocked, _set(ksteps=17)), (blocked, _set(x_f32=1, C=8))]:
        _refused(launch, edit, case, -1)
    for cfg in range(9):  # every illegal (cfg, kw)
        for kw in range(2, 34):
            if not CV.legal(cfg, kw):
                _refused(launch, _set(kw=kw), blocked, -5, cfg, kw)
    for cfg in list(range(9, 16)) + [41]:
        _refused(launch, _set(), blocked, -2, cfg)
        _refused(launch, _set(), _by_name("xrow-m1"), -2, cfg)  # (K = 64: cfg 41 gets as far as the tile switch)
    # the LDS tiles reached through hz_conv_launch: never with an fp32 input or a zinit preset
    cv = G.CV_CASES[0]
    _refused(launch, _set(x_f32=1), cv, -1, 19)
    _refused(launch, _set(zinit=out.data_ptr(), zbias=out.data_ptr(), z_C=64, z_HW=35), cv, -1, 19)


def test_conv2_launch_refusals():
    lib = N.lib()
    a, b = _by_name("3x3-5x7-n3"), _by_name("1x1s2-6x9")

    def attempt(edit, code, cfg=0, kw=1):
        oa, ob = G.new_out(a, DEV), G.new_out(b, DEV)
        pa, ka = GL.params(a, "exact", cfg, kw, oa)
        pb, kb = GL.params(b, "exact", cfg, kw, ob)
        edit(pa, pb)
        rc = lib.hz_conv2_launch(pa, pb, cfg, N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == code, (rc, code)
        assert bool(oa.isnan().all()) and bool(ob.isnan().all())

    attempt(lambda pa, pb: setattr(pb, "kw", 2), -5)                       # unequal kw
    attempt(lambda pa, pb: setattr(pa, "kw", 4), -5, kw=2)
    z = torch.zeros(64, device=DEV)
    attempt(lambda pa, pb: [setattr(pb, k, v) for k, v in
                            dict(zinit=z.data_ptr(), zbias=z.data_ptr(), z_C=32, z_HW=1).items()], -1)
    attempt(lambda pa, pb: setattr(pb, "x_f32", 1), -1)
    attempt(lambda pa, pb: setattr(pb, "Cout", 98), -1)
    attempt(lambda pa, pb: setattr(pa, "C", 40), -1)
    attempt(lambda pa, pb: setattr(pa, "x_rowmajor", 1), -1)
    attempt(lambda pa, pb: setattr(pa, "ksteps", 3), -1)
    attempt(lambda pa, pb: None, -2, cfg=9)
    for cfg in range(9):
        for kw in range(2, 34):
            if not CV.legal(cfg, kw):
                attempt(lambda pa, pb: [setattr(pa, "kw", kw), setattr(pb, "kw", kw)], -5, cfg, kw)


def test_zz_worst_ratios():
    """Prints the worst error / bound per kernel family seen by this module (profiles/gemm_oracle/README.md)."""
    for fam, (ratio, label) in sorted(GL.WORST.items()):
        print(f"\nWORST {fam}: {ratio:.3f} ({label})")
        assert ratio <= 1.0
