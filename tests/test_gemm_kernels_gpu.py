"""The LDS-tiled kernel of csrc/gemm.hip (``gemm_lds_kernel``, the product build), launched alone on MI355X
and judged against the fp64 oracle of tests/gemm_oracle.py, element by element under the derived bound with
random operands and bit for bit with integer-valued ones:

* GEMM mode on all 25 tiles of ``LDS_TILES``: M in {64, BM + 9, 577}, K = 64 .. 320 (1 to 5 stages' worth,
  around NS - 1), N in {4, 132, one full plus one partial tile} as ``lds_fits`` allows, ``ldx = K + 8`` and
  ``ldo = N + 8`` with NaN guard columns, residual, the four activations, fp32 output;
* CV mode (implicit-GEMM conv) on all 14 ``LDS_CONV_CFGS``, launched directly at M far below the heuristic's
  limit, bitwise equal to the register-ring kernel on the exact cases;
* ``HIPZAP_GEMM_GROUP`` = 1 and 3 (child processes) bitwise equal to the default raster;
* the launcher's refusals;
* the debug library (``HIPZAP_DEBUG=1``, a child process) on the exact cases of both kernels' tables: no
  contract failure, outputs bitwise those of the release library.

The folded-LayerNorm epilogue is an experiment and not part of the product library: not covered."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

import gemm_launch as GL
import gemm_oracle as G
from hipzap import _native as N
from hipzap.ops import conv as CV

pytestmark = pytest.mark.gpu
DEV = GL.DEV
ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("cfg", sorted(CV.LDS_TILES))
def test_lds_gemm_tile(cfg):
    cases = G.gemm_cases(cfg)
    widths = G.gemm_widths(cfg)
    assert len(widths) >= 2 and len(cases) == 3 * len(G.GEMM_K) * len(widths)  # nothing skipped
    ran = 0
    for i, case in enumerate(cases):
        assert CV.lds_fits(cfg, case.cout) and CV.lds_ok(case.M, case.K, True)
        for kind in GL.kinds_of(case):
            raw = GL.run(case, kind, cfg, 1, direct_lds=i % 2 == 0)  # hz_gemm_lds_launch itself / via hz_conv_launch
            GL.judge(case, kind, raw, f"{case.name}/{kind} cfg {cfg}", "lds-gemm")
            ran += 1
    assert ran >= len(cases)


@pytest.mark.parametrize("cfg", CV.LDS_CONV_CFGS)
def test_lds_conv_tile(cfg):
    cases = G.cv_cases(cfg)
    bn = CV.LDS_TILES[cfg][1]
    assert len(cases) == 2 * len(G._CV_GEOM) and {c.cout for c in cases} == {bn, 2 * bn}
    for i, case in enumerate(cases):
        for kind in GL.kinds_of(case):
            raw = GL.run(case, kind, cfg, 1, direct_lds=i % 2 == 1)
            GL.judge(case, kind, raw, f"{case.name}/{kind} cfg {cfg}", "lds-conv")
            if kind == "exact":  # the same bits as the register-ring kernel
                assert torch.equal(G.bits(raw), G.bits(GL.run(case, kind, 0, 1))), f"{case.name} cfg {cfg} vs ring"


def _child(sets, extra_env, timeout=240):
    """Digests of the raw outputs of ``sets`` from a fresh process with ``extra_env``."""
    env = dict(os.environ, HIPZAP_NO_AUTOBUILD="1", PYTHONPATH=str(ROOT))
    env.pop("HIPZAP_GEMM_GROUP", None)
    env.pop("HIPZAP_DEBUG", None)
    env.update(extra_env)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "gemm_launch.py"), *sets], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, f"child {extra_env} ended with {r.returncode}: {r.stderr[-3000:]}"
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def test_gemm_group_raster_is_bitwise_the_default():
    """``HIPZAP_GEMM_GROUP`` (docs/ENV.md) only changes which workgroup computes which tile. M = 577 gives 10,
    5 or 3 tile rows: the ``gsz`` tail of ``grouped_tile`` is taken at the default 8, at 3 and (trivially) at 1."""
    sets = ["gemm-tail"]
    base = GL.digests(sets) if "HIPZAP_GEMM_GROUP" not in os.environ else _child(sets, {})["digests"]
    assert len(base) >= 25 * len(G.GEMM_K) * 2
    for group in ("1", "3"):  # one after the other: a failed child ends the test before the next starts
        got = _child(sets, {"HIPZAP_GEMM_GROUP": group})
        assert not got["debug"] and got["digests"].keys() == base.keys()
        diff = [k for k in base if base[k] != got["digests"][k]]
        assert not diff, f"HIPZAP_GEMM_GROUP={group}: {len(diff)} outputs differ, first {diff[0]}"


def test_debug_library_on_the_exact_cases():
    """The ``HZ_DCHECK`` contracts at one-tile, partial-tile and short-K launches: none fires, and the checked
    kernels store the same bits as the release ones."""
    assert not N.DEBUG
    assert (ROOT / "hipzap" / "_lib" / "libhipzap_debug.so").exists(), "build it first: python -m hipzap.build --debug"
    sets = ["ring-exact", "gemm-exact", "cv-exact"]
    got = _child(sets, {"HIPZAP_DEBUG": "1"})
    assert got["debug"] and got["kcheck"] == [], got["kcheck"]
    base = GL.digests(sets)
    assert len(base) > 500 and got["digests"].keys() == base.keys()
    diff = [k for k in base if base[k] != got["digests"][k]]
    assert not diff, f"debug library: {len(diff)} outputs differ from the release library, first {diff[0]}"


# ------------------------------------------------------------------------------------------------
def _refused(case, cfg, code, edit=None):
    out = G.new_out(case, DEV)
    prm, keep = GL.params(case, "exact", cfg, 1, out)
    if edit:
        for k, v in edit.items():
            setattr(prm, k, v)
    rc = GL.lds_launcher()(prm, cfg, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == code, (case.name, cfg, edit, rc, code)
    assert bool(out.isnan().all()), "a refused launch wrote its output"
    del keep


def test_gemm_lds_launch_refusals():
    g = G.gemm_case(64, 64, 132, 0)
    assert GL.run(g, "exact", 19, 1, direct_lds=True).isnan().sum() > 0  # accepted as it stands (guards stay NaN)
    _refused(next(c for c in G.XROW_CASES if c.name == "xrow-k96-n4"), 19, -1)       # K % 64
    for edit in (dict(ldx=76), dict(Cout=130), dict(out_rowmajor=0), dict(ksteps=3), dict(K=96, ksteps=3)):
        _refused(g, 19, -1, edit)
    for cfg in (34, 35, 36, 37, 38, 39, 40):  # BN = 96 / 192 / 288 on a width lds_fits rejects
        n = next(n for n in (4, 100, 132) if not CV.lds_fits(cfg, n))
        _refused(G.gemm_case(64, 64, n, 0), cfg, -4)
    cv1 = next(c for c in G.CV_CASES if c.name == "cv-1x1-5x7-n3-co64")
    cv3 = next(c for c in G.CV_CASES if c.name == "cv-3x3-5x7-n3-co64")
    for cfg in list(range(9, 16)) + [41, 0]:
        _refused(g, cfg, -2)
        _refused(cv3, cfg, -2)
    for cfg in (24, 34, 25, 35, 40):            # GEMM-only tiles do not run CV
        _refused(cv3, cfg, -2)
    _refused(cv1, 19, -1, dict(C=32, R=1, S=2))   # C % 64 (K = R S C = 64 still)
    _refused(cv3, 19, -1, dict(out_rowmajor=1))
    _refused(cv3, 16, -1)                         # Cout = 64 on a BN = 128 tile
    _refused(cv3, 19, -1, dict(K=512, ksteps=16))  # K != R S C
    # an input of 2**31 bytes, by its parameters alone (nothing that large is allocated; nothing runs)
    _refused(cv1, 19, -1, dict(N=1, H=4096, W=4096, P=4096, Q=4096, M=4096 * 4096))


def test_zz_worst_ratios():
    """Prints the worst error / bound per kernel family seen by this module (profiles/gemm_oracle/README.md)."""
    for fam, (ratio, label) in sorted(GL.WORST.items()):
        print(f"\nWORST {fam}: {ratio:.3f} ({label})")
        assert ratio <= 1.0
