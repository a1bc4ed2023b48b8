"""HZ_K_SEARCH_PQASSIGN (csrc/search.hip search_pqassign_kernel) against ``pq_assign_f32``, its arithmetic in numpy
float32: codes and distances bit for bit, for every shape, N and case of ``search_pqenc_cases``."""
import numpy as np
import pytest
import torch

from hipzap import search as S
from hipzap.ops import search as OS

import search_pqenc_cases as P
from search_pqenc_cases import T, u32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x5A5A5A5A5A5A5A5A
PLANT = 0xA7  # what the code rows hold before the launch: bytes M .. ldc-1 must keep it
NEVER = 7.0   # what the distances hold before the launch


def guarded(nbytes):
    """A device buffer of ``nbytes`` (a multiple of 16) between two 16-B guard regions -> (all of it as int64, the
    payload as uint8)."""
    buf = torch.full((nbytes // 8 + 4,), GUARD, dtype=torch.int64, device=DEV)
    return buf, buf[2:-2].view(torch.uint8)


def intact(buf):
    g = buf.cpu().numpy()
    return bool((g[:2] == GUARD).all() and (g[-2:] == GUARD).all())


def assign(rows32, cb, N=None, D=None, M=None, ldr=None, ldc=None, want_dist=True, tweak=None, replays=1, via_table=False):
    """One launch over device copies -> (rc, codes uint8 [n, M], dist fp32 [n, M] or None, ok): ``ok`` says that the
    guards around both outputs are intact and that the pitch bytes of the code rows kept ``PLANT``; with ``replays``
    the outputs of every launch."""
    n, d = rows32.shape
    m = cb.shape[0]
    ldr, ldc = ldr or d, ldc or m
    host = np.full((n, max(ldr, d)), 0x7FC0, np.uint16)  # the pitch of a row holds NaN: never read
    host[:, :d] = S.to_bf16(rows32)
    rd = torch.from_numpy(host.view(np.int16)).to(DEV)
    cd = torch.from_numpy(np.array(cb, np.float32)).to(DEV)  # a copy: the shared case is read-only
    cbuf, cpay = guarded(n * max(ldc, m) + (-(n * max(ldc, m))) % 16)
    dbuf, dpay = guarded(n * m * 4 + (-(n * m * 4)) % 16)
    p = OS.PqAssignParams(rd.data_ptr(), cd.data_ptr(), cpay.data_ptr(), dpay.data_ptr() if want_dist else 0,
                          n * m * 4 if want_dist else 0, n if N is None else N, d if D is None else D,
                          m if M is None else M, ldr, ldc)
    if tweak:
        tweak(p)
    outs = []
    for _ in range(replays):
        cpay.fill_(PLANT)
        dpay.view(torch.float32).fill_(NEVER)
        if via_table:
            import ctypes as C
            from hipzap import _native as N_
            rc = N_.lib().hz_launch_kernel(N_.HZ_K_SEARCH_PQASSIGN, C.byref(p), torch.cuda.current_stream().cuda_stream)
        else:
            rc = OS.launch_pq_assign(p, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        c = cpay.cpu().numpy()[:n * max(ldc, m)].reshape(n, max(ldc, m))
        dist = dpay.view(torch.float32).cpu().numpy()[:n * m].reshape(n, m).copy()
        outs.append((c[:, :m].copy(), dist, bool((c[:, m:] == PLANT).all())))
    ok = intact(cbuf) and intact(dbuf) and all(o[2] for o in outs)
    if replays > 1:
        return rc, outs, ok
    return rc, outs[0][0], (outs[0][1] if want_dist else None), ok and (want_dist or bool((outs[0][1] == NEVER).all()))


def same(codes, dist, want):
    return np.array_equal(codes, want[0]) and (dist is None or np.array_equal(u32(dist), u32(want[1])))


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("D,M", P.SHAPES)
def test_codes_and_distances_equal_the_float32_oracle_bit_for_bit(D, M, kind):
    for N in P.NS:
        rows, cb = P.make(kind, N, D, M)
        want = P.ref(kind, N, D, M)
        rc, codes, dist, ok = assign(rows, cb)
        assert rc == 0 and ok and same(codes, dist, want), (N, "codes and dist")
        rc, codes, dist, ok = assign(rows, cb, want_dist=False)  # dist null: the same codes, no distance written
        assert rc == 0 and ok and dist is None and same(codes, None, want), (N, "dist null")
        rc, codes, dist, ok = assign(rows, cb, ldr=D + 8, ldc=M + 16)  # padded pitches
        assert rc == 0 and ok and same(codes, dist, want), (N, "padded pitches")


def test_a_rows_bits_do_not_depend_on_placement_or_replay():
    for D, M in ((768, 96), (48, 16), (1024, 16)):
        rows, cb = P.make("neartie", P.NMAX, D, M)
        wc, wd = P.ref("neartie", P.NMAX, D, M)
        one = 2 * T + 77  # a row of the full case ...
        seen = set()
        for N, at in ((1, 0), (T + 1, 0), (T + 1, T), (3 * T + 5, 3 * T + 4), (3 * T + 5, 2 * T - 1)):
            r = rows[:N].copy()
            r[at] = rows[one]  # ... alone, at position 0, in the last partial tile, at a tile's last row
            rc, codes, dist, ok = assign(r, cb)
            assert rc == 0 and ok and np.array_equal(codes[at], wc[one]), (D, M, N, at)
            seen.add(u32(dist[at]).tobytes())
        assert seen == {u32(wd[one]).tobytes()}
        rc, outs, ok = assign(rows, cb, replays=20)
        assert rc == 0 and ok
        for codes, dist, _ in outs:
            assert same(codes, dist, (wc, wd))


def test_a_nan_never_displaces_and_an_all_nan_column_gives_code_zero():
    rows, cb = P.make("inexact", T + 1, 128, 16)
    rows, cb = rows.copy(), cb.copy()
    cb[0, 0] = np.nan        # sub-space 0: the walk starts on a NaN and nothing is below it
    cb[1, 5] = np.nan        # sub-space 1: a NaN in the middle is never chosen
    cb[2, :, 3] = np.nan     # sub-space 2: every distance is NaN
    rows[7, 24:32] = np.inf  # row 7, sub-space 3: inf - finite = inf everywhere: no value is below the first
    want = S.pq_assign_f32(rows, cb)
    assert (want[0][:, 0] == 0).all() and (want[0][:, 1] != 5).all() and (want[0][:, 2] == 0).all() and want[0][7, 3] == 0
    rc, codes, dist, ok = assign(rows, cb)
    assert rc == 0 and ok and np.array_equal(codes, want[0])
    assert np.array_equal(np.isnan(dist), np.isnan(want[1])) and np.array_equal(u32(dist)[~np.isnan(dist)], u32(want[1])[~np.isnan(dist)])


def test_the_launcher_refuses_misuse_without_launching():
    rows, cb = P.make("integer", 40, 128, 16)
    seen = {}

    def refused(what, code, **kw):
        rc, codes, dist, ok = assign(rows, cb, **kw)
        assert rc == code, (what, rc)
        assert (codes == PLANT).all() and (dist is None or (dist == NEVER).all()) and ok, what  # nothing ran
        seen[what] = rc

    for field in ("rows", "codebook", "codes"):
        refused(field + " null", -129, tweak=lambda p, f=field: setattr(p, f, 0))
    refused("D % M", -130, D=120)
    refused("M % 16", -131, M=24, D=120)
    refused("M < 16", -132, M=0)
    refused("M > 96", -132, M=112, D=224, ldc=112)
    refused("dsub > 64", -133, D=16 * 65, tweak=lambda p: setattr(p, "ldr", 16 * 65))
    refused("D > 2048", -134, D=2064, M=48, ldc=48, tweak=lambda p: setattr(p, "ldr", 2064))
    refused("ldr < D", -135, tweak=lambda p: setattr(p, "ldr", 120))
    refused("ldr % 8", -135, tweak=lambda p: setattr(p, "ldr", 132))
    refused("ldc < M", -136, tweak=lambda p: setattr(p, "ldc", 0))
    refused("ldc % 16", -136, tweak=lambda p: setattr(p, "ldc", 24))
    refused("N = 0", -137, N=0)
    refused("N < 0", -137, N=-5)
    refused("rows misaligned", -138, tweak=lambda p: setattr(p, "rows", p.rows + 8))
    refused("codebook misaligned", -138, tweak=lambda p: setattr(p, "codebook", p.codebook + 4))
    refused("codes misaligned", -138, tweak=lambda p: setattr(p, "codes", p.codes + 8))
    refused("dist misaligned", -138, tweak=lambda p: setattr(p, "dist", p.dist + 4))
    refused("short dist", -139, tweak=lambda p: setattr(p, "dist_bytes", p.dist_bytes - 4))
    assert set(seen.values()) == set(range(-139, -128))  # all eleven codes
    rc, codes, dist, ok = assign(rows, cb)  # and the same buffers are accepted
    assert rc == 0 and ok and same(codes, dist, P.ref("integer", 40, 128, 16))


def test_the_kind_launches_through_the_table():
    rows, cb = P.make("inexact", T + 1, 128, 16)
    rc, codes, dist, ok = assign(rows, cb, via_table=True)
    assert rc == 0 and ok and same(codes, dist, P.ref("inexact", T + 1, 128, 16))


DEBUG_CHILD = """
import sys
sys.path.insert(0, "tests")
from hipzap.utils import kcheck
import search_pqenc_cases as P
import test_search_pqenc_gpu as G
assert kcheck.enabled()
for D, M in P.SHAPES:
    for N in P.NS:
        rows, cb = P.make("inexact", N, D, M)
        want = P.ref("inexact", N, D, M)
        for kw in ({}, {"want_dist": False}, {"ldr": D + 8, "ldc": M + 16}):
            rc, codes, dist, ok = G.assign(rows, cb, **kw)
            assert rc == 0 and ok and G.same(codes, dist, want), (D, M, N, kw, rc)
fails = kcheck.poll()
assert fails == [], fails
print("silent")
"""


def test_the_debug_library_checks_stay_silent():
    """The HZ_DCHECK unit of search.hip guards the kernel's codebook staging range, its row loads (row < N) and its code
    and distance stores: the debug library (a child process: HIPZAP_DEBUG selects the library at import) runs every
    shape at every N with the right answers and no record."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(os.path.join(root, "hipzap", "_lib", "libhipzap_debug.so")), "python -m hipzap.build --debug"
    env = dict(os.environ, HIPZAP_DEBUG="1", HIPZAP_NO_AUTOBUILD="1")
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "silent" in r.stdout, r.stderr[-4000:]
