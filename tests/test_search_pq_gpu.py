"""The product-quantisation kernels (csrc/search.hip): HZ_K_SEARCH_PQLUT against the fp64 table within the fmaf chain's
bound, and HZ_K_SEARCH_PQSCAN + the existing merge against ``search_pq_cases.scan_ref`` -- the device's own table read
back, summed by ``pq_scores_from_lut`` -- bit for bit."""
import numpy as np
import pytest
import torch

from hipzap import search as S
from hipzap.ops import search as OS

import search_pq_cases as P
from search_pq_cases import T, u32

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x5A5A5A5A5A5A5A5A
FILL = 0xFF  # what dead rows and the pitch padding hold


def dev(a, dt=np.int32):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(DEV)


def table(q, cb, Q=None, D=None, M=None, tweak=None):
    """HZ_K_SEARCH_PQLUT over device copies -> (rc, table fp32 [Q, M, 256], guards intact, the device buffers)."""
    m, _, dsub = cb.shape
    Qn = q.shape[0] if Q is None else Q
    qd, cd = dev(q), dev(cb)
    words = max(q.shape[0], 1) * m * 256
    buf = torch.full((words // 2 + 4,), GUARD, dtype=torch.int64, device=DEV)  # two guard words on each side
    lut = buf[2:-2].view(torch.float32)
    lut.fill_(7.0)  # "never written"
    p = OS.PqLutParams(qd.data_ptr(), cd.data_ptr(), lut.data_ptr(), words * 4, m * dsub if D is None else D,
                       m if M is None else M, Qn, 0)
    if tweak:
        tweak(p)
    rc = OS.launch_pq_lut(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g = buf.cpu().numpy()
    intact = bool((g[:2] == GUARD).all() and (g[-2:] == GUARD).all())
    return rc, lut.cpu().numpy().reshape(max(q.shape[0], 1), m, 256).copy(), intact, (qd, cd, buf, lut)


def scan(codes, cb, q, k, live=None, tags=None, filt=None, N=None, D=None, Q=None, M=None, ldc=None, span=0, tweak=None,
         fill=FILL, replays=1):
    """Table, scan and merge over device copies -> (scan rc, merge rc, scores [Q, k], ids [Q, k], the device's table,
    guards intact). Dead rows and the bytes from M to the pitch's end hold ``fill``; ``cand`` and the table lie
    between guard words."""
    n, m = codes.shape
    dsub = cb.shape[2]
    live = np.ones(n, bool) if live is None else np.asarray(live, bool)
    ldc = ldc or m
    host = np.full((n, max(ldc, m)), fill, np.uint8)
    host[:, :m] = codes
    host[~live] = fill
    rc, lut, lut_ok, (qd, cd, lbuf, ld) = table(q, cb)
    assert rc == 0 and lut_ok
    corpus = torch.from_numpy(host).to(DEV)
    Qn = q.shape[0] if Q is None else Q
    nbytes = max(OS.scratch_bytes(n, min(max(Qn, 1), 16), min(max(k, 1), 128)), 8)
    buf = torch.full((nbytes // 8 + 4,), GUARD, dtype=torch.int64, device=DEV)
    cand = buf[2:-2]
    cand.zero_()
    sc = torch.full((max(Qn, 1), max(k, 1)), 7.0, dtype=torch.float32, device=DEV)  # 7 / -7: "never written"
    ids = torch.full((max(Qn, 1), max(k, 1)), -7, dtype=torch.int32, device=DEV)
    lw = S.pack_live(live)
    lv = dev(lw)
    tg = None if tags is None else dev(np.ascontiguousarray(tags, np.uint32))
    fl = None if filt is None else dev(np.ascontiguousarray(filt, np.uint32).reshape(-1, 2))
    p = OS.PqScanParams(corpus.data_ptr(), qd.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(),
                        n if N is None else N, m * dsub if D is None else D, Qn, k, ldc, 0, nbytes, lv.data_ptr(),
                        0 if tg is None else tg.data_ptr(), 0 if fl is None else fl.data_ptr(), lw.size * 4,
                        ld.data_ptr(), q.shape[0] * m * 1024, m if M is None else M, span)
    if tweak:
        tweak(p)
    outs = []
    for _ in range(replays):
        rc = OS.launch_pq(p, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append((sc.cpu().numpy().copy(), ids.cpu().numpy().copy()))
    g, gl = buf.cpu().numpy(), lbuf.cpu().numpy()
    intact = bool((g[:2] == GUARD).all() and (g[-2:] == GUARD).all() and (gl[:2] == GUARD).all() and (gl[-2:] == GUARD).all())
    if replays > 1:
        return rc[0], rc[1], outs, lut, intact
    return rc[0], rc[1], outs[0][0], outs[0][1], lut, intact


def check(codes, k, allow, sc, ids, lut):
    assert np.array_equal(P.keys_of(sc, ids), P.scan_ref(lut, codes, k, allow)), "keys differ from pq_scores_from_lut"
    assert (sc[ids < 0] == -np.inf).all()


# ------------------------------------------------------------------------------------------------ table
@pytest.mark.parametrize("Q", [1, 3, 16])
@pytest.mark.parametrize("D,M", P.SHAPES)
def test_every_table_entry_is_within_the_chain_bound(D, M, Q):
    _, cb, q = P.make("inexact", 1, D, M, Q)
    rc, lut, intact, _ = table(q, cb)
    assert rc == 0 and intact
    want, bound = P.lut_oracle(q, cb)
    err = np.abs(lut.astype(np.float64) - want)
    print(f"D={D} M={M} Q={Q}: worst error / bound = {(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all()
    for kind in ("integer", "lossless"):
        _, cb, q = P.make(kind, 1, D, M, Q)
        rc, lut, intact, _ = table(q, cb)
        assert rc == 0 and intact and np.array_equal(lut.astype(np.float64), P.lut_oracle(q, cb)[0])  # exact


# ------------------------------------------------------------------------------------ scan + merge
NS = [1, T - 1, T, T + 1, 2 * T + 5, 3 * T + 5]


@pytest.mark.parametrize("pitch", [0, 16])
@pytest.mark.parametrize("N", NS)
def test_keys_equal_the_table_sum_bit_for_bit(N, pitch):
    for (D, M), k in zip(((768, 96), (768, 48), (128, 16)), (1, 10, 128)):
        codes, cb, q = P.make("inexact", N, D, M, 3, salt=N)
        rs, rm, sc, ids, lut, intact = scan(codes, cb, q, k, ldc=M + pitch)
        assert (rs, rm) == (0, 0) and intact, (D, M, k)
        check(codes, k, None, sc, ids, lut)
        s, b = P.score_oracle(codes, cb, q)  # and the contract's bound against the reconstructed rows
        got = np.take_along_axis(s, np.maximum(ids, 0).astype(np.int64), axis=1)
        bnd = np.take_along_axis(b, np.maximum(ids, 0).astype(np.int64), axis=1)
        assert (np.abs(sc.astype(np.float64) - got)[ids >= 0] <= bnd[ids >= 0]).all()


@pytest.mark.parametrize("M", [16, 32, 48, 64, 80, 96])
def test_every_m_bucket_and_the_integer_case_with_its_ties(M):
    D = 2 * M
    codes, cb, q = P.make("integer", 2 * T + 5, D, M, 16)
    rs, rm, sc, ids, lut, intact = scan(codes, cb, q, 128)
    assert (rs, rm) == (0, 0) and intact
    check(codes, 128, None, sc, ids, lut)
    assert np.array_equal(lut.astype(np.float64), P.lut_oracle(q, cb)[0])
    ws, wi = S.pq_search_ref(codes, cb, q, 128)  # exact arithmetic: the fp64 oracle's answer, ties by id
    assert np.array_equal(ids, wi) and np.array_equal(sc.astype(np.float64), ws)
    same = sc[:, 1:] == sc[:, :-1]
    assert same.sum() > 100 and (np.diff(ids, axis=1)[same] > 0).all()


def test_lossless_ids_equal_exact_search_over_the_rows():
    for D, M in ((768, 96), (2048, 32), (64, 16)):
        codes, cb, q = P.make("lossless", 3 * T + 5, D, M, 4)
        rows = S.pq_decode(codes, cb)
        rs, rm, sc, ids, lut, intact = scan(S.pq_encode(rows, cb), cb, q, 10)
        assert (rs, rm) == (0, 0) and intact
        ws, wi = S.search_ref(rows, q, 10)
        assert np.array_equal(ids, wi) and np.array_equal(sc.astype(np.float64), ws)


def test_identical_rows_come_back_in_id_order():
    codes, cb, q = P.make("inexact", 1, 768, 96, 3)
    codes = np.repeat(codes, 700, axis=0)
    rs, rm, sc, ids, lut, intact = scan(codes, cb, q, 128)
    assert (rs, rm) == (0, 0) and intact
    assert np.array_equal(ids, np.tile(np.arange(128, dtype=np.int32), (3, 1)))
    assert all(len(set(u32(sc[qi]).tolist())) == 1 for qi in range(3))


def test_score_bits_do_not_depend_on_placement_span_or_replay():
    D, M = 768, 96
    codes, cb, q16 = P.make("inexact", 3 * T + 5, D, M, 16, salt=3)
    one = q16[5:6].copy()
    lut1 = table(one, cb)[1]
    best = np.argmax(lut1[0], axis=1).astype(np.uint8)  # the row that scores highest for this query
    want = S.pq_scores_from_lut(lut1[0], best[None, :])[0]
    seen = set()
    for N, at in ((1, 0), (T, T - 1), (T + 1, T), (3 * T + 5, 3 * T + 4), (3 * T + 5, 2)):
        c = codes[:N].copy()
        c[at] = best
        tags = (np.arange(N) % 3).astype(np.uint32)
        tags[at] = 2
        for Q, slot, k, filtered, span in ((1, 0, 1, False, 0), (16, 7, 128, True, 1), (16, 0, 10, False, 2), (16, 15, 1, True, 3),
                                            (16, 3, 10, False, 0)):
            qs = one if Q == 1 else q16.copy()
            qs[slot] = one[0]
            kw = {"tags": tags, "filt": np.tile(np.array([[3, 2]], np.uint32), (Q, 1))} if filtered else {}
            rs, rm, sc, ids, lut, intact = scan(c, cb, qs, k, span=span, **kw)
            assert (rs, rm) == (0, 0) and intact and ids[slot, 0] == at, (N, at, Q, slot, k, filtered, span)
            assert np.array_equal(u32(lut[slot]), u32(lut1[0]))  # the table's bits do not depend on the slot either
            seen.add(int(u32(sc)[slot, 0]))
    assert seen == {int(u32(want))}, seen
    base = None
    for span in (1, 2, 3, 0, 100):  # the whole answer, span by span
        rs, rm, sc, ids, lut, _ = scan(codes, cb, q16, 128, span=span)
        assert (rs, rm) == (0, 0)
        base = base or (u32(sc).copy(), ids.copy())
        assert np.array_equal(u32(sc), base[0]) and np.array_equal(ids, base[1]), span
    check(codes, 128, None, sc, ids, lut)
    rs, rm, outs, lut, intact = scan(codes, cb, q16, 128, replays=20)
    assert (rs, rm) == (0, 0) and intact
    for sc, ids in outs:
        assert np.array_equal(u32(sc), base[0]) and np.array_equal(ids, base[1])
    assert OS.pq_span(3 * T + 5, 16, M) >= 1 and OS.pq_span(0, 1, M) == 0 and OS.pq_span(T, 1, 24) == 0
    assert OS.pq_span(10 ** 6, 16, 96) > OS.pq_span(10 ** 6, 16, 48) == 3  # one workgroup per compute unit: long spans


def test_live_bitmaps_tag_predicates_dead_waves_and_no_passing_row():
    N, D, M, k = 2 * T + 60, 768, 48, 10
    codes, cb, q = P.make("inexact", N, D, M, 4, salt=9)
    tags = (np.arange(N) % 11).astype(np.uint32)
    filt = np.array([[0, 0], [0xFFFFFFFF, 99], [0xFFFFFFFF, 5], [4, 4]], np.uint32)  # all, none, tags == 5, bit 2 set
    patterns = {"every third dead": np.arange(N) % 3 != 0, "a dead wave": ~((np.arange(N) >= 64) & (np.arange(N) < 128)),
                "a dead tile": np.arange(N) >= T, "one live row": np.arange(N) == T + 3, "none": np.zeros(N, bool)}
    for name, live in patterns.items():
        for kw, allow in (({}, live), ({"tags": tags, "filt": filt}, live[None, :] & ((tags[None, :] & filt[:, :1]) == filt[:, 1:]))):
            base = scan(codes, cb, q, k, live, ldc=M + 16, **kw)
            assert base[:2] == (0, 0) and base[5], name
            check(codes, k, allow, base[2], base[3], base[4])
            other = scan(codes, cb, q, k, live, ldc=M + 16, fill=0, **kw)  # what dead rows and the padding hold changes no key
            assert np.array_equal(u32(base[2]), u32(other[2])) and np.array_equal(base[3], other[3]), name
        assert (base[3][1] == -1).all() and (base[2][1] == -np.inf).all()  # no passing row: sentinels
    assert (base[3] == -1).all()


def test_the_launchers_refuse_misuse_without_launching():
    codes, cb, q = P.make("integer", 40, 128, 16, 2)
    live, tags, filt = np.ones(40, bool), np.zeros(40, np.uint32), np.zeros((2, 2), np.uint32)
    seen = {}

    def refused(what, code, k=10, tags=tags, filt=filt, **kw):
        rs, rm, sc, ids, lut, intact = scan(codes, cb, q, k, live, tags, filt, **kw)
        assert rs == code and rm is None, (what, rs)
        assert (sc == 7.0).all() and (ids == -7).all() and intact, what  # nothing ran
        seen[what] = rs

    for field in ("corpus", "queries", "cand", "out_score", "out_id", "lut"):
        refused(field + " null", -112, tweak=lambda p, f=field: setattr(p, f, 0))
    refused("D % M", -113, D=120)
    refused("M % 16", -114, M=24)
    refused("M < 16", -115, M=0)
    refused("M > 96", -115, M=112, D=224, ldc=112)
    refused("dsub > 64", -116, D=16 * 65)
    refused("D > 2048", -117, D=2064, M=48, ldc=48)
    refused("ldc < M", -118, tweak=lambda p: setattr(p, "ldc", 0))
    refused("ldc % 16", -118, tweak=lambda p: setattr(p, "ldc", 24))
    refused("N = 0", -119, N=0)
    refused("N < 0", -119, N=-5)
    refused("Q = 0", -120, Q=0)
    refused("Q = 17", -120, Q=17)
    refused("k = 0", -121, k=0)
    refused("k = 129", -121, k=129)
    refused("corpus misaligned", -122, tweak=lambda p: setattr(p, "corpus", p.corpus + 8))
    refused("queries misaligned", -122, tweak=lambda p: setattr(p, "queries", p.queries + 4))
    refused("lut misaligned", -122, tweak=lambda p: setattr(p, "lut", p.lut + 8))
    refused("cand misaligned", -122, tweak=lambda p: setattr(p, "cand", p.cand + 4))
    refused("tags misaligned", -122, tweak=lambda p: setattr(p, "tags", p.tags + 2))
    refused("filt misaligned", -122, tweak=lambda p: setattr(p, "filt", p.filt + 2))
    refused("live misaligned", -122, tweak=lambda p: setattr(p, "live", p.live + 2))
    refused("live null", -123, tweak=lambda p: setattr(p, "live", 0))
    refused("short live", -124, tweak=lambda p: setattr(p, "live_bytes", 4))  # 40 rows need 2 words
    refused("filt without tags", -125, tags=None)
    refused("short cand", -126, tweak=lambda p: setattr(p, "cand_bytes", p.cand_bytes - 8))
    refused("short lut", -127, tweak=lambda p: setattr(p, "lut_bytes", p.lut_bytes - 4))
    refused("span < 0", -128, span=-1)
    assert set(seen.values()) == set(range(-128, -111))  # every code of the list is hit
    for what, code, kw in (("queries null", -112, dict(tweak=lambda p: setattr(p, "queries", 0))),
                           ("codebook null", -112, dict(tweak=lambda p: setattr(p, "codebook", 0))),
                           ("lut null", -112, dict(tweak=lambda p: setattr(p, "lut", 0))), ("D % M", -113, dict(D=120)),
                           ("M % 16", -114, dict(M=24)), ("M > 96", -115, dict(M=112, D=224)), ("dsub > 64", -116, dict(D=16 * 65)),
                           ("D > 2048", -117, dict(D=2064, M=48)), ("Q = 0", -120, dict(Q=0)), ("Q = 17", -120, dict(Q=17)),
                           ("codebook misaligned", -122, dict(tweak=lambda p: setattr(p, "codebook", p.codebook + 4))),
                           ("lut misaligned", -122, dict(tweak=lambda p: setattr(p, "lut", p.lut + 4))),
                           ("short lut", -127, dict(tweak=lambda p: setattr(p, "lut_bytes", p.lut_bytes - 4)))):
        rc, lut, intact, _ = table(q, cb, **kw)
        assert rc == code and (lut == 7.0).all() and intact, what
    rs, rm, sc, ids, lut, intact = scan(codes, cb, q, 10, live, tags, filt)  # and the same buffers are accepted
    assert (rs, rm) == (0, 0) and intact
    check(codes, 10, live, sc, ids, lut)


def test_the_kinds_launch_through_the_table():
    import ctypes as C
    from hipzap import _native as N
    lib = N.lib()
    _, cb, q = P.make("integer", 1, 128, 16, 2)
    rc, lut, intact, (qd, cd, buf, ld) = table(q, cb)
    ld.fill_(7.0)
    p = OS.PqLutParams(qd.data_ptr(), cd.data_ptr(), ld.data_ptr(), 2 * 16 * 1024, 128, 16, 2, 0)
    assert lib.hz_launch_kernel(N.HZ_K_SEARCH_PQLUT, C.byref(p), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(ld.cpu().numpy().reshape(2, 16, 256), lut)


DEBUG_CHILD = """
import sys
sys.path.insert(0, "tests")
import numpy as np
from hipzap.utils import kcheck
import search_pq_cases as P
import test_search_pq_gpu as G
assert kcheck.enabled()
T = P.T
for (D, M), k in zip(((768, 96), (768, 48), (128, 16)), (1, 10, 128)):
    for N in (1, T + 1, 3 * T + 5):
        codes, cb, q = P.make("inexact", N, D, M, 3, salt=N)
        for pitch, span in ((0, 0), (16, 2)):
            rs, rm, sc, ids, lut, intact = G.scan(codes, cb, q, k, ldc=M + pitch, span=span)
            assert (rs, rm) == (0, 0) and intact, (D, M, N, rs, rm)
            G.check(codes, k, None, sc, ids, lut)
codes, cb, q = P.make("inexact", 700, 768, 48, 4, salt=9)
tags = (np.arange(700) % 11).astype(np.uint32)
filt = np.array([[0, 0], [0xFFFFFFFF, 99], [0xFFFFFFFF, 5], [4, 4]], np.uint32)
for live in (np.arange(700) % 3 != 0, np.arange(700) >= T, np.zeros(700, bool)):
    rs, rm, sc, ids, lut, intact = G.scan(codes, cb, q, 10, live, tags, filt)
    assert (rs, rm) == (0, 0) and intact
    G.check(codes, 10, live[None, :] & ((tags[None, :] & filt[:, :1]) == filt[:, 1:]), sc, ids, lut)
fails = kcheck.poll()
assert fails == [], fails
print("silent")
"""


def test_the_debug_library_checks_stay_silent():
    """The HZ_DCHECK unit of search.hip guards the table's stores, the table copy, the tile range, the code loads
    (row < N), ``code < 256`` and the candidate writes of the two kernels: the debug library (a child process:
    HIPZAP_DEBUG selects the library at import) runs shapes of every kind with the right answers and no record."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(os.path.join(root, "hipzap", "_lib", "libhipzap_debug.so")), "python -m hipzap.build --debug"
    env = dict(os.environ, HIPZAP_DEBUG="1", HIPZAP_NO_AUTOBUILD="1")
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "silent" in r.stdout, r.stderr[-4000:]
