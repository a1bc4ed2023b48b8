"""The batch scan (csrc/search.hip, HZ_K_SEARCH_XSCAN), its merge (HZ_K_SEARCH_MERGEN over the same block) and the
rescore for any number of queries (HZ_K_SEARCH_RESCOREN) through ``hz_launch_kernel``, against the fp64 oracle over
the SPLIT queries (tests/search_batch_cases.py: bound and cases).

Scores: within ``beta(3D) * sum (|h'| + |m'| + |l'|) |r|`` of the fp64 score of the split query. Ids: equal to the
oracle's in every forced slot; tests/test_search_batch_cpu.py asserts on the host that at most 2 % of the slots of a
case are unforced. Wherever two GPU runs are compared, they are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from hipzap import _native as N
from hipzap import search as S
from hipzap.ops import search as OS

import search_batch_cases as F
from search_batch_cases import QB, T, make

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 3  # output rows past Q that must keep their canary


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def launch(bits, q, k, live, fill=None, tweak=None, want_cand=False):
    """Kinds 44 and 40 over device copies -> (scan rc, merge rc, scores [Q, k], ids [Q, k]) (+ the candidate keys).
    ``fill``: a uint16 pattern written over the dead rows first. The outputs have PAD rows past Q and the scratch PAD
    lists past its end, which must keep their canaries."""
    n, d = bits.shape
    host = bits.copy()
    if fill is not None:
        host[~np.asarray(live, bool)] = fill
    corpus = torch.from_numpy(host.view(np.int16)).to(DEV)
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV)
    Q = q.shape[0]
    nbytes = max(OS.self_scratch_bytes(n, Q, k), 8)
    cand = torch.full((nbytes // 8 + PAD * k,), -1, dtype=torch.int64, device=DEV)  # all ones: no valid list
    sc = torch.full((Q + PAD, k), 7.0, dtype=torch.float32, device=DEV)
    ids = torch.full((Q + PAD, k), -7, dtype=torch.int32, device=DEV)
    words = S.pack_live(live)
    lv = torch.from_numpy(words.view(np.int32)).to(DEV)
    p = OS.BatchScanParams(corpus.data_ptr(), qd.data_ptr(), lv.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(),
                           words.size * 4, nbytes, n, d, Q, k, d, 0)
    if tweak:
        tweak(p)
    st = torch.cuda.current_stream().cuda_stream
    lib = N.lib()
    rs = lib.hz_launch_kernel(N.HZ_K_SEARCH_XSCAN, C.byref(p), st)
    rm = lib.hz_launch_kernel(N.HZ_K_SEARCH_MERGEN, C.byref(p), st) if rs == 0 else None
    torch.cuda.synchronize()
    sch, idh, ch = sc.cpu().numpy(), ids.cpu().numpy(), cand.cpu().numpy()
    assert (sch[Q:] == 7.0).all() and (idh[Q:] == -7).all() and (ch[nbytes // 8:] == -1).all()  # the slots past Q
    if rs != 0:
        assert (sch == 7.0).all() and (idh == -7).all() and (ch == -1).all()  # refused: nothing ran
    out = (rs, rm, sch[:Q], idh[:Q])
    return out + (ch[:nbytes // 8].view(np.uint64).reshape(-1, Q, k),) if want_cand else out


@pytest.mark.parametrize("name", F.NAMES)
def test_the_batch_scan_matches_the_oracle_over_the_split_queries(name):
    bits, c32, q, k, live, kind = F.build_case(name)
    s, b, rs_, ri, forced = F.case_oracle(name)
    rs, rm, sc, ids = launch(bits, q, k, live)
    assert (rs, rm) == (0, 0)
    worst = F.check_against_oracle(sc, ids, s, b, rs_, ri, forced, live)
    print(f"{name}: unforced {int((~forced).sum())}/{forced.size}, worst |err|/bound {worst:.4f}")
    assert (~forced).mean() <= F.MAX_UNFORCED


def test_integer_cases_are_exact_bit_for_bit():
    """Queries that use all three split terms against rows of -1, 0, 1: every partial sum is an integer below 2^24."""
    bits, c32, q, dots = F.exact_case()
    n = bits.shape[0]
    live = np.ones(n, bool)
    h, m, l = S.split3(q)
    assert (h != 0).all() and (m != 0).all() and (l != 0).all()
    rs, rm, sc, ids = launch(bits, q, 128, live)
    assert (rs, rm) == (0, 0)
    for qi in range(q.shape[0]):
        want = dots[qi, ids[qi]].astype(np.float32) + np.float32(0.0)
        assert np.array_equal(u32(sc[qi]), u32(want)), qi
        order = np.lexsort((np.arange(n), -dots[qi]))[:128]  # exact scores: the order rule alone decides
        assert np.array_equal(ids[qi], order), qi


def test_the_bits_of_a_score_depend_on_the_query_and_the_row_only():
    """One pair (q, r): alone and in a full block, in slot 0 and slot 63 and past a block edge, the row in tile 0 and
    in the last partial tile, at k = 1 and k = 128, in a two-row corpus, and over 20 replays."""
    n, d = 300, 768
    bits, c32, qs = make(n, d, 2 * QB + 2, 8)
    q = qs[:1]
    r0, r1 = 9, n - 2
    top = S.to_bf16(q * np.float32(4.0))[0]  # about 4 |q|^2: the best row for q by far
    bits[r0] = top
    live = np.ones(n, bool)
    others = qs[1:]
    want = None
    for batch, at in ((q, 0), (np.concatenate([q, others[:QB - 1]]), 0), (np.concatenate([others[:QB - 1], q]), QB - 1),
                      (np.concatenate([others[:QB + 5], q, others[QB + 5:]]), QB + 5)):
        for k in (1, 128):
            rs, rm, sc, ids = launch(bits, batch, k, live)
            assert (rs, rm) == (0, 0) and ids[at, 0] == r0
            got = int(u32(sc)[at, 0])
            want = got if want is None else want
            assert got == want, (batch.shape[0], at, k)
    moved = bits.copy()
    moved[r1], moved[r0] = top, bits[r1]  # the same row bits in the last, partial tile
    for _ in range(20):
        rs, rm, sc, ids = launch(moved, q, 1, live)
        assert ids[0, 0] == r1 and int(u32(sc)[0, 0]) == want
    small = np.ascontiguousarray(moved[[3, r1]])  # N = 2
    rs, rm, sc, ids = launch(small, q, 1, np.ones(2, bool))
    assert ids[0, 0] == 1 and int(u32(sc)[0, 0]) == want


def test_a_query_block_is_independent_of_the_other_blocks_and_of_k():
    bits, c32, q, k, live, kind = F.build_case("d768_q130_k10")
    rs, rm, sc, ids = launch(bits, q, k, live)
    for a in range(0, q.shape[0], QB):
        part = launch(bits, q[a:a + QB], k, live)
        assert np.array_equal(u32(part[2]), u32(sc[a:a + QB])) and np.array_equal(part[3], ids[a:a + QB])
    wide = launch(bits, q[:5], 128, live)
    assert np.array_equal(u32(wide[2][:, :k]), u32(sc[:5])) and np.array_equal(wide[3][:, :k], ids[:5])


@pytest.mark.parametrize("pattern", [0x7FC0, 0x7F80, 0xFF80])
@pytest.mark.parametrize("name", ["d768_q65_k64", "d64_q1_k128_neg"])
def test_what_a_dead_row_holds_never_reaches_a_result(name, pattern):
    bits, c32, q, k, live, kind = F.build_case(name)
    zero = launch(bits, q, k, live, fill=0, want_cand=True)
    bad = launch(bits, q, k, live, fill=pattern, want_cand=True)
    assert zero[:2] == bad[:2] == (0, 0)
    assert np.array_equal(u32(zero[2]), u32(bad[2])) and np.array_equal(zero[3], bad[3]) and np.array_equal(zero[4], bad[4])
    real = bad[3] >= 0
    assert np.isfinite(bad[2][real]).all() and live[bad[3][real]].all()
    if name == "d64_q1_k128_neg":  # "dead_tile": every row of the second tile is dead -> that tile's lists are zero keys
        assert not live[T:].any() and (bad[4][1] == 0).all() and (bad[4][0][:, :k] != 0).all()


REFUSALS = [
    (-100, dict(corpus=0)), (-100, dict(queries=0)), (-100, dict(live=0)), (-100, dict(cand=0)),
    (-101, dict(D=72, ldc=72)), (-102, dict(D=0, ldc=0)), (-103, dict(D=2080, ldc=2080)), (-104, dict(ldc=32)), (-104, dict(ldc=100)),
    (-105, dict(N=0)), (-106, dict(Q=0)), (-106, dict(Q=65535 * QB + 1, cand_bytes=2 ** 62)), (-107, dict(k=0)),
    (-107, dict(k=129, cand_bytes=2 ** 40)), (-108, dict(corpus=8)), (-108, dict(cand=4)), (-108, dict(live=2)),
    (-109, dict(live_bytes=4 * ((300 + 31) // 32) - 1)), (-110, dict(cand_bytes=2 * 3 * 10 * 8 - 1)), (-111, dict(queries=4)),
]


@pytest.mark.parametrize("code,kw", REFUSALS)
def test_every_refusal_launches_nothing(code, kw):
    """Pointer cases ADD the value to the real address (0 replaces it); ``launch`` asserts that every output and the
    scratch keep their canaries after a refusal."""
    bits, c32, q = make(300, 64, 3, 4)

    def tweak(p):
        for name, v in kw.items():
            real = getattr(p, name)
            setattr(p, name, (real + v if v else 0) if name in ("corpus", "queries", "live", "cand") else v)
    rs, rm, sc, ids = launch(bits, q, 10, np.ones(300, bool), tweak=tweak)
    assert rs == code and rm is None


def test_every_refusal_code_has_a_case():
    assert {c for c, _ in REFUSALS} == set(range(-111, -99))


def rescore(kind, bits, q, in_id, k, Q0=0, Q1=None):
    n, d = bits.shape
    Q1 = q.shape[0] if Q1 is None else Q1
    Q, R = Q1 - Q0, in_id.shape[1]
    corpus = torch.from_numpy(bits.view(np.int16)).to(DEV)
    qd = torch.from_numpy(np.ascontiguousarray(q[Q0:Q1], np.float32)).to(DEV)
    idd = torch.from_numpy(np.ascontiguousarray(in_id[Q0:Q1], np.int32)).to(DEV)
    sc = torch.full((Q + PAD, k), 7.0, dtype=torch.float32, device=DEV)
    ids = torch.full((Q + PAD, k), -7, dtype=torch.int32, device=DEV)
    p = OS.RescoreParams(corpus.data_ptr(), qd.data_ptr(), idd.data_ptr(), sc.data_ptr(), ids.data_ptr(), n, d, Q, R, k, d)
    rc = N.lib().hz_launch_kernel(kind, C.byref(p), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    sch, idh = sc.cpu().numpy(), ids.cpu().numpy()
    assert (sch[Q:] == 7.0).all() and (idh[Q:] == -7).all()
    return rc, sch[:Q], idh[:Q]


@pytest.mark.parametrize("Q", [1, 17, 130])
def test_kind_45_equals_kind_35_sixteen_at_a_time(Q):
    n, d, R, k = 300, 96, 40, 10
    bits, c32, q = make(n, d, Q, 12)
    rng = np.random.default_rng(Q)
    in_id = np.stack([rng.permutation(n)[:R] for _ in range(Q)]).astype(np.int32)
    in_id[:, -3:] = -1          # empty slots
    in_id[0, :] = -1            # a query without candidates
    rc, sc, ids = rescore(N.HZ_K_SEARCH_RESCOREN, bits, q, in_id, k)
    assert rc == 0 and (ids[0] == -1).all() and np.isneginf(sc[0]).all()
    for a in range(0, Q, 16):
        rc35, s35, i35 = rescore(N.HZ_K_SEARCH_RESCORE, bits, q, in_id, k, a, min(Q, a + 16))
        assert rc35 == 0 and np.array_equal(u32(s35), u32(sc[a:a + 16])) and np.array_equal(i35, ids[a:a + 16])
    if Q > 16:  # kind 35 keeps its limit, kind 45 its refusals
        assert rescore(N.HZ_K_SEARCH_RESCORE, bits, q, in_id, k)[0] == -4
    assert rescore(N.HZ_K_SEARCH_RESCOREN, bits, q, in_id, R + 1)[0] == -31


DEBUG_CHILD = """
import sys
sys.path.insert(0, "tests")
from hipzap.utils import kcheck
import search_batch_cases as F
import test_search_batch_gpu as G
assert kcheck.enabled()
for name in ("d32_q1_k1", "d768_q65_k64", "d64_q130_k65", "d64_q1_k128_neg"):
    bits, c32, q, k, live, kind = F.build_case(name)
    rs, rm, sc, ids = G.launch(bits, q, k, live)
    assert (rs, rm) == (0, 0), (name, rs, rm)
    s, b, rs_, ri, forced = F.case_oracle(name)
    F.check_against_oracle(sc, ids, s, b, rs_, ri, forced, live)
fails = kcheck.poll()
assert fails == [], fails
print("silent")
"""


def test_the_debug_library_checks_stay_silent_on_the_edge_shapes():
    """The HZ_DCHECK unit of search.hip guards the query loads, the tile range, the pool and every candidate write of the
    batch scan: the debug library (a child process: HIPZAP_DEBUG selects the library at import) runs the smallest and
    the most ragged cases with the right answers and no record."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(os.path.join(root, "hipzap", "_lib", "libhipzap_debug.so")), "python -m hipzap.build --debug"
    env = dict(os.environ, HIPZAP_DEBUG="1", HIPZAP_NO_AUTOBUILD="1")
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "silent" in r.stdout, r.stderr[-4000:]
