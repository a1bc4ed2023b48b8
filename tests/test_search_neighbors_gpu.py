"""The self scan (csrc/search.hip, HZ_K_SEARCH_MSCAN) and its merge (HZ_K_SEARCH_MERGEN) through ``hz_launch_kernel``,
against the fp64 oracle ``search_ref`` over the stored rows (tests/search_neighbors_cases.py: bound and cases).

Scores: within ``beta_D * sum |a_i b_i|`` of the fp64 dot. Ids: equal to the oracle's wherever its answer is forced
under that bound; tests/test_search_neighbors_cpu.py asserts on the host how many queries of each case that is.
Wherever two GPU runs are compared, they are compared bit for bit.

The worst |err| / bound over the cases and whether score(a, b) == score(b, a) held are printed by the tests and
recorded in profiles/search_neighbors/README.md; the header promises neither."""
import ctypes as C

import numpy as np
import pytest
import torch

from hipzap import _native as N
from hipzap import search as S
from hipzap.ops import search as OS

import search_neighbors_cases as F
from search_neighbors_cases import QB, T, make

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def launch(bits, qid, k, live, skip_self, fill=None, tweak=None):
    """Kinds 39 and 40 over device copies -> (scan rc, merge rc, scores [Q, k], ids [Q, k]). ``fill``: a uint16
    pattern written over the dead rows first."""
    n, d = bits.shape
    host = bits.copy()
    if fill is not None:
        host[~np.asarray(live, bool)] = fill
    corpus = torch.from_numpy(host.view(np.int16)).to(DEV)
    qd = torch.from_numpy(np.ascontiguousarray(qid, np.int32)).to(DEV)
    Q = len(qid)
    nbytes = max(OS.self_scratch_bytes(n, Q, k), 8)
    cand = torch.full((nbytes // 8,), -1, dtype=torch.int64, device=DEV)  # all ones: "never written" is no valid list
    sc = torch.full((Q, k), 7.0, dtype=torch.float32, device=DEV)
    ids = torch.full((Q, k), -7, dtype=torch.int32, device=DEV)
    words = S.pack_live(live)
    lv = torch.from_numpy(words.view(np.int32)).to(DEV)
    p = OS.SelfScanParams(corpus.data_ptr(), qd.data_ptr(), lv.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(),
                          words.size * 4, nbytes, n, d, Q, k, d, 0, int(skip_self), 0)
    if tweak:
        tweak(p)
    st = torch.cuda.current_stream().cuda_stream
    lib = N.lib()
    rs = lib.hz_launch_kernel(N.HZ_K_SEARCH_MSCAN, C.byref(p), st)
    rm = lib.hz_launch_kernel(N.HZ_K_SEARCH_MERGEN, C.byref(p), st) if rs == 0 else None
    torch.cuda.synchronize()
    return rs, rm, sc.cpu().numpy(), ids.cpu().numpy()


WORST = {}


@pytest.mark.parametrize("name", F.NAMES)
def test_neighbours_match_the_oracle(name):
    bits, c32, qid, k, live, skip, kind = F.build_case(name)
    s, b, allow, rs_, ri = F.case_oracle(name)
    rs, rm, sc, ids = launch(bits, qid, k, live, skip)
    assert (rs, rm) == (0, 0)
    ok, worst = F.check_against_oracle(sc, ids, s, b, allow, rs_, ri, k)
    WORST[name] = worst
    print(f"{name}: forced {int(ok.sum())}/{ok.size}, worst |err|/bound {worst:.4f}")
    if kind != "normal":
        assert ok.all()


@pytest.mark.parametrize("pattern", [0x7FC0, 0x7F80, 0xFF80])
@pytest.mark.parametrize("name", ["t_group", "t3_tile"])
def test_what_a_dead_row_holds_never_reaches_a_result(name, pattern):
    bits, c32, qid, k, live, skip, kind = F.build_case(name)
    zero = launch(bits, qid, k, live, skip, fill=0)
    bad = launch(bits, qid, k, live, skip, fill=pattern)
    assert zero[:2] == bad[:2] == (0, 0)
    assert np.array_equal(u32(zero[2]), u32(bad[2])) and np.array_equal(zero[3], bad[3])
    assert (bad[3] >= 0).all() and np.isfinite(bad[2]).all() and live[bad[3]].all()


def test_a_planted_duplicate_ties_by_id_and_only_skip_self_hides_the_query():
    bits, c32, a, b = F.planted_pair()
    n = bits.shape[0]
    live = np.ones(n, bool)
    qid = np.array([a, b], np.int32)
    for skip in (0, 1):
        rs, rm, sc, ids = launch(bits, qid, 10, live, skip)
        assert (rs, rm) == (0, 0)
        s, bb, allow, rs_, ri = F.oracle(c32, qid, 10, live, skip)
        ok = F.forced(s, bb, 10, allow, allow_ties=True)  # the pair's exact tie is settled by id
        assert ok.all()
        F.check_against_oracle(sc, ids, s, bb, allow, rs_, ri, 10, must=ok)
        if skip:
            assert ids[0, 0] == b and ids[1, 0] == a and a not in ids[0] and b not in ids[1]
        else:
            assert ids[:, :2].tolist() == [[a, b], [a, b]]  # equal bits: equal scores, the lower id first
            assert u32(sc)[0, 0] == u32(sc)[0, 1] == u32(sc)[1, 0] == u32(sc)[1, 1]


def test_a_qid_outside_the_corpus_gives_zero_keys_and_reads_nothing():
    bits, c32, _ = make(T + 9, 96, 1, 6)
    n = bits.shape[0]
    live = np.ones(n, bool)
    qid = np.array([3, -1, n, 5, 2 ** 31 - 1, -2 ** 31], np.int32)
    rs, rm, sc, ids = launch(bits, qid, 10, live, 1)
    assert (rs, rm) == (0, 0)
    bad = [1, 2, 4, 5]
    assert (ids[bad] == -1).all() and (sc[bad] == -np.inf).all()
    good = launch(bits, qid[[0, 3]], 10, live, 1)
    assert np.array_equal(u32(good[2]), u32(sc[[0, 3]])) and np.array_equal(good[3], ids[[0, 3]])


def test_the_bits_of_a_score_depend_on_the_two_rows_only():
    """One pair (a, r): alone and inside a full block, at two positions of the query in qid, with the row in tile 0
    and (the same bits) in the last partial tile, at k = 1 and k = 128."""
    n, d = 3 * T + 5, 768
    bits, c32, _ = make(n, d, 1, 8)
    a, r0, r1 = 100, 9, n - 2
    top = S.to_bf16((c32[a] * np.float32(4.0))[None, :])[0]  # 4 |a|^2: the best row for query a by far; exact in bf16
    bits[r0] = top
    live = np.ones(n, bool)
    others = np.setdiff1d(np.arange(n), [a, r0, r1])[:2 * QB + 2].astype(np.int32)
    want = None
    for qid, at in ((np.array([a], np.int32), 0),
                    (np.concatenate([[a], others[:QB - 1]]).astype(np.int32), 0),
                    (np.concatenate([others[:QB + 5], [a], others[QB + 5:]]).astype(np.int32), QB + 5)):
        for k in (1, 128):
            rs, rm, sc, ids = launch(bits, qid, k, live, 1)
            assert (rs, rm) == (0, 0) and ids[at, 0] == r0
            got = int(u32(sc)[at, 0])
            want = got if want is None else want
            assert got == want, (len(qid), at, k)
    moved = bits.copy()
    moved[r1], moved[r0] = top, bits[r1]  # the same row bits in the last, partial tile
    rs, rm, sc, ids = launch(moved, np.array([a], np.int32), 1, live, 1)
    assert ids[0, 0] == r1 and int(u32(sc)[0, 0]) == want
    small = np.ascontiguousarray(moved[[a, r1]])  # N = 2: the same two rows alone
    rs, rm, sc, ids = launch(small, np.array([0], np.int32), 1, np.ones(2, bool), 1)
    assert ids[0, 0] == 1 and int(u32(sc)[0, 0]) == want


def test_replays_are_bitwise_equal_and_symmetry_is_reported():
    bits, c32, qid, k, live, skip, kind = F.build_case("t3_tile")
    first = launch(bits, qid, k, live, skip)
    for _ in range(3):
        again = launch(bits, qid, k, live, skip)
        assert np.array_equal(u32(first[2]), u32(again[2])) and np.array_equal(first[3], again[3])
    # score(a, b) against score(b, a): reported, not promised
    rows = np.flatnonzero(live)[:100].astype(np.int32)
    rs, rm, sc, ids = launch(bits[rows], np.arange(100, dtype=np.int32), 99, np.ones(100, bool), 1)
    full = np.zeros((100, 100), np.uint32)
    for qi in range(100):
        full[qi, ids[qi]] = u32(sc)[qi]
    sym = int((full == full.T).sum()) - 100
    print(f"score(a, b) == score(b, a) for {sym} of {100 * 99} ordered pairs")


def test_a_query_block_is_independent_of_the_other_blocks_and_of_k():
    """Q = 2 QB + 3 in one launch equals its three blocks launched alone, and the first 10 of k = 128 equal k = 10."""
    bits, c32, qid, k, live, skip, kind = F.build_case("t_p1_d2048")
    rs, rm, sc, ids = launch(bits, qid, k, live, skip)
    for a in range(0, len(qid), QB):
        part = launch(bits, qid[a:a + QB], k, live, skip)
        assert np.array_equal(u32(part[2]), u32(sc[a:a + QB])) and np.array_equal(part[3], ids[a:a + QB])
    wide = launch(bits, qid[:5], 128, live, skip)
    assert np.array_equal(u32(wide[2][:, :k]), u32(sc[:5])) and np.array_equal(wide[3][:, :k], ids[:5])


DEBUG_CHILD = """
import sys
sys.path.insert(0, "tests")
from hipzap.utils import kcheck
import search_neighbors_cases as F
import test_search_neighbors_gpu as G
assert kcheck.enabled()
for name in ("n1_skip", "n_k", "t3_tile", "t3_k128"):
    bits, c32, qid, k, live, skip, kind = F.build_case(name)
    rs, rm, sc, ids = G.launch(bits, qid, k, live, skip)
    assert (rs, rm) == (0, 0), (name, rs, rm)
    F.check_against_oracle(sc, ids, *F.case_oracle(name), k)
fails = kcheck.poll()
assert fails == [], fails
print("silent")
"""


def test_the_debug_library_checks_stay_silent_on_the_edge_shapes():
    """The HZ_DCHECK unit of search.hip guards the gather, the tile range and every candidate write of the self scan:
    the debug library (a child process: HIPZAP_DEBUG selects the library at import) runs the smallest and the most
    ragged cases with the right answers and no record."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(os.path.join(root, "hipzap", "_lib", "libhipzap_debug.so")), "python -m hipzap.build --debug"
    env = dict(os.environ, HIPZAP_DEBUG="1", HIPZAP_NO_AUTOBUILD="1")
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "silent" in r.stdout, r.stderr[-4000:]
