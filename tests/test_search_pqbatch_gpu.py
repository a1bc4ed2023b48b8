"""Kinds 50 and 51 (csrc/search.hip). Kind 50's contract is bit identity with kind 44 over the decoded bf16 rows: its
merged keys are compared with that kernel's, and one shape with the fp64 oracle so the two cannot share a mistake."""
import ctypes as C

import numpy as np
import pytest
import torch

from hipzap import _native as N
from hipzap import search as S
from hipzap.ops import search as OS

import search_batch_cases as F
import test_search_batch_gpu as B
from test_search_batch_gpu import DEV, PAD, u32

pytestmark = pytest.mark.gpu
# (D, M): four k-steps, one code chunk; a code byte serves two fragments; dsub no power of two; the production shape
# (six code chunks); the largest
SHAPES = [(128, 16), (256, 16), (384, 16), (768, 96), (2048, 32)]
# (N, Q, k, live pattern): one row; a partial tile; two tiles; three tiles with a dead group and a dead row in a live one
RUNS = [(1, 1, 1, "all"), (255, 65, 64, "all"), (257, 69, 65, "all"), (600, 69, 128, "dead_group")]


def make(n, d, m, nq, seed, codes="random"):
    """-> (codes uint8 [n, m] that include 0 and 255, codebook fp32 [m, 256, d / m], queries fp32 [nq, d])."""
    rng = np.random.default_rng(seed)
    cb = rng.standard_normal((m, 256, d // m)).astype(np.float32)
    c = rng.integers(0, 256, (n, m)).astype(np.uint8)
    if codes == "same":
        c[:] = c[0]
    elif codes == "every":  # all 256 codes inside the first tile, in every sub-space
        c[:256] = (np.arange(256)[:, None] + np.arange(m)[None, :]) % 256
    else:
        c[0], c[n // 2] = 0, 255
    return c, cb, rng.standard_normal((nq, d)).astype(np.float32)


def launch(codes, cb8, q, k, live, tweak=None):
    """Kinds 50 and 40 -> (scan rc, merge rc, scores [Q, k], ids [Q, k]); canaries as in test_search_batch_gpu.launch."""
    n, m = codes.shape
    Q, d = q.shape
    cd = torch.from_numpy(codes.copy()).to(DEV)
    tb = torch.from_numpy(cb8.view(np.int16).copy()).to(DEV)
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV)
    nbytes = max(OS.self_scratch_bytes(n, Q, k), 8)
    cand = torch.full((nbytes // 8 + PAD * k,), -1, dtype=torch.int64, device=DEV)
    sc = torch.full((Q + PAD, k), 7.0, dtype=torch.float32, device=DEV)
    ids = torch.full((Q + PAD, k), -7, dtype=torch.int32, device=DEV)
    words = S.pack_live(live)
    lv = torch.from_numpy(words.view(np.int32)).to(DEV)
    p = OS.PqBatchScanParams(cd.data_ptr(), qd.data_ptr(), lv.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(),
                             words.size * 4, nbytes, n, d, Q, k, m, 0, (C.c_int * 2)(), tb.data_ptr(), cb8.nbytes, m, 0)
    if tweak:
        tweak(p)
    st = torch.cuda.current_stream().cuda_stream
    lib = N.lib()
    rs = lib.hz_launch_kernel(N.HZ_K_SEARCH_PQXSCAN, C.byref(p), st)
    rm = lib.hz_launch_kernel(N.HZ_K_SEARCH_MERGEN, C.byref(p), st) if rs == 0 else None
    torch.cuda.synchronize()
    sch, idh, ch = sc.cpu().numpy(), ids.cpu().numpy(), cand.cpu().numpy()
    assert (sch[Q:] == 7.0).all() and (idh[Q:] == -7).all() and (ch[nbytes // 8:] == -1).all()
    if rs != 0:
        assert (sch == 7.0).all() and (idh == -7).all() and (ch == -1).all()  # refused: nothing ran
    return rs, rm, sch[:Q], idh[:Q]


@pytest.mark.parametrize("n,nq,k,pattern", RUNS)
@pytest.mark.parametrize("d,m", SHAPES)
def test_the_merged_keys_are_the_batch_scans_over_the_decoded_rows(d, m, n, nq, k, pattern):
    codes, cb, q = make(n, d, m, nq, d + n)
    cb8, live = S.pq_table_bf16(cb), F.live_pattern(pattern, n)
    live[n - 3:n - 2] &= pattern == "all"  # with the dead group, a dead row in a live group of the last tile
    got = launch(codes, cb8, q, k, live)
    want = B.launch(S.pq_decode_bf16(codes, cb8), q, k, live)
    assert got[:2] == want[:2] == (0, 0)
    assert np.array_equal(u32(got[2]), u32(want[2])) and np.array_equal(got[3], want[3])


@pytest.mark.parametrize("codes", ["same", "every"])
def test_one_code_everywhere_and_every_code_in_a_tile_against_the_fp64_oracle(codes):
    n, d, m, nq, k = 300, 256, 16, 5, 10
    c, cb, q = make(n, d, m, nq, 5, codes)
    cb8, live = S.pq_table_bf16(cb), np.ones(n, bool)
    bits = S.pq_decode_bf16(c, cb8)
    rs, rm, sc, ids = launch(c, cb8, q, k, live)
    assert (rs, rm) == (0, 0)
    s, b, rs_, ri, forced = F.oracle(S.bf16_to_f32(bits), q, k, live)
    if codes == "same":  # equal rows: equal scores, the lower ids first
        forced[:] = False
        assert (ids == np.arange(k)[None, :]).all() and (u32(sc) == u32(sc[:, :1])).all()
    F.check_against_oracle(sc, ids, s, b, rs_, ri, forced, live)


def test_integer_cases_are_exact_bit_for_bit():
    """A codebook of -1, 0, 1 and integer queries below 2^17: every partial sum is an integer below 128 * 2^17 = 2^24."""
    n, d, m = 300, 128, 16
    codes, cb, _ = make(n, d, m, 1, 2)
    cb = np.random.default_rng(3).integers(-1, 2, cb.shape).astype(np.float32)
    q = F.exact_case(D=d, Q=5)[2]
    rs, rm, sc, ids = launch(codes, S.pq_table_bf16(cb), q, 128, np.ones(n, bool))
    assert (rs, rm) == (0, 0)
    dots = q.astype(np.int64) @ S.pq_decode(codes, cb).astype(np.int64).T
    for qi in range(q.shape[0]):
        assert np.array_equal(u32(sc[qi]), u32(dots[qi, ids[qi]].astype(np.float32) + np.float32(0.0))), qi
        assert np.array_equal(ids[qi], np.lexsort((np.arange(n), -dots[qi]))[:128]), qi


def test_the_bits_of_a_score_depend_on_the_query_the_codes_and_the_table_only():
    """100 rows alone, 20 replays; then as the only live rows of a 600-row corpus, slot 0 and 68, k = 100 and 128."""
    d, m = 768, 96
    codes, cb, qs = make(600, d, m, 69, 9)
    cb8 = S.pq_table_bf16(cb)
    part, q = codes[:100], qs[68:]
    rs, rm, sc, ids = launch(part, cb8, q, 128, np.ones(100, bool))
    assert (rs, rm) == (0, 0) and (ids[0, 100:] == -1).all()
    want = dict(zip(ids[0, :100].tolist(), u32(sc)[0, :100].tolist()))
    for _ in range(20):
        again = launch(part, cb8, q, 128, np.ones(100, bool))
        assert np.array_equal(u32(again[2]), u32(sc)) and np.array_equal(again[3], ids)
    big = codes.copy()
    big[200:300] = part
    live = np.zeros(600, bool)
    live[200:300] = True
    for batch, at in ((q, 0), (qs, 68)):
        for k in (100, 128):
            rs, rm, s2, i2 = launch(big, cb8, batch, k, live)
            assert (rs, rm) == (0, 0)
            assert dict(zip((i2[at, :100] - 200).tolist(), u32(s2)[at, :100].tolist())) == want, (at, k)


def rescore51(tweak=None):
    """Kinds 46 and 51 over fixed inputs -> (kind 51's rc, scores, ids, last, the inputs, kind 46's table)."""
    n, d, m, Q, R, k = 300, 384, 16, 5, 40, 10
    codes, cb, q = make(n, d, m, Q, 4)
    rng = np.random.default_rng(1)
    in_id = np.stack([rng.permutation(n)[:R] for _ in range(Q)]).astype(np.int32)
    in_id[:, -3:] = -1
    in_id[0, :] = -1  # a query without candidates
    in_sc = rng.standard_normal((Q, R)).astype(np.float32)
    t = {name: torch.from_numpy(a).to(DEV) for name, a in dict(codes=codes, cb=cb, q=q, id=in_id, sc=in_sc).items()}
    lut = torch.zeros((Q, m, 256), dtype=torch.float32, device=DEV)
    os_, oi = torch.full((Q, k + 1), 7.0, device=DEV), torch.full((Q, k + 1), -7, dtype=torch.int32, device=DEV)
    ol = torch.full((Q,), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    lp = OS.PqLutParams(t["q"].data_ptr(), t["cb"].data_ptr(), lut.data_ptr(), lut.numel() * 4, d, m, Q, 0)
    rp = OS.PqRescoreParams(t["codes"].data_ptr(), t["cb"].data_ptr(), t["q"].data_ptr(), t["id"].data_ptr(), t["sc"].data_ptr(),
                            os_.data_ptr(), oi.data_ptr(), ol.data_ptr(), n, d, m, Q, R, k, m, 0)
    if tweak:
        tweak(rp)
    assert N.lib().hz_launch_kernel(N.HZ_K_SEARCH_PQLUT, C.byref(lp), st) == 0
    rc = OS.launch_pq_rescore(rp, st)
    torch.cuda.synchronize()
    sc, ids, last = os_.cpu().numpy().ravel(), oi.cpu().numpy().ravel(), ol.cpu().numpy()
    if rc != 0:
        assert (sc == 7.0).all() and (ids == -7).all() and (last == 7.0).all()  # refused: nothing ran
    assert (sc[Q * k:] == 7.0).all() and (ids[Q * k:] == -7).all()  # the outputs are [Q][k], packed
    return rc, sc[:Q * k].reshape(Q, k), ids[:Q * k].reshape(Q, k), last, (codes, in_id, in_sc), lut.cpu().numpy()


def test_kind_51_gives_the_table_scans_bits_and_order():
    rc, sc, ids, last, (codes, in_id, in_sc), table = rescore51()
    assert rc == 0 and np.array_equal(u32(last), u32(in_sc[:, -1]))
    assert (ids[0] == -1).all() and np.isneginf(sc[0]).all()
    for qi in range(1, ids.shape[0]):
        cand = in_id[qi][in_id[qi] >= 0]
        s = S.pq_scores_from_lut(table[qi], codes[cand]) + np.float32(0.0)
        order = np.lexsort((cand, -s))[:ids.shape[1]]  # the order rule: higher score first, then the lower id
        assert np.array_equal(ids[qi], cand[order]) and np.array_equal(u32(sc[qi]), u32(s[order])), qi


POINTERS = ("codes", "queries", "live", "cand", "cb8", "codebook", "in_id", "in_score", "out_score", "out_id", "out_last")
REFUSALS = [  # -143 .. -157: kind 50 at N = 300, D = 128, M = 16, Q = 3, k = 10; -158 .. -164: kind 51 (rescore51's shape)
    (-143, dict(codes=0)), (-143, dict(queries=0)), (-143, dict(live=0)), (-143, dict(cand=0)), (-143, dict(cb8=0)),
    (-144, dict(D=144)), (-145, dict(D=2304, M=48)), (-146, dict(M=80)), (-147, dict(D=192, M=24, ldc=32)),
    (-148, dict(D=1792, M=112, ldc=112)), (-149, dict(D=192)), (-150, dict(ldc=8)), (-150, dict(ldc=24)), (-151, dict(N=0)),
    (-152, dict(Q=0)), (-152, dict(Q=1025, cand_bytes=2 ** 40)), (-153, dict(k=0)), (-153, dict(k=129, cand_bytes=2 ** 40)),
    (-154, dict(codes=8)), (-154, dict(queries=4)), (-154, dict(cb8=2)), (-154, dict(cand=4)), (-154, dict(live=2)),
    (-155, dict(live_bytes=4 * ((300 + 31) // 32) - 1)), (-156, dict(cand_bytes=2 * 3 * 10 * 8 - 1)), (-157, dict(cb8_bytes=512 * 128 - 1)),
    (-158, dict(M=24)), (-158, dict(D=392)), (-158, dict(ldc=8)), (-158, dict(ldc=24)), (-159, dict(N=0)), (-160, dict(Q=0)),
    (-161, dict(R=0)), (-161, dict(R=129)), (-162, dict(k=0)), (-162, dict(k=41)), (-163, dict(codes=0)), (-163, dict(codebook=0)),
    (-163, dict(in_score=0)), (-163, dict(out_last=0)), (-164, dict(codes=8)), (-164, dict(in_id=2)), (-164, dict(out_last=2)),
]


@pytest.mark.parametrize("code,kw", REFUSALS)
def test_every_refusal_launches_nothing(code, kw):
    """Pointer cases ADD the value to the real address (0 replaces it); both helpers assert the canaries after a refusal."""
    def tweak(p):
        for name, v in kw.items():
            setattr(p, name, (getattr(p, name) + v if v else 0) if name in POINTERS else v)
    if code <= -158:
        assert rescore51(tweak)[0] == code
    else:
        codes, cb, q = make(300, 128, 16, 3, 6)
        rs, rm, sc, ids = launch(codes, S.pq_table_bf16(cb), q, 10, np.ones(300, bool), tweak=tweak)
        assert rs == code and rm is None
    assert {c for c, _ in REFUSALS} == set(range(-164, -142))  # every code has a case


DEBUG_CHILD = """
import sys
sys.path.insert(0, "tests")
from hipzap.utils import kcheck
import test_search_pqbatch_gpu as G
assert kcheck.enabled()
for (d, m), (n, nq, k, pattern) in zip(G.SHAPES, G.RUNS + G.RUNS[-1:]):
    G.test_the_merged_keys_are_the_batch_scans_over_the_decoded_rows(d, m, n, nq, k, pattern)
G.test_kind_51_gives_the_table_scans_bits_and_order()
fails = kcheck.poll()
assert fails == [], fails
print("silent")
"""


def test_the_debug_library_checks_stay_silent_on_the_edge_shapes():
    """The HZ_DCHECK unit guards the table gathers, the code loads and every candidate write (a child process)."""
    import os, subprocess, sys  # noqa: E401
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(os.path.join(root, "hipzap", "_lib", "libhipzap_debug.so")), "python -m hipzap.build --debug"
    env = dict(os.environ, HIPZAP_DEBUG="1", HIPZAP_NO_AUTOBUILD="1")
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "silent" in r.stdout, r.stderr[-4000:]
