"""The rescore kernel (csrc/search.hip, HZ_K_SEARCH_RESCORE): the second stage of a two-stage search.

Its contract is bitwise: a real (q, r) scores the bits of HZ_K_SEARCH_SCAN for the same query and the same bf16 row,
and the scan's bits do not depend on a row's position. So the expected answer of every case is the existing scan +
merge (k = 128) over the gathered sub-corpus of the query's chosen rows, in ascending id order (the sub-corpus'
positions then break ties as the ids do); scores are compared bit for bit and ids exactly."""
import numpy as np
import pytest
import torch

from hipzap import search as S
from hipzap.ops import search as OS

import search_rescore_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # elements after each output buffer that no launch may touch


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scan_merge(bits, q, k):
    """The existing scan + merge -> (scores [Q, k], ids [Q, k])."""
    n, d = bits.shape
    corpus = torch.from_numpy(bits.view(np.int16)).to(DEV)
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV)
    nbytes = OS.scratch_bytes(n, q.shape[0], k)
    cand = torch.zeros(nbytes // 8, dtype=torch.int64, device=DEV)
    sc = torch.full((q.shape[0], k), 7.0, dtype=torch.float32, device=DEV)
    ids = torch.full((q.shape[0], k), -7, dtype=torch.int32, device=DEV)
    p = OS.SearchParams(corpus.data_ptr(), qd.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(), n, d,
                        q.shape[0], k, d, 0, nbytes)
    assert OS.launch(p, torch.cuda.current_stream().cuda_stream) == (0, 0)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), ids.cpu().numpy()


def expected(bits, q, in_id, k):
    """Per query: scan + merge over its chosen rows (ascending id), mapped back to the ids."""
    sc = np.full((q.shape[0], k), -np.inf, np.float32)
    ids = np.full((q.shape[0], k), -1, np.int32)
    for qi in range(q.shape[0]):
        chosen = np.sort(in_id[qi][in_id[qi] >= 0])
        if chosen.size:
            s, i = scan_merge(np.ascontiguousarray(bits[chosen]), q[qi:qi + 1], k)
            sc[qi] = s[0]
            ids[qi] = np.where(i[0] >= 0, chosen[np.maximum(i[0], 0)], -1)
    return sc, ids


def rescore(bits, q, in_id, k, ldc=None, tweak=None):
    """One rescore launch over device copies -> (code, scores [Q, k], ids [Q, k]); asserts that the guard elements
    after [Q][k] still hold the fill 7.0 / -7."""
    n, d = bits.shape
    ldc = ldc or d
    host = np.zeros((n, ldc), np.uint16)
    host[:, :d] = bits
    rows = torch.from_numpy(host.view(np.int16)).to(DEV)
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV)
    idd = torch.from_numpy(np.ascontiguousarray(in_id, np.int32)).to(DEV)
    Q, Rn = in_id.shape
    sc = torch.full((Q * k + GUARD,), 7.0, dtype=torch.float32, device=DEV)
    ids = torch.full((Q * k + GUARD,), -7, dtype=torch.int32, device=DEV)
    p = OS.RescoreParams(rows.data_ptr(), qd.data_ptr(), idd.data_ptr(), sc.data_ptr(), ids.data_ptr(), n, d, Q, Rn, k, ldc)
    if tweak:
        tweak(p)
    rc = OS.launch_rescore(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    s, i = sc.cpu().numpy(), ids.cpu().numpy()
    assert (s[Q * k:] == 7.0).all() and (i[Q * k:] == -7).all(), "a write past [Q][k]"
    return rc, s[:Q * k].reshape(Q, k), i[:Q * k].reshape(Q, k)


def written(sc, ids):
    return not (sc == 7.0).any() and not (ids == -7).any()


# ---------------------------------------------------------------------------------- 1. bitwise against the scan
@pytest.mark.parametrize("Q", R.BITS_Q)
@pytest.mark.parametrize("D", R.BITS_D)
def test_scores_are_the_scans_bits(D, Q):
    bits, _, q16 = R.bits_corpus(D)
    q = q16[:Q]
    in_id = R.choose_ids(Q, R.BITS_N, seed=D + Q)
    es, ei = expected(bits, q, in_id, 128)
    assert (ei[:, :100] >= 0).all() and (ei[:, 100:] == -1).all()
    for k, ldc in ((10, D), (128, D + 8)):
        rc, sc, ids = rescore(bits, q, in_id, k, ldc=ldc)
        assert rc == 0 and written(sc, ids)
        assert np.array_equal(ids, ei[:, :k]), (D, Q, k)
        assert np.array_equal(u32(sc), u32(es[:, :k])), (D, Q, k)
    assert (ids[:, 100:] == -1).all() and (sc[:, 100:] == -np.inf).all()


# ---------------------------------------------------------------------------------- 2. order and ties
def test_equal_scores_come_out_by_id_and_a_negative_zero_row_ties_with_a_positive_zero_row():
    """All other scores are negative, so neither padding nor an empty slot can outrank a real candidate. A score of
    -0.0 itself cannot leave the fmaf chain (it starts from +0, and -0 + +0 = +0): the row of -0.0 elements is the
    nearest case, and it must tie with the row of +0.0 elements at the bits of +0.0, the lower id first."""
    rng = np.random.default_rng(90)
    N, D = 40, 72
    c = -rng.uniform(0.5, 1.5, (N, D)).astype(np.float32)
    q = rng.uniform(0.5, 1.5, (2, D)).astype(np.float32)
    bits = S.to_bf16(c)
    for dup in (17, 30, 5):
        bits[dup] = bits[11]         # one row at four ids
    bits[22] = 0x0000               # +0.0 elements
    bits[9] = 0x8000                # -0.0 elements
    in_id = np.stack([rng.permutation(N).astype(np.int32), rng.permutation(N).astype(np.int32)])
    in_id = np.concatenate([in_id, np.full((2, 8), -1, np.int32)], axis=1)[:, rng.permutation(N + 8)]
    rc, sc, ids = rescore(bits, q, in_id, 48)
    assert rc == 0 and written(sc, ids)
    es, ei = expected(bits, q, in_id, 48)
    assert np.array_equal(ids, ei) and np.array_equal(u32(sc), u32(es))
    for qi in range(2):
        assert ids[qi, :2].tolist() == [9, 22] and (u32(sc[qi, :2]) == 0).all()   # +0.0 bits, the lower id first
        at = [int(np.flatnonzero(ids[qi] == r)[0]) for r in (5, 11, 17, 30)]
        assert at == list(range(at[0], at[0] + 4)) and len(set(u32(sc[qi, at]).tolist())) == 1
        assert (sc[qi, 2:N] < 0).all() and (ids[qi, N:] == -1).all() and (sc[qi, N:] == -np.inf).all()


# ---------------------------------------------------------------------------------- 3. edges of R and k
@pytest.mark.parametrize("Rn,k,real", [(1, 1, 1), (5, 5, 5), (5, 3, 4), (127, 127, 127), (127, 10, 90), (128, 128, 128),
                                       (128, 128, 0), (16, 10, 0), (16, 10, 4), (128, 128, 100)])
def test_edges_of_r_and_k(Rn, k, real):
    D, Q = 520, 3
    bits, _, q16 = R.bits_corpus(D)
    q = q16[:Q]
    in_id = R.choose_ids(Q, R.BITS_N, R=Rn, real=real, seed=Rn + k + real)
    rc, sc, ids = rescore(bits, q, in_id, k)
    assert rc == 0 and written(sc, ids)   # nothing of the 7.0 / -7 fill survives inside [Q][k]
    es, ei = expected(bits, q, in_id, k)
    assert np.array_equal(ids, ei) and np.array_equal(u32(sc), u32(es))
    assert (ids[:, :min(k, real)] >= 0).all() and (ids[:, real:] == -1).all() and (sc[:, real:] == -np.inf).all()


# ---------------------------------------------------------------------------------- 4. independence
def test_a_pair_scores_the_same_bits_wherever_it_stands():
    D = 768
    bits, _, q16 = R.bits_corpus(D)
    row = 123
    bits[row] = S.to_bf16((q16[9] * np.float32(3.0))[None, :])[0]   # far above the N(0, 1) rows' scores for query 9
    seen = set()
    rng = np.random.default_rng(91)
    for Rn, slot, Q, qi in ((8, 0, 1, 0), (8, 7, 16, 9), (128, 5, 1, 0), (128, 126, 16, 9), (128, 64, 16, 9)):
        q = q16[9:10] if Q == 1 else q16
        rest = np.delete(np.arange(R.BITS_N), row)  # other candidates, drawn anew for every launch
        in_id = np.stack([rng.choice(rest, Rn, replace=False) for _ in range(Q)]).astype(np.int32)
        in_id[qi, slot] = row
        rc, sc, ids = rescore(bits, q, in_id, min(Rn, 10))
        assert rc == 0 and ids[qi, 0] == row, (Rn, slot, Q)
        seen.add(int(u32(sc)[qi, 0]))
    s, i = scan_merge(bits, q16[9:10], 1)
    assert i[0, 0] == row
    seen.add(int(u32(s)[0, 0]))
    assert len(seen) == 1, seen


# ---------------------------------------------------------------------------------- 5. refusals
def test_the_launcher_refuses_misuse_without_launching():
    bits, _, q16 = R.bits_corpus(520)
    bits, q = bits[:40, :32].copy(), q16[:2, :32].copy()
    in_id = R.choose_ids(2, 40, R=16, real=12, seed=5)
    seen = {}

    def refused(what, code, k=10, tweak=None, **kw):
        rc, sc, ids = rescore(bits, q, in_id, k, tweak=tweak, **kw)
        assert rc == code, (what, rc)
        assert (sc == 7.0).all() and (ids == -7).all(), what  # nothing ran
        seen[what] = rc

    def setp(**kv):
        return lambda p: [setattr(p, a, v(p) if callable(v) else v) for a, v in kv.items()]

    refused("D % 8", -2, tweak=setp(D=28))
    refused("D < 8", -2, tweak=setp(D=0))
    refused("D > 2048", -2, tweak=setp(D=2056, ldc=2056))
    refused("ldc < D", -2, tweak=setp(ldc=24))
    refused("ldc % 8", -2, tweak=setp(ldc=36))
    refused("N = 0", -3, tweak=setp(N=0))
    refused("Q = 0", -4, tweak=setp(Q=0))
    refused("Q = 17", -4, tweak=setp(Q=17))
    refused("R = 0", -30, tweak=setp(R=0))
    refused("R = 129", -30, tweak=setp(R=129))
    refused("k = 0", -31, tweak=setp(k=0))
    refused("k > R", -31, tweak=setp(k=17))
    for name in ("rows", "queries", "in_id", "out_score", "out_id"):
        refused(name + " null", -32, tweak=setp(**{name: 0}))
    refused("rows misaligned", -33, tweak=setp(rows=lambda p: p.rows + 8))
    refused("queries misaligned", -33, tweak=setp(queries=lambda p: p.queries + 4))
    for name in ("in_id", "out_score", "out_id"):
        refused(name + " misaligned", -33, tweak=setp(**{name: lambda p, n=name: getattr(p, n) + 2}))
    assert set(seen.values()) == {-2, -3, -4, -30, -31, -32, -33}
    rc, sc, ids = rescore(bits, q, in_id, 10)  # and the same buffers are accepted
    es, ei = expected(bits, q, in_id, 10)
    assert rc == 0 and np.array_equal(ids, ei) and np.array_equal(u32(sc), u32(es))
