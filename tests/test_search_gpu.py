"""The vector-search kernels (csrc/search.hip) and the GPU index (csrc/index.cpp) against the fp64 oracle
``hipzap.search.search_ref``.

Scores: for every returned (query, id), ``|score - fp64 dot| <= gamma_D * sum_i |q_i c_i|`` with
``gamma_D = D u / (1 - D u)``, ``u = 2^-24``: the bound of an fp32 inner product in any summation order,
with or without FMA (the bf16 -> fp32 widening is exact). Ids: the seeds below are chosen on the CPU so
that no case is ambiguous (the fp64 gap between the oracle's k-th and (k+1)-th score is at least twice that
bound) and no two distinct rows tie in fp64 -- asserted on the host by ``test_cases_are_unambiguous`` --
and the returned id lists then equal the oracle's exactly, in order.

Data kinds: "normal" = N(0, 1) rows and queries; "pos" = rows U(0.9, 1.1) scaled by 1.01^(a permutation of
0..N-1), queries U(0.5, 1.5) (every product positive: scores spread over decades, so large D / Q / k cases
stay unambiguous under the rigorous bound); "neg" = "pos" with the rows negated (every score negative:
the padding of a partial tile must not outrank a real row)."""
import threading

import numpy as np
import pytest
import torch

from hipzap import search as S
from hipzap.ops import search as OS

T = OS.tile_rows()
U = 2.0 ** -24


def gamma(D):
    return D * U / (1 - D * U)


def make(N, D, Q, seed, kind="normal"):
    """-> (corpus bf16 bits uint16 [N, D], the same rows as fp32, queries fp32 [Q, D])."""
    rng = np.random.default_rng(seed)
    if kind == "normal":
        c, q = rng.standard_normal((N, D)), rng.standard_normal((Q, D))
    else:
        c = rng.uniform(0.9, 1.1, (N, D)) * (1.01 ** rng.permutation(N))[:, None]
        q = rng.uniform(0.5, 1.5, (Q, D))
        if kind == "neg":
            c = -c
    bits = S.to_bf16(c.astype(np.float32))
    return bits, S.bf16_to_f32(bits), q.astype(np.float32)


def oracle(c32, q, k):
    """(fp64 scores [Q, N], bounds [Q, N], ref scores [Q, k], ref ids [Q, k])."""
    c64, q64 = c32.astype(np.float64), q.astype(np.float64)
    s = np.stack([(c64 * r[None, :]).sum(axis=1) for r in q64])
    b = gamma(c32.shape[1]) * np.stack([np.abs(c64 * r[None, :]).sum(axis=1) for r in q64])
    rs, ri = S.search_ref(c32, q, k)
    return s, b, rs, ri


def ambiguous(s, b, k, allow_ties=False):
    """Queries for which the oracle's answer is not forced: two neighbours among its first k + 1 scores (the
    k-th / (k+1)-th gap included) are closer than twice the bound, or two rows tie in fp64 (``allow_ties``:
    exact ties, which the order rule settles by id, do not count)."""
    bad = 0
    for qi in range(s.shape[0]):
        order = np.argsort(-s[qi], kind="stable")
        srt, bs = s[qi][order], b[qi][order]
        tie = srt[1:] == srt[:-1]
        top = slice(0, min(k, srt.size - 1))
        close = (srt[:-1] - srt[1:] < 2 * np.maximum(bs[:-1], bs[1:]))[top]
        if allow_ties:
            bad += bool(np.any(close & ~tie[top]))
        else:
            bad += bool(np.any(tie) or np.any(close))
    return bad


def plant(bits, q, rows_scales):
    """Overwrite rows with multiples of query 0 (scores far above the N(0, 1) rows'): {row: scale}."""
    for r, a in rows_scales.items():
        bits[r] = S.to_bf16((q[0] * np.float32(a))[None, :])[0]
    return bits, S.bf16_to_f32(bits)


# (name, N, D, Q, k, kind, seed): every N of {1, k-1, k, T-1, T, T+1, 3T+5}, D of {8, 72, 768, 2048},
# Q of {1, 3, 16} and k of {1, 10, 128} appears; the seeds make every case unambiguous (asserted below)
CASES = [
    ("n1", 1, 8, 1, 1, "normal", 0),
    ("n1_k10", 1, 72, 3, 10, "normal", 0),
    ("n_km1", 9, 768, 3, 10, "normal", 0),
    ("n_k", 10, 2048, 1, 10, "normal", 0),
    ("n_km1_128", 127, 72, 16, 128, "pos", 2),
    ("n_k_128", 128, 8, 3, 128, "normal", 0),
    ("t_m1", T - 1, 768, 1, 10, "normal", 0),
    ("t", T, 72, 16, 1, "normal", 0),
    ("t_p1", T + 1, 2048, 3, 10, "pos", 0),
    ("t_p1_k128", T + 1, 8, 1, 128, "normal", 0),
    ("t3_d8", 3 * T + 5, 8, 16, 10, "normal", 0),
    ("t3_d72", 3 * T + 5, 72, 3, 128, "pos", 0),
    ("t3_d768", 3 * T + 5, 768, 16, 10, "pos", 0),
    ("t3_d2048", 3 * T + 5, 2048, 16, 128, "pos", 0),
    ("t3_d768_k128", 3 * T + 5, 768, 3, 128, "pos", 1),
    ("t3_q1_k1", 3 * T + 5, 2048, 1, 1, "normal", 0),
    ("neg_partial", 2 * T + 3, 72, 3, 10, "neg", 0),
    ("neg_small", 5, 768, 16, 10, "neg", 0),
]
# planted arrangements on a 3T+5 corpus of N(0, 1) rows, one query: {row: multiple of the query}
ARRANGE = {
    "best_is_last_row_of_partial_tile": (10, {3 * T + 4: 3.0}),
    "best_k_in_one_tile": (10, {T + 7 * j + 1: 3.0 - 0.125 * j for j in range(10)}),
    "best_k_one_per_tile": (4, {j * T + (37 * j + 5) % T if j < 3 else 3 * T + 2: 3.0 - 0.25 * j for j in range(4)}),
}
ARRANGE_SEED = 0


def build_case(name):
    for n, N, D, Q, k, kind, seed in CASES:
        if n == name:
            bits, c32, q = make(N, D, Q, seed, kind)
            return bits, c32, q, k
    k, rows = ARRANGE[name]
    bits, c32, q = make(3 * T + 5, 768, 1, ARRANGE_SEED)
    bits, c32 = plant(bits, q, rows)
    return bits, c32, q, k


ALL = [c[0] for c in CASES] + list(ARRANGE)


def test_cases_are_unambiguous():
    """Host only: the seeds give zero ambiguous cases and no fp64 tie between distinct rows."""
    for name in ALL:
        bits, c32, q, k = build_case(name)
        s, b, rs, ri = oracle(c32, q, k)
        assert ambiguous(s, b, k) == 0, name
    assert {c[1] for c in CASES} >= {1, 9, 10, T - 1, T, T + 1, 3 * T + 5}
    assert {c[2] for c in CASES} == {8, 72, 768, 2048} and {c[3] for c in CASES} == {1, 3, 16}
    assert {c[4] for c in CASES} == {1, 10, 128}


# ------------------------------------------------------------------------------------------ the launch
def launch(bits, q, k, ldc=None, N=None, D=None, Q=None, tweak=None):
    """Scan + merge over device copies -> (scan rc, merge rc, scores [Q, k], ids [Q, k])."""
    dev = "cuda:0"
    n, d = bits.shape
    ldc = ldc or d
    host = np.zeros((n, ldc), np.uint16)
    host[:, :d] = bits
    corpus = torch.from_numpy(host.view(np.int16)).to(dev)
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(dev)
    Qn = q.shape[0] if Q is None else Q
    nbytes = max(OS.scratch_bytes(n, min(max(Qn, 1), 16), min(max(k, 1), 128)), 8)
    cand = torch.zeros(nbytes // 8, dtype=torch.int64, device=dev)
    sc = torch.full((max(Qn, 1), max(k, 1)), 7.0, dtype=torch.float32, device=dev)  # 7 / -7: "never written"
    ids = torch.full((max(Qn, 1), max(k, 1)), -7, dtype=torch.int32, device=dev)
    p = OS.SearchParams(corpus.data_ptr(), qd.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(),
                        n if N is None else N, d if D is None else D, Qn, k, ldc, 0, nbytes)
    if tweak:
        tweak(p)
    rc = OS.launch(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc[0], rc[1], sc.cpu().numpy(), ids.cpu().numpy()


def check_against_oracle(c32, q, k, sc, ids):
    s, b, rs, ri = oracle(c32, q, k)
    assert np.array_equal(ids, ri), "ids differ from search_ref"
    for qi in range(q.shape[0]):
        for j in range(k):
            i = ids[qi, j]
            if i < 0:
                assert sc[qi, j] == -np.inf
            else:
                assert abs(float(sc[qi, j]) - s[qi, i]) <= b[qi, i], (qi, j, i, sc[qi, j], s[qi, i], b[qi, i])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_topk_matches_the_oracle(name):
    bits, c32, q, k = build_case(name)
    rs, rm, sc, ids = launch(bits, q, k)
    assert (rs, rm) == (0, 0)
    check_against_oracle(c32, q, k, sc, ids)
    if name in ARRANGE:
        assert list(ids[0, :len(ARRANGE[name][1])]) == list(ARRANGE[name][1])  # the planted rows, in their order
    if name.startswith("neg"):
        real = ids >= 0
        assert (sc[real] < 0).all() and (ids[:, :min(k, c32.shape[0])] >= 0).all()


@pytest.mark.gpu
def test_zero_query_scores_plus_zero_and_ids_ascend():
    bits, c32, q = make(T + 9, 72, 3, 5)
    q[1] = 0
    q[2] = -0.0
    _, _, sc, ids = launch(bits, q, 10)
    for qi in (1, 2):
        assert list(ids[qi]) == list(range(10))
        assert (sc[qi].view(np.uint32) == 0).all()  # +0.0, not -0.0
    assert np.array_equal(ids, S.search_ref(c32, q, 10)[1])


@pytest.mark.gpu
def test_a_row_stride_above_d():
    bits, c32, q = make(T + 3, 72, 3, 6)
    a = launch(bits, q, 10)
    b = launch(bits, q, 10, ldc=88)
    assert a[:2] == b[:2] == (0, 0)
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)) and np.array_equal(a[3], b[3])


@pytest.mark.gpu
def test_ties_come_back_in_ascending_id_with_equal_bits():
    N, k = 2 * T + 40, 10
    bits, c32, q = make(N, 72, 3, 7)
    dup = [3, 17, T - 1, T + 4, 2 * T + 9]  # three in tile 0, one in each later tile
    bits, c32 = plant(bits, q, {r: 3.0 for r in dup})
    s, b, _, _ = oracle(c32, q, k)
    assert ambiguous(s, b, k, allow_ties=True) == 0  # host: only the duplicates tie
    _, _, sc, ids = launch(bits, q, k)
    assert list(ids[0, :5]) == dup
    assert len(set(sc[0, :5].view(np.uint32).tolist())) == 1
    for qi in range(3):  # the duplicates tie for every query: wherever they rank, they ascend
        at = [j for j in range(k) if ids[qi, j] in dup]
        assert [ids[qi, j] for j in at] == sorted(ids[qi, j] for j in at)
        assert len({int(sc[qi, j].view(np.uint32)) for j in at}) <= 1
    assert np.array_equal(ids, S.search_ref(c32, q, k)[1])
    # N < k: the slots past N hold -1 / -inf
    few, few32 = bits[[3, 17, 40, T - 1]], c32[[3, 17, 40, T - 1]]
    _, _, sc, ids = launch(few, q, k)
    assert list(ids[0]) == [0, 1, 3, 2] + [-1] * 6 and (sc[:, 4:] == -np.inf).all() and (ids[:, 4:] == -1).all()
    assert sc[0, 0].view(np.uint32) == sc[0, 1].view(np.uint32) == sc[0, 2].view(np.uint32)
    assert np.array_equal(ids, S.search_ref(few32, q, k)[1])


@pytest.mark.gpu
def test_a_score_depends_on_its_query_and_row_only():
    N, D, k = 3 * T + 5, 768, 10
    bits, c32, q16 = make(N, D, 16, 8)
    one = q16[5:6].copy()
    _, _, s1, i1 = launch(bits, one, k)
    for slot in (0, 7, 15):  # the same query alone and as row 0, 7, 15 of a batch of 16
        batch = q16.copy()
        batch[slot] = one[0]
        _, _, sb, ib = launch(bits, batch, k)
        assert np.array_equal(sb[slot].view(np.uint32), s1[0].view(np.uint32)) and np.array_equal(ib[slot], i1[0])
    # the same row at another position, in a corpus of another N and with another k
    row = S.to_bf16((one * np.float32(3.0)))[0]
    a = bits[:T - 1].copy()
    a[3] = row
    b = bits.copy()
    b[2 * T + 100] = row
    _, _, sa, ia = launch(a, one, 1)
    _, _, sb, ib = launch(b, one, 128)
    assert ia[0, 0] == 3 and ib[0, 0] == 2 * T + 100
    assert sa[0, 0].view(np.uint32) == sb[0, 0].view(np.uint32)
    # two runs of the same search
    r1, r2 = launch(bits, q16, 128), launch(bits, q16, 128)
    assert np.array_equal(r1[2].view(np.uint32), r2[2].view(np.uint32)) and np.array_equal(r1[3], r2[3])


@pytest.mark.gpu
def test_the_launcher_refuses_misuse_without_launching():
    bits, c32, q = make(40, 16, 2, 9)

    def refused(**kw):
        rs, rm, sc, ids = launch(bits, q, kw.pop("k", 10), **kw)
        assert rs != 0 and rm is None, kw
        assert (sc == 7.0).all() and (ids == -7).all()  # nothing ran

    refused(D=12)                                    # D % 8
    refused(D=0)                                     # D < 8
    refused(D=2056, ldc=2056)                        # D > 2048
    refused(tweak=lambda p: setattr(p, "ldc", 8))    # ldc < D
    refused(N=0)                                     # N < 1
    refused(N=-1)                                    # 2^31 and above do not fit the field: negative
    refused(Q=0)
    refused(Q=17)
    refused(k=0)
    refused(k=129)
    refused(tweak=lambda p: setattr(p, "corpus", p.corpus + 2))    # unaligned pointers
    refused(tweak=lambda p: setattr(p, "queries", p.queries + 4))
    refused(tweak=lambda p: setattr(p, "cand", p.cand + 4))
    refused(tweak=lambda p: setattr(p, "cand_bytes", p.cand_bytes - 8))  # scratch too small
    refused(tweak=lambda p: setattr(p, "out_id", 0))
    assert OS.scratch_bytes(2 ** 31, 1, 1) == 0 and OS.scratch_bytes(2 ** 31 - 1, 1, 1) > 0
    assert OS.scratch_bytes(T + 1, 16, 128) == 2 * 16 * 128 * 8
    rs, rm, sc, ids = launch(bits, q, 10)  # and the same buffers are accepted
    assert (rs, rm) == (0, 0) and np.array_equal(ids, S.search_ref(c32, q, 10)[1])


@pytest.fixture(scope="module")
def index_file(tmp_path_factory):
    rng = np.random.default_rng(12)  # chosen on the CPU: unambiguous for k = 1, 7, 10
    vec = rng.standard_normal((2 * T + 31, 72)).astype(np.float32)
    path = str(tmp_path_factory.mktemp("idx") / "a.hzidx")
    S.write_index(path, vec, "cosine", labels=[f"row{i}" for i in range(vec.shape[0])], model="test")
    q = S.normalize_rows(rng.standard_normal((37, 72)).astype(np.float32))
    return path, q


@pytest.mark.gpu
def test_index_file_round_trip_on_the_device(index_file):
    path, q = index_file
    c32 = S.bf16_to_f32(S.read_rows(path))
    with S.Index(path) as ix:
        assert (ix.dim, ix.count, ix.metric, ix.labels[5]) == (72, 2 * T + 31, "cosine", "row5")
        for k in (1, 10):
            sc, ids = ix.search(q, k)  # 37 queries: 16 + 16 + 5
            s, b, rs, ri = oracle(c32, q, k)
            assert ambiguous(s, b, k) == 0  # host: the oracle's ids are forced
            assert np.array_equal(ids, ri)
            got = np.take_along_axis(s, ids.astype(np.int64), 1)
            assert (np.abs(sc - got) <= np.take_along_axis(b, ids.astype(np.int64), 1)).all()
            again = ix.search(q, k)  # the captured programs give the first (eager) run's bits
            assert np.array_equal(again[0].view(np.uint32), sc.view(np.uint32)) and np.array_equal(again[1], ids)
        d = ix.describe()
        assert d["contexts"] == 2 and d["tile_rows"] == T and d["programs"] >= 2 and d["count"] == ix.count
        with pytest.raises(ValueError, match="non-finite"):
            ix.search(np.full((1, 72), np.nan, np.float32), 3)
        with pytest.raises(ValueError, match=r"\[Q, 72\]"):
            ix.search(np.zeros((1, 64), np.float32), 3)
        with pytest.raises(ValueError, match="k must be"):
            ix.search(q[:1], 129)


@pytest.mark.gpu
def test_two_contexts_from_two_threads(index_file):
    path, q = index_file
    with S.Index(path) as ix:
        want = [ix.search(q[:16], 10), ix.search(q[16:32], 7)]
        got, errs = [None, None], []

        def work(t):
            try:
                for _ in range(20):
                    got[t] = ix.search(q[:16], 10, ctx=0) if t == 0 else ix.search(q[16:32], 7, ctx=1)
                    assert np.array_equal(got[t][1], want[t][1])
                    assert np.array_equal(got[t][0].view(np.uint32), want[t][0].view(np.uint32))
            except Exception as e:  # noqa: BLE001 - reported by the main thread
                errs.append(e)
        th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
