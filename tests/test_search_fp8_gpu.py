"""The quantised scan (csrc/search.hip, HZ_K_SEARCH_QSCAN: e4m3fn byte rows, one fp32 scale per row) against the
fp64 oracle ``search_ref(scales=...)``.

Ids equal the oracle's exactly: tests/test_search_fp8_cpu.py asserts on the host that every case is unambiguous
over its passing rows under twice the bound ``gamma(D + 1) * |scale_r| * sum_i |q_i c_ri|`` (one fp32 product
applied to a D-term fp32 sum). Wherever two GPU runs are compared, they are compared bit for bit."""
import numpy as np
import pytest
import torch

from hipzap import search as S
from hipzap.ops import search as OS

import search_fp8_cases as P
from search_fp8_cases import T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def launch(codes, scales, q, k, live=None, tags=None, filt=None, N=None, D=None, Q=None, ldc=None, tweak=None,
           fill=None, scale_fill=None):
    """Quantised scan + merge over device copies -> (scan rc, merge rc, scores [Q, k], ids [Q, k]). ``fill`` /
    ``scale_fill``: a code and a scale written over the dead rows first."""
    n, d = codes.shape
    live = np.ones(n, bool) if live is None else np.asarray(live, bool)
    ldc = ldc or d
    host = np.zeros((n, max(ldc, d)), np.uint8)
    host[:, :d] = codes
    sh = np.ascontiguousarray(scales, np.float32).copy()
    if fill is not None:
        host[~live] = fill
    if scale_fill is not None:
        sh[~live] = scale_fill
    corpus = torch.from_numpy(host).to(DEV)
    sd = torch.from_numpy(sh).to(DEV)
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV)
    Qn = q.shape[0] if Q is None else Q
    nbytes = max(OS.scratch_bytes(n, min(max(Qn, 1), 16), min(max(k, 1), 128)), 8)
    cand = torch.zeros(nbytes // 8, dtype=torch.int64, device=DEV)
    sc = torch.full((max(Qn, 1), max(k, 1)), 7.0, dtype=torch.float32, device=DEV)  # 7 / -7: "never written"
    ids = torch.full((max(Qn, 1), max(k, 1)), -7, dtype=torch.int32, device=DEV)
    words = S.pack_live(live)
    lv = torch.from_numpy(words.view(np.int32)).to(DEV)
    tg = None if tags is None else torch.from_numpy(np.ascontiguousarray(tags, np.uint32).view(np.int32)).to(DEV)
    fl = None if filt is None else torch.from_numpy(np.ascontiguousarray(filt, np.uint32).reshape(-1, 2).view(np.int32)).to(DEV)
    p = OS.QuantScanParams(corpus.data_ptr(), qd.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(),
                           n if N is None else N, d if D is None else D, Qn, k, ldc, 0, nbytes, lv.data_ptr(),
                           0 if tg is None else tg.data_ptr(), 0 if fl is None else fl.data_ptr(), words.size * 4,
                           sd.data_ptr())
    if tweak:
        tweak(p)
    rc = OS.launch_quant(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc[0], rc[1], sc.cpu().numpy(), ids.cpu().numpy()


def check(codes, scales, q, k, allow, sc, ids):
    s, b = P.oracle_q(codes, scales, q)
    assert np.array_equal(ids, P.ref_ids(codes, scales, q, k, allow)), "ids differ from search_ref(scales=...)"
    for qi in range(q.shape[0]):
        for j in range(k):
            i = ids[qi, j]
            if i < 0:
                assert sc[qi, j] == -np.inf
            else:
                assert abs(float(sc[qi, j]) - s[qi, i]) <= b[qi, i], (qi, j, i, sc[qi, j], s[qi, i], b[qi, i])


@pytest.mark.parametrize("name", P.NAMES)
def test_quantised_topk_matches_the_oracle(name):
    codes, scales, q, k, live = P.build_case(name)
    rs, rm, sc, ids = launch(codes, scales, q, k, live)
    assert (rs, rm) == (0, 0)
    check(codes, scales, q, k, live, sc, ids)
    npass = int(live.sum())
    assert (ids[:, :min(k, npass)] >= 0).all() and (ids[:, npass:] == -1).all() and (sc[:, npass:] == -np.inf).all()
    if name.startswith("neg"):
        assert (sc[ids >= 0] < 0).all()  # neither padding nor a dead row outranks a negative score


# all 254 finite codes in two launches of 127 rows; +0 and -0 share the first launch (a tie at +0)
DECODE_SETS = [np.r_[0x00:0x3F, 0x80:0xC0].astype(np.uint8), np.r_[0x3F:0x7F, 0xC0:0xFF].astype(np.uint8)]


def decode_rows(which):
    codes = np.zeros((127, 16), np.uint8)
    codes[:, 0] = DECODE_SETS[which]
    q = np.zeros((1, 16), np.float32)
    q[0, 0] = 1.0
    return codes, q


@pytest.mark.parametrize("which", [0, 1])
def test_every_finite_code_decodes_exactly(which):
    assert sorted(np.concatenate(DECODE_SETS).tolist()) == [c for c in range(256) if c & 0x7F != 0x7F]
    codes, q = decode_rows(which)
    rs, rm, sc, ids = launch(codes, np.ones(127, np.float32), q, 127)
    assert (rs, rm) == (0, 0)
    val = S.e4m3_to_f32(codes[:, 0]) + np.float32(0.0)  # -0 is reported as +0
    order = np.argsort(-val, kind="stable")  # equal values: ascending id
    assert np.array_equal(ids[0], order)
    assert np.array_equal(u32(sc[0]), u32(val[order]))
    if which == 0:
        zeros = [j for j in range(127) if ids[0, j] in (0, 63)]
        assert [ids[0, j] for j in zeros] == [0, 63] and (u32(sc[0])[zeros] == 0).all()


def test_the_scale_is_one_exact_multiply():
    for which in (0, 1):
        codes, q = decode_rows(which)
        _, _, s1, i1 = launch(codes, np.ones(127, np.float32), q, 127)
        for e in (-20, -3, 0, 5):
            rs, rm, sc, ids = launch(codes, np.full(127, 2.0 ** e, np.float32), q, 127)
            assert (rs, rm) == (0, 0) and np.array_equal(ids, i1)
            assert np.array_equal(u32(sc), u32(s1 * np.float32(2.0 ** e)))
        for scale in (np.float32(0.3), np.float32(1.7182818)):
            rs, rm, sc, ids = launch(codes, np.full(127, scale, np.float32), q, 127)
            assert (rs, rm) == (0, 0) and np.array_equal(ids, i1)
            assert np.array_equal(u32(sc), u32(scale * s1))  # fl32(scale * s1), s1 as read back from the GPU


def test_score_bits_depend_on_query_codes_and_scale_only():
    D = 768
    codes, scales, q16 = P.make_q(3 * T + 5, D, 16, 41)
    one = q16[5:6].copy()
    row, rscale = S.quantize_rows(one * np.float32(3.0))  # far above the N(0, 1) rows' scores
    seen = set()
    plans = [(1, None, 1, False), (16, 7, 128, True), (16, 0, 128, False), (16, 15, 1, True)]  # Q, slot, k, filtered
    for N, at in ((9, 0), (T, T - 1), (T + 1, T), (3 * T + 5, 3 * T + 4)):
        c, s = codes[:N].copy(), scales[:N].copy()
        c[at], s[at] = row[0], rscale[0]
        tags = (np.arange(N) % 3).astype(np.uint32)
        tags[at] = 2
        for Q, slot, k, filtered in plans:
            if Q == 1:
                qs, slot = one, 0
            else:
                qs = q16.copy()
                qs[slot] = one[0]
            kw = {"tags": tags, "filt": np.tile(np.array([[3, 2]], np.uint32), (Q, 1))} if filtered else {}
            rs, rm, sc, ids = launch(c, s, qs, k, **kw)
            assert (rs, rm) == (0, 0) and ids[slot, 0] == at, (N, at, Q, slot, k, filtered)
            seen.add(int(u32(sc)[slot, 0]))
    assert len(seen) == 1, seen


@pytest.mark.parametrize("code_fill", [0x00, 0x7F, 0xFF])
def test_what_a_dead_row_holds_never_reaches_a_result(code_fill):
    N, D, Q, k = 2 * T + 9, 80, 3, 10
    codes, scales, q = P.make_q(N, D, Q, 42)
    live = np.random.default_rng(42).random(N) < 0.5
    live[T:T + 8] = False   # two whole groups of four rows
    live[2 * T:] = [True, False] * 4 + [False]
    tags = (np.arange(N) % 3).astype(np.uint32)
    filt = np.array([[0, 0], [3, 1], [3, 2]], np.uint32)
    for kw in ({}, {"tags": tags, "filt": filt}):
        base = launch(codes, scales, q, k, live, **kw)
        assert base[:2] == (0, 0)
        for scale_fill in (0.0, np.nan, np.inf, -np.inf):
            bad = launch(codes, scales, q, k, live, fill=code_fill, scale_fill=scale_fill, **kw)
            assert bad[:2] == (0, 0)
            assert np.array_equal(u32(base[2]), u32(bad[2])) and np.array_equal(base[3], bad[3])
            assert (bad[3] >= 0).all() and np.isfinite(bad[2]).all() and live[bad[3]].all()


def test_per_query_filters_in_one_launch():
    N, D, k = 3 * T + 5, 80, 10
    codes, scales, q = P.make_q(N, D, 4, 43)
    live = np.ones(N, bool)
    live[::7] = False
    tags = (np.arange(N) % 11).astype(np.uint32)
    filt = np.array([[0, 0], [0xFFFFFFFF, 99], [0xFFFFFFFF, 5], [4, 4]], np.uint32)  # all, none, tags == 5, bit 2 set
    rs, rm, sc, ids = launch(codes, scales, q, k, live, tags, filt)
    assert (rs, rm) == (0, 0)
    assert (ids[1] == -1).all() and (sc[1] == -np.inf).all()
    assert (tags[ids[2]] == 5).all() and (tags[ids[3]] & 4 == 4).all() and live[ids[[0, 2, 3]]].all()
    for qi in range(4):
        _, _, s1, i1 = launch(codes, scales, q[qi:qi + 1], k, live, tags, filt[qi:qi + 1])
        assert np.array_equal(u32(s1[0]), u32(sc[qi])) and np.array_equal(i1[0], ids[qi])


def test_the_quantised_launcher_refuses_misuse_without_launching():
    codes, scales, q = P.make_q(40, 32, 2, 44)
    live, tags, filt = np.ones(40, bool), np.zeros(40, np.uint32), np.zeros((2, 2), np.uint32)
    seen = {}

    def refused(what, k=10, tags=tags, filt=filt, **kw):
        rs, rm, sc, ids = launch(codes, scales, q, k, live, tags, filt, **kw)
        assert rs != 0 and rm is None, what
        assert (sc == 7.0).all() and (ids == -7).all(), what  # nothing ran
        seen[what] = rs

    refused("D % 16", D=24, ldc=32)
    refused("D < 16", D=8, ldc=16)
    refused("D > 2048", D=2064, ldc=2064)
    refused("ldc < D", tweak=lambda p: setattr(p, "ldc", 16))
    refused("ldc % 16", tweak=lambda p: setattr(p, "ldc", 40))
    refused("scales null", tweak=lambda p: setattr(p, "scales", 0))
    refused("scales misaligned", tweak=lambda p: setattr(p, "scales", p.scales + 2))
    assert len(set(seen.values())) == 7, seen  # each new refusal has its own code
    refused("Q = 17", Q=17)
    refused("k = 129", k=129)
    refused("N = 0", N=0)
    refused("short cand", tweak=lambda p: setattr(p, "cand_bytes", p.cand_bytes - 8))
    refused("short live", tweak=lambda p: setattr(p, "live_bytes", 4))  # 40 rows need 2 words
    refused("filt without tags", tags=None)
    refused("live null", tweak=lambda p: setattr(p, "live", 0))
    refused("corpus misaligned", tweak=lambda p: setattr(p, "corpus", p.corpus + 8))
    assert len(set(seen.values())) >= 13, seen
    rs, rm, sc, ids = launch(codes, scales, q, 10, live, tags, filt)  # and the same buffers are accepted
    assert (rs, rm) == (0, 0) and np.array_equal(ids, P.ref_ids(codes, scales, q, 10, live))


def test_a_row_stride_above_d_and_replays_give_equal_bits():
    codes, scales, q = P.make_q(T + 3, 80, 3, 45)
    a = launch(codes, scales, q, 10)
    b = launch(codes, scales, q, 10, ldc=96)
    assert a[:2] == b[:2] == (0, 0)
    assert np.array_equal(u32(a[2]), u32(b[2])) and np.array_equal(a[3], b[3])
    codes, scales, q = P.make_q(3 * T + 5, 768, 16, 46)
    runs = [launch(codes, scales, q, 128) for _ in range(3)]
    for r in runs[1:]:
        assert r[:2] == (0, 0)
        assert np.array_equal(u32(r[2]), u32(runs[0][2])) and np.array_equal(r[3], runs[0][3])
