"""Bulk search on the host: ``split3`` (the batch scan's split of an fp32 query into three bf16 terms), the certificate,
``RefIndex.search_batch`` against ``RefIndex.search``, the oracle's share of forced slots for the GPU cases, the
refusals of kinds 44 and 45 (nothing is launched, so no GPU is needed), their Python mirrors and the route on the CPU
backend."""
import ctypes as C

import numpy as np
import pytest
import torch

from hipzap import _native as N
from hipzap import search as S
from hipzap.ops import search as OS

import search_batch_cases as F
from search_batch_cases import QB, T, make


def bits_of(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------- 1. the split
def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


SPLIT_VALUES = {
    "random": np.random.default_rng(0).standard_normal(4096).astype(np.float32) * np.float32(3.0),
    # every exponent from 2^-102 up, below which a term can fall under 2^-126 (the flush has its own test)
    "random_exponents": f32(np.random.default_rng(1).integers(0x0C800000, 0x7F800000, 4096, dtype=np.uint32)),
    "powers_of_two": np.ldexp(np.float32(1.0), np.arange(-110, 128)).astype(np.float32),
    "all_significand_bits": f32((np.arange(20, 254, dtype=np.uint32) << 23) | 0x7FFFFF),
    "zeros": f32([0x00000000, 0x80000000]),
    "largest": f32([0x7F7FFFFF, 0xFF7FFFFF]),
}


@pytest.mark.parametrize("name", sorted(SPLIT_VALUES))
def test_split3_is_exact_and_every_term_is_a_bf16_value(name):
    x = SPLIT_VALUES[name]
    x = np.concatenate([x, -x])
    h, m, l = S.split3(x)
    for t in (h, m, l):
        assert t.dtype == np.float32 and (bits_of(t) & 0xFFFF == 0).all()  # a bf16 value: the low 16 bits are zero
        assert ((bits_of(t) & 0x7F800000 != 0) | (bits_of(t) & 0x7FFFFFFF == 0)).all()  # normal, or a zero
        assert ((t == 0) | (np.signbit(t) == np.signbit(x))).all()  # no term opposes x, so |h| + |m| + |l| = |x'|
    assert np.array_equal(h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64), x.astype(np.float64))
    assert np.array_equal(bits_of(h) & 0x7FFFFFFF, bits_of(x) & 0x7FFF0000)  # h: the top 16 bits of x
    if name == "all_significand_bits":
        assert (m != 0).all() and (l != 0).all()  # all three terms are in use


def test_split3_flushes_each_term_whose_exponent_field_is_zero():
    """fp32 subnormals and values just above 2^-126: x' term by term."""
    tiny = np.float32(2.0 ** -126)
    # a subnormal: every term has a zero exponent field -> x' = 0 with the sign of x
    sub = f32([0x00000001, 0x007FFFFF, 0x00400000, 0x80000001, 0x807FFFFF])
    h, m, l = S.split3(sub)
    for t in (h, m, l):
        assert (bits_of(t) & 0x7FFFFFFF == 0).all()
    # 2^-126 * (1 + 2^-7 + 2^-23): h = 2^-126 * (1 + 2^-7) stays, x - h = 2^-149 is subnormal: m' = l' = 0
    x = f32([0x00810001])
    h, m, l = S.split3(x)
    assert bits_of(h)[0] == 0x00810000 and bits_of(m)[0] == 0 and bits_of(l)[0] == 0
    # 2^-110 * (1 + 2^-8 + 2^-16): three normal terms, the smallest one 2^-126 exactly -> kept, x' = x
    x = np.array([2.0 ** -110 * (1 + 2.0 ** -8 + 2.0 ** -16)], np.float32)
    h, m, l = S.split3(x)
    assert (h[0], m[0], l[0]) == (np.float32(2.0 ** -110), np.float32(2.0 ** -118), tiny)
    # one binade lower the last term is 2^-127: flushed, x' = h + m
    x = np.array([2.0 ** -111 * (1 + 2.0 ** -8 + 2.0 ** -16)], np.float32)
    h, m, l = S.split3(x)
    assert (h[0], m[0]) == (np.float32(2.0 ** -111), np.float32(2.0 ** -119)) and bits_of(l)[0] == 0
    assert abs(float(x[0]) - (float(h[0]) + float(m[0]) + float(l[0]))) < 2.0 ** -126  # what a flush can cost
    # from 2^-102 up no term of any value can be below 2^-126: 2^-102 * 2^-8 * 2^-8 * 2^-8
    big = f32(np.random.default_rng(2).integers(0x0C800000, 0x7F800000, 4096, dtype=np.uint32))
    h, m, l = S.split3(big)
    assert np.array_equal(h.astype(np.float64) + m + l, big.astype(np.float64))


# ------------------------------------------------------------------------------- 2. the certificate
def test_the_certificate_on_hand_built_scores():
    d = 64
    q = np.zeros((4, d), np.float32)
    q[:, 0] = 1.0
    E = S.batch_slack(q, "cosine")
    beta, gamma = F.beta(3 * d), F.gamma(d)
    assert E.shape == (4,) and np.allclose(E, (beta + gamma) * (1 + 2.0 ** -7), rtol=1e-12, atol=0)
    assert np.allclose(S.batch_slack(2 * q, "cosine"), 2 * E, rtol=1e-12) and S.batch_slack(q, "ip") is None
    t_k = np.float32([0.9, 0.9, 0.9, -np.inf])
    s_last = np.array([0.5, np.float32(0.9) - E[1] / 2, -np.inf, -np.inf])  # a clear gap, one smaller than E, fewer than R rows (twice)
    assert S.batch_certain(s_last, t_k, E).tolist() == [True, False, True, True]
    assert S.batch_certain(s_last, t_k, None).tolist() == [False, False, True, True]  # an ip index: the first clause only
    assert S.batch_certain([0.9 - E[0]], [0.9], E[:1]).tolist() == [False]  # s_R + E == t_k proves nothing
    assert S.batch_certain(np.float32([0.5]), np.float32([0.5]), E[:1]).tolist() == [False]  # a tie across the cut


def test_candidates_and_k_are_checked():
    assert [S.batch_candidates(k) for k in (1, 8, 10, 32, 33, 100, 128)] == [33, 40, 42, 128, 128, 128, 128]
    assert S.batch_candidates(10, 10) == 10 and S.batch_candidates(10, 128) == 128
    for bad in (9, 129, 0, 2.5, True, "40"):
        with pytest.raises(ValueError, match=r"candidates must be None or an integer in k\.\.128"):
            S.batch_candidates(10, bad)


# ------------------------------------------------------------------------------- 3. RefIndex
@pytest.fixture(scope="module")
def clustered(tmp_path_factory):
    rows, q = F.clustered()
    path = str(tmp_path_factory.mktemp("ix") / "c.hzidx")
    S.write_index(path, rows, "cosine")
    return path, rows, q


def test_refindex_search_batch_equals_search_id_for_id(clustered):
    path, rows, q = clustered
    with S.RefIndex(path) as ix:
        want_s, want_i = ix.search(q, 10)
        s, i, certain = ix.search_batch(q, 10, fallback=False)
        assert s.dtype == np.float32 and i.dtype == np.int32 and certain.dtype == bool and certain.shape == (F.IX_Q,)
        assert certain.sum() >= 1  # the GPU test needs a query certified without fallback
        assert np.array_equal(i[certain], want_i[certain]) and np.array_equal(s[certain], want_s[certain])
        s, i, certain = ix.search_batch(q, 10)
        assert certain.all() and np.array_equal(i, want_i) and np.array_equal(s, want_s)
        s, i, certain = ix.search_batch(q[:7], 3, candidates=3)  # R = k
        assert np.array_equal(i[certain], ix.search(q[:7], 3)[1][certain])
        assert ix.search_batch(q[0], 5)[1].shape == (1, 5)
        for k in (0, 129, 2.5, True):
            with pytest.raises(ValueError, match="k must be an integer in 1..128"):
                ix.search_batch(q, k)
        with pytest.raises(ValueError, match="candidates must be"):
            ix.search_batch(q, 10, candidates=9)
        with pytest.raises(ValueError, match=r"query vectors must be \[Q, 64\]"):
            ix.search_batch(q[:, :32], 10)
        gone = int(want_i[0, 0])
        ix.delete([gone])
        assert gone not in ix.search_batch(q[:1], 10)[1]


def test_more_ties_than_candidates_are_uncertain_until_the_fallback(tmp_path):
    rows, q = F.duplicated()
    path = str(tmp_path / "d.hzidx")
    S.write_index(path, rows, "cosine")
    with S.RefIndex(path) as ix:
        s, i, certain = ix.search_batch(q, 10, fallback=False)
        assert certain.tolist() == [False]
        s, i, certain = ix.search_batch(q, 10)
        assert certain.tolist() == [True] and np.array_equal(i, ix.search(q, 10)[1]) and i[0].tolist() == list(range(10))


def test_an_ip_index_certifies_only_when_every_row_was_a_candidate(tmp_path):
    _, c32, q = make(60, 64, 5, 3, "pos")
    path = str(tmp_path / "p.hzidx")
    S.write_index(path, c32, "ip")
    with S.RefIndex(path) as ix:
        assert not ix.search_batch(q, 10, fallback=False)[2].any()          # R = 42 < 60 rows: no bound, no proof
        s, i, certain = ix.search_batch(q, 10, candidates=128, fallback=False)  # fewer than R rows: proven
        assert certain.all() and np.array_equal(i, ix.search(q, 10)[1])


def test_refused_indexes_are_named(tmp_path):
    _, c32, q = make(300, 128, 1, 5)
    kinds = {"q": dict(dtype="fp8"), "b": dict(dtype="bin"), "i": dict(ivf=4), "qi": None}
    msgs = {"q": "an fp8_e4m3 index of version 3", "b": "a bin_sign index of version 8", "i": "an IVF index of version 5"}
    for name, msg in msgs.items():
        path = str(tmp_path / f"{name}.hzidx")
        S.write_index(path, c32, "ip", **kinds[name])
        with S.RefIndex(path) as ix:
            with pytest.raises(ValueError, match=f"search_batch is built for plain bf16 indexes .* {msg}"):
                ix.search_batch(q, 3)
    odd = str(tmp_path / "o.hzidx")
    S.write_index(odd, make(20, 72, 1, 0)[1], "ip")
    with S.RefIndex(odd) as ix:
        with pytest.raises(ValueError, match=r"search_batch needs dim % 32 == 0 .* got dim = 72"):
            ix.search_batch(np.zeros((1, 72), np.float32), 3)


# ------------------------------------------------------------------------------- 4. the GPU cases, from the oracle alone
def test_the_case_matrix_covers_what_the_kernel_can_get_wrong():
    assert {c[1] for c in F.CASES} == {300, 256} and {c[2] for c in F.CASES} == {32, 64, 768}
    assert {c[3] for c in F.CASES} == {1, QB, QB + 1, 2 * QB + 2} and {c[4] for c in F.CASES} == {1, 10, 64, 65, 128}
    assert T == 256 and QB == OS.SELF_QB


@pytest.mark.parametrize("name", F.NAMES)
def test_the_oracle_forces_all_but_two_percent_of_the_slots(name):
    s, b, rs, ri, forced = F.case_oracle(name)
    assert (~forced).mean() <= F.MAX_UNFORCED, (name, int((~forced).sum()), forced.size)


def test_the_exact_case_is_exact_and_uses_all_three_terms():
    bits, c32, q, dots = F.exact_case()
    h, m, l = S.split3(q)
    assert (h != 0).all() and (m != 0).all() and (l != 0).all()
    assert np.abs(q).max() < 2 ** 17 and np.abs(c32).max() <= 1 and q.shape[1] * 2 ** 17 <= 2 ** 23
    assert np.array_equal(dots.astype(np.float32).astype(np.int64), dots)
    x, mag = F.eff64(q)
    assert np.array_equal(x @ c32.astype(np.float64).T, dots.astype(np.float64))


# ------------------------------------------------------------------------------- 5. kinds and refusals
def test_kinds_44_and_45_are_mirrored():
    lib = N.lib()
    assert (N.HZ_K_SEARCH_XSCAN, N.HZ_K_SEARCH_RESCOREN) == (44, 45)
    assert lib.hz_kernel_name(44) == b"HZ_K_SEARCH_XSCAN" and lib.hz_kernel_name(45) == b"HZ_K_SEARCH_RESCOREN"
    assert N.KIND_STRUCT[44] is OS.BatchScanParams and N.KIND_STRUCT[45] is N.KIND_STRUCT[35] is OS.RescoreParams
    assert C.sizeof(OS.BatchScanParams) == lib.hz_kernel_param_size(44) == lib.hz_kernel_param_size(40)
    assert C.sizeof(OS.RescoreParams) == lib.hz_kernel_param_size(45)
    for name, _ in OS.SelfScanParams._fields_:  # kind 40 reads a batch block through the self scan's
        other = {"qid": "queries", "skip_self": "pad_"}.get(name, name)
        assert getattr(OS.SelfScanParams, name).offset == getattr(OS.BatchScanParams, other).offset or name == "pad_"


def _block(**kw):
    """A block that would launch, over made-up addresses: every test below breaks exactly one thing."""
    n, d, q, k = 300, 64, QB + 1, 10
    v = dict(corpus=0x10000, queries=0x20000, live=0x30000, cand=0x40000, out_score=0x50000, out_id=0x60000,
             live_bytes=4 * ((n + 31) // 32), cand_bytes=OS.self_scratch_bytes(n, q, k), N=n, D=d, Q=q, k=k, ldc=d, ntile=0)
    v.update(kw)
    return OS.BatchScanParams(**v)


SCAN_REFUSALS = [
    (-100, dict(corpus=0)), (-100, dict(queries=0)), (-100, dict(live=0)), (-100, dict(cand=0)),
    (-101, dict(D=72, ldc=72)), (-101, dict(D=40, ldc=40)), (-102, dict(D=0, ldc=0)), (-102, dict(D=-32)),
    (-103, dict(D=2080, ldc=2080)), (-104, dict(ldc=32)), (-104, dict(ldc=100)),
    (-105, dict(N=0)), (-105, dict(N=-1)), (-106, dict(Q=0)), (-106, dict(Q=65535 * QB + 1, cand_bytes=2 ** 62)),
    (-107, dict(k=0)), (-107, dict(k=129, cand_bytes=2 ** 40)),
    (-108, dict(corpus=0x10008)), (-108, dict(cand=0x40004)), (-108, dict(live=0x30001)),
    (-109, dict(live_bytes=4 * ((300 + 31) // 32) - 1)), (-109, dict(live_bytes=0)),
    (-110, dict(cand_bytes=2 * (QB + 1) * 10 * 8 - 1)), (-110, dict(cand_bytes=0)),
    (-111, dict(queries=0x20008)), (-111, dict(queries=0x20004)),
]


@pytest.mark.parametrize("code,kw", SCAN_REFUSALS)
def test_the_batch_scan_launcher_refuses(code, kw):
    p = _block(**kw)
    assert N.lib().hz_search_xscan_launch(C.byref(p), None) == code
    assert N.lib().hz_launch_kernel(N.HZ_K_SEARCH_XSCAN, C.byref(p), None) == code


def test_every_refusal_code_has_a_case_and_the_rescore_launchers_differ_in_q_only():
    assert {c for c, _ in SCAN_REFUSALS} == set(range(-111, -99))
    lib = N.lib()

    def block(**kw):
        v = dict(rows=0x10000, queries=0x20000, in_id=0x30000, out_score=0x50000, out_id=0x60000, N=300, D=64, Q=17, R=40, k=10, ldc=64)
        v.update(kw)
        return OS.RescoreParams(**v)
    for code, kw in ((-2, dict(D=68)), (-2, dict(ldc=32)), (-3, dict(N=0)), (-4, dict(Q=0)), (-4, dict(Q=65535 * QB + 1)),
                     (-30, dict(R=129)), (-30, dict(R=0)), (-31, dict(k=41)), (-31, dict(k=0)), (-32, dict(rows=0)),
                     (-32, dict(in_id=0)), (-33, dict(queries=0x20008)), (-33, dict(in_id=0x30002))):
        p = block(**kw)
        assert lib.hz_search_rescoren_launch(C.byref(p), None) == code, kw
        assert lib.hz_launch_kernel(N.HZ_K_SEARCH_RESCOREN, C.byref(p), None) == code, kw
    p = block()
    assert lib.hz_search_rescore_launch(C.byref(p), None) == -4  # Q <= 16 stays the rule of kind 35
    for code, kw in ((-2, dict(D=68, Q=16)), (-30, dict(R=129, Q=16)), (-31, dict(k=41, Q=16)), (-32, dict(rows=0, Q=16)),
                     (-33, dict(queries=0x20008, Q=16))):
        p = block(**kw)
        assert lib.hz_search_rescore_launch(C.byref(p), None) == code, kw


# ------------------------------------------------------------------------------- 6. the route
@pytest.fixture()
def served(tmp_path):
    from transformers import BertConfig, BertModel
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    root = tmp_path
    torch.manual_seed(0)
    torch.save(BertModel(BertConfig(num_hidden_layers=1), add_pooling_layer=False).eval().state_dict(), str(root / "enc.pth"))
    rows, q = F.clustered(n=300, d=768, nq=20)
    S.write_index(str(root / "c.hzidx"), rows, "cosine", labels=[f"doc{i}" for i in range(300)])
    S.write_index(str(root / "q.hzidx"), rows, "cosine", dtype="fp8")
    emb = {"pooling": "mean", "normalize": True}
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["c"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={"embed": emb, "seq_len": 32, "index": "c.hzidx"})
    st.models["q"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={"embed": emb, "seq_len": 32, "index": "q.hzidx"})
    srv = ModelServer(st, backend="cpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, q
    srv.close()
    app_mod.set_server(None)


def test_the_route_takes_batch_true_and_refuses_with_400(served):
    client, q = served
    plain = client.post("/search", json={"model": "c", "vectors": q.tolist(), "k": 5})
    r = client.post("/search", json={"model": "c", "vectors": q.tolist(), "k": 5, "batch": True})
    assert plain.status_code == r.status_code == 200, r.data
    assert r.json["results"] == plain.json["results"] and r.json["certain"] == [True] * 20 and r.json["batch"] is True
    assert "certain" not in plain.json and "batch" not in plain.json
    for body, msg in (({"model": "q", "vectors": q[:1].tolist(), "batch": True}, "an fp8_e4m3 index of version 3"),
                      ({"model": "c", "vectors": q[:1].tolist(), "batch": 1}, "batch must be true or false"),
                      ({"model": "c", "vectors": q[:1].tolist(), "batch": True, "tag": 1}, "batch takes no filter")):
        bad = client.post("/search", json=body)
        assert bad.status_code == 400 and msg in bad.json["message"], (body, bad.data)
