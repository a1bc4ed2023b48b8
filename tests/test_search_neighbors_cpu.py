"""Neighbours of stored rows on the host: the oracle's shares of forced queries for the GPU cases, ``RefIndex.neighbors``
and ``knn_graph``, every refusal of the two launchers (nothing is launched, so no GPU is needed), the Python mirrors
of kinds 39 and 40, ``POST /index/neighbors`` on the CPU backend and ``hipzap knn --backend cpu``."""
import ctypes as C
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hipzap import _native as N
from hipzap import search as S
from hipzap.ops import search as OS

import search_neighbors_cases as F
from search_neighbors_cases import QB, T, make

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------- 1. the cases
def test_the_case_matrix_covers_what_the_kernel_can_get_wrong():
    assert {c[1] for c in F.CASES} >= {1, 10, T - 1, T, T + 1, 3 * T + 5}
    assert {c[2] for c in F.CASES} == {32, 96, 768, 2048}
    assert {c[3] for c in F.CASES} == {1, QB - 1, QB, QB + 1, 2 * QB + 3}
    assert {c[4] for c in F.CASES} == {1, 10, 128} and {c[7] for c in F.CASES} == {0, 1}
    assert {c[6] for c in F.CASES} == {"all", "one_dead", "dead_group", "dead_tile", "alternating"}
    assert any(c[1] == c[4] for c in F.CASES)  # N = k
    for name in F.NAMES:
        bits, c32, qid, k, live, skip, kind = F.build_case(name)
        assert live[qid].all() and qid.dtype == np.int32
        if len(qid) >= 4:
            rows = np.flatnonzero(live)
            assert qid[0] == rows[-1] and qid[-1] == rows[0] and qid[1] == qid[2]
    # D = 2048 and k = 128 use the "pos" kinds: random data is mostly ambiguous under this bound there
    assert all(c[5] != "normal" for c in F.CASES if c[2] == 2048 or c[4] == 128)


@pytest.mark.parametrize("name", F.NAMES)
def test_the_oracle_forces_enough_queries(name):
    """From the oracle alone: "pos" / "neg" corpora force every query, "normal" ones at D <= 768 and k <= 10 at least
    half -- a bad seed fails here and not on the GPU."""
    bits, c32, qid, k, live, skip, kind = F.build_case(name)
    s, b, allow, rs, ri = F.case_oracle(name)
    ok = F.forced(s, b, k, allow)
    if kind == "normal":
        assert c32.shape[1] <= 768 and k <= 10 and 2 * ok.sum() >= ok.size, (name, int(ok.sum()), ok.size)
    else:
        assert ok.all(), (name, int(ok.sum()), ok.size)


def test_the_planted_pair_and_the_index_scenario_are_forced():
    bits, c32, a, b = F.planted_pair()
    live = np.ones(bits.shape[0], bool)
    qid = np.array([a, b], np.int32)
    for skip in (0, 1):
        s, bb, allow, rs, ri = F.oracle(c32, qid, 10, live, skip)
        assert F.forced(s, bb, 10, allow, allow_ties=True).all()
        assert not F.forced(s, bb, 10, allow).all() or skip  # with the query in its own list the pair is an exact tie
        assert (ri[:, :2].tolist() == [[a, b], [a, b]]) if not skip else (ri[0, 0] == b and ri[1, 0] == a)
    A, B = F.index_data()
    c32 = np.concatenate([A, B])
    for count in (F.IX_N, F.IX_N + 30, F.IX_N + T):
        live = np.ones(count, bool)
        qid = F.index_ids(80, count)
        for k in (10, 11):  # 11: the cross-check against search(k + 1)
            s, bb, allow, rs, ri = F.oracle(c32[:count], qid, k, live, 1)
            assert F.forced(s, bb, k, allow).all(), (count, k)


# ------------------------------------------------------------------------------- 2. RefIndex
@pytest.fixture()
def plain(tmp_path):
    A, B = F.index_data()
    path = str(tmp_path / "a.hzidx")
    S.write_index(path, A, "ip", labels=[f"row{i}" for i in range(F.IX_N)])
    return path, A, B


def test_refindex_neighbors_is_search_ref_over_the_stored_rows(plain):
    path, A, B = plain
    with S.RefIndex(path) as ix:
        ids = F.index_ids(70, F.IX_N)
        sc, near = ix.neighbors(ids, 10)
        assert sc.dtype == np.float32 and near.dtype == np.int32 and sc.shape == near.shape == (70, 10)
        s, b, allow, rs, ri = F.oracle(A, ids, 10, np.ones(F.IX_N, bool), 1)
        assert np.array_equal(near, ri) and np.array_equal(sc, rs.astype(np.float32))
        assert not (near == ids[:, None]).any()
        sc2, near2 = ix.neighbors(ids, 10, include_self=True)
        assert np.array_equal(near2, S.search_ref(A, A[ids], 10)[1])
        big = int(np.argmax((A.astype(np.float64) ** 2).sum(axis=1)))  # the largest row is its own best neighbour
        assert ix.neighbors([big], 3, include_self=True)[1][0, 0] == big and big not in ix.neighbors([big], 3)[1]
        one = ix.neighbors(int(ids[3]), 4)
        assert np.array_equal(one[1], near[3:4, :4])
        assert ix.neighbors([], 3)[0].shape == (0, 3)
        # delete: the row leaves the others' lists, and asking for it raises
        gone = int(near[0, 0])
        assert ix.delete([gone]) == 1
        assert gone not in ix.neighbors(ids[:1], 10)[1]
        with pytest.raises(ValueError, match=f"id {gone} is deleted"):
            ix.neighbors([5, gone], 10)


def test_refindex_knn_graph(plain):
    path, A, B = plain
    with S.RefIndex(path) as ix:
        ix.delete([3, F.IX_N - 1])
        ids, scores = ix.knn_graph(5, block=100)
        assert ids.shape == scores.shape == (F.IX_N, 5) and ids.dtype == np.int32 and scores.dtype == np.float32
        assert (ids[[3, F.IX_N - 1]] == -1).all() and np.isneginf(scores[[3, F.IX_N - 1]]).all()
        live = np.flatnonzero(ix._live)
        want = ix.neighbors(live, 5)
        assert np.array_equal(ids[live], want[1]) and np.array_equal(scores[live], want[0])
        assert not np.isin(ids, [3, F.IX_N - 1]).any() and not (ids[live] == live[:, None]).any()
        assert np.array_equal(ix.knn_graph(5)[0], ids)
        with pytest.raises(ValueError, match="block"):
            ix.knn_graph(5, block=0)


def test_every_value_error_names_the_value(plain, tmp_path):
    path, A, B = plain
    with S.RefIndex(path) as ix:
        with pytest.raises(ValueError, match=rf"id {F.IX_N} is outside \[0, {F.IX_N}\)"):
            ix.neighbors([0, F.IX_N])
        with pytest.raises(ValueError, match=r"id -1 is outside"):
            ix.neighbors([-1])
        for k in (0, 129, 2.5, True):
            with pytest.raises(ValueError, match="k must be an integer in 1..128"):
                ix.neighbors([0], k)
        with pytest.raises(ValueError, match="k must be"):
            ix.knn_graph(0)
    fp8, ivf, odd = str(tmp_path / "q.hzidx"), str(tmp_path / "i.hzidx"), str(tmp_path / "o.hzidx")
    S.write_index(fp8, A, "ip", dtype="fp8")
    S.write_index(ivf, A, "ip", ivf=4)
    S.write_index(odd, make(20, 72, 1, 0)[1], "ip")
    for p, msg in ((fp8, "an fp8_e4m3 index of version 3"), (ivf, "an IVF index of version 5"),
                   (odd, r"dim % 32 == 0 .* got dim = 72")):
        with S.RefIndex(p) as ix:
            with pytest.raises(ValueError, match=msg):
                ix.neighbors([0], 3)
            with pytest.raises(ValueError, match=msg):
                ix.knn_graph(3)


# ------------------------------------------------------------------------------- 3. kinds and refusals
def test_kinds_39_and_40_are_mirrored():
    lib = N.lib()
    assert (N.HZ_K_SEARCH_MSCAN, N.HZ_K_SEARCH_MERGEN) == (39, 40)
    assert lib.hz_kernel_name(39) == b"HZ_K_SEARCH_MSCAN" and lib.hz_kernel_name(40) == b"HZ_K_SEARCH_MERGEN"
    assert N.KIND_STRUCT[39] is N.KIND_STRUCT[40] is OS.SelfScanParams
    assert C.sizeof(OS.SelfScanParams) == lib.hz_kernel_param_size(39) == lib.hz_kernel_param_size(40)
    assert OS.SELF_QB == QB and OS.SELF_MAX_Q == 65535 * QB and OS.INDEX_SELF_MAX_Q == S.NEIGHBORS_BLOCK == 1024
    assert OS.self_scratch_bytes(3 * T + 5, 2 * QB + 3, 10) == 4 * (2 * QB + 3) * 10 * 8
    for bad in ((0, 1, 1), (2 ** 31, 1, 1), (1, 0, 1), (1, OS.SELF_MAX_Q + 1, 1), (1, 1, 0), (1, 1, 129)):
        assert OS.self_scratch_bytes(*bad) == 0, bad
    assert OS.self_scratch_bytes(2 ** 31 - 1, OS.SELF_MAX_Q, 128) == 2 ** 23 * OS.SELF_MAX_Q * 128 * 8


def _block(**kw):
    """A block that would launch, over made-up addresses: every test below breaks exactly one thing, so the launcher
    answers before anything reaches a device."""
    n, d, q, k = 3 * T + 5, 96, QB + 1, 10
    v = dict(corpus=0x10000, qid=0x20000, live=0x30000, cand=0x40000, out_score=0x50000, out_id=0x60000,
             live_bytes=4 * ((n + 31) // 32), cand_bytes=OS.self_scratch_bytes(n, q, k), N=n, D=d, Q=q, k=k, ldc=d, ntile=0,
             skip_self=1, pad_=0)
    v.update(kw)
    return OS.SelfScanParams(**v)


SCAN_REFUSALS = [
    (-50, dict(corpus=0)), (-50, dict(qid=0)), (-50, dict(live=0)), (-50, dict(cand=0)),
    (-51, dict(D=72, ldc=72)), (-51, dict(D=40, ldc=40)), (-52, dict(D=0, ldc=0)), (-52, dict(D=-32)),
    (-53, dict(D=2080, ldc=2080)), (-54, dict(ldc=64)), (-54, dict(ldc=100)),
    (-55, dict(N=0)), (-55, dict(N=-1)), (-56, dict(Q=0)), (-56, dict(Q=65535 * QB + 1, cand_bytes=2 ** 62)),
    (-57, dict(k=0)), (-57, dict(k=129, cand_bytes=2 ** 40)),
    (-58, dict(corpus=0x10008)), (-58, dict(cand=0x40004)), (-58, dict(qid=0x20002)), (-58, dict(live=0x30001)),
    (-59, dict(live_bytes=4 * ((3 * T + 5 + 31) // 32) - 1)), (-59, dict(live_bytes=0)),
    (-60, dict(cand_bytes=4 * (QB + 1) * 10 * 8 - 1)), (-60, dict(cand_bytes=0)),
]
MERGE_REFUSALS = [
    (-50, dict(cand=0)), (-50, dict(out_score=0)), (-50, dict(out_id=0)),
    (-55, dict(N=0)), (-56, dict(Q=0)), (-56, dict(Q=65535 * QB + 1, cand_bytes=2 ** 62)), (-57, dict(k=0)), (-57, dict(k=129)),
    (-58, dict(cand=0x40004)), (-58, dict(out_score=0x50002)), (-58, dict(out_id=0x60001)),
    (-60, dict(cand_bytes=4 * (QB + 1) * 10 * 8 - 1)),
]


@pytest.mark.parametrize("code,kw", SCAN_REFUSALS)
def test_the_self_scan_launcher_refuses(code, kw):
    p = _block(**kw)
    assert N.lib().hz_search_mscan_launch(C.byref(p), None) == code
    assert N.lib().hz_launch_kernel(N.HZ_K_SEARCH_MSCAN, C.byref(p), None) == code


@pytest.mark.parametrize("code,kw", MERGE_REFUSALS)
def test_the_merge_launcher_refuses(code, kw):
    p = _block(**kw)
    assert N.lib().hz_search_mergen_launch(C.byref(p), None) == code
    assert N.lib().hz_launch_kernel(N.HZ_K_SEARCH_MERGEN, C.byref(p), None) == code


def test_every_refusal_code_has_a_case_and_kind_32_keeps_its_limit():
    assert {c for c, _ in SCAN_REFUSALS} == set(range(-60, -49))
    assert {c for c, _ in MERGE_REFUSALS} == {-50, -55, -56, -57, -58, -60}
    p = OS.SearchParams(0x10000, 0x20000, 0x40000, 0x50000, 0x60000, 3 * T + 5, 96, 17, 10, 96, 0, 2 ** 40)
    assert N.lib().hz_search_merge_launch(C.byref(p), None) == -4  # Q <= 16 stays the rule of kind 32


# ------------------------------------------------------------------------------- 4. route and CLI
@pytest.fixture()
def served(tmp_path):
    from transformers import BertConfig, BertModel
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    root = tmp_path
    torch.manual_seed(0)
    torch.save(BertModel(BertConfig(num_hidden_layers=1), add_pooling_layer=False).eval().state_dict(), str(root / "enc.pth"))
    _, c32, _ = make(60, 768, 1, 41, "pos")
    S.write_index(str(root / "nb.hzidx"), c32, "ip", labels=[f"doc{i}" for i in range(60)])
    S.write_index(str(root / "q.hzidx"), c32, "ip", dtype="fp8")
    emb = {"pooling": "mean", "normalize": True}
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["nb"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={"embed": emb, "seq_len": 32, "index": "nb.hzidx"})
    st.models["q"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={"embed": emb, "seq_len": 32, "index": "q.hzidx"})
    st.models["bare"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={"embed": emb, "seq_len": 32})
    srv = ModelServer(st, backend="cpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, srv, str(root / "nb.hzidx")
    srv.close()
    app_mod.set_server(None)


def test_the_route_answers_in_both_shapes_and_refuses_with_400(served):
    client, srv, path = served
    assert "POST /index/neighbors" in client.get("/").json["routes"]
    ids = [59, 7, 7, 0]
    with S.RefIndex(path) as ref:
        want_s, want_i = ref.neighbors(ids, 4)
        r = client.post("/index/neighbors", json={"model": "nb", "ids": ids, "k": 4})  # a read-only index serves it
        assert r.status_code == 200, r.data
        j = r.json
        assert (j["model"], j["backend"], j["k"], j["include_self"], j["count"], j["ids"]) == ("nb", "cpu", 4, False, 60, ids)
        assert [[h["id"] for h in row] for row in j["results"]] == want_i.tolist()
        assert [[h["label"] for h in row] for row in j["results"]] == [[f"doc{i}" for i in row] for row in want_i]
        assert np.array_equal(np.asarray([[h["score"] for h in row] for row in j["results"]], np.float32), want_s)
        r = client.post("/index/neighbors", json={"model": "nb", "ids": ids, "include_self": True},
                        headers={"Accept": "application/octet-stream"})
        assert r.status_code == 200 and r.mimetype == "application/octet-stream"
        out = np.load(io.BytesIO(r.data), allow_pickle=False)
        s2, i2 = ref.neighbors(ids, 10, include_self=True)
        assert out.shape == (4, 10) and np.array_equal(out["id"], i2) and np.array_equal(out["score"], s2)
        assert client.post("/index/neighbors?k=3", json={"model": "nb", "ids": [1]}).json["k"] == 3
    for body, msg in (({"model": "nb", "ids": [60]}, "id 60 is outside [0, 60)"),
                      ({"model": "nb", "ids": [1], "k": 129}, "k must be an integer in 1..128"),
                      ({"model": "nb", "ids": []}, "ids must be a non-empty list of integers"),
                      ({"model": "nb", "ids": [1.5]}, "ids must be a non-empty list of integers"),
                      ({"model": "nb", "ids": [1], "include_self": 1}, "include_self must be true or false"),
                      ({"model": "q", "ids": [1]}, "an fp8_e4m3 index of version 3"),
                      ({"model": "bare", "ids": [1]}, "is served without extra.index")):
        r = client.post("/index/neighbors", json=body)
        assert r.status_code == 400 and msg in r.json["message"], (body, r.data)


def test_hipzap_knn_on_the_cpu_backend(plain, tmp_path):
    path, A, B = plain
    out = str(tmp_path / "g.npz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "hipzap", "knn", path, "--k", "6", "--out", out, "--backend", "cpu", "--block", "100"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout)
    assert (info["count"], info["k"], info["backend"], info["rows_with_neighbors"]) == (F.IX_N, 6, "cpu", F.IX_N)
    g = np.load(out)
    with S.RefIndex(path) as ix:
        ids, scores = ix.knn_graph(6)
    assert sorted(g.files) == ["ids", "scores"] and np.array_equal(g["ids"], ids) and np.array_equal(g["scores"], scores)
    r = subprocess.run([sys.executable, "-m", "hipzap", "knn", path, "--k", "0", "--out", out, "--backend", "cpu"],
                       capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode != 0 and "k must be an integer in 1..128" in r.stderr
