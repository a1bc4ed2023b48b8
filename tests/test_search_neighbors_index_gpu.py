"""``Index.neighbors`` / ``knn_graph`` (csrc/index.cpp: hz_index_neighbors), ``POST /index/neighbors`` and ``hipzap knn``
on the GPU against the host ``RefIndex`` -- ids equal wherever the oracle's answer is forced under the bound of
tests/search_neighbors_cases.py, scores within it -- and against ``Index.search`` over the widened rows, an
independent kernel over the same exact products."""
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hipzap import search as S

import search_neighbors_cases as F
from search_neighbors_cases import T, make

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def agree(ix, ref, ids, k, include_self=False, need_all=False):
    """GPU ``neighbors`` against the oracle over the host index's rows -> (scores, ids, forced mask)."""
    ids = np.asarray(ids, np.int32)
    sc, near = ix.neighbors(ids, k, include_self=include_self)
    n = ref.count
    s, b, allow, rs, ri = F.oracle(ref._rows[:n], ids, k, ref._live[:n], not include_self)
    assert np.array_equal(ref.neighbors(ids, k, include_self=include_self)[1], ri)
    ok, _ = F.check_against_oracle(sc, near, s, b, allow, rs, ri, k)
    assert ok.all() or not need_all
    return sc, near, ok


@pytest.fixture()
def pair(tmp_path):
    A, B = F.index_data()
    path = str(tmp_path / "a.hzidx")
    S.write_index(path, A, "ip")
    with S.Index(path) as ix, S.RefIndex(path) as ref:
        yield ix, ref, A, B


def test_neighbors_and_knn_graph_equal_refindex_through_add_delete_and_growth(pair):
    ix, ref, A, B = pair
    ids = F.index_ids(80, F.IX_N)
    sc, near, _ = agree(ix, ref, ids, 10, need_all=True)
    agree(ix, ref, ids, 10, include_self=True)
    assert np.array_equal(ix.neighbors(int(ids[5]), 10)[1], near[5:6])
    ix.neighbors(ids, 10, ctx=0)
    programs = ix.describe()["programs"]  # context 0 holds the program of (80, 10, skip_self) now
    # a delete changes device data only: the row leaves the others' lists, asking for it raises, the programs stay
    gone = int(near[0, 0])
    assert ix.delete([gone]) == ref.delete([gone]) == 1
    same_n = np.where(ids == gone, ids[1] if ids[0] == gone else ids[0], ids)  # 80 ids again: the program of (80, 10, 1)
    assert gone not in ix.neighbors(same_n, 10, ctx=0)[1] and ix.describe()["programs"] == programs
    sc2, near2, _ = agree(ix, ref, same_n, 10)  # any context: it may capture that context's own program
    assert gone not in near2
    with pytest.raises(ValueError, match=f"id {gone} is deleted"):
        ix.neighbors([1, gone], 10)
    # an add inside the last tile keeps the programs, one across the tile boundary and past the capacity drops them
    for part in (B[:30], B[30:]):
        assert np.array_equal(ix.add(part), ref.add(part))
        live_ids = F.index_ids(80, ix.count)
        agree(ix, ref, live_ids[live_ids != gone], 10)
    assert ix.count == F.IX_N + T and ix.capacity() >= ix.count
    gi, gs = ix.knn_graph(10, block=200)
    ri, rs = ref.knn_graph(10)
    assert gi.shape == gs.shape == (ix.count, 10) and (gi[gone] == -1).all() and np.isneginf(gs[gone]).all()
    live = np.flatnonzero(ref._live)
    s, b, allow, os_, oi = F.oracle(ref._rows, live.astype(np.int32), 10, ref._live, True)
    ok, _ = F.check_against_oracle(gs[live], gi[live], s, b, allow, os_, oi, 10)
    assert np.array_equal(oi, ri[live]) and ok.sum() >= 0.9 * ok.size


def test_neighbors_equal_search_over_the_widened_rows_with_the_self_hit_removed(pair):
    ix, ref, A, B = pair
    ids = F.index_ids(80, F.IX_N)
    sc, near, ok = agree(ix, ref, ids, 10, need_all=True)
    s2, i2 = ix.search(A[ids], 11)  # forced at k + 1 too (tests/test_search_neighbors_cpu.py)
    for qi, a in enumerate(ids):
        keep = i2[qi] != a
        assert np.array_equal(i2[qi][keep][:10], near[qi]), (qi, a)


def test_n_above_the_per_pass_maximum_is_split_and_replays_are_bitwise_equal(pair):
    ix, ref, A, B = pair
    ids = F.index_ids(150, F.IX_N)
    whole = ix.neighbors(ids, 10)
    assert ix._lib.hz_index_neighbors_max(ix._h, 0) == 1024
    assert ix._lib.hz_index_neighbors_max(ix._h, 64) == 64  # a small maximum: 150 ids are three passes
    try:
        split = ix.neighbors(ids, 10)
        assert np.array_equal(u32(split[0]), u32(whole[0])) and np.array_equal(split[1], whole[1])
        out_s, out_i = np.empty((65, 10), np.float32), np.empty((65, 10), np.int32)
        rc = ix._lib.hz_index_neighbors(ix._h, 0, ids[:65].ctypes.data, 65, 10, 1, out_s.ctypes.data, out_i.ctypes.data)
        assert rc == -4 and b"1..64 ids a call, got 65" in ix._lib.hz_index_last_error()
    finally:
        assert ix._lib.hz_index_neighbors_max(ix._h, 1024) == 1024
    for _ in range(50):  # the captured program of (150, 10, skip_self)
        again = ix.neighbors(ids, 10)
        assert np.array_equal(u32(again[0]), u32(whole[0])) and np.array_equal(again[1], whole[1])
    k1 = ix.neighbors(ids, 1)
    assert np.array_equal(u32(k1[0][:, 0]), u32(whole[0][:, 0]))  # the same pair's bits at k = 1 and k = 10


def test_every_value_error_names_the_value(pair, tmp_path):
    ix, ref, A, B = pair
    with pytest.raises(ValueError, match=rf"id {F.IX_N} is outside \[0, {F.IX_N}\)"):
        ix.neighbors([0, F.IX_N])
    for k in (0, 129):
        with pytest.raises(ValueError, match="k must be an integer in 1..128"):
            ix.neighbors([0], k)
    fp8, ivf, odd = str(tmp_path / "q.hzidx"), str(tmp_path / "i.hzidx"), str(tmp_path / "o.hzidx")
    S.write_index(fp8, A, "ip", dtype="fp8")
    S.write_index(ivf, A, "ip", ivf=4)
    S.write_index(odd, make(20, 72, 1, 0)[1], "ip")
    out_s, out_i, one = np.empty((1, 3), np.float32), np.empty((1, 3), np.int32), np.zeros(1, np.int32)
    for p, msg, code in ((fp8, "an fp8_e4m3 index of version 3", -35), (ivf, "an IVF index of version 5", -35),
                         (odd, "dim % 32 == 0", -36)):
        with S.Index(p) as bad:
            with pytest.raises(ValueError, match=msg):
                bad.neighbors([0], 3)
            with pytest.raises(ValueError, match=msg):
                bad.knn_graph(3)
            rc = bad._lib.hz_index_neighbors(bad._h, 0, one.ctypes.data, 1, 3, 1, out_s.ctypes.data, out_i.ctypes.data)
            assert rc == code and msg.encode() in bad._lib.hz_index_last_error()


@pytest.fixture(scope="module")
def served(tmp_path_factory):
    from transformers import BertConfig, BertModel
    from hipzap.engine import plan as P
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    root = tmp_path_factory.mktemp("artifacts")
    torch.manual_seed(0)
    ckpt = str(root / "enc.pth")
    torch.save(BertModel(BertConfig(num_hidden_layers=1), add_pooling_layer=False).eval().state_dict(), ckpt)
    emb = {"pooling": "mean", "normalize": True}
    plan = P.export_from_checkpoint("bert-base", ckpt, batch=2, seq_len=32, embed=emb)
    _, c32, _ = make(T + 40, 768, 1, 41, "pos")
    S.write_index(str(root / "nb.hzidx"), c32, "ip", labels=[f"doc{i}" for i in range(T + 40)])
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["nb"] = ModelSpec(name="bert-base", key="enc.pth", batch=2,
                                extra={"embed": emb, "seq_len": 32, "plan": plan, "index": "nb.hzidx"})
    srv = ModelServer(st, backend="gpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, srv, str(root / "nb.hzidx")
    srv.close()
    app_mod.set_server(None)


def test_the_route_and_the_cli_on_the_gpu(served, tmp_path):
    client, srv, path = served
    ids = [T + 39, 7, 7, 0, T]
    with S.RefIndex(path) as ref:
        s, b, allow, rs, ri = F.oracle(ref._rows, np.asarray(ids, np.int32), 5, ref._live, True)
        must = F.forced(s, b, 5, allow)
        assert must.all()
        r = client.post("/index/neighbors", json={"model": "nb", "ids": ids, "k": 5})
        assert r.status_code == 200 and r.json["backend"] == "gpu", r.data
        got = np.asarray([[h["id"] for h in row] for row in r.json["results"]], np.int32)
        sc = np.asarray([[h["score"] for h in row] for row in r.json["results"]], np.float32)
        F.check_against_oracle(sc, got, s, b, allow, rs, ri, 5, must=must)
        assert [[h["label"] for h in row] for row in r.json["results"]] == [[f"doc{i}" for i in row] for row in ri]
        r = client.post("/index/neighbors", json={"model": "nb", "ids": ids, "k": 5}, headers={"Accept": "application/octet-stream"})
        out = np.load(io.BytesIO(r.data), allow_pickle=False)
        assert r.status_code == 200 and np.array_equal(out["id"], got) and np.array_equal(u32(out["score"]), u32(sc))
        for body, msg in (({"model": "nb", "ids": [T + 40]}, f"id {T + 40} is outside"), ({"model": "nb", "ids": [1], "k": 0}, "k must be")):
            r = client.post("/index/neighbors", json=body)
            assert r.status_code == 400 and msg in r.json["message"], r.data
        assert isinstance(srv.index("nb", srv.text("nb")), S.Index)
        g = str(tmp_path / "g.npz")
        r = subprocess.run([sys.executable, "-m", "hipzap", "knn", path, "--k", "5", "--out", g], capture_output=True, text=True,
                           cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
        assert r.returncode == 0 and json.loads(r.stdout)["backend"] == "gpu", r.stderr
        z = np.load(g)
        all_ids = np.arange(ref.count, dtype=np.int32)
        s, b, allow, rs, ri = F.oracle(ref._rows, all_ids, 5, ref._live, True)
        ok, _ = F.check_against_oracle(z["scores"], z["ids"], s, b, allow, rs, ri, 5)
        assert ok.sum() >= 0.9 * ok.size
