"""The filtered scan (csrc/search.hip, HZ_K_SEARCH_FSCAN) and the live GPU index (csrc/index.cpp) against the
fp64 oracle ``search_ref(allow=...)`` and the host ``RefIndex``.

Ids equal the oracle's exactly: tests/test_search_filter_cpu.py asserts on the host that every case here is
unambiguous over its passing rows. Scores are within the existing suite's bound ``gamma_D * sum |q_i c_i|``;
wherever two GPU runs are compared, they are compared bit for bit."""
import threading

import numpy as np
import pytest
import torch

from hipzap import search as S
from hipzap.ops import search as OS

import search_filter_cases as F
from search_filter_cases import T, make, plant
from test_search_gpu import launch as launch_unfiltered

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def launch(bits, q, k, live, tags=None, filt=None, N=None, tweak=None, fill=None):
    """Filtered scan + merge over device copies -> (scan rc, merge rc, scores [Q, k], ids [Q, k]). ``fill``: a
    uint16 pattern written over the dead rows first."""
    n, d = bits.shape
    host = bits.copy()
    if fill is not None:
        host[~np.asarray(live, bool)] = fill
    corpus = torch.from_numpy(host.view(np.int16)).to(DEV)
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV)
    Q = q.shape[0]
    nbytes = max(OS.scratch_bytes(n, Q, min(max(k, 1), 128)), 8)
    cand = torch.zeros(nbytes // 8, dtype=torch.int64, device=DEV)
    sc = torch.full((Q, max(k, 1)), 7.0, dtype=torch.float32, device=DEV)  # 7 / -7: "never written"
    ids = torch.full((Q, max(k, 1)), -7, dtype=torch.int32, device=DEV)
    words = S.pack_live(live)
    lv = torch.from_numpy(words.view(np.int32)).to(DEV)
    tg = None if tags is None else torch.from_numpy(np.ascontiguousarray(tags, np.uint32).view(np.int32)).to(DEV)
    fl = None if filt is None else torch.from_numpy(np.ascontiguousarray(filt, np.uint32).reshape(Q, 2).view(np.int32)).to(DEV)
    p = OS.FilterScanParams(corpus.data_ptr(), qd.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(),
                            n if N is None else N, d, Q, k, d, 0, nbytes, lv.data_ptr(),
                            0 if tg is None else tg.data_ptr(), 0 if fl is None else fl.data_ptr(), words.size * 4)
    if tweak:
        tweak(p)
    rc = OS.launch_filtered(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc[0], rc[1], sc.cpu().numpy(), ids.cpu().numpy()


def check(c32, q, k, allow, sc, ids):
    s, b, ri = F.allowed_oracle(c32, q, k, allow)
    assert np.array_equal(ids, ri), "ids differ from search_ref(allow=...)"
    for qi in range(q.shape[0]):
        for j in range(k):
            i = ids[qi, j]
            if i < 0:
                assert sc[qi, j] == -np.inf
            else:
                assert abs(float(sc[qi, j]) - s[qi, i]) <= b[qi, i], (qi, j, i, sc[qi, j], s[qi, i], b[qi, i])


@pytest.mark.parametrize("name", F.NAMES)
def test_filtered_topk_matches_the_oracle(name):
    bits, c32, q, k, live = F.build_case(name)
    rs, rm, sc, ids = launch(bits, q, k, live)
    assert (rs, rm) == (0, 0)
    check(c32, q, k, live, sc, ids)
    npass = int(live.sum())
    assert (ids[:, :min(k, npass)] >= 0).all() and (ids[:, npass:] == -1).all()
    if name.startswith("neg"):
        assert (sc[ids >= 0] < 0).all()  # neither padding nor a dead row outranks a negative score


@pytest.mark.parametrize("N,D,Q,k", [(3 * T + 5, 768, 16, 10), (T + 1, 72, 3, 128), (1, 8, 1, 1), (T, 2048, 3, 10)])
def test_all_live_without_filter_is_bitwise_the_unfiltered_scan(N, D, Q, k):
    bits, c32, q = make(N, D, Q, 11)
    a = launch_unfiltered(bits, q, k)
    b = launch(bits, q, k, np.ones(N, bool))
    c = launch(bits, q, k, np.ones(N, bool), tags=np.arange(N), filt=np.zeros((Q, 2)))  # mask 0, value 0: all pass
    for r in (b, c):
        assert a[:2] == r[:2] == (0, 0)
        assert np.array_equal(u32(a[2]), u32(r[2])) and np.array_equal(a[3], r[3])


def test_a_passing_score_has_the_unfiltered_scans_bits():
    N, D, Q = 100, 768, 3
    bits, c32, q = make(N, D, Q, 12)
    rng = np.random.default_rng(12)
    live, tags = rng.random(N) < 0.6, rng.integers(0, 4, N).astype(np.uint32)
    filt = np.array([[0, 0], [3, 1], [2, 2]], np.uint32)
    _, _, full_s, full_i = launch_unfiltered(bits, q, N)  # k = N <= 128: every row's unfiltered score
    rs, rm, sc, ids = launch(bits, q, 10, live, tags, filt)
    assert (rs, rm) == (0, 0)
    for qi in range(Q):
        allow = live & ((tags & filt[qi, 0]) == filt[qi, 1])
        assert allow.sum() >= 10 and set(ids[qi]) <= set(np.flatnonzero(allow))
        for j in range(10):
            at = int(np.flatnonzero(full_i[qi] == ids[qi, j])[0])
            assert u32(sc)[qi, j] == u32(full_s)[qi, at]
        want = [i for i in full_i[qi] if allow[i]][:10]  # the unfiltered order, restricted
        assert list(ids[qi]) == want


@pytest.mark.parametrize("pattern", [0x7FC0, 0x7F80, 0xFF80])
def test_what_a_dead_row_holds_never_reaches_a_result(pattern):
    N, D, Q, k = 2 * T + 9, 72, 3, 10
    bits, c32, q = make(N, D, Q, 13)
    live = np.random.default_rng(13).random(N) < 0.5
    live[T:T + 8] = False   # two whole groups of four rows
    live[2 * T:] = [True, False] * 4 + [False]
    tags = (np.arange(N) % 3).astype(np.uint32)
    filt = np.array([[0, 0], [3, 1], [3, 2]], np.uint32)
    for kw in ({}, {"tags": tags, "filt": filt}):
        zero = launch(bits, q, k, live, fill=0, **kw)
        bad = launch(bits, q, k, live, fill=pattern, **kw)
        assert zero[:2] == bad[:2] == (0, 0)
        assert np.array_equal(u32(zero[2]), u32(bad[2])) and np.array_equal(zero[3], bad[3])
        assert (bad[3] >= 0).all() and np.isfinite(bad[2]).all() and live[bad[3]].all()


def test_per_query_filters_in_one_launch():
    N, D, k = 3 * T + 5, 72, 10
    bits, c32, q = make(N, D, 4, 14)
    live = np.ones(N, bool)
    live[::7] = False
    tags = (np.arange(N) % 11).astype(np.uint32)
    filt = np.array([[0, 0], [0xFFFFFFFF, 99], [0xFFFFFFFF, 5], [4, 4]], np.uint32)  # all, none, tags == 5, bit 2 set
    rs, rm, sc, ids = launch(bits, q, k, live, tags, filt)
    assert (rs, rm) == (0, 0)
    assert (ids[1] == -1).all() and (sc[1] == -np.inf).all()
    assert (tags[ids[2]] == 5).all() and (tags[ids[3]] & 4 == 4).all() and live[ids[[0, 2, 3]]].all()
    for qi in range(4):
        _, _, s1, i1 = launch(bits, q[qi:qi + 1], k, live, tags, filt[qi:qi + 1])
        assert np.array_equal(u32(s1[0]), u32(sc[qi])) and np.array_equal(i1[0], ids[qi])


def test_the_filtered_launcher_refuses_misuse_without_launching():
    bits, c32, q = make(40, 16, 2, 9)
    live, tags, filt = np.ones(40, bool), np.zeros(40, np.uint32), np.zeros((2, 2), np.uint32)

    def refused(k=10, tweak=None, tags=tags, filt=filt, N=None):
        rs, rm, sc, ids = launch(bits, q, k, live, tags, filt, N=N, tweak=tweak)
        assert rs != 0 and rm is None
        assert (sc == 7.0).all() and (ids == -7).all()  # nothing ran

    refused(tweak=lambda p: setattr(p, "live", 0))
    refused(tweak=lambda p: setattr(p, "live", p.live + 2))
    refused(tweak=lambda p: setattr(p, "live_bytes", 4))       # 40 rows need 2 words
    refused(tags=None)                                           # a filter without tags
    refused(tweak=lambda p: setattr(p, "tags", p.tags + 1))
    refused(tweak=lambda p: setattr(p, "filt", p.filt + 2))
    refused(k=0)                                                 # the scan's own refusals still hold
    refused(k=129)
    refused(N=0)
    refused(tweak=lambda p: setattr(p, "D", 12))
    refused(tweak=lambda p: setattr(p, "Q", 17))
    refused(tweak=lambda p: setattr(p, "corpus", p.corpus + 2))
    refused(tweak=lambda p: setattr(p, "cand_bytes", p.cand_bytes - 8))
    refused(tweak=lambda p: setattr(p, "out_score", 0))
    rs, rm, sc, ids = launch(bits, q, 10, live, tags, filt)  # and the same buffers are accepted
    assert (rs, rm) == (0, 0) and np.array_equal(ids, S.search_ref(c32, q, 10)[1])


# ------------------------------------------------------------------------------------------ the index
def same(a, b):
    return np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1])


def within_bound(rows32, q, got):
    s, b, _, _ = F.oracle(rows32, q, got[1].shape[1])
    for qi in range(q.shape[0]):
        for j, i in enumerate(got[1][qi]):
            assert (got[0][qi, j] == -np.inf) if i < 0 else abs(float(got[0][qi, j]) - s[qi, i]) <= b[qi, i]


def test_add_delete_tags_and_filters_equal_refindex(tmp_path):
    A, B, q = F.index_data()
    path = str(tmp_path / "a.hzidx")
    S.write_index(path, A, "ip", tags=F.index_tags(F.IX_N))
    with S.Index(path, reserve=F.IX_N + 40) as ix, S.RefIndex(path) as ref:
        assert ix.describe()["capacity"] == 2 * T and not ix.describe()["filtered"]
        got, want = F.drive(ix, B, q), F.drive(ref, B, q)
        for g, w in zip(got, want):
            assert np.array_equal(g[1], w[1])
            within_bound(ref._rows, q, g)
        d = ix.describe()
        assert (d["count"], d["live"], d["tags"], d["filtered"]) == (F.IX_N + T, F.IX_N + T - 2, True, True)
        assert d["capacity"] >= d["count"] and d["capacity"] % T == 0
        with pytest.raises(ValueError, match="outside"):
            ix.delete([d["count"]])
        # save and reopen, and compact as RefIndex does
        keep, comp, rcomp = (str(tmp_path / n) for n in ("keep.hzidx", "comp.hzidx", "rcomp.hzidx"))
        ix.save(keep)
        ix.save(comp, compact=True)
        ref.save(rcomp, compact=True)
        last = ix.search(q, 10)
    assert np.array_equal(S.read_rows(comp), S.read_rows(rcomp)) and np.array_equal(S.read_tags(comp), S.read_tags(rcomp))
    assert S.read_live(comp).all() and S.read_header(comp)["count"] == S.read_header(rcomp)["count"]
    with S.Index(keep) as k2:
        assert k2.describe()["live"] == F.IX_N + T - 2 and k2.describe()["filtered"]
        assert same(k2.search(q, 10), last)
    with S.Index(comp) as c2, S.RefIndex(rcomp) as r2:
        assert c2.count == F.IX_N + T - 2
        g, w = c2.search(q, 10, filter=(0xFFFFFFFF, 3)), r2.search(q, 10, filter=(0xFFFFFFFF, 3))
        assert np.array_equal(g[1], w[1])


def test_add_gives_the_bits_of_a_fresh_index_of_the_union(tmp_path):
    A, B, q = F.index_data()
    pa, pab = str(tmp_path / "a.hzidx"), str(tmp_path / "ab.hzidx")
    S.write_index(pa, A, "cosine")
    S.write_index(pab, np.concatenate([A, B]), "cosine")
    qn = S.normalize_rows(q)
    with S.Index(pa) as ix, S.Index(pab) as fresh:
        ix.add(B)
        for k in (1, 10, 128):
            assert same(ix.search(qn, k), fresh.search(qn, k))
        assert np.array_equal(ix._state()[0], S.read_rows(pab))


@pytest.mark.parametrize("reserve", [2 * T, 0], ids=["tile_crossing", "growth"])
def test_no_stale_program_after_an_add(tmp_path, reserve):
    bits, c32, q = make(T - 6, 768, 1, 15)
    path = str(tmp_path / "a.hzidx")
    S.write_index(path, c32, "ip")
    with S.Index(path, contexts=1, reserve=reserve) as ix:
        ix.delete([0])  # the filtered program from the start
        first = ix.search(q, 10)
        assert same(ix.search(q, 10), first) and ix.describe()["programs"] == 1  # captured and replayed
        cap = ix.describe()["capacity"]
        new = make(12, 768, 1, 16)[1]
        new[9] = S.bf16_to_f32(S.to_bf16((q[0] * np.float32(3.0))[None]))[0]  # row T + 3 of the index: the next tile
        ids = ix.add(new)
        assert ids[9] == T + 3 and (ix.describe()["capacity"] > cap) == (reserve == 0)
        got = ix.search(q, 10)
        assert got[1][0, 0] == T + 3 and set(got[1][0, 1:]) <= set(first[1][0]) | set(ids.tolist())
        assert same(ix.search(q, 10), got)


def test_delete_hides_the_best_row_and_keeps_programs_and_bits(tmp_path):
    bits, c32, q = make(2 * T + 31, 72, 3, 17)
    path = str(tmp_path / "a.hzidx")
    S.write_index(path, c32, "ip")
    with S.Index(path) as ix:
        ix.set_tags([0], [1])
        before = ix.search(q, 10, filter=(0, 0))  # the filtered program of (3, 10)
        ix.search(q[:1], 10, filter=(0, 0))
        progs = ix.describe()["programs"]
        best = int(before[1][0, 0])
        assert ix.delete([best]) == 1 and ix.describe()["programs"] == progs
        after = ix.search(q, 11)
        for qi in range(3):
            keep = [j for j in range(10) if before[1][qi, j] != best]
            assert best not in after[1][qi]
            assert list(after[1][qi, :len(keep)]) == [before[1][qi, j] for j in keep]
            assert list(u32(after[0])[qi, :len(keep)]) == [u32(before[0])[qi, j] for j in keep]
        assert ix.delete([best]) == 0


def test_searches_are_constant_while_another_thread_mutates(tmp_path):
    bits, c32, q = make(2 * T + 31, 72, 2, 18)
    bits, c32 = plant(bits, q, {5: 3.0, T + 9: 2.5})
    bits, c32 = plant(bits, q[1:], {17: 3.0, 2 * T + 4: 2.5})
    path = str(tmp_path / "a.hzidx")
    S.write_index(path, c32, "ip")
    extra = make(16, 72, 1, 19)[1]
    with S.Index(path) as ix:  # the adds cross a tile boundary and then outgrow the capacity of 3 tiles
        ix.delete([1])
        want = [ix.search(q[:1], 2), ix.search(q[1:], 2)]
        assert list(want[0][1][0]) == [5, T + 9] and list(want[1][1][0]) == [17, 2 * T + 4]
        errs = []

        def searcher(t):
            try:
                for _ in range(60):
                    assert same(ix.search(q[t:t + 1], 2), want[t])
            except Exception as e:  # noqa: BLE001 - reported by the main thread
                errs.append(e)

        def mutator():
            try:
                for _ in range(20):
                    ids = ix.add(extra)
                    assert ix.delete(ids[:8]) == 8
                    ix.set_tags(ids[8:], [3] * 8)
            except Exception as e:  # noqa: BLE001
                errs.append(e)
        th = [threading.Thread(target=searcher, args=(0,)), threading.Thread(target=searcher, args=(1,)),
              threading.Thread(target=mutator)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        d = ix.describe()
        assert d["count"] == 2 * T + 31 + 320 and d["live"] == d["count"] - 1 - 160 and d["capacity"] > 3 * T
        assert same(ix.search(q[:1], 2), want[0])


def test_labels_that_spell_header_keys_and_the_first_mutation_drops_the_unfiltered_programs(tmp_path):
    bits, c32, q = make(T + 9, 72, 1, 22)
    path = str(tmp_path / "a.hzidx")
    labels = ["tags_off", "live_off", "capacity"] + [f"r{i}" for i in range(T + 6)]
    S.write_index(path, c32, "ip", labels=labels, tags=np.arange(T + 9) % 3)
    with S.Index(path, contexts=1) as ix:  # the native open reads the offsets, not the labels
        first = ix.search(q, 5)
        ix.search(q, 7)
        assert ix.describe()["programs"] == 2 and not ix.describe()["filtered"]
        victim = int(first[1][0, 4])
        assert ix.delete([victim]) == 1
        assert ix.describe()["programs"] == 0 and ix.describe()["filtered"]  # (Q, k, unfiltered) can never replay again
        after = ix.search(q, 4)
        assert np.array_equal(after[1], first[1][:, :4]) and np.array_equal(u32(after[0]), u32(first[0][:, :4]))
        assert ix.labels[1] == "live_off" and ix.describe()["programs"] == 1


# ------------------------------------------------------------------------------------------ the routes
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
    bits, c32, q = make(T - 3, 768, 3, 20, "pos")
    S.write_index(str(root / "c.hzidx"), c32, "ip", tags=(np.arange(T - 3) % 4).astype(np.uint32))
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["live"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={
        "embed": emb, "seq_len": 32, "plan": plan, "index": "c.hzidx", "index_writable": True, "index_reserve": 2 * T})
    srv = ModelServer(st, backend="gpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, srv, str(root / "c.hzidx"), q
    srv.close()
    app_mod.set_server(None)


def test_add_tag_search_and_delete_routes_equal_the_oracle(served):
    client, srv, path, q = served
    new = make(8, 768, 1, 21, "pos")[1] * np.float32(0.5)
    with S.RefIndex(path) as ref:
        def hits(**kw):
            r = client.post("/search", json=dict({"model": "live", "vectors": q.tolist(), "k": 10}, **kw))
            assert r.status_code == 200 and r.json["backend"] == "gpu", r.data
            return [[h["id"] for h in row] for row in r.json["results"]]
        assert hits() == ref.search(q, 10)[1].tolist()
        r = client.post("/index/add", json={"model": "live", "vectors": new.tolist(), "tags": [2] * 8})
        assert r.status_code == 200 and r.json["ids"] == list(range(T - 3, T + 5)), r.data  # crosses into the next tile
        ref.add(new, tags=[2] * 8)
        assert hits(tag=2) == ref.search(q, 10, filter=(0xFFFFFFFF, 2))[1].tolist()
        gone = [hits(tag=2)[0][0], T + 4]
        assert client.post("/index/delete", json={"model": "live", "ids": gone}).json["deleted"] == ref.delete(gone) == 2
        assert hits(tag=2) == ref.search(q, 10, filter=(0xFFFFFFFF, 2))[1].tolist()
        assert hits(filter={"mask": 1, "value": 1}) == ref.search(q, 10, filter=(1, 1))[1].tolist()
        assert hits() == ref.search(q, 10)[1].tolist()
        s, b, _, _ = F.oracle(ref._rows, q, 10)  # host: each of these answers is forced
        for allow in (ref._live, ref._live & (ref._tags == 2), ref._live & (ref._tags & 1 == 1)):
            assert F.subset_ambiguous(s, b, 10, allow) == 0
    assert isinstance(srv.index("live", srv.text("live")), S.Index)
