"""IVF indexes on the host: the version-5 file, the k-means build, ``RefIndex`` with ``nprobe``, the refusals, the
command line and the routes on the CPU backend; and that every query of tests/test_search_ivf_index_gpu.py is
forced (``search_ivf_cases.forced``), so the GPU test leaves no case out."""
import json

import numpy as np
import pytest

from hipzap import search as S
from hipzap.__main__ import main as cli

import search_ivf_cases as V
from search_ivf_cases import T


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The index-level scenario: (vectors, queries, the IVF file, the plain file of the same vectors and tags)."""
    d = tmp_path_factory.mktemp("ivf")
    v, q = V.clustered_data()
    ivf, plain = str(d / "ivf.hzidx"), str(d / "plain.hzidx")
    S.write_index(plain, v, "cosine", tags=V.index_tags())
    S.write_index(ivf, v, "cosine", tags=V.index_tags(), ivf=V.IX_LISTS, nprobe=2, ivf_seed=1)
    return v, q, ivf, plain


def test_version_5_round_trip_and_layout(files, tmp_path):
    v, q, path, plain = files
    hdr = S.read_header(path)
    t = S.read_ivf(path)
    assert hdr["count"] == V.IX_N and hdr["capacity"] % T == 0 and hdr["capacity"] >= 3 * T
    assert (hdr["ivf"]["nlist"], hdr["ivf"]["nprobe"], hdr["ivf"]["seed"], hdr["ivf"]["iters"]) == (V.IX_LISTS, 2, 1, 10)
    assert all(hdr["ivf"][k] % S.ALIGN == 0 for k in S.IVF_KEYS)
    rows, tags, live = S.read_rows(path), S.read_tags(path), S.read_live(path)
    assert rows.shape == (hdr["capacity"], V.IX_D) and live.sum() == V.IX_N
    # the stored bits are a plain index's; every row is in exactly one list, ascending in id; lists start on tiles
    real = t["rowid"] >= 0
    assert np.array_equal(live, real) and np.array_equal(np.sort(t["rowid"][real]), np.arange(V.IX_N))
    assert np.array_equal(rows[real], S.read_rows(plain)[t["rowid"][real]])
    assert np.array_equal(tags[real], V.index_tags()[t["rowid"][real]]) and not rows[~real].any() and not tags[~real].any()
    seen = 0
    for l in range(V.IX_LISTS):
        tiles = t["list_tiles"][t["list_off"][l]:t["list_off"][l + 1]]
        ids = t["rowid"].reshape(-1, T)[tiles].reshape(-1)
        n = int((ids >= 0).sum())
        assert (ids[:n] >= 0).all() and (ids[n:] == -1).all() and (np.diff(ids[:n]) > 0).all()
        assert np.array_equal(np.flatnonzero(t["list_of"] == l), ids[:n]) and tiles.size == -(-n // T)
        seen += n
    assert seen == V.IX_N
    # a row's list is the centroid of largest inner product; the same seed gives the same file
    c32, r32 = S.bf16_to_f32(t["centroids"]), S.bf16_to_f32(S.read_rows(plain))
    assert np.array_equal(t["list_of"], np.argmax(r32 @ c32.T, axis=1))
    again = str(tmp_path / "again.hzidx")
    S.write_index(again, v, "cosine", tags=V.index_tags(), ivf=V.IX_LISTS, nprobe=2, ivf_seed=1)
    assert open(again, "rb").read() == open(path, "rb").read()
    assert abs(np.linalg.norm(c32, axis=1) - 1).max() < 1e-2  # spherical k-means
    assert S.write_index(again, v, "ip", ivf=7)["ivf"]["nprobe"] == 7 and S.write_index(again, v, "ip", ivf=40)["ivf"]["nprobe"] == 16


def test_versions_1_to_4_are_byte_identical_around_an_ivf_write(tmp_path):
    v, _ = V.clustered_data()

    def write_all(tag):
        out = []
        for name, kw in (("v1", {}), ("v2", {"tags": V.index_tags()}), ("v3", {"dtype": "fp8"}),
                         ("v4", {"dtype": "fp8", "rescore": True, "tags": V.index_tags()})):
            p = str(tmp_path / f"{name}_{tag}.hzidx")
            S.write_index(p, v, "cosine", labels=[f"r{i}" for i in range(V.IX_N)], model="m", **kw)
            out.append(open(p, "rb").read())
        return out
    before = write_all("a")
    S.write_index(str(tmp_path / "ivf.hzidx"), v, "cosine", ivf=5)
    after = write_all("b")
    assert before == after
    assert [S.HEAD.unpack(b[:S.HEAD.size])[1] for b in before] == [1, 2, 3, 4]
    assert all(b"ivf" not in b[:4096] for b in before)


def test_refindex_over_every_list_equals_a_plain_refindex(files):
    v, q, path, plain = files
    with S.RefIndex(path) as ix, S.RefIndex(plain) as ref:
        def same(**kw):
            for k in (1, 10, 128):
                a, b = ix.search(q, k, nprobe="all", **kw), ref.search(q, k, **kw)
                assert np.array_equal(a[1], b[1]) and np.array_equal(u32(a[0]), u32(b[0]))
        same()
        same(filter=(0xFFFFFFFF, 3))
        a = ix.search(q, 10, nprobe=V.IX_LISTS)  # nprobe >= nlist is every list
        assert np.array_equal(a[1], ref.search(q, 10)[1])
        gone = [int(ref.search(q, 1)[1][0, 0]), 5]
        assert ix.delete(gone) == ref.delete(gone) == 2
        ix.set_tags([7, 8], [3, 3]), ref.set_tags([7, 8], [3, 3])
        same()
        same(filter=(0xFFFFFFFF, 3))
        assert ix.describe()["live"] == V.IX_N - 2 and ix.describe()["ivf"]["nlist"] == V.IX_LISTS


def test_probes_are_search_ref_over_the_centroids_and_restrict_the_answer(files):
    v, q, path, plain = files
    with S.RefIndex(path) as ix:
        cent = S.bf16_to_f32(S.read_ivf(path)["centroids"])
        for n in (1, 2, V.IX_LISTS):
            assert np.array_equal(ix.probes(q, n), S.search_ref(cent, q, n)[1])
        assert ix.probes(q, 2).dtype == np.int32 and ix.probes(q[0], 2).shape == (1, 2)
        for n in (1, 2):
            s, ids = ix.search(q, 10, nprobe=n)
            pr = ix.probes(q, n)
            for qi in range(q.shape[0]):
                near = np.isin(ix.ivf["list_of"], pr[qi])
                want = S.search_ref(ix._rows, q[qi:qi + 1], 10, near)[1][0]
                assert np.array_equal(ids[qi], want) and set(ix.ivf["list_of"][ids[qi][ids[qi] >= 0]]) <= set(pr[qi])
        assert np.array_equal(ix.search(q, 10)[1], ix.search(q, 10, nprobe=2)[1])  # None: the header's default
        ix.nprobe = 1
        assert np.array_equal(ix.search(q, 10)[1], ix.search(q, 10, nprobe=1)[1])


def test_every_query_of_the_gpu_index_test_is_forced(files):
    v, q, path, plain = files
    with S.RefIndex(path) as ix:
        for n in (1, 2):
            for k in (1, 10):
                assert V.forced(ix, q, k, n).all(), (n, k)
            assert V.forced(ix, q, 10, n, allow=ix._tags == 3).all()
        sizes = np.bincount(ix.ivf["list_of"], minlength=V.IX_LISTS)
        assert ix.header["capacity"] // T >= 3 and (sizes > 0).sum() >= 3
        ids = [int(i) for i in ix.search(q, 10, nprobe=1)[1][:, 0]]  # the GPU test re-tags these and filters on the tag
        ix.set_tags(ids, [77] * len(ids))
        assert V.forced(ix, q, 10, 1, allow=ix._tags == 77).all()


def test_write_refusals_name_the_value(tmp_path):
    v, _ = V.clustered_data()
    p = str(tmp_path / "x.hzidx")
    for bad in (0, -1, V.IX_N + 1, 70000, 2.5, True, "6"):
        with pytest.raises(ValueError, match="ivf must be an integer in 1..min"):
            S.write_index(p, v, "cosine", ivf=bad)
    with pytest.raises(ValueError, match=r"ivf=4 goes with dtype='bf16'"):
        S.write_index(p, v, "cosine", ivf=4, dtype="fp8")
    with pytest.raises(ValueError, match="rescore"):
        S.write_index(p, v, "cosine", ivf=4, dtype="fp8", rescore=True)
    for bad in (0, 5, 129, "all"):
        with pytest.raises(ValueError, match="nprobe must be an integer in 1..min"):
            S.write_index(p, v, "cosine", ivf=4, nprobe=bad)
    assert S.write_index(p, v[:300], "ip", ivf=300)["ivf"]["nlist"] == 300  # one list per row at the most


def test_search_and_mutation_refusals(files, tmp_path):
    v, q, path, plain = files
    with S.RefIndex(path) as ix, S.RefIndex(plain) as ref:
        for bad in (0, -1, 1.5, True, "some", [1]):
            with pytest.raises(ValueError, match="nprobe must be an integer in 1.."):
                ix.search(q, 10, nprobe=bad)
        for n in (1, "all"):
            with pytest.raises(ValueError, match="needs an IVF index"):
                ref.search(q, 10, nprobe=n)
        with pytest.raises(ValueError, match="needs an IVF index"):
            ref.probes(q, 1)
        with pytest.raises(ValueError, match="refine=16: an IVF index has no rescore rows"):
            ix.search(q, 10, refine=16)
        for bad in (0, V.IX_LISTS + 1, "all"):
            with pytest.raises(ValueError, match="nprobe must be an integer"):
                ix.probes(q, bad)
        with pytest.raises(ValueError, match="IVF indexes do not take add yet"):
            ix.add(v[:2])
        with pytest.raises(ValueError, match=r"IVF indexes do not take save\(compact=True\) yet"):
            ix.save(str(tmp_path / "c.hzidx"), compact=True)
        with pytest.raises(ValueError, match="outside"):
            ix.delete([V.IX_N])
        # save() writes version 5 again: the same tables, the mutations kept, ids unchanged
        ix.delete([11]), ix.set_tags([12], [77])
        out = str(tmp_path / "saved.hzidx")
        ix.save(out)
        want = ix.search(q, 10, nprobe=2)
    assert S.file_info(out)["version"] == 5 and S.file_info(out)["live"] == V.IX_N - 1
    a, b = S.read_ivf(out), S.read_ivf(path)
    assert all(np.array_equal(a[k], b[k]) for k in ("centroids", "list_off", "list_tiles", "rowid"))
    with S.RefIndex(out) as again:
        got = again.search(q, 10, nprobe=2)
        assert np.array_equal(got[1], want[1]) and np.array_equal(u32(got[0]), u32(want[0]))
        assert not again._live[11] and again._tags[12] == 77


def _corrupt(src, dst, key, index, value, dtype="<i4"):
    raw = bytearray(open(src, "rb").read())
    off = S.read_header(src)["ivf"][key] + index * np.dtype(dtype).itemsize
    raw[off:off + np.dtype(dtype).itemsize] = np.array([value], dtype).tobytes()
    open(dst, "wb").write(bytes(raw))


def test_the_reader_refuses_corrupt_tables(files, tmp_path):
    v, q, path, plain = files
    t = S.read_ivf(path)
    ntile = t["list_tiles"].size
    pad = int(np.flatnonzero(t["rowid"] < 0)[0])
    first = int(np.flatnonzero(t["rowid"] >= 0)[0])
    bad = str(tmp_path / "bad.hzidx")
    for key, index, value, msg in (
            ("list_off_off", 1, -1, "list_off does not rise"),
            ("list_off_off", V.IX_LISTS, ntile + 1, "list_off does not rise"),
            ("list_off_off", 0, 1, "list_off does not rise"),
            ("list_tiles_off", 0, ntile, "outside"),
            ("list_tiles_off", 0, -1, "outside"),
            ("list_tiles_off", 0, int(t["list_tiles"][1]), "names a tile twice"),
            ("rowid_off", pad, 0, "not a permutation"),
            ("rowid_off", first, -1, "not a permutation"),
            ("rowid_off", first, V.IX_N, "not a permutation"),
            ("rowid_off", first, int(t["rowid"][first + 1]), "not a permutation")):
        _corrupt(path, bad, key, index, value)
        with pytest.raises(ValueError, match=msg):
            S.RefIndex(bad)
    a, b = int(t["rowid"][first]), int(t["rowid"][first + 1])  # two ids of one list swapped: still a permutation
    raw = bytearray(open(path, "rb").read())
    off = S.read_header(path)["ivf"]["rowid_off"] + 4 * first
    raw[off:off + 8] = np.array([b, a], "<i4").tobytes()
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="do not ascend"):
        S.read_ivf(bad)
    hdr = S.read_header(path)
    open(bad, "wb").write(open(path, "rb").read()[:hdr["ivf"]["rowid_off"] + 8])  # a truncated table
    with pytest.raises(ValueError, match="ivf block rowid"):
        S.read_header(bad)
    raw = bytearray(open(plain, "rb").read())
    raw[8:12] = np.array([5], "<u4").tobytes()  # a version-5 head without the block
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="ivf block"):
        S.read_header(bad)


def test_cli_index_ivf_and_info(tmp_path, capsys):
    v, _ = V.clustered_data()
    vec, out = str(tmp_path / "v.npy"), str(tmp_path / "cli.hzidx")
    np.save(vec, v)
    cli(["index", "--vectors", vec, "--out", out, "--ivf", "6", "--nprobe", "3", "--ivf-seed", "4"])
    made = json.loads(capsys.readouterr().out)
    assert made["ivf"]["nlist"] == 6 and made["ivf"]["nprobe"] == 3 and made["ivf"]["seed"] == 4
    ref = str(tmp_path / "ref.hzidx")
    S.write_index(ref, v, "cosine", ivf=6, nprobe=3, ivf_seed=4)
    assert open(ref, "rb").read() == open(out, "rb").read()
    cli(["info", out])
    info = json.loads(capsys.readouterr().out)
    t = S.read_ivf(out)
    sizes = np.bincount(t["list_of"], minlength=6)
    assert info["version"] == 5 and info["ivf"]["nlist"] == 6 and info["ivf"]["empty_lists"] == int((sizes == 0).sum())
    assert info["ivf"]["largest_list"] == int(sizes.max()) and info["ivf"]["padding_rows"] == info["capacity"] - V.IX_N
    with pytest.raises(SystemExit, match="go with --ivf"):
        cli(["index", "--vectors", vec, "--out", out, "--nprobe", "3"])


# ------------------------------------------------------------------------------------------ the routes
@pytest.fixture()
def served(tmp_path, monkeypatch):
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings

    class Embedder:  # what the routes need of an embedding backend; the requests below carry their own vectors
        backend = "cpu"
        embed = {"dim": V.IX_D, "pooling": "mean", "normalize": True}
    v, q = V.clustered_data()
    S.write_index(str(tmp_path / "ivf.hzidx"), v, "cosine", tags=V.index_tags(), ivf=V.IX_LISTS, nprobe=2, ivf_seed=1)
    S.write_index(str(tmp_path / "plain.hzidx"), v, "cosine")
    st = Settings(default_model="resnet18", artifact_root=str(tmp_path))
    for name, extra in (("ivf", {"index": "ivf.hzidx", "index_writable": True}),
                        ("ivf1", {"index": "ivf.hzidx", "index_nprobe": 1}), ("plain", {"index": "plain.hzidx"})):
        st.models[name] = ModelSpec(name="bert-base", key="none.pth", extra=dict(extra, embed=Embedder.embed))
    srv = ModelServer(st, backend="cpu")
    monkeypatch.setattr(app_mod, "_embedding_backend", lambda s, model: Embedder)
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, q, str(tmp_path / "ivf.hzidx")
    srv.close()
    app_mod.set_server(None)


def test_routes_take_nprobe_and_refuse_what_an_ivf_index_cannot_do(served):
    client, q, path = served

    def post(route="/search", **kw):
        return client.post(route, json=dict({"model": "ivf", "vectors": q.tolist(), "k": 10}, **kw))

    def ids(r):
        assert r.status_code == 200, r.data
        return [[h["id"] for h in row] for row in r.json["results"]]
    with S.RefIndex(path) as ref:
        r = post()
        assert ids(r) == ref.search(q, 10, nprobe=2)[1].tolist() and r.json["ivf"] is True and r.json["nprobe"] == 2
        r = post(nprobe=1, tag=3)
        assert ids(r) == ref.search(q, 10, nprobe=1, filter=(0xFFFFFFFF, 3))[1].tolist() and r.json["nprobe"] == 1
        r = post(nprobe="all")
        assert ids(r) == ref.search(q, 10, nprobe="all")[1].tolist() and r.json["nprobe"] == "all"
        assert post(nprobe=V.IX_LISTS).json["nprobe"] == "all"
        r = post(model="ivf1")  # extra.index_nprobe overrides the header's 2
        assert ids(r) == ref.search(q, 10, nprobe=1)[1].tolist() and r.json["nprobe"] == 1
        for bad in (0, -3, V.IX_LISTS + 1, 1.5, "some", True, [2]):
            r = post(nprobe=bad)
            assert r.status_code == 400 and "nprobe" in r.json["message"], (bad, r.data)
        r = post(model="plain", nprobe=1)
        assert r.status_code == 400 and "IVF" in r.json["message"]
        r = post(model="plain")
        assert r.status_code == 200 and "ivf" not in r.json and "nprobe" not in r.json
        assert post(refine=16).status_code == 400
        r = client.post("/index/add", json={"model": "ivf", "vectors": q[:1].tolist()})
        assert r.status_code == 400 and "IVF indexes do not take add yet" in r.json["message"]
        gone = ids(post())[0][:2]
        r = client.post("/index/delete", json={"model": "ivf", "ids": gone})
        assert r.status_code == 200 and r.json["deleted"] == ref.delete(gone) == 2
        assert ids(post()) == ref.search(q, 10, nprobe=2)[1].tolist()
        assert client.post("/index/save", json={"model": "ivf"}).status_code == 200
    assert S.file_info(path)["version"] == 5 and S.file_info(path)["live"] == V.IX_N - 2
