"""Two-stage search on the host: the version-4 ``.hzidx`` format, ``RefIndex.search(refine=)``, the seeds of the GPU
files' index cases (asserted forced here, on the oracles alone), and the routes and the CLI on the CPU backend."""
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from hipzap import search as S

import search_fp8_cases as P
import search_rescore_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def block(path, off, nbytes):
    with open(path, "rb") as f:
        f.seek(off)
        return f.read(nbytes)


# ------------------------------------------------------------------------------------------- format
def test_version_4_round_trip_and_its_blocks(tmp_path):
    v, tags, _ = R.covered_data()
    p4, p3, p1 = R.write_pair(tmp_path, v, tags=tags)
    h4, h3, h1 = S.read_header(p4), S.read_header(p3), S.read_header(p1)
    assert struct.unpack_from("<I", block(p4, 8, 4))[0] == 4 and h4["dtype"] == "fp8_e4m3" and h4["rescore"] == "bf16"
    assert h4["rescore_off"] % 4096 == 0 and h4["rescore_off"] >= h4["live_off"] + 4 * (-(-R.IX_N // 32))
    assert list(h4)[-3:] == ["rescore", "rescore_off", "data_off"]  # the new keys come last: version 3's stay where they were
    n, d = v.shape
    assert block(p4, h4["data_off"], n * d) == block(p3, h3["data_off"], n * d)          # codes
    for key, nbytes in (("scales_off", 4 * n), ("tags_off", 4 * n), ("live_off", 4 * (-(-n // 32)))):
        assert block(p4, h4[key], nbytes) == block(p3, h3[key], nbytes), key
    assert block(p4, h4["rescore_off"], 2 * n * d) == block(p1, h1["data_off"], 2 * n * d)
    assert np.array_equal(S.read_rescore_rows(p4), S.read_rows(p1)) and np.array_equal(S.read_rows(p4), S.read_rows(p3))
    assert np.array_equal(S.read_rescore_rows(p4), S.prepare_rows(v, "cosine"))
    assert S.file_info(p4)["version"] == 4 and S.file_info(p4)["rescore"] == "bf16" and S.file_info(p3)["version"] == 3
    with pytest.raises(ValueError, match="without rescore rows"):
        S.read_rescore_rows(p3)
    # without tags: scales, then the rescore block
    q4 = str(tmp_path / "plain4.hzidx")
    h = S.write_index(q4, v, "ip", dtype="fp8", rescore=True)
    assert "tags_off" not in h and h["rescore_off"] >= h["scales_off"] + 4 * n
    assert np.array_equal(S.read_rescore_rows(q4), S.to_bf16(v))
    with pytest.raises(ValueError, match="rescore rows go with an fp8 index"):
        S.write_index(str(tmp_path / "no.hzidx"), v, dtype="bf16", rescore=True)


def test_writing_without_rescore_is_unchanged(tmp_path):
    v, tags, _ = R.covered_data()
    for kw in ({}, {"tags": tags}, {"dtype": "fp8"}, {"dtype": "fp8", "tags": tags}):
        a, b = str(tmp_path / "a.hzidx"), str(tmp_path / "b.hzidx")
        ha, hb = S.write_index(a, v, **kw), S.write_index(b, v, rescore=False, **kw)
        assert ha == hb and open(a, "rb").read() == open(b, "rb").read()
        want = 3 if kw.get("dtype") else 2 if "tags" in kw else 1
        assert struct.unpack_from("<I", block(a, 8, 4))[0] == want and "rescore" not in ha and "rescore_off" not in ha


def rewrite(src, dst, version=None, edit=None, cut=None):
    """``src`` with another version word and / or an edited JSON header of the SAME length (offsets stay valid)."""
    raw = bytearray(open(src, "rb").read())
    head = list(S.HEAD.unpack_from(raw))
    if version is not None:
        head[1] = version
    if edit is not None:
        js = raw[S.HEAD.size:S.HEAD.size + head[2]].decode()
        new = edit(js)
        new = new[:-1] + " " * (len(js) - len(new)) + "}"  # a shorter value: blanks before the closing brace
        assert len(new) == len(js) and new != js, (js, new)
        raw[S.HEAD.size:S.HEAD.size + head[2]] = new.encode()
    S.HEAD.pack_into(raw, 0, *head)
    open(dst, "wb").write(bytes(raw[:cut] if cut else raw))
    return dst


def test_read_header_refusals(tmp_path):
    v, tags, _ = R.covered_data()
    p4, p3, _ = R.write_pair(tmp_path, v, tags=tags)
    h4 = S.read_header(p4)
    bad = str(tmp_path / "bad.hzidx")
    off = h4["rescore_off"]

    def refused(words, **kw):
        with pytest.raises(ValueError, match=words):
            S.read_header(rewrite(kw.pop("src", p4), bad, **kw))

    refused("version-4 file without rescore", src=p3, version=4)
    refused("version-4 file without rescore", edit=lambda js: js.replace('"rescore_off"', '"rescore_of_"'))
    refused("version-4 file without rescore", edit=lambda js: js.replace('"rescore": "bf16"', '"rescore": "fp16"'))
    refused("rescore keys in a version-3 file", version=3)
    refused("not a multiple of 4096", edit=lambda js: js.replace(f'"rescore_off": {off}', f'"rescore_off": {off + 8}'))
    refused("overlaps another block", edit=lambda js: js.replace(f'"rescore_off": {off}', f'"rescore_off": {h4["live_off"]}'))
    refused("overlaps another block", edit=lambda js: js.replace(f'"rescore_off": {off}', f'"rescore_off": {h4["data_off"]}'))
    refused("outside the file", cut=off + 2 * R.IX_N * R.IX_D - 2)
    assert S.read_header(rewrite(p4, bad)) == h4  # and the unedited copy is accepted


def test_convert_index_keeps_the_rows_as_the_rescore_block(tmp_path):
    v, tags, _ = R.covered_data()
    src, dst, plain = str(tmp_path / "s.hzidx"), str(tmp_path / "d.hzidx"), str(tmp_path / "p.hzidx")
    labels = [f"r{i}" for i in range(R.IX_N)]
    S.write_index(src, v, "cosine", labels=labels, tags=tags, model="m")
    ix = S.RefIndex(src, reserve=700)
    ix.delete([3, 77])
    ix.save()
    h = S.convert_index(src, dst, "fp8", rescore=True)
    S.convert_index(src, plain, "fp8")
    assert S.file_info(dst)["version"] == 4 and h["labels"] == labels and h["model"] == "m" and h["capacity"] == 700
    assert np.array_equal(S.read_rescore_rows(dst), S.read_rows(src))
    assert np.array_equal(S.read_rows(dst), S.read_rows(plain)) and np.array_equal(S.read_scales(dst), S.read_scales(plain))
    assert np.array_equal(S.read_tags(dst), S.read_tags(src)) and np.array_equal(S.read_live(dst), S.read_live(src))
    assert not S.read_live(dst)[[3, 77]].any() and S.read_live(dst).sum() == R.IX_N - 2
    with pytest.raises(ValueError, match="rescore rows go with an fp8 index"):
        S.convert_index(src, dst, "bf16", rescore=True)


# ------------------------------------------------------------------------------------------- RefIndex
def direct(ref, q, k, Rn, allow):
    """The two-stage answer computed directly in fp64 from the index's arrays."""
    s8, _ = P.oracle_q(ref._bits, ref.scales, q)
    c = ref._rrows.astype(np.float64)
    ids = np.full((q.shape[0], k), -1, np.int32)
    sc = np.full((q.shape[0], k), -np.inf)
    for qi in range(q.shape[0]):
        rows = np.flatnonzero(allow)
        cand = rows[np.argsort(-(s8[qi, rows] + 0.0), kind="stable")[:Rn]]
        s = c[cand] @ q[qi].astype(np.float64) + 0.0
        best = sorted(range(cand.size), key=lambda j: (-s[j], cand[j]))[:k]
        ids[qi, :len(best)], sc[qi, :len(best)] = cand[best], s[best]
    return sc, ids


def test_refindex_refine_against_a_direct_computation(tmp_path):
    v, q = R.clustered_data()
    p4, p3, p1 = R.write_pair(tmp_path, v)
    r4, r3, r1 = S.RefIndex(p4), S.RefIndex(p3), S.RefIndex(p1)
    assert r4.rescore and r4.version == 4 and not r3.rescore and r3.version == 3 and r1.version == 1
    for Rn in (10, 40, 128):
        sc, ids = r4.search(q, 10, refine=Rn)
        ds, di = direct(r4, q, 10, Rn, r4._live)
        assert np.array_equal(ids, di) and np.allclose(sc, ds, rtol=0, atol=1e-6)  # float32 of the same fp64 sums
    none, zero = r4.search(q, 10), r4.search(q, 10, refine=0)
    assert np.array_equal(none[1], r4.search(q, 10, refine=128)[1])       # None: R = 128
    assert np.array_equal(zero[1], r3.search(q, 10)[1]) and np.array_equal(zero[0], r3.search(q, 10)[0])  # 0: the fp8 answer
    for other in (r3, r1):  # any other index: None and 0 as before, everything else refused
        assert np.array_equal(other.search(q, 10, refine=None)[1], other.search(q, 10)[1])
        assert np.array_equal(other.search(q, 10, refine=0)[1], other.search(q, 10)[1])
        with pytest.raises(ValueError, match=f"{other.dtype} index of version {other.version}"):
            other.search(q, 10, refine=10)
    for badv in (9, 129, -1, 2.5, "x", True):
        with pytest.raises(ValueError, match="fp8_e4m3 index of version 4"):
            r4.search(q, 10, refine=badv)
    # live: delete and filters act in stage one, add writes both halves
    r4.delete(none[1][:, 0])
    assert not np.isin(r4.search(q, 10)[1], none[1][:, 0]).any()
    ids = r4.add(v[:3] * np.float32(1.0))
    assert r4._rbits.shape == (R.IX_N + 3, R.IX_D) and np.array_equal(r4._rbits[ids], S.prepare_rows(v[:3], "cosine"))
    out = str(tmp_path / "saved.hzidx")
    r4.save(out)
    assert S.file_info(out)["version"] == 4 and np.array_equal(S.read_rescore_rows(out), r4._rbits)
    r4.save(out, compact=True)
    assert S.file_info(out)["version"] == 4 and np.array_equal(S.read_rescore_rows(out), r4._rbits[r4._live])


def test_the_clustered_case_loses_under_fp8_what_rescoring_recovers(tmp_path):
    """The seeds of tests/test_search_rescore_index_gpu.py's cases, on the oracles alone."""
    v, q = R.clustered_data()
    p4, p3, p1 = R.write_pair(tmp_path, v)
    r4, r3, r1 = S.RefIndex(p4), S.RefIndex(p3), S.RefIndex(p1)
    fp8_ids, bf_ids = r3.search(q, 10)[1], r1.search(q, 10)[1]
    assert any(not np.array_equal(a, b) for a, b in zip(fp8_ids, bf_ids))  # fp8 loses the order inside a cluster
    assert R.forced(r4, q, 10, 128)   # bf16's top 10 inside fp8's top 128 by the margin, and unambiguous itself
    assert P.index_unambiguous(r3, q, 10)  # the fp8 answer is forced too: refine=0 can be compared by ids
    assert np.array_equal(r4.search(q, 10, refine=128)[1], bf_ids)
    # covered: 120 passing rows / 100 live rows, R = 128 covers them all
    v, tags, q = R.covered_data()
    p4, _, p1 = R.write_pair(tmp_path, v, tags=tags, name="cov")
    r4, r1 = S.RefIndex(p4), S.RefIndex(p1)
    assert int(r4.allow(S.check_filter(R.COVER_FILTER, 3))[0].sum()) == 120 and R.forced(r4, q, 10, 128, R.COVER_FILTER)
    assert np.array_equal(r4.search(q, 10, filter=R.COVER_FILTER)[1], r1.search(q, 10, filter=R.COVER_FILTER)[1])
    r4.delete(R.covered_deletes())
    assert int(r4._live.sum()) == 100 and R.forced(r4, q, 10, 128)


def test_the_live_scenario_is_forced_at_every_step(tmp_path):
    rows, q = R.live_data()
    p4 = str(tmp_path / "live4.hzidx")
    S.write_index(p4, rows[:R.LIVE_N0], "ip", tags=R.live_tags(R.LIVE_N0), dtype="fp8", rescore=True)
    ref = S.RefIndex(p4, reserve=256)
    steps = R.drive(ref, rows, q, tmp_path / "live_saved.hzidx",
                    on_step=lambda ix, k, filt: pytest.fail("ambiguous") if not R.forced(ix, q, k, 128, filt) else None)
    assert len(steps) == 8 and all((s[0][:, 0] >= 0).all() for s in steps)
    saved = str(tmp_path / "live_saved.hzidx")
    assert S.file_info(saved)["version"] == 4 and np.array_equal(S.read_rescore_rows(saved), ref._rbits)
    assert np.array_equal(S.read_rescore_rows(saved), S.to_bf16(rows))


# ------------------------------------------------------------------------------------------- routes, CLI
@pytest.fixture(scope="module")
def served(tmp_path_factory):
    import torch
    from transformers import BertConfig, BertModel
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    root = tmp_path_factory.mktemp("artifacts")
    torch.manual_seed(0)
    torch.save(BertModel(BertConfig(num_hidden_layers=1), add_pooling_layer=False).eval().state_dict(), str(root / "enc.pth"))
    rng = np.random.default_rng(5)
    corpus = rng.standard_normal((200, 768)).astype(np.float32)
    S.write_index(str(root / "v4.hzidx"), corpus, "cosine", dtype="fp8", rescore=True)
    S.write_index(str(root / "v3.hzidx"), corpus, "cosine", dtype="fp8")
    emb = {"pooling": "mean", "normalize": True}
    st = Settings(default_model="resnet18", artifact_root=str(root))
    for name in ("v4", "v3"):
        st.models[name] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={
            "embed": emb, "seq_len": 32, "index": str(root / f"{name}.hzidx"), "index_writable": True,
            "index_rescore_rows": "host"})
    srv = ModelServer(st, backend="cpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, str(root), corpus
    srv.close()
    app_mod.set_server(None)


def test_search_route_refine(served):
    client, root, corpus = served
    q = np.random.default_rng(6).standard_normal((2, 768)).astype(np.float32)
    ref = S.RefIndex(os.path.join(root, "v4.hzidx"))
    qn = S.normalize_rows(q)

    def ids(j):
        return [[h["id"] for h in row] for row in j["results"]]

    for body, Rn in (({}, 128), ({"refine": None}, 128), ({"refine": 40}, 40), ({"refine": 0}, 0), ({"refine": 5}, 5)):
        r = client.post("/search", json=dict(body, model="v4", vectors=q.tolist(), k=5))
        assert r.status_code == 200, r.data
        assert r.json["refine"] == Rn and r.json["dtype"] == "fp8_e4m3"
        assert ids(r.json) == ref.search(qn, 5, refine=Rn)[1].tolist()
    r = client.post("/search", json={"model": "v3", "vectors": q.tolist(), "k": 5})
    assert r.status_code == 200 and r.json["refine"] == 0
    assert client.post("/search", json={"model": "v3", "vectors": q.tolist(), "k": 5, "refine": 0}).json["refine"] == 0
    for model, val, words in (("v4", 4, "version 4"), ("v4", 129, "[k, 128]"), ("v4", "many", "fp8_e4m3 index"),
                              ("v4", 7.5, "refine must be"), ("v3", 10, "fp8_e4m3 index of version 3")):
        r = client.post("/search", json={"model": model, "vectors": q.tolist(), "k": 5, "refine": val})
        assert r.status_code == 400 and words in r.json["message"], r.data


def test_index_add_and_save_routes_on_a_version_4_index(served):
    client, root, corpus = served
    new = np.random.default_rng(7).standard_normal((3, 768)).astype(np.float32)
    r = client.post("/index/add", json={"model": "v4", "vectors": new.tolist()})
    assert r.status_code == 200 and r.json["ids"] == [200, 201, 202], r.data
    r = client.post("/search", json={"model": "v4", "vectors": new.tolist(), "k": 1})
    assert [row[0]["id"] for row in r.json["results"]] == [200, 201, 202] and r.json["refine"] == 128
    r = client.post("/index/save", json={"model": "v4"})
    assert r.status_code == 200 and r.json["count"] == 203, r.data
    path = os.path.join(root, "v4.hzidx")
    assert S.file_info(path)["version"] == 4
    assert np.array_equal(S.read_rescore_rows(path), S.prepare_rows(np.concatenate([corpus, new]), "cosine"))
    codes, scales = S.prepare_rows_fp8(np.concatenate([corpus, new]), "cosine")
    assert np.array_equal(S.read_rows(path), codes) and np.array_equal(S.read_scales(path), scales)


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "hipzap", *args], capture_output=True, text=True, cwd=ROOT, timeout=120)


def test_cli_rescore(tmp_path):
    v = np.random.default_rng(8).standard_normal((40, 32)).astype(np.float32)
    np.save(str(tmp_path / "v.npy"), v)
    out, conv, bf = str(tmp_path / "x.hzidx"), str(tmp_path / "y.hzidx"), str(tmp_path / "b.hzidx")
    r = _cli("index", "--vectors", str(tmp_path / "v.npy"), "--dtype", "fp8", "--rescore", "--out", out)
    assert r.returncode == 0, r.stderr
    j = json.loads(r.stdout)
    assert j["rescore"] == "bf16" and j["rescore_off"] % 4096 == 0 and j["dtype"] == "fp8_e4m3"
    assert np.array_equal(S.read_rescore_rows(out), S.prepare_rows(v, "cosine"))
    r = _cli("info", out)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["version"] == 4 and json.loads(r.stdout)["rescore"] == "bf16"
    S.write_index(bf, v)
    r = _cli("index", "--from-index", bf, "--dtype", "fp8", "--rescore", "--out", conv)
    assert r.returncode == 0, r.stderr
    assert S.file_info(conv)["version"] == 4 and np.array_equal(S.read_rescore_rows(conv), S.read_rows(bf))
    for extra in (["--vectors", str(tmp_path / "v.npy")], ["--from-index", bf]):
        r = _cli("index", *extra, "--dtype", "bf16", "--rescore", "--out", str(tmp_path / "no.hzidx"))
        assert r.returncode != 0 and "--rescore goes with --dtype fp8" in r.stderr and "already holds its rows in bf16" in r.stderr
        assert not os.path.exists(str(tmp_path / "no.hzidx"))
