"""fp8 vector indexes without a GPU: the e4m3fn encoder and decoder against torch, the quantiser's error bound,
the version-3 ``.hzidx`` file, ``RefIndex`` on it, ``convert_index``, the CLI and the CPU backend's routes. Also
asserts, on the host, that every case of the fp8 GPU tests is unambiguous over its passing rows under twice the
bound ``gamma(D + 1) * |scale_r| * sum_i |q_i c_ri|``."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from hipzap import search as S

import search_filter_cases as F
import search_fp8_cases as P
from search_fp8_cases import T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINITE = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)


def _torch_e4m3(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------ 1. the encoder
def test_encoder_and_decoder_equal_torch_bit_for_bit():
    val = torch.from_numpy(FINITE.copy()).view(torch.float8_e4m3fn).float().numpy()
    assert FINITE.size == 254 and np.array_equal(u32(S.e4m3_to_f32(FINITE)), u32(val))
    assert np.array_equal(S.to_e4m3(val), FINITE)  # every finite value is its own code, -0 included
    pos = np.sort(val[val >= 0])[1:]  # the 127 non-negative values (one of the two zeros dropped)
    assert pos.size == 127 and pos[0] == 0 and pos[-1] == 448
    mid = ((pos[:-1].astype(np.float64) + pos[1:]) / 2).astype(np.float32)  # exact in fp32
    assert np.array_equal(mid.astype(np.float64), (pos[:-1].astype(np.float64) + pos[1:]) / 2)
    below, above = np.nextafter(mid, np.float32(0)), np.nextafter(mid, np.float32(1e9))
    sub = np.linspace(-2.0 ** -6, 2.0 ** -6, 4097).astype(np.float32)  # the subnormal range, step 2^-18
    rnd = np.random.default_rng(0).uniform(-448, 448, 100000).astype(np.float32)
    edge = np.array([448, -448, 0.0, -0.0, 2.0 ** -9, 2.0 ** -10, -2.0 ** -10, 2.0 ** -11, 3 * 2.0 ** -10], np.float32)
    for x in (mid, -mid, below, -below, above, -above, sub, rnd, edge):
        assert np.array_equal(S.to_e4m3(x), _torch_e4m3(x))
    ties = S.to_e4m3(mid)
    assert (ties & 1 == 0).all()  # ties go to the even code


# ---------------------------------------------------------------------------------- 2. the quantiser
@pytest.mark.parametrize("kind,metric", [("normal", "ip"), ("pos", "ip"), ("normal", "cosine")])
def test_quantiser_error_bound(kind, metric):
    _, v, _ = P.make(300, 80, 1, 3, kind)
    codes, scales = S.prepare_rows_fp8(v, metric)
    if metric == "cosine":
        v = S.normalize_rows(v)
    assert codes.dtype == np.uint8 and scales.dtype == np.float32 and codes.shape == v.shape and scales.shape == (300,)
    v64, s64 = v.astype(np.float64), scales.astype(np.float64)[:, None]
    x = np.abs(v64 / s64)
    err = np.abs(v64 - s64 * S.e4m3_to_f32(codes).astype(np.float64))
    # half an ulp of 3 mantissa bits, half the subnormal step, and the fp32 division
    assert (err <= s64 * np.maximum(x * 2.0 ** -4, 2.0 ** -10) * (1 + 2.0 ** -10)).all()
    assert (np.abs(S.e4m3_to_f32(codes)).max(axis=1) == 448).all()
    assert not np.isin(codes, [0x7F, 0xFF]).any()


def test_quantiser_edges_and_shared_checks():
    v = np.zeros((3, 16), np.float32)
    v[1, 3] = 1e-42   # amax below 448 * the smallest normal: the scale is raised
    v[2] = np.linspace(-1, 1, 16)
    codes, scales = S.prepare_rows_fp8(v, "ip")
    assert scales[0] == 1.0 and not codes[0].any()
    assert scales[1] == np.finfo(np.float32).tiny and np.isfinite(S.e4m3_to_f32(codes[1])).all()
    assert np.isfinite(scales).all() and not np.isin(codes, [0x7F, 0xFF]).any()
    assert np.abs(S.e4m3_to_f32(codes[2])).max() == 448 and u32(scales[2:]) == u32(np.float32(1) / np.float32(448))
    for bad, word in ((np.zeros((2, 24), np.float32), "multiple of 16"), (np.zeros((2, 8), np.float32), "multiple of 16"),
                      (np.full((1, 16), np.nan, np.float32), "non-finite"), (np.zeros((2, 16), np.int32), "float array")):
        with pytest.raises(ValueError, match=word):
            S.prepare_rows_fp8(bad, "ip")
    with pytest.raises(ValueError, match="metric"):
        S.prepare_rows_fp8(v, "l2")
    # rows are quantised one by one: a row's bytes do not depend on its neighbours
    a, b = S.prepare_rows_fp8(v[2:], "cosine"), S.prepare_rows_fp8(v, "cosine")
    assert np.array_equal(a[0], b[0][2:]) and np.array_equal(u32(a[1]), u32(b[1][2:]))


# -------------------------------------------------------------------------------------- 3. the format
def test_default_dtype_writes_todays_bytes_and_version_3_round_trips(tmp_path):
    rng = np.random.default_rng(1)
    v = rng.standard_normal((70, 32)).astype(np.float32)
    labels = [f"d{i}" for i in range(70)]
    tags = rng.integers(0, 2 ** 32, 70, dtype=np.uint64).astype(np.uint32)
    rows = S.to_bf16(S.normalize_rows(v))

    def al(x):
        return -(-x // 4096) * 4096
    # version 1 by hand
    p1 = str(tmp_path / "v1.hzidx")
    S.write_index(p1, v, "cosine", labels=labels, model="m")
    js = json.dumps({"dim": 32, "count": 70, "dtype": "bf16", "metric": "cosine", "model": "m", "embed": None,
                     "labels": labels}).encode()
    off = al(S.HEAD.size + len(js))
    assert open(p1, "rb").read() == S.HEAD.pack(S.MAGIC, 1, len(js), off, 70, 32, 0) + js + bytes(off - S.HEAD.size - len(js)) + rows.tobytes()
    # version 2 by hand
    p2 = str(tmp_path / "v2.hzidx")
    S.write_index(p2, v, "cosine", labels=labels, model="m", tags=tags, dtype="bf16")
    hdr = {"dim": 32, "count": 70, "dtype": "bf16", "metric": "cosine", "model": "m", "embed": None, "labels": labels,
           "capacity": 70, "tags_off": 0, "live_off": 0}
    for _ in range(4):
        js = json.dumps(hdr).encode()
        off = al(S.HEAD.size + len(js))
        hdr["tags_off"] = al(off + rows.nbytes)
        hdr["live_off"] = al(hdr["tags_off"] + 280)
    js = json.dumps(hdr).encode()
    want = S.HEAD.pack(S.MAGIC, 2, len(js), off, 70, 32, 0) + js + bytes(off - S.HEAD.size - len(js)) + rows.tobytes()
    want += bytes(hdr["tags_off"] - len(want)) + tags.astype("<u4").tobytes()
    want += bytes(hdr["live_off"] - len(want)) + S.pack_live(np.ones(70, bool)).astype("<u4").tobytes()
    assert open(p2, "rb").read() == want
    assert S.file_info(p2) == {"version": 2, "capacity": 70, "live": 70, "tags": True}
    # version 3 without and with tags
    codes, scales = S.prepare_rows_fp8(v, "cosine")
    p3, p3t = str(tmp_path / "v3.hzidx"), str(tmp_path / "v3t.hzidx")
    h3 = S.write_index(p3, v, "cosine", labels=labels, model="m", dtype="fp8")
    assert h3["dtype"] == "fp8_e4m3" and h3["scales_off"] % 4096 == 0 and "tags_off" not in h3 and "capacity" not in h3
    assert S.HEAD.unpack(open(p3, "rb").read(S.HEAD.size))[1] == 3
    assert os.path.getsize(p3) == h3["scales_off"] + 280
    assert S.file_info(p3) == {"version": 3, "capacity": 70, "live": 70, "tags": False, "dtype": "fp8_e4m3"}
    h3t = S.write_index(p3t, v, "cosine", labels=labels, model="m", tags=tags, dtype="fp8")
    got = S.read_header(p3t)
    data_off = got.pop("data_off")
    assert got == h3t and h3t["capacity"] == 70 and data_off + 70 * 32 <= h3t["scales_off"] < h3t["tags_off"] < h3t["live_off"]
    for p in (p3, p3t):
        assert S.read_rows(p).dtype == np.uint8 and np.array_equal(S.read_rows(p), codes)
        assert np.array_equal(u32(S.read_scales(p)), u32(scales)) and S.read_live(p).all()
        assert S.read_header(p)["labels"] == labels
    assert np.array_equal(S.read_tags(p3t), tags) and not S.read_tags(p3).any()
    assert S.file_info(p3t) == {"version": 3, "capacity": 70, "live": 70, "tags": True, "dtype": "fp8_e4m3"}
    with pytest.raises(ValueError, match="no scales"):
        S.read_scales(p1)
    with pytest.raises(ValueError, match="dtype must be"):
        S.write_index(str(tmp_path / "x.hzidx"), v, "ip", dtype="int8")


def _rewrite(src, dst, version=None, dim=None, **keys):
    """A copy of the file ``src`` with JSON keys (and head fields) replaced; the JSON keeps its length class."""
    raw = open(src, "rb").read()
    magic, ver, jl, off, count, d, metric = S.HEAD.unpack(raw[:S.HEAD.size])
    hdr = json.loads(raw[S.HEAD.size:S.HEAD.size + jl])
    hdr.update(keys)
    if dim is not None:
        hdr["dim"] = dim
    js = json.dumps(hdr).encode()
    assert S.HEAD.size + len(js) <= off
    head = S.HEAD.pack(magic, ver if version is None else version, len(js), off, count, d if dim is None else dim, metric)
    open(dst, "wb").write(head + js + bytes(off - S.HEAD.size - len(js)) + raw[off:])


def test_read_header_refuses_a_bad_version_3_file(tmp_path):
    v = np.random.default_rng(2).standard_normal((96, 48)).astype(np.float32)
    good, bad = str(tmp_path / "g.hzidx"), str(tmp_path / "b.hzidx")
    h = S.write_index(good, v, "ip", dtype="fp8")
    data_off = S.read_header(good)["data_off"]
    for keys, word in (({"scales_off": h["scales_off"] + 8}, "not a multiple of 4096"),
                       ({"scales_off": data_off}, "overlaps the rows"),
                       ({"scales_off": h["scales_off"] + 4096}, "scales block lies outside"),
                       ({"dtype": "bf16"}, "version 3 means fp8"),
                       ({"scales_off": None}, "scales_off")):
        _rewrite(good, bad, **keys)
        with pytest.raises(ValueError, match=word):
            S.read_header(bad)
    _rewrite(good, bad, dim=24)  # 96 x 48 bytes read as 192 x 24: the same block, a refused dimension
    with pytest.raises(ValueError, match="multiple of 16"):
        S.read_header(bad)
    plain = str(tmp_path / "p.hzidx")
    S.write_index(plain, v, "ip")
    _rewrite(plain, bad, dtype="fp8_e4m3")
    with pytest.raises(ValueError, match="version 3 means fp8"):
        S.read_header(bad)
    # tags in front of the scales
    ht = S.write_index(good, v, "ip", tags=np.arange(96), dtype="fp8")
    _rewrite(good, bad, tags_off=ht["scales_off"])
    with pytest.raises(ValueError, match="tags block lies outside"):
        S.read_header(bad)
    assert S.read_header(good)["tags_off"] == ht["tags_off"]


# ------------------------------------------------------------------------------------- 4. RefIndex
def test_search_ref_scales_and_default():
    rng = np.random.default_rng(4)
    c = S.bf16_to_f32(S.to_bf16(rng.standard_normal((60, 16)).astype(np.float32)))
    q = rng.standard_normal((3, 16)).astype(np.float32)
    s0, i0 = S.search_ref(c, q, 5)
    want = np.sort((c.astype(np.float64) @ q.astype(np.float64).T).T, axis=1)[:, ::-1][:, :5]
    assert np.allclose(s0, want, rtol=1e-12, atol=0)
    s1, i1 = S.search_ref(c, q, 5, None, None)
    assert np.array_equal(s0.view(np.uint64), s1.view(np.uint64)) and np.array_equal(i0, i1)
    # fixed values: today's arithmetic
    fs, fi = S.search_ref(np.array([[1.0, 2.0], [3.0, -1.0], [-0.0, 0.0]]), np.array([[2.0, 0.5]]), 3)
    assert fs.tolist() == [[5.5, 3.0, 0.0]] and fi.tolist() == [[1, 0, 2]]
    sc = rng.uniform(0.5, 2, 60).astype(np.float32)
    s2, i2 = S.search_ref(c, q, 60, scales=sc)
    full = (c.astype(np.float64) * q[1].astype(np.float64)[None]).sum(axis=1) * sc.astype(np.float64)
    assert np.array_equal(i2[1], np.argsort(-full, kind="stable")) and np.array_equal(s2[1], full[i2[1]])


def test_refindex_on_a_version_3_file(tmp_path):
    rng = np.random.default_rng(5)
    A, B = rng.standard_normal((40, 32)).astype(np.float32) * 3, rng.standard_normal((25, 32)).astype(np.float32) * 3
    q = rng.standard_normal((2, 32)).astype(np.float32)
    pa, pab, out = str(tmp_path / "a.hzidx"), str(tmp_path / "ab.hzidx"), str(tmp_path / "o.hzidx")
    S.write_index(pa, A, "cosine", dtype="fp8")
    S.write_index(pab, np.concatenate([A, B]), "cosine", dtype="fp8")
    with S.RefIndex(pa) as ix:
        assert ix.dtype == "fp8_e4m3" and ix.describe()["dtype"] == "fp8_e4m3"
        assert np.array_equal(ix._rows, S.e4m3_to_f32(S.read_rows(pa))) and np.array_equal(ix.scales, S.read_scales(pa))
        s, i = ix.search(q, 5)
        rs, ri = S.search_ref(ix._rows, q, 5, scales=ix.scales)
        assert np.array_equal(i, ri) and np.array_equal(s, rs.astype(np.float32))
        ids = ix.add(B)
        assert list(ids) == list(range(40, 65))
        ix.save(out)
        assert open(out, "rb").read() == open(pab, "rb").read()  # add(B) onto A: the bytes of write_index(A u B)
        ix.set_tags(ids, np.arange(25))
        full, fsc = S.e4m3_to_f32(S.read_rows(pab)), S.read_scales(pab)
        best = int(ix.search(q, 5)[1][0, 0])
        assert ix.delete([best, 41]) == 2 and ix.delete([best]) == 0
        allow = np.ones(65, bool)
        allow[[best, 41]] = False
        assert np.array_equal(ix.search(q, 5)[1], S.search_ref(full, q, 5, allow, scales=fsc)[1])
        assert ix.search(q, 5, filter=(0xFFFFFFFF, 7))[1].tolist() == [[47, -1, -1, -1, -1]] * 2
        tags = np.concatenate([np.zeros(40, np.uint32), np.arange(25, dtype=np.uint32)])
        _, i4 = ix.search(q, 70, filter=[(1, 1), (0, 0)])
        assert np.array_equal(i4, S.search_ref(full, q, 70, np.stack([allow & (tags & 1 == 1), allow]), scales=fsc)[1])
        with pytest.raises(ValueError, match=r"\[N, 32\]"):
            ix.add(np.ones((1, 48), np.float32))
        keep, comp = str(tmp_path / "keep.hzidx"), str(tmp_path / "comp.hzidx")
        ix.save(keep)
        ix.save(comp, compact=True)
        want = ix.search(q, 8)
        live, tg = ix._live.copy(), ix._tags.copy()
    assert S.file_info(keep) == {"version": 3, "capacity": 80, "live": 63, "tags": True, "dtype": "fp8_e4m3"}
    with S.RefIndex(keep) as k2:
        got = k2.search(q, 8)
        assert np.array_equal(got[1], want[1]) and np.array_equal(u32(got[0]), u32(want[0])) and k2.delete([best]) == 0
    with S.RefIndex(comp) as c2:
        assert c2.count == 63 and c2._live.all() and np.array_equal(c2._tags, tg[live])
        assert np.array_equal(u32(c2.scales), u32(fsc[live]))
        got = c2.search(q, 8)
        assert np.array_equal(got[1], (np.cumsum(live) - 1)[want[1]]) and np.array_equal(u32(got[0]), u32(want[0]))


# -------------------------------------------------------------------------------- 5. convert_index
def test_convert_index_keeps_ids_labels_tags_live_and_capacity(tmp_path):
    rng = np.random.default_rng(6)
    v = rng.standard_normal((50, 32)).astype(np.float32)
    src, mid, dst = (str(tmp_path / n) for n in ("s.hzidx", "m.hzidx", "d.hzidx"))
    S.write_index(src, v, "cosine", labels=[f"r{i}" for i in range(50)], model="m", tags=np.arange(50) % 3,
                  embed={"pooling": "mean", "normalize": True, "dim": 32})
    with S.RefIndex(src, reserve=100) as ix:
        ix.delete([4, 9])
        ix.save(mid)
    hdr = S.convert_index(mid, dst, "fp8")
    codes, scales = S.quantize_rows(S.bf16_to_f32(S.read_rows(mid)))  # the stored rows, not renormalised
    same = S.prepare_rows_fp8(S.bf16_to_f32(S.read_rows(mid)), "ip")
    assert np.array_equal(codes, same[0]) and np.array_equal(u32(scales), u32(same[1]))
    assert np.array_equal(S.read_rows(dst), codes) and np.array_equal(u32(S.read_scales(dst)), u32(scales))
    a, b = S.read_header(mid), S.read_header(dst)
    for key in ("dim", "count", "metric", "model", "embed", "labels", "capacity"):
        assert a[key] == b[key], key
    assert (b["dtype"], hdr["capacity"]) == ("fp8_e4m3", 100) and S.file_info(dst)["live"] == 48
    assert np.array_equal(S.read_tags(dst), S.read_tags(mid)) and np.array_equal(S.read_live(dst), S.read_live(mid))
    plain = str(tmp_path / "p.hzidx")
    S.write_index(plain, v, "ip")
    assert "tags_off" not in S.convert_index(plain, dst, "fp8") and S.file_info(dst)["version"] == 3
    with pytest.raises(ValueError, match="only a bf16 index"):
        S.convert_index(dst, plain, "fp8")
    S.write_index(plain, v[:, :24], "ip")
    with pytest.raises(ValueError, match="multiple of 16"):
        S.convert_index(plain, dst, "fp8")


# ------------------------------------------------------------------------------------------ 6. CLI
def _cli(*args):
    return subprocess.run([sys.executable, "-m", "hipzap", *args], capture_output=True, text=True, cwd=ROOT, timeout=120)


def test_cli_dtype_from_index_and_info(tmp_path):
    v = np.random.default_rng(7).standard_normal((9, 32)).astype(np.float32)
    np.save(str(tmp_path / "v.npy"), v)
    np.save(str(tmp_path / "t.npy"), np.arange(9, dtype=np.uint32))
    bf, q8, conv = (str(tmp_path / n) for n in ("bf.hzidx", "q8.hzidx", "conv.hzidx"))
    r = _cli("index", "--vectors", str(tmp_path / "v.npy"), "--tags", str(tmp_path / "t.npy"), "--metric", "ip", "--dtype", "fp8", "--out", q8)
    assert r.returncode == 0 and json.loads(r.stdout)["dtype"] == "fp8_e4m3", r.stderr
    codes, scales = S.prepare_rows_fp8(v, "ip")
    assert np.array_equal(S.read_rows(q8), codes) and np.array_equal(S.read_tags(q8), np.arange(9))
    r = _cli("index", "--vectors", str(tmp_path / "v.npy"), "--tags", str(tmp_path / "t.npy"), "--metric", "ip", "--out", bf)
    assert r.returncode == 0 and S.read_header(bf)["dtype"] == "bf16", r.stderr
    r = _cli("index", "--from-index", bf, "--dtype", "fp8", "--out", conv)
    assert r.returncode == 0 and json.loads(r.stdout)["scales_off"] > 0, r.stderr
    assert np.array_equal(S.read_rows(conv), S.quantize_rows(S.bf16_to_f32(S.read_rows(bf)))[0])
    r = _cli("info", conv)
    j = json.loads(r.stdout)
    assert r.returncode == 0 and (j["version"], j["dtype"], j["capacity"], j["live"], j["tags"], j["count"]) == (3, "fp8_e4m3", 9, 9, True, 9)
    assert json.loads(_cli("info", bf).stdout)["dtype"] == "bf16"
    assert _cli("index", "--from-index", bf, "--vectors", str(tmp_path / "v.npy"), "--out", conv).returncode != 0


@pytest.fixture()
def served(tmp_path):
    from transformers import BertConfig, BertModel
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    root = tmp_path
    torch.manual_seed(0)
    torch.save(BertModel(BertConfig(num_hidden_layers=1), add_pooling_layer=False).eval().state_dict(), str(root / "enc.pth"))
    corpus = np.random.default_rng(8).standard_normal((50, 768)).astype(np.float32)
    tags = (np.arange(50) % 4).astype(np.uint32)
    S.write_index(str(root / "rw.hzidx"), corpus, "cosine", tags=tags, dtype="fp8")
    emb = {"pooling": "mean", "normalize": True}
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["rw"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={
        "embed": emb, "seq_len": 32, "index": "rw.hzidx", "index_writable": True, "index_reserve": 100})
    srv = ModelServer(st, backend="cpu")
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, srv, str(root / "rw.hzidx")
    srv.close()
    app_mod.set_server(None)


def test_cpu_server_on_a_version_3_index_matches_refindex(served):
    client, srv, path = served
    rng = np.random.default_rng(9)
    q, new = rng.standard_normal((2, 768)).astype(np.float32), rng.standard_normal((3, 768)).astype(np.float32)
    qn = S.normalize_rows(q)

    def ids(r):
        return [[h["id"] for h in row] for row in r.json["results"]]
    with S.RefIndex(path) as ref:
        r = client.post("/search", json={"model": "rw", "vectors": q.tolist(), "k": 6})
        assert r.status_code == 200 and r.json["dtype"] == "fp8_e4m3" and ids(r) == ref.search(qn, 6)[1].tolist(), r.data
        r = client.post("/search", json={"model": "rw", "vectors": q.tolist(), "k": 6, "tag": 3})
        assert ids(r) == ref.search(qn, 6, filter=(0xFFFFFFFF, 3))[1].tolist()
        r = client.post("/index/add", json={"model": "rw", "vectors": new.tolist(), "tags": [9, 9, 1]})
        assert r.status_code == 200 and r.json["ids"] == [50, 51, 52], r.data
        ref.add(new, tags=[9, 9, 1])
        r = client.post("/search", json={"model": "rw", "vectors": new[:1].tolist(), "k": 2})
        assert ids(r) == ref.search(S.normalize_rows(new[:1]), 2)[1].tolist() and ids(r)[0][0] == 50
        assert client.post("/index/delete", json={"model": "rw", "ids": [51]}).json["deleted"] == ref.delete([51]) == 1
        r = client.post("/index/save", json={"model": "rw"})
        assert r.status_code == 200 and r.json["count"] == 53, r.data
        want = str(path) + ".ref"
        ref.save(want)
    assert open(path, "rb").read() == open(want, "rb").read()
    assert S.file_info(path) == {"version": 3, "capacity": 100, "live": 52, "tags": True, "dtype": "fp8_e4m3"}


# ----------------------------------------------------------------------------------- 7. unambiguity
def test_gpu_cases_are_unambiguous_over_their_passing_rows():
    for name in P.NAMES:
        codes, scales, q, k, live = P.build_case(name)
        s, b = P.oracle_q(codes, scales, q)
        assert F.subset_ambiguous(s, b, k, live) == 0, name
    assert {c[1] for c in P.CASES} >= {1, 9, T - 1, T, T + 1, 3 * T + 5}
    assert {c[2] for c in P.CASES} == {16, 80, 768, 1024, 1040, 2048} and {c[3] for c in P.CASES} == {1, 3, 16}
    assert {c[4] for c in P.CASES} == {1, 10, 128} and {c[5] for c in P.CASES} == {"normal", "pos", "neg"}
    assert {c[6] for c in P.CASES} == {"all", "mid_tile_dead", "dead_groups", "few_total"}
    assert any(c[2:4] == (2048, 16) for c in P.CASES)  # the LDS maximum
    _, _, _, k, live = P.build_case("few_total")
    assert 0 < live.sum() < k


def test_the_index_scenarios_are_unambiguous_on_the_host(tmp_path):
    """What tests/test_search_fp8_index_gpu.py compares with RefIndex: every search of it has a forced answer."""
    path = str(tmp_path / "a.hzidx")
    c32, q = P.big_data()
    S.write_index(path, c32, "ip", dtype="fp8")
    with S.RefIndex(path) as ix:
        assert P.index_unambiguous(ix, q, 10) and P.index_unambiguous(ix, q, 1)
    A, B, q = P.index_data()
    S.write_index(path, A, "ip", tags=F.index_tags(F.IX_N), dtype="fp8")
    with S.RefIndex(path) as ix:
        F.drive(ix, B, q)
        live, tags = ix._live, ix._tags
        assert P.index_unambiguous(ix, q, 10) and P.index_unambiguous(ix, q, 10, live & (tags == 3))
        assert P.index_unambiguous(ix, q, 7, live & (tags & 1 == 1)) and (live & (tags == 9)).sum() == 2
    _, c32, q = P.make(2 * T + 31, 80, 2, 36, "pos")  # the concurrency test: its mutations never change the top 2
    extra = P.make(16, 80, 1, 37, "pos")[1] * np.float32(1e-3)
    S.write_index(path, c32, "ip", dtype="fp8")
    with S.RefIndex(path) as ix:
        assert P.index_unambiguous(ix, q, 2)
        want = ix.search(q, 2)
        ix.delete([int(np.setdiff1d(np.arange(8), want[1].ravel())[0])])
        for _ in range(3):
            ids = ix.add(extra)
            ix.delete(ids[:8])
            ix.set_tags(ids[8:], [3] * 8)
            got = ix.search(q, 2)
            assert np.array_equal(got[1], want[1]) and np.array_equal(u32(got[0]), u32(want[0]))
    _, c32, q = P.make(T - 3, 768, 3, 38, "pos")  # the served index, before its add
    S.write_index(path, c32, "ip", tags=(np.arange(T - 3) % 4).astype(np.uint32), dtype="fp8")
    with S.RefIndex(path) as ix:
        assert P.index_unambiguous(ix, q, 10) and P.index_unambiguous(ix, q, 10, ix._tags == 2)
    _, c32, q = P.make(T - 6, 80, 1, 33, "pos")  # the mutation test's first search
    S.write_index(path, c32, "ip", dtype="fp8")
    with S.RefIndex(path) as ix:
        assert P.index_unambiguous(ix, q, 10)
