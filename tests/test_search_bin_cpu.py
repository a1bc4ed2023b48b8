"""Binary (sign-bit) indexes on the host: the bits, the .hzidx versions 8 and 9, every reader refusal, RefIndex
(the oracle and the CPU backend), the by-name refusals and the CLI's argument errors. No GPU."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hipzap import search as S

import search_bin_cases as B
from search_bin_cases import T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ bits
def test_prepare_rows_bin_matches_a_bit_by_bit_loop():
    rng = np.random.default_rng(1)
    v = rng.standard_normal((7, 256)).astype(np.float32)
    for metric in S.METRICS:
        words = S.prepare_rows_bin(v, metric)
        assert words.dtype == np.uint32 and words.shape == (7, 8)
        vn = S.normalize_rows(v) if metric == "cosine" else v
        for r in range(7):
            for i in range(256):
                bit = (int(words[r, i >> 5]) >> (i & 31)) & 1
                assert bit == (0 if np.signbit(vn[r, i]) else 1), (metric, r, i)
        assert np.array_equal(words, B.binarize(vn))
    for bad, msg in ((v[:, :64], "multiple of 128"), (v[:, :192], "multiple of 128"),
                     (np.zeros((2, 2176), np.float32), "128..2048")):
        with pytest.raises(ValueError, match=msg):
            S.prepare_rows_bin(bad, "ip")


def test_fp32_and_stored_bf16_binarisation_agree_on_every_sign_edge():
    vals = B.sign_edge_values()
    rows = np.resize(vals, (3, 128)).astype(np.float32)
    rows[1] = rows[1][::-1]
    bits = S.to_bf16(rows)
    # -0.0 and the negative values that round to zero magnitude stay negative zeros in bf16: the sign survives
    assert (S.bf16_to_f32(bits)[rows == 0] == 0).all() and np.array_equal(np.signbit(S.bf16_to_f32(bits)), np.signbit(rows))
    assert (bits[np.abs(rows) < 4e-41] & 0x7FFF == 0).all()  # below half the smallest bf16 subnormal: zero magnitude
    assert np.array_equal(S.binarize(rows), S.binarize_bf16(bits))
    assert np.array_equal(S.binarize(rows), B.binarize(rows))
    one = S.binarize(np.array([[0.0, -0.0] + [1.0] * 126], np.float32))
    assert one[0, 0] & 3 == 1  # +0.0 gives 1, -0.0 gives 0
    rng = np.random.default_rng(2)
    v = (rng.standard_normal((50, 768)) * 10.0 ** rng.integers(-44, 3, (50, 768))).astype(np.float32)
    for metric in S.METRICS:
        assert np.array_equal(S.prepare_rows_bin(v, metric), S.binarize_bf16(S.prepare_rows(v, metric)))


# ----------------------------------------------------------------------------------------------- files
def vectors(n=300, d=128):
    i = np.arange(n * d, dtype=np.uint64)
    return (((i * np.uint64(2654435761)) % np.uint64(2003)).astype(np.float32) / np.float32(1001.5) - np.float32(1.0)).reshape(n, d)


TAGS = (np.arange(300) % 5).astype(np.uint32)
# what the parent commit's write_index / convert_index wrote for `vectors()`: offsets, sizes, and for the versions
# without k-means the digest of the whole file
RECORDED = {
    "v1": {'size': 80896, 'data_off': 4096, 'sha256': '195c174d5587e1f9709b101293d590e4d17e64571f37dda6347c3f8d3f619797'},
    "v2": {'tags_off': 81920, 'live_off': 86016, 'size': 86056, 'data_off': 4096,
           'sha256': 'd4bfb3e64e2e01c4bfe0b26fbb4cb992aac8a970fd98cefc48af93e34c27a9f5'},
    "v3": {'scales_off': 45056, 'size': 46256, 'data_off': 4096,
           'sha256': '503f58b08ba713ec400034a4cf11b00dde090c5b79af4e54cd5514f4ac09fea8'},
    "v4": {'scales_off': 45056, 'tags_off': 49152, 'live_off': 53248, 'rescore_off': 57344, 'size': 134144, 'data_off': 4096,
           'sha256': '1c78698e1a341be39432cb16f5c771ee01708e1e46644ab3af70fbfaa3088060'},
    "v5": {'tags_off': 200704, 'live_off': 204800, 'centroids_off': 208896, 'list_off_off': 212992, 'list_tiles_off': 217088,
           'rowid_off': 221184, 'size': 224256, 'data_off': 4096},
    "v6": {'scales_off': 102400, 'tags_off': 106496, 'live_off': 110592, 'centroids_off': 114688, 'list_off_off': 118784,
           'list_tiles_off': 122880, 'rowid_off': 126976, 'size': 130048, 'data_off': 4096},
    "v7": {'scales_off': 102400, 'tags_off': 106496, 'live_off': 110592, 'rescore_off': 131072, 'centroids_off': 114688,
           'list_off_off': 118784, 'list_tiles_off': 122880, 'rowid_off': 126976, 'size': 207872, 'data_off': 4096},
}


def test_versions_1_to_7_are_written_as_before(tmp_path):
    v, out = vectors(), {}
    for name, kw in (("v1", {}), ("v2", {"tags": TAGS}), ("v3", {"dtype": "fp8"}),
                     ("v4", {"dtype": "fp8", "rescore": True, "tags": TAGS}),
                     ("v5", {"tags": TAGS, "ivf": 3, "nprobe": 2, "ivf_seed": 1})):
        out[name] = str(tmp_path / f"{name}.hzidx")
        S.write_index(out[name], v, "cosine", labels=[f"r{i}" for i in range(300)], model="m", **kw)
    out["v6"], out["v7"] = str(tmp_path / "v6.hzidx"), str(tmp_path / "v7.hzidx")
    S.convert_index(out["v5"], out["v6"], "fp8")
    S.convert_index(out["v5"], out["v7"], "fp8", rescore=True)
    for i, (name, p) in enumerate(out.items()):
        raw = open(p, "rb").read()
        h = S.read_header(p)
        offs = {k: h[k] for k in ("scales_off", "tags_off", "live_off", "rescore_off") if k in h}
        offs.update({k: h["ivf"][k] for k in S.IVF_KEYS} if "ivf" in h else {})
        rec = dict(offs, size=len(raw), data_off=h["data_off"])
        if "sha256" in RECORDED[name]:
            rec["sha256"] = hashlib.sha256(raw).hexdigest()
        assert rec == RECORDED[name], name
        assert S.HEAD.unpack(raw[:S.HEAD.size])[1] == i + 1 and S.file_info(p)["version"] == i + 1


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("bin")
    v = vectors()
    p = {k: str(root / f"{k}.hzidx") for k in ("v1", "v2", "v8", "v8t", "v9", "v9t", "fp8", "ivf")}
    labels = [f"r{i}" for i in range(300)]
    S.write_index(p["v1"], v, "cosine", labels=labels, model="m")
    S.write_index(p["v2"], v, "cosine", labels=labels, model="m", tags=TAGS)
    h8 = S.write_index(p["v8"], v, "cosine", labels=labels, model="m", dtype="bin")
    h8t = S.write_index(p["v8t"], v, "cosine", labels=labels, model="m", dtype="bin", tags=TAGS)
    h9 = S.write_index(p["v9"], v, "cosine", labels=labels, model="m", dtype="bin", rescore=True)
    h9t = S.write_index(p["v9t"], v, "cosine", labels=labels, model="m", dtype="bin", rescore=True, tags=TAGS)
    S.write_index(p["fp8"], v, "cosine", dtype="fp8")
    S.write_index(p["ivf"], v, "cosine", ivf=3)
    return p, v, {"v8": h8, "v8t": h8t, "v9": h9, "v9t": h9t}


def test_version_8_and_9_byte_layout(files):
    p, v, hdrs = files
    words = S.prepare_rows_bin(v, "cosine")
    want = {"v8": (8, {}), "v8t": (8, {"tags_off": 12288, "live_off": 16384}),
            "v9": (9, {"rescore_off": 12288}), "v9t": (9, {"tags_off": 12288, "live_off": 16384, "rescore_off": 20480})}
    for name, (version, offs) in want.items():
        raw = open(p[name], "rb").read()
        magic, ver, jl, data_off, count, dim, metric = S.HEAD.unpack(raw[:S.HEAD.size])
        h = json.loads(raw[S.HEAD.size:S.HEAD.size + jl])
        assert (magic, ver, data_off, count, dim, metric) == (S.MAGIC, version, 4096, 300, 128, 0), name
        assert h == hdrs[name] and h["dtype"] == "bin_sign" and "scales_off" not in h
        assert {k: h[k] for k in ("tags_off", "live_off", "rescore_off") if k in h} == offs, name
        assert ("capacity" in h) == ("tags_off" in h)
        assert raw[data_off:data_off + 300 * 16] == words.astype("<u4").tobytes()  # uint32 [count][W], W = 4
        end = data_off + 4800
        if "tags_off" in h:
            assert raw[h["tags_off"]:h["tags_off"] + 1200] == TAGS.astype("<u4").tobytes()
            assert raw[h["live_off"]:h["live_off"] + 40] == S.pack_live(np.ones(300, bool)).astype("<u4").tobytes()
            end = h["live_off"] + 40
        if "rescore_off" in h:  # byte-identical to the bf16 file's row block, and the last block
            bf = open(p["v1"], "rb").read()
            assert raw[h["rescore_off"]:] == bf[4096:4096 + 300 * 128 * 2]
            end = h["rescore_off"] + 300 * 256
        assert len(raw) == end, name
        info = S.file_info(p[name])
        assert (info["version"], info["dtype"], info["live"], info["tags"]) == (version, "bin_sign", 300, "tags_off" in h)
        assert np.array_equal(S.read_rows(p[name]), words) and S.read_rows(p[name]).dtype == np.uint32
        assert np.array_equal(S.read_tags(p[name]), TAGS if "tags_off" in h else np.zeros(300, np.uint32))
    assert np.array_equal(S.read_rescore_rows(p["v9"]), S.read_rows(p["v1"]))


def test_convert_index_round_trip(files, tmp_path):
    p, v, _ = files
    for src, rescore, same_as in (("v1", False, "v8"), ("v1", True, "v9"), ("v2", False, "v8t"), ("v2", True, "v9t")):
        dst = str(tmp_path / f"c_{src}_{rescore}.hzidx")
        h = S.convert_index(p[src], dst, "bin", rescore=rescore)
        assert h["dtype"] == "bin_sign" and open(dst, "rb").read() == open(p[same_as], "rb").read()  # bits of the stored rows
        assert np.array_equal(S.read_rows(dst), S.binarize_bf16(S.read_rows(p[src])))
    for kw, src, msg in (({"ivf": 3}, "v1", "ivf=3 with dtype='bin'"), ({}, "ivf", "dtype='bin'.*IVF index"),
                         ({}, "fp8", "dtype='bin'.*fp8_e4m3")):
        with pytest.raises(ValueError, match=msg):
            S.convert_index(p[src], str(tmp_path / "no.hzidx"), "bin", **kw)
    with pytest.raises(ValueError, match="ivf=3 with dtype='bin'"):
        S.write_index(str(tmp_path / "no.hzidx"), v, "cosine", dtype="bin", ivf=3)
    with pytest.raises(ValueError, match="dtype must be one of"):
        S.write_index(str(tmp_path / "no.hzidx"), v, "cosine", dtype="bits")
    with pytest.raises(ValueError, match="multiple of 128"):
        S.write_index(str(tmp_path / "no.hzidx"), v[:, :64], "cosine", dtype="bin")
    assert not os.path.exists(str(tmp_path / "no.hzidx"))


def _rewrite(src, dst, version=None, edit=None, cut=None, dim=None):
    """A copy of ``src`` with another version word or dim, an edited JSON header (same length) or a shorter tail."""
    raw = bytearray(open(src, "rb").read())
    magic, ver, jl, data_off, count, d, metric = S.HEAD.unpack(raw[:S.HEAD.size])
    if version is not None:
        raw[8:12] = np.array([version], "<u4").tobytes()
    if dim is not None:
        raw[32:36] = np.array([dim], "<u4").tobytes()
    if edit is not None:
        js = raw[S.HEAD.size:S.HEAD.size + jl].decode()
        new = edit(js)
        assert len(new) <= jl, (len(new), jl)
        raw[S.HEAD.size:S.HEAD.size + jl] = new.ljust(jl).encode()
    if cut is not None:
        raw = raw[:cut]
    open(dst, "wb").write(bytes(raw))
    return dst


def reader_refusals(p):
    """(name, source, rewrite arguments, words of the Python message)."""
    return [
        ("bin dtype in version 3", "v8", dict(version=3), "version-3"),
        ("bf16 dtype in version 8", "v8", dict(edit=lambda s: s.replace('"bin_sign"', '"bf16"')), "version-8"),
        ("fp8 dtype in version 9", "v9", dict(edit=lambda s: s.replace('"bin_sign"', '"fp8_e4m3"')), "version-9"),
        ("version 8 with rescore keys", "v9", dict(version=8), "rescore keys in a version-8"),
        ("version 9 without them", "v8", dict(version=9), "version-9 file without rescore"),
        ("ivf block in version 8", "v8t", dict(edit=lambda s: s.replace('"capacity": 300', '"ivf": {}')), "ivf block"),
        ("dim % 128", "v8", dict(dim=64, edit=lambda s: s.replace('"dim": 128', '"dim": 64')), "multiple of 128"),
        ("unaligned tags", "v8t", dict(edit=lambda s: s.replace('"tags_off": 12288', '"tags_off": 12292')), "tags block"),
        ("tags over the rows", "v8t", dict(edit=lambda s: s.replace('"tags_off": 12288', '"tags_off": 4096')), "tags block"),
        ("rescore over the live block", "v9t", dict(edit=lambda s: s.replace('"rescore_off": 20480', '"rescore_off": 16384')),
         "overlaps another block"),
        ("unaligned rescore", "v9", dict(edit=lambda s: s.replace('"rescore_off": 12288', '"rescore_off": 12296')), "rescore_off"),
        ("rows outside the file", "v8", dict(cut=4096 + 100), "row block"),
        ("live outside the file", "v8t", dict(cut=16384 + 8), "live block"),
        ("rescore outside the file", "v9", dict(cut=12288 + 1000), "rescore block lies outside"),
    ]


def test_every_reader_refusal(files, tmp_path):
    p, _, _ = files
    for name, src, kw, words in reader_refusals(p):
        bad = _rewrite(p[src], str(tmp_path / "bad.hzidx"), **kw)
        with pytest.raises(ValueError, match=words):
            S.read_header(bad)
    for src in ("v8", "v8t", "v9", "v9t"):  # and the files as written are accepted
        assert S.read_header(p[src])["dtype"] == "bin_sign"


# --------------------------------------------------------------------------------------------- RefIndex
def test_refindex_stage_one_is_exact_hamming_under_the_order_rule(files):
    p, v, _ = files
    q = vectors(5, 128)[::-1].copy()
    with S.RefIndex(p["v8"]) as ix:
        s, i = ix.search(q, 128)
        assert s.dtype == np.float32 and (s == np.round(s)).all() and (np.abs(s) <= 128).all() and (s % 2 == 0).all()
        want = B.bin_scan_ref(S.read_rows(p["v8"]), B.binarize(q), 128)
        assert np.array_equal(B.keys_of(s, i), want)
        assert ((np.diff(s, axis=1) < 0) | (np.diff(i, axis=1) > 0)).all()  # ties in id order
        d = ix.describe()
        assert (d["dtype"], ix.version, d["backend"]) == ("bin_sign", 8, "cpu")
        for refine in (None, 0):
            assert np.array_equal(ix.search(q, 10, refine=refine)[1], i[:, :10])
        for bad in (10, 128, True, "x"):
            with pytest.raises(ValueError, match="refine must be None or 0.*bin_sign index of version 8"):
                ix.search(q, 10, refine=bad)


def test_refindex_refine_rules_on_a_version_9_index(files):
    p, v, _ = files
    q = vectors(4, 128)[::-1].copy()
    with S.RefIndex(p["v9"]) as ix, S.RefIndex(p["v1"]) as bf:
        assert ix.version == 9 and ix.rescore
        s0, i0 = ix.search(q, 10, refine=0)
        with S.RefIndex(p["v8"]) as one:
            assert np.array_equal(i0, one.search(q, 10)[1])
        sn, i_n = ix.search(q, 10)
        s128, i128 = ix.search(q, 10, refine=128)
        assert np.array_equal(i_n, i128) and np.array_equal(u32(sn), u32(s128))  # None means R = 128
        for R in (10, 40, 128):
            s, i = ix.search(q, 10, refine=R)
            cand = ix.search(q, R, refine=0)[1]
            for a in range(4):  # stage two: the existing fp64 rescoring of stage one's R ids
                ws, wi = S.rescore_ref(bf._rows, q[a], cand[a], 10)
                assert np.array_equal(i[a], wi) and np.array_equal(u32(s[a]), u32(ws.astype(np.float32)))
        for bad in (9, 129, -1, True, 7.5, "many"):
            with pytest.raises(ValueError, match=r"refine must be None, 0 or an integer in \[k, 128\].*bin_sign index of version 9"):
                ix.search(q, 10, refine=bad)
        # R covers every passing row: the bf16 index's answer
        filt = (0xFFFFFFFF, 3)
    with S.RefIndex(p["v9t"]) as ix, S.RefIndex(p["v2"]) as bf:
        s, i = ix.search(q, 10, filter=filt, refine=128)  # 60 rows carry tag 3
        ws, wi = bf.search(q, 10, filter=filt)
        assert np.array_equal(i, wi) and np.array_equal(u32(s), u32(ws))


def test_the_cluster_fixture_meets_its_precondition(tmp_path):
    """tests/test_search_bin_index_gpu.py relies on this: every bf16 top-10 id lies among the Hamming top 128 under
    the order rule, while the binary answer alone differs from the bf16 one."""
    for D in (128, 768):
        v, q = B.clusters(D)
        p9, p1 = str(tmp_path / f"c9_{D}.hzidx"), str(tmp_path / f"c1_{D}.hzidx")
        S.write_index(p9, v, "cosine", dtype="bin", rescore=True)
        S.write_index(p1, v, "cosine")
        qn = S.normalize_rows(q)
        with S.RefIndex(p9) as ix, S.RefIndex(p1) as bf:
            top = bf.search(qn, 10)[1]
            ham = ix.search(qn, 128, refine=0)[1]
            for a in range(q.shape[0]):
                assert set(top[a].tolist()) <= set(ham[a].tolist()), (D, a)
            assert not np.array_equal(ix.search(qn, 10, refine=0)[1], top)
            assert np.array_equal(ix.search(qn, 10, refine=128)[1], top)


def test_refindex_live_scenario_save_and_compact(tmp_path):
    D = 128
    A, Bv, q = B.index_data(D)
    for rescore in (False, True):
        p = str(tmp_path / f"live_{rescore}.hzidx")
        S.write_index(p, A, "ip", dtype="bin", rescore=rescore, labels=[f"a{i}" for i in range(B.IX_N)])
        with S.RefIndex(p, reserve=2 * T) as ix:
            assert ix.capacity() == 2 * T
            with pytest.raises(ValueError, match="labels are required"):
                ix.add(Bv)
            ids = ix.add(Bv, tags=np.arange(T) % 3, labels=[f"b{i}" for i in range(T)])
            assert ids.tolist() == list(range(B.IX_N, B.IX_N + T)) and ix.count == B.IX_N + T and ix.capacity() == 4 * T
            words = np.concatenate([S.prepare_rows_bin(A, "ip"), S.prepare_rows_bin(Bv, "ip")])
            assert np.array_equal(ix._state()[0], words)
            assert ix.delete([0, 5, 5, B.IX_N + 1]) == 3
            ix.set_tags([7, 8], [9, 9])
            live = np.ones(B.IX_N + T, bool)
            live[[0, 5, B.IX_N + 1]] = False
            s, i = ix.search(q, 10, refine=0)
            assert np.array_equal(B.keys_of(s, i), B.bin_scan_ref(words, B.binarize(q), 10, live))
            s, i = ix.search(q, 10, filter=(0xFFFFFFFF, 9), refine=0)
            assert (np.sort(i[:, :2], axis=1) == [7, 8]).all() and (i[:, 2:] == -1).all()
            with pytest.raises(ValueError, match="outside"):
                ix.delete([B.IX_N + T])
            saved = str(tmp_path / f"saved_{rescore}.hzidx")
            h = ix.save(saved)
            assert S.file_info(saved)["version"] == (9 if rescore else 8) and h["capacity"] == 4 * T and "tags_off" in h
            assert np.array_equal(S.read_rows(saved), words) and np.array_equal(S.read_live(saved), live)
            if rescore:
                assert np.array_equal(S.read_rescore_rows(saved), np.concatenate([S.prepare_rows(A, "ip"), S.prepare_rows(Bv, "ip")]))
            with S.RefIndex(saved) as again:
                for kw in ({}, {"filter": (3, 1)}):
                    a, b = ix.search(q, 10, **kw), again.search(q, 10, **kw)
                    assert np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1])
            compact = str(tmp_path / f"compact_{rescore}.hzidx")
            h = ix.save(compact, compact=True)
            assert h["count"] == B.IX_N + T - 3 and np.array_equal(S.read_rows(compact), words[live])
            assert len(h["labels"]) == h["count"] and h["labels"][0] == "a1"


def test_every_by_name_refusal(files):
    p, v, _ = files
    q = vectors(2, 128)
    for name, version in (("v8", 8), ("v9t", 9)):
        what = f"a bin_sign index of version {version}"
        with S.RefIndex(p[name]) as ix:
            for call in (lambda: ix.search(q, 5, nprobe=2), lambda: ix.search(q, 5, nprobe="all"), lambda: ix.probes(q, 2),
                         lambda: ix.neighbors([0, 1], 5), lambda: ix.knn_graph(5), lambda: ix.cluster(3)):
                with pytest.raises(ValueError, match=what):
                    call()


def test_cli_index_dtype_bin_and_its_argument_errors(files, tmp_path):
    p, v, _ = files
    np.save(str(tmp_path / "v.npy"), v)

    def run(*args):
        return subprocess.run([sys.executable, "-m", "hipzap", "index", *args], capture_output=True, text=True, cwd=ROOT,
                              timeout=300)
    out = str(tmp_path / "cli9.hzidx")
    r = run("--vectors", str(tmp_path / "v.npy"), "--dtype", "bin", "--rescore", "--out", out)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["dtype"] == "bin_sign" and S.file_info(out)["version"] == 9
    assert np.array_equal(S.read_rows(out), S.prepare_rows_bin(v, "cosine"))
    out8 = str(tmp_path / "cli8.hzidx")
    r = run("--from-index", p["v1"], "--dtype", "bin", "--out", out8)
    assert r.returncode == 0 and S.file_info(out8)["version"] == 8, r.stderr
    r = subprocess.run([sys.executable, "-m", "hipzap", "info", out8], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and '"bin_sign"' in r.stdout and '"version": 8' in r.stdout, r.stdout + r.stderr
    for args, words in ((("--vectors", str(tmp_path / "v.npy"), "--dtype", "bin", "--ivf", "3"), "IVF lists over binary rows are not built"),
                        (("--from-index", p["v1"], "--dtype", "bin", "--ivf", "3"), "IVF lists over binary rows are not built"),
                        (("--from-index", p["fp8"], "--dtype", "bin"), "fp8_e4m3"),
                        (("--vectors", str(tmp_path / "v.npy"), "--dtype", "bits"), "invalid choice")):
        r = run(*args, "--out", str(tmp_path / "no.hzidx"))
        assert r.returncode != 0 and words in r.stderr, (args, r.stderr)
    assert not os.path.exists(str(tmp_path / "no.hzidx"))


def test_routes_on_a_binary_index_through_the_cpu_backend(tmp_path):
    import torch
    from transformers import BertConfig, BertModel
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    root = tmp_path
    torch.manual_seed(0)
    torch.save(BertModel(BertConfig(num_hidden_layers=1), add_pooling_layer=False).eval().state_dict(), str(root / "enc.pth"))
    corpus = np.random.default_rng(5).standard_normal((200, 768)).astype(np.float32)
    S.write_index(str(root / "v9.hzidx"), corpus, "cosine", dtype="bin", rescore=True)
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["v9"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={
        "embed": {"pooling": "mean", "normalize": True}, "seq_len": 32, "index": str(root / "v9.hzidx"),
        "index_writable": True, "index_rescore_rows": "host"})
    srv = ModelServer(st, backend="cpu")
    app_mod.set_server(srv)
    try:
        with app_mod.app.test_client() as client:
            q = np.random.default_rng(6).standard_normal((2, 768)).astype(np.float32)
            qn = S.normalize_rows(q)
            ref = S.RefIndex(str(root / "v9.hzidx"))
            for body, Rn in (({}, 128), ({"refine": 40}, 40), ({"refine": 0}, 0)):
                r = client.post("/search", json=dict(body, model="v9", vectors=q.tolist(), k=5))
                assert r.status_code == 200 and r.json["refine"] == Rn and r.json["dtype"] == "bin_sign", r.data
                assert [[h["id"] for h in row] for row in r.json["results"]] == ref.search(qn, 5, refine=Rn)[1].tolist()
            r = client.post("/search", json={"model": "v9", "vectors": q.tolist(), "k": 5, "nprobe": 2})
            assert r.status_code == 400 and "a bin_sign index of version 9" in r.json["message"], r.data
            new = np.random.default_rng(7).standard_normal((3, 768)).astype(np.float32)
            r = client.post("/index/add", json={"model": "v9", "vectors": new.tolist()})
            assert r.status_code == 200 and r.json["ids"] == [200, 201, 202], r.data
            r = client.post("/search", json={"model": "v9", "vectors": new.tolist(), "k": 1})
            assert [row[0]["id"] for row in r.json["results"]] == [200, 201, 202]
            assert client.post("/index/delete", json={"model": "v9", "ids": [200]}).json["deleted"] == 1
            r = client.post("/index/save", json={"model": "v9"})
            assert r.status_code == 200 and r.json["count"] == 203
            assert S.file_info(str(root / "v9.hzidx"))["version"] == 9 and S.file_info(str(root / "v9.hzidx"))["live"] == 202
    finally:
        srv.close()
        app_mod.set_server(None)
