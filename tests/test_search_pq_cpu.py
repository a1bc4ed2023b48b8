"""Product-quantised (pq8) indexes on the host: training, encoding, the table and the scan's emulation, the .hzidx
versions 10 and 11, every reader refusal, RefIndex (the oracle and the CPU backend), the by-name refusals, the CLI's
argument errors and the routes. No GPU."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hipzap import search as S

import search_pq_cases as P
from search_pq_cases import T, u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vectors(n=300, d=128):
    i = np.arange(n * d, dtype=np.uint64)
    return (((i * np.uint64(2654435761)) % np.uint64(2003)).astype(np.float32) / np.float32(1001.5) - np.float32(1.0)).reshape(n, d)


TAGS = (np.arange(300) % 5).astype(np.uint32)


# ------------------------------------------------------------------------------------- train and encode
def test_pq_train_is_deterministic_and_its_distortion_does_not_rise():
    x = vectors(900, 64)
    a, b = S.pq_train(x, 16, seed=3, iters=3), S.pq_train(x, 16, seed=3, iters=3)
    assert a.dtype == np.float32 and a.shape == (16, 256, 4) and np.array_equal(u32(a), u32(b))
    assert not np.array_equal(a, S.pq_train(x, 16, seed=4, iters=3))
    few = S.pq_train(x, 16, seed=3, iters=3, sample=500)  # a sample: still deterministic, another codebook
    assert np.array_equal(few, S.pq_train(x, 16, seed=3, iters=3, sample=500)) and not np.array_equal(few, a)
    # one Lloyd iteration at a time through `init`: the same sample each time, so the chain is pq_train(iters=i).
    # Each step minimises the distortion over the assignment, then over the centroids; a centroid is the fp64 mean
    # rounded to fp32, which costs at most count * |c|^2 * 2^-48 -- far below the 1e-9 relative slack allowed here.
    cb, dist = S.pq_train(x, 16, seed=3, iters=0), []
    for i in range(5):
        dist.append(S.pq_distortion(x, cb))
        cb = S.pq_train(x, 16, seed=3, iters=1, init=cb)
    assert np.array_equal(cb, S.pq_train(x, 16, seed=3, iters=5))
    print("distortion per iteration:", dist)
    assert all(b <= a * (1 + 1e-9) for a, b in zip(dist, dist[1:])) and dist[-1] < dist[0]
    init = P.make("inexact", 1, 64, 16, 1)[1]
    assert np.array_equal(u32(S.pq_train(x, 16, iters=0, init=init)), u32(init))  # the identity
    for kw, msg in ((dict(m=8), "multiple of 16"), (dict(m=112), "16..96"), (dict(m=48), "multiple of m = 48"),
                    (dict(m=16, iters=-1), "iters"), (dict(m=16, init=init[:, :, :2]), "codebook must be")):
        with pytest.raises(ValueError, match=msg):
            S.pq_train(x, **kw)
    with pytest.raises(ValueError, match="dim / m in 1..64"):
        S.pq_train(np.zeros((4, 2048), np.float32), 16)  # dsub = 128


def test_pq_encode_picks_the_nearest_centroid_and_the_lower_index_on_ties():
    cb = np.full((16, 256, 2), 100.0, np.float32)
    cb[:, 3], cb[:, 9], cb[:, 200], cb[:, 201] = [1, 0], [-1, 0], [5, 5], [5, 5]
    x = np.zeros((4, 32), np.float32)   # row 0: equidistant from centroids 3 and 9 -> 3
    x[1] = np.tile([5, 5], 16)          # a duplicated centroid -> the lower index
    x[2] = np.tile([-0.9, 0.1], 16)     # nearest 9
    x[3] = np.tile([4, 4], 16)          # nearest 200 (distance 2) rather than 3 (distance 25)
    codes = S.pq_encode(x, cb)
    assert codes.dtype == np.uint8 and codes.tolist() == [[3] * 16, [200] * 16, [9] * 16, [200] * 16]
    rng = np.random.default_rng(0)
    cb = rng.standard_normal((16, 256, 8)).astype(np.float32)
    x = rng.standard_normal((50, 128)).astype(np.float32)
    d = ((x.reshape(50, 16, 1, 8).astype(np.float64) - cb[None].astype(np.float64)) ** 2).sum(axis=3)  # [50, 16, 256]
    assert np.array_equal(S.pq_encode(x, cb), d.argmin(axis=2))


@pytest.mark.parametrize("D,M", P.SHAPES)
def test_the_lossless_case_round_trips(D, M):
    codes, cb, q = P.make("lossless", 300, D, M, 3)
    x = S.pq_decode(codes, cb)
    assert x.dtype == np.float32 and x.shape == (300, D)
    assert np.array_equal(x, S.bf16_to_f32(S.to_bf16(x)))  # bf16-exact rows
    again = S.pq_encode(x, cb)
    assert np.array_equal(S.pq_decode(again, cb), x)  # the codes may name an equal centroid of lower index
    s_pq, i_pq = S.pq_search_ref(again, cb, q, 10)
    s_x, i_x = S.search_ref(x, q, 10)
    assert np.array_equal(i_pq, i_x) and np.array_equal(s_pq, s_x)  # PQ search IS exact search over the rows


@pytest.mark.parametrize("D,M", P.SHAPES)
@pytest.mark.parametrize("kind", P.KINDS)
def test_scores_from_the_table_stay_within_the_bound(kind, D, M):
    codes, cb, q = P.make(kind, 300, D, M, 3)
    lut, lb = P.lut_oracle(q, cb)
    assert np.allclose(lut, S.pq_lut_ref(q, cb), rtol=0, atol=0)
    lut32 = lut.astype(np.float32)  # one rounding per entry: within gamma(dsub) of the fp64 table
    got = S.pq_scores_from_lut(lut32, codes)
    s, b = P.score_oracle(codes, cb, q)
    assert got.dtype == np.float32 and got.shape == (3, 300) and (np.abs(got - s) <= b).all()
    assert np.array_equal(S.pq_scores_from_lut(lut32[1], codes), got[1])
    if kind != "inexact":  # every table entry and every partial sum is exact in fp32
        assert np.array_equal(lut32.astype(np.float64), lut) and np.array_equal(got.astype(np.float64), s)
        assert len(np.unique(got)) < got.size  # ties
    else:  # the order of the additions is part of the result
        rev = S.pq_scores_from_lut(lut32[:, ::-1], codes[:, ::-1])
        assert not np.array_equal(u32(rev), u32(got))
    ids = S.pq_search_ref(codes, cb, q, 10)[1]
    assert np.array_equal(ids, S.search_ref(S.pq_decode(codes, cb), q, 10)[1]) or kind == "inexact"


# ----------------------------------------------------------------------------------------------- files
# whole-file digests (sizes where k-means decides bytes) of what the parent commit's writer produced for `vectors()`
RECORDED = {
    "v1": "195c174d5587e1f9709b101293d590e4d17e64571f37dda6347c3f8d3f619797",
    "v2": "d4bfb3e64e2e01c4bfe0b26fbb4cb992aac8a970fd98cefc48af93e34c27a9f5",
    "v3": "503f58b08ba713ec400034a4cf11b00dde090c5b79af4e54cd5514f4ac09fea8",
    "v4": "1c78698e1a341be39432cb16f5c771ee01708e1e46644ab3af70fbfaa3088060",
    "v5": 224256, "v6": 130048, "v7": 207872,
    "v8": "fe46f9f7e6d30c1350a81f4211fefe33c76425284c15c744ce93d409b166a3ce",
    "v8t": "a4135cdf526b8a323d1676bd663499de99d09b24ebc8446fe9a8f82c9ffb3cb5",
    "v9": "239d2bed81b6c304f3466f159795201ee86ad0702de08bdfb4c480f6e09bb16e",
    "v9t": "45c4689933864c9d46af16be8d180963fa6554e0c3cb1c55ee5c361d1901efe8",
}


def test_versions_1_to_9_are_written_as_before(tmp_path):
    v, out = vectors(), {}
    for name, kw in (("v1", {}), ("v2", {"tags": TAGS}), ("v3", {"dtype": "fp8"}),
                     ("v4", {"dtype": "fp8", "rescore": True, "tags": TAGS}),
                     ("v5", {"tags": TAGS, "ivf": 3, "nprobe": 2, "ivf_seed": 1}), ("v8", {"dtype": "bin"}),
                     ("v8t", {"dtype": "bin", "tags": TAGS}), ("v9", {"dtype": "bin", "rescore": True}),
                     ("v9t", {"dtype": "bin", "rescore": True, "tags": TAGS})):
        out[name] = str(tmp_path / f"{name}.hzidx")
        S.write_index(out[name], v, "cosine", labels=[f"r{i}" for i in range(300)], model="m", **kw)
    out["v6"], out["v7"] = str(tmp_path / "v6.hzidx"), str(tmp_path / "v7.hzidx")
    S.convert_index(out["v5"], out["v6"], "fp8")
    S.convert_index(out["v5"], out["v7"], "fp8", rescore=True)
    for name, p in out.items():
        raw = open(p, "rb").read()
        want = RECORDED[name]
        assert (len(raw) if isinstance(want, int) else hashlib.sha256(raw).hexdigest()) == want, name
        assert S.file_info(p)["version"] == int(name[1]) and "pq" not in S.read_header(p)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("pq")
    v = vectors()
    cb = S.pq_train(S.bf16_to_f32(S.prepare_rows(v, "cosine")), 16, seed=1, iters=2)
    p = {k: str(root / f"{k}.hzidx") for k in ("v1", "v2", "v10", "v10t", "v11", "v11t", "fp8", "ivf")}
    labels = [f"r{i}" for i in range(300)]
    S.write_index(p["v1"], v, "cosine", labels=labels, model="m")
    S.write_index(p["v2"], v, "cosine", labels=labels, model="m", tags=TAGS)
    kw = dict(labels=labels, model="m", dtype="pq", pq_m=16, pq_codebook=cb)
    hdrs = {"v10": S.write_index(p["v10"], v, "cosine", **kw), "v10t": S.write_index(p["v10t"], v, "cosine", tags=TAGS, **kw),
            "v11": S.write_index(p["v11"], v, "cosine", rescore=True, **kw),
            "v11t": S.write_index(p["v11t"], v, "cosine", rescore=True, tags=TAGS, **kw)}
    S.write_index(p["fp8"], v, "cosine", dtype="fp8")
    S.write_index(p["ivf"], v, "cosine", ivf=3)
    return p, v, hdrs, cb


def test_version_10_and_11_byte_layout(files):
    p, v, hdrs, cb = files
    codes = S.pq_encode(S.bf16_to_f32(S.prepare_rows(v, "cosine")), cb)
    want = {"v10": (10, {}), "v10t": (10, {"tags_off": 143360, "live_off": 147456}), "v11": (11, {"rescore_off": 143360}),
            "v11t": (11, {"tags_off": 143360, "live_off": 147456, "rescore_off": 151552})}
    for name, (version, offs) in want.items():
        raw = open(p[name], "rb").read()
        magic, ver, jl, data_off, count, dim, metric = S.HEAD.unpack(raw[:S.HEAD.size])
        h = json.loads(raw[S.HEAD.size:S.HEAD.size + jl])
        assert (magic, ver, data_off, count, dim, metric) == (S.MAGIC, version, 4096, 300, 128, 0), name
        assert h == hdrs[name] and h["dtype"] == "pq8" and "scales_off" not in h
        assert h["pq"] == {"m": 16, "ksub": 256, "dsub": 8, "codebook_off": 12288}
        assert {k: h[k] for k in ("tags_off", "live_off", "rescore_off") if k in h} == offs, name
        assert ("capacity" in h) == ("tags_off" in h)
        assert raw[4096:4096 + 300 * 16] == codes.tobytes()  # uint8 [count][M]
        assert raw[12288:12288 + 131072] == cb.astype("<f4").tobytes()  # fp32 [M][256][dsub], where version 3 has scales
        end = 12288 + 131072
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
        assert (info["version"], info["dtype"], info["live"], info["tags"]) == (version, "pq8", 300, "tags_off" in h)
        assert info["pq"] == {"m": 16, "dsub": 8, "codebook_bytes": 131072}
        assert np.array_equal(S.read_rows(p[name]), codes) and S.read_rows(p[name]).dtype == np.uint8
        assert np.array_equal(u32(S.read_codebook(p[name])), u32(cb))
    assert np.array_equal(S.read_rescore_rows(p["v11"]), S.read_rows(p["v1"]))
    with pytest.raises(ValueError, match="no codebook"):
        S.read_codebook(p["v1"])


def test_write_index_and_convert_index_store_the_same_bytes(files, tmp_path):
    p, v, _, cb = files
    for src, rescore, same_as in (("v1", False, "v10"), ("v1", True, "v11"), ("v2", False, "v10t"), ("v2", True, "v11t")):
        dst = str(tmp_path / f"c_{src}_{rescore}.hzidx")
        h = S.convert_index(p[src], dst, "pq", rescore=rescore, pq_m=16, pq_codebook=cb)
        assert h["dtype"] == "pq8" and open(dst, "rb").read() == open(p[same_as], "rb").read()
    # and when both train: the rounded rows are the stored rows, so the codebooks and the codes agree too
    a, b = str(tmp_path / "a.hzidx"), str(tmp_path / "b.hzidx")
    S.write_index(a, v, "cosine", dtype="pq", pq_m=32, pq_seed=2, pq_iters=1)
    S.convert_index(p["v1"], b, "pq", pq_m=32, pq_seed=2, pq_iters=1)
    assert np.array_equal(S.read_rows(a), S.read_rows(b)) and np.array_equal(u32(S.read_codebook(a)), u32(S.read_codebook(b)))
    no = str(tmp_path / "no.hzidx")
    for kw, src, msg in ((dict(pq_m=16, ivf=3), "v1", "ivf=3 with dtype='pq'"), (dict(pq_m=16), "ivf", "dtype='pq'.*IVF lists"),
                         (dict(pq_m=16), "fp8", "dtype='pq'.*fp8_e4m3"), ({}, "v1", "needs pq_m"),
                         (dict(pq_m=48), "v1", "multiple of m = 48"), (dict(pq_m=24), "v1", "multiple of 16")):
        with pytest.raises(ValueError, match=msg):
            S.convert_index(p[src], no, "pq", **kw)
    for kw, msg in ((dict(dtype="pq", pq_m=16, ivf=3), "ivf=3 with dtype='pq'"), (dict(dtype="pq"), "needs pq_m"),
                    (dict(dtype="pq", pq_m=16, pq_codebook=cb[:, :, :4]), "codebook must be"),
                    (dict(dtype="fp8", pq_m=16), "go with dtype='pq'"), (dict(dtype="pq", pq_m=128), "16..96")):
        with pytest.raises(ValueError, match=msg):
            S.write_index(no, v, "cosine", **kw)
    assert not os.path.exists(no)


def _rewrite(src, dst, version=None, edit=None, cut=None, dim=None):
    """A copy of ``src`` with another version word or dim, an edited JSON header (same length) or a shorter tail."""
    raw = bytearray(open(src, "rb").read())
    jl = S.HEAD.unpack(raw[:S.HEAD.size])[2]
    if version is not None:
        raw[8:12] = np.array([version], "<u4").tobytes()
    if dim is not None:
        raw[32:36] = np.array([dim], "<u4").tobytes()
    if edit is not None:
        new = edit(raw[S.HEAD.size:S.HEAD.size + jl].decode())
        assert len(new) <= jl, (len(new), jl)
        raw[S.HEAD.size:S.HEAD.size + jl] = new.ljust(jl).encode()
    if cut is not None:
        raw = raw[:cut]
    open(dst, "wb").write(bytes(raw))
    return dst


def reader_refusals():
    """(name, source, rewrite arguments, words of the Python message, words of the native message)."""
    def sub(a, b):
        return lambda s: s.replace(a, b)

    def bf16(s):  # one byte longer, taken back from the model's name
        return s.replace('"pq8"', '"bf16"').replace('"model": "m"', '"model": ""')
    return [
        ("pq dtype in version 3", "v10", dict(version=3), "version-3", "dtype"),
        ("bf16 dtype in version 10", "v10", dict(edit=bf16), "version-10", "dtype"),
        ("bf16 dtype in version 11", "v11", dict(edit=bf16), "version-11", "dtype"),
        ("version 10 with rescore keys", "v11", dict(version=10), "rescore keys in a version-10", "rescore keys"),
        ("version 11 without them", "v10", dict(version=11), "version-11 file without rescore", "without rescore"),
        ("no pq block", "v10", dict(edit=sub('"pq":', '"qp":')), "without a pq block", "without a pq block"),
        ("pq block without m", "v10", dict(edit=sub('"m": 16', '"n": 16')), "without a pq block", "pq block lacks m"),
        ("malformed codebook_off", "v10", dict(edit=sub('"codebook_off": 12288', '"codebook_off": "x"  ')), "without a pq block",
         "pq block lacks codebook_off"),
        ("ksub 128", "v10", dict(edit=sub('"ksub": 256', '"ksub": 128')), "ksub must be 256", "ksub must be 256"),
        ("m % 16", "v10", dict(edit=sub('"m": 16, "ksub": 256, "dsub": 8', '"m": 8, "ksub": 256, "dsub": 16')), "multiple of 16", "m % 16"),
        ("m > 96", "v10", dict(edit=lambda s: bf16(s.replace('"m": 16, "ksub": 256, "dsub": 8', '"m": 128, "ksub": 256, "dsub": 1')).replace('"bf16"', '"pq8"')),
         "16..96", "m <= 96"),
        ("dim % m", "v10", dict(edit=sub('"m": 16', '"m": 48')), "multiple of m = 48", "dim % m"),
        ("dsub disagrees", "v10", dict(edit=sub('"dsub": 8', '"dsub": 4')), "dsub 4 is not dim / m", "dsub"),
        ("ivf block", "v10t", dict(edit=sub('"capacity": 300', '"ivf": {}')), "ivf block", "ivf block"),
        ("unaligned codebook", "v10", dict(edit=sub('"codebook_off": 12288', '"codebook_off": 12292')), "codebook block", "codebook block"),
        ("codebook over the rows", "v10", dict(edit=sub('"codebook_off": 12288', '"codebook_off": 4096 ')), "codebook block", "codebook block"),
        ("codebook outside the file", "v10", dict(cut=12288 + 1000), "codebook block", "codebook block"),
        ("tags over the codebook", "v10t", dict(edit=sub('"tags_off": 143360', '"tags_off": 12288 ')), "tags block", "tags or live block"),
        ("unaligned tags", "v10t", dict(edit=sub('"tags_off": 143360', '"tags_off": 143364')), "tags block", "tags or live block"),
        ("rescore over the live block", "v11t", dict(edit=sub('"rescore_off": 151552', '"rescore_off": 147456')),
         "overlaps another block", "rescore block"),
        ("unaligned rescore", "v11", dict(edit=sub('"rescore_off": 143360', '"rescore_off": 143368')), "rescore_off", "rescore block"),
        ("rows outside the file", "v10", dict(cut=4096 + 100), "row block", "row block"),
        ("live outside the file", "v10t", dict(cut=147456 + 8), "live block", "tags or live block"),
        ("rescore outside the file", "v11", dict(cut=143360 + 1000), "rescore block lies outside", "rescore block"),
        ("pq block in version 2", "v10t", dict(version=2, edit=bf16), "pq block belongs", "pq block in a version-2"),
    ]


def test_every_reader_refusal(files, tmp_path):
    p = files[0]
    for name, src, kw, words, _ in reader_refusals():
        bad = _rewrite(p[src], str(tmp_path / "bad.hzidx"), **kw)
        with pytest.raises(ValueError, match=words):
            S.read_header(bad)
    for src in ("v10", "v10t", "v11", "v11t"):  # and the files as written are accepted
        assert S.read_header(p[src])["dtype"] == "pq8"


def test_the_native_reader_refuses_the_same_files_before_it_touches_a_device(files, tmp_path):
    from hipzap import _native as N
    from hipzap.ops import search as OS  # noqa: F401  (the signatures)
    lib, p = N.lib(), files[0]
    for name, src, kw, _, words in reader_refusals():
        bad = _rewrite(p[src], str(tmp_path / "bad.hzidx"), **kw)
        assert not lib.hz_index_open3(os.fsencode(bad), 0, 1, 0, 0), name
        assert words in lib.hz_index_last_error().decode(), (name, lib.hz_index_last_error())


def test_the_kinds_are_registered_and_refuse_without_a_device():
    from hipzap import _native as N
    from hipzap.ops import search as OS
    lib = N.lib()
    assert (N.HZ_K_SEARCH_PQLUT, N.HZ_K_SEARCH_PQSCAN) == (46, 47)
    assert lib.hz_kernel_name(46) == b"HZ_K_SEARCH_PQLUT" and lib.hz_kernel_name(47) == b"HZ_K_SEARCH_PQSCAN"
    assert lib.hz_kernel_param_size(46) == C.sizeof(OS.PqLutParams) and lib.hz_kernel_param_size(47) == C.sizeof(OS.PqScanParams)
    lp = OS.PqLutParams(16, 16, 16, 16 * 16 * 1024, 128, 16, 1, 0)
    for field, value, code in (("queries", 0, -112), ("M", 24, -114), ("M", 112, -115), ("D", 120, -113), ("D", 2064, -116),
                               ("Q", 0, -120), ("Q", 17, -120), ("lut", 24, -122), ("lut_bytes", 1023 * 16, -127)):
        bad = OS.PqLutParams.from_buffer_copy(lp)
        setattr(bad, field, value)
        assert lib.hz_launch_kernel(N.HZ_K_SEARCH_PQLUT, C.byref(bad), None) == code, (field, value)
    big = OS.PqLutParams(16, 16, 16, 1 << 30, 4096, 64, 1, 0)  # dsub 64 is allowed, D > 2048 is not
    assert lib.hz_launch_kernel(N.HZ_K_SEARCH_PQLUT, C.byref(big), None) == -117


# --------------------------------------------------------------------------------------------- RefIndex
def test_the_index_fixture_is_unambiguous_under_the_bound(tmp_path):
    """tests/test_search_pq_index_gpu.py compares ids with the fp64 RefIndex: no query's top-k may hinge on a gap
    smaller than the contract's bound, over all rows and over each filter the test uses."""
    A, Bv, cb, q = P.index_data()
    p = str(tmp_path / "ix.hzidx")
    S.write_index(p, np.concatenate([A, Bv]), "ip", dtype="pq", pq_m=P.IX_M, pq_codebook=cb)
    codes = S.read_rows(p)
    s, b = P.score_oracle(codes, cb, q)
    n = codes.shape[0]
    tags = P.index_tags(n)
    live = np.ones(n, bool)
    live[[0, 5, P.IX_N + 1]] = False
    for rows in (np.arange(n) < P.IX_N, np.ones(n, bool), live, live & (tags == 1)):
        for k in (P.IX_K, 40):
            assert P.subset_ambiguous(s, b, k, rows) == 0


def test_refindex_live_scenario_save_and_compact(tmp_path):
    A, Bv, cb, q = P.index_data()
    for rescore in (False, True):
        p = str(tmp_path / f"live_{rescore}.hzidx")
        S.write_index(p, A, "ip", dtype="pq", pq_m=P.IX_M, pq_codebook=cb, rescore=rescore, labels=[f"a{i}" for i in range(P.IX_N)])
        with S.RefIndex(p, reserve=2 * T) as ix:
            d = ix.describe()
            assert (d["dtype"], ix.version, d["m"], d["dsub"], d["codebook_bytes"]) == ("pq8", 11 if rescore else 10, 16, 8, 131072)
            assert ix.capacity() == 2 * T
            with pytest.raises(ValueError, match="labels are required"):
                ix.add(Bv)
            ids = ix.add(Bv, tags=P.index_tags(T, P.IX_N), labels=[f"b{i}" for i in range(T)])
            assert ids.tolist() == list(range(P.IX_N, P.IX_N + T)) and ix.count == P.IX_N + T and ix.capacity() == 4 * T
            codes = np.concatenate([S.prepare_rows_pq(A, "ip", 16, cb)[0], S.prepare_rows_pq(Bv, "ip", 16, cb)[0]])
            assert np.array_equal(ix._state()[0], codes)
            assert ix.delete([0, 5, 5, P.IX_N + 1]) == 3
            ix.set_tags([7, 8], [9, 9])
            live = np.ones(P.IX_N + T, bool)
            live[[0, 5, P.IX_N + 1]] = False
            s, i = ix.search(q, 10, refine=0)
            ws, wi = S.pq_search_ref(codes, cb, q, 10, live)
            assert np.array_equal(i, wi) and np.array_equal(u32(s), u32(ws.astype(np.float32)))
            s, i = ix.search(q, 10, filter=(0xFFFFFFFF, 9), refine=0)
            assert (np.sort(i[:, :2], axis=1) == [7, 8]).all() and (i[:, 2:] == -1).all()
            if rescore:  # R covers every passing row: the bf16 answer
                bf = str(tmp_path / "bf.hzidx")
                S.write_index(bf, np.concatenate([A, Bv]), "ip", tags=np.concatenate([np.zeros(P.IX_N, np.uint32), P.index_tags(T, P.IX_N)]))
                with S.RefIndex(bf) as ref:
                    a, b = ix.search(q, 10, filter=(0xFFFFFFFF, 1), refine=128), ref.search(q, 10, filter=(0xFFFFFFFF, 1))
                    assert np.array_equal(a[1], b[1]) and np.array_equal(u32(a[0]), u32(b[0]))
            else:
                with pytest.raises(ValueError, match="refine must be None or 0.*pq8 index of version 10"):
                    ix.search(q, 10, refine=40)
            saved = str(tmp_path / f"saved_{rescore}.hzidx")
            h = ix.save(saved)
            assert S.file_info(saved)["version"] == (11 if rescore else 10) and h["capacity"] == 4 * T and "tags_off" in h
            assert np.array_equal(S.read_rows(saved), codes) and np.array_equal(S.read_live(saved), live)
            assert np.array_equal(u32(S.read_codebook(saved)), u32(cb))
            with S.RefIndex(saved) as again:
                for kw in ({}, {"filter": (3, 1)}):
                    a, b = ix.search(q, 10, **kw), again.search(q, 10, **kw)
                    assert np.array_equal(u32(a[0]), u32(b[0])) and np.array_equal(a[1], b[1])
            compact = str(tmp_path / f"compact_{rescore}.hzidx")
            h = ix.save(compact, compact=True)
            assert h["count"] == P.IX_N + T - 3 and np.array_equal(S.read_rows(compact), codes[live])
            assert len(h["labels"]) == h["count"] and h["labels"][0] == "a1"


def test_every_by_name_refusal(files):
    p, v = files[0], files[1]
    q = vectors(2, 128)
    for name, version in (("v10", 10), ("v11t", 11)):
        what = f"a pq8 index of version {version}"
        with S.RefIndex(p[name]) as ix:
            for call in (lambda: ix.search(q, 5, nprobe=2), lambda: ix.search(q, 5, nprobe="all"), lambda: ix.probes(q, 2),
                         lambda: ix.neighbors([0, 1], 5), lambda: ix.knn_graph(5), lambda: ix.cluster(3),
                         lambda: ix.search_batch(q, 5)):
                with pytest.raises(ValueError, match=what):
                    call()


def test_cli_index_dtype_pq_and_its_argument_errors(files, tmp_path):
    p, v = files[0], files[1]
    np.save(str(tmp_path / "v.npy"), v)

    def run(*args):
        return subprocess.run([sys.executable, "-m", "hipzap", "index", *args], capture_output=True, text=True, cwd=ROOT,
                              timeout=300)
    out = str(tmp_path / "cli11.hzidx")
    r = run("--vectors", str(tmp_path / "v.npy"), "--dtype", "pq", "--pq-m", "16", "--pq-iters", "1", "--pq-seed", "2", "--rescore",
            "--out", out)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["dtype"] == "pq8" and S.file_info(out)["version"] == 11
    want = S.prepare_rows_pq(v, "cosine", 16, seed=2, iters=1)
    assert np.array_equal(S.read_rows(out), want[0]) and np.array_equal(S.read_codebook(out), want[1])
    out10 = str(tmp_path / "cli10.hzidx")
    r = run("--from-index", p["v1"], "--dtype", "pq", "--pq-m", "16", "--pq-iters", "1", "--pq-seed", "2", "--out", out10)
    assert r.returncode == 0 and S.file_info(out10)["version"] == 10, r.stderr
    assert np.array_equal(S.read_rows(out10), want[0])
    r = subprocess.run([sys.executable, "-m", "hipzap", "info", out10], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0 and '"pq8"' in r.stdout and '"version": 10' in r.stdout, r.stdout + r.stderr
    vn = str(tmp_path / "v.npy")
    for args, words in ((("--vectors", vn, "--dtype", "pq", "--pq-m", "16", "--ivf", "3"), "IVF lists over pq8 rows are not built"),
                        (("--from-index", p["v1"], "--dtype", "pq", "--pq-m", "16", "--ivf", "3"), "IVF lists over pq8 rows are not built"),
                        (("--vectors", vn, "--dtype", "pq"), "needs --pq-m"),
                        (("--vectors", vn, "--dtype", "fp8", "--pq-m", "16"), "go with --dtype pq"),
                        (("--vectors", vn, "--dtype", "pq", "--pq-m", "48"), "multiple of m = 48"),
                        (("--from-index", p["fp8"], "--dtype", "pq", "--pq-m", "16"), "fp8_e4m3")):
        r = run(*args, "--out", str(tmp_path / "no.hzidx"))
        assert r.returncode != 0 and words in r.stderr, (args, r.stderr)
    assert not os.path.exists(str(tmp_path / "no.hzidx"))


def test_routes_on_a_pq_index_through_the_cpu_backend(tmp_path):
    import torch
    from transformers import BertConfig, BertModel
    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings
    root = tmp_path
    torch.manual_seed(0)
    torch.save(BertModel(BertConfig(num_hidden_layers=1), add_pooling_layer=False).eval().state_dict(), str(root / "enc.pth"))
    corpus = np.random.default_rng(5).standard_normal((200, 768)).astype(np.float32)
    S.write_index(str(root / "v11.hzidx"), corpus, "cosine", dtype="pq", pq_m=48, pq_iters=1, rescore=True)
    st = Settings(default_model="resnet18", artifact_root=str(root))
    st.models["v11"] = ModelSpec(name="bert-base", key="enc.pth", batch=2, extra={
        "embed": {"pooling": "mean", "normalize": True}, "seq_len": 32, "index": str(root / "v11.hzidx"),
        "index_writable": True, "index_rescore_rows": "host"})
    srv = ModelServer(st, backend="cpu")
    app_mod.set_server(srv)
    try:
        with app_mod.app.test_client() as client:
            q = np.random.default_rng(6).standard_normal((2, 768)).astype(np.float32)
            qn = S.normalize_rows(q)
            ref = S.RefIndex(str(root / "v11.hzidx"))
            for body, Rn in (({}, 128), ({"refine": 40}, 40), ({"refine": 0}, 0)):
                r = client.post("/search", json=dict(body, model="v11", vectors=q.tolist(), k=5))
                assert r.status_code == 200 and r.json["refine"] == Rn and r.json["dtype"] == "pq8", r.data
                assert [[h["id"] for h in row] for row in r.json["results"]] == ref.search(qn, 5, refine=Rn)[1].tolist()
            for body in ({"nprobe": 2}, {"batch": True}):
                r = client.post("/search", json=dict(body, model="v11", vectors=q.tolist(), k=5))
                assert r.status_code == 400 and "a pq8 index of version 11" in r.json["message"], r.data
            new = np.random.default_rng(7).standard_normal((3, 768)).astype(np.float32)
            r = client.post("/index/add", json={"model": "v11", "vectors": new.tolist()})
            assert r.status_code == 200 and r.json["ids"] == [200, 201, 202], r.data
            r = client.post("/search", json={"model": "v11", "vectors": new.tolist(), "k": 1})
            assert [row[0]["id"] for row in r.json["results"]] == [200, 201, 202]
            assert client.post("/index/delete", json={"model": "v11", "ids": [200]}).json["deleted"] == 1
            r = client.post("/index/save", json={"model": "v11"})
            assert r.status_code == 200 and r.json["count"] == 203
            info = S.file_info(str(root / "v11.hzidx"))
            assert info["version"] == 11 and info["live"] == 202
    finally:
        srv.close()
        app_mod.set_server(None)
