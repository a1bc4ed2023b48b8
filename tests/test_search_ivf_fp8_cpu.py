"""fp8 IVF indexes on the host: the version-6 and version-7 files, the ``convert_index`` forms that
write them, the readers' refusals, ``RefIndex`` with ``nprobe`` and ``refine`` together, the command line and the
routes on the CPU backend; and that every query of tests/test_search_ivf_fp8_index_gpu.py is forced
(``search_ivf_fp8_cases.forced``), so a GPU disagreement there is a kernel error and not a tie."""
import json

import numpy as np
import pytest

from hipzap import search as S
from hipzap.__main__ import main as cli

import search_ivf_fp8_cases as V
from search_ivf_fp8_cases import T


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(u32(a[0]), u32(b[0]))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return V.write_files(tmp_path_factory.mktemp("ivf_fp8"))


@pytest.fixture(scope="module")
def data():
    return V.clustered_data()


# ------------------------------------------------------------------------------------------ the files
def test_version_5_converts_to_6_and_7(files):
    h5, h6, h7 = (S.read_header(files[k]) for k in ("v5", "v6", "v7"))
    t5 = S.read_ivf(files["v5"])
    real = t5["rowid"] >= 0
    cap = h5["capacity"]
    for key, h in (("v6", h6), ("v7", h7)):
        p = files[key]
        raw = open(p, "rb").read()
        assert S.HEAD.unpack(raw[:S.HEAD.size])[1] == int(key[1]) and S.file_info(p)["version"] == int(key[1])
        assert h["dtype"] == S.FP8 and h["count"] == V.IX_N and h["capacity"] == cap and h["scales_off"] % S.ALIGN == 0
        assert {k: h["ivf"][k] for k in ("nlist", "nprobe", "seed", "iters")} == {k: h5["ivf"][k] for k in ("nlist", "nprobe", "seed", "iters")}
        t = S.read_ivf(p)
        assert all(np.array_equal(t[k], t5[k]) for k in ("centroids", "list_off", "list_tiles", "rowid", "pos", "list_of"))
        assert np.array_equal(S.read_tags(p), S.read_tags(files["v5"])) and np.array_equal(S.read_live(p), S.read_live(files["v5"]))
        # codes and scales of every real row are the plain conversion's, byte for byte; padding: code 0, scale 1, dead
        codes, scales = S.read_rows(p), S.read_scales(p)
        assert codes.dtype == np.uint8 and codes.shape == (cap, V.IX_D) and scales.shape == (cap,)
        assert np.array_equal(codes[real], S.read_rows(files["p3"])[t["rowid"][real]])
        assert np.array_equal(u32(scales[real]), u32(S.read_scales(files["p3"])[t["rowid"][real]]))
        assert not codes[~real].any() and (scales[~real] == 1).all() and not S.read_live(p)[~real].any()
    assert "rescore_off" not in h6 and h7["rescore"] == "bf16" and h7["rescore_off"] % S.ALIGN == 0
    # the rescore block: id order, the plain bf16 index's rows, the last block of the file
    assert np.array_equal(S.read_rescore_rows(files["v7"]), S.read_rows(files["plain"]))
    assert h7["rescore_off"] > h7["ivf"]["rowid_off"] and h7["rescore_off"] + 2 * V.IX_N * V.IX_D == len(open(files["v7"], "rb").read())
    with pytest.raises(ValueError, match="without rescore rows"):
        S.read_rescore_rows(files["v6"])
    info = S.file_info(files["v7"])
    assert info["dtype"] == S.FP8 and info["rescore"] == "bf16" and info["ivf"]["nlist"] == V.IX_LISTS and info["live"] == V.IX_N


def test_a_plain_index_converts_with_ivf_to_5_6_and_7(files, data, tmp_path):
    v, q = data
    out = {}
    for name, kw in (("5", {"dtype": "bf16"}), ("6", {"dtype": "fp8"}), ("7", {"dtype": "fp8", "rescore": True})):
        out[name] = str(tmp_path / f"c{name}.hzidx")
        h = S.convert_index(files["plain"], out[name], ivf=V.IX_LISTS, nprobe=2, ivf_seed=0, **kw)
        assert S.file_info(out[name])["version"] == int(name) and h["ivf"]["nprobe"] == 2 and h["ivf"]["seed"] == 0
    # the lists are trained on the stored rows, which are what write_index(ivf=) trains on: the same files
    assert open(out["5"], "rb").read() == open(files["v5"], "rb").read()
    assert open(out["6"], "rb").read() == open(files["v6"], "rb").read()
    assert open(out["7"], "rb").read() == open(files["v7"], "rb").read()
    # a version-2 source with a deleted row and labels: the id stays, dead, in a list; labels, model, tags carried
    src, dst = str(tmp_path / "src.hzidx"), str(tmp_path / "dst.hzidx")
    S.write_index(src, v, "cosine", labels=[f"r{i}" for i in range(V.IX_N)], model="m", tags=V.index_tags())
    with S.RefIndex(src) as ix:
        ix.delete([17])
        ix.save()
    h = S.convert_index(src, dst, "fp8", rescore=True, ivf=4, ivf_seed=3, ivf_iters=2)
    assert h["labels"][17] == "r17" and h["model"] == "m" and (h["ivf"]["nlist"], h["ivf"]["nprobe"], h["ivf"]["iters"]) == (4, 4, 2)
    with S.RefIndex(dst) as ix:
        assert ix.version == 7 and not ix._live[17] and ix._live.sum() == V.IX_N - 1 and ix.ivf["list_of"][17] in range(4)
        assert np.array_equal(ix._tags, V.index_tags()) and 17 not in ix.search(q, 128, nprobe="all")[1]
    v1, d1 = str(tmp_path / "v1.hzidx"), str(tmp_path / "d1.hzidx")
    S.write_index(v1, v, "ip")
    assert S.convert_index(v1, d1, "bf16", ivf=5)["ivf"]["nprobe"] == 5 and S.read_live(d1).sum() == V.IX_N


# sizes and offsets of the files the unchanged calls write for the IX scenario (600 x 64, labels r0.., model "m")
RECORDED = {
    "v1": {"size": 84992, "data_off": 8192},
    "v2": {"size": 90188, "data_off": 8192, "tags_off": 86016, "live_off": 90112},
    "v3": {"size": 51552, "data_off": 8192, "scales_off": 49152},
    "v4": {"size": 138240, "data_off": 8192, "scales_off": 49152, "tags_off": 53248, "live_off": 57344, "rescore_off": 61440},
    "v5": {"size": 235520, "data_off": 8192, "tags_off": 204800, "live_off": 212992, "centroids_off": 217088,
           "list_off_off": 221184, "list_tiles_off": 225280, "rowid_off": 229376},
}


def test_versions_1_to_5_are_written_as_before(data, tmp_path):
    v, _ = data

    def write_all(tag):
        out = {}
        for name, kw in (("v1", {}), ("v2", {"tags": V.index_tags()}), ("v3", {"dtype": "fp8"}),
                         ("v4", {"dtype": "fp8", "rescore": True, "tags": V.index_tags()}),
                         ("v5", {"tags": V.index_tags(), "ivf": V.IX_LISTS, "nprobe": 2, "ivf_seed": 1})):
            p = str(tmp_path / f"{name}_{tag}.hzidx")
            h = S.write_index(p, v, "cosine", labels=[f"r{i}" for i in range(V.IX_N)], model="m", **kw)
            raw = open(p, "rb").read()
            offs = {k: h[k] for k in ("scales_off", "tags_off", "live_off", "rescore_off") if k in h}
            offs.update({k: h["ivf"][k] for k in S.IVF_KEYS} if "ivf" in h else {})
            assert dict(offs, size=len(raw), data_off=S.HEAD.unpack(raw[:S.HEAD.size])[3]) == RECORDED[name], name
            out[name] = raw
        return out
    before = write_all("a")
    plain = str(tmp_path / "v1_a.hzidx")
    S.convert_index(str(tmp_path / "v5_a.hzidx"), str(tmp_path / "x7.hzidx"), "fp8", rescore=True)
    S.convert_index(plain, str(tmp_path / "x6.hzidx"), "fp8", ivf=3)
    assert before == write_all("b")
    assert [S.HEAD.unpack(before[k][:S.HEAD.size])[1] for k in ("v1", "v2", "v3", "v4", "v5")] == [1, 2, 3, 4, 5]
    # and the plain conversions are what they were: versions 3 and 4 of the stored bf16 rows, requantised
    p3, p4 = str(tmp_path / "p3.hzidx"), str(tmp_path / "p4.hzidx")
    S.convert_index(plain, p3, "fp8"), S.convert_index(plain, p4, "fp8", rescore=True)
    codes, scales = S.quantize_rows(S.bf16_to_f32(S.read_rows(plain)))
    assert (S.file_info(p3)["version"], S.file_info(p4)["version"], len(open(p3, "rb").read())) == (3, 4, RECORDED["v3"]["size"])
    assert np.array_equal(S.read_rows(p3), codes) and np.array_equal(u32(S.read_scales(p4)), u32(scales))
    assert np.array_equal(S.read_rescore_rows(p4), S.read_rows(plain))


# ------------------------------------------------------------------------------------------ the refusals
def _rewrite(src, dst, version=None, edit=None, cut=None):
    """A copy of ``src`` with another version word, an edited JSON header (same length) or a shorter tail."""
    raw = bytearray(open(src, "rb").read())
    magic, ver, jl, data_off, count, dim, metric = S.HEAD.unpack(raw[:S.HEAD.size])
    if version is not None:
        raw[8:12] = np.array([version], "<u4").tobytes()
    if edit is not None:
        js = raw[S.HEAD.size:S.HEAD.size + jl].decode()
        new = edit(js)
        assert len(new) == len(js), "the edit must keep the header's length"
        raw[S.HEAD.size:S.HEAD.size + jl] = new.encode()
    open(dst, "wb").write(bytes(raw[:cut] if cut else raw))


def _bump(key, by):
    """The JSON edit that moves offset ``key`` by ``by`` bytes (same number of digits)."""
    def edit(js):
        at = js.rindex(f'"{key}": ') + len(key) + 4
        end = at
        while js[end].isdigit():
            end += 1
        new = str(int(js[at:end]) + by)
        assert len(new) <= end - at
        return js[:at] + new + js[end:] + " " * (end - at - len(new))  # trailing spaces keep the length
    return edit


def test_the_readers_refuse_damaged_files(files, tmp_path):
    bad = str(tmp_path / "bad.hzidx")
    h6, h7 = S.read_header(files["v6"]), S.read_header(files["v7"])

    def refused(msg, src, **kw):
        _rewrite(src, bad, **kw)
        with pytest.raises(ValueError, match=msg):
            S.read_header(bad)
        with pytest.raises(ValueError, match=msg):
            S.RefIndex(bad)
    # a dtype or a key set that disagrees with the version
    refused("dtype bf16 in a version-6 file", files["v5"], version=6)
    refused("dtype fp8_e4m3 in a version-5 file", files["v6"], version=5)
    refused("version-7 file without rescore", files["v6"], version=7)
    refused("rescore keys in a version-6 file", files["v7"], version=6)
    refused("version-7 file without rescore", files["v7"], edit=lambda js: js.replace('"rescore": "bf16"', '"rescore": "fp16"'))
    refused("ivf block belongs", files["p3"], version=6)
    refused("ivf block belongs", files["p4"], version=7)
    refused("ivf block belongs", files["v6"], version=3)
    refused("ivf block lacks", files["v6"], edit=lambda js: js.replace('"rowid_off"', '"rowid_of_"'))
    refused("scales_off", files["v6"], edit=lambda js: js.replace('"scales_off"', '"scales_of_"'))
    refused("capacity", files["v6"], edit=_bump("capacity", -1))
    refused("out of range", files["v6"], edit=lambda js: js.replace('"nprobe": 2', '"nprobe": 7'))
    # blocks that are unaligned, overlap another or lie outside the file
    refused("scales_off .* is not a multiple", files["v6"], edit=_bump("scales_off", 4))
    refused("scales block at .* overlaps the rows", files["v6"], edit=_bump("scales_off", -4096))
    refused("scales block lies outside", files["v6"], edit=_bump("scales_off", 4096 * 40))
    refused("tags block lies outside", files["v6"], edit=_bump("tags_off", -4096 * 2))
    refused("live block lies outside", files["v6"], edit=_bump("live_off", 4096 * 40))
    refused("ivf block centroids", files["v6"], edit=_bump("centroids_off", -4096))
    refused("ivf block list_tiles", files["v6"], edit=_bump("list_tiles_off", 8))
    refused("ivf block rowid", files["v6"], cut=h6["ivf"]["rowid_off"] + 8)
    refused("rescore_off .* is not a multiple", files["v7"], edit=_bump("rescore_off", 2))
    refused("rescore block at .* overlaps another block", files["v7"], edit=_bump("rescore_off", -4096))
    refused("rescore block lies outside", files["v7"], cut=h7["rescore_off"] + 2 * V.IX_N * V.IX_D - 2)
    # dim % 16: a bf16 IVF file of dim 24 under an fp8 version word
    v24 = str(tmp_path / "d24.hzidx")
    S.write_index(v24, V.clustered_data(d=24)[0], "cosine", ivf=3)
    _rewrite(v24, bad, version=6, edit=lambda js: js.replace('"dtype": "bf16"', '"dtype": "fp8_"'))
    with pytest.raises(ValueError, match="disagrees"):
        S.read_header(bad)
    raw = bytearray(open(v24, "rb").read())
    js = raw[S.HEAD.size:S.HEAD.size + S.HEAD.unpack(raw[:S.HEAD.size])[2]].decode()
    grown = js.replace('"dtype": "bf16"', '"dtype": "fp8_e4m3", "scales_off": 0')
    raw[S.HEAD.size:S.HEAD.size + len(grown)] = grown.encode()  # the padding before data_off takes the longer header
    raw[8:16] = np.array([6, len(grown)], "<u4").tobytes()
    open(bad, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="dim of an fp8 index must be a multiple of 16"):
        S.read_header(bad)
    # the table checks of read_ivf hold for the new versions
    t = S.read_ivf(files["v6"])
    first, pad, ntile = int(np.flatnonzero(t["rowid"] >= 0)[0]), int(np.flatnonzero(t["rowid"] < 0)[0]), t["list_tiles"].size
    for src in (files["v6"], files["v7"]):
        hdr = S.read_header(src)
        for key, index, value, msg in (("list_off_off", 1, -1, "list_off does not rise"), ("list_off_off", 0, 1, "list_off does not rise"),
                                       ("list_tiles_off", 0, ntile, "outside"), ("list_tiles_off", 0, int(t["list_tiles"][1]), "names a tile twice"),
                                       ("rowid_off", pad, 0, "not a permutation"), ("rowid_off", first, V.IX_N, "not a permutation"),
                                       ("rowid_off", first, int(t["rowid"][first + 1]), "not a permutation")):
            raw = bytearray(open(src, "rb").read())
            off = hdr["ivf"][key] + 4 * index
            raw[off:off + 4] = np.array([value], "<i4").tobytes()
            open(bad, "wb").write(bytes(raw))
            with pytest.raises(ValueError, match=msg):
                S.RefIndex(bad)
        raw = bytearray(open(src, "rb").read())
        word = hdr["live_off"] + 4 * (pad // 32)
        raw[word:word + 4] = (np.frombuffer(bytes(raw[word:word + 4]), "<u4") | np.uint32(1 << (pad % 32))).astype("<u4").tobytes()
        open(bad, "wb").write(bytes(raw))
        with pytest.raises(ValueError, match="padding row of the IVF index is live"):
            S.read_ivf(bad)


def test_convert_refusals_name_the_value(files, tmp_path):
    out = str(tmp_path / "x.hzidx")
    for src in ("p3", "p4", "v6", "v7"):
        with pytest.raises(ValueError, match="only a bf16 index can be converted, this one holds fp8_e4m3"):
            S.convert_index(files[src], out, "fp8")
        with pytest.raises(ValueError, match="only a bf16 index can be converted"):
            S.convert_index(files[src], out, "fp8", ivf=4)
    with pytest.raises(ValueError, match=r"ivf=4: .* is an IVF index already \(nlist 6\)"):
        S.convert_index(files["v5"], out, "fp8", ivf=4)
    for bad in (0, -1, V.IX_N + 1, 70000, 2.5, True, "6"):
        with pytest.raises(ValueError, match="ivf must be an integer in 1..min"):
            S.convert_index(files["plain"], out, "fp8", ivf=bad)
    for bad in (0, 5, 129, "all"):
        with pytest.raises(ValueError, match="nprobe must be an integer in 1..min"):
            S.convert_index(files["plain"], out, "fp8", ivf=4, nprobe=bad)
    with pytest.raises(ValueError, match="ivf_seed and ivf_iters must be integers >= 0, got -1"):
        S.convert_index(files["plain"], out, "fp8", ivf=4, ivf_seed=-1)
    with pytest.raises(ValueError, match="nprobe=3.* go with ivf=nlist"):
        S.convert_index(files["plain"], out, "fp8", nprobe=3)
    with pytest.raises(ValueError, match="nprobe=3.* go with ivf=nlist"):
        S.convert_index(files["v5"], out, "fp8", nprobe=3)
    with pytest.raises(ValueError, match="rescore rows go with an fp8 index"):
        S.convert_index(files["v5"], out, "bf16", rescore=True)
    with pytest.raises(ValueError, match="dtype must be one of"):
        S.convert_index(files["v5"], out, "fp16")
    d24 = str(tmp_path / "d24.hzidx")
    S.write_index(d24, V.clustered_data(d=24)[0], "cosine", ivf=3)
    with pytest.raises(ValueError, match="multiple of 16 in 16..2048, got 24"):
        S.convert_index(d24, out, "fp8")
    # write_index keeps its refusals; the message now names the route
    v = V.clustered_data()[0]
    with pytest.raises(ValueError, match=r"ivf=4 goes with dtype='bf16'.*convert_index"):
        S.write_index(out, v, "cosine", ivf=4, dtype="fp8")
    with pytest.raises(ValueError, match="rescore"):
        S.write_index(out, v, "cosine", ivf=4, dtype="fp8", rescore=True)
    assert S.read_header(S.convert_index(files["v5"], out, "bf16") and out)["ivf"]["nlist"] == V.IX_LISTS  # a copy: version 5


# ------------------------------------------------------------------------------------------ RefIndex
def test_refindex_over_every_list_equals_the_plain_refindexes(files, data):
    v, q = data
    for key in ("v6", "v7"):
        with S.RefIndex(files[key]) as ix, S.RefIndex(files["p3"]) as r3, S.RefIndex(files["p4"]) as r4:
            assert ix.version == int(key[1]) and ix.rescore == (key == "v7") and ix.dtype == S.FP8
            for k in (1, 10, 128):
                for kw in ({}, {"filter": (0xFFFFFFFF, 3)}):
                    assert same(ix.search(q, k, nprobe="all", refine=0, **kw), r3.search(q, k, **kw))
                    if key == "v7":
                        assert same(ix.search(q, k, nprobe="all", refine=128, **kw), r4.search(q, k, refine=128, **kw))
                        assert same(ix.search(q, k, nprobe="all", **kw), r4.search(q, k, **kw))  # None: 128
            if key == "v7":
                assert same(ix.search(q, 10, nprobe=V.IX_LISTS, refine=40), r4.search(q, 10, refine=40))
            gone = [int(r3.search(q, 1)[1][0, 0]), 5]
            assert ix.delete(gone) == r3.delete(gone) == r4.delete(gone) == 2
            for r in (ix, r3, r4):
                r.set_tags([7, 8], [3, 3])
            assert same(ix.search(q, 10, nprobe="all", refine=0, filter=(0xFFFFFFFF, 3)), r3.search(q, 10, filter=(0xFFFFFFFF, 3)))
            if key == "v7":
                assert same(ix.search(q, 10, nprobe="all"), r4.search(q, 10))
            d = ix.describe()
            assert d["live"] == V.IX_N - 2 and d["dtype"] == S.FP8 and d["ivf"]["nlist"] == V.IX_LISTS
            assert d.get("rescore") == ("bf16" if key == "v7" else None)


def test_refindex_stage_one_is_search_ref_over_the_probed_lists(files, data):
    v, q = data
    with S.RefIndex(files["v7"]) as ix, S.RefIndex(files["v5"]) as r5, S.RefIndex(files["v6"]) as r6:
        for n in (1, 2):
            assert np.array_equal(ix.probes(q, n), r5.probes(q, n)) and np.array_equal(r6.probes(q, n), r5.probes(q, n))
            pr = ix.probes(q, n)
            near = (ix.ivf["list_of"][None, :, None] == pr[:, None, :]).any(axis=2)
            want1 = S.search_ref(ix._rows, q, 40, near, scales=ix.scales)
            assert same(r6.search(q, 40, nprobe=n), (want1[0].astype(np.float32), want1[1]))
            got = ix.search(q, 10, nprobe=n, refine=40)
            for qi in range(q.shape[0]):
                s, i = S.rescore_ref(ix._rrows, q[qi], want1[1][qi], 10)
                assert np.array_equal(got[1][qi], i) and np.array_equal(u32(got[0][qi]), u32(s.astype(np.float32)))
        assert same(ix.search(q, 10), ix.search(q, 10, nprobe=2, refine=128))  # the defaults: the header's nprobe, R = 128


def test_refindex_mutations_save_and_what_it_refuses(files, data, tmp_path):
    v, q = data
    for key in ("v6", "v7"):
        out = str(tmp_path / f"saved{key}.hzidx")
        with S.RefIndex(files[key]) as ix:
            with pytest.raises(ValueError, match="IVF indexes do not take add yet"):
                ix.add(v[:2])
            with pytest.raises(ValueError, match=r"IVF indexes do not take save\(compact=True\) yet"):
                ix.save(out, compact=True)
            with pytest.raises(ValueError, match="outside"):
                ix.delete([V.IX_N])
            for bad in (0, -1, 1.5, True, "some"):
                with pytest.raises(ValueError, match="nprobe must be an integer in 1.."):
                    ix.search(q, 10, nprobe=bad)
            if key == "v6":
                with pytest.raises(ValueError, match="refine=16: an IVF index has no rescore rows"):
                    ix.search(q, 10, refine=16)
            else:
                for bad in (5, 129, -1, 2.5, True):
                    with pytest.raises(ValueError, match="refine must be None, 0 or an integer"):
                        ix.search(q, 10, refine=bad)
            ix.delete([11]), ix.set_tags([12], [77])
            ix.save(out)
            want = [ix.search(q, 10, nprobe=n) for n in (1, 2, "all")]
        assert S.file_info(out)["version"] == int(key[1]) and S.file_info(out)["live"] == V.IX_N - 1
        a, b = S.read_ivf(out), S.read_ivf(files[key])
        assert all(np.array_equal(a[k], b[k]) for k in ("centroids", "list_off", "list_tiles", "rowid"))
        assert np.array_equal(S.read_rows(out), S.read_rows(files[key])) and np.array_equal(u32(S.read_scales(out)), u32(S.read_scales(files[key])))
        if key == "v7":
            assert np.array_equal(S.read_rescore_rows(out), S.read_rescore_rows(files[key]))
        with S.RefIndex(out) as again:
            assert all(same(again.search(q, 10, nprobe=n), w) for n, w in zip((1, 2, "all"), want))
            assert not again._live[11] and again._tags[12] == 77
    with S.RefIndex(files["v5"]) as r5:  # the bf16 IVF index keeps refusing refine
        with pytest.raises(ValueError, match="refine=16: an IVF index has no rescore rows"):
            r5.search(q, 10, refine=16)


# ------------------------------------------------------------------------------------------ forcing
def test_every_query_of_the_gpu_index_test_is_forced(files, data):
    v, q = data
    with S.RefIndex(files["v5"]) as r5:
        sizes = np.bincount(r5.ivf["list_of"], minlength=V.IX_LISTS)
        assert sizes.tolist() == [93, 62, 91, 45, 219, 90]  # one list above R = 128: stage one cuts there
        cover = r5._tags == V.COVER_FILTER[1]
        per_list = np.bincount(r5.ivf["list_of"][cover], minlength=V.IX_LISTS)
        # R = 128 covers every passing row of any two lists under the filter
        assert np.sort(per_list)[-2:].sum() <= V.MAX_K and per_list.max() <= 44, per_list
        for n in (1, 2):
            assert V.V.forced(r5, q, 10, n, allow=cover).all()  # version 5's answer under the filter
    with S.RefIndex(files["v6"]) as r6, S.RefIndex(files["v7"]) as r7:
        for n in (1, 2, V.IX_LISTS):
            for k in (1, 10):
                assert V.forced(r6, q, k, n).all(), (6, n, k)
                assert V.forced(r6, q, k, n, allow=r6._tags == 3).all(), (6, n, k, "filter")
                for R in (V.MAX_K, 40):
                    assert V.forced(r7, q, k, n, refine=R).all(), (7, n, k, R)
                assert V.forced(r7, q, k, n, refine=V.MAX_K, allow=cover).all(), (7, n, k, "cover")
        # the GPU test deletes the best row of each query and re-tags the next ones, then searches again
        first = r7.search(q, 10, nprobe=1)[1]
        r7.delete([int(i) for i in first[:, 0]]), r6.delete([int(i) for i in first[:, 0]])
        ids = [int(i) for i in first[:, 1]]
        r7.set_tags(ids, [77] * len(ids)), r6.set_tags(ids, [77] * len(ids))
        for n in (1, 2):
            assert V.forced(r6, q, 10, n).all() and V.forced(r7, q, 10, n, refine=V.MAX_K).all()
            assert V.forced(r6, q, 10, n, allow=r6._tags == 77).all()
            assert V.forced(r7, q, 10, n, refine=V.MAX_K, allow=r7._tags == 77).all()


# ------------------------------------------------------------------------------------------ the command line
def test_cli_builds_converts_and_describes(files, data, tmp_path, capsys):
    v, _ = data
    vec, tags = str(tmp_path / "v.npy"), str(tmp_path / "t.npy")
    np.save(vec, v), np.save(tags, V.index_tags())
    one = str(tmp_path / "one.hzidx")
    cli(["index", "--vectors", vec, "--tags", tags, "--out", one, "--ivf", "6", "--nprobe", "2", "--ivf-seed", "0", "--dtype", "fp8",
         "--rescore"])
    made = json.loads(capsys.readouterr().out)
    assert made["ivf"]["nlist"] == 6 and made["dtype"] == S.FP8 and made["rescore"] == "bf16"
    assert open(one, "rb").read() == open(files["v7"], "rb").read() and not list(tmp_path.glob("*.tmp"))
    six = str(tmp_path / "six.hzidx")
    cli(["index", "--vectors", vec, "--tags", tags, "--out", six, "--ivf", "6", "--nprobe", "2", "--ivf-seed", "0", "--dtype", "fp8"])
    capsys.readouterr()
    assert open(six, "rb").read() == open(files["v6"], "rb").read()
    for src, flags, want in ((files["v5"], ["--dtype", "fp8"], files["v6"]), (files["v5"], ["--dtype", "fp8", "--rescore"], files["v7"]),
                             (files["plain"], ["--ivf", "6", "--nprobe", "2", "--ivf-seed", "0"], files["v5"]),
                             (files["plain"], ["--ivf", "6", "--nprobe", "2", "--ivf-seed", "0", "--dtype", "fp8", "--rescore"], files["v7"])):
        out = str(tmp_path / "conv.hzidx")
        cli(["index", "--from-index", src, *flags, "--out", out])
        capsys.readouterr()
        assert open(out, "rb").read() == open(want, "rb").read(), flags
    cli(["info", files["v7"]])
    info = json.loads(capsys.readouterr().out)
    assert (info["version"], info["dtype"], info["rescore"]) == (7, S.FP8, "bf16")
    assert info["ivf"]["nlist"] == 6 and info["ivf"]["padding_rows"] == info["capacity"] - V.IX_N
    cli(["info", files["v6"]])
    info = json.loads(capsys.readouterr().out)
    assert info["version"] == 6 and "rescore" not in info and info["ivf"]["nprobe"] == 2
    with pytest.raises(SystemExit, match="go with --ivf"):
        cli(["index", "--from-index", files["plain"], "--nprobe", "3", "--out", one])
    with pytest.raises(SystemExit, match="is an IVF index already"):
        cli(["index", "--from-index", files["v5"], "--ivf", "4", "--out", one])
    with pytest.raises(SystemExit, match="only a bf16 index can be converted"):
        cli(["index", "--from-index", files["v6"], "--dtype", "fp8", "--out", one])


# ------------------------------------------------------------------------------------------ the routes
@pytest.fixture()
def served(files, tmp_path, monkeypatch):
    import shutil

    from hipzap.serve import app as app_mod
    from hipzap.serve.server import ModelServer
    from hipzap.serve.settings import ModelSpec, Settings

    class Embedder:  # what the routes need of an embedding backend; the requests below carry their own vectors
        backend = "cpu"
        embed = {"dim": V.IX_D, "pooling": "mean", "normalize": True}
    for k in ("v6", "v7"):
        shutil.copy(files[k], tmp_path / f"{k}.hzidx")
    st = Settings(default_model="resnet18", artifact_root=str(tmp_path))
    for name, extra in (("v6", {"index": "v6.hzidx"}), ("v7", {"index": "v7.hzidx", "index_writable": True}),
                        ("v7n1", {"index": "v7.hzidx", "index_nprobe": 1, "index_rescore_rows": "host"})):
        st.models[name] = ModelSpec(name="bert-base", key="none.pth", extra=dict(extra, embed=Embedder.embed))
    srv = ModelServer(st, backend="cpu")
    monkeypatch.setattr(app_mod, "_embedding_backend", lambda s, model: Embedder)
    app_mod.set_server(srv)
    with app_mod.app.test_client() as c:
        yield c, str(tmp_path / "v7.hzidx")
    srv.close()
    app_mod.set_server(None)


def test_routes_take_nprobe_and_refine_together(served, data):
    client, path = served
    _, q = data

    def post(model="v7", **kw):
        return client.post("/search", json=dict({"model": model, "vectors": q.tolist(), "k": 10}, **kw))

    def ids(r):
        assert r.status_code == 200, r.data
        return [[h["id"] for h in row] for row in r.json["results"]]
    with S.RefIndex(path) as ref:
        r = post()
        assert ids(r) == ref.search(q, 10, nprobe=2, refine=128)[1].tolist()
        assert (r.json["ivf"], r.json["nprobe"], r.json["refine"], r.json["dtype"]) == (True, 2, 128, S.FP8)
        r = post(nprobe=1, refine=40, tag=3)
        assert ids(r) == ref.search(q, 10, nprobe=1, refine=40, filter=(0xFFFFFFFF, 3))[1].tolist()
        assert (r.json["nprobe"], r.json["refine"]) == (1, 40)
        r = post(nprobe="all", refine=0)
        assert ids(r) == ref.search(q, 10, nprobe="all", refine=0)[1].tolist() and (r.json["nprobe"], r.json["refine"]) == ("all", 0)
        r = post(model="v7n1")
        assert ids(r) == ref.search(q, 10, nprobe=1)[1].tolist() and (r.json["nprobe"], r.json["refine"]) == (1, 128)
        r = post(model="v6", nprobe=1)
        assert ids(r) == ref.search(q, 10, nprobe=1, refine=0)[1].tolist() and (r.json["refine"], r.json["dtype"]) == (0, S.FP8)
        r = post(model="v6", refine=16)
        assert r.status_code == 400 and "no rescore rows" in r.json["message"]
        for bad in (5, 129, "many"):
            r = post(refine=bad)
            assert r.status_code == 400 and "refine" in r.json["message"], bad
        assert post(nprobe=0, refine=16).status_code == 400
        r = client.post("/index/add", json={"model": "v7", "vectors": q[:1].tolist()})
        assert r.status_code == 400 and "IVF indexes do not take add yet" in r.json["message"]
        gone = ids(post())[0][:2]
        r = client.post("/index/delete", json={"model": "v7", "ids": gone})
        assert r.status_code == 200 and r.json["deleted"] == ref.delete(gone) == 2
        assert ids(post()) == ref.search(q, 10)[1].tolist()
        assert client.post("/index/save", json={"model": "v7"}).status_code == 200
    assert S.file_info(path)["version"] == 7 and S.file_info(path)["live"] == V.IX_N - 2
