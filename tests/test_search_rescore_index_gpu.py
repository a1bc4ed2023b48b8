"""The two-stage GPU index (csrc/index.cpp, a version-4 ``.hzidx``): fp8 scan and merge at k = R, then the rescore
kernel over the bf16 rows held in device memory or in pinned host memory.

Two GPU runs are compared bit for bit; against ``RefIndex`` ids are compared, and tests/test_search_rescore_cpu.py
asserts on the host that every such answer is forced (the seeds of tests/search_rescore_cases.py)."""
import ctypes as C

import numpy as np
import pytest

from hipzap import search as S

import search_rescore_cases as R

pytestmark = pytest.mark.gpu
PLACES = ("device", "host")


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(u32(a[0]), u32(b[0]))


@pytest.mark.parametrize("place", PLACES)
def test_equals_the_bf16_index_when_r_covers_every_passing_row(tmp_path, place):
    v, tags, q = R.covered_data()
    p4, _, p1 = R.write_pair(tmp_path, v, tags=tags)
    with S.Index(p4, rescore_rows=place) as two, S.Index(p1) as bf:
        d = two.describe()
        assert d["rescore_rows"] == place and d["rescore"] == "bf16" and "rescore_rows" not in bf.describe()
        qn = S.normalize_rows(q)
        got, want = two.search(qn, 10, filter=R.COVER_FILTER, refine=128), bf.search(qn, 10, filter=R.COVER_FILTER)
        assert (want[1] >= 0).all() and same(got, want)
        assert same(two.search(qn, 10, filter=R.COVER_FILTER), want)  # None: R = 128
        gone = R.covered_deletes()
        assert two.delete(gone) == 500 and bf.delete(gone) == 500
        got, want = two.search(qn, 10, refine=128), bf.search(qn, 10)
        assert (want[1] >= 0).all() and not np.isin(want[1], gone).any() and same(got, want)
        got, want = two.search(qn, 100, refine=100), bf.search(qn, 100)  # k = R = every live row
        assert same(got, want)


@pytest.mark.parametrize("place", PLACES)
def test_rescoring_recovers_what_fp8_loses(tmp_path, place):
    v, q = R.clustered_data()
    p4, p3, p1 = R.write_pair(tmp_path, v)
    with S.Index(p4, rescore_rows=place) as two, S.Index(p3) as fp8, S.Index(p1) as bf:
        refined, plain = two.search(q, 10, refine=128), two.search(q, 10, refine=0)
        assert same(refined, bf.search(q, 10))
        assert same(plain, fp8.search(q, 10))
        assert not np.array_equal(refined[1], plain[1])
        # the host placement leaves the index at an fp8 index's device bytes, plus the intermediate buffers
        extra = two.describe()["device_bytes"] - fp8.describe()["device_bytes"]
        rows = two.describe()["capacity"] * R.IX_D * 2
        per_ctx = 2 * 16 * 128 * 4
        assert extra == 2 * per_ctx + (rows if place == "device" else 0)


@pytest.mark.parametrize("place", PLACES)
def test_a_live_two_stage_index_follows_refindex(tmp_path, place):
    rows, q = R.live_data()
    p4, pr = str(tmp_path / "g.hzidx"), str(tmp_path / "r.hzidx")
    for p in (p4, pr):
        S.write_index(p, rows[:R.LIVE_N0], "ip", tags=R.live_tags(R.LIVE_N0), dtype="fp8", rescore=True)
    saved_g, saved_r = tmp_path / "g_saved.hzidx", tmp_path / "r_saved.hzidx"
    with S.Index(p4, contexts=1, reserve=256, rescore_rows=place) as ix:  # one context: its programs are the index's
        assert ix.capacity() == 256
        got = R.drive(ix, rows, q, saved_g)
        assert ix.capacity() == 1024
    want = R.drive(S.RefIndex(pr, reserve=256), rows, q, saved_r)
    for step, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g[0], w[0]), step
    # the programs: first use captures one; an add inside the tile keeps it; growth and the
    # tile-boundary add drop it; delete keeps it; each new (k, filtered) shape adds one; set_tags keeps them
    assert [(g[1], g[2]) for g in got] == [(0, 1), (1, 1), (0, 1), (0, 1), (0, 1), (1, 1), (1, 2), (2, 2)]
    assert S.file_info(str(saved_g))["version"] == 4
    assert np.array_equal(S.read_rescore_rows(str(saved_g)), S.read_rescore_rows(str(saved_r)))
    assert np.array_equal(S.read_rescore_rows(str(saved_g)), S.to_bf16(rows))
    for read in (S.read_rows, S.read_scales, S.read_tags, S.read_live):
        assert np.array_equal(read(str(saved_g)), read(str(saved_r))), read.__name__
    with S.Index(str(saved_g), rescore_rows=place) as again:  # reopened: the same answers
        assert np.array_equal(again.search(q, 7, filter=(0xFFFFFFFF, 3), refine=128)[1], want[-1][0])
        assert np.array_equal(again.search(q, 10, refine=128)[1], S.RefIndex(str(saved_r)).search(q, 10, refine=128)[1])


def test_refusals(tmp_path):
    v, q = R.clustered_data()
    p4, p3, p1 = R.write_pair(tmp_path, v)
    with S.Index(p4) as two, S.Index(p3) as fp8, S.Index(p1) as bf:
        for ix in (fp8, bf):
            with pytest.raises(ValueError, match=f"{ix.dtype} index of version {ix.version}"):
                ix.search(q, 10, refine=64)
            assert same(ix.search(q, 10, refine=None), ix.search(q, 10)) and same(ix.search(q, 10, refine=0), ix.search(q, 10))
        for bad in (9, 129):
            with pytest.raises(ValueError, match="fp8_e4m3 index of version 4"):
                two.search(q, 10, refine=bad)
        lib = two._lib
        sc, ids = np.full((3, 10), 7.0, np.float32), np.full((3, 10), -7, np.int32)

        def native(ix, refine):
            return lib.hz_index_search2(ix._h, 0, q.ctypes.data, None, 3, 10, refine, sc.ctypes.data, ids.ctypes.data)

        assert native(fp8, 64) == -27 and b"rescore rows" in lib.hz_index_last_error() and b"fp8_e4m3" in lib.hz_index_last_error()
        assert native(bf, 64) == -27 and b"bf16" in lib.hz_index_last_error()
        assert native(two, 9) == -28 and native(two, 129) == -28 and b"refine" in lib.hz_index_last_error()
        assert (sc == 7.0).all() and (ids == -7).all()
        assert native(two, 10) == 0 and same((sc, ids), two.search(q, 10, refine=10))
        # the fp8-only add on a two-stage index: refused, and nothing is added
        codes, scales = S.prepare_rows_fp8(v[:2], "cosine")
        first = C.c_longlong(-1)
        rc = lib.hz_index_add_q(two._h, codes.ctypes.data, scales.ctypes.data, 2, None, C.byref(first))
        assert rc == -29 and b"hz_index_add_qr" in lib.hz_index_last_error()
        rr = S.prepare_rows(v[:2], "cosine")
        rc = lib.hz_index_add_qr(fp8._h, codes.ctypes.data, scales.ctypes.data, rr.ctypes.data, 2, None, C.byref(first))
        assert rc == -29 and b"hz_index_add_q" in lib.hz_index_last_error()
        assert two.describe()["live"] == R.IX_N and fp8.describe()["live"] == R.IX_N and first.value == -1
