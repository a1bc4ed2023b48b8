"""``Index.search_batch_fp8`` (hz_index_search_batch_q) against ``RefIndex.search_batch_fp8`` and ``Index.search`` on
version 3 and 4 files, through a delete between two calls, split calls, and beside the entry points that keep refusing."""
import numpy as np
import pytest

from hipzap import search as S

from search_pq_cases import u32

pytestmark = pytest.mark.gpu
N, D, K = 600, 64, 10


@pytest.mark.parametrize("rescore,placement", [(False, "device"), (True, "device"), (True, "host")])
def test_the_index_equals_the_oracle_and_search_through_a_delete(tmp_path, rescore, placement):
    rng = np.random.default_rng(7)
    v = rng.standard_normal((N, D)).astype(np.float32)
    q = S.normalize_rows(rng.standard_normal((70, D)).astype(np.float32))
    path = str(tmp_path / "a.hzidx")
    S.write_index(path, v, "cosine", dtype="fp8", rescore=rescore)
    R = S.batch_candidates(K)
    with S.Index(path, contexts=1, rescore_rows=placement) as ix, S.RefIndex(path) as ref:
        assert ix.describe()["batch_fp8"] is True
        for step in ("open", "delete"):
            if step == "delete":  # device data only (4v's rule): the captured program stays and honours it
                programs = ix.describe()["programs"]
                ix.delete([5, 299, 599]), ref.delete([5, 299, 599])
                assert ix.describe()["programs"] == programs > 0
            got = ix.search_batch_fp8(q, K, fallback=False)
            want = ref.search_batch_fp8(q, K, fallback=False)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), step
            assert np.allclose(got[0], want[0], rtol=1e-5, atol=1e-6)  # the oracle's scores are fp64 sums
            s, i = ix.search(q, K, refine=R) if rescore else ix.search(q, K)
            c = got[2]
            assert c.all() != rescore and np.array_equal(got[1][c], i[c]) and np.array_equal(u32(got[0][c]), u32(s[c]))
            full = ix.search_batch_fp8(q, K, fallback=True)
            assert full[2].all() and np.array_equal(full[1], i) and np.array_equal(u32(full[0]), u32(s))
        assert not np.isin(got[1], [5, 299, 599]).any()
        # Q above hz_index_neighbors_max is split; the other entry points keep refusing on the same handle
        assert ix._lib.hz_index_neighbors_max(ix._h, 32) == 32
        split = ix.search_batch_fp8(q, K, fallback=False)
        assert np.array_equal(u32(split[0]), u32(got[0])) and np.array_equal(split[1], got[1])
        out_s, out_i, last = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int32), np.zeros(2, np.float32)
        args = (ix._h, 0, q.ctypes.data, 2, 3, 3, out_s.ctypes.data, out_i.ctypes.data, last.ctypes.data)
        assert ix._lib.hz_index_search_batch(*args) == -44 and ix._lib.hz_index_search_batch_pq(*args) == -46
        assert ix._lib.hz_index_search_batch_q(*args[:5], 2, *args[6:]) == -188  # R below k
        with pytest.raises(ValueError, match=f"an fp8_e4m3 index of version {4 if rescore else 3}"):
            ix.search_batch(q, K)
        with pytest.raises(ValueError, match="candidates"):
            ix.search_batch_fp8(q, K, candidates=K - 1)


@pytest.mark.parametrize("kw,d,code,what", [(dict(), 128, -186, "a bf16 index of version 1"), (dict(dtype="fp8"), 48, -187, "dim % 32")])
def test_the_native_call_refuses_by_name(tmp_path, kw, d, code, what):
    v = np.random.default_rng(1).standard_normal((300, d)).astype(np.float32)
    S.write_index(str(tmp_path / "a.hzidx"), v, "ip", **kw)
    with S.Index(str(tmp_path / "a.hzidx"), contexts=1) as ix:
        out_s, out_i, last = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int32), np.zeros(2, np.float32)
        assert ix._lib.hz_index_search_batch_q(ix._h, 0, v.ctypes.data, 2, 3, 3, out_s.ctypes.data, out_i.ctypes.data,
                                               last.ctypes.data) == code
        assert what in ix._lib.hz_index_last_error().decode()
        with pytest.raises(ValueError, match=what):
            ix.search_batch_fp8(v[:2], 3)
