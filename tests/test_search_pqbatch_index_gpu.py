"""``Index.search_batch_pq`` (hz_index_search_batch_pq) against ``RefIndex.search_batch_pq`` on version 10 and 11 files,
through adds across a tile boundary, deletes, split calls, and beside the entry points that keep refusing."""
import numpy as np
import pytest

from hipzap import search as S

import search_pq_cases as P

pytestmark = pytest.mark.gpu
N, D, M, K = 600, 128, 16, 10


@pytest.mark.parametrize("rescore,placement", [(False, "device"), (True, "device"), (True, "host")])
def test_the_index_equals_the_oracle_through_adds_and_deletes(tmp_path, rescore, placement):
    codes, cb, q = P.make("inexact", N + 100, D, M, 70)
    v = S.bf16_to_f32(S.to_bf16(S.pq_decode(codes, cb)))
    path = str(tmp_path / "a.hzidx")
    S.write_index(path, v[:N], "ip", dtype="pq", pq_m=M, pq_codebook=cb, rescore=rescore)
    with S.Index(path, contexts=1, reserve=1024, rescore_rows=placement) as ix, S.RefIndex(path, reserve=1024) as ref:
        d = ix.describe()
        assert d["cb8_bytes"] == 512 * D and d["batch_pq"] is True
        for step in ("open", "add", "delete"):
            if step == "add":  # 600 -> 700 rows: the scan crosses from 3 tiles to 3 tiles + new rows; then past 768
                ix.add(v[N:]), ref.add(v[N:])
                ix.add(v[:100]), ref.add(v[:100])
                assert ix.describe()["programs"] == 0  # N and ntile are held by value: every program was dropped
            if step == "delete":
                ix.delete([5, 299, 650]), ref.delete([5, 299, 650])  # device data only (4v's rule): the programs stay
            got = ix.search_batch_pq(q, K, fallback=False)
            want = ref.search_batch_pq(q, K, fallback=False)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), step
            assert np.allclose(got[0], want[0], rtol=1e-5, atol=1e-5)  # the oracle's scores are fp64 sums
            if rescore:  # every query is uncertain: the fallback is search(refine=R), bit for bit
                full, (s, i) = ix.search_batch_pq(q, K, fallback=True), ix.search(q, K, refine=S.batch_candidates(K))
                assert not got[2].any() and np.array_equal(full[1], i) and np.array_equal(P.u32(full[0]), P.u32(s))
            else:
                s, i = ix.search(q, K)
                c = got[2]
                assert c.any() and np.array_equal(got[1][c], i[c]) and np.array_equal(P.u32(got[0][c]), P.u32(s[c]))
                full = ix.search_batch_pq(q, K)  # fallback=None: True on version 10
                assert full[2].all() and np.array_equal(full[1], i) and np.array_equal(P.u32(full[0]), P.u32(s))
        assert not np.isin(got[1], [5, 299, 650]).any()
        # Q above hz_index_neighbors_max is split; the old entry point keeps refusing on the same handle
        assert ix._lib.hz_index_neighbors_max(ix._h, 32) == 32
        split = ix.search_batch_pq(q, K, fallback=False)
        assert np.array_equal(P.u32(split[0]), P.u32(got[0])) and np.array_equal(split[1], got[1])
        out_s, out_i, last = np.zeros((2, 3), np.float32), np.zeros((2, 3), np.int32), np.zeros(2, np.float32)
        assert ix._lib.hz_index_search_batch(ix._h, 0, q.ctypes.data, 2, 3, 3, out_s.ctypes.data, out_i.ctypes.data,
                                             last.ctypes.data) == -44
        with pytest.raises(ValueError, match="a pq8 index of version 1[01]"):
            ix.search_batch(q, K)
        with pytest.raises(ValueError, match="candidates"):
            ix.search_batch_pq(q, K, candidates=K - 1)

