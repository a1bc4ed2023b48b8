"""Bulk search over pq8 indexes on the host: the bf16 table, ``RefIndex.search_batch_pq``, refusals, the slack."""
import numpy as np
import pytest

from hipzap import search as S

import search_pq_cases as P


@pytest.mark.parametrize("dsub", [8, 16, 24])
def test_the_table_is_the_codebook_in_bf16_by_8_column_chunk(dsub):
    m = 16
    cb = P.make("inexact", 1, m * dsub, m, 1)[1]
    cb8 = S.pq_table_bf16(cb)
    assert cb8.shape == (m * dsub // 8, 256, 8) and cb8.dtype == np.uint16 and cb8.flags.c_contiguous
    bits = S.to_bf16(cb)
    for g in range(cb8.shape[0]):
        sub = 8 * g // dsub
        for c in (0, 1, 200, 255):
            assert np.array_equal(cb8[g, c], bits[sub, c, 8 * g - sub * dsub:8 * g - sub * dsub + 8]), (g, c)
    codes = P.make("inexact", 40, m * dsub, m, 1)[0]
    assert np.array_equal(S.pq_decode_bf16(codes, cb8), S.to_bf16(S.pq_decode(codes, cb)))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    A, B, cb, q = P.index_data()
    root = tmp_path_factory.mktemp("pqbatch")
    paths = {v: str(root / f"v{v}.hzidx") for v in (10, 11)}
    for v in paths:
        S.write_index(paths[v], A, "ip", dtype="pq", pq_m=P.IX_M, pq_codebook=cb, rescore=v == 11)
    return paths, cb, np.concatenate([q, A[:20] * np.float32(0.5)])


def test_version_10_certain_means_equal_to_search_in_ids_and_score_bits(files):
    paths, cb, q = files
    with S.RefIndex(paths[10]) as ref:
        ref.delete([3])
        s, i, certain = ref.search_batch_pq(q, P.IX_K, fallback=False)
        ws, wi = ref.search(q, P.IX_K)
        assert certain.any() and np.array_equal(i[certain], wi[certain]) and np.array_equal(P.u32(s[certain]), P.u32(ws[certain]))
        s2, i2, c2 = ref.search_batch_pq(q, P.IX_K)  # fallback=None: True here
        assert c2.all() and np.array_equal(i2, wi) and np.array_equal(P.u32(s2), P.u32(ws))
        assert not (i == 3).any()


def test_version_11_returns_the_exact_rescoring_of_the_decoded_top_r(files):
    paths, cb, q = files
    R = 20
    with S.RefIndex(paths[11]) as ref:
        s, i, certain = ref.search_batch_pq(q, P.IX_K, candidates=R)  # fallback=None: False here
        assert not certain.any()  # more than R rows pass and no bound relates the two orders
        rows = S.bf16_to_f32(S.pq_decode_bf16(S.read_rows(paths[11]), S.pq_table_bf16(cb)))
        h, m, l = (t.astype(np.float64) for t in S.split3(q))
        top = S.search_ref(rows, h + m + l, R)[1]
        rr = S.bf16_to_f32(S.read_rescore_rows(paths[11]))
        for a in range(q.shape[0]):
            ws, wi = S.rescore_ref(rr, q[a], top[a], P.IX_K)
            assert set(i[a]) <= set(top[a]) and np.array_equal(i[a], wi) and np.array_equal(s[a], ws.astype(np.float32))
        s2, i2, c2 = ref.search_batch_pq(q, P.IX_K, candidates=R, fallback=True)
        want = ref.search(q, P.IX_K, refine=R)
        assert c2.all() and np.array_equal(i2, want[1]) and np.array_equal(P.u32(s2), P.u32(want[0]))


def test_other_indexes_and_dsub_4_are_refused_by_name(tmp_path, files):
    paths, cb, q = files
    A = P.index_data()[0]
    bf, p4 = str(tmp_path / "bf.hzidx"), str(tmp_path / "p4.hzidx")
    S.write_index(bf, A, "ip")
    S.write_index(p4, A[:, :64], "ip", dtype="pq", pq_m=16, pq_iters=1)
    with S.RefIndex(bf) as ref, pytest.raises(ValueError, match="built for pq8 indexes.*a bf16 index of version"):
        ref.search_batch_pq(q, 3)
    with S.RefIndex(p4) as ref, pytest.raises(ValueError, match="dsub % 8 == 0.*got dsub = 4"):
        ref.search_batch_pq(q[:, :64], 3)
    with pytest.raises(ValueError, match="dsub % 8 == 0"):
        S.pq_table_bf16(np.zeros((16, 256, 4), np.float32))
    with S.RefIndex(paths[10]) as ref, pytest.raises(ValueError, match="candidates"):
        ref.search_batch_pq(q, 10, candidates=5)


def test_the_slack_grows_with_each_of_its_terms():
    def slack(m, scale=1.0):
        qm = np.full((1, 8 * m), np.sqrt(128 / (8 * m)))
        return float(S.pq_batch_slack(qm, np.full((m, 256, 8), scale / np.sqrt(8 * m)))[0])
    base = slack(16)  # ||q|| = sqrt(128) and xmax = 1 + 2^-8 in every call below
    assert base > 2.0 ** -8 * np.sqrt(128)                       # the bf16 rounding of the codebook alone
    assert slack(32) > base and slack(96) > slack(32)            # beta(3D) and gamma(dsub + M) grow with D and M
    assert slack(16, 2.0) == pytest.approx(2 * base, rel=1e-12)  # linear in xmax, as in ||q||
    two = S.pq_batch_slack(np.array([[1.0] * 128, [2.0] * 128]), np.full((16, 256, 8), 0.1, np.float32))
    assert two[1] == pytest.approx(2 * two[0], rel=1e-12)
