"""The means step of product-quantisation training on the host: ``pq_means_seq`` (the oracle of HZ_K_SEARCH_PQUPDATE
and the ``means="seq"`` option) against a literal loop over the rows, and what ``pq_train(means=)`` accepts."""
import numpy as np
import pytest

from hipzap import search as S

from search_pqtrain_cases import make_codes, sentinels, u32, wide_rows


def test_pq_means_seq_is_the_strict_row_order_chain_from_minus_zero():
    n, d, m = 300, 48, 16
    dsub = d // m
    x, codes, cb = wide_rows(n, d, m), make_codes("low16", n, m), sentinels(m, dsub)
    codes[:, 2] = np.where(codes[:, 2] == 9, 8, codes[:, 2])  # centroid 9 of sub-space 2 is empty among the used ones
    acc = np.full((m, 256, dsub), -0.0, np.float64)
    half = np.full((2, m, 256, dsub), -0.0, np.float64)  # the same members, summed as two halves of the rows
    cnt = np.zeros((m, 256), np.int64)
    for r in range(n):
        for j in range(m):
            v = x[r, j * dsub:(j + 1) * dsub].astype(np.float64)
            acc[j, codes[r, j]] += v
            half[int(r >= n // 2), j, codes[r, j]] += v
            cnt[j, codes[r, j]] += 1
    want = cb.copy()
    used = cnt > 0
    want[used] = (acc[used] / cnt[used][:, None]).astype(np.float32)
    got, counts = S.pq_means_seq(x, codes, cb)
    assert got.dtype == np.float32 and np.array_equal(u32(got), u32(want))
    assert counts.dtype == np.int32 and np.array_equal(counts, cnt)
    assert not used[2, 9] and not used[:, 16:].any() and np.array_equal(u32(got[~used]), u32(cb[~used]))  # kept
    assert used[1, :16].all() and (u32(got[1, :16]) == 0x80000000).all()  # members of -0.0 only: the sign stays
    assert (u32(((half[0] + half[1])[used] / cnt[used][:, None]).astype(np.float32)) != u32(want[used])).any()


def test_pq_train_means_host_is_the_default_and_seq_agrees_where_the_sums_are_exact():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((600, 32)).astype(np.float32)
    x = S.bf16_to_f32(S.to_bf16(x / np.linalg.norm(x, axis=1, keepdims=True)))
    base = S.pq_train(x, 16, iters=3)
    assert np.array_equal(u32(base), u32(S.pq_train(x, 16, iters=3, means="host")))
    assert np.array_equal(u32(base), u32(S.pq_train(x, 16, iters=3, means="seq")))
    f32 = S.pq_train(x, 16, iters=3, backend="f32")
    assert np.array_equal(u32(f32), u32(S.pq_train(x, 16, iters=3, backend="f32", means="seq")))


@pytest.mark.parametrize("kw,words", [(dict(means="gpu"), "backend"), (dict(means="gpu", backend="cpu"), "backend"),
                                      (dict(means="gpu", backend="f32"), "means"), (dict(means="rows"), "means")])
def test_pq_train_refuses_a_means_it_cannot_serve(kw, words):
    x = np.zeros((300, 32), np.float32)
    with pytest.raises(ValueError, match=words):
        S.pq_train(x, 16, **kw)
    with pytest.raises(ValueError, match=words):
        S.prepare_rows_pq(x + 1.0, "ip", 16, **kw)
    with pytest.raises(ValueError, match=words):
        S.write_index("unused.hzidx", x + 1.0, "ip", dtype="pq", pq_m=16, **{"pq_" + k: v for k, v in kw.items()})
