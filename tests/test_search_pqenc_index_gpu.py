"""The GPU backend of product-quantisation training and encoding (``hz_pq_encode`` over HZ_K_SEARCH_PQASSIGN) against
the ``"f32"`` backend, its arithmetic in numpy: ``pq_encode``, ``pq_train``, ``write_index`` / ``convert_index``,
``Index.add`` and the CLI give the same bytes either way."""
import numpy as np
import pytest

from hipzap import search as S
from hipzap.ops import search as OS

import search_pq_cases as PQ
import search_pqenc_cases as P
from search_pqenc_cases import T, u32

pytestmark = pytest.mark.gpu


def test_pq_encode_gpu_equals_f32_wherever_the_chunk_edges_fall():
    N = P.NMAX
    for kind, D, M in (("neartie", 768, 48), ("inexact", 128, 16), ("integer", 48, 16)):
        rows, cb = P.make(kind, N, D, M)
        want = P.ref(kind, N, D, M)
        for chunk in (0, 1, T, T + 1, N):
            assert np.array_equal(S.pq_encode(rows, cb, backend="gpu", chunk_rows=chunk), want[0]), (kind, D, M, chunk)
        codes, dist = OS.pq_encode_rows(S.to_bf16(rows), cb, chunk_rows=T + 1, want_dist=True)  # and the distances
        assert np.array_equal(codes, want[0]) and np.array_equal(u32(dist), u32(want[1]))
    assert S.pq_encode(rows[:0], cb, backend="gpu").shape == (0, 16)
    with pytest.raises(ValueError, match="chunk_rows"):
        S.pq_encode(rows, cb, backend="gpu", chunk_rows=-1)


@pytest.mark.parametrize("D,M", [(128, 16), (768, 48)])
def test_pq_train_gpu_equals_f32_bit_for_bit(D, M):
    g = np.random.default_rng(D + M).standard_normal((2000, D)).astype(np.float32)
    x = S.bf16_to_f32(S.to_bf16(g / np.linalg.norm(g, axis=1, keepdims=True)))
    a = S.pq_train(x, M, seed=2, iters=3, backend="gpu")
    assert np.array_equal(u32(a), u32(S.pq_train(x, M, seed=2, iters=3, backend="f32")))
    few = S.pq_train(x, M, seed=2, iters=2, sample=700, backend="gpu")  # a sample: gathered on the host once
    assert np.array_equal(u32(few), u32(S.pq_train(x, M, seed=2, iters=2, sample=700, backend="f32")))
    assert not np.array_equal(few, a)


def searches_like_the_oracle(path, q, k=10):
    """The file opens, and a first-stage search returns rows whose scores are within the contract's bound of their
    exact scores and whose j-th score is within the bound of the exact j-th best."""
    codes, cb = S.read_rows(path), S.read_codebook(path)
    s64, bound = PQ.score_oracle(codes, cb, q)
    with S.Index(path, contexts=1) as ix, S.RefIndex(path) as ref:
        got, want = ix.search(q, k, refine=0), ref.search(q, k, refine=0)
    assert (got[1] >= 0).all() and all(len(set(r.tolist())) == k for r in got[1])
    at = got[1].astype(np.int64)
    assert (np.abs(got[0].astype(np.float64) - np.take_along_axis(s64, at, axis=1)) <= np.take_along_axis(bound, at, axis=1)).all()
    slack = bound.max(axis=1, keepdims=True) + np.abs(want[0]) * 2.0 ** -24
    assert (np.abs(got[0].astype(np.float64) - want[0].astype(np.float64)) <= slack).all()
    clear = np.abs(np.diff(-np.sort(-s64, axis=1)[:, :k + 1], axis=1)).min(axis=1) > 2 * bound.max(axis=1)
    assert np.array_equal(got[1][clear], want[1][clear])  # where no gap is inside the bound the ids are the oracle's


def test_write_index_and_convert_index_on_the_gpu_store_the_f32_bytes(tmp_path):
    A, B = P.index_vectors()
    p = {k: str(tmp_path / f"{k}.hzidx") for k in ("bf", "gpu", "f32", "cgpu", "gpu11", "f3211", "cgpu11")}
    kw = dict(dtype="pq", pq_m=P.IX_M, pq_iters=2, pq_seed=1)
    tags = (np.arange(P.IX_N) % 3).astype(np.uint32)
    S.write_index(p["bf"], A, "cosine", tags=tags)
    hg = S.write_index(p["gpu"], A, "cosine", tags=tags, pq_backend="gpu", **kw)
    hf = S.write_index(p["f32"], A, "cosine", tags=tags, pq_backend="f32", **kw)
    assert hg == hf and hg["dtype"] == "pq8" and open(p["gpu"], "rb").read() == open(p["f32"], "rb").read()
    S.convert_index(p["bf"], p["cgpu"], pq_backend="gpu", **kw)  # from the bf16 file: the same bytes as from the vectors
    assert open(p["cgpu"], "rb").read() == open(p["gpu"], "rb").read()
    S.write_index(p["gpu11"], A, "cosine", tags=tags, rescore=True, pq_backend="gpu", **kw)
    S.write_index(p["f3211"], A, "cosine", tags=tags, rescore=True, pq_backend="f32", **kw)
    S.convert_index(p["bf"], p["cgpu11"], rescore=True, pq_backend="gpu", **kw)
    assert open(p["gpu11"], "rb").read() == open(p["f3211"], "rb").read() == open(p["cgpu11"], "rb").read()
    assert S.file_info(p["gpu"])["version"] == 10 and S.file_info(p["gpu11"])["version"] == 11
    q = np.ascontiguousarray(B[:3])
    searches_like_the_oracle(p["gpu"], q)
    searches_like_the_oracle(p["gpu11"], q)


@pytest.mark.parametrize("rescore", [False, True])
def test_index_add_with_the_gpu_encoder_stores_the_f32_codes(tmp_path, rescore):
    A, B = P.index_vectors()
    path = str(tmp_path / "a.hzidx")
    S.write_index(path, A, "cosine", dtype="pq", pq_m=P.IX_M, pq_iters=1, rescore=rescore)
    cb = S.read_codebook(path)
    want = S.pq_encode(S.bf16_to_f32(S.prepare_rows(B, "cosine")), cb, backend="f32")
    with S.Index(path, contexts=1, reserve=T) as ix, S.RefIndex(path, reserve=T) as ref:
        ids = ix.add(B, encoder="gpu")  # past the tile boundary at 2T and past the capacity
        assert np.array_equal(ids, np.arange(P.IX_N, P.IX_N + P.IX_ADD, dtype=np.int32))
        assert np.array_equal(ref.add(B, encoder="f32"), ids)
        state = ix._state()
        assert np.array_equal(state[0][P.IX_N:], want) and np.array_equal(state[0], ref._state()[0])
        assert np.array_equal(state[0][:P.IX_N], S.read_rows(path))
        q = np.ascontiguousarray(B[[0, 100, P.IX_ADD - 1]])  # each added row is the best match of itself
        if rescore:  # the bf16 second stage scores a row against itself with 1: found, and first
            assert ix.search(q, 5, refine=128)[1][:, 0].tolist() == [P.IX_N, P.IX_N + 100, P.IX_N + P.IX_ADD - 1]
        first = ix.search(q, 5, refine=0)  # the first stage sees the new codes: the keys of a fresh file (below)
        assert (first[1] >= P.IX_N).any()
        with pytest.raises(ValueError, match="encoder must be one of"):
            ix.add(B[:1], encoder="hip")
    both = str(tmp_path / "both.hzidx")
    S.write_index(both, np.concatenate([A, B]), "cosine", dtype="pq", pq_m=P.IX_M, pq_codebook=cb, pq_backend="f32",
                  rescore=rescore)
    assert np.array_equal(S.read_rows(both)[P.IX_N:], want)
    with S.Index(both, contexts=1) as fresh:
        again = fresh.search(q, 5, refine=0)
    assert np.array_equal(u32(first[0]), u32(again[0])) and np.array_equal(first[1], again[1])
    bf = str(tmp_path / "bf.hzidx")
    S.write_index(bf, A, "cosine")
    with S.Index(bf, contexts=1) as plain:
        with pytest.raises(ValueError, match="goes with a pq8 index"):
            plain.add(B, encoder="gpu")
        assert plain.count == P.IX_N


def test_cli_pq_backend_gpu_writes_the_f32_file(tmp_path):
    from hipzap.__main__ import main
    A, _ = P.index_vectors()
    vn, out, want = str(tmp_path / "v.npy"), str(tmp_path / "cli.hzidx"), str(tmp_path / "want.hzidx")
    np.save(vn, A)
    main(["index", "--vectors", vn, "--dtype", "pq", "--pq-m", "16", "--pq-iters", "2", "--pq-backend", "gpu", "--out", out])
    S.write_index(want, A, "cosine", dtype="pq", pq_m=16, pq_iters=2, pq_backend="f32")
    assert open(out, "rb").read() == open(want, "rb").read()
    conv = str(tmp_path / "conv.hzidx")
    bf = str(tmp_path / "bf.hzidx")
    S.write_index(bf, A, "cosine")
    main(["index", "--from-index", bf, "--dtype", "pq", "--pq-m", "16", "--pq-iters", "2", "--pq-backend", "gpu", "--out", conv])
    assert open(conv, "rb").read() == open(want, "rb").read()
