"""The bulk binary scan (csrc/search.hip, HZ_K_SEARCH_BXSCAN) with HZ_K_SEARCH_MERGEN through hz_launch_kernel against
``hipzap.search.bin_search_ref``, and ``Index.search_batch_bin`` against ``Index.search``.

Scores are integers, so every comparison is exact in ids and score bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from hipzap import _native as N
from hipzap import search as S
from hipzap.ops import search as OS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x5A5A5A5A5A5A5A5A
T, QG, NROWS = 256, 32, 1000  # four tiles, the last one partial


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def corpus(kind: str, D: int, Q: int):
    """-> (words uint32 [NROWS, W], queries fp32 [Q, D], live bool [NROWS])."""
    rng = np.random.default_rng(sum(map(ord, kind)) + D + Q)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    live = np.ones(NROWS, bool)
    if kind == "patterns":  # eight distinct rows: whole tiles and slabs tie, ids alone decide
        words = S.binarize(rng.standard_normal((8, D)).astype(np.float32))[rng.integers(0, 8, NROWS)]
    elif kind == "ascending":  # every tile is nearer to query 0 than the one before: each stages all its rows
        flip = (3 - np.arange(NROWS) // T) * (D // 4)  # the columns a row of that tile flips: 3, 2, 1, 0 quarters
        words = S.binarize(np.where(np.arange(D)[None, :] < flip[:, None], -q[0], q[0]))
    else:
        words = S.binarize(rng.standard_normal((NROWS, D)).astype(np.float32))
    if kind in ("sparse", "few"):  # tile 1 dead; tile 2 (a slab of its own at span 1) holds 5 live rows; "few": 7 in all
        live[T:2 * T] = False
        live[2 * T + 5:3 * T] = False
        if kind == "few":
            live[:] = False
            live[[3, 40, 2 * T + 1, 2 * T + 4, 3 * T, 3 * T + 7, NROWS - 1]] = True
        words[~live] = S.binarize(q[:1])[0]  # a dead row that equals query 0: scoring it would win
    return words, q, live


def launch(words, q, live, R, span, replays=2):
    """Kinds 59 and 40 through hz_launch_kernel -> ((rc59, rc40), [(scores, ids) per replay], guards intact)."""
    n, w = words.shape
    Q = q.shape[0]
    dw = torch.from_numpy(words.view(np.int32)).to(DEV)  # as corpus() built them: the dead rows hold query 0's bits
    dq = torch.from_numpy(q).to(DEV)
    lw = S.pack_live(live)
    dl = torch.from_numpy(lw.view(np.int32)).to(DEV)
    nbytes = OS.bin_batch_scratch_bytes(n, Q, R, span)
    buf = torch.full((nbytes // 8 + 4,), GUARD, dtype=torch.int64, device=DEV)  # two guard words on each side
    out = torch.full((2, Q * R + 2), -7, dtype=torch.int32, device=DEV)         # and two after each output
    sc, ids = out[0].view(torch.float32), out[1]
    p = OS.BinBatchScanParams(dw.data_ptr(), dq.data_ptr(), dl.data_ptr(), buf[2:].data_ptr(), sc.data_ptr(), ids.data_ptr(),
                              lw.size * 4, nbytes, n, 32 * w, Q, R, w, 0, span, 0)
    ntile = -(-n // T)
    mp = p.merge_params(-(-ntile // min(span or OS.bin_batch_span(n, Q, R), ntile)))
    st, lib, outs = torch.cuda.current_stream().cuda_stream, N.lib(), []
    for _ in range(replays):
        rc = (lib.hz_launch_kernel(N.HZ_K_SEARCH_BXSCAN, C.byref(p), st), lib.hz_launch_kernel(N.HZ_K_SEARCH_MERGEN, C.byref(mp), st))
        torch.cuda.synchronize()
        o = out.cpu().numpy()
        outs.append((o[0, :Q * R].view(np.float32).reshape(Q, R).copy(), o[1, :Q * R].reshape(Q, R).copy()))
    g = buf.cpu().numpy()
    intact = bool((g[:2] == GUARD).all() and (g[-2:] == GUARD).all() and (o[:, -2:] == -7).all())
    return rc, outs, intact


# D, span, Q, R, corpus: every D bucket, span (1: a slab per tile; 3: a slab of three tiles and one of one; 0: the launcher
# fills it in -- with four tiles it picks 1, so its arithmetic over a large grid and its switch at k = 79 are seen by
# scripts/bench_search_binbatch.py alone: they need a device and a large N), Q around a query group and R at its ends,
# drawn over the four corpora
CASES = [(128, 1, 1, 1, "random"), (128, 3, QG + 1, 128, "random"), (128, 0, QG, 10, "patterns"),
         (768, 3, QG + 1, 10, "patterns"), (768, 1, 1, 128, "ascending"), (768, 0, QG, 10, "ascending"),
         (2048, 3, QG + 1, 128, "ascending"), (768, 1, QG + 1, 10, "sparse"), (2048, 0, 1, 128, "sparse"),
         (768, 3, QG, 10, "few"), (128, 1, 1, 128, "few")]


@pytest.mark.parametrize("D,span,Q,R,kind", CASES)
def test_kinds_59_and_40_equal_bin_search_ref_exactly(D, span, Q, R, kind):
    words, q, live = corpus(kind, D, Q)
    rc, outs, intact = launch(words, q, live, R, span)
    assert rc == (0, 0) and intact
    want_s, want_i = S.bin_search_ref(words, S.binarize(q), D, R, live)
    for sc, ids in outs:  # a second launch gives the same bytes
        assert np.array_equal(ids, want_i) and np.array_equal(u32(sc), u32(want_s.astype(np.float32)))
    if kind == "few":
        assert (outs[0][1][:, 7:] == -1).all() and (outs[0][0][:, 7:] == -np.inf).all()  # seven live rows in all


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("binbatch")
    rng = np.random.default_rng(11)
    v = rng.standard_normal((T - 20, 128)).astype(np.float32)
    for name, rescore in (("v8", False), ("v9", True)):
        S.write_index(str(root / f"{name}.hzidx"), v, "ip", dtype="bin", rescore=rescore)
    return root, rng.standard_normal((40, 128)).astype(np.float32), rng.standard_normal((70, 128)).astype(np.float32)


@pytest.mark.parametrize("name,refines", [("v8", (None, 0)), ("v9", (None, 40, 0))])
def test_index_search_batch_bin_equals_search(files, name, refines):
    root, more, q = files
    path = str(root / f"{name}.hzidx")
    with S.Index(path, contexts=1) as x, S.RefIndex(path) as ref:
        def agree():
            for refine in refines:
                for nq in (1, 17, 70):
                    want = x.search(q[:nq], 10, refine=refine)
                    for _ in range(2):  # the eager run, then the replay
                        got = x.search_batch_bin(q[:nq], 10, refine=refine)
                        assert np.array_equal(got[1], want[1]) and np.array_equal(u32(got[0]), u32(want[0])), (refine, nq)
                    if refine == 0:
                        r = ref.search(q[:nq], 10, refine=0)
                        assert np.array_equal(got[1], r[1]) and np.array_equal(u32(got[0]), u32(r[0]))
        assert N.lib().hz_index_neighbors_max(x._h, 32) == 32  # 70 queries: three calls
        agree()
        x.add(more), ref.add(more)  # across the tile boundary at T: the programs hold N
        agree()
        assert x.delete([3, T - 19, T + 2]) == 3 and ref.delete([3, T - 19, T + 2]) == 3  # device data only
        agree()
