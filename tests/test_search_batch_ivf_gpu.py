"""Bulk search over IVF indexes on the GPU (csrc/search.hip HZ_K_SEARCH_LXSCAN / HZ_K_SEARCH_RESCOREP, csrc/index.cpp,
DESIGN.md 4ab) against ``Index.search`` bit for bit, the host ``RefIndex`` and the fp64 oracle, on the inputs of
search_batch_ivf_cases.py; tests/test_search_batch_ivf_cpu.py asserts what those inputs are on the host."""
import ctypes as C

import numpy as np
import pytest
import torch

from hipzap import _native as N
from hipzap import search as S
from hipzap.ops import search as OS

import search_batch_ivf_cases as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KC = ((1, 1), (10, None), (10, 10))


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("batch_ivf")
    out = {d: (str(root / f"d{d}.hzidx"), V.write(str(root / f"d{d}.hzidx"), d)) for d in V.DIMS}
    out["ip"] = (str(root / "ip.hzidx"), V.write(str(root / "ip.hzidx"), 96, "ip"))
    return out


def one_by_one(ix, q, k, nprobe):
    """``search`` query by query: what the parent commit answers."""
    two = [ix.search(q[a:a + 1], k, nprobe=nprobe) for a in range(q.shape[0])]
    return np.concatenate([t[0] for t in two]), np.concatenate([t[1] for t in two])


@pytest.mark.parametrize("d", V.DIMS)
@pytest.mark.parametrize("nprobe", (1, 2, "all"))
def test_equals_search_bit_for_bit_and_the_oracle(files, d, nprobe):
    path, q = files[d]
    with S.Index(path) as ix, S.RefIndex(path) as ref:
        lists = ref._nprobe(nprobe)
        for k, cand in KC:
            ws, wi = one_by_one(ix, q, k, nprobe)
            s, i, certain = ix.search_batch_ivf(q, k, nprobe=nprobe, candidates=cand)
            assert certain.all() and np.array_equal(i, wi) and np.array_equal(u32(s), u32(ws)), (k, cand)
            s0, i0, c0 = ix.search_batch_ivf(q, k, nprobe=nprobe, candidates=cand, fallback=False)
            assert np.array_equal(i0[c0], wi[c0]) and np.array_equal(u32(s0[c0]), u32(ws[c0])), (k, cand)
            few, enough = V.clauses(ref, q, k, lists, cand)
            assert c0[few].all() and (nprobe != 1 or few[V.EMPTY])  # s_R == -inf certifies: fewer than R live rows probed
            assert cand is not None or (c0 & enough).any()          # ... and the slack clause somebody with R or more
            rs, ri, rc = ref.search_batch_ivf(q, k, nprobe=nprobe, candidates=cand, fallback=False)
            want, sure = V.forced(ref, q, k, lists)
            assert np.array_equal(i0[c0 & sure], want[c0 & sure]) and np.array_equal(i0[c0 & rc & sure], ri[c0 & rc & sure])


@pytest.mark.parametrize("nprobe", (1, 2, "all"))
def test_deleted_rows_never_return(files, nprobe):
    path, q = files[96]
    with S.Index(path) as ix:
        ivf = S.read_ivf(path)
        group = ivf["rowid"][:16]                                  # the first 16 stored rows of list 0: a whole row group
        whole = np.flatnonzero(ivf["list_of"] == 4)                # every row of list 4
        dead = np.unique(np.concatenate([group, whole, np.arange(0, V.N, 37)]))
        assert (group >= 0).all() and ix.delete(dead) == dead.size
        for k, cand in KC:
            s, i, certain = ix.search_batch_ivf(q, k, nprobe=nprobe, candidates=cand)
            ws, wi = one_by_one(ix, q, k, nprobe)
            assert certain.all() and not np.isin(i, dead).any()
            assert np.array_equal(i, wi) and np.array_equal(u32(s), u32(ws))


def test_ties_across_lists_break_on_the_external_id(files):
    path, q = files["ip"]
    zero = np.zeros((3, 96), np.float32)
    with S.Index(path) as ix:
        ivf = S.read_ivf(path)
        gone = np.sort(np.flatnonzero(ivf["list_of"] <= 1))[[0, 3]]  # two of the lowest ids of the probed lists
        ix.delete(gone)
        assert np.array_equal(ix.probes(zero, 2), [[0, 1]] * 3)      # every centroid scores +0: the lower lists
        want = np.setdiff1d(np.flatnonzero(ivf["list_of"] <= 1), gone)[:10]
        s, i, certain = ix.search_batch_ivf(zero, 10, nprobe=2, fallback=False)
        assert (u32(s) == 0).all() and (i == want[None, :]).all()
        assert np.array_equal(i, ix.search(zero, 10, nprobe=2)[1])


def test_probes_batch_equals_probes(files):
    path, q = files["ip"]
    with S.Index(path) as ix, S.RefIndex(path) as ref:
        for n, cand in ((1, None), (2, None), (2, 2), (5, 5)):
            want = ix.probes(q, n)
            lists, certain = ix.probes_batch(q, n, candidates=cand, fallback=False)
            assert lists.dtype == np.int32 and np.array_equal(lists[certain], want[certain])
            assert cand is not None or certain.all()                 # fewer than Rc lists: s_Rc is -inf
            assert np.array_equal(certain, ref.probes_batch(q, n, candidates=cand, fallback=False)[1]) or cand is not None
            lists, certain = ix.probes_batch(q, n, candidates=cand)
            assert certain.all() and np.array_equal(lists, want)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to(DEV)


def test_the_list_scan_has_the_batch_scans_bits_and_refuses_a_short_work_list(files):
    """A hand-made work list over the stored rows: tile x goes to slot x for the queries 0..63 and to slot x + 1 for the
    queries 64..69, so every (query, tile) list must equal kind 44's for that tile, the id read through rowid."""
    path, q = files[96]
    ivf, bits = S.read_ivf(path), S.read_rows(path)
    rowid, (n, d), k = ivf["rowid"], bits.shape, 12
    ntile, P, Q = n // 256, n // 256 + 1, V.Q
    words = S.pack_live(rowid >= 0)
    corpus, qd, lv, rid = dev(bits, np.int16), dev(q, np.float32), dev(words, np.int32), dev(rowid, np.int32)
    items = np.array([[x, x, first, nq] for x in ivf["list_tiles"] for first, nq in ((0, 64), (64, 6))], np.int32)
    entries = np.array([[a, 0] for a in range(64)] + [[a, 1] for a in range(64, Q)], np.int32)
    it, en = dev(items, np.int32), dev(entries, np.int32)
    st = torch.cuda.current_stream().cuda_stream
    lib = N.lib()
    xc = torch.full((ntile * Q * k,), -1, dtype=torch.int64, device=DEV)
    xp = OS.BatchScanParams(corpus.data_ptr(), qd.data_ptr(), lv.data_ptr(), xc.data_ptr(), 0, 0, words.size * 4, xc.numel() * 8,
                            n, d, Q, k, d, 0)
    assert lib.hz_launch_kernel(N.HZ_K_SEARCH_XSCAN, C.byref(xp), st) == 0
    lc = torch.full((P * Q * k + k,), -1, dtype=torch.int64, device=DEV)
    lp = OS.ListBatchScanParams(corpus.data_ptr(), qd.data_ptr(), lv.data_ptr(), lc.data_ptr(), 0, 0, words.size * 4, P * Q * k * 8,
                                n, d, Q, k, d, 0, (C.c_int * 2)(), rid.data_ptr(), it.data_ptr(), en.data_ptr(), items.nbytes,
                                entries.nbytes, items.shape[0], entries.shape[0], P, 0)
    for field, short, code in (("items_bytes", items.nbytes - 1, -202), ("entries_bytes", entries.nbytes - 1, -203)):
        bad = OS.ListBatchScanParams.from_buffer_copy(lp)
        setattr(bad, field, short)
        assert lib.hz_launch_kernel(N.HZ_K_SEARCH_LXSCAN, C.byref(bad), st) == code
    torch.cuda.synchronize()
    assert (lc.cpu().numpy() == -1).all()  # refused: nothing ran
    assert lib.hz_launch_kernel(N.HZ_K_SEARCH_LXSCAN, C.byref(lp), st) == 0
    torch.cuda.synchronize()
    x = xc.cpu().numpy().view(np.uint64).reshape(ntile, Q, k)
    got = lc.cpu().numpy().view(np.uint64)
    assert (got[P * Q * k:] == np.uint64(2 ** 64 - 1)).all()
    got = got[:P * Q * k].reshape(P, Q, k)
    mine = np.concatenate([got[:ntile, :64], got[1:, 64:]], axis=1)  # [tile][query]: the slot each block owns
    assert (got[ntile, :64] == 0).all() and (got[0, 64:] == 0).all()  # the slots nobody owns hold the cleared keys
    real = x != 0
    assert np.array_equal(mine != 0, real) and np.array_equal(mine >> np.uint64(32), x >> np.uint64(32))
    pos = (~x[real]).astype(np.uint32).astype(np.int64)
    assert np.array_equal((~mine[real]).astype(np.uint32).astype(np.int64), rowid[pos])


def test_refusals_from_python(files, tmp_path):
    path, q = files[32]
    flat, fp8, odd = (str(tmp_path / n) for n in ("flat.hzidx", "fp8.hzidx", "odd.hzidx"))
    v, _, init, _ = V.data(32, "cosine")
    S.write_index(flat, v, "cosine")
    S.convert_index(path, fp8, "fp8")
    S.write_index(odd, v[:, :24], "cosine", ivf=V.NLIST, ivf_iters=0, ivf_init=init[:, :24])
    with S.Index(flat) as ix, pytest.raises(ValueError, match="built for IVF indexes over bf16 rows.*without lists of version 1"):
        ix.search_batch_ivf(q, 10)
    with S.Index(fp8) as ix, pytest.raises(ValueError, match="an fp8 IVF index of version 6"):
        ix.search_batch_ivf(q, 10)
    with S.Index(odd) as ix, pytest.raises(ValueError, match="dim % 32 == 0.*dim = 24"):
        ix.probes_batch(q[:, :24], 2)
    with S.Index(path) as ix:
        with pytest.raises(ValueError, match="nprobe must be"):
            ix.search_batch_ivf(q, 10, nprobe=0)
        with pytest.raises(ValueError, match="nprobe must be"):
            ix.probes_batch(q, V.NLIST + 1)
        out = np.empty((2, 1), np.float32)  # the native call names a probe id outside the lists
        bad = np.array([[0], [V.NLIST]], np.int32)
        q2 = np.ascontiguousarray(q[:2], np.float32)
        rc = ix._lib.hz_index_search_batch_ivf(ix._h, 0, q2.ctypes.data, 2, bad.ctypes.data, 1, 1, 1, out.ctypes.data,
                                               out.ctypes.data, out.ctypes.data)
        assert rc == -217 and b"probe 5 of query 1 is outside [0, 5)" in ix._lib.hz_index_last_error()
