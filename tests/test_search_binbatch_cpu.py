"""Bulk search over binary indexes without a GPU: the host oracle, the by-name refusals, kind 59's
registration and its launcher's refusal codes."""
import ctypes as C

import numpy as np
import pytest

from hipzap import search as S


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("binbatch_cpu")
    v = np.random.default_rng(3).standard_normal((300, 128)).astype(np.float32)
    S.write_index(str(root / "v8.hzidx"), v, "ip", dtype="bin")
    S.write_index(str(root / "v9.hzidx"), v, "ip", dtype="bin", rescore=True)
    S.write_index(str(root / "v1.hzidx"), v, "ip")
    S.write_index(str(root / "v3.hzidx"), v, "ip", dtype="fp8")
    return root


@pytest.mark.parametrize("name,refine", [("v8", None), ("v8", 0), ("v9", None), ("v9", 40), ("v9", 0)])
def test_refindex_search_batch_bin_equals_search(files, name, refine):
    q = np.random.default_rng(4).standard_normal((19, 128)).astype(np.float32)
    with S.RefIndex(str(files / f"{name}.hzidx")) as ix:
        ix.delete([1, 7, 299])
        got, want = ix.search_batch_bin(q, 10, refine=refine), ix.search(q, 10, refine=refine)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        assert not np.isin(got[1], [1, 7, 299]).any()


@pytest.mark.parametrize("name,what", [("v1", "a bf16 index of version 1"), ("v3", "an fp8_e4m3 index of version 3")])
def test_any_other_index_is_refused_by_name(files, name, what):
    q = np.zeros((2, 128), np.float32)
    with S.RefIndex(str(files / f"{name}.hzidx")) as ix:
        with pytest.raises(ValueError, match=f"search_batch_bin needs a bin_sign index .*this one is {what}"):
            ix.search_batch_bin(q, 5)
    with S.RefIndex(str(files / "v8.hzidx")) as ix:
        with pytest.raises(ValueError, match="a bin_sign index of version 8"):
            ix.search_batch(q, 5)  # search_batch keeps refusing a binary index
        with pytest.raises(ValueError, match="refine must be None or 0"):
            ix.search_batch_bin(q, 5, refine=40)


def test_kind_59_is_registered_and_its_launcher_refuses_without_a_device():
    from hipzap import _native as N
    from hipzap.ops import search as OS
    lib = N.lib()
    assert N.HZ_K_SEARCH_BXSCAN == 59 and lib.hz_kernel_name(59) == b"HZ_K_SEARCH_BXSCAN"
    assert lib.hz_kernel_param_size(59) == C.sizeof(OS.BinBatchScanParams) == 96  # 6 pointers, 2 u64, 8 ints
    # corpus, queries, live, cand, out_score, out_id, live_bytes, cand_bytes, N, D, Q, k, ldc, ntile, span, nslab
    ok = OS.BinBatchScanParams(16, 16, 16, 16, 16, 16, 40, 2 * 3 * 10 * 8, 300, 256, 3, 10, 8, 0, 1, 0)
    cases = [(f, 0, -80) for f in ("corpus", "queries", "cand", "out_score", "out_id")]
    cases += [("D", 192, -81), ("D", 0, -82), ("D", 2176, -83), ("ldc", 4, -84), ("ldc", 10, -84), ("N", 0, -85), ("k", 0, -87),
              ("k", 129, -87), ("corpus", 24, -88), ("queries", 20, -88), ("cand", 20, -88), ("live", 18, -88), ("live", 0, -89),
              ("live_bytes", 36, -90), ("span", -1, -257), ("Q", 0, -258), ("Q", OS.SELF_MAX_Q + 1, -258),
              ("cand_bytes", 2 * 3 * 10 * 8 - 8, -259)]
    for field, value, code in cases:
        bad = OS.BinBatchScanParams.from_buffer_copy(ok)
        setattr(bad, field, value)
        assert lib.hz_launch_kernel(59, C.byref(bad), None) == code, (field, value)
    assert OS.bin_batch_scratch_bytes(300, 3, 10, 1) == 2 * 3 * 10 * 8 and OS.bin_batch_scratch_bytes(300, 3, 10, 5) == 3 * 10 * 8
    assert OS.bin_batch_scratch_bytes(300, 3, 129, 1) == 0 and OS.bin_batch_scratch_bytes(300, 3, 10, -1) == 0
