"""The quantised list-scan kernel (csrc/search.hip, HZ_K_SEARCH_QLSCAN) through its launcher, against the quantised
scan (HZ_K_SEARCH_QSCAN + merge) over the same stored codes and scales.

The reference of a case is ONE quantised scan at k = 128 whose per-query filter passes exactly the rows of that
query's probed lists (a row's tag carries one bit per list): its positions go through ``rowid`` and are ordered on
the host under the order rule over external ids. The list scan must return the first k of that, id for id and score
bit for score bit. The padding rows hold NaN codes and NaN scales: a load of either would show in the keys."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from hipzap import search as S
from hipzap.ops import search as OS

import search_ivf_fp8_cases as V
from search_ivf_fp8_cases import T
from test_search_ivf_gpu import P_EXTRA, dev_i32, host_merge, list_filter, u32, user_filter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = Path(__file__).resolve().parent.parent
FF = np.uint64(0xFFFFFFFFFFFFFFFF)


class Bufs:
    """Device copies of a quantised layout, kept alive for the launches of one test."""

    def __init__(self, lay):
        self.corpus = torch.from_numpy(lay["codes"]).to(DEV)
        self.scales = torch.from_numpy(lay["scales"]).to(DEV)
        self.q = torch.from_numpy(np.ascontiguousarray(lay["q"], np.float32)).to(DEV)
        self.words = S.pack_live(lay["live"])
        self.live = dev_i32(self.words)
        self.tags = dev_i32(lay["tags"])
        self.list_off, self.list_tiles, self.rowid = dev_i32(V.LIST_OFF), dev_i32(V.LIST_TILES), dev_i32(lay["rowid"])
        self.n, self.d = lay["codes"].shape


def qlscan(b, k, probes, P, filt=None, tweak=None, Q=None, merge=True):
    """-> (scan rc, merge rc, scores [Q, k], ids [Q, k], cand uint64 as the scan left it, the guard after it)."""
    Q = b.q.shape[0] if Q is None else Q
    kk, QQ, PP = min(max(k, 1), 128), min(max(Q, 1), 16), max(P, 1)
    n = PP * QQ * kk
    cand = torch.full((n + 64,), -1, dtype=torch.int64, device=DEV)  # 0xFF bytes: a missing zero-fill shows; 64 guards
    sc = torch.full((QQ, kk), 7.0, dtype=torch.float32, device=DEV)
    ids = torch.full((QQ, kk), -7, dtype=torch.int32, device=DEV)
    pr = None if probes is None else dev_i32(probes)
    fl = None if filt is None else dev_i32(np.ascontiguousarray(filt, np.uint32).reshape(-1, 2))
    p = OS.QuantListScanParams(b.corpus.data_ptr(), b.q.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(),
                               b.n, b.d, Q, k, b.d, 0, n * 8, b.live.data_ptr(), b.tags.data_ptr(),
                               0 if fl is None else fl.data_ptr(), b.words.size * 4,
                               0 if pr is None else pr.data_ptr(), b.list_off.data_ptr(), b.list_tiles.data_ptr(),
                               b.rowid.data_ptr(), V.NLIST, 0 if probes is None else probes.shape[1], P, 0,
                               b.scales.data_ptr())
    if tweak:
        tweak(p)
    st = torch.cuda.current_stream().cuda_stream
    rs = OS.N.lib().hz_search_qlscan_launch(OS.C.byref(p), st)
    torch.cuda.synchronize()
    left = cand.cpu().numpy().view(np.uint64).copy()
    rm = None
    if rs == 0 and merge:
        mp = p.merge_params()
        rm = OS.N.lib().hz_search_merge_launch(OS.C.byref(mp), st)
        torch.cuda.synchronize()
    return rs, rm, sc.cpu().numpy(), ids.cpu().numpy(), left[:n], left[n:]


def qscan128(b, filt):
    """Kind 34 + merge over the stored rows at k = 128 -> (scores [Q, 128], positions [Q, 128])."""
    Q = b.q.shape[0]
    nbytes = OS.scratch_bytes(b.n, Q, 128)
    cand = torch.zeros(nbytes // 8, dtype=torch.int64, device=DEV)
    sc = torch.zeros((Q, 128), dtype=torch.float32, device=DEV)
    ids = torch.zeros((Q, 128), dtype=torch.int32, device=DEV)
    fl = dev_i32(np.ascontiguousarray(filt, np.uint32).reshape(Q, 2))
    p = OS.QuantScanParams(b.corpus.data_ptr(), b.q.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(), b.n, b.d, Q,
                           128, b.d, 0, nbytes, b.live.data_ptr(), b.tags.data_ptr(), fl.data_ptr(), b.words.size * 4,
                           b.scales.data_ptr())
    assert OS.launch_quant(p, torch.cuda.current_stream().cuda_stream) == (0, 0)
    torch.cuda.synchronize()
    return sc.cpu().numpy(), ids.cpu().numpy()


@pytest.mark.parametrize("name", V.KNAMES)
def test_quant_list_scan_equals_the_quantised_scan_over_the_probed_lists(name):
    _, D, Q, k, nprobe, filtered = V.KCASES[V.KNAMES.index(name)]
    lay = V.kernel_layout(D, Q)
    b = Bufs(lay)
    probes = V.kernel_probes(Q, nprobe)
    tiles = V.probe_tiles(probes)
    P = max(len(t) for t in tiles) + P_EXTRA
    filt, want = user_filter(Q, filtered)
    rs, rm, sc, ids, cand, guard = qlscan(b, k, probes, P, filt)
    assert (rs, rm) == (0, 0)
    ref_s, ref_pos = qscan128(b, list_filter(probes, want))
    exp_s, exp_i = host_merge(ref_s, ref_pos, lay["rowid"], k)
    assert np.isfinite(ref_s[ref_pos >= 0]).all()  # no NaN code or scale of the padding reached a score
    assert np.array_equal(ids, exp_i), "ids or their order differ from the quantised scan over the probed lists"
    assert np.array_equal(u32(sc), u32(exp_s)), "score bits differ from kind 34's"
    # every slot was written and nothing after them; a workgroup past its query's probe set left key 0
    cand = cand.reshape(P, Q, k)
    assert (cand != FF).all() and (guard == FF).all()
    for qi in range(Q):
        assert (cand[len(tiles[qi]):, qi] == 0).all()
        assert (cand[:len(tiles[qi]), qi, 0] != 0).all() or filtered  # an unfiltered whole tile has a best row
    assert (ids[ids >= 0] < V.N_EXT).all()
    if nprobe >= 2 and not filtered:  # query 0 probes both lists of the duplicate pair: the lower id first
        a, c = [int(np.flatnonzero(ids[0] == i)[0]) if i in ids[0] else -1 for i in V.DUP]
        assert a == 0 and (k == 1 or (c == 1 and u32(sc)[0, 0] == u32(sc)[0, 1]))
    again = qlscan(b, k, probes, P, filt)
    assert np.array_equal(u32(again[2]), u32(sc)) and np.array_equal(again[3], ids) and np.array_equal(again[4].reshape(P, Q, k), cand)


@pytest.mark.parametrize("D,Q,k", [(16, 16, 10), (528, 3, 128), (1024, 1, 1), (1040, 3, 10), (2048, 16, 10)])
def test_every_list_equals_the_quantised_scan_over_the_stored_rows(D, Q, k):
    lay = V.kernel_layout(D, Q)
    b = Bufs(lay)
    rs, rm, sc, ids, cand, guard = qlscan(b, k, None, V.NTILE)
    assert (rs, rm) == (0, 0) and (guard == FF).all()
    ref_s, ref_pos = qscan128(b, np.zeros((Q, 2), np.uint32))
    exp_s, exp_i = host_merge(ref_s, ref_pos, lay["rowid"], k)
    assert np.array_equal(ids, exp_i) and np.array_equal(u32(sc), u32(exp_s))
    assert ids[0, 0] == V.DUP[0] and (k == 1 or ids[0, 1] == V.DUP[1])
    again = qlscan(b, k, None, V.NTILE)
    assert np.array_equal(u32(again[2]), u32(sc)) and np.array_equal(again[3], ids) and np.array_equal(again[4], cand)


def test_the_score_bits_do_not_depend_on_the_launch():
    """The same (query, row) scores the same bits whatever the probe set, P, Q, k and the filter are."""
    lay = V.kernel_layout(528, 3)
    b = Bufs(lay)
    _, _, s_all, i_all, _, _ = qlscan(b, 128, np.array([[4, 1, 3, 2, 0]] * 3, np.int32), V.NTILE)
    seen = {(qi, int(i)): s for qi in range(3) for i, s in zip(i_all[qi], u32(s_all)[qi]) if i >= 0}
    for k, probes, filt in ((1, np.array([[4], [3], [1]], np.int32), None), (10, np.array([[1, 4], [4, 3], [2, 1]], np.int32), None),
                            (10, np.array([[4, 3], [1, 2], [3, 4]], np.int32), user_filter(3, True)[0])):
        P = max(len(t) for t in V.probe_tiles(probes))
        _, _, sc, ids, _, _ = qlscan(b, k, probes, P, filt)
        for qi in range(3):
            for i, s in zip(ids[qi], u32(sc)[qi]):
                assert i < 0 or (qi, int(i)) not in seen or seen[(qi, int(i))] == s
    one = Bufs(dict(lay, q=lay["q"][1:2]))  # Q = 1: query 1 alone
    _, _, sc, ids, _, _ = qlscan(one, 10, np.array([[4, 3]], np.int32), 5)
    assert all(seen.get((1, int(i)), s) == s for i, s in zip(ids[0], u32(sc)[0]))


def test_the_quant_list_launcher_refuses_misuse_without_launching():
    lay = V.kernel_layout(16, 3)
    b = Bufs(lay)
    probes = V.kernel_probes(3, 2)

    def refused(code, k=10, P=6, probes=probes, tweak=None, Q=None):
        rs, rm, sc, ids, cand, guard = qlscan(b, k, probes, P, tweak=tweak, Q=Q)
        assert rs == code and rm is None, (rs, code)
        assert (cand == FF).all() and (guard == FF).all() and (sc == 7.0).all() and (ids == -7).all()  # nothing ran

    def setd(p, D, ldc=None):
        p.D, p.ldc = D, D if ldc is None else ldc
    refused(-16, tweak=lambda p: setd(p, 24))                               # the byte rows' cases
    refused(-17, tweak=lambda p: setd(p, 8))
    refused(-18, tweak=lambda p: setd(p, 2064))
    refused(-19, tweak=lambda p: setd(p, 32, 16))
    refused(-23, tweak=lambda p: setd(p, 16, 24))
    refused(-24, tweak=lambda p: setattr(p, "scales", 0))
    refused(-25, tweak=lambda p: setattr(p, "scales", p.scales + 2))
    refused(-12, tweak=lambda p: setattr(p, "live", 0))                    # the filtered scan's refusals
    refused(-13, tweak=lambda p: setattr(p, "live_bytes", 4))
    refused(-14, tweak=lambda p: (setattr(p, "filt", p.live), setattr(p, "tags", 0)))
    refused(-15, tweak=lambda p: setattr(p, "tags", p.tags + 1))
    refused(-5, k=0)
    refused(-5, k=129)
    refused(-4, Q=17)
    refused(-6, tweak=lambda p: setattr(p, "corpus", p.corpus + 2))
    refused(-1, tweak=lambda p: setattr(p, "out_score", 0))
    refused(-3, tweak=lambda p: setattr(p, "N", 0))
    refused(-7, tweak=lambda p: setattr(p, "cand_bytes", p.cand_bytes - 8))  # below P * Q * k * 8
    refused(-40, tweak=lambda p: setattr(p, "nlist", 0))                   # the list launcher's
    refused(-41, tweak=lambda p: setattr(p, "nprobe", 0))
    refused(-41, tweak=lambda p: setattr(p, "nprobe", V.NLIST + 1))
    refused(-41, tweak=lambda p: (setattr(p, "nlist", 200), setattr(p, "nprobe", 129)))
    refused(-42, P=0)
    refused(-42, P=V.NTILE - 1, probes=None)                                # every list: P is the tile count
    refused(-43, tweak=lambda p: setattr(p, "N", p.N - 1))
    for table in ("list_off", "list_tiles", "rowid"):
        refused(-44, tweak=lambda p, t=table: setattr(p, t, 0))
        refused(-45, tweak=lambda p, t=table: setattr(p, t, getattr(p, t) + 2))
    refused(-45, tweak=lambda p: setattr(p, "probes", p.probes + 1))
    rs, rm, sc, ids, cand, guard = qlscan(b, 10, probes, 6)  # and the same buffers are accepted
    assert (rs, rm) == (0, 0) and (ids >= 0).all()


def test_tables_that_point_outside_only_idle_their_workgroups():
    """A probe id outside [0, nlist), offsets that do not ascend and a tile id outside the index end in zero keys
    for the queries they concern -- nothing is read through them -- and leave the other queries' answers alone."""
    lay = V.kernel_layout(16, 3)
    b = Bufs(lay)
    probes = V.kernel_probes(3, 2)
    good = qlscan(b, 10, probes, 6)
    bad = probes.copy()
    bad[1] = (-1, V.NLIST)
    rs, rm, sc, ids, cand, guard = qlscan(b, 10, bad, 6)
    assert (rs, rm) == (0, 0) and (cand.reshape(6, 3, 10)[:, 1] == 0).all() and (ids[1] == -1).all()
    assert np.array_equal(ids[[0, 2]], good[3][[0, 2]]) and np.array_equal(u32(sc[[0, 2]]), u32(good[2][[0, 2]]))
    keep = b.list_tiles
    b.list_tiles = dev_i32(np.where(V.LIST_TILES == 6, V.NTILE, V.LIST_TILES).astype(np.int32))  # list 3's first tile
    rs, rm, sc, ids, cand, guard = qlscan(b, 10, np.array([[3], [2], [4]], np.int32), 4)
    assert (rs, rm) == (0, 0) and (cand.reshape(4, 3, 10)[0, 0] == 0).all() and (cand.reshape(4, 3, 10)[1, 0] != 0).all()
    b.list_tiles = keep
    b.list_off = dev_i32(np.array([0, 0, 1, 9, 4, 7], np.int32))  # list 2 would run past the table
    rs, rm, sc, ids, cand, guard = qlscan(b, 10, np.array([[2], [1], [4]], np.int32), 4)
    assert (rs, rm) == (0, 0) and (ids[0] == -1).all() and (ids[1] >= 0).all() and (guard == FF).all()


DEBUG_CHILD = r"""
import json, os, sys
sys.path.insert(0, "tests")
import numpy as np
import search_ivf_fp8_cases as V
import test_search_ivf_fp8_gpu as G
from hipzap import _native as N
from hipzap.utils import kcheck
assert N.DEBUG and os.path.basename(N._LIB_PATH) == "libhipzap_debug.so", N._LIB_PATH
ran = 0
for name, D, Q, k, nprobe, filtered in V.KCASES:
    b = G.Bufs(V.kernel_layout(D, Q))
    probes = V.kernel_probes(Q, nprobe)
    P = max(len(t) for t in V.probe_tiles(probes)) + G.P_EXTRA
    rc = G.qlscan(b, k, probes, P, G.user_filter(Q, filtered)[0])[:2]
    rc2 = G.qlscan(b, k, None, V.NTILE)[:2]
    assert rc == (0, 0) and rc2 == (0, 0), (name, rc, rc2)
    ran += 2
print("RESULT " + json.dumps({"fails": kcheck.poll(), "ran": ran}))
"""


def test_debug_contracts_hold_over_the_kernel_cases():
    lib = ROOT / "hipzap" / "_lib" / "libhipzap_debug.so"
    assert lib.exists(), "build it first: python -m hipzap.build --debug"
    env = dict(os.environ, HIPZAP_DEBUG="1", HIPZAP_NO_AUTOBUILD="1")
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert res["fails"] == [] and res["ran"] == 2 * len(V.KCASES), res
