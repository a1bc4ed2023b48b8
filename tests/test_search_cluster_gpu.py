"""The assign kernel (csrc/search.hip, HZ_K_SEARCH_ASSIGN) and the mean kernel (HZ_K_SEARCH_CMEAN) through
``hz_launch_kernel``, against the fp64 oracles of tests/search_cluster_cases.py (bounds and cases there).

Assign: the chosen centroid's fp64 score is within twice the bound of the fp64 maximum and equals the oracle's index
wherever the oracle's margin exceeds twice the bound; the score is within the bound of the chosen centroid's fp64
score; rows without their bit give -1 / -inf; memory past N keeps its poison. Wherever two GPU runs are compared, they
are compared bit for bit -- kind 39's scores included."""
import ctypes as C

import numpy as np
import pytest
import torch

from hipzap import _native as N
from hipzap import search as S
from hipzap.ops import search as OS

import search_cluster_cases as F
from search_cluster_cases import T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 37  # poisoned words past N in both outputs


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assign(rows_bits, cent_bits, live, fill=None):
    """Kind 41 over device copies -> (rc, out_list [N], out_score [N]); asserts the poison past N. ``fill``: a uint16
    pattern written over the rows without their bit first."""
    n, d = rows_bits.shape
    host = rows_bits.copy()
    if fill is not None:
        host[~np.asarray(live, bool)] = fill
    corpus = torch.from_numpy(host.view(np.int16)).to(DEV)
    cent = torch.from_numpy(np.ascontiguousarray(cent_bits).view(np.int16)).to(DEV)
    words = S.pack_live(live)
    lv = torch.from_numpy(words.view(np.int32)).to(DEV)
    ol = torch.full((n + PAD,), -7, dtype=torch.int32, device=DEV)
    osc = torch.full((n + PAD,), 7.0, dtype=torch.float32, device=DEV)
    p = OS.AssignParams(corpus.data_ptr(), cent.data_ptr(), lv.data_ptr(), ol.data_ptr(), osc.data_ptr(), words.size * 4,
                        n, d, cent_bits.shape[0], d, d, 0)
    rc = N.lib().hz_launch_kernel(N.HZ_K_SEARCH_ASSIGN, C.byref(p), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ol, osc = ol.cpu().numpy(), osc.cpu().numpy()
    assert (ol[n:] == -7).all() and (osc[n:] == 7.0).all()
    return rc, ol[:n], osc[:n]


@pytest.mark.parametrize("name", F.ASSIGN_NAMES)
def test_the_nearest_centroid_matches_the_oracle(name):
    rb, cb, live = F.build_assign(name)
    rc, ol, osc = assign(rb, cb, live)
    assert rc == 0
    soft, worst = F.check_assign(ol, osc, *F.assign_oracle(name), live)
    print(f"{name}: rows inside the margin {soft}/{rb.shape[0]}, worst |err|/bound {worst:.4f}")


@pytest.mark.parametrize("pattern", [0x7FC0, 0x7F80, 0xFF80])
@pytest.mark.parametrize("name", ["n255_c63", "n600_c200", "n600_c200_d2048"])
def test_what_a_dead_row_holds_never_reaches_a_result(name, pattern):
    rb, cb, live = F.build_assign(name)
    zero, bad = assign(rb, cb, live, fill=0), assign(rb, cb, live, fill=pattern)
    assert zero[0] == bad[0] == 0
    assert np.array_equal(zero[1], bad[1]) and np.array_equal(u32(zero[2]), u32(bad[2]))
    assert np.isfinite(bad[2][live]).all() and (bad[1][~live] == -1).all()


def test_duplicate_centroids_in_different_blocks_tie_to_the_lower_index():
    rb, cb = F.make_assign(600, 96, 200, 11)
    cb[70] = cb[5]
    rb[[3, 300, 597]] = cb[5]  # rows that are the duplicated centroid: an exact tie at the top
    live = np.ones(600, bool)
    rc, ol, osc = assign(rb, cb, live)
    assert rc == 0 and (ol[[3, 300, 597]] == 5).all() and not (ol == 70).any()
    best = F.assign_ref(rb, cb, live)[0]
    assert (best == 5).sum() >= 3 and np.array_equal(ol[best == 5], best[best == 5])
    swapped = cb.copy()
    swapped[[5, 130]] = swapped[[130, 5]]  # now 70 and 130 hold the pattern: 70 wins
    rc, ol2, osc2 = assign(rb, swapped, live)
    assert (ol2[[3, 300, 597]] == 70).all() and np.array_equal(u32(osc2[[3, 300, 597]]), u32(osc[[3, 300, 597]]))


def test_the_bits_of_a_score_depend_on_the_centroid_and_the_row_only():
    """One pair (c*, r*): at C = 1 and inside C = 200, at centroid index 0 and 130, at row 3 of tile 0 and in the last
    partial tile, with other live bits flipped, over 20 replays."""
    d, n = 96, 600
    rb, cb = F.make_assign(n, d, 200, 12)
    cstar = cb[17].copy()
    rstar = S.to_bf16((S.bf16_to_f32(cstar) * np.float32(4.0))[None, :])[0]  # 4 |c*|^2: c* is its best by far
    rc, ol, osc = assign(rstar[None, :], cstar[None, :], np.ones(1, bool))
    assert rc == 0 and ol[0] == 0
    want = int(u32(osc)[0])
    for at in (0, 130):
        cents = cb.copy()
        cents[17] = cb[at]
        cents[at] = cstar
        for row in (3, n - 3):
            rows = rb.copy()
            rows[row] = rstar
            for live in (np.ones(n, bool), F.live_pattern("alternating", n) | (np.arange(n) == row),
                         F.live_pattern("dead_tile", n) | (np.arange(n) == row)):
                rc, ol, osc = assign(rows, cents, live)
                assert rc == 0 and ol[row] == at and int(u32(osc)[row]) == want, (at, row)
    first = assign(rows, cents, live)
    for _ in range(20):
        again = assign(rows, cents, live)
        assert np.array_equal(first[1], again[1]) and np.array_equal(u32(first[2]), u32(again[2]))


def test_the_scores_are_kind_39s_bits():
    """A corpus of 64 rows followed by 64 centroids: the self scan with qid = the centroid rows, k = 128, skip_self = 0
    returns every score; the assign kernel's score of each row is bitwise the maximum over the centroids of kind 39's
    scores, and its list the lowest such centroid."""
    import test_search_neighbors_gpu as G
    rb, cb = F.make_assign(64, 96, 64, 13)
    cb[40] = cb[9]  # an exact tie for the rows nearest to centroid 9
    rb[5] = cb[9]   # and one such row for certain
    both = np.concatenate([rb, cb])
    qid = np.arange(64, 128, dtype=np.int32)
    rs, rm, sc, ids = G.launch(both, qid, 128, np.ones(128, bool), 0)
    assert (rs, rm) == (0, 0) and (ids >= 0).all()
    full = np.zeros((64, 128), np.float32)  # [centroid, row of the corpus]
    for c in range(64):
        full[c, ids[c]] = sc[c]
    full = full[:, :64]
    rc, ol, osc = assign(rb, cb, np.ones(64, bool))
    assert rc == 0
    assert np.array_equal(u32(osc), u32(full.max(axis=0)))
    assert np.array_equal(ol, np.argmax(full, axis=0).astype(np.int32))  # the lowest index among equals
    assert (ol == 9).any() and not (ol == 40).any()


# ---------------------------------------------------------------------------------------- cmean
def cmean(rows_bits, order, seg_off, cosine, cent_bits=None, c32=True):
    """Kind 42 over device copies -> (rc, cent bits [C, D], cent32 [C, D])."""
    n, d = rows_bits.shape
    c = len(seg_off) - 1
    start = np.full((c, d), 0x4049, np.uint16) if cent_bits is None else cent_bits  # 3.140625: "untouched"
    corpus = torch.from_numpy(rows_bits.view(np.int16)).to(DEV)
    od = torch.from_numpy(np.ascontiguousarray(order, np.int32)).to(DEV)
    sd = torch.from_numpy(np.ascontiguousarray(seg_off, np.int32)).to(DEV)
    cd = torch.from_numpy(np.ascontiguousarray(start).view(np.int16).copy()).to(DEV)
    c32d = torch.full((c, d), -5.0, dtype=torch.float32, device=DEV)
    p = OS.CmeanParams(corpus.data_ptr(), od.data_ptr(), sd.data_ptr(), cd.data_ptr(), c32d.data_ptr() if c32 else None,
                       n, d, c, len(order), d, d, int(cosine), 0)
    rc = N.lib().hz_launch_kernel(N.HZ_K_SEARCH_CMEAN, C.byref(p), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, cd.cpu().numpy().view(np.uint16), c32d.cpu().numpy()


@pytest.mark.parametrize("cosine", [0, 1])
@pytest.mark.parametrize("d", [32, 2048])
def test_the_means_match_the_oracle(d, cosine):
    rows, order, seg_off = F.make_cmean(d)
    rc, bits, c32 = cmean(rows, order, seg_off, cosine)
    assert rc == 0
    ref, sabs, cnt = F.cmean_ref(rows, order, seg_off, cosine)
    bound = F.cmean_bound(rows, order, seg_off, cosine)
    assert (bits[0] == 0x4049).all() and (c32[0] == -5.0).all()  # the empty segment leaves both outputs untouched
    err = np.abs(c32[1:].astype(np.float64) - ref[1:])
    print(f"D={d} cosine={cosine}: worst |err|/bound {(err / bound[1:]).max():.4f}")
    assert (err <= bound[1:]).all()
    assert np.array_equal(bits[1:], S.to_bf16(c32[1:]))  # the RNE rounding of the kernel's own fp32 values
    rc, bits2, _ = cmean(rows, order, seg_off, cosine, c32=False)  # cent32 may be null
    assert rc == 0 and np.array_equal(bits, bits2)
    # the skipped ids neither count nor add: the segment without them gives the same bits
    keep = np.ones(order.size, bool)
    keep[[seg_off[3] + 5, seg_off[3] + 200]] = False
    off2 = seg_off.copy()
    off2[4:] -= 2
    rc, bits3, c323 = cmean(rows, order[keep], off2, cosine)
    assert rc == 0 and np.array_equal(u32(c323[[1, 2, 4]]), u32(c32[[1, 2, 4]]))
    assert (np.abs(c323[3].astype(np.float64) - ref[3]) <= bound[3]).all()


def test_the_means_are_replayable_and_independent_of_the_other_segments():
    rows, order, seg_off = F.make_cmean(2048)
    first = cmean(rows, order, seg_off, 1)
    for _ in range(20):
        again = cmean(rows, order, seg_off, 1)
        assert np.array_equal(first[1], again[1]) and np.array_equal(u32(first[2]), u32(again[2]))
    # the 1000-member segment alone (C = 1), and placed third of seven with other segments around it
    big = order[seg_off[4]:seg_off[5]]
    rc, b1, c1 = cmean(rows, big, np.array([0, big.size], np.int32), 1)
    assert rc == 0 and np.array_equal(u32(c1[0]), u32(first[2][4])) and np.array_equal(b1[0], first[1][4])
    other = order[seg_off[3]:seg_off[4]]
    order7 = np.concatenate([other[:10], other[10:40], big, other[40:], other[:3]])
    off7 = np.array([0, 10, 40, 40 + big.size, 40 + big.size, 40 + big.size + other.size - 40, order7.size - 1, order7.size], np.int32)
    rc, b7, c7 = cmean(rows, order7, off7, 1)
    assert rc == 0 and np.array_equal(u32(c7[2]), u32(first[2][4])) and np.array_equal(b7[2], first[1][4])
    assert (b7[3] == 0x4049).all()


def test_a_segment_table_that_is_no_table_writes_nothing():
    rows, order, seg_off = F.make_cmean(32)
    for bad in ([0, -1, 3, 3, 3, 3], [0, 5, 2, 2, 2, 2], [0, 1, 2, 3, 4, order.size + 1]):
        rc, bits, c32 = cmean(rows, order, np.array(bad, np.int32), 0)
        assert rc == 0
        for c in range(5):
            lo, hi = bad[c], bad[c + 1]
            if lo < 0 or hi < lo or hi > order.size or hi == lo:
                assert (bits[c] == 0x4049).all() and (c32[c] == -5.0).all(), (bad, c)


DEBUG_CHILD = """
import sys
sys.path.insert(0, "tests")
import numpy as np
from hipzap.utils import kcheck
import search_cluster_cases as F
import test_search_cluster_gpu as G
assert kcheck.enabled()
for name in ("n1_c1", "n255_c63", "n257_c65", "n600_c200", "n600_c1_d32"):
    rb, cb, live = F.build_assign(name)
    rc, ol, osc = G.assign(rb, cb, live)
    assert rc == 0, (name, rc)
    F.check_assign(ol, osc, *F.assign_oracle(name), live)
rows, order, seg_off = F.make_cmean(32)
rc, bits, c32 = G.cmean(rows, order, seg_off, 1)
ref = F.cmean_ref(rows, order, seg_off, True)[0]
assert rc == 0 and (np.abs(c32[1:] - ref[1:]) <= F.cmean_bound(rows, order, seg_off, True)[1:]).all()
fails = kcheck.poll()
assert fails == [], fails
print("silent")
"""


def test_the_debug_library_checks_stay_silent_on_the_edge_shapes():
    """The HZ_DCHECK unit of search.hip guards the tile range, the centroid range and both output writes of the assign
    kernel and the member reads of the mean kernel: the debug library (a child process: HIPZAP_DEBUG selects the
    library at import) runs the smallest and the most ragged cases with the right answers and no record."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(os.path.join(root, "hipzap", "_lib", "libhipzap_debug.so")), "python -m hipzap.build --debug"
    env = dict(os.environ, HIPZAP_DEBUG="1", HIPZAP_NO_AUTOBUILD="1")
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "silent" in r.stdout, r.stderr[-4000:]
