"""The binary scan (csrc/search.hip, HZ_K_SEARCH_BSCAN: sign-bit rows, queries binarised in the kernel) and the
existing merge against the exact oracle ``search_bin_cases.bin_scan_ref``.

Scores are integers, so every comparison is bit for bit: the keys the merge returns equal the oracle's keys."""
import numpy as np
import pytest
import torch

from hipzap import search as S
from hipzap.ops import search as OS

import search_bin_cases as B
from search_bin_cases import T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x5A5A5A5A5A5A5A5A
FILL = 0xFFFFFFFF  # what dead rows and the pitch padding hold


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def launch(words, q, k, live=None, tags=None, filt=None, N=None, D=None, Q=None, ldc=None, tweak=None, fill=FILL,
           replays=1):
    """Binary scan + merge over device copies -> (scan rc, merge rc, scores [Q, k], ids [Q, k], guards intact).
    Dead rows and the words from W to the pitch's end hold ``fill``; ``cand`` lies between two guard words."""
    n, w = words.shape
    live = np.ones(n, bool) if live is None else np.asarray(live, bool)
    ldc = ldc or w
    host = np.full((n, max(ldc, w)), fill, np.uint32)
    host[:, :w] = words
    host[~live] = fill
    corpus = torch.from_numpy(host.view(np.int32)).to(DEV)
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV)
    Qn = q.shape[0] if Q is None else Q
    nbytes = max(OS.scratch_bytes(n, min(max(Qn, 1), 16), min(max(k, 1), 128)), 8)
    buf = torch.full((nbytes // 8 + 4,), GUARD, dtype=torch.int64, device=DEV)  # two guard words on each side
    cand = buf[2:-2]
    cand.zero_()
    sc = torch.full((max(Qn, 1), max(k, 1)), 7.0, dtype=torch.float32, device=DEV)  # 7 / -7: "never written"
    ids = torch.full((max(Qn, 1), max(k, 1)), -7, dtype=torch.int32, device=DEV)
    lw = S.pack_live(live)
    lv = torch.from_numpy(lw.view(np.int32)).to(DEV)
    tg = None if tags is None else torch.from_numpy(np.ascontiguousarray(tags, np.uint32).view(np.int32)).to(DEV)
    fl = None if filt is None else torch.from_numpy(np.ascontiguousarray(filt, np.uint32).reshape(-1, 2).view(np.int32)).to(DEV)
    p = OS.BinScanParams(corpus.data_ptr(), qd.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(),
                         n if N is None else N, 32 * w if D is None else D, Qn, k, ldc, 0, nbytes, lv.data_ptr(),
                         0 if tg is None else tg.data_ptr(), 0 if fl is None else fl.data_ptr(), lw.size * 4)
    if tweak:
        tweak(p)
    outs = []
    for _ in range(replays):
        rc = OS.launch_bin(p, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        outs.append((sc.cpu().numpy().copy(), ids.cpu().numpy().copy()))
    g = buf.cpu().numpy()
    intact = bool((g[:2] == GUARD).all() and (g[-2:] == GUARD).all())
    if replays > 1:
        return rc[0], rc[1], outs, intact
    return rc[0], rc[1], outs[0][0], outs[0][1], intact


def check(words, q, k, allow, sc, ids):
    want = B.bin_scan_ref(words, B.binarize(q), k, allow)
    got = B.keys_of(sc, ids)
    assert np.array_equal(got, want), "keys differ from bin_scan_ref"
    assert (sc[ids < 0] == -np.inf).all()


@pytest.mark.parametrize("pitch", [0, 4])
@pytest.mark.parametrize("name", B.GRID_NAMES)
def test_keys_equal_the_oracle_bit_for_bit(name, pitch):
    words, q, k = B.grid_case(name)
    rs, rm, sc, ids, intact = launch(words, q, k, ldc=words.shape[1] + pitch)
    assert (rs, rm) == (0, 0) and intact
    check(words, q, k, None, sc, ids)


def test_identical_and_duplicated_rows_come_back_in_id_order():
    row, q = B.make(1, 768, 3, 5)
    words = np.repeat(row, 700, axis=0)
    rs, rm, sc, ids, intact = launch(words, q, 128)
    assert (rs, rm) == (0, 0) and intact
    assert np.array_equal(ids, np.tile(np.arange(128, dtype=np.int32), (3, 1)))
    assert all(len(set(u32(sc[qi]).tolist())) == 1 for qi in range(3))
    words, q = B.make(600, 256, 3, 6)
    words[300:] = words[:300]  # row i + 300 equals row i: always right behind it
    rs, rm, sc, ids, _ = launch(words, q, 128)
    assert (rs, rm) == (0, 0)
    check(words, q, 128, None, sc, ids)
    for qi in range(3):
        same = sc[qi, 1:] == sc[qi, :-1]
        assert same.sum() >= 64 and (np.diff(ids[qi])[same] > 0).all()  # every row has a twin: ties, in id order

@pytest.mark.parametrize("D", [128, 768, 2048])
def test_the_extremes_are_plus_d_and_minus_d_and_not_the_sentinel(D):
    W = D // 32
    words = np.zeros((300, W), np.uint32)
    words[::2] = 0xFFFFFFFF  # even rows: every sign clear; odd rows: every sign set
    q = np.abs(np.random.default_rng(0).standard_normal((2, D))).astype(np.float32) + np.float32(0.1)
    rs, rm, sc, ids, intact = launch(words, q, 128)
    assert (rs, rm) == (0, 0) and intact
    assert (sc == D).all() and np.array_equal(ids[0], np.arange(0, 256, 2))
    odd = np.arange(300) % 2 == 1
    rs, rm, sc, ids, _ = launch(words, q, 10, odd)
    assert (rs, rm) == (0, 0) and (sc == -D).all() and np.array_equal(ids[1], np.arange(1, 21, 2))


def test_query_sign_edges_are_binarised_like_the_rows():
    vals = B.sign_edge_values()
    rng = np.random.default_rng(3)
    q = vals[rng.integers(0, vals.size, (16, 256))]
    rows = vals[rng.integers(0, vals.size, (300, 256))]
    words = S.binarize(rows)
    assert np.array_equal(words, B.binarize(rows))
    rs, rm, sc, ids, _ = launch(words, q, 10)
    assert (rs, rm) == (0, 0)
    check(words, q, 10, None, sc, ids)
    # a query of -0.0 alone matches exactly the all-set rows: score +D against a row of zeros words
    qz = np.full((1, 128), -0.0, np.float32)
    w2 = np.zeros((2, 4), np.uint32)
    w2[1] = 0xFFFFFFFF
    rs, rm, sc, ids, _ = launch(w2, qz, 2)
    assert ids.tolist() == [[0, 1]] and sc.tolist() == [[128.0, -128.0]]
    rs, rm, sc, ids, _ = launch(w2, -qz, 2)  # +0.0: sign clear
    assert ids.tolist() == [[1, 0]] and sc.tolist() == [[128.0, -128.0]]


@pytest.mark.parametrize("pattern", B.LIVE_PATTERNS)
def test_live_bitmaps_and_tag_predicates(pattern):
    N, D, k = 700, 768, 10
    words, q = B.make(N, D, 4, 21)
    live = B.live_pattern(pattern, N)
    tags = (np.arange(N) % 11).astype(np.uint32)
    filt = np.array([[0, 0], [0xFFFFFFFF, 99], [0xFFFFFFFF, 5], [4, 4]], np.uint32)  # all, none, tags == 5, bit 2 set
    for kw, allow in (({}, live),
                      ({"tags": tags, "filt": filt}, live[None, :] & ((tags[None, :] & filt[:, :1]) == filt[:, 1:]))):
        base = launch(words, q, k, live, ldc=28, **kw)
        assert base[:2] == (0, 0) and base[4]
        check(words, q, k, allow, base[2], base[3])
        other = launch(words, q, k, live, ldc=28, fill=0, **kw)  # what dead rows and the padding hold changes no key
        assert np.array_equal(u32(base[2]), u32(other[2])) and np.array_equal(base[3], other[3])
    assert (base[3][1] == -1).all()


def test_score_bits_depend_on_the_query_bits_and_the_row_words_only():
    D = 768
    words, q16 = B.make(3 * T + 5, D, 16, 41)
    one = q16[5:6].copy()
    row = B.binarize(one)[0]
    row[0] ^= 0x7  # three bits from the query: score D - 6, above every other row's
    seen = set()
    plans = [(1, None, 1, False), (16, 7, 128, True), (16, 0, 128, False), (16, 15, 1, True)]  # Q, slot, k, filtered
    for N, at in ((1, 0), (T, T - 1), (T + 1, T), (3 * T + 5, 3 * T + 4)):
        w = words[:N].copy()
        w[at] = row
        tags = (np.arange(N) % 3).astype(np.uint32)
        tags[at] = 2
        for Q, slot, k, filtered in plans:
            if Q == 1:
                qs, slot = one, 0
            else:
                qs = q16.copy()
                qs[slot] = one[0]
            kw = {"tags": tags, "filt": np.tile(np.array([[3, 2]], np.uint32), (Q, 1))} if filtered else {}
            rs, rm, sc, ids, _ = launch(w, qs, k, **kw)
            assert (rs, rm) == (0, 0) and ids[slot, 0] == at, (N, at, Q, slot, k, filtered)
            seen.add(int(u32(sc)[slot, 0]))
    assert seen == {int(u32(np.float32(D - 6)))}, seen


def test_twenty_replays_are_bitwise_equal():
    words, q = B.make(3 * T + 5, 768, 16, 46)
    rs, rm, outs, intact = launch(words, q, 128, replays=20)
    assert (rs, rm) == (0, 0) and intact
    for sc, ids in outs[1:]:
        assert np.array_equal(u32(sc), u32(outs[0][0])) and np.array_equal(ids, outs[0][1])
    check(words, q, 128, None, *outs[0])


def test_the_launcher_refuses_misuse_without_launching():
    words, q = B.make(40, 256, 2, 44)
    live, tags, filt = np.ones(40, bool), np.zeros(40, np.uint32), np.zeros((2, 2), np.uint32)
    seen = {}

    def refused(what, code, k=10, tags=tags, filt=filt, **kw):
        rs, rm, sc, ids, intact = launch(words, q, k, live, tags, filt, **kw)
        assert rs == code and rm is None, (what, rs)
        assert (sc == 7.0).all() and (ids == -7).all() and intact, what  # nothing ran
        seen[what] = rs

    for field in ("corpus", "queries", "cand", "out_score", "out_id"):
        refused(field + " null", -80, tweak=lambda p, f=field: setattr(p, f, 0))
    refused("D % 128", -81, D=192)
    refused("D < 128", -82, D=0)
    refused("D > 2048", -83, D=2176, ldc=68)
    refused("ldc < W", -84, tweak=lambda p: setattr(p, "ldc", 4))
    refused("ldc % 4", -84, tweak=lambda p: setattr(p, "ldc", 10))
    refused("N = 0", -85, N=0)
    refused("N < 0", -85, N=-5)
    refused("Q = 0", -86, Q=0)
    refused("Q = 17", -86, Q=17)
    refused("k = 0", -87, k=0)
    refused("k = 129", -87, k=129)
    refused("corpus misaligned", -88, tweak=lambda p: setattr(p, "corpus", p.corpus + 8))
    refused("queries misaligned", -88, tweak=lambda p: setattr(p, "queries", p.queries + 4))
    refused("cand misaligned", -88, tweak=lambda p: setattr(p, "cand", p.cand + 4))
    refused("tags misaligned", -88, tweak=lambda p: setattr(p, "tags", p.tags + 2))
    refused("filt misaligned", -88, tweak=lambda p: setattr(p, "filt", p.filt + 2))
    refused("live misaligned", -88, tweak=lambda p: setattr(p, "live", p.live + 2))
    refused("live null", -89, tweak=lambda p: setattr(p, "live", 0))
    refused("short live", -90, tweak=lambda p: setattr(p, "live_bytes", 4))  # 40 rows need 2 words
    refused("filt without tags", -91, tags=None)
    refused("short cand", -92, tweak=lambda p: setattr(p, "cand_bytes", p.cand_bytes - 8))
    assert set(seen.values()) == set(range(-92, -79))  # every code of the list is hit
    rs, rm, sc, ids, intact = launch(words, q, 10, live, tags, filt)  # and the same buffers are accepted
    assert (rs, rm) == (0, 0) and intact
    check(words, q, 10, live, sc, ids)


def test_the_kind_is_registered_and_launches_through_the_table():
    from hipzap import _native as N
    lib = N.lib()
    assert N.KINDS["HZ_K_SEARCH_BSCAN"] == 43 and lib.hz_kernel_name(43) == b"HZ_K_SEARCH_BSCAN"
    import ctypes as C
    assert lib.hz_kernel_param_size(43) == C.sizeof(OS.BinScanParams)


DEBUG_CHILD = """
import sys
sys.path.insert(0, "tests")
import numpy as np
from hipzap.utils import kcheck
import search_bin_cases as B
import test_search_bin_gpu as G
assert kcheck.enabled()
for name in B.GRID_NAMES:
    words, q, k = B.grid_case(name)
    for pitch in (0, 4):
        rs, rm, sc, ids, intact = G.launch(words, q, k, ldc=words.shape[1] + pitch)
        assert (rs, rm) == (0, 0) and intact, (name, rs, rm)
        G.check(words, q, k, None, sc, ids)
words, q = B.make(700, 768, 4, 21)
for pattern in B.LIVE_PATTERNS:
    live = B.live_pattern(pattern, 700)
    rs, rm, sc, ids, intact = G.launch(words, q, 10, live)
    assert (rs, rm) == (0, 0) and intact
    G.check(words, q, 10, live, sc, ids)
fails = kcheck.poll()
assert fails == [], fails
print("silent")
"""


def test_the_debug_library_checks_stay_silent_on_the_grid():
    """The HZ_DCHECK unit of search.hip guards the tile range, row < N, the live words and ``rank < k`` of the binary
    scan: the debug library (a child process: HIPZAP_DEBUG selects the library at import) runs the grid and the live
    patterns with the right answers and no record."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(os.path.join(root, "hipzap", "_lib", "libhipzap_debug.so")), "python -m hipzap.build --debug"
    env = dict(os.environ, HIPZAP_DEBUG="1", HIPZAP_NO_AUTOBUILD="1")
    r = subprocess.run([sys.executable, "-c", DEBUG_CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "silent" in r.stdout, r.stderr[-4000:]
