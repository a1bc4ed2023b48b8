"""``Index.cluster`` and the IVF build on the GPU against ``RefIndex.cluster``, ``ivf_kmeans`` and the fp64 oracles of
tests/search_cluster_cases.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hipzap import search as S

import search_cluster_cases as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    rows, lab, init = F.planted()
    path = str(tmp_path_factory.mktemp("cl") / "planted.hzidx")
    S.write_index(path, rows, "cosine")
    return path, rows, lab, init


@pytest.fixture(scope="module")
def rand(tmp_path_factory):
    rows = F.random_rows()
    path = str(tmp_path_factory.mktemp("cl") / "random.hzidx")
    S.write_index(path, rows, "cosine")
    return path, rows


def test_the_planted_labels_come_back_exactly(planted):
    path, rows, lab, init = planted
    with S.Index(path) as ix, S.RefIndex(path) as ref:
        bits, assign, score = ix.cluster(8, iters=4, init=init)
        rbits, rassign, rscore = ref.cluster(8, iters=4, init=init)
        kbits, kassign = S.ivf_kmeans(S.bf16_to_f32(S.read_rows(path)), 8, "cosine", 0, 4, init=init)
    assert np.array_equal(assign, lab) and np.array_equal(rassign, lab) and np.array_equal(kassign, lab)
    assert bits.dtype == np.uint16 and assign.dtype == np.int32 and score.dtype == np.float32
    assert np.abs(bits.astype(np.int64) - rbits.astype(np.int64)).max() <= 1  # one bf16 ulp of the fp64 oracle's
    s, b = F.scores64(S.read_rows(path), bits)
    assert (np.abs(score - s[np.arange(600), lab]) <= b[np.arange(600), lab]).all()


@pytest.mark.parametrize("seed", [0, 3])
def test_iters_0_gives_the_bits_of_ivf_kmeans(rand, seed):
    path, rows = rand
    with S.Index(path) as ix:
        bits, assign, score = ix.cluster(16, iters=0, seed=seed)
    stored = S.bf16_to_f32(S.read_rows(path))
    kb, ka = S.ivf_kmeans(stored, 16, "cosine", seed, 0)
    assert np.array_equal(bits, kb)
    F.check_assign(assign, score, *F.scores64(S.read_rows(path), bits), *F.assign_ref(S.read_rows(path), bits, np.ones(1000, bool)),
                   np.ones(1000, bool))


def test_random_rows_the_argmax_and_the_means_hold(rand):
    path, rows = rand
    rb = S.read_rows(path)
    with S.Index(path) as ix:
        bits, assign, score = ix.cluster(16, iters=3, seed=1)
        train, c32 = ix._cluster_trace
        again = ix.cluster(16, iters=3, seed=1)
    assert np.array_equal(bits, again[0]) and np.array_equal(assign, again[1]) and np.array_equal(score.view(np.uint32), again[2].view(np.uint32))
    live = np.ones(1000, bool)
    F.check_assign(assign, score, *F.scores64(rb, bits), *F.assign_ref(rb, bits, live), live)
    # every centroid with members is, within the cmean bound, the mean of the rows of the last training assignment
    assert (train >= 0).all()  # 1000 rows <= 256 * 16: the sample is every row
    order = np.argsort(train, kind="stable").astype(np.int32)
    seg_off = np.concatenate([[0], np.cumsum(np.bincount(train, minlength=16))]).astype(np.int32)
    ref, sabs, cnt = F.cmean_ref(rb, order, seg_off, True)
    bound = F.cmean_bound(rb, order, seg_off, True)
    has = cnt > 0
    assert has.sum() >= 8 and (np.abs(c32[has] - ref[has]) <= bound[has]).all()
    assert np.array_equal(bits[has], S.to_bf16(c32[has]))


def test_deleted_rows_are_left_out_and_nothing_is_reallocated(rand):
    path, rows = rand
    rb = S.read_rows(path)
    with S.Index(path) as ix:
        ix.cluster(16, iters=1, seed=2, ctx=0)  # a context's buffers are its own: the same context both times
        before = ix.describe()["device_bytes"]
        gone = np.arange(100, 200, 2)
        assert ix.delete(gone) == 50
        bits, assign, score = ix.cluster(16, iters=2, seed=2, ctx=0)
        assert ix.describe()["device_bytes"] == before
        assert (assign[gone] == -1).all() and (score[gone] == -np.inf).all()
        live = np.ones(1000, bool)
        live[gone] = False
        assert (assign[live] >= 0).all()
        F.check_assign(assign, score, *F.scores64(rb, bits), *F.assign_ref(rb, bits, live), live)
        b0 = ix.cluster(16, iters=0, seed=2)[0]
    dead = {rb[r].tobytes() for r in gone}
    alive = {rb[r].tobytes() for r in np.flatnonzero(live)}
    assert all(b0[c].tobytes() in alive and b0[c].tobytes() not in dead for c in range(16))


def test_fp8_and_ivf_indexes_are_refused_by_name(rand, tmp_path):
    path, rows = rand
    fp8, ivf = str(tmp_path / "q.hzidx"), str(tmp_path / "l.hzidx")
    S.write_index(fp8, rows, "cosine", dtype="fp8")
    S.write_index(ivf, rows, "cosine", ivf=4)
    with S.Index(fp8) as ix, pytest.raises(ValueError, match="fp8_e4m3 index of version 3"):
        ix.cluster(4)
    with S.Index(ivf) as ix, pytest.raises(ValueError, match="an IVF index of version 5"):
        ix.cluster(4)
    with S.Index(fp8) as ix:  # the native entry points refuse on their own
        out, sc = np.empty(1000, np.int32), np.empty(1000, np.float32)
        cb = np.zeros((4, 96), np.uint16)
        assert ix._lib.hz_index_assign(ix._h, 0, cb.ctypes.data, 4, None, out.ctypes.data, sc.ctypes.data) == -38
        assert b"fp8_e4m3 index of version 3" in ix._lib.hz_index_last_error()


def test_an_ivf_index_built_on_the_gpu(rand, tmp_path):
    path, rows = rand
    out, plain = str(tmp_path / "ivf.hzidx"), path
    hdr = S.write_index(out, rows, "cosine", ivf=16, ivf_seed=1, ivf_iters=3, ivf_backend="gpu")
    assert hdr["ivf"]["nlist"] == 16
    assert not [n for n in os.listdir(tmp_path) if n.startswith(".cluster-")]  # the temporary index is gone
    with S.Index(plain) as ix:
        bits, assign, _ = ix.cluster(16, iters=3, seed=1)
    t = S.read_ivf(out)
    lay = S.ivf_layout(assign, 16)
    assert np.array_equal(t["centroids"], bits)
    for k in ("list_off", "list_tiles", "rowid"):
        assert np.array_equal(t[k], lay[k]), k
    q = F.random_rows(8, 96, 9)
    with S.Index(out) as gi, S.RefIndex(out) as ri, S.Index(plain) as pi:
        s, i = gi.search(q, 10, nprobe="all")
        ps, pid = pi.search(q, 10)
        assert np.array_equal(i, pid) and np.array_equal(s.view(np.uint32), ps.view(np.uint32))
        rs, rid = ri.search(q, 10, nprobe="all")
        assert np.array_equal(rid, i)
    conv = str(tmp_path / "ivf8.hzidx")
    S.convert_index(plain, conv, "fp8", rescore=True, ivf=16, ivf_seed=1, ivf_iters=3, ivf_backend="gpu")
    assert np.array_equal(S.read_ivf(conv)["rowid"], lay["rowid"]) and S.RefIndex(conv).version == 7


def test_hipzap_cluster_on_the_gpu_backend(rand, tmp_path):
    path, rows = rand
    out = str(tmp_path / "clusters.npz")
    r = subprocess.run([sys.executable, "-m", "hipzap", "cluster", path, "--k", "16", "--iters", "3", "--seed", "1", "--out", out,
                        "--backend", "gpu"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["backend"] == "gpu"
    z = np.load(out)
    with S.Index(path) as ix:
        bits, assign, score = ix.cluster(16, iters=3, seed=1)
    assert np.array_equal(z["centroids"], bits) and np.array_equal(z["assign"], assign)
    assert np.array_equal(z["score"].view(np.uint32), score.view(np.uint32))
