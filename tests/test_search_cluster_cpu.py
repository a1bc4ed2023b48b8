"""Clustering on the host: the case matrix and its oracle margins, ``RefIndex.cluster`` against ``ivf_kmeans`` on
planted data, ``ivf_kmeans(init=)``, the Python mirrors of kinds 41 and 42, every refusal of the two launchers (nothing
is launched, so no GPU is needed), the ValueErrors, ``hipzap cluster --backend cpu`` and ``write_index(ivf_backend=)``."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hipzap import _native as N
from hipzap import search as S
from hipzap.ops import search as OS

import search_cluster_cases as F
from search_cluster_cases import CB, T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------- 1. the cases
def test_the_case_matrix_covers_what_the_kernels_can_get_wrong():
    Ns, Ds, Cs = ({c[i] for c in F.ASSIGN_CASES} for i in (1, 2, 3))
    assert Ns >= {1, T - 1, T, T + 1, 600} and Ds >= {32, 96, 2048} and Cs >= {1, CB - 1, CB, CB + 1, 200}
    pats = {c[4] for c in F.ASSIGN_CASES}
    assert pats >= {"one_dead", "dead_group", "dead_tile"}
    for name, n, d, c, pat, seed in F.ASSIGN_CASES:
        live = F.live_pattern(pat, n)
        groups = live[:n // 16 * 16].reshape(-1, 16)
        if pat == "one_dead":
            assert (groups.any(axis=1) & ~groups.all(axis=1)).any()  # a dead row in a mixed group
        if pat == "dead_group":
            assert (~groups.any(axis=1)).any()
        if pat == "dead_tile":
            assert not live[T:2 * T].any() and n % T and not live[n - 2]  # a dead tile; a partial last tile
    assert any(c[1] % T for c in F.ASSIGN_CASES)
    assert set(F.CMEAN_SIZES) == {0, 1, 2, 257, 1000}
    rows, order, seg_off = F.make_cmean(32)
    assert ((order < 0) | (order >= F.CMEAN_N)).sum() == 2 and seg_off[-1] == order.size


@pytest.mark.parametrize("name", F.ASSIGN_NAMES)
def test_at_most_one_row_in_a_hundred_is_inside_the_margin(name):
    rb, cb, live = F.build_assign(name)
    s, b, best, top, second = F.assign_oracle(name)
    soft = F.unclear(s, b, best, top, second, live)
    assert soft.sum() <= 0.01 * rb.shape[0], (name, int(soft.sum()))
    # the oracle passes its own check: fp32 of its score, its own index
    F.check_assign(best, np.where(live, top, -np.inf).astype(np.float32).astype(np.float64), s, np.maximum(b, 2.0 ** -20 * np.abs(s)),
                   best, top, second, live)


def test_cmean_ref_is_the_mean_and_the_bound_is_small():
    rows, order, seg_off = F.make_cmean(32)
    for cosine in (False, True):
        ref, sabs, cnt = F.cmean_ref(rows, order, seg_off, cosine)
        assert cnt.tolist() == [0, 1, 2, 255, 1000] and np.isnan(ref[0]).all()
        assert np.allclose(ref[1], S.bf16_to_f32(rows[order[0]]) / (np.linalg.norm(S.bf16_to_f32(rows[order[0]]).astype(np.float64)) if cosine else 1))
        if cosine:
            assert np.allclose(np.linalg.norm(ref[1:], axis=1), 1)
        bound = F.cmean_bound(rows, order, seg_off, cosine)
        assert (bound[0] == 0).all() and (bound[1:] > 0).all() and bound.max() < 1e-3


# ------------------------------------------------------------------------------- 2. the Python side
@pytest.fixture(scope="module")
def planted(tmp_path_factory):
    rows, lab, init = F.planted()
    path = str(tmp_path_factory.mktemp("cl") / "planted.hzidx")
    S.write_index(path, rows, "cosine")
    return path, rows, lab, init


def test_refindex_cluster_recovers_the_planted_labels_like_ivf_kmeans(planted):
    path, rows, lab, init = planted
    with S.RefIndex(path) as ix:
        bits, assign, score = ix.cluster(8, iters=4, init=init)
        stored = S.bf16_to_f32(S.read_rows(path))
        assert np.array_equal(assign, lab) and assign.dtype == np.int32 and score.dtype == np.float32
        assert bits.dtype == np.uint16 and bits.shape == (8, 64)
        kb, ka = S.ivf_kmeans(stored, 8, "cosine", 0, 4, init=init)
        assert np.array_equal(ka, lab)
        assert np.abs(bits.astype(np.int64) - kb.astype(np.int64)).max() <= 1  # fp64 against fp32 means: one bf16 ulp
        # the margin of the planted data against the assign bound
        s, b = F.scores64(S.read_rows(path), bits)
        best, top, second = F.assign_ref(S.read_rows(path), bits, np.ones(600, bool))
        assert (top - second).min() > 0.8 and b.max() < 1e-5
        # random starts: the same draw as ivf_kmeans
        for seed in (0, 3):
            b0 = ix.cluster(8, iters=0, seed=seed)[0]
            assert np.array_equal(b0, S.ivf_kmeans(stored, 8, "cosine", seed, 0)[0])
        b5, a5, _ = ix.cluster(16, iters=3, seed=1)
        assert (a5 == S.ivf_kmeans(stored, 16, "cosine", 1, 3)[1]).mean() > 0.99


def test_refindex_cluster_leaves_deleted_rows_out(planted, tmp_path):
    path, rows, lab, init = planted
    with S.RefIndex(path) as ix:
        gone = np.arange(0, 100, 2)
        ix.delete(gone)
        bits, assign, score = ix.cluster(8, iters=2, seed=5)
        assert (assign[gone] == -1).all() and (score[gone] == -np.inf).all()
        keep = np.setdiff1d(np.arange(600), gone)
        assert (assign[keep] >= 0).all()
        b0 = ix.cluster(8, iters=0, seed=5)[0]
        stored = S.read_rows(path)
        for c in range(8):  # every first centroid is a live row
            assert any(np.array_equal(b0[c], stored[r]) for r in keep) and not any(np.array_equal(b0[c], stored[r]) for r in gone)


def test_init_leaves_the_default_ivf_kmeans_output_unchanged():
    rows = F.random_rows(400, 32, 3)
    a = S.ivf_kmeans(rows, 8, "cosine", 2, 3)
    b = S.ivf_kmeans(rows, 8, "cosine", 2, 3, init=None)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # checksums of the default path's output, recorded from the code before init= existed
    assert int(a[0].astype(np.uint64).sum()) == 8277963 and int((a[1].astype(np.int64) * np.arange(400)).sum()) == 286319
    first = rows[:8]
    c = S.ivf_kmeans(rows, 8, "cosine", 2, 0, init=first)
    assert np.array_equal(c[0], S.to_bf16(first))


def test_every_value_error_names_the_value(planted, tmp_path):
    path, rows, lab, init = planted
    with S.RefIndex(path) as ix:
        for kw, word in ((dict(nlist=0), "0"), (dict(nlist=601), "601"), (dict(nlist=2.5), "2.5"), (dict(nlist=True), "True"),
                         (dict(nlist=8, iters=-1), "-1"), (dict(nlist=8, iters=1.5), "1.5"), (dict(nlist=8, seed=-2), "-2"),
                         (dict(nlist=8, seed="x"), "'x'"),
                         (dict(nlist=8, init=init[:7]), "[7, 64]"), (dict(nlist=8, init=init[:, :32]), "[8, 32]"),
                         (dict(nlist=8, init=init.astype(np.int32)), "int32"),
                         (dict(nlist=8, init=np.where(np.arange(64) == 3, np.nan, init)), "nan"),
                         (dict(nlist=8, init=np.where(np.arange(64) == 3, np.inf, init)), "inf")):
            nlist = kw.pop("nlist")
            with pytest.raises(ValueError, match=r".*" + word.replace("[", r"\[").replace("]", r"\]")):
                ix.cluster(nlist, **kw)
    with pytest.raises(ValueError, match="init must have the shape .*got .7, 32."):
        S.ivf_kmeans(rows, 8, "cosine", init=np.zeros((7, 32), np.float32))
    fp8, ivf, odd = (str(tmp_path / n) for n in ("q.hzidx", "l.hzidx", "o.hzidx"))
    S.write_index(fp8, rows, "cosine", dtype="fp8")
    S.write_index(ivf, rows, "cosine", ivf=4)
    S.write_index(odd, rows[:, :40], "cosine")
    with S.RefIndex(fp8) as ix, pytest.raises(ValueError, match="fp8_e4m3 index of version 3"):
        ix.cluster(4)
    with S.RefIndex(ivf) as ix, pytest.raises(ValueError, match="an IVF index of version 5"):
        ix.cluster(4)
    with S.RefIndex(odd) as ix, pytest.raises(ValueError, match="dim = 40"):
        ix.cluster(4)
    with pytest.raises(ValueError, match="ivf_backend must be one of .*'tpu'"):
        S.write_index(odd, rows, "cosine", ivf=4, ivf_backend="tpu")
    with pytest.raises(ValueError, match="ivf_backend='gpu' goes with ivf=nlist"):
        S.write_index(odd, rows, "cosine", ivf_backend="gpu")
    with pytest.raises(ValueError, match="dim = 40"):
        S.write_index(odd, rows[:, :40], "cosine", ivf=4, ivf_backend="gpu")
    with pytest.raises(ValueError, match="ivf_backend must be one of .*'x'"):
        S.convert_index(path, odd, "bf16", ivf=4, ivf_backend="x")


def test_write_index_with_the_cpu_backend_is_byte_identical_to_the_default(planted, tmp_path):
    path, rows, lab, init = planted
    a, b, c, d = (str(tmp_path / n) for n in ("a.hzidx", "b.hzidx", "c.hzidx", "d.hzidx"))
    S.write_index(a, rows, "cosine", ivf=8, ivf_seed=1, ivf_iters=3)
    S.write_index(b, rows, "cosine", ivf=8, ivf_seed=1, ivf_iters=3, ivf_backend="cpu")
    assert open(a, "rb").read() == open(b, "rb").read()
    S.convert_index(path, c, "fp8", ivf=8, ivf_seed=1)
    S.convert_index(path, d, "fp8", ivf=8, ivf_seed=1, ivf_backend="cpu")
    assert open(c, "rb").read() == open(d, "rb").read()


# ------------------------------------------------------------------------------- 3. the native side
def test_kinds_41_and_42_are_mirrored():
    lib = N.lib()
    assert (N.HZ_K_SEARCH_ASSIGN, N.HZ_K_SEARCH_CMEAN) == (41, 42)
    assert lib.hz_kernel_name(41) == b"HZ_K_SEARCH_ASSIGN" and lib.hz_kernel_name(42) == b"HZ_K_SEARCH_CMEAN"
    assert N.KIND_STRUCT[41] is OS.AssignParams and N.KIND_STRUCT[42] is OS.CmeanParams
    assert C.sizeof(OS.AssignParams) == lib.hz_kernel_param_size(41) == 72
    assert C.sizeof(OS.CmeanParams) == lib.hz_kernel_param_size(42) == 72
    assert OS.ASSIGN_MAX_C == S.IVF_MAX_LISTS == 65536 and OS.ASSIGN_CB == CB


def assign_params(**kw):
    v = dict(corpus=0x10000, cent=0x20000, live=0x30000, out_list=0x40000, out_score=0x50000, live_bytes=4 * 19,
             N=600, D=96, C=200, ldc=96, ldk=96, ntile=0)
    v.update(kw)
    return OS.AssignParams(**v)


def cmean_params(**kw):
    v = dict(corpus=0x10000, order=0x20000, seg_off=0x30000, cent=0x40000, cent32=0x50000, N=600, D=96, C=5, M=100, ldc=96,
             ldk=96, cosine=1, pad_=0)
    v.update(kw)
    return OS.CmeanParams(**v)


ASSIGN_REFUSALS = [
    (-61, dict(corpus=None)), (-61, dict(cent=None)), (-61, dict(live=None)), (-61, dict(out_list=None)), (-61, dict(out_score=None)),
    (-62, dict(D=40, ldc=40, ldk=40)), (-63, dict(D=0)), (-64, dict(D=2080, ldc=2080, ldk=2080)),
    (-65, dict(ldc=64)), (-65, dict(ldc=100)), (-65, dict(ldk=64)), (-65, dict(ldk=100)),
    (-66, dict(N=0)), (-66, dict(N=-5)), (-67, dict(C=0)), (-67, dict(C=65537)),
    (-68, dict(corpus=0x10008)), (-68, dict(cent=0x20008)), (-68, dict(live=0x30002)), (-68, dict(out_list=0x40001)),
    (-68, dict(out_score=0x50002)), (-69, dict(live_bytes=4 * 18)),
]
CMEAN_REFUSALS = [
    (-70, dict(corpus=None)), (-70, dict(order=None)), (-70, dict(seg_off=None)), (-70, dict(cent=None)),
    (-71, dict(D=40, ldc=40, ldk=40)), (-72, dict(D=0)), (-73, dict(D=2080, ldc=2080, ldk=2080)),
    (-74, dict(ldc=64)), (-74, dict(ldk=100)), (-75, dict(N=0)), (-76, dict(C=0)), (-76, dict(C=65537)), (-77, dict(M=-1)),
    (-78, dict(corpus=0x10008)), (-78, dict(cent=0x40008)), (-78, dict(order=0x20002)), (-78, dict(seg_off=0x30001)),
    (-78, dict(cent32=0x50002)), (-79, dict(cosine=2)), (-79, dict(cosine=-1)),
]


@pytest.mark.parametrize("code,kw", ASSIGN_REFUSALS)
def test_the_assign_launcher_refuses(code, kw):
    p = assign_params(**kw)
    assert N.lib().hz_search_assign_launch(C.byref(p), None) == code
    assert N.lib().hz_launch_kernel(N.HZ_K_SEARCH_ASSIGN, C.byref(p), None) == code


@pytest.mark.parametrize("code,kw", CMEAN_REFUSALS)
def test_the_cmean_launcher_refuses(code, kw):
    p = cmean_params(**kw)
    assert N.lib().hz_search_cmean_launch(C.byref(p), None) == code
    assert N.lib().hz_launch_kernel(N.HZ_K_SEARCH_CMEAN, C.byref(p), None) == code


def test_every_refusal_code_has_a_case():
    assert {c for c, _ in ASSIGN_REFUSALS} == set(range(-69, -60))
    assert {c for c, _ in CMEAN_REFUSALS} == set(range(-79, -69))
    # the first rule that fails names the code: a null pointer before the shape, the shape before the alignment
    assert N.lib().hz_search_assign_launch(C.byref(assign_params(corpus=None, D=40)), None) == -61
    assert N.lib().hz_search_assign_launch(C.byref(assign_params(D=40, corpus=0x10008)), None) == -62


# ------------------------------------------------------------------------------- 4. the command line
def test_hipzap_cluster_on_the_cpu_backend(planted, tmp_path):
    path, rows, lab, init = planted
    out = str(tmp_path / "clusters.npz")
    r = subprocess.run([sys.executable, "-m", "hipzap", "cluster", path, "--k", "8", "--iters", "3", "--seed", "2", "--out", out,
                        "--backend", "cpu"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["k"] == 8 and info["count"] == 600 and info["clustered_rows"] == 600 and info["backend"] == "cpu"
    z = np.load(out)
    with S.RefIndex(path) as ix:
        bits, assign, score = ix.cluster(8, iters=3, seed=2)
    assert np.array_equal(z["centroids"], bits) and np.array_equal(z["assign"], assign) and np.array_equal(z["score"], score)
    assert z["centroids"].dtype == np.uint16 and z["assign"].dtype == np.int32 and z["score"].dtype == np.float32
    r = subprocess.run([sys.executable, "-m", "hipzap", "cluster", path, "--k", "0", "--out", out, "--backend", "cpu"],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "got 0" in r.stderr
