"""Product quantisation's assignment step on the host: ``pq_assign_f32`` (the oracle of HZ_K_SEARCH_PQASSIGN and the
``"f32"`` backend) against the fp64 encoder, the backends of ``pq_train`` / ``pq_encode`` / ``write_index`` /
``convert_index`` / ``Index.add``, the CLI's argument errors, and the digests of every file version written with
default arguments. No GPU."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

from hipzap import search as S

import search_pqenc_cases as P
from search_pqenc_cases import T, gamma, u32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vectors(n=300, d=128):
    i = np.arange(n * d, dtype=np.uint64)
    return (((i * np.uint64(2654435761)) % np.uint64(2003)).astype(np.float32) / np.float32(1001.5) - np.float32(1.0)).reshape(n, d)


TAGS = (np.arange(300) % 5).astype(np.uint32)


# ------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("D,M", P.SHAPES)
def test_integer_case_equals_the_fp64_encoder_and_ties_go_to_the_lower_index(D, M):
    rows, cb = P.make("integer", P.NMAX, D, M)
    codes, dist = P.ref("integer", P.NMAX, D, M)
    assert codes.dtype == np.uint8 and dist.dtype == np.float32 and codes.shape == dist.shape == (P.NMAX, M)
    assert np.array_equal(codes, S.pq_encode(rows, cb))
    assert (codes < P.DUP).all()  # centroid c + DUP .. repeats centroid c: the lower one wins every tie
    assert np.array_equal(dist.astype(np.float64), P.d64(rows, cb, codes))  # exact
    brute = ((rows.reshape(-1, M, 1, D // M).astype(np.float64) - cb[None].astype(np.float64)) ** 2).sum(axis=3)[:40]
    assert np.array_equal(codes[:40], np.argmin(brute, axis=2))


@pytest.mark.parametrize("kind", ["inexact", "neartie"])
@pytest.mark.parametrize("D,M", P.SHAPES)
def test_where_float32_and_fp64_choose_differently_the_certificate_holds(D, M, kind):
    """|d^ - d| <= g d with g = gamma(dsub + 2) (one rounding in the subtraction, one in the square, dsub - 1 in the
    sum; every term is non-negative), so the float32 winner c' has d(c') <= d(c*) (1 + g) / (1 - g)."""
    rows, cb = P.make(kind, P.NMAX, D, M)
    codes, dist = P.ref(kind, P.NMAX, D, M)
    g = gamma(D // M + 2)
    mine = P.d64(rows, cb, codes)
    assert (np.abs(dist.astype(np.float64) - mine) <= g * mine).all()
    c64 = S.pq_encode(rows, cb)
    differ = codes != c64
    print(f"D={D} M={M} {kind}: {int(differ.sum())} of {differ.size} codes differ from the fp64 encoder")
    assert (mine[differ] <= P.d64(rows, cb, c64)[differ] * (1 + g) / (1 - g)).all()
    if kind == "neartie" and D // M >= 2:
        assert differ.any()  # the case is hard enough to tell the two apart


def test_results_do_not_depend_on_chunking_or_on_n():
    rows, cb = P.make("neartie", P.NMAX, 48, 16)
    want = P.ref("neartie", P.NMAX, 48, 16)
    for chunk in (1, 7, T, P.NMAX, 10 ** 6):
        got = S.pq_assign_f32(rows, cb, chunk=chunk)
        assert np.array_equal(got[0], want[0]) and np.array_equal(u32(got[1]), u32(want[1])), chunk
    one = S.pq_assign_f32(rows[500:501], cb)
    assert np.array_equal(one[0][0], want[0][500]) and np.array_equal(u32(one[1][0]), u32(want[1][500]))
    assert np.array_equal(S.pq_encode(rows, cb, backend="f32"), want[0])
    assert S.pq_encode(rows[:0], cb, backend="f32").shape == (0, 16)
    with pytest.raises(ValueError, match="chunk"):
        S.pq_assign_f32(rows, cb, chunk=0)
    with pytest.raises(ValueError, match=r"rows must be \[N, 48\]"):
        S.pq_assign_f32(rows[:, :32], cb)


def test_a_nan_never_displaces_and_a_column_that_starts_on_one_keeps_code_zero():
    rows, cb = P.make("inexact", 20, 128, 16)
    cb = cb.copy()
    cb[0, 0], cb[1, 5], cb[2, :, 3] = np.nan, np.nan, np.nan
    codes, dist = S.pq_assign_f32(rows, cb)
    assert (codes[:, 0] == 0).all() and np.isnan(dist[:, 0]).all()
    assert (codes[:, 1] != 5).all() and not np.isnan(dist[:, 1]).any()
    assert (codes[:, 2] == 0).all() and np.isnan(dist[:, 2]).all()
    clean = S.pq_assign_f32(rows, P.make("inexact", 20, 128, 16)[1])
    assert np.array_equal(codes[:, 3:], clean[0][:, 3:]) and np.array_equal(u32(dist[:, 3:]), u32(clean[1][:, 3:]))


# ------------------------------------------------------------------------------------------- training
# sha256 of pq_train(bf16(vectors(900, 64)), 16, seed=3, iters=3) as the parent commit computed it
PARENT_CODEBOOK = "68164e595e241ed16063282b9a9e25ce56f9702628dcfcd9dcafbde1c9b83bec"


def test_pq_train_backends():
    x = S.bf16_to_f32(S.prepare_rows(vectors(900, 64), "ip"))
    assert hashlib.sha256(S.pq_train(x, 16, seed=3, iters=3).tobytes()).hexdigest() == PARENT_CODEBOOK
    assert hashlib.sha256(S.pq_train(x, 16, seed=3, iters=3, backend="cpu").tobytes()).hexdigest() == PARENT_CODEBOOK
    a, b = S.pq_train(x, 16, seed=3, iters=3, backend="f32"), S.pq_train(x, 16, seed=3, iters=3, backend="f32")
    assert a.dtype == np.float32 and a.shape == (16, 256, 4) and np.array_equal(u32(a), u32(b))  # deterministic
    assert not np.array_equal(a, S.pq_train(x, 16, seed=4, iters=3, backend="f32"))
    # the same sample and first centroids whatever the backend, and iters=0 / init are honoured
    assert np.array_equal(u32(S.pq_train(x, 16, seed=3, iters=0, backend="f32")), u32(S.pq_train(x, 16, seed=3, iters=0)))
    cb = S.pq_train(x, 16, seed=3, iters=0, backend="f32")
    for _ in range(3):
        cb = S.pq_train(x, 16, seed=3, iters=1, init=cb, backend="f32")
    assert np.array_equal(u32(cb), u32(a))
    init = P.make("inexact", 1, 64, 16)[1]
    assert np.array_equal(u32(S.pq_train(x, 16, iters=0, init=init, backend="f32")), u32(init))
    # one iteration is the means of pq_assign_f32's clusters: fp64 sums in row order, rounded to fp32; a centroid
    # without members keeps its value (900 rows cannot fill 256 clusters of a far-away codebook)
    far = init.copy()
    far[:, 100:] += np.float32(50.0)
    got = S.pq_train(x, 16, seed=3, iters=1, init=far, backend="f32")
    codes = S.pq_assign_f32(x, far)[0]
    sub = x.reshape(900, 16, 4)
    for j in (0, 7, 15):
        for c in range(256):
            members = sub[codes[:, j] == c, j].astype(np.float64)
            want = far[j, c] if members.shape[0] == 0 else (np.add.reduce(members, axis=0) / members.shape[0]).astype(np.float32)
            assert np.array_equal(u32(got[j, c]), u32(want)), (j, c)
    assert (codes < 100).all() and np.array_equal(u32(got[:, 100:]), u32(far[:, 100:]))  # empty clusters are kept


def test_value_errors():
    x = S.bf16_to_f32(S.prepare_rows(vectors(300, 64), "ip"))
    cb = S.pq_train(x, 16, iters=0)
    for call in (lambda: S.pq_encode(x, cb, backend="cuda"), lambda: S.pq_train(x, 16, backend="fp32"),
                 lambda: S.prepare_rows_pq(x, "ip", 16, backend="")):
        with pytest.raises(ValueError, match=r"backend must be one of \('cpu', 'f32', 'gpu'\)"):
            call()
    odd = x.copy()
    odd[5, 3] = np.float32(1.0) + np.float32(2.0 ** -20)  # not a bf16 number
    with pytest.raises(ValueError, match="exactly representable in bf16"):
        S.pq_encode(odd, cb, backend="gpu")
    with pytest.raises(ValueError, match="exactly representable in bf16"):
        S.pq_train(odd, 16, iters=1, backend="gpu")
    assert S.pq_encode(odd, cb, backend="f32").shape == (300, 16)  # the numpy backends take any fp32 row


def test_write_and_convert_with_the_f32_backend_store_the_same_bytes(tmp_path):
    v = vectors()
    p = {k: str(tmp_path / f"{k}.hzidx") for k in ("v1", "w", "c", "wt", "ct", "cpu", "no")}
    S.write_index(p["v1"], v, "cosine")
    ha = S.write_index(p["w"], v, "cosine", dtype="pq", pq_m=16, pq_iters=2, pq_backend="f32")
    hb = S.convert_index(p["v1"], p["c"], "pq", pq_m=16, pq_iters=2, pq_backend="f32")
    assert ha == hb and open(p["w"], "rb").read() == open(p["c"], "rb").read()
    rows = S.bf16_to_f32(S.prepare_rows(v, "cosine"))
    cb = S.pq_train(rows, 16, iters=2, backend="f32")
    assert np.array_equal(u32(S.read_codebook(p["w"])), u32(cb))
    assert np.array_equal(S.read_rows(p["w"]), S.pq_assign_f32(rows, cb)[0])
    # a given codebook: only the encoder changes, and with it at most the codes the certificate allows
    S.write_index(p["wt"], v, "cosine", dtype="pq", pq_m=16, pq_codebook=cb, pq_backend="f32", rescore=True)
    S.convert_index(p["v1"], p["ct"], "pq", pq_m=16, pq_codebook=cb, pq_backend="f32", rescore=True)
    assert open(p["wt"], "rb").read() == open(p["ct"], "rb").read() and S.file_info(p["wt"])["version"] == 11
    S.write_index(p["cpu"], v, "cosine", dtype="pq", pq_m=16, pq_codebook=cb, rescore=True)
    assert len(open(p["cpu"], "rb").read()) == len(open(p["wt"], "rb").read())
    for kw, msg in ((dict(dtype="pq", pq_m=16, pq_backend="hip"), "pq_backend must be one of"),
                    (dict(dtype="fp8", pq_backend="f32"), "go with dtype='pq'"), (dict(pq_backend="gpu"), "go with dtype='pq'")):
        with pytest.raises(ValueError, match=msg):
            S.write_index(p["no"], v, "cosine", **kw)
        with pytest.raises(ValueError, match=msg):
            S.convert_index(p["v1"], p["no"], **{"dtype": "bf16", **kw})
    assert not os.path.exists(p["no"])


def test_refindex_add_takes_an_encoder_on_a_pq_index_only(tmp_path):
    v = vectors()
    rows = S.bf16_to_f32(S.prepare_rows(v, "cosine"))
    cb = S.pq_train(rows, 16, iters=1)
    pq, bf = str(tmp_path / "pq.hzidx"), str(tmp_path / "bf.hzidx")
    S.write_index(pq, v[:200], "cosine", dtype="pq", pq_m=16, pq_codebook=cb)
    S.write_index(bf, v[:200], "cosine")
    with S.RefIndex(pq, reserve=200) as ix:
        ids = ix.add(v[200:], encoder="f32")
        assert np.array_equal(ids, np.arange(200, 300, dtype=np.int32))
        assert np.array_equal(ix._bits[200:300], S.pq_assign_f32(rows[200:], cb)[0])
        with pytest.raises(ValueError, match="encoder must be one of"):
            ix.add(v[:2], encoder="fast")
    with S.RefIndex(bf) as ix:
        for enc in ("f32", "gpu"):
            with pytest.raises(ValueError, match="goes with a pq8 index"):
                ix.add(v[200:], encoder=enc)
        assert ix.add(v[200:202], encoder="cpu").tolist() == [200, 201]  # the default is accepted everywhere


def test_cli_argument_errors(tmp_path):
    from hipzap.__main__ import main
    v = vectors()
    vn, out = str(tmp_path / "v.npy"), str(tmp_path / "no.hzidx")
    np.save(vn, v)
    for args, words in ((("--vectors", vn, "--pq-backend", "gpu"), "--pq-backend goes with --dtype pq"),
                        (("--vectors", vn, "--dtype", "fp8", "--pq-backend", "f32"), "--pq-backend goes with --dtype pq"),
                        (("--vectors", vn, "--dtype", "bin", "--pq-backend", "cpu"), "--pq-backend goes with --dtype pq")):
        with pytest.raises(SystemExit) as e:
            main(["index", *args, "--out", out])
        assert words in str(e.value), (args, e.value)
    with pytest.raises(SystemExit) as e:  # argparse's own refusal of a fourth name
        main(["index", "--vectors", vn, "--dtype", "pq", "--pq-m", "16", "--pq-backend", "hip", "--out", out])
    assert e.value.code == 2 and not os.path.exists(out)
    ok = str(tmp_path / "f32.hzidx")
    main(["index", "--vectors", vn, "--dtype", "pq", "--pq-m", "16", "--pq-iters", "1", "--pq-backend", "f32", "--out", ok])
    want = S.prepare_rows_pq(v, "cosine", 16, iters=1, backend="f32")
    assert np.array_equal(S.read_rows(ok), want[0]) and np.array_equal(u32(S.read_codebook(ok)), u32(want[1]))


def test_the_kind_is_registered_and_refuses_without_a_device():
    from hipzap import _native as N
    from hipzap.ops import search as OS
    lib = N.lib()
    assert N.HZ_K_SEARCH_PQASSIGN == 48 and lib.hz_kernel_name(48) == b"HZ_K_SEARCH_PQASSIGN"
    assert lib.hz_kernel_param_size(48) == C.sizeof(OS.PqAssignParams) == 72
    good = OS.PqAssignParams(16, 16, 16, 16, 40 * 16 * 4, 40, 128, 16, 128, 16)
    for field, value, code in (("rows", 0, -129), ("codebook", 0, -129), ("codes", 0, -129), ("D", 120, -130), ("M", 48, -130),
                               ("M", 0, -132), ("D", 16 * 65, -133), ("ldr", 120, -135), ("ldr", 132, -135), ("ldc", 0, -136),
                               ("ldc", 24, -136), ("N", 0, -137), ("rows", 24, -138), ("dist", 20, -138),
                               ("dist_bytes", 40 * 16 * 4 - 1, -139)):
        bad = OS.PqAssignParams.from_buffer_copy(good)
        setattr(bad, field, value)
        assert lib.hz_launch_kernel(N.HZ_K_SEARCH_PQASSIGN, C.byref(bad), None) == code, (field, value)
        assert OS.launch_pq_assign(bad) == code
    for d, m, code in ((120, 24, -131), (224, 112, -132), (2064, 48, -134)):
        bad = OS.PqAssignParams(16, 16, 16, 0, 0, 40, d, m, 2064, 112)
        assert OS.launch_pq_assign(bad) == code, (d, m)
    # the batch job returns the launcher's codes for a shape before it touches a device
    x = np.zeros((4, 128), np.uint16)
    cbk = np.zeros((16, 256, 8), np.float32)
    out = np.zeros((4, 16), np.uint8)
    for n, d, m, code in ((4, 120, 16, -130), (4, 120, 24, -131), (4, 224, 112, -132), (4, 16 * 65, 16, -133), (4, 2064, 48, -134),
                          (0, 128, 16, -137)):
        assert lib.hz_pq_encode(0, x.ctypes.data, n, d, m, cbk.ctypes.data, 0, out.ctypes.data, None) == code, (n, d, m)
    assert lib.hz_pq_encode(0, None, 4, 128, 16, cbk.ctypes.data, 0, out.ctypes.data, None) == -129
    assert lib.hz_pq_encode(0, x.ctypes.data, 4, 128, 16, cbk.ctypes.data, -1, out.ctypes.data, None) == -141
    assert b"chunk_rows" in lib.hz_index_last_error()


# ----------------------------------------------------------------------------------------------- files
# Whole-file digests of what the parent commit's writer produced for `vectors()` with default arguments: the numbers of
# tests/test_search_pq_cpu.py for versions 1-9 (sizes where the IVF k-means decides bytes), and versions 10 / 11 trained
# and encoded by the default ("cpu") backend. This test passes on the parent commit too, by design.
RECORDED = {
    "v1": "195c174d5587e1f9709b101293d590e4d17e64571f37dda6347c3f8d3f619797",
    "v2": "d4bfb3e64e2e01c4bfe0b26fbb4cb992aac8a970fd98cefc48af93e34c27a9f5",
    "v3": "503f58b08ba713ec400034a4cf11b00dde090c5b79af4e54cd5514f4ac09fea8",
    "v4": "1c78698e1a341be39432cb16f5c771ee01708e1e46644ab3af70fbfaa3088060",
    "v5": 224256, "v6": 130048, "v7": 207872,
    "v8": "fe46f9f7e6d30c1350a81f4211fefe33c76425284c15c744ce93d409b166a3ce",
    "v8t": "a4135cdf526b8a323d1676bd663499de99d09b24ebc8446fe9a8f82c9ffb3cb5",
    "v9": "239d2bed81b6c304f3466f159795201ee86ad0702de08bdfb4c480f6e09bb16e",
    "v9t": "45c4689933864c9d46af16be8d180963fa6554e0c3cb1c55ee5c361d1901efe8",
    "v10": "d0fac976599cf677fa541a034601a2581647b57d810345d6958faf3eacd25f52",
    "v10t": "e746ecf62e85e1667def34de93363a7b3999fc2741b8dced829f018c32b72825",
    "v10c": "d0fac976599cf677fa541a034601a2581647b57d810345d6958faf3eacd25f52",
    "v11": "4a3bc1e3d970f363ba2096c6325906c55531dbcca11efba4be8a28c918cc43f7",
    "v11t": "5e98ee894560f5d0744eeeab9eee79a19fecba632d1b3e1df405622ff0671c6f",
}


def test_versions_1_to_11_are_written_as_before(tmp_path):
    v, out = vectors(), {}
    for name, kw in (("v1", {}), ("v2", {"tags": TAGS}), ("v3", {"dtype": "fp8"}),
                     ("v4", {"dtype": "fp8", "rescore": True, "tags": TAGS}),
                     ("v5", {"tags": TAGS, "ivf": 3, "nprobe": 2, "ivf_seed": 1}), ("v8", {"dtype": "bin"}),
                     ("v8t", {"dtype": "bin", "tags": TAGS}), ("v9", {"dtype": "bin", "rescore": True}),
                     ("v9t", {"dtype": "bin", "rescore": True, "tags": TAGS}), ("v10", {"dtype": "pq", "pq_m": 16}),
                     ("v10t", {"dtype": "pq", "pq_m": 16, "tags": TAGS}), ("v11", {"dtype": "pq", "pq_m": 16, "rescore": True}),
                     ("v11t", {"dtype": "pq", "pq_m": 32, "rescore": True, "tags": TAGS, "pq_seed": 3, "pq_iters": 2})):
        out[name] = str(tmp_path / f"{name}.hzidx")
        S.write_index(out[name], v, "cosine", labels=[f"r{i}" for i in range(300)], model="m", **kw)
    out["v6"], out["v7"], out["v10c"] = str(tmp_path / "v6.hzidx"), str(tmp_path / "v7.hzidx"), str(tmp_path / "v10c.hzidx")
    S.convert_index(out["v5"], out["v6"], "fp8")
    S.convert_index(out["v5"], out["v7"], "fp8", rescore=True)
    S.convert_index(out["v1"], out["v10c"], "pq", pq_m=16)
    for name, p in out.items():
        raw = open(p, "rb").read()
        want = RECORDED[name]
        assert (len(raw) if isinstance(want, int) else hashlib.sha256(raw).hexdigest()) == want, name
        assert S.file_info(p)["version"] == int(name.rstrip("tc")[1:])
