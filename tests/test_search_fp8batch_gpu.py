"""Kinds 52 and 53 (csrc/search.hip): kind 52's merged keys against kind 44 over the decoded rows (bit for bit) and the fp64
oracle over the split query (two kernels sharing one mistake cannot pass both); kind 53 bit for bit against kinds 34 + 32."""
import ctypes as C

import numpy as np
import pytest
import torch

from hipzap import _native as N
from hipzap import search as S
from hipzap.ops import search as OS

import search_batch_cases as F
import test_search_batch_gpu as B
from test_search_batch_gpu import DEV, PAD, u32

pytestmark = pytest.mark.gpu
FINITE = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)  # the 254 finite e4m3fn codes
# (D, N, Q, k, live pattern): one row; a partial tile; two tiles, a full query block; three tiles, two blocks, dead rows
SHAPES = [(32, 1, 1, 1, "all"), (96, 255, 63, 10, "all"), (768, 257, 64, 128, "all"), (96, 600, 69, 128, "dead_group"),
          (768, 600, 69, 10, "dead_group")]


def make(n, d, nq, seed):
    rng = np.random.default_rng(seed)
    return FINITE[rng.integers(0, 254, (n, d))], rng.standard_normal((nq, d)).astype(np.float32), rng


def launch(codes, scales, q, k, live, tweak=None, poison=False):
    """Kinds 52 and 40 -> (scan rc, merge rc, scores, ids). ``poison``: NaN codes and scales in the dead rows and past N."""
    n, d = codes.shape
    Q = q.shape[0]
    ch, sh = np.concatenate([codes, np.zeros((300, d), np.uint8)]), np.concatenate([scales, np.ones(300, np.float32)])
    if poison:
        dead = np.concatenate([~np.asarray(live, bool), np.ones(300, bool)])
        ch[dead], sh[dead] = 0x7F, np.nan
    cd, sd = torch.from_numpy(ch).to(DEV), torch.from_numpy(sh.astype(np.float32)).to(DEV)
    qd = torch.from_numpy(np.ascontiguousarray(q, np.float32)).to(DEV)
    nbytes = max(OS.self_scratch_bytes(n, Q, k), 8)
    cand = torch.full((nbytes // 8 + PAD * k,), -1, dtype=torch.int64, device=DEV)
    sc = torch.full((Q + PAD, k), 7.0, dtype=torch.float32, device=DEV)
    ids = torch.full((Q + PAD, k), -7, dtype=torch.int32, device=DEV)
    words = S.pack_live(live)
    lv = torch.from_numpy(words.view(np.int32)).to(DEV)
    p = OS.QuantBatchScanParams(cd.data_ptr(), qd.data_ptr(), lv.data_ptr(), cand.data_ptr(), sc.data_ptr(), ids.data_ptr(),
                                words.size * 4, nbytes, n, d, Q, k, d, 0, (C.c_int * 2)(), sd.data_ptr(), 4 * n)
    if tweak:
        tweak(p)
    st = torch.cuda.current_stream().cuda_stream
    rs = N.lib().hz_launch_kernel(N.HZ_K_SEARCH_QXSCAN, C.byref(p), st)
    rm = N.lib().hz_launch_kernel(N.HZ_K_SEARCH_MERGEN, C.byref(p), st) if rs == 0 else None
    torch.cuda.synchronize()
    sch, idh, cah = sc.cpu().numpy(), ids.cpu().numpy(), cand.cpu().numpy()
    assert (sch[Q:] == 7.0).all() and (idh[Q:] == -7).all() and (cah[nbytes // 8:] == -1).all()
    if rs != 0:
        assert (sch == 7.0).all() and (idh == -7).all() and (cah == -1).all()  # refused: nothing ran
    return rs, rm, sch[:Q], idh[:Q]


@pytest.mark.parametrize("scaling", ["one", "pow2", "general"])
@pytest.mark.parametrize("d,n,nq,k,pattern", SHAPES)
def test_the_merged_keys_against_kind_44_and_the_fp64_oracle(d, n, nq, k, pattern, scaling):
    codes, q, rng = make(n, d, nq, d + n)
    live = F.live_pattern(pattern, n)
    live[n - 3:n - 2] &= pattern == "all"
    dec = S.e4m3_to_f32(codes)
    scales = {"one": np.ones(n), "pow2": 2.0 ** rng.integers(-3, 4, n), "general": rng.uniform(0.001, 3.0, n)}[scaling].astype(np.float32)
    rs, rm, sc, ids = launch(codes, scales, q, k, live)
    assert (rs, rm) == (0, 0)
    if scaling != "general":  # e4m3 times 2^-3 .. 2^3 is a bf16 value: every partial sum scales exactly
        want = B.launch(S.to_bf16(dec * scales[:, None]), q, k, live)
        assert want[:2] == (0, 0) and np.array_equal(u32(sc), u32(want[2])) and np.array_equal(ids, want[3])
        return
    x, mag = F.eff64(q)
    s = (x @ dec.astype(np.float64).T) * scales[None, :]
    b = (F.beta(3 * d) * (1 + 2.0 ** -24) + 2.0 ** -24) * (mag @ np.abs(dec).astype(np.float64).T) * scales[None, :]
    nl = min(k, int(live.sum()))
    for a in range(nq):
        got = ids[a, :nl]
        assert (ids[a, nl:] == -1).all() and live[got].all() and len(set(got.tolist())) == nl, a
        assert (np.abs(sc[a, :nl].astype(np.float64) - s[a, got]) <= b[a, got]).all(), a
        rest = live.copy()
        rest[got] = False  # a live row left out scored no more than the last one returned
        assert ((s[a] - b[a])[rest] <= float(sc[a, nl - 1])).all() and (np.diff(sc[a, :nl]) <= 0).all(), a


def test_every_finite_code_against_power_of_two_queries_exactly():
    """A query of +-2^e with one e: every partial sum is a multiple of 2^(e-9) below 32 * 448 * 2^e, 23 bits, so exact."""
    n, d = 254, 32
    codes = FINITE[(np.arange(n)[:, None] + np.arange(d)[None, :] * 8) % 254]
    rng = np.random.default_rng(0)
    q = (rng.choice([-1.0, 1.0], (5, d)) * 2.0 ** np.array([-7, -3, 0, 1, 5])[:, None]).astype(np.float32)
    scales = (2.0 ** (np.arange(n) % 3 - 1)).astype(np.float32)
    rs, rm, sc, ids = launch(codes, scales, q, 128, np.ones(n, bool))
    assert (rs, rm) == (0, 0) and set(np.unique(codes)) == set(FINITE)
    dots = (q.astype(np.float64) @ S.e4m3_to_f32(codes).astype(np.float64).T) * scales[None, :] + 0.0
    for a in range(5):
        assert np.array_equal(ids[a], np.lexsort((np.arange(n), -dots[a]))[:128]) and np.array_equal(u32(sc[a]), u32(dots[a, ids[a]])), a


def test_dead_rows_of_nan_codes_and_nan_scales_change_nothing_and_replays_are_bitwise_equal():
    codes, q, rng = make(600, 96, 69, 3)
    scales = rng.uniform(0.5, 2.0, 600).astype(np.float32)
    live = F.live_pattern("dead_group", 600)
    live[[5, 597]] = False  # dead rows inside live groups, one in the last (partial) tile
    clean = launch(codes, scales, q, 10, live)
    assert clean[:2] == (0, 0)
    for _ in range(20):
        again = launch(codes, scales, q, 10, live, poison=True)
        assert again[:2] == (0, 0) and np.array_equal(u32(again[2]), u32(clean[2])) and np.array_equal(again[3], clean[3])


def rescore53(d=96, tweak=None):
    """Kinds 34 + 32 over every row (n <= 128 = k), then kind 53 over R = 40 -> (.., {(q, id): kind 34's score bits})."""
    n, Q, R, k = 100, 5, 40, 10
    codes, q, rng = make(n, d, Q, d)
    scales = rng.uniform(0.001, 3.0, n).astype(np.float32)
    in_id = np.stack([rng.permutation(n)[:R] for _ in range(Q)]).astype(np.int32)
    in_id[:, -3:], in_id[1, 0], in_id[2, 1], in_id[0, :] = -1, n, 2 ** 31 - 1, -1  # empty slots, ids outside [0, N), no candidate
    in_sc = rng.standard_normal((Q, R)).astype(np.float32)
    t = {name: torch.from_numpy(a).to(DEV) for name, a in dict(codes=codes, sc=scales, q=q, id=in_id, s1=in_sc).items()}
    lv = torch.from_numpy(S.pack_live(np.ones(n, bool)).view(np.int32)).to(DEV)
    cand = torch.zeros(OS.scratch_bytes(n, Q, 128) // 8, dtype=torch.int64, device=DEV)
    fs, fi = torch.zeros((Q, 128), device=DEV), torch.zeros((Q, 128), dtype=torch.int32, device=DEV)
    qp = OS.QuantScanParams(t["codes"].data_ptr(), t["q"].data_ptr(), cand.data_ptr(), fs.data_ptr(), fi.data_ptr(), n, d, Q, 128, d, 0,
                            cand.numel() * 8, lv.data_ptr(), 0, 0, lv.numel() * 4, t["sc"].data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    assert OS.launch_quant(qp, st) == (0, 0)
    os_, oi = torch.full((Q, k + 1), 7.0, device=DEV), torch.full((Q, k + 1), -7, dtype=torch.int32, device=DEV)
    ol = torch.full((Q,), 7.0, device=DEV)
    rp = OS.QuantRescoreParams(t["codes"].data_ptr(), t["sc"].data_ptr(), t["q"].data_ptr(), t["id"].data_ptr(), t["s1"].data_ptr(),
                               os_.data_ptr(), oi.data_ptr(), ol.data_ptr(), n, d, Q, R, k, d)
    if tweak:
        tweak(rp)
    rc = OS.launch_quant_rescore(rp, st)
    torch.cuda.synchronize()
    sc, ids, last = os_.cpu().numpy().ravel(), oi.cpu().numpy().ravel(), ol.cpu().numpy()
    if rc != 0:
        assert (sc == 7.0).all() and (ids == -7).all() and (last == 7.0).all()  # refused: nothing ran
    assert (sc[Q * k:] == 7.0).all() and (ids[Q * k:] == -7).all()  # the outputs are [Q][k], packed
    full = {(a, int(i)): int(b) for a in range(Q) for i, b in zip(fi.cpu().numpy()[a], u32(fs.cpu().numpy())[a]) if i >= 0}
    return rc, sc[:Q * k].reshape(Q, k), ids[:Q * k].reshape(Q, k), last, in_id, in_sc, full


@pytest.mark.parametrize("d", [96, 1040])  # one chunk per lane; two, the second partial
def test_kind_53_gives_kind_34s_bits_and_the_order_rule(d):
    rc, sc, ids, last, in_id, in_sc, full = rescore53(d)
    assert rc == 0 and np.array_equal(u32(last), u32(in_sc[:, -1])) and (ids[0] == -1).all() and np.isneginf(sc[0]).all()
    for a in range(1, ids.shape[0]):
        cand = in_id[a][(in_id[a] >= 0) & (in_id[a] < 100)]
        bits = np.array([full[a, int(i)] for i in cand], np.uint32)
        order = np.lexsort((cand, -bits.view(np.float32).astype(np.float64)))[:ids.shape[1]]
        assert np.array_equal(ids[a], cand[order]) and np.array_equal(u32(sc[a]), bits[order]), a


POINTERS = ("codes", "queries", "live", "cand", "scales", "in_id", "in_score", "out_score", "out_id", "out_last")
REFUSALS = [  # -165 .. -178: kind 52 at N = 300, D = 128, Q = 3, k = 10; -179 .. -185: kind 53 (rescore53's shape)
    (-165, dict(codes=0)), (-165, dict(queries=0)), (-165, dict(live=0)), (-165, dict(cand=0)), (-166, dict(D=144, ldc=144)),
    (-167, dict(D=0)), (-168, dict(D=2080, ldc=2080)), (-169, dict(ldc=96)), (-169, dict(ldc=136)), (-170, dict(N=0)),
    (-171, dict(Q=0)), (-172, dict(k=0)), (-172, dict(k=129, cand_bytes=2 ** 40)), (-173, dict(codes=8)), (-173, dict(cand=4)),
    (-173, dict(live=2)), (-174, dict(live_bytes=4 * ((300 + 31) // 32) - 1)), (-175, dict(cand_bytes=2 * 3 * 10 * 8 - 1)),
    (-176, dict(queries=4)), (-177, dict(scales=0)), (-177, dict(scales=2)), (-178, dict(scales_bytes=4 * 300 - 1)),
    (-179, dict(D=104)), (-179, dict(D=2064, ldc=2064)), (-179, dict(ldc=80)), (-179, dict(ldc=104)), (-180, dict(N=0)),
    (-181, dict(Q=0)), (-182, dict(R=0)), (-182, dict(R=129)), (-183, dict(k=0)), (-183, dict(k=41)), (-184, dict(scales=0)),
    (-184, dict(in_score=0)), (-184, dict(out_last=0)), (-185, dict(codes=8)), (-185, dict(scales=2)), (-185, dict(out_last=2)),
]


@pytest.mark.parametrize("code,kw", REFUSALS)
def test_every_refusal_launches_nothing(code, kw):
    """Pointer cases ADD the value to the real address (0 replaces it); the helpers assert the canaries after a refusal."""
    def tweak(p):
        for name, v in kw.items():
            setattr(p, name, (getattr(p, name) + v if v else 0) if name in POINTERS else v)
    if code <= -179:
        assert rescore53(tweak=tweak)[0] == code
    else:
        codes, q, rng = make(300, 128, 3, 6)
        rs, rm, sc, ids = launch(codes, np.ones(300, np.float32), q, 10, np.ones(300, bool), tweak=tweak)
        assert rs == code and rm is None
    assert {c for c, _ in REFUSALS} == set(range(-185, -164))  # every code has a case
