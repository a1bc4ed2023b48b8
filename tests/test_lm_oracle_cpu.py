"""The oracles of tests/lm_oracle.py, judged on the CPU on exactly the inputs tests/test_lm_kernels_gpu.py
runs: anchored to independent code (``torch.nn.LSTMCell`` and one step of the eager AWD-LSTM, both in
fp64), every planted fault outside the bound at every case while the same math in fp32 stays inside, and
the host geometry functions of the library."""
import ctypes

import numpy as np
import pytest
import torch

import lm_oracle as O
from hipzap import _native as N
from hipzap.engine.lm import pack_awd_lstm
from hipzap.models.awd_lstm import get_language_model

CELL, XC, DEC, HH, SAMP = O.cell_cases(), O.x_cases(), O.dec_cases(), O.hh_cases(), O.sampler_cases()
ids = lambda cs: [s.id for s in cs]  # noqa: E731


def _close(a, b, what):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    rel = float((a - b).abs().max() / b.abs().max())
    assert rel < 1e-12, (what, rel)


# ------------------------------------------------------------------------------------------------
# anchors
@pytest.mark.parametrize("s", [s for s in CELL if s.id.endswith("-plain")], ids=lambda s: s.id)
@pytest.mark.parametrize("par", [0, 1])
def test_cell_ref_is_torch_lstmcell(s, par):
    c = O.build(s)
    cell = torch.nn.LSTMCell(c.In, c.H).double()
    with torch.no_grad():
        cell.weight_ih.copy_(c.w_ih)
        cell.weight_hh.copy_(c.w_hh)
        cell.bias_ih.copy_(c.b)
        cell.bias_hh.zero_()
        h, cc = cell(c.x_state[par ^ 1].double()[None], (c.h_state[par].double()[None], c.c_state[par].double()[None]))
    ref = O.cell_oracle(c, par)
    _close(ref["h"].ref, h[0], c.id + " h")
    _close(ref["c"].ref, cc[0], c.id + " c")


@pytest.mark.parametrize("tied", [True, False])
def test_oracles_are_one_step_of_the_eager_model(tied):
    """get_language_model in double, from the state dict the packer reads: cell_ref per layer, decoder_ref."""
    torch.manual_seed(3)
    V, E, NH, L = 41, 24, 37, 3
    m = get_language_model(V, E, NH, L, pad_token=1, tie_weights=tied).eval()
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.to(torch.bfloat16).float())  # biases too: b_ih + b_hh is then exact in fp32
        if m[1].decoder.bias is not None:
            m[1].decoder.bias.normal_()
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    pk = pack_awd_lstm(sd, "cpu", split=False)
    md = get_language_model(V, E, NH, L, pad_token=1, tie_weights=tied).double().eval()
    md.load_state_dict({k: v.double() for k, v in sd.items()})
    g = torch.Generator().manual_seed(5)
    states = [(torch.randn(2, ly["H"], generator=g), torch.randn(2, ly["H"], generator=g)) for ly in pk["layers"]]
    par, tok = 1, 17
    md[0].hidden = [(h[par].double()[None, None], c[par].double()[None, None]) for h, c in states]
    with torch.no_grad():
        logits, raw, _ = md(torch.tensor([[tok]]))
    x = pk["emb"][tok, :E].double()
    for l, (ly, (h, c)) in enumerate(zip(pk["layers"], states)):
        ref = O.cell_ref(ly["w"], ly["bias"], h, c, par, ly["In"], ly["H"], x=x)
        _close(ref["h"].ref, raw[l][0, 0], f"layer {l} h")
        _close(ref["c"].ref, md[0].hidden[l][1][0, 0], f"layer {l} c")
        x = ref["h"].ref
    hs = torch.zeros(2, E, dtype=torch.float64)
    hs[par ^ 1] = x
    dec = O.decoder_ref(pk["dec"], pk["dec_bias"], hs, par, V, E)
    _close(dec.ref, logits[0], "logits")


def test_x_cell_and_hh_compose_to_the_classic_cell():
    """split mode is the same cell: W_ih x + (W_hh h + b) through hh_ref and x_cell_ref = cell_ref."""
    c = O.cell_case(300, 301)
    for par in (0, 1):
        K = c.In + c.H
        w_hh = O.pack_rows(c.w[:, c.In:K].float(), O._pad_to(c.H, 64))
        hs = torch.stack([c.h_state[1], c.h_state[0]])  # hh_rows reads par ^ 1: the state before this step
        pre = O.hh_ref([w_hh], [c.bias], [hs], par, [c.H])[0].ref
        got = O.x_cell_ref(c.w[:, :O._pad_to(c.In, 64)], pre, c.h_state, c.c_state, par, c.In, c.H, x_state=c.x_state)
        ref = O.cell_oracle(c, par)
        _close(got["h"].ref, ref["h"].ref, "h")
        _close(got["c"].ref, ref["c"].ref, "c")


def test_gumbel_np_matches_a_scalar_philox():
    def philox(c, k):
        c, k = list(c), list(k)
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
            k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
        return c
    seed, t = O.DEC_SEED, 5
    got = O.gumbel_np(seed, t, 11)
    for j in range(11):
        r = philox([j >> 2, t, 0x5EED, 0], [seed & 0xFFFFFFFF, seed >> 32])[j & 3]
        assert got[j] == -np.log(-np.log(((r >> 9) + 0.5) / 8388608.0))
    assert np.isfinite(O.gumbel_bound(seed, t, 4000)).all()


def test_gumbel_uniform_is_exact_in_fp32_and_inside_the_unit_interval():
    """common.h gumbel_of's u in float32 arithmetic, as the device forms it, at the extreme random words
    (all ones: the k at which 24 bits gave u == 1.0f and a key of +inf), around the point where k + 0.5f
    stops being exact with 24 bits, and on a stride through every k: the float64 value, bit for bit, inside
    [2**-24, 1 - 2**-24], and a finite noise with a finite bound."""
    edge = np.array([0, 1, 0x1FF, 0x200, 0x7FFFFFFF, 0x80000000, 0x800001FF, 0xFFFFFDFF, 0xFFFFFE00, 0xFFFFFFFF], np.uint64)
    r = np.concatenate([edge, np.arange(0, 1 << 32, 0x10001, dtype=np.uint64)])
    u32, u64 = O.uniform_of(r, np.float32), O.uniform_of(r)
    assert u32.dtype == np.float32 and np.array_equal(u32.astype(np.float64), u64)
    assert u64.min() == 2.0 ** -24 and u64.max() == 1 - 2.0 ** -24 and u32.max() < np.float32(1)
    g, b = O.gumbel_of(r), O.gumbel_bound_of(r)
    assert np.isfinite(g).all() and np.isfinite(b).all() and b.max() < 1e-5
    assert abs(g[len(edge) - 1] - 16.6355) < 1e-3 and abs(g[0] + 2.8115) < 1e-3
    old = (np.float32(0xFFFFFFFF >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)  # what 24 bits gave
    assert old == np.float32(1)


# ------------------------------------------------------------------------------------------------
# planted faults: outside the bound; the same math in fp32: inside
def _judge(cid, oracle, hooks, pars=(0, 1)):
    worst = 0.0
    for par in pars:
        ref = oracle(par)
        f32 = oracle(par, dtype=torch.float32)
        for name in _names(ref):
            rep = O.compare(_get(f32, name).ref, _get(ref, name))
            assert rep.ok, O.describe(f"{cid} par {par} {name} in fp32", rep)
            worst = max(worst, rep.ratio)
        for hk in hooks:
            bad = oracle(par, hooks={hk: True})
            assert any(not O.compare(_get(bad, n).ref, _get(ref, n)).ok for n in _names(ref)), \
                f"{cid} par {par}: planted fault {hk} stays inside the bound"
    print(f"{cid}: fp32 worst err/bound {worst:.3g}; {len(hooks)} planted faults all outside")


def _names(ref):
    return list(ref) if isinstance(ref, dict) else list(range(len(ref))) if isinstance(ref, list) else [None]


def _get(ref, name):
    return ref if name is None else ref[name]


@pytest.mark.parametrize("s", CELL, ids=ids(CELL))
def test_cell_faults(s):
    c = O.build(s)
    _judge(c.id, lambda par, **kw: O.cell_oracle(c, par, **kw), c.hooks)


@pytest.mark.parametrize("s", XC, ids=ids(XC))
def test_x_cell_faults(s):
    c = O.build(s)
    _judge(c.id, lambda par, **kw: O.x_oracle(c, par, **kw), c.hooks)


@pytest.mark.parametrize("s", DEC, ids=ids(DEC))
def test_decoder_faults(s):
    c = O.build(s)
    _judge(c.id, lambda par, **kw: O.dec_oracle(c, par, **kw), c.hooks)


@pytest.mark.parametrize("s", HH, ids=ids(HH))
def test_hh_faults(s):
    c = O.build(s)
    _judge(c.id, lambda par, **kw: O.hh_oracle(c, par, **kw), c.hooks)


@pytest.mark.parametrize("s", [s for s in DEC if not s.id.endswith("-exact")], ids=lambda s: s.id)
def test_keys_bound_bites(s):
    """a key moved by a thousandth, or the noise of the neighbouring row or step, leaves the keys bound"""
    c = O.build(s)
    lg = O.dec_oracle(c, 0)
    ref = O.keys_ref(lg, O.DEC_SEED, 3)
    f32 = (O.dec_oracle(c, 0, dtype=torch.float32).ref + torch.from_numpy(O.gumbel_np(O.DEC_SEED, 3, c.V)).float())
    assert O.compare(f32, ref).ok
    assert not O.compare(ref.ref + 1e-3, ref).ok
    assert not O.compare(O.keys_ref(lg, O.DEC_SEED, 4).ref, ref).ok
    assert not O.compare(O.keys_ref(lg, O.DEC_SEED + 1, 3).ref, ref).ok


@pytest.mark.parametrize("s", SAMP, ids=ids(SAMP))
def test_sampler_faults(s):
    c = O.build(s)
    draws, tok, mx = O.sampler_oracle(c)
    assert draws == sorted(range(c.V), key=lambda r: (-float(c.keys[r]), r))[:10]
    assert tok == O.token_from_maxima(*mx, c.V) or all(d == 0 or d in c.exclude for d in draws)
    if all(d == 0 or d in c.exclude for d in draws) and c.V <= 9:
        assert tok == draws[0] == O.token_from_maxima(*mx, c.V)  # the fallback: the first draw
    for hk in c.hooks:
        d2, t2, m2 = O.sampler_oracle(c, hooks={hk: True})
        assert d2 != draws or t2 != tok or any(not np.array_equal(a, b) for a, b in zip(mx, m2)), \
            f"{c.id}: planted fault {hk} changes nothing"


def test_fused_token_cases():
    for c in (O.build(s) for s in CELL if "-fused" in s.id or "-emb" in s.id):
        if c.form == "emb":  # the maxima passed with a forced token name another one
            assert O.token_from_maxima(c.bmax_val, c.bmax_idx, c.bacc_val, c.bacc_idx, c.V) == c.V - 1 - c.tok != c.tok
        if c.form == "fused":
            assert 0 <= c.tok < c.V
            if c.nblk > 256 and not c.fallback:
                assert c.tok == 1200  # equal maxima in two per-thread slots: the lower row
            if c.fallback:
                assert c.tok == int(c.bmax_idx[np.argmax(c.bmax_val)])


# ------------------------------------------------------------------------------------------------
# host geometry of the library
GEOM_V = [1, 7, 9, 10, 11, 31, 32, 33, 8191, 8192, 8193, 60000]


@pytest.mark.skipif(not N.available(), reason="native library not built")
@pytest.mark.parametrize("V", GEOM_V)
def test_geometry(V):
    lib = N.lib()
    nblk, rpb = ctypes.c_int(), ctypes.c_int()
    lib.hz_decoder_geometry(V, ctypes.byref(nblk), ctypes.byref(rpb))
    assert nblk.value * rpb.value >= V and rpb.value % 8 == 0 and 1 <= nblk.value <= 2048
    assert (nblk.value - 1) * rpb.value < V  # no empty workgroup
    assert (nblk.value, rpb.value) == O.decoder_geometry(V)
    nb = lib.hz_lmb_dec_blocks(V)  # csrc/lmbatch.hip: workgroups of 256 vocabulary rows (DROWS)
    assert nb * 256 >= V and 1 <= nb <= 2048
