"""The single-request AWD-LSTM decode kernels of csrc/lstm.hip, each launched alone on MI355X from prepared
device buffers against the fp64 oracle of the same op (tests/lm_oracle.py), element by element under the
derived bounds: ``lstm_cell_kernel<NCH, 2>`` for NCH 1..6 (classic, layer-0 and fused-sampler forms),
``lstm_x_kernel<NCH, false>`` for NCH 1..6 and ``<NCH, true>`` for NCH 1..3, ``decoder_kernel<NCH, 4, *>`` for
NCH 1..4 with and without bias and keys, ``hh_rows`` for 2 and 4 layers, both samplers on host-made keys,
and the parameters the launchers must reject.

Every launch runs at t = step + step_off in {0, 1, 3, 4} (both parities, both offsets). What the kernel
writes sits between guard words; the half of the state it writes and every half it does not read are NaN
before the launch. After it: the written half inside the bound and finite, everything else bitwise as it
was. The inputs and references are those tests/test_lm_oracle_cpu.py judges on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import lm_oracle as O
from hipzap import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64            # words on either side of a written buffer (keeps 256-B alignment)
PATTERN = 0x5EADBEE5  # the guard word (as fp32: 2.1e19, as int32: far outside every id)
STEPS = [(0, 0), (1, 0), (0, 3), (1, 3)]  # (device step, step_off)
NAN = float("nan")


class Buf:
    """A device buffer of 4-byte words inside a larger allocation with a guard pattern on both sides."""

    def __init__(self, data, dtype=torch.float32):
        data = torch.as_tensor(data).to(dtype).contiguous()
        self.shape, self.dtype, self.n = data.shape, dtype, data.numel()
        self.raw = torch.full((self.n + 2 * GUARD,), PATTERN, dtype=torch.int32, device=DEV)
        self.set(data)

    def set(self, data):
        self.raw[GUARD:GUARD + self.n] = torch.as_tensor(data).to(self.dtype).contiguous().reshape(-1).view(torch.int32).to(DEV)
        self.before = self.raw.cpu().clone()

    @property
    def ptr(self):
        return self.raw.data_ptr() + 4 * GUARD

    def get(self):
        """the data after a launch; the guards must be intact"""
        r = self.raw.cpu()
        assert (r[:GUARD] == PATTERN).all() and (r[-GUARD:] == PATTERN).all(), "guard words overwritten"
        self.after = r
        return r[GUARD:GUARD + self.n].view(self.dtype).reshape(self.shape).clone()

    def unchanged(self, what, sel=None):
        """bitwise as before the launch (``sel``: an index into the data, default all of it)"""
        a = self.raw.cpu()[GUARD:GUARD + self.n].reshape(self.shape)
        b = self.before[GUARD:GUARD + self.n].reshape(self.shape)
        if sel is not None:
            a, b = a[sel], b[sel]
        assert torch.equal(a, b), f"{what} was written"


def _dev(t):
    return t.contiguous().to(DEV)


def _half_nan(state, half):
    s = state.clone()
    s[half] = NAN
    return s


def _ints(a):
    return torch.as_tensor(np.asarray(a)).to(torch.int32)


def _sync_launch(fn, prm, what):
    N.check(fn(ctypes.byref(prm), N.stream_ptr()), what)
    torch.cuda.synchronize()


def _check_state(what, buf, ref, par):
    """the written half (par ^ 1) against the oracle, the other half untouched"""
    got = buf.get()
    assert torch.isfinite(got[par ^ 1]).all(), f"{what}: not finite"
    rep = O.check(what, got[par ^ 1], ref)
    buf.unchanged(f"{what}: the input parity half", par)
    return rep.ratio


# ------------------------------------------------------------------------------------------------
# lstm_cell_kernel
@pytest.mark.parametrize("s", O.cell_cases(), ids=lambda s: s.id)
def test_lstm_cell(s):
    c = O.build(s)
    lib = N.lib()
    w, bias = _dev(c.w), _dev(c.bias)
    emb = _dev(c.emb) if c.form != "plain" else None
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    n_forced = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = 0.0
    for s0, off in STEPS:
        t = s0 + off
        par = t & 1
        step.fill_(s0)
        h = Buf(_half_nan(c.h_state, par ^ 1))
        cs = Buf(_half_nan(c.c_state, par ^ 1))
        toks = torch.full((8,), 7, dtype=torch.int32)
        prm = N.LstmParams()
        prm.w, prm.bias, prm.h_state, prm.c_state, prm.step = w.data_ptr(), bias.data_ptr(), h.ptr, cs.ptr, step.data_ptr()
        prm.In, prm.H, prm.ldk, prm.step_off = c.In, c.H, c.ldk, off
        keep = [h, cs]
        if c.form == "plain":
            x = _dev(_half_nan(c.x_state, par))  # the previous layer's input parity half is not read
            prm.x_state = x.data_ptr()
        else:  # both layer-0 forms get the decoder maxima: t < n_forced takes tok_seq[t], t >= n_forced the maxima
            prm.emb, prm.lde = emb.data_ptr(), c.lde
            if c.form == "emb":
                toks[t] = c.tok
            n_forced.fill_(t + 1 if c.form == "emb" else t)
            mx = [Buf(c.bmax_val), Buf(_ints(c.bmax_idx), torch.int32), Buf(c.bacc_val), Buf(_ints(c.bacc_idx), torch.int32)]
            prm.bmax_val, prm.bmax_idx, prm.bacc_val, prm.bacc_idx = (b.ptr for b in mx)
            prm.nblk, prm.V, prm.n_forced = c.nblk, c.V, n_forced.data_ptr()
            keep += mx
        tok_seq = Buf(toks, torch.int32)
        prm.tok_seq = tok_seq.ptr
        _sync_launch(lib.hz_lstm_cell_launch, prm, c.id)
        ref = O.cell_oracle(c, par)
        worst = max(worst, _check_state(f"{c.id} t={t} h", h, ref["h"], par), _check_state(f"{c.id} t={t} c", cs, ref["c"], par))
        got_toks = tok_seq.get()
        for b in keep[2:]:
            b.get()
            b.unchanged(f"{c.id}: the decoder maxima")
        if c.form == "fused":
            assert int(got_toks[t]) == c.tok, (c.id, t, int(got_toks[t]), c.tok)
            got_toks[t] = 7
            assert (got_toks == 7).all(), "other tokens written"
        else:
            tok_seq.unchanged(f"{c.id}: tok_seq")
    print(f"{c.id}: lstm_cell_kernel<{c.nch}, 2> worst err/bound {worst:.3g}")


# ------------------------------------------------------------------------------------------------
# lstm_x_kernel
@pytest.mark.parametrize("s", O.x_cases(), ids=lambda s: s.id)
def test_lstm_x(s):
    c = O.build(s)
    lib = N.lib()
    w, pre = _dev(c.w), _dev(c.pre)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    n_forced = torch.zeros(1, dtype=torch.int32, device=DEV)
    if c.fold:
        xtab, pre0 = _dev(c.xtab), _dev(c.pre0)
    worst = 0.0
    for s0, off in STEPS:
        t = s0 + off
        par = t & 1
        step.fill_(s0)
        h = Buf(_half_nan(c.h_state, par ^ 1))
        cs = Buf(_half_nan(c.c_state, par ^ 1))
        toks = torch.full((8,), 7, dtype=torch.int32)
        prm = N.LstmParams()
        prm.w, prm.pre, prm.h_state, prm.c_state, prm.step = w.data_ptr(), pre.data_ptr(), h.ptr, cs.ptr, step.data_ptr()
        prm.In, prm.H, prm.ldk, prm.step_off = c.In, c.H, c.ldk, off
        mx = []
        if c.fold:
            h0 = Buf(torch.full_like(c.h0_state, NAN))  # never read: the kernel rebuilds h0 from xtab + pre0
            c0 = Buf(_half_nan(c.c0_state, par ^ 1))
            prm.xtab, prm.pre0, prm.h0_state, prm.c0_state, prm.H0 = xtab.data_ptr(), pre0.data_ptr(), h0.ptr, c0.ptr, c.In
            if not c.fused:
                toks[t] = c.tok
            n_forced.fill_(t if c.fused else t + 1)  # either side of ``t >= n_forced``, the maxima always passed
            mx = [Buf(c.bmax_val), Buf(_ints(c.bmax_idx), torch.int32), Buf(c.bacc_val), Buf(_ints(c.bacc_idx), torch.int32)]
            prm.bmax_val, prm.bmax_idx, prm.bacc_val, prm.bacc_idx = (b.ptr for b in mx)
            prm.nblk, prm.V, prm.n_forced = c.nblk, c.V, n_forced.data_ptr()
        else:
            x = _dev(_half_nan(c.x_state, par))
            prm.x_state = x.data_ptr()
        tok_seq = Buf(toks, torch.int32)
        prm.tok_seq = tok_seq.ptr
        _sync_launch(lib.hz_lstm_cell_launch, prm, c.id)
        ref = O.x_oracle(c, par)
        worst = max(worst, _check_state(f"{c.id} t={t} h", h, ref["h"], par), _check_state(f"{c.id} t={t} c", cs, ref["c"], par))
        if c.fold:
            worst = max(worst, _check_state(f"{c.id} t={t} h0", h0, ref["h0"], par),
                        _check_state(f"{c.id} t={t} c0", c0, ref["c0"], par))
        got_toks = tok_seq.get()
        for b in mx:
            b.get()
            b.unchanged(f"{c.id}: the decoder maxima")
        if c.fold and c.fused:
            assert int(got_toks[t]) == c.tok
            got_toks[t] = 7
            assert (got_toks == 7).all(), "other tokens written"
        else:
            tok_seq.unchanged(f"{c.id}: tok_seq")
    print(f"{c.id}: lstm_x_kernel<{c.nch}, {'true' if c.fold else 'false'}> worst err/bound {worst:.3g}")


# ------------------------------------------------------------------------------------------------
# decoder_kernel
EXCLUDES = [[], [3], [1, 2, 3, 4, 5, 6, 30, 32], [0, 5, 6, 7, 8, 9, 10, 11]]  # 0, 1 and 8 ids


class Decoder:
    """One decoder case on the device; ``run`` launches once and returns what was written."""

    def __init__(self, c, hh=None):
        self.c, self.hh = c, hh
        self.w = _dev(c.w)
        self.bias = _dev(c.bias) if c.bias is not None else None
        self.step = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.seed = torch.full((1,), O.DEC_SEED, dtype=torch.int64, device=DEV)
        if hh is not None:
            self.hw, self.hb = [_dev(w) for w in hh.ws], [_dev(b) for b in hh.biases]

    def run(self, s, off, keys=False, exclude=(), n_hh=0):
        c = self.c
        t = s + off
        par = t & 1
        self.step.fill_(s)
        h = _dev(_half_nan(c.h_state, par))  # the decoder reads this step's output half only
        o = {k: Buf(torch.zeros(n), dt) for k, n, dt in
             [("logits", c.V, torch.float32), ("keys", c.V, torch.float32), ("bmax_val", c.nblk, torch.float32),
              ("bmax_idx", c.nblk, torch.int32), ("bacc_val", c.nblk, torch.float32), ("bacc_idx", c.nblk, torch.int32)]}
        p = N.DecoderParams()
        p.w, p.bias, p.h_state, p.step, p.step_off = self.w.data_ptr(), N.ptr(self.bias), h.data_ptr(), self.step.data_ptr(), off
        p.logits, p.V, p.H, p.ldk, p.nblk, p.rpb = o["logits"].ptr, c.V, c.H, c.ldk, c.nblk, c.rpb
        if keys:
            p.keys, p.seed = o["keys"].ptr, self.seed.data_ptr()
            p.bmax_val, p.bmax_idx, p.bacc_val, p.bacc_idx = (o[k].ptr for k in ("bmax_val", "bmax_idx", "bacc_val", "bacc_idx"))
            p.n_exclude = len(exclude)
            for i, e in enumerate(exclude):
                p.exclude[i] = e
        hh_out = []
        if n_hh:
            hh = self.hh
            hs = [_dev(_half_nan(x, par)) for x in hh.h_states]
            p.n_hh, p.hh_blocks = n_hh, hh.blk[n_hh]
            for l in range(n_hh):
                hh_out.append(Buf(torch.full((4 * hh.Hs[l],), NAN)))
                p.hh_w[l], p.hh_b[l], p.hh_h[l], p.hh_out[l] = self.hw[l].data_ptr(), self.hb[l].data_ptr(), hs[l].data_ptr(), hh_out[l].ptr
                p.hh_H[l], p.hh_ld[l], p.hh_blk[l] = hh.Hs[l], hh.lds[l], hh.blk[l]
            p.hh_blk[n_hh] = hh.blk[n_hh]
        _sync_launch(N.lib().hz_decoder_launch, p, c.id)
        res = {k: b.get() for k, b in o.items()}
        if not keys:
            for k in ("keys", "bmax_val", "bmax_idx", "bacc_val", "bacc_idx"):
                o[k].unchanged(f"{c.id}: {k} without keys")
        res["hh"] = [b.get() for b in hh_out]
        return res, par, t


def _check_logits(c, got, par, what):
    ref = O.dec_oracle(c, par)
    assert torch.isfinite(got).all()
    if c.exact:
        assert torch.equal(got, ref.ref.float()), f"{what}: integer logits not exact"
        return 0.0
    return O.check(what, got, ref).ratio


@pytest.mark.parametrize("s", O.dec_cases(), ids=lambda s: s.id)
def test_decoder(s):
    c = O.build(s)
    d = Decoder(c)
    worst = worst_k = 0.0
    for (s0, off), ex in zip(STEPS, EXCLUDES):
        ex = [e for e in ex if e < max(c.V, 2)]
        plain, par, t = d.run(s0, off)
        worst = max(worst, _check_logits(c, plain["logits"], par, f"{c.id} t={t} logits"))
        r, _, _ = d.run(s0, off, keys=True, exclude=ex)
        assert torch.equal(r["logits"].view(torch.int32), plain["logits"].view(torch.int32)), "logits differ with keys"
        if not c.exact:
            worst_k = max(worst_k, O.check(f"{c.id} t={t} keys", r["keys"], O.keys_ref(O.dec_oracle(c, par), O.DEC_SEED, t)).ratio)
        mx = O.block_maxima(r["keys"].numpy(), c.nblk, c.rpb, ex)  # from the kernel's own keys: exact
        for name, want in zip(("bmax_val", "bmax_idx", "bacc_val", "bacc_idx"), mx):
            assert np.array_equal(r[name].numpy(), want), (c.id, t, name, ex)
    print(f"{c.id}: decoder_kernel<{c.nch}, 4, 0> worst err/bound logits {worst:.3g} keys {worst_k:.3g}")


@pytest.mark.parametrize("s", O.hh_cases(), ids=lambda s: s.id)
def test_decoder_hh_rows(s):
    c = O.build(s)
    d = Decoder(c.dec, c)
    worst = 0.0
    for s0, off in STEPS:
        plain, par, t = d.run(s0, off)
        r, _, _ = d.run(s0, off, n_hh=c.n)
        assert torch.equal(r["logits"].view(torch.int32), plain["logits"].view(torch.int32)), "logits differ with hh_rows"
        _check_logits(c.dec, r["logits"], par, f"{c.id} t={t} logits")
        for l, (got, ref) in enumerate(zip(r["hh"], O.hh_oracle(c, par))):
            assert torch.isfinite(got).all()
            if c.exact:
                assert torch.equal(got, ref.ref.float()), f"{c.id} layer {l}: integer partials not exact"
            else:
                worst = max(worst, O.check(f"{c.id} t={t} hh_out[{l}]", got, ref).ratio)
    print(f"{c.id}: decoder_kernel<1, 4, 3> hh_rows x{c.n} worst err/bound {worst:.3g}")


# ------------------------------------------------------------------------------------------------
# samplers
@pytest.mark.parametrize("s", O.sampler_cases(), ids=lambda s: s.id)
def test_samplers(s):
    c = O.build(s)
    draws_ref, tok_ref, mx = O.sampler_oracle(c)
    keys = _dev(torch.from_numpy(c.keys))
    dmx = [_dev(torch.from_numpy(a)) for a in mx]
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    n_forced = torch.zeros(1, dtype=torch.int32, device=DEV)
    for s0, off in STEPS[1:3]:
        t = s0 + off
        step.fill_(s0)
        for tournament in (True, False):
            tok_seq = Buf(torch.full((8,), -5), torch.int32)
            draws = Buf(torch.full((6, 10), -5), torch.int32)
            p = N.SamplerParams()
            p.keys, p.tok_seq, p.step, p.step_off, p.n_forced = keys.data_ptr(), tok_seq.ptr, step.data_ptr(), off, n_forced.data_ptr()
            p.V, p.n_exclude, p.nblk, p.rpb = c.V, len(c.exclude), c.nblk, c.rpb
            for i, e in enumerate(c.exclude):
                p.exclude[i] = e
            p.bmax_val, p.bmax_idx, p.bacc_val, p.bacc_idx = (a.data_ptr() for a in dmx)
            p.draws = draws.ptr if tournament else 0
            _sync_launch(N.lib().hz_sampler_launch, p, c.id)
            toks, dr = tok_seq.get(), draws.get()
            assert int(toks[t + 1]) == tok_ref, (c.id, tournament, int(toks[t + 1]), tok_ref)
            toks[t + 1] = -5
            assert (toks == -5).all(), "other tokens written"
            if tournament:
                assert dr[t, :len(draws_ref)].tolist() == draws_ref, (c.id, dr[t].tolist(), draws_ref)
                dr[t] = -5
            assert (dr == -5).all(), "other draw rows written"


# ------------------------------------------------------------------------------------------------
# parameters the launchers reject (nothing is launched: each call returns non-zero)
def test_rejected_parameters():
    lib = N.lib()
    c = O.cell_case(37, 6)
    bufs = [_dev(c.w), _dev(c.bias), _dev(c.h_state), _dev(c.c_state), _dev(c.x_state), torch.zeros(1, dtype=torch.int32, device=DEV)]
    big = torch.zeros(1 << 16, device=DEV)  # every pointer of a rejected call still names real memory

    def lstm(**kw):
        p = N.LstmParams()
        p.w, p.bias, p.h_state, p.c_state, p.x_state, p.step = (b.data_ptr() for b in bufs)
        p.In, p.H, p.ldk = c.In, c.H, c.ldk
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.hz_lstm_cell_launch(ctypes.byref(p), N.stream_ptr())

    assert lstm(ldk=72) != 0            # ldk % 64
    assert lstm(ldk=0) != 0 and lstm(In=60, ldk=64) != 0  # ldk < In + H
    assert lstm(ldk=3136) != 0          # ldk > 3072
    assert lstm(pre=big.data_ptr(), ldk=3136) != 0 and lstm(pre=big.data_ptr(), ldk=72) != 0
    assert lstm(pre=big.data_ptr(), In=80, ldk=64) != 0
    d = O.dec_case(33, 96, 96)
    dw, db, dh = _dev(d.w), _dev(d.bias), _dev(d.h_state)

    def dec(**kw):
        p = N.DecoderParams()
        p.w, p.bias, p.h_state, p.step, p.logits = dw.data_ptr(), db.data_ptr(), dh.data_ptr(), bufs[5].data_ptr(), big.data_ptr()
        p.V, p.H, p.ldk, p.nblk, p.rpb = d.V, d.H, d.ldk, d.nblk, d.rpb
        for k, v in kw.items():
            if isinstance(v, dict):
                for i, e in v.items():
                    getattr(p, k)[i] = e
            else:
                setattr(p, k, v)
        return lib.hz_decoder_launch(ctypes.byref(p), N.stream_ptr())

    at = lambda words: big.data_ptr() + 4 * words  # noqa: E731  disjoint slices: logits at 0, then W, b, h, out
    hh_ok = dict(n_hh=1, hh_blocks=2, hh_w={0: at(4096)}, hh_b={0: at(8192)}, hh_h={0: at(12288)},
                 hh_out={0: at(16384)}, hh_H={0: 8}, hh_blk={0: 0, 1: 2})
    assert dec(H=95) != 0               # odd H
    assert dec(nblk=d.nblk + 1) != 0 and dec(rpb=d.rpb + 8) != 0
    assert dec(n_hh=5) != 0
    assert dec(**hh_ok, hh_ld={0: 1600}) != 0   # hh_ld > 1536
    assert dec(**hh_ok, hh_ld={0: 72}) != 0     # hh_ld % 64
    torch.cuda.synchronize()
    assert dec() == 0 and dec(**hh_ok, hh_ld={0: 64}) == 0  # the same parameters, valid: accepted
    torch.cuda.synchronize()
