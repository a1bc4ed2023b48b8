"""HZ_K_SEARCH_PQUPDATE (csrc/search.hip search_pqupdate_kernel) against ``pq_means_seq``, its contract in numpy, bit
for bit; the device-resident trainer (``hz_pq_train``) against ``pq_train(backend="f32", means="seq")``; the refusals."""
import numpy as np
import pytest
import torch

from hipzap import _native as N_
from hipzap import search as S
from hipzap.ops import search as OS

from search_pqtrain_cases import PATTERNS, make_codes, sentinels, u32, wide_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, B = OS.PQ_UPDATE_TILE, OS.PQ_UPDATE_BATCH
NAN_BITS, NEVER = 0x7FC0, -7  # what the rows' pitch and the rows past N hold; what the outputs hold before a launch
SHAPES = [(1, 16, 16), (255, 48, 16), (257, 1024, 16), (1000, 768, 96), (T - 1, 80, 16), (T, 80, 16), (T + 1, 80, 16),
          (B + 1, 80, 16)]


def update(x, codes, cb, ldr=None, ldc=None, in_place=False, tweak=None):
    """One launch over device copies -> (rc, codebook_out, counts). The buffers hold two rows more than N: rows of NaN
    with codes in range, and the pitch bytes of a code row are in range too, so reading either would show."""
    n, d = x.shape
    m = cb.shape[0]
    ldr, ldc = ldr or d, ldc or m
    rows = np.full((n + 2, ldr), NAN_BITS, np.uint16)
    rows[:n, :d] = S.to_bf16(x)
    cpad = np.full((n + 2, ldc), 3, np.uint8)
    cpad[:n, :m] = codes
    rd, cd = torch.from_numpy(rows.view(np.int16)).to(DEV), torch.from_numpy(cpad).to(DEV)
    src = torch.from_numpy(np.array(cb, np.float32)).to(DEV)
    out = src if in_place else torch.full_like(src, float(NEVER))
    cnt = torch.full((m, 256), NEVER, dtype=torch.int32, device=DEV)
    p = OS.PqUpdateParams(rd.data_ptr(), cd.data_ptr(), src.data_ptr(), out.data_ptr(), cnt.data_ptr(), n, d, m, ldr, ldc)
    if tweak:
        tweak(p)
    rc = OS.launch_pq_update(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n,d,m", SHAPES)
def test_the_kernel_equals_pq_means_seq_bit_for_bit(n, d, m, pattern):
    x, codes, cb = wide_rows(n, d, m), make_codes(pattern, n, m), sentinels(m, d // m)
    want, counts = S.pq_means_seq(x, codes, cb)
    assert np.array_equal(counts, np.stack([np.bincount(codes[:, j], minlength=256) for j in range(m)]))
    rc, got, cnt = update(x, codes, cb)
    assert rc == 0 and np.array_equal(u32(got), u32(want)) and np.array_equal(cnt, counts)


@pytest.mark.parametrize("kw", [dict(in_place=True), dict(ldr=88, ldc=32), dict(in_place=True, ldr=88, ldc=32)])
def test_in_place_and_padded_pitches_give_the_same_bits(kw):
    n, d, m = T + 1, 80, 16
    x, codes, cb = wide_rows(n, d, m), make_codes("uniform", n, m), sentinels(m, d // m)
    want, counts = S.pq_means_seq(x, codes, cb)
    rc, got, cnt = update(x, codes, cb, **kw)
    assert rc == 0 and np.array_equal(u32(got), u32(want)) and np.array_equal(cnt, counts)


@pytest.mark.parametrize("n,d,m,iters,init", [(100, 32, 16, 3, False), (300, 48, 16, 3, False), (2000, 768, 96, 2, False),
                                              (300, 48, 16, 3, True)])
def test_the_device_trainer_equals_the_seq_means_over_the_f32_assignment(n, d, m, iters, init):
    x = wide_rows(n, d, m, seed=5, span=20)
    first = wide_rows(256 * m, d // m, 1, seed=6, span=20).reshape(m, 256, d // m) if init else None
    want = S.pq_train(x, m, iters=iters, init=first, backend="f32", means="seq")
    got = S.pq_train(x, m, iters=iters, init=first, backend="gpu", means="gpu")
    assert np.array_equal(u32(got), u32(want))  # n < 256: the centroids without members keep their value in both


REFUSALS = [("rows null", -129, dict(tweak=lambda p: setattr(p, "rows", 0))),
            ("codes null", -129, dict(tweak=lambda p: setattr(p, "codes", 0))),
            ("codebook_in null", -129, dict(tweak=lambda p: setattr(p, "codebook_in", 0))),
            ("codebook_out null", -129, dict(tweak=lambda p: setattr(p, "codebook_out", 0))),
            ("D % M", -130, dict(tweak=lambda p: setattr(p, "D", 120))),
            ("M % 16", -131, dict(tweak=lambda p: (setattr(p, "M", 24), setattr(p, "D", 120)))),
            ("M < 16", -132, dict(tweak=lambda p: setattr(p, "M", 0))),
            ("M > 96", -132, dict(tweak=lambda p: (setattr(p, "M", 112), setattr(p, "D", 224)))),
            ("dsub > 64", -133, dict(tweak=lambda p: setattr(p, "D", 16 * 65))),
            ("D > 2048", -134, dict(tweak=lambda p: (setattr(p, "M", 48), setattr(p, "D", 2064)))),
            ("ldr < D", -135, dict(tweak=lambda p: setattr(p, "ldr", 120))),
            ("ldr % 8", -135, dict(tweak=lambda p: setattr(p, "ldr", 132))),
            ("ldc < M", -136, dict(tweak=lambda p: setattr(p, "ldc", 0))),
            ("ldc % 16", -136, dict(tweak=lambda p: setattr(p, "ldc", 24))),
            ("N = 0", -137, dict(tweak=lambda p: setattr(p, "N", 0))),
            ("rows misaligned", -138, dict(tweak=lambda p: setattr(p, "rows", p.rows + 8))),
            ("codes misaligned", -138, dict(tweak=lambda p: setattr(p, "codes", p.codes + 8))),
            ("codebook_out misaligned", -138, dict(tweak=lambda p: setattr(p, "codebook_out", p.codebook_out + 4))),
            ("counts misaligned", -138, dict(tweak=lambda p: setattr(p, "counts", p.counts + 2))),
            ("N > 2^31 - 1", -142, dict(tweak=lambda p: setattr(p, "N", 2 ** 31)))]


@pytest.mark.parametrize("what,code,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_launcher_refuses_without_launching(what, code, kw):
    x, codes, cb = wide_rows(40, 128, 16), make_codes("uniform", 40, 16), sentinels(16, 8)
    rc, got, cnt = update(x, codes, cb, **kw)
    assert rc == code and (got == NEVER).all() and (cnt == NEVER).all()  # nothing ran


def test_hz_pq_train_refuses_negative_iters_with_a_message():
    bits, cb = S.to_bf16(wide_rows(40, 128, 16)), sentinels(16, 8)
    lib = N_.lib()
    assert lib.hz_pq_train(0, bits.ctypes.data, 40, 128, 16, cb.ctypes.data, -1, None) == -141
    assert b"iters" in lib.hz_index_last_error() and np.array_equal(cb, sentinels(16, 8))
    assert lib.hz_pq_train(0, bits.ctypes.data, 40, 120, 16, cb.ctypes.data, 1, None) == -130  # the launchers' codes
    with pytest.raises(ValueError, match="iters"):
        OS.pq_train_rows(bits, cb, -1)
    assert np.array_equal(u32(OS.pq_train_rows(bits, cb, 0)), u32(cb))  # no iteration: the codebook as it came
