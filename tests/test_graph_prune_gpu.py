"""The pruning kernel (csrc/search.hip, HZ_K_GRAPH_PRUNE) against ``hipzap.search.graph_prune_ref``: integers, so
``order`` and ``detours`` are compared bit for bit; the launcher's refusals; and the route through an index."""
import faulthandler

import numpy as np
import pytest
import torch

from hipzap import search as S
from hipzap.ops import search as OS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # elements after each output buffer that no launch may touch
N_ROWS = 301  # not a multiple of the four rows of a workgroup


@pytest.fixture(autouse=True)
def time_limit():
    """A test that hangs on the GPU ends the run here instead of holding the card."""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def nearest():
    """The 128 nearest rows of each of 301 random unit rows, best first (fp64, the row itself left out): real lists, so
    neighbours share neighbours and detours exist."""
    x = np.random.default_rng(0).standard_normal((N_ROWS, 8))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.argsort(-(x @ x.T), axis=1, kind="stable").astype(np.int32)[:, 1:129]


def spoiled(knn, seed):
    """A fixed 5 % of the entries overwritten with padding, the row's own id, an id past N, or the row's column 0."""
    n, w = knn.shape
    rng = np.random.default_rng(seed)
    hit, kind = rng.random((n, w)) < 0.05, rng.integers(0, 4, (n, w))
    junk = np.choose(kind, [-1, np.arange(n)[:, None], n + 3, knn[:, :1]]).astype(np.int32)
    return np.where(hit, junk, knn)


def run(knn, tweak=None, detours=True):
    """One launch over a device copy -> (code, order, detours); the guard elements keep their fill."""
    n, w = knn.shape
    src = torch.from_numpy(np.ascontiguousarray(knn, np.int32)).to(DEV)
    order = torch.full((n * w + GUARD,), -7, dtype=torch.int32, device=DEV)
    det = torch.full((n * w + GUARD,), -7, dtype=torch.int32, device=DEV)
    p = OS.GraphPruneParams(src.data_ptr(), order.data_ptr(), det.data_ptr() if detours else None, n, w)
    if tweak:
        tweak(p)
    rc = OS.launch_graph_prune(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o, d = order.cpu().numpy(), det.cpu().numpy()
    assert (o[n * w:] == -7).all() and (d[n * w:] == -7).all(), "a write past an output"
    return rc, o[:n * w].reshape(n, w), d[:n * w].reshape(n, w)


@pytest.mark.parametrize("n,w", [(N_ROWS, 16), (N_ROWS, 24), (N_ROWS, 64), (N_ROWS, 128), (1, 16)])
def test_the_kernel_is_the_numpy_rule_bit_for_bit(nearest, n, w):
    knn = spoiled(nearest[:, :w], seed=w) if n > 1 else np.array([[0, -1, 3, 0] * 4], np.int32)
    want_order, want_det = S.graph_prune_ref(knn)
    assert n == 1 or want_det.max() >= 2  # the case has something to count
    rc, order, det = run(knn)
    assert rc == 0 and np.array_equal(det, want_det) and np.array_equal(order, want_order)
    rc, order, det = run(knn, detours=False)
    assert rc == 0 and np.array_equal(order, want_order) and (det == -7).all()
    assert np.array_equal(S.graph_prune(knn, "gpu"), want_order)  # the host job: H2D, the kernel, D2H


def setp(**kv):
    return lambda p: [setattr(p, a, v(p) if callable(v) else v) for a, v in kv.items()]


@pytest.mark.parametrize("what,code,tweak", [
    ("W < 16", -238, setp(W=8)), ("W > 128", -238, setp(W=136)), ("W % 8", -238, setp(W=20)), ("N = 0", -239, setp(N=0)),
    ("N * W >= 2^31", -239, setp(N=2 ** 27, W=16)), ("knn null", -240, setp(knn=0)), ("order null", -240, setp(order=0)),
    ("knn misaligned", -241, setp(knn=lambda p: p.knn + 2)), ("detours misaligned", -241, setp(detours=lambda p: p.detours + 1))])
def test_the_launcher_refuses_misuse_without_launching(nearest, what, code, tweak):
    rc, order, det = run(nearest[:40, :16] % 40, tweak=tweak)
    assert rc == code and (order == -7).all() and (det == -7).all(), what
    with pytest.raises(ValueError, match="-238"):
        OS.graph_prune_lists(np.zeros((4, 8), np.int32))


def test_a_pruned_graph_through_the_index(tmp_path):
    rng = np.random.default_rng(1)
    rows = rng.integers(-3, 4, (512, 64)).astype(np.float32)  # exact integer scores: both backends order every list alike
    q = rng.integers(-3, 4, (5, 64)).astype(np.float32)
    path, cpu, gpu = (str(tmp_path / n) for n in ("p.hzidx", "c.hzidx", "g.hzidx"))
    S.write_index(path, rows, "ip")
    with S.Index(path) as ix, S.RefIndex(path) as ref:
        g = ix.build_graph(16, prune=True)
        assert np.array_equal(g, ref.build_graph(16, prune=True)) and not np.array_equal(g, ref.build_graph(16))
        ref.set_graph(g)
        a, b = ix.search_graph(q, 10, beam=32, stats=True), ref.search_graph(q, 10, beam=32, stats=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    S.write_index(cpu, rows, "ip", graph=16, graph_prune=True)
    S.convert_index(path, gpu, "bf16", graph=16, graph_backend="gpu", graph_prune=True)
    assert np.array_equal(S.read_graph(cpu)[0], g) and open(cpu, "rb").read() == open(gpu, "rb").read()
