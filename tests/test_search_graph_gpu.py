"""The graph-search kernel (csrc/search.hip, HZ_K_SEARCH_GRAPH) through ``launch_graph`` against the numpy walk
(``hipzap.search.search_graph_ref``). On integer data every score is an exact integer in fp32 and in fp64, so the fp64
walk decides every comparison as the kernel must: ids, score bits and stats are compared exactly."""
import numpy as np
import pytest
import torch

from hipzap import search as S
from hipzap.ops import search as OS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # elements after each output buffer that no launch may touch


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def integer_case(N, D, deg, seed, Q=3):
    """Integers in [-3, 3] (ties abound) and a random graph with padding, duplicate edges and self-loops."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-3, 4, (N, D)).astype(np.float32)
    q = rng.integers(-3, 4, (Q, D)).astype(np.float32)
    graph = rng.integers(0, N, (N, deg)).astype(np.int32)
    graph[rng.random((N, deg)) < 0.15] = -1
    graph[::7, 1] = graph[::7, 0]            # duplicate edges
    graph[::5, 2] = np.arange(N)[::5]        # self-loops
    return S.to_bf16(rows), rows, q, graph


def run(bits, q, graph, entries, k, beam, width, iters, ldc=None, tweak=None):
    """One launch over device copies -> (code, scores, ids, stats); the guard elements keep their fill."""
    n, d = bits.shape
    ldc = ldc or d
    host = np.zeros((n, ldc), np.uint16)
    host[:, :d] = bits
    dev = [torch.from_numpy(a).to(DEV) for a in (host.view(np.int16), np.ascontiguousarray(q, np.float32),
                                                 np.ascontiguousarray(graph, np.int32), np.ascontiguousarray(entries, np.int32))]
    Q = q.shape[0]
    sc = torch.full((Q * k + GUARD,), 7.0, dtype=torch.float32, device=DEV)
    ids = torch.full((Q * k + GUARD,), -7, dtype=torch.int32, device=DEV)
    st = torch.full((Q * 2 + GUARD,), -7, dtype=torch.int32, device=DEV)
    p = OS.GraphParams(*(t.data_ptr() for t in dev), sc.data_ptr(), ids.data_ptr(), st.data_ptr(), n, d, Q, k, ldc, beam,
                       graph.shape[1], width, iters, len(entries))
    if tweak:
        tweak(p)
    rc = OS.launch_graph(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    s, i, t = sc.cpu().numpy(), ids.cpu().numpy(), st.cpu().numpy()
    assert (s[Q * k:] == 7.0).all() and (i[Q * k:] == -7).all() and (t[Q * 2:] == -7).all(), "a write past an output"
    return rc, s[:Q * k].reshape(Q, k), i[:Q * k].reshape(Q, k), t[:Q * 2].reshape(Q, 2)


def check(bits, rows, q, graph, entries, k, beam, width, iters, **kw):
    rc, sc, ids, st = run(bits, q, graph, entries, k, beam, width, iters, **kw)
    es, ei, est = S.search_graph_ref(rows, q, graph, entries, k, beam, width, iters)
    assert rc == 0
    assert np.array_equal(ids, ei) and np.array_equal(u32(sc), u32(es)) and np.array_equal(st, est), (k, beam, width, iters)
    return ids, st


@pytest.mark.parametrize("beam", [32, 256])
@pytest.mark.parametrize("deg,width", [(8, 1), (8, 4), (64, 4)])
@pytest.mark.parametrize("D", [24, 520, 2048])
def test_the_kernel_is_the_numpy_walk_bit_for_bit(D, deg, width, beam):
    bits, rows, q, graph = integer_case(300, D, deg, seed=D + deg + width)
    entries = np.array([5, 5, 299, -1, 300, 17, 40], np.int32)  # a duplicate and two invalid ids
    for k in (1, 10, min(beam, 128)):
        check(bits, rows, q, graph, entries, k, beam, width, 12, ldc=D + 8 if k == 10 else D)


def test_a_small_component_ends_the_walk_early():
    bits, rows, q, graph = integer_case(300, 72, 8, seed=1)
    rng = np.random.default_rng(2)
    comp = np.sort(rng.choice(300, 20, replace=False)).astype(np.int32)
    graph[comp] = comp[rng.integers(0, 20, (20, 8))]
    graph[comp[:-1], 0] = comp[1:]  # a chain, so all 20 are reached
    ids, st = check(bits, rows, q, graph, comp[:1], 32, 32, 1, 200)
    assert (st[:, 0] < 200).all() and (st[:, 1] == 20).all()
    assert (ids[:, :20] >= 0).all() and (ids[:, 20:] == -1).all()


@pytest.mark.parametrize("iters", [7, 31])  # the bound of the small and of the large visited table with 64 entries
def test_a_full_visited_table(iters):
    bits, rows, q, graph = integer_case(40000, 8, 64, seed=3)
    entries = S.graph_entries(40000)
    assert 64 + iters * 256 <= (OS.GRAPH_CAP_SMALL if iters == 7 else OS.GRAPH_CAP_LARGE) // 2 < 64 + (iters + 1) * 256
    _, st = check(bits, rows, q, graph, entries, 128, 256, 4, iters)
    assert (st[:, 0] == iters).all() and (st[:, 1] > (entries.size + iters * 256) // 2).all()  # 15 % padding, few repeats


def test_a_complete_graph_is_the_exact_search():
    bits, rows, q, _ = integer_case(40, 64, 64, seed=4)
    graph = np.array([np.r_[np.delete(np.arange(40), r), [-1] * 25] for r in range(40)], np.int32)
    rc, sc, ids, _ = run(bits, q, graph, np.array([7], np.int32), 64, 64, 1, 5)
    es, ei = S.search_ref(rows, q, 40)
    assert rc == 0 and np.array_equal(ids[:, :40], ei) and np.array_equal(u32(sc[:, :40]), u32(es))
    assert (ids[:, 40:] == -1).all() and (sc[:, 40:] == -np.inf).all()


def test_scores_are_the_rescore_kernels_bits_on_real_data():
    rng = np.random.default_rng(5)
    N, D, Q, k = 2000, 768, 3, 64
    bits = S.prepare_rows(rng.standard_normal((N, D)).astype(np.float32), "cosine")
    q = rng.standard_normal((Q, D)).astype(np.float32)
    graph = rng.integers(0, N, (N, 32)).astype(np.int32)
    rc, sc, ids, st = run(bits, q, graph, S.graph_entries(N), k, 128, 2, 40)
    again = run(bits, q, graph, S.graph_entries(N), k, 128, 2, 40)
    assert rc == 0 and np.array_equal(u32(sc), u32(again[1])) and np.array_equal(ids, again[2]) and np.array_equal(st, again[3])
    assert (ids >= 0).all() and all(len(set(r.tolist())) == k for r in ids)
    tie = (sc[:, :-1] == sc[:, 1:]) & (ids[:, :-1] < ids[:, 1:])
    assert ((sc[:, :-1] > sc[:, 1:]) | tie).all()  # strictly descending under (score, then the lower id)
    dev = [torch.from_numpy(a).to(DEV) for a in (bits.view(np.int16), q, ids)]
    rs = torch.zeros((Q, k), dtype=torch.float32, device=DEV)
    ri = torch.zeros((Q, k), dtype=torch.int32, device=DEV)
    p = OS.RescoreParams(*(t.data_ptr() for t in dev), rs.data_ptr(), ri.data_ptr(), N, D, Q, k, k, D)
    assert OS.launch_rescore(p, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(ri.cpu().numpy(), ids) and np.array_equal(u32(rs.cpu().numpy()), u32(sc))


def setp(**kv):
    return lambda p: [setattr(p, a, v(p) if callable(v) else v) for a, v in kv.items()]


@pytest.mark.parametrize("what,code,tweak", [
    ("D % 8", -218, setp(D=28)), ("ldc < D", -218, setp(ldc=24)), ("N = 0", -219, setp(N=0)), ("Q = 0", -220, setp(Q=0)),
    ("k > beam", -221, setp(k=33)), ("k > 128", -221, setp(k=129, beam=256)), ("beam % 32", -222, setp(beam=48)),
    ("beam > 256", -222, setp(beam=288)), ("deg % 8", -223, setp(deg=12)), ("deg > 64", -223, setp(deg=72)),
    ("width * deg > 256", -224, setp(width=33)), ("iters = 0", -225, setp(iters=0)), ("E = 0", -226, setp(E=0)),
    ("E > 256", -226, setp(E=257)), ("visited bound", -227, setp(iters=1024)), ("graph null", -228, setp(graph=0)),
    ("out_id null", -228, setp(out_id=0)), ("corpus misaligned", -229, setp(corpus=lambda p: p.corpus + 8)),
    ("out_stats misaligned", -229, setp(out_stats=lambda p: p.out_stats + 2))])
def test_the_launcher_refuses_misuse_without_launching(what, code, tweak):
    bits, rows, q, graph = integer_case(40, 32, 8, seed=6)
    rc, sc, ids, st = run(bits, q, graph, np.arange(8, dtype=np.int32), 10, 32, 1, 1000, tweak=tweak)
    assert rc == code and (sc == 7.0).all() and (ids == -7).all() and (st == -7).all(), what
