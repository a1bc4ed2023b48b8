"""Per-query entry rows on the GPU: the seed kernel (csrc/search.hip, HZ_K_GRAPH_SEED) against
``hipzap.search.graph_seed_ref``, HZ_K_SEARCH_GRAPH reading ``[Q][estride]`` entries, and ``Index.search_graph(seeds=)`` on
a version-13 file. Rows and queries are integers in -3..3: every partial sum is exact in fp32, ties abound, so ids are
compared one for one and the position tie-break is exercised."""
import numpy as np
import pytest
import torch

from hipzap import search as S
from hipzap.ops import search as OS

from test_graph_seed_cpu import clustered_case, recall

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16  # elements after an output buffer that no launch may touch


def integer_case(N, D, Q, S_, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(-3, 4, (N, D)).astype(np.float32)
    q = rng.integers(-3, 4, (Q, D)).astype(np.float32)
    seeds = rng.integers(0, N, S_).astype(np.int32)  # repeats are legal for the kernel
    seeds[1::13], seeds[2::29], seeds[5::31] = -1, N, seeds[0]
    return S.to_bf16(rows), rows, q, seeds


def run_seed(bits, q, seeds, E, estride=None, ldc=None, tweak=None):
    """One launch over device copies -> (code, out [Q, estride]); the guard and the columns from E on keep their fill."""
    (n, d), Q, estride = bits.shape, q.shape[0], estride or E
    host = np.zeros((n, ldc or d), np.uint16)
    host[:, :d] = bits
    dev = [torch.from_numpy(a).to(DEV) for a in (host.view(np.int16), np.ascontiguousarray(q, np.float32),
                                                 np.ascontiguousarray(seeds, np.int32))]
    out = torch.full((Q * estride + GUARD,), -7, dtype=torch.int32, device=DEV)
    p = OS.GraphSeedParams(*(t.data_ptr() for t in dev), out.data_ptr(), n, d, Q, len(seeds), E, ldc or d, estride)
    if tweak:
        tweak(p)
    rc = OS.launch_graph_seed(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[Q * estride:] == -7).all(), "a write past the output"
    return rc, o[:Q * estride].reshape(Q, estride)


@pytest.mark.parametrize("D,S_,Q,E", [
    (24, 1, 1, 1), (24, 17, 16, 8), (24, 197, 17, 64), (520, 17, 33, 64), (520, 197, 1, 8), (520, 4200, 17, 64),
    (520, 4200, 33, 1), (2048, 197, 33, 64), (2048, 17, 1, 8), (64, 4200, 16, 8), (768, 8192, 5, 16)])
def test_the_seed_kernel_is_graph_seed_ref_id_for_id(D, S_, Q, E):
    bits, rows, q, seeds = integer_case(300, D, Q, S_, seed=D + S_ + Q + E)
    rc, out = run_seed(bits, q, seeds, E, estride=E + 3, ldc=D + 8 if Q == 17 else D)
    want = S.graph_seed_ref(rows, q, seeds, E)
    assert rc == 0 and np.array_equal(out[:, :E], want) and (out[:, E:] == -7).all()
    valid = int(((seeds >= 0) & (seeds < 300)).sum())
    assert (want[:, min(E, valid):] == -1).all() and (want[:, :min(E, valid)] >= 0).all()  # E > valid seeds: a -1 tail


def run_graph(bits, q, graph, entries, k, beam, width, iters, E, estride):
    dev = [torch.from_numpy(a).to(DEV) for a in (bits.view(np.int16), np.ascontiguousarray(q, np.float32),
                                                 np.ascontiguousarray(graph, np.int32), np.ascontiguousarray(entries, np.int32))]
    Q = q.shape[0]
    sc = torch.full((Q * k + GUARD,), 7.0, dtype=torch.float32, device=DEV)
    ids = torch.full((Q * k + GUARD,), -7, dtype=torch.int32, device=DEV)
    st = torch.full((Q * 2 + GUARD,), -7, dtype=torch.int32, device=DEV)
    p = OS.GraphParams(*(t.data_ptr() for t in dev), sc.data_ptr(), ids.data_ptr(), st.data_ptr(), bits.shape[0], bits.shape[1],
                       Q, k, bits.shape[1], beam, graph.shape[1], width, iters, E, estride)
    rc = OS.launch_graph(p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    s, i, t = sc.cpu().numpy(), ids.cpu().numpy(), st.cpu().numpy()
    assert (s[Q * k:] == 7.0).all() and (i[Q * k:] == -7).all() and (t[Q * 2:] == -7).all(), "a write past an output"
    return rc, s[:Q * k].reshape(Q, k), i[:Q * k].reshape(Q, k), t[:Q * 2].reshape(Q, 2)


@pytest.mark.parametrize("D,deg,width", [(24, 8, 4), (520, 16, 1)])
def test_the_walk_reads_its_entries_per_query(D, deg, width):
    Q, E, estride, k, beam, iters = 5, 6, 9, 10, 32, 12
    bits, rows, q, _ = integer_case(300, D, Q, 8, seed=D)
    rng = np.random.default_rng(D + 1)
    graph = rng.integers(0, 300, (300, deg)).astype(np.int32)
    graph[rng.random((300, deg)) < 0.15] = -1
    entries = rng.integers(0, 300, (Q, estride)).astype(np.int32)
    entries[1, 3:], entries[2, 0], entries[3, 1] = -1, 300, entries[3, 0]  # -1 padding, an invalid id, a repeat
    rc, sc, ids, st = run_graph(bits, q, graph, entries, k, beam, width, iters, E, estride)
    assert rc == 0
    for a in range(Q):
        es, ei, est = S.search_graph_ref(rows, q[a:a + 1], graph, entries[a, :E], k, beam, width, iters)
        assert np.array_equal(ids[a], ei[0]) and np.array_equal(sc[a].view(np.uint32), es[0].astype(np.float32).view(np.uint32))
        assert np.array_equal(st[a], est[0])
    rc, sc, ids, st = run_graph(bits, q, graph, entries, k, beam, width, iters, E, 0)  # the old mode: row 0, shared
    es, ei, est = S.search_graph_ref(rows, q, graph, entries[0, :E], k, beam, width, iters)
    assert rc == 0 and np.array_equal(ids, ei) and np.array_equal(st, est)
    assert np.array_equal(sc.view(np.uint32), es.astype(np.float32).view(np.uint32))


def setp(**kv):
    return lambda p: [setattr(p, a, v(p) if callable(v) else v) for a, v in kv.items()]


@pytest.mark.parametrize("what,code,tweak", [
    ("D % 8", -243, setp(D=28)), ("ldc < D", -243, setp(ldc=24)), ("N = 0", -244, setp(N=0)), ("Q = 0", -245, setp(Q=0)),
    ("S = 0", -246, setp(S=0)), ("S > 8192", -246, setp(S=8193)), ("E = 0", -247, setp(E=0)), ("E > 64", -247, setp(E=65, estride=65)),
    ("estride < E", -248, setp(estride=3)), ("seeds null", -249, setp(seeds=0)), ("out null", -249, setp(out=0)),
    ("queries misaligned", -250, setp(queries=lambda p: p.queries + 8)), ("out misaligned", -250, setp(out=lambda p: p.out + 2))])
def test_the_seed_launcher_refuses_misuse_without_launching(what, code, tweak):
    bits, rows, q, seeds = integer_case(40, 32, 3, 20, seed=6)
    rc, out = run_seed(bits, q, seeds, 4, tweak=tweak)
    assert rc == code and (out == -7).all(), what


@pytest.mark.parametrize("estride", [-1, 3])
def test_the_walk_refuses_a_stride_below_its_entries(estride):
    bits, rows, q, _ = integer_case(40, 32, 3, 8, seed=7)
    graph = np.random.default_rng(8).integers(0, 40, (40, 8)).astype(np.int32)
    rc, sc, ids, st = run_graph(bits, q, graph, np.zeros((3, 4), np.int32), 10, 32, 1, 5, 4, estride)
    assert rc == -251 and (sc == 7.0).all() and (ids == -7).all() and (st == -7).all()


def test_a_version_13_index_is_the_reference_index(tmp_path):
    rng = np.random.default_rng(9)
    rows, q = rng.integers(-3, 4, (600, 96)).astype(np.float32), rng.integers(-3, 4, (21, 96)).astype(np.float32)
    path = str(tmp_path / "s.hzidx")
    S.write_index(path, rows, "ip", graph=16, graph_seeds=100)
    with S.Index(path) as ix, S.RefIndex(path) as ref:
        assert ix.version == 13 and ix.describe()["graph_seeds"] == 100
        for E in (4, 64):
            want = ref.search_graph(q, 10, beam=64, iters=20, seeds=E, stats=True)
            for _ in range(2):  # the eager run, then the captured program's replay
                got = ix.search_graph(q, 10, beam=64, iters=20, seeds=E, stats=True)
                assert all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got, want)), E
        got, want = ix.search_graph(q, 10, beam=64, iters=20), ref.search_graph(q, 10, beam=64, iters=20)
        assert np.array_equal(got[1], want[1]) and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))  # None: shared
        ix.set_graph(ix.graph, seeds=[5, 599, 17])  # an explicit table replaces the file's
        ref.set_graph(ref.graph, seeds=[5, 599, 17])
        assert np.array_equal(ix.search_graph(q, 10, beam=64, iters=20, seeds=4)[1], ref.search_graph(q, 10, beam=64, iters=20, seeds=4)[1])
        ix.set_graph(ix.graph)
        with pytest.raises(ValueError, match="has none"):
            ix.search_graph(q, 10, seeds=4)


def test_per_query_entries_reach_the_querys_cluster(tmp_path):
    """Non-integer rows: a selection near-tie may pick another entry than the fp64 oracle, so recall is asserted, not
    equality. The fp64 walk gives 1.000 with seeds=16 of 512 and 0.375 with the shared entries (test_graph_seed_cpu)."""
    rows, q = clustered_case()
    path = str(tmp_path / "c.hzidx")
    S.write_index(path, rows, "cosine", graph=16, graph_seeds=512)
    with S.Index(path) as ix:
        truth = ix.search(q, 10)[1]
        shared = recall(ix.search_graph(q, 10, beam=64, width=1, iters=64)[1], truth)
        seeded = recall(ix.search_graph(q, 10, beam=64, width=1, iters=64, seeds=16)[1], truth)
    print(f"recall@10 on the GPU: shared entries {shared:.3f}, seeds=16 of 512 {seeded:.3f}")
    assert seeded >= 0.95 and shared < 0.6
