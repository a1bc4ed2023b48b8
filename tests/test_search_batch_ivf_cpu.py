"""Bulk search over IVF indexes on the host: ``RefIndex.probes_batch`` / ``search_batch_ivf``, the shared
refusals, and the claims that tests/test_search_batch_ivf_gpu.py rests on for the inputs of search_batch_ivf_cases.py."""
import numpy as np
import pytest

from hipzap import search as S

import search_batch_ivf_cases as V


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    root = tmp_path_factory.mktemp("batch_ivf")
    return {d: (str(root / f"d{d}.hzidx"), V.write(str(root / f"d{d}.hzidx"), d)) for d in V.DIMS}


def test_the_corpus_has_the_lists_the_cases_describe(files):
    path, q = files[32]
    with S.RefIndex(path) as ref:
        sizes = np.bincount(ref.ivf["list_of"], minlength=V.NLIST)
        assert tuple(sizes) == V.SIZES and np.diff(ref.ivf["list_off"]).tolist() == [2, 1, 0, 1, 1]
        first = ref.probes(q, 1)[:, 0]
        assert (first[:66] == 0).all() and (first == 1).sum() == 1 and first[V.LONE] == 1 and first[V.EMPTY] == 2
        assert not (ref.probes(q, 2) == 1)[np.arange(V.Q) != V.LONE].any()  # list 1 is the lone query's alone


@pytest.mark.parametrize("d", V.DIMS)
@pytest.mark.parametrize("nprobe", (1, 2, "all"))
@pytest.mark.parametrize("k, cand", ((1, 1), (10, None), (10, 10)))
def test_ref_equals_search_and_the_oracle(files, d, nprobe, k, cand):
    path, q = files[d]
    with S.RefIndex(path) as ref:
        lists = ref._nprobe(nprobe)
        s, i, certain = ref.search_batch_ivf(q, k, nprobe=nprobe, candidates=cand)
        assert certain.all() and np.array_equal(i, ref.search(q, k, nprobe=nprobe)[1])
        s0, i0, c0 = ref.search_batch_ivf(q, k, nprobe=nprobe, candidates=cand, fallback=False)
        want, sure = V.forced(ref, q, k, lists)
        assert np.array_equal(i0[c0 & sure], want[c0 & sure]) and (c0 & sure).sum() >= (1 if cand is None or nprobe == 1 else 0)
        few, enough = V.clauses(ref, q, k, lists, cand)
        assert c0[few].all()  # fewer than R live rows probed: s_R is -inf
        if nprobe == 1:
            assert few[V.EMPTY] and (i0[V.EMPTY] == -1).all() and np.isneginf(s0[V.EMPTY]).all()
        if cand is None:
            assert (c0 & enough).any()  # the slack clause certifies somebody


def test_probes_batch_on_an_ip_index_with_unequal_centroid_norms(tmp_path):
    path = str(tmp_path / "ip.hzidx")
    q = V.write(path, 96, "ip")
    with S.RefIndex(path) as ref:
        norms = np.sqrt((ref._cent.astype(np.float64) ** 2).sum(axis=1))
        assert norms.max() / norms.min() >= 3.9
        for n, cand in ((1, None), (2, None), (2, 2), (5, 5)):
            lists, certain = ref.probes_batch(q, n, candidates=cand, fallback=False)
            assert np.array_equal(lists[certain], ref.probes(q, n)[certain]) and (cand is not None or certain.all())
            lists, certain = ref.probes_batch(q, n, candidates=cand)
            assert certain.all() and np.array_equal(lists, ref.probes(q, n))


def test_refusals_name_the_rule(files, tmp_path):
    path, q = files[32]
    flat, fp8, odd = (str(tmp_path / n) for n in ("flat.hzidx", "fp8.hzidx", "odd.hzidx"))
    v, _, init, _ = V.data(32, "cosine")
    S.write_index(flat, v, "cosine")
    S.convert_index(path, fp8, "fp8")
    S.write_index(odd, v[:, :24], "cosine", ivf=V.NLIST, ivf_iters=0, ivf_init=init[:, :24])
    with S.RefIndex(flat) as ix, pytest.raises(ValueError, match="built for IVF indexes over bf16 rows.*without lists of version 1"):
        ix.search_batch_ivf(q, 10)
    with S.RefIndex(fp8) as ix, pytest.raises(ValueError, match="an fp8 IVF index of version 6"):
        ix.probes_batch(q, 2)
    with S.RefIndex(odd) as ix, pytest.raises(ValueError, match="dim % 32 == 0.*dim = 24"):
        ix.search_batch_ivf(q[:, :24], 10)
    with S.RefIndex(path) as ix:
        for bad in (0, -1, 1.5, "some"):
            with pytest.raises(ValueError, match="nprobe must be"):
                ix.search_batch_ivf(q, 10, nprobe=bad)
        with pytest.raises(ValueError, match="nprobe must be"):
            ix.probes_batch(q, V.NLIST + 1)
        with pytest.raises(ValueError, match="candidates must be"):
            ix.search_batch_ivf(q, 10, candidates=9)
