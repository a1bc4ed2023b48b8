"""Bulk search over fp8 indexes on the host: ``RefIndex.search_batch_fp8`` against ``RefIndex.search``, the slack, refusals."""
import numpy as np
import pytest

from hipzap import search as S

from search_pq_cases import u32

N, D, K, SEED = 600, 64, 10, 7


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    rng = np.random.default_rng(SEED)
    v = rng.standard_normal((N, D)).astype(np.float32)
    q = S.normalize_rows(rng.standard_normal((70, D)).astype(np.float32))
    root = tmp_path_factory.mktemp("fp8batch")
    paths = {}
    for version, metric in ((3, "cosine"), (3, "ip"), (4, "cosine")):
        paths[version, metric] = str(root / f"v{version}{metric}.hzidx")
        S.write_index(paths[version, metric], v, metric, dtype="fp8", rescore=version == 4)
    return paths, v, q


@pytest.mark.parametrize("version,metric", [(3, "cosine"), (3, "ip"), (4, "cosine")])
def test_certain_or_fallback_means_equal_to_search_in_ids_and_score_bits(data, version, metric):
    paths, v, q = data
    with S.RefIndex(paths[version, metric]) as ref:
        ref.delete([3, 300])
        R = S.batch_candidates(K)
        ws, wi = ref.search(q, K, refine=R) if version == 4 else ref.search(q, K)
        s, i, c = ref.search_batch_fp8(q, K, fallback=False)
        # SEED certifies every query of the cosine case, so this comparison is not vacuous; nothing bounds the others
        assert c.all() if (version, metric) == (3, "cosine") else not c.any()
        assert np.array_equal(i[c], wi[c]) and np.array_equal(u32(s[c]), u32(ws[c])) and not np.isin(i, [3, 300]).any()
        s2, i2, c2 = ref.search_batch_fp8(q, K, fallback=True)
        assert c2.all() and np.array_equal(i2, wi) and np.array_equal(u32(s2), u32(ws))
        assert ref.search_batch_fp8(q, K)[2].all() == (version == 3)  # fallback=None: True on version 3 only
        few = ref.search_batch_fp8(q[:2], 5, candidates=128)  # fewer than R rows pass: certain without any bound
        ref.delete(np.arange(100, N))
        assert ref.search_batch_fp8(q[:2], 5, candidates=128, fallback=False)[2].all() and few[0].shape == (2, 5)


def test_the_slack_covers_a_brute_force_fp64_bound(data):
    """Per (query, row): the three error terms of the docstring over the row as decoded, summed in fp64."""
    paths, v, q = data
    q = np.concatenate([q, q[:3] * np.float32(2.0 ** -110)])  # queries whose split flushes terms
    codes, scales = S.prepare_rows_fp8(v, "cosine")
    x = np.abs(S.e4m3_to_f32(codes).astype(np.float64) * scales.astype(np.float64)[:, None])
    assert np.sqrt((x * x).sum(axis=1)).max() <= S.fp8_cosine_rmax(D) < 1.125
    bf = S.bf16_to_f32(S.to_bf16(S.normalize_rows(v)))  # convert_index: stored bf16 rows, requantised as they stand
    c2, s2 = S.quantize_rows(bf)
    assert np.sqrt(((S.e4m3_to_f32(c2).astype(np.float64) * s2[:, None]) ** 2).sum(axis=1)).max() <= S.fp8_cosine_rmax(D)
    u, b = 2.0 ** -24, 3 * D * 2.0 ** -23 / (1 - 3 * D * 2.0 ** -23)
    g = (D + 1) * u / (1 - (D + 1) * u)
    brute = ((b * (1 + u) + u + g) * (np.abs(q.astype(np.float64)) @ x.T) + 3 * 2.0 ** -126 * x.sum(axis=1)[None, :]).max(axis=1)
    slack = S.fp8_batch_slack(q, "cosine")
    assert (brute <= slack).all() and (slack[:70] < 4 * brute[:70]).all() and S.fp8_batch_slack(q, "ip") is None


@pytest.mark.parametrize("kw,what", [(dict(), "a bf16 index of version 1"), (dict(dtype="pq", pq_m=16), "a pq8 index of version 10"),
                                     (dict(dtype="bin"), "a bin_sign index of version 8"),
                                     (dict(dtype="fp8", ivf=4), "an fp8 IVF index of version 6"), (dict(dtype="fp8"), "dim % 32")])
def test_refusals_by_name(tmp_path, kw, what):
    d = 48 if what == "dim % 32" else 128
    v = np.random.default_rng(1).standard_normal((300, d)).astype(np.float32)
    if "ivf" in kw:  # an fp8 IVF file is a converted bf16 IVF file
        S.write_index(str(tmp_path / "b.hzidx"), v, "ip", ivf=4)
        S.convert_index(str(tmp_path / "b.hzidx"), str(tmp_path / "a.hzidx"), "fp8")
    else:
        S.write_index(str(tmp_path / "a.hzidx"), v, "ip", **kw)
    with S.RefIndex(str(tmp_path / "a.hzidx")) as ref:
        with pytest.raises(ValueError, match=f"search_batch_fp8 .*{what}"):
            ref.search_batch_fp8(v[:2], 5)
