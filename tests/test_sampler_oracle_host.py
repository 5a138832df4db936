"""tests/sampler_oracle.py on the host: the Random123 known answers for
Philox4x32-10, the distributions the restated transforms produce, and the
TruncatedNormal rejections of one seed (found independently of this file).
No GPU."""

import numpy as np
import pytest
from scipy import stats

from tests import sampler_oracle as S
from zenflow_amd import _lib as L


@pytest.mark.parametrize(
    "counter,key,want",
    [
        ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
        ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
        ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
         [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
    ],
)
def test_philox_known_answers(counter, key, want):
    got = S.philox4x32_10(np.array(counter, np.uint32), np.array(key, np.uint32))
    assert [int(v) for v in got] == want
    # vectorised over rows: the same answer on every row of a batch
    batch = S.philox4x32_10(np.tile(np.array(counter, np.uint32), (5, 1)), np.array(key, np.uint32))
    assert batch.shape == (5, 4) and all([int(v) for v in row] == want for row in batch)


def test_philox_at_counter_layout():
    """counter = (row lo, row hi, dim, stream), key = (seed lo, seed hi)."""
    row, dim, stream, seed = (3 << 32) | 17, 5, 9, (0xABCD << 32) | 0x1234
    got = S.philox_at(seed, np.array([row]), dim, stream)[0]
    want = S.philox4x32_10(np.array([17, 3, 5, 9], np.uint32), np.array([0x1234, 0xABCD], np.uint32))
    assert np.array_equal(got, want)


def test_unit_interval_ends():
    b = np.array([0, 0xFF, 0x100, 0xFFFFFFFF], np.uint32)
    assert S.u01_co(b).tolist() == [0.0, 0.0, 2.0**-24, 1.0 - 2.0**-24]
    assert S.u01_oc(b).tolist() == [2.0**-24, 2.0**-24, 2.0**-23, 1.0]


@pytest.mark.parametrize(
    "latent,param,ref",
    [
        (L.ZF_LATENT_NORMAL, 0.0, stats.norm(0.5, 0.1)),
        (L.ZF_LATENT_TRUNCNORM, 0.0, stats.truncnorm(-5, 5, loc=0.5, scale=0.1)),
        (L.ZF_LATENT_BETA, 12.0, stats.beta(12, 12)),
        (L.ZF_LATENT_BETA, 3.0, stats.beta(3, 3)),
        (L.ZF_LATENT_UNIFORM, 0.0, stats.uniform(0, 1)),
    ],
)
def test_oracle_distribution_ks(latent, param, ref):
    """The five distributions of tests/test_gpu_sampling.py, same n and seed."""
    z, _ = S.sample(latent, param, 7, 1 << 16, 3)
    assert z.dtype == np.float32 and np.isfinite(z).all()
    for j in range(3):
        p = stats.kstest(z[:, j].astype(np.float64), ref.cdf).pvalue
        assert p > 1e-4, f"dim {j}: KS p={p:.2e}"


def test_truncated_normal_rejections_seed7():
    """Seed 7, dim 0: the first trial is rejected at exactly three rows below
    2^22, with |n| = 5.080, 5.033, 5.032, and no draw lies within 1e-3 of the
    +-5 boundary (so the device's last-bit differences cannot move a row
    across it)."""
    n = 1 << 22
    z, info = S.latent_draw(L.ZF_LATENT_TRUNCNORM, 0.0, 7, np.arange(n), 0)
    first = info["n"][0]["n"]
    rej = np.flatnonzero(info["trial"] > 0)
    assert rej.tolist() == [1151898, 2400647, 3474826]
    assert np.all(info["trial"][rej] == 1)
    np.testing.assert_allclose(np.abs(first[rej]), [5.080, 5.033, 5.032], atol=5e-4)
    for tr in info["n"]:
        assert np.abs(np.abs(tr["n"]) - 5.0).min() > 1e-3
    assert z.min() >= 0.0 and z.max() <= 1.0
    # the second-trial value is what a row gets
    second = info["n"][1]
    assert second["idx"].tolist() == rej.tolist()
    assert np.array_equal(z[rej], (0.5 + np.float64(np.float32(0.1)) * second["n"].astype(np.float64)).astype(np.float32))


def test_beta_retries_and_near_ties():
    """Marsaglia-Tsang at alpha = 1 accepts ~95% of first trials: retries are
    present; the near-tie share is what the GPU test's condition assumes."""
    n = 1 << 16
    for a in (12.0, 3.0, 1.0):
        z, info = S.latent_draw(L.ZF_LATENT_BETA, a, 7, np.arange(n), 0)
        assert np.all(info["trial"] >= 0) and np.all((z > 0) & (z < 1))
        assert S.near_ties(info, n, 1e-4, 1e-5).mean() <= 1e-3
    assert (info["trial"] > 0).mean() > 0.03
