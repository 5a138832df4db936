"""On-device latent sampling: Distribution.sample and
Flow.sample with the counter-based Philox generator (zf_latent_sample,
zf_flow_sample).

jax.random's threefry draws cannot be reproduced without JAX, so parity with
JAX is (1) statistical — Kolmogorov-Smirnov against scipy's distributions and
the moment checks of the reference's tests/test_distributions.py — and (2)
structural: Flow.sample(seed) is bit-identical to Chain.inverse applied to
Distribution.sample(seed), and Chain.inverse is parity-tested against the
oracle (tests/test_gpu_flow.py).

The device stream itself is fully specified (Philox4x32-10 and the transforms
of zf_random.h) and pinned to its host restatement, tests/sampler_oracle.py:
Uniform bit for bit, Normal / TruncatedNormal / Beta within bounds derived
from the precision of the device's libm calls, with the rejection loops'
trial indices checked and near-ties of the discontinuous acceptance tests set
aside."""

import numpy as np
import pytest
from scipy import stats

import zenflow_amd.distributions as dist
from zenflow_amd import _lib as L
from zenflow_amd.random import PRNGKey, key_to_seed
from tests import sampler_oracle as S
from tests.flowcases import build_flow, make_case

pytestmark = pytest.mark.gpu

N = 1 << 16


def _draw(d, n=N, dim=3, seed=7):
    d._dim = dim
    return d.sample(n, PRNGKey(seed))


@pytest.mark.parametrize(
    "d,ref",
    [
        (dist.Normal(), stats.norm(0.5, 0.1)),
        (dist.TruncatedNormal(), stats.truncnorm(-5, 5, loc=0.5, scale=0.1)),
        (dist.Beta(), stats.beta(12, 12)),
        (dist.Beta(3.0), stats.beta(3, 3)),
        (dist.Uniform(), stats.uniform(0, 1)),
    ],
)
def test_latent_distribution_ks(d, ref):
    z = _draw(d)
    assert z.shape == (N, 3) and z.dtype == np.float32 and np.isfinite(z).all()
    for j in range(3):
        p = stats.kstest(z[:, j].astype(np.float64), ref.cdf).pvalue
        assert p > 1e-4, f"dim {j}: KS p={p:.2e}"
    # dims independent (sample correlation ~ N(0, 1/N))
    r = np.corrcoef(z.T)
    assert np.abs(r[np.triu_indices(3, 1)]).max() < 6 / np.sqrt(N)


def test_latent_support_and_moments():
    """tests/test_distributions.py moment / support checks at the same n."""
    n = 20000
    zn = _draw(dist.Normal(), n)
    np.testing.assert_allclose(zn.mean(0), 0.5, atol=5e-2)
    np.testing.assert_allclose(np.cov(zn.T), 0.1**2 * np.identity(3), atol=5e-2)
    zt = _draw(dist.TruncatedNormal(), n)
    assert np.all(np.abs(zt - 0.5) <= 0.5 + 1e-6)
    zb = _draw(dist.Beta(), n)
    assert np.all(zb > 0) and np.all(zb < 1)
    zu = _draw(dist.Uniform(), n)
    assert zu.min() >= 0 and zu.max() < 1


def test_latent_determinism_and_row_independence():
    d = dist.Beta()
    a = _draw(d, 5000, seed=11)
    b = _draw(d, 5000, seed=11)
    c = _draw(d, 1000, seed=11)
    e = _draw(d, 1000, seed=12)
    assert np.array_equal(a, b)
    assert np.array_equal(a[:1000], c)  # counter-based: row r depends only on (seed, r)
    assert not np.array_equal(c, e)


def test_latent_sample_errors():
    lib = L.load_library()
    z = L.DeviceArray((4, 2))
    assert lib.zf_latent_sample(L.ZF_LATENT_BETA, 0.5, 1, z.ptr, 4, 2, None) == -1
    assert lib.zf_latent_sample(99, 0.0, 1, z.ptr, 4, 2, None) == -1
    assert lib.zf_latent_sample(L.ZF_LATENT_NORMAL, 0.0, 1, z.ptr, 0, 2, None) == 0


@pytest.mark.parametrize("name", ["cfg2", "cfg1", "cfg4", "small", "cfg5", "h512", "h384c2"])
def test_flow_sample_equals_inverse_of_latent(name):
    """zf_flow_sample (latent drawn in the inverse kernel's prologue) ==
    Chain.inverse(Distribution.sample) bit for bit, on both fused kernels."""
    case = make_case(name, N=8, seed=43)
    cfg = case["cfg"]
    flow = build_flow(cfg)
    bf = flow.bind(case["variables"], cfg["D"], cfg["C"])
    prog = bf.program
    n = 3000
    c = None
    if cfg["C"]:
        c = L.DeviceArray.from_numpy(np.random.default_rng(5).standard_normal((n, cfg["C"])).astype(np.float32))
    seed = key_to_seed(PRNGKey(9))
    xs = prog.sample(n, seed, c).numpy()
    flow.latent._dim = cfg["D"]
    z = flow.latent.sample(n, PRNGKey(9))
    xi = prog.inverse(L.DeviceArray.from_numpy(z), c).numpy()
    assert np.array_equal(xs, xi, equal_nan=True)
    assert np.isfinite(xs).mean() > 0.99


def test_flow_sample_api_statistics():
    """Flow.sample through the API: the flow maps its latent samples back to
    data, so log_prob of the samples is finite and forward(samples) has the
    latent's moments (cfg2: Normal(0.5, 0.1) latent)."""
    case = make_case("cfg2", N=4096, seed=44)
    flow = build_flow(case["cfg"])
    flow.init(PRNGKey(0), case["x"][:1])
    xs = flow.apply(case["variables"], 20000, method="sample", seed=5)
    assert xs.shape == (20000, 4) and np.isfinite(xs).all()
    sub = {k: v["bijector"] for k, v in case["variables"].items()}
    z, _ = flow.bijector.apply(sub, xs)
    inside = np.all((z > 0.02) & (z < 0.98), axis=1)  # away from ShiftBounds clipping
    assert inside.mean() > 0.99
    np.testing.assert_allclose(z[inside].mean(0), 0.5, atol=5e-3)
    np.testing.assert_allclose(z[inside].std(0), 0.1, atol=5e-3)


# ---------------------------------------------------------------------------
# The device stream against its host restatement (tests/sampler_oracle.py).
# ---------------------------------------------------------------------------

SHAPES = [(5000, 3), (257, 1), (1000, 7)]
SEEDS = [7, 2**40 + 5]


def _device(d, n, dim, seed):
    d._dim = dim
    return d.sample(n, PRNGKey(seed))


@pytest.mark.parametrize("n,dim", SHAPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_uniform_bit_equal_to_oracle(n, dim, seed):
    """Philox words, counter layout, key halves and the 24-bit conversion are
    exact: the device equals the restatement bit for bit."""
    z = _device(dist.Uniform(), n, dim, seed)
    ref, _ = S.sample(L.ZF_LATENT_UNIFORM, 0.0, key_to_seed(PRNGKey(seed)), n, dim)
    assert np.array_equal(z.view(np.uint32), ref.view(np.uint32))


def test_seed_upper_bits_reach_the_key():
    a = _device(dist.Uniform(), 257, 2, 5)
    b = _device(dist.Uniform(), 257, 2, 2**40 + 5)
    c = _device(dist.Uniform(), 257, 2, 2**63 + 5)
    assert not np.array_equal(a, b) and not np.array_equal(a, c) and not np.array_equal(b, c)


@pytest.mark.parametrize("n,dim", SHAPES)
@pytest.mark.parametrize("seed", SEEDS)
def test_normal_matches_oracle(n, dim, seed):
    """|z - z_ref| <= 1e-6.  r <= sqrt(-2 ln 2^-24) = 5.77; 2 ulp in logf and
    sqrtf and 2 ulp of 1 in cospif give |dn| <~ 3e-6, so |dz| <~ 3e-7 plus one
    rounding of z: about 3x margin."""
    z = _device(dist.Normal(), n, dim, seed)
    ref, _ = S.sample(L.ZF_LATENT_NORMAL, 0.0, key_to_seed(PRNGKey(seed)), n, dim)
    err = np.abs(z.astype(np.float64) - ref.astype(np.float64)).max()
    print(f"normal n={n} dim={dim} seed={seed}: max |z - z_ref| = {err:.3g}")
    assert err <= 1e-6


def test_truncated_normal_matches_oracle_through_a_retry():
    """1.2e6 rows of seed 7, dim 0 reach the one retry below that count (row
    1151898, first |n| = 5.080): the device takes the second trial's value
    there; the Normal bound holds on every row and every draw is in [0, 1]."""
    n = 1_200_000
    z = _device(dist.TruncatedNormal(), n, 1, 7)
    ref, info = S.latent_draw(L.ZF_LATENT_TRUNCNORM, 0.0, 7, np.arange(n), 0)
    assert info["trial"][1151898] == 1 and (info["trial"] > 0).sum() == 1
    second = info["n"][1]
    assert second["idx"].tolist() == [1151898]
    want = np.float32(0.5 + np.float64(np.float32(0.1)) * np.float64(second["n"][0]))
    assert ref[1151898] == want
    err = np.abs(z[:, 0].astype(np.float64) - ref.astype(np.float64))
    print(f"truncnorm: max |z - z_ref| = {err.max():.3g}, at the retried row {err[1151898]:.3g}")
    assert abs(float(z[1151898, 0]) - float(want)) <= 1e-6
    assert err.max() <= 1e-6
    assert z.min() >= 0.0 and z.max() <= 1.0


@pytest.mark.parametrize("peakness", [12.0, 3.0, 1.0])
def test_beta_matches_oracle(peakness):
    """Elements where any trial of either gamma draw has an acceptance margin
    below 1e-4, or |v| below 1e-5 in the v <= 0 test, are set aside (at most
    1e-3 of them: the restatement alone gives ~4e-4); elsewhere
    |z - z_ref| <= 5e-6 (dv <= 0.41 dn, d(v^3) / v^3 = 3 dv / v, and
    z (1 - z) <= 1/4 times the two gamma draws' relative errors)."""
    n, dim = 65536, 3
    z = _device(dist.Beta(peakness), n, dim, 7)
    ref, infos = S.sample(L.ZF_LATENT_BETA, peakness, 7, n, dim)
    tie = np.stack([S.near_ties(i, n, 1e-4, 1e-5) for i in infos], axis=1)
    trial = np.stack([i["trial"] for i in infos], axis=1)
    err = np.abs(z.astype(np.float64) - ref.astype(np.float64))
    print(f"beta({peakness}): set aside {tie.mean():.3g}, max |z - z_ref| = {err[~tie].max():.3g}, "
          f"retried {np.mean(trial > 0):.3g}")
    assert tie.mean() <= 1e-3
    assert err[~tie].max() <= 5e-6
    assert np.all(trial >= 0)
    if peakness == 1.0:
        assert (trial > 0).any()  # first-trial acceptance is ~95%: retries are compared


def test_columns_do_not_depend_on_the_width():
    """counter = (row, dim): the first two columns of a 3-wide draw are the
    2-wide draw."""
    for d in (dist.Normal(), dist.Beta(), dist.TruncatedNormal(), dist.Uniform()):
        a = _device(d, 3001, 3, 21)
        b = _device(d, 3001, 2, 21)
        assert np.array_equal(a[:, :2].view(np.uint32), b.view(np.uint32))


def test_layered_sample_second_chunk():
    """h1024k5 holds 65536 rows per chunk: at 70000 rows lay_draw_kernel runs
    a second time with row0 = 65536, and the samples still equal
    Chain.inverse of the latent's own draw bit for bit."""
    case = make_case("h1024k5", N=8, seed=43)
    cfg = case["cfg"]
    flow = build_flow(cfg)
    prog = flow.bind(case["variables"], cfg["D"], cfg["C"]).program
    n = 70000
    xs = prog.sample(n, key_to_seed(PRNGKey(9))).numpy()
    flow.latent._dim = cfg["D"]
    z = flow.latent.sample(n, PRNGKey(9))
    xi = prog.inverse(L.DeviceArray.from_numpy(z)).numpy()
    assert np.array_equal(xs, xi, equal_nan=True)
    assert np.isfinite(xs[65536:]).mean() > 0.99
    zref, _ = S.latent_draw(L.ZF_LATENT_TRUNCNORM, 0.0, key_to_seed(PRNGKey(9)), np.arange(65536, n), 0)
    assert np.abs(z[65536:, 0].astype(np.float64) - zref).max() <= 1e-6
