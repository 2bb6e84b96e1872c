"""cpu: the float64 mixture oracle's own properties (tests/mixture_oracle.py), the numpy restatement of gr_mixture_dev's operation chains against it
within the bounds derived from those chains (tests/mixture_paths.py) on the shapes tests/test_gpu_mixture.py runs, and the bindings and options."""
import numpy as np
import pytest

import mixture_oracle as mo
import mixture_paths as mp

# the shapes of tests/test_gpu_mixture.py: block edges, one that crosses the partial sets' boundary, columns, components
ROW_SHAPES = [(2, 1, 1), (511, 5, 2), (512, 5, 2), (513, 5, 2), (512 * (mp.P + 1) + 3, 2, 2)]
COLUMN_SHAPES = [(700, d, 3) for d in (1, 3, 100, 255, 256)]
COMPONENT_SHAPES = [(1500, 32, k) for k in (1, 2, 31, 32, 33, 255, 256)]
SHAPES = ROW_SHAPES + COLUMN_SHAPES + COMPONENT_SHAPES
EXCLUDED_SHARE = 0.02


def worst(err, bound):
    """max err / bound; an element whose bound is 0 must be exact"""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert np.isfinite(err).all()
    assert not (err[bound == 0] != 0).any()
    return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def case(n, d, k):
    """(x, weights, means, variances, var_floor) of a shape: blobs 6 sigma apart, parameters a few steps from a fit"""
    x, _ = mo.blobs(n, d, k, seed=3)
    return (x,) + mo.spread_start(x, k, seed=n + d) + (np.float32(1e-3),)


def check_e_step(got, x, w, mu, var, name):
    """got: dict(rowll, labels, post, loglik) from the code under test (rowll and post as float64 or float32) -> the worst ratio"""
    ref = mo.e_step(x, w, mu, var)
    lb = mp.ell_bound(x, w, mu, var)
    as_float = np.asarray(got["rowll"]).dtype == np.float32
    ratios = dict(rowll=worst(np.abs(got["rowll"].astype(np.float64) - ref["rowll"]), mp.rowll_bound(ref, lb, as_float=as_float)),
                  loglik=worst(abs(got["loglik"] - ref["loglik"]), mp.loglik_bound(ref, lb)))
    decided = mp.decided_rows(ref, lb)
    excluded = 1.0 - decided.mean()
    assert excluded <= EXCLUDED_SHARE, f"{name}: {excluded:.3%} of the rows have no decided label"
    assert np.array_equal(np.asarray(got["labels"])[decided], ref["labels"][decided])
    same = decided & (np.asarray(got["labels"]) == ref["labels"])
    ratios["post"] = worst(np.abs(got["post"].astype(np.float64) - ref["post"])[same], mp.post_bound(ref, lb)[same])
    print(f"{name}: E-step err / bound " + ", ".join(f"{q} {v:.3g}" for q, v in ratios.items()) + f"; rows without a decided label {excluded:.3%}")
    assert max(ratios.values()) <= 1
    return ratios, as_float


def check_m_step(got, x, w, mu, var, var_floor, name):
    """got: (weights', means', variances') from the code under test -> the worst ratio"""
    ref_e = mo.e_step(x, w, mu, var)
    lb = mp.ell_bound(x, w, mu, var)
    rw, rmu, rvar = mo.m_step(x, ref_e["r"], w, mu, var, float(var_floor))
    b = mp.m_step_bounds(x, ref_e, lb, mu, float(var_floor))
    assert (np.abs(b["big_n"] - 1.0) > b["big_n_bound"]).all(), "a component on the edge of N_j = 1: choose other inputs"
    ratios = dict(weights=worst(np.abs(got[0].astype(np.float64) - rw), b["weights"]), means=worst(np.abs(got[1].astype(np.float64) - rmu), b["means"]),
                  variances=worst(np.abs(got[2].astype(np.float64) - rvar), b["variances"]))
    print(f"{name}: M-step err / bound " + ", ".join(f"{q} {v:.3g}" for q, v in ratios.items()))
    assert max(ratios.values()) <= 1
    return ratios


# ------------------------------------------------------------------ 1. the oracle
def test_one_component_one_iteration_is_mean_and_biased_variance():
    x, _ = mo.blobs(300, 4, 2, seed=1)
    w0, mu0, var0 = mo.start(x, x[:1])
    w, mu, var, hist, _ = mo.fit(x, w0, mu0, var0, 1, 1e-9)
    x64 = x.astype(np.float64)
    assert np.allclose(mu[0], x64.mean(axis=0), rtol=1e-13, atol=0) and np.allclose(var[0], x64.var(axis=0), rtol=1e-12, atol=0)
    assert w.tolist() == [1.0] and len(hist) == 2


@pytest.mark.parametrize("n,d,k", [(700, 8, 3), (513, 5, 2), (2000, 100, 20)])
def test_loglik_never_decreases_and_the_weights_sum_to_one(n, d, k):
    x, centres = mo.blobs(n, d, k, seed=2)
    w0, mu0, var0 = mo.start(x, x[:k])
    floor = 1e-9
    w, mu, var, hist, _ = mo.fit(x, w0, mu0, var0, 6, floor)
    assert (var > floor).all()                                          # the floor never bound: EM's guarantee applies
    assert (np.diff(hist) >= -1e-12 * np.abs(hist[:-1])).all(), hist
    assert abs(w.sum() - 1.0) <= 1e-12


def test_a_far_away_component_keeps_its_parameters_and_gets_weight_zero():
    x, _ = mo.blobs(400, 3, 2, seed=4)
    w0, mu0, var0 = mo.start(x, np.concatenate([x[:2], np.full((1, 3), 1e4, np.float32)]))
    var0[2] = 0.01                                                      # narrow and far: its density underflows for every row
    e = mo.e_step(x, w0, mu0, var0)
    assert not e["r"][:, 2].any()
    w, mu, var = mo.m_step(x, e["r"], w0, mu0, var0, 1e-6)
    assert w[2] == 0.0 and np.array_equal(mu[2], mu0[2].astype(np.float64)) and np.array_equal(var[2], var0[2].astype(np.float64))
    e2 = mo.e_step(x, w, mu, var)                                       # dead from here on: l = -inf, and the rest is finite
    assert np.isneginf(e2["l"][:, 2]).all() and np.isfinite(e2["rowll"]).all()


def test_first_maximum_is_the_label():
    x = np.zeros((4, 2), np.float32)
    w, mu, var = np.full(3, 1 / 3, np.float32), np.zeros((3, 2), np.float32), np.ones((3, 2), np.float32)
    assert mo.e_step(x, w, mu, var)["labels"].tolist() == [0, 0, 0, 0]
    assert mp.e_step(x, w, mu, var)["labels"].tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------ 2. the restated chains against the oracle, within the derived bounds
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_restated_steps_hold_the_bounds(n, d, k):
    x, w, mu, var, floor = case(n, d, k)
    check_e_step(mp.e_step(x, w, mu, var), x, w, mu, var, f"({n}, {d}, {k})")
    check_m_step(mp.m_step(x, w, mu, var, floor), x, w, mu, var, floor, f"({n}, {d}, {k})")


@pytest.mark.parametrize("n,d,k", [(700, 8, 3), (513, 5, 2), (2000, 100, 20), (1500, 32, 256)])
def test_undecided_rows_stay_rare_over_six_iterations(n, d, k):
    """the label comparison's exclusion, on the oracle alone: blobs 6 sigma apart, first-row initial means"""
    x, _ = mo.blobs(n, d, k, seed=2)
    w, mu, var = (a.astype(np.float64) for a in mo.start(x, x[:k]))
    for it in range(7):
        e = mo.e_step(x, w, mu, var)
        share = 1.0 - mp.decided_rows(e, mp.ell_bound(x, w, mu, var)).mean()
        assert share <= EXCLUDED_SHARE, (it, share)
        w, mu, var = mo.m_step(x, e["r"], w, mu, var, 1e-9)


# ------------------------------------------------------------------ 3. bindings and options
def test_the_library_exports_and_binds_the_mixture():
    import ganrev._lib as L
    from ganrev import mixture
    assert "gr_mixture_dev" in L._SIGS and "gr_cluster_members_wide_dev" in L._SIGS
    assert callable(L.Context.mixture_dev) and callable(L.Context.cluster_members_wide_dev)
    assert callable(mixture.fit) and callable(mixture.score) and mixture.Mixture
    lib = L.load_library()
    assert lib.gr_mixture_dev and lib.gr_cluster_members_wide_dev


def test_mixture_with_host_is_refused_by_name(capsys):
    from ganrev import apply_r
    with pytest.raises(SystemExit):
        apply_r.parse(["--synthetic", "3x32x32x32", "--host", "--mixture", "4"])
    assert "--mixture" in capsys.readouterr().err


def test_more_than_256_components_are_refused_by_name(capsys):
    from ganrev import apply_r
    with pytest.raises(SystemExit):
        apply_r.parse(["--synthetic", "3x32x32x32", "--nbClusters", "257", "--mixture", "4"])
    err = capsys.readouterr().err
    assert "257" in err and "--mixture" in err
    assert apply_r.mixtureOptions(apply_r.parse(["--synthetic", "3x32x32x32", "--nbClusters", "256", "--mixture", "0"])) == 0
    assert apply_r.mixtureOptions(apply_r.parse(["--synthetic", "3x32x32x32"])) is None
