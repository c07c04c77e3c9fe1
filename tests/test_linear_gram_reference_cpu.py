"""linear_gram_cases.gram_reference against the host linear learner (device_type=cpu): the ridge
solve of the reference's Gram system of every leaf of a second tree reproduces the model's leaf
coefficients and constants, without NaNs and with about 2 % of them. This validates the
reference (kept rows, [A | c], the usable count's threshold) before test_linear_gram_kernel.py
lets it judge the HIP kernels.

Measured once on the CPU: the largest discrepancy max |model - reference| / max |reference| over a
leaf's unknowns was 3.24e-14 without NaNs and 4.07e-14 with them (fp64 sums and an fp64 Cholesky
on the host against np.longdouble here); the tolerance is ten times the larger, 4.07e-13."""
import numpy as np
import pytest

import lambdagap_amd as lgb

import linear_gram_cases as lc

MEASURED = 4.07e-14
RTOL = 10 * MEASURED
LR, LAMBDA = 0.1, 0.01


def _solve(A, c, lam):
    """z = -(A + lam diag(1, .., 1, 0))^-1 c by Cholesky in np.longdouble."""
    m = c.size
    A = A.copy()
    for j in range(m - 1):
        A[j, j] += lam
    L = np.zeros_like(A)
    for i in range(m):
        for j in range(i + 1):
            s = A[i, j] - (L[i, :j] * L[j, :j]).sum()
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    y = np.zeros(m, dtype=np.longdouble)
    for i in range(m):
        y[i] = (-c[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    z = np.zeros(m, dtype=np.longdouble)
    for i in range(m - 1, -1, -1):
        z[i] = (y[i] - (L[i + 1:, i] * z[i + 1:]).sum()) / L[i, i]
    return z


def _leaves(node, path, out):
    if "split_index" in node:
        _leaves(node["left_child"], path + [node["split_feature"]], out)
        _leaves(node["right_child"], path + [node["split_feature"]], out)
    else:
        out[node["leaf_index"]] = (sorted(set(path)), node)
    return out


@pytest.mark.parametrize("with_nan", [False, True])
def test_leaf_models_solve_the_reference_system(with_nan):
    rng = np.random.default_rng(31)
    n, f = 6000, 6
    X = rng.standard_normal((n, f)).astype(np.float32)
    y = (X[:, 0] * np.where(X[:, 1] > 0, 2.0, -1.0) + 0.7 * X[:, 2] + np.abs(X[:, 3]) + 0.5 * X[:, 4] * X[:, 5]
         + 0.1 * rng.standard_normal(n)).astype(np.float32)
    if with_nan:
        X[rng.random((n, f)) < 0.02] = np.nan
    params = {"objective": "regression", "linear_tree": True, "linear_lambda": LAMBDA, "learning_rate": LR,
              "num_leaves": 12, "min_data_in_leaf": 60, "device_type": "cpu", "verbosity": -1, "seed": 2}
    b = lgb.train(params, lgb.Dataset(X.astype(np.float64), y, params=params), 2)
    assert b.num_trees() == 2
    # the second tree's gradients: fp32 (score - label) of the first tree's scores, h = 1
    s1 = b.predict(X.astype(np.float64), num_iteration=1, raw_score=True)
    g = (s1 - y.astype(np.float64)).astype(np.float32)
    h = np.ones(n, dtype=np.float32)
    leaf_of = np.asarray(b.predict(X.astype(np.float64), pred_leaf=True)).reshape(n, -1)[:, 1]
    leaves = _leaves(b.dump_model()["tree_info"][1]["tree_structure"], [], {})
    assert len(leaves) > 6
    worst = 0.0
    for leaf, (feats, node) in sorted(leaves.items()):
        rows = np.flatnonzero(leaf_of == leaf)
        assert rows.size == node["leaf_count"]
        A, c, usable, _, _ = lc.gram_reference(X, g, h, rows, feats)
        k = len(feats)
        assert k >= 1 and (usable if with_nan else rows.size) >= k + 1
        z = _solve(A, c, np.longdouble(LAMBDA)) * LR
        got = np.zeros(k + 1, dtype=np.longdouble)
        for fi, co in zip(node["leaf_features"], node["leaf_coeff"]):
            got[feats.index(fi)] = co
        got[k] = node["leaf_const"]
        assert len(node["leaf_features"]) == k, (leaf, node["leaf_features"], feats)
        err = float(np.abs(got - z).max() / np.abs(z).max())
        worst = max(worst, err)
        assert err <= RTOL, (leaf, feats, err, got.astype(float), z.astype(float))
    print(f"with_nan={with_nan}: worst relative discrepancy {worst:.3g}")
