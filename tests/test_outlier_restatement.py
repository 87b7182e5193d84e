"""The numpy restatement of StatisticalOutlierRemoval / RadiusOutlierRemoval (tests/outlier_restatement.py) pinned to the
reference's own answers on bun0 (tests/golden/outlier_removal_bun0.json): the GPU tests compare with it."""
import json
import os

import numpy as np
import pytest

import outlier_restatement as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "outlier_removal_bun0.json")) as f:
        return json.load(f)


def test_sor_bun0(bunny, gold):
    b = bunny["bun0"][:, :3]
    g = gold["sor"]
    r = rs.statistical_outlier_removal(b, g["mean_k"], g["std_mul"])
    assert len(r["kept"]) == g["kept"] and len(r["removed"]) == len(b) - g["kept"]
    np.testing.assert_allclose(b[r["kept"][-1]], g["last_kept"], atol=1e-4)
    assert r["valid"] == len(b)
    rn = rs.statistical_outlier_removal(b, g["mean_k"], g["std_mul"], negative=True)
    assert len(rn["kept"]) == g["negative_kept"]
    np.testing.assert_allclose(b[rn["kept"][-1]], g["negative_last_kept"], atol=1e-4)
    assert np.array_equal(np.sort(np.concatenate([r["kept"], rn["kept"]])), np.arange(len(b)))


def test_ror_bun0(bunny, gold):
    b = bunny["bun0"][:, :3]
    g = gold["ror"]
    r = rs.radius_outlier_removal(b, g["radius"], g["min_pts"])
    assert len(r["kept"]) == g["kept"]
    np.testing.assert_allclose(b[r["kept"][-1]], g["last_kept"], atol=1e-4)
    rn = rs.radius_outlier_removal(b, g["radius"], g["min_pts"], negative=True)
    assert len(rn["kept"]) == g["negative_kept"]
    # bun0 is dense and has no point at the boundary: the radiusSearch rule gives the same answer
    assert np.array_equal(rs.radius_outlier_removal(b, g["radius"], g["min_pts"], dense=False)["kept"], r["kept"])


def test_restatement_edges():
    nan = np.float32("nan")
    c = np.array([[0, 0, 0], [nan, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    r = rs.statistical_outlier_removal(c, 50, 1.0)
    assert r["valid"] == 3 and r["dist"][1] == 0.0
    assert 1 in r["kept"]  # a NaN point is kept when negative is off
    one = rs.statistical_outlier_removal(c[:1], 5, 1.0)  # K = 1: 0 / 0
    assert np.isnan(one["dist"][0]) and list(one["kept"]) == [0]
    # lattice at spacing 0.5: d2 == r*r exactly; dense keeps the neighbour, non-dense does not
    lat = np.array([[0, 0, 0], [0.5, 0, 0]], np.float32)
    assert len(rs.radius_outlier_removal(lat, 0.5, 1, dense=True)["kept"]) == 2
    assert len(rs.radius_outlier_removal(lat, 0.5, 1, dense=False)["kept"]) == 0
    assert list(rs.radius_outlier_removal(c, 2.0, 1, dense=False, negative=True)["kept"]) == []
    assert 1 in rs.radius_outlier_removal(c, 2.0, 5, dense=True, negative=True)["kept"]
