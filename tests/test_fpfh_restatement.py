"""tests/fpfh_restatement.py pinned on the reference's own numbers (tests/golden/fpfh_bun0.json: the three golden blocks of
test/features/test_pfh_estimation.cpp on bun0) and on the properties the GPU tests of tests/test_gpu_fpfh.py lean on."""
import json
import os

import numpy as np
import pytest

import fpfh_restatement as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(ROOT, "tests", "golden", "fpfh_bun0.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def bun0():
    return fr.load_bun0()


@pytest.fixture(scope="module")
def restated(bun0):
    pts, nrm = bun0
    return {r: fr.restate(pts, nrm, r) for r in (0.02, 1.0)}


def test_bun0_file_is_the_fixture_cloud(bun0, bunny):
    pts, nrm = bun0
    assert np.array_equal(pts, bunny["bun0"][:, :3]) and np.array_equal(nrm, bunny["bun0"][:, 3:6])


def test_spfh_row0_is_the_reference(restated, gold):
    r = restated[1.0]
    assert (r["m"] == 397).all()  # the neighbourhood of the reference's test: every point
    g = gold["spfh_row0"]
    assert np.abs(r["spfh"][0] - np.array(g["values"])).max() <= g["tolerance"]


def test_weighting_is_the_reference(restated, gold):
    spfh = restated[1.0]["spfh"]
    g = gold["weighted"]
    got = fr.weight_float32(spfh, np.arange(397), np.arange(397, dtype=np.float32))
    assert np.abs(got - np.array(g["values"])).max() <= g["tolerance"]


def test_fpfhs0_is_the_reference(restated, gold):
    g = gold["fpfhs0"]
    assert np.abs(restated[1.0]["fpfh32"][0] - np.array(g["values"])).max() <= g["tolerance"]


@pytest.mark.parametrize("radius", [0.02, 1.0])
def test_float32_and_float64_bin_alike_outside_the_unstable_set(restated, radius):
    r = restated[radius]
    print("r = %g: %d pairs, %d points own an unstable pair, %d stable pairs binned differently" %
          (radius, r["pairs"], int((r["unstable"] > 0).sum()), int(r["disagree"].sum())))
    assert r["disagree"].sum() == 0
    assert (r["unstable"] > 0).mean() <= 0.10
    # and inside it: a pair moves at most one hit in each of its three histograms
    l1 = np.abs(r["counts"] - r["counts64"]).sum(axis=1)
    assert (l1 <= 6 * r["unstable"]).all()


@pytest.mark.parametrize("radius", [0.02, 1.0])
def test_reference_order_sits_inside_the_summation_bound(restated, radius):
    """float32 ascending-order FPFH against the float64 one: within (m + 4) * 2^-24 * 100 per bin -- a sequential float sum
    of m non-negative products (one rounding each), bins summing to 100, the normaliser and the final rounding."""
    r = restated[radius]
    bound = (r["m"] + 4) * 2.0 ** -24 * 100.0
    err = np.abs(r["fpfh32"].astype(np.float64) - r["fpfh64"]).max(axis=1)
    print("r = %g: largest error / bound = %.3f" % (radius, float((err / bound).max())))
    assert (err <= bound).all()


def test_counts_are_recovered_from_rows(restated):
    r = restated[0.02]
    assert np.array_equal(fr.counts_from_rows(r["spfh"], r["m"]), r["counts"])


def test_edge_cases():
    rng = np.random.default_rng(5)
    pts = rng.uniform(0, 1, (40, 3)).astype(np.float32)
    nrm = rng.normal(size=(40, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    pts[7] = pts[3]          # an exact duplicate
    pts[11] = (50, 50, 50)   # isolated
    pts[13] = np.nan         # dropped
    nrm[17] = np.nan
    r = fr.restate(pts, nrm, 0.4)
    assert (r["spfh"][11] == 0).all() and (r["fpfh32"][11] == 0).all()
    assert np.isnan(r["spfh"][13]).all() and np.isnan(r["fpfh32"][13]).all()
    assert np.isnan(r["spfh"][17]).all() and np.isnan(r["fpfh32"][17]).all()
    for b in (5, 16, 27):
        assert r["counts"][3, b] >= 1 and r["counts"][7, b] >= 1
