"""The fp64 motion estimators on the device (libviso_amd/csrc/covariance.hip, refine.hip, window.hip) where good starts and round
sizes never take them (tests/estimator_cases.py): the Levenberg-Marquardt loop's rejections, its LM_MAX_ACCEPT and LM_MAX_REJECT
exits and a record that fails after the loop ran, from far starts the restatements decide robustly; the sums at the seams of
block_sum (n around 64, 256 and 512); dropped points at the seams of the compaction to L'; and a permuted list, which the
covariance's weights tell from the sorted one."""
import numpy as np
import pytest

import libviso_amd

import covariance_ref as CR
import estimator_cases as EC
import refine_ref as RR
import window_ref as WR
from estimator_util import ambiguous, check_points
from test_gpu_covariance import _check as check_covariance
from test_gpu_refine import _check as check_refine
from window_cases import check as check_window, direct_frames

pytestmark = pytest.mark.gpu

MODES = ((1, None), (2, 0.3))


def _refine_against_restatement(X, obs, tr, inl, param, what, far=False, status=None):
    """The direct call against the restatement, record and points, in both modes; and twice, for equal bytes."""
    for mode, sigma in MODES:
        with np.errstate(all="ignore"):
            want = RR.refine(X, obs, tr, inl, param, mode, sigma)
        assert status is None or want["status"] == status, (what, want["status"])
        got, pts = libviso_amd.pose_refine(X, obs, tr, inl, param, mode=mode, sigma=sigma)
        check_refine(got, want, (what, mode), far=far)
        if want["status"] == 1:
            check_points(pts, want, (what, mode))
        else:
            assert pts.shape == (3, 0), what
        again, pts2 = libviso_amd.pose_refine(X, obs, tr, inl, param, mode=mode, sigma=sigma)
        assert got.tobytes() == again.tobytes() and pts.tobytes() == pts2.tobytes(), what
    return want


@pytest.mark.parametrize("s", sorted(EC.CASES))
def test_refine_from_a_far_start(viso, s):
    tags = EC.CASES[s]
    want = _refine_against_restatement(*EC.refine_case(s), (s, tags), far=True, status=-2 if "record_fails" in tags else 1)
    if "max_accept" in tags or "max_reject" in tags:
        assert not ambiguous(want) and want["gap"] > 1e-6      # check_refine held iters to the restatement's, exactly
    if "max_accept" in tags:
        assert want["iters"] == RR.MAX_ACCEPT


@pytest.mark.parametrize("s", sorted(EC.WINDOW_CASES))
def test_window_from_a_far_start(viso, s):
    frames, param = EC.window_case(s)
    for mode, sigma in MODES:
        with np.errstate(all="ignore"):
            want = WR.window(frames, 2, 3, param, mode, sigma)
        assert want["status"] == 1 and want["len"] == 3 and EC.tags_of(want) == EC.WINDOW_CASES[s]
        got = libviso_amd.window_refine(direct_frames(frames), param, mode=mode, sigma=sigma)
        check_window(got, want, (s, mode), far=True)
        again = libviso_amd.window_refine(direct_frames(frames), param, mode=mode, sigma=sigma)
        assert got.tobytes() == again.tobytes(), s


@pytest.mark.parametrize("n", EC.SEAMS)
def test_sums_at_the_block_sum_seams(viso, n):
    X, obs, tr, inl, param = EC.seam_case(n)
    for mode, sigma in MODES:
        got = libviso_amd.pose_covariance(X, obs, tr, inl, param, mode=mode, sigma=sigma)
        want = CR.motion_cov(X, obs, tr, inl, param, mode, sigma)
        assert want["status"] == 1 and want["n"] == n
        check_covariance(got, want, (n, mode))
    # with the outliers the refinement ends as the restatement's does (status 1 at n = 63, else -2 at the record); without, it
    # converges and every sum over the n points is in the record
    _refine_against_restatement(X, obs, tr, inl, param, (n, "outliers"), far=True, status=1 if n == 63 else -2)
    want = _refine_against_restatement(*EC.seam_case(n, clean=True), (n, "clean"), status=1)
    assert want["n"] == n and want["iters"] >= 3


def test_dropped_points_at_the_compaction_seams(viso):
    X, obs, tr, inl, param = EC.dropped_case()
    want = _refine_against_restatement(X, obs, tr, inl, param, "dropped", status=1)
    # check_refine compared n and the record, check_points the points in L''s order: the list's, less the four dropped entries
    assert want["n"] == 296 and np.array_equal(want["idx"], np.delete(inl, sorted(EC.DROPPED)))


def test_covariance_of_a_permuted_list(viso):
    X, obs, tr, inl, param = EC.permuted_case()
    for mode, sigma in MODES:
        got = libviso_amd.pose_covariance(X, obs, tr, inl, param, mode=mode, sigma=sigma)
        check_covariance(got, CR.motion_cov(X, obs, tr, inl, param, mode, sigma), ("permuted", mode))
        # entry j's weight comes from the observation in column j, not inl[j] (cov_point's j against its k): the sorted list gives
        # another record, by far more than the 1e-9 the device is held to
        sorted_want = CR.motion_cov(X, obs, tr, np.sort(inl), param, mode, sigma)
        assert CR.whitened_error(sorted_want["cov"], np.asarray(got["cov"])) > 1e-6, mode
