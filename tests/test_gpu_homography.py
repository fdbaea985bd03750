"""find_homography_block (csrc/geom.hip) on the constructed inputs of tests/homography_cases.py (what each case forces is proved in
tests/test_homography_cases_cpu.py): alone through eagle_op_find_homography with each case's own threshold, iteration bound and LM steps, and inside
post_kernel (another LDS offset) through eagle_op_post.  The reference is oracle.prims.find_homography_ransac with the same parameters and EVERY comparison is
exact: the flag, the inlier mask and the nine doubles of H.  One launch of one workgroup per case."""
import numpy as np
import pytest

import homography_cases as HC

pytestmark = pytest.mark.gpu

CASES = HC.cases()
HEAT = HC.heat_cases()
_expected = {}


def expected(name):
    if name not in _expected:
        from oracle import prims as P
        c = CASES[name]
        _expected[name] = P.find_homography_ransac(c["img"], c["world"], c["thresh"], c["max_iters"], 0.995, c["lm_iters"])
    return _expected[name]


def solve(name):
    from eagle_amd import lib
    c = CASES[name]
    return lib.op_find_homography(c["img"], c["world"], c["thresh"], c["max_iters"], c["lm_iters"])


@pytest.mark.parametrize("name", list(CASES))
def test_solver_alone(name):
    H0, m0 = expected(name)
    H1, m1 = solve(name)
    assert (H0 is None) == (H1 is None), f"ok: oracle {H0 is not None}, kernel {H1 is not None}"
    if H0 is not None:
        assert np.array_equal(m0, m1), f"mask: oracle {m0.tolist()}, kernel {m1.tolist()}"
        assert np.array_equal(H0, H1), f"H differs by {np.abs(H0 - H1).max()}"


def test_whole_list_twice_gives_identical_bytes():
    def sweep():
        out = []
        for name in CASES:
            H, m = solve(name)
            out.append(b"none" if H is None else H.tobytes() + m.tobytes())
        return out
    a, b = sweep(), sweep()
    assert [n for n, x, y in zip(CASES, a, b) if x != y] == []


def test_88_points_are_refused():
    from eagle_amd import lib
    img, world = HC.garbage_points(1, HC.MAX_KP + 1)
    with pytest.raises(lib.EagleError):
        lib.op_find_homography(img, world)


# the solver's parameters are launch parameters of post_kernel: the ordinary case runs with values of its own
HEAT_PARAMS = {"heat_camera": (0.5, 300, 3), "heat_reject_1000_after_50_iterations": (5.0, 2000, 10), "heat_past_table_best_after": (5.0, 2000, 10)}


@pytest.mark.parametrize("name", list(HEAT))
def test_solver_inside_post_kernel(name):
    from eagle_amd import lib
    from eagle_amd.pitch import LANDMARKS
    from oracle import prims as P
    c = HEAT[name]
    thresh, max_iters, lm_iters = HEAT_PARAMS[name]
    parts = np.zeros((1, 1, 64), lib.PART_DTYPE)
    parts["score"] = -1.0; parts["idx"] = 0x7fffffff
    parts["score"][0, 0, :57] = c["score"]; parts["idx"][0, 0, :57] = c["idx"]
    out, _ = lib.op_post(HC.HM, HC.FRAME, parts=parts, ransac_thresh=thresh, ransac_max_iters=max_iters, lm_iters=lm_iters)
    rec = out[0]
    kp = rec["kp"][:int(rec["n_kp"])]
    kp = kp[kp["on_plane"] != 0]                                                # the solver's input, in the record's own order
    img = np.stack([kp["x"], kp["y"]], 1).astype(np.float32)
    world = np.array([[LANDMARKS[int(l)][2], LANDMARKS[int(l)][3]] for l in kp["label"]], np.float32)
    e_img, e_world, _ = HC.heat_points(c)
    assert np.array_equal(img, e_img) and np.array_equal(world, e_world), "the record's points are not the case's (decode / synthesis: tests/test_gpu_tail.py)"
    H0, m0 = P.find_homography_ransac(img, world, thresh, max_iters, 0.995, lm_iters)
    assert bool(rec["H_valid"]) == (H0 is not None)
    if H0 is None:
        assert not rec["H"].any() and not kp["inlier"].any()
    else:
        assert np.array_equal(kp["inlier"], m0), f"inlier flags: oracle {m0.tolist()}, kernel {kp['inlier'].tolist()}"
        assert np.array_equal(rec["H"].reshape(3, 3), H0), f"H differs by {np.abs(rec['H'].reshape(3, 3) - H0).max()}"
