"""numpy fp64 oracles and seeded scenes for the homography / warp tests (tests/test_homography_cpu.py, tests/test_gpu_homography.py,
tests/test_gpu_warp.py).  Written from the formulas of include/gim_hip.h, independent of gim_amd/pose.py and of the kernels:

  transfer_error:  |dst - proj(H src)|^2, inf where w == 0 or the value is not finite
  warp_oracle:     dst(x, y) = sum over the four neighbours of floor(u, v) of the exact bilinear weight times the source pixel, a
                   neighbour outside the source contributing 0; (u, v) = proj(H^-1 (x, y, 1)); 0 where w == 0 or (u, v) is not finite.
                   Everything in fp64, nothing rounded: the caller rounds (rint for uint8) and bounds the difference."""
import numpy as np

W, H_IMG = 640, 480
CORNERS = np.array([[0.0, 0.0], [W - 1.0, 0.0], [W - 1.0, H_IMG - 1.0], [0.0, H_IMG - 1.0]])


def proj(H, p):
    """H [3,3], p [P,2] -> [P,2] (plain division: inf / nan where w == 0)"""
    q = np.concatenate([p, np.ones((len(p), 1))], 1) @ np.asarray(H, dtype=np.float64).T
    with np.errstate(all="ignore"):
        return q[:, :2] / q[:, 2:]


def transfer_error(H, src, dst):
    """H [..., 3, 3], src / dst [P, 2] -> [..., P]"""
    H = np.asarray(H, dtype=np.float64)
    x, y = src[:, 0], src[:, 1]
    h = lambda i, j: H[..., i, j, None]   # noqa: E731
    w = h(2, 0) * x + h(2, 1) * y + h(2, 2)
    with np.errstate(all="ignore"):
        ex = dst[:, 0] - (h(0, 0) * x + h(0, 1) * y + h(0, 2)) / w
        ey = dst[:, 1] - (h(1, 0) * x + h(1, 1) * y + h(1, 2)) / w
        e = ex * ex + ey * ey
    return np.where((w != 0) & np.isfinite(e), e, np.inf)


def corner_error(H, H_true):
    """largest distance, in pixels, between the images of the four frame corners under H and under the truth"""
    return float(np.sqrt(((proj(H, CORNERS) - proj(H_true, CORNERS)) ** 2).sum(1)).max())


def warp_oracle(image, H, out_hw):
    """image [C, Hs, Ws] (any real dtype), H [3, 3] mapping image pixels to output pixels -> fp64 [C, Hd, Wd], unrounded"""
    img = np.asarray(image, dtype=np.float64)
    C, Hs, Ws = img.shape
    Hd, Wd = out_hw
    Hi = np.linalg.inv(np.asarray(H, dtype=np.float64))
    ys, xs = np.mgrid[0:Hd, 0:Wd].astype(np.float64)
    with np.errstate(all="ignore"):
        w = Hi[2, 0] * xs + Hi[2, 1] * ys + Hi[2, 2]
        u = (Hi[0, 0] * xs + Hi[0, 1] * ys + Hi[0, 2]) / w
        v = (Hi[1, 0] * xs + Hi[1, 1] * ys + Hi[1, 2]) / w
    ok = (w != 0) & np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 1e9) & (np.abs(v) < 1e9)
    u, v = np.where(ok, u, -10.0), np.where(ok, v, -10.0)
    x0, y0 = np.floor(u), np.floor(v)
    ax, ay = u - x0, v - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    out = np.zeros((C, Hd, Wd))
    for dy, wy in ((0, 1.0 - ay), (1, ay)):
        for dx, wx in ((0, 1.0 - ax), (1, ax)):
            xx, yy = x0 + dx, y0 + dy
            inside = ok & (xx >= 0) & (xx < Ws) & (yy >= 0) & (yy < Hs)
            px = img[:, np.clip(yy, 0, Hs - 1), np.clip(xx, 0, Ws - 1)]
            out += np.where(inside, wx * wy, 0.0) * px
    return out


# ---- seeded scenes -----------------------------------------------------------------------------------------------------------
def general_h(rng):
    """a general projective H of the 640 x 480 frame: rotation, anisotropic scale, shear, shift and perspective terms that keep w
    within [0.7, 1.4] over the frame"""
    a = rng.uniform(-0.4, 0.4)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    A = R @ np.array([[rng.uniform(0.8, 1.25), rng.uniform(-0.15, 0.15)], [0.0, rng.uniform(0.8, 1.25)]])
    H = np.eye(3)
    H[:2, :2] = A
    H[:2, 2] = rng.uniform(-60, 60, 2)
    H[2, :2] = rng.uniform(-3e-4, 3e-4, 2)
    return H


def decidable_scene(seed, P=300, inlier_share=0.6, min_dist=5.0):
    """P matches src -> dst in the frame: the outliers first (each at least `min_dist` px from its true transfer, redrawn until it
    is), then the exact inliers of a known H, then shuffled.  -> (H_true, src [P,2], dst [P,2], truth bool [P])"""
    rng = np.random.default_rng(seed)
    H = general_h(rng)
    n_out = P - int(round(inlier_share * P))
    src = rng.uniform([0, 0], [W, H_IMG], (P, 2))
    dst = proj(H, src)
    out = rng.uniform([0, 0], [W, H_IMG], (n_out, 2))
    while True:
        near = np.sqrt(((out - dst[:n_out]) ** 2).sum(1)) < min_dist
        if not near.any():
            break
        out[near] = rng.uniform([0, 0], [W, H_IMG], (int(near.sum()), 2))
    assert (np.sqrt(((out - dst[:n_out]) ** 2).sum(1)) >= min_dist).all()
    dst[:n_out] = out
    truth = np.arange(P) >= n_out
    perm = rng.permutation(P)
    return H, np.ascontiguousarray(src[perm]), np.ascontiguousarray(dst[perm]), truth[perm]
