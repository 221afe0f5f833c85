"""numpy float32 restatement of the cut planes' predicate (include/svr.h, "cut planes": svr_set_cut_planes), in the
operation order stated there, for both modes.  The predicate is a function of the ray and of the float counter ``iter``,
not of the sample's position or value: composite_twin and iso_twin take ``cut_planes`` / ``cut_mode`` and ask a
``RayCut`` of their rays which counters are cut."""
import numpy as np

from twin_common import _dot

f32 = np.float32
MAX_CUT_PLANES = 8


def host_planes(planes, world):
    """The per-call host part: (g [K, 3], h [K], nhat [K, 3]) in f32 for ``planes`` (K x abcd, world space) and the
    row-major ``world`` matrix (m[4c + r] of the header is world[r, c])."""
    P = np.asarray(planes, f32).reshape(-1, 4)
    W = np.asarray(world, f32)
    g = np.zeros((len(P), 3), f32)
    h = np.zeros(len(P), f32)
    nhat = np.zeros((len(P), 3), f32)
    for k, (a, b, c, d) in enumerate(P):
        for j in range(3):
            g[k, j] = (W[0, j] * a + W[1, j] * b) + W[2, j] * c
        h[k] = ((W[0, 3] * a + W[1, 3] * b) + W[2, 3] * c) - d
        ln = np.sqrt((a * a + b * b) + c * c)
        nhat[k] = (a / ln, b / ln, c / ln)
    return g, h, nhat


class RayCut:
    """A_k and B_k of every ray of a set-up ``S`` (twin_common.setup_rays), and the predicate on them."""

    def __init__(self, S, planes, mode):
        self.all = str(mode).upper() == "ALL"
        assert self.all or str(mode).upper() == "ANY", mode
        self.g, self.h, self.nhat = host_planes(planes, S["world"])
        assert len(self.g) <= MAX_CUT_PLANES
        size = S["size"]
        p0 = [S["start"][a] * size[a] - f32(0.5) for a in range(3)]
        sd = [S["step"][a] * size[a] for a in range(3)]
        self.A = [_dot(list(g), p0) + h for g, h in zip(self.g, self.h)]
        self.B = [_dot(list(g), sd) for g in self.g]

    def __len__(self):
        return len(self.g)

    def behind(self, k, iters, at=None):
        """behind_k(iter) for the rays ``at`` (an index tuple; default all), ``iters`` a scalar or one per ray."""
        A, B = (self.A[k], self.B[k]) if at is None else (self.A[k][at], self.B[k][at])
        return (A + f32(iters) * B if np.isscalar(iters) else A + iters.astype(f32) * B) < f32(0.0)

    def cut(self, iters, at=None):
        """Is the counter cut away?  ``False`` without planes."""
        if not len(self):
            return np.False_
        behind = [self.behind(k, iters, at) for k in range(len(self))]
        return np.logical_and.reduce(behind) if self.all else np.logical_or.reduce(behind)
