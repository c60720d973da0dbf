"""The planted scene of the triangulation tests: cameras on a line (every
second one SIMPLE_RADIAL), one keypoint pool over their images, and match edges
that hold every case the track builder and the per-track RANSAC distinguish.
Built from fixed numpy seeds; nothing here touches the GPU."""
import numpy as np

import triangulate_ref as tr

ITERS, THR, MIN_ANGLE, MAX_TRACK = 64, 4.0, 1.5, 64
# Picked together so that the preconditions of the device comparison hold
# (tests/test_gpu_triangulate.py asserts them on the restatement): above all,
# none of the 64 pairs the sampler draws for the MAX_TRACK-row component takes
# two rows of one image.  Such a pair triangulates the camera centre, where the
# depth is 0 up to rounding and the sign test has no margin.  About one sampler
# seed in 400 qualifies for a given scene.
FIXTURE_SEED, SEED = 1, 141
# The second call of the GPU test: one kept component of LONG_ROWS rows (a real
# 9-view track inside junk), more members than a wave has lanes, so every
# lane-strided loop of the wave kernel takes several passes.  max_track = 64
# cannot hold such a track, so it gets its own edges and its own call with
# LONG_MAX_TRACK; LONG_SEED is picked like SEED (no same-image pair among the 64
# drawn, and at least one draw inside the real track).
LONG_ROWS, LONG_MAX_TRACK, LONG_SEED = 140, 160, 2465
NCAM = 9                                      # sets 0..8 on the line; set 9 sits 0.002 from set 0
SET_SIZES = [300, 2049, 120, 60, 250, 97, 180, 133, 64, 70]


class Builder:
    def __init__(self, seed):
        self.rng = np.random.RandomState(seed)
        cams, poses = tr.line_cameras(NCAM)
        R9, C9 = tr.rot_y(-2.0), np.array([0.002, 0.0, 0.0])
        c9, p9 = cams[:1].copy(), np.concatenate([R9, (-R9 @ C9)[:, None]], 1).reshape(1, 12)
        self.cams, self.poses = np.concatenate([cams, c9]), np.concatenate([poses, p9])
        self.set_off = np.concatenate([[0], np.cumsum(SET_SIZES)]).astype(np.int32)
        N = int(self.set_off[-1])
        # isolated rows keep these random pixels
        self.kp = np.stack([self.rng.uniform(0, 640, N), self.rng.uniform(0, 480, N)], 1).astype(
            np.float32)
        self.free = [list(self.set_off[s] + self.rng.permutation(SET_SIZES[s]))
                     for s in range(len(SET_SIZES))]
        self.edges = []
        self.cases = {}                       # name -> list of dicts(rows=..., X=...)

    def row(self, s, xy=None):
        r = int(self.free[s].pop())
        if xy is not None:
            self.kp[r] = xy
        return r

    def point(self, views, depth):
        """a point in front of the middle of the cameras ``views``"""
        mid = 0.45 * float(np.mean([v for v in views if v < NCAM] or [0]))
        return np.array([mid + self.rng.uniform(-0.25, 0.25) * depth / 3.0,
                         self.rng.uniform(-0.2, 0.2) * depth / 3.0, depth])

    def track(self, case, views, depth, sigma=0.0, edges="tree"):
        X = self.point(views, depth)
        rows = [self.row(s, tr.observe(self.cams[s], self.poses[s], X, self.rng, sigma))
                for s in views]
        if edges == "chain":
            for k in range(len(rows) - 1):
                e = (rows[k], rows[k + 1])
                self.edges.append(e[::-1] if k % 3 == 1 else e)
                if k % 4 == 2:
                    self.edges.append(e)                       # a duplicate
                    self.edges.append(e[::-1])                 # and its reverse
        elif edges == "tree":
            for k in range(1, len(rows)):
                self.edges.append((rows[k], rows[int(self.rng.randint(k))]))
            if len(rows) > 2:
                self.edges.append((rows[0], rows[-1]))
        self.cases.setdefault(case, []).append(dict(rows=rows, X=X, views=list(views)))
        return rows, X

    def junk_around(self, rows, total):
        """grow the component of ``rows`` to ``total`` rows with junk rows (random
        pixels), each tied to an earlier member in another set"""
        sid = tr.set_of_rows(self.set_off)
        comp = list(rows)
        while len(comp) < total:
            s = int(self.rng.randint(len(SET_SIZES)))
            partner = comp[int(self.rng.randint(len(comp)))]
            if sid[partner] == s or not self.free[s]:
                continue
            r = self.row(s)
            self.edges.append((r, partner) if len(comp) % 2 else (partner, r))
            comp.append(r)
        return comp


def build(seed):
    b = Builder(seed)
    rng = b.rng
    for _ in range(20):                                        # exact two-view tracks
        a = int(rng.randint(NCAM - 2))
        b.track("two_view", [a, a + 1 + int(rng.randint(2))], rng.uniform(3, 6))
    b.track("chain8", list(range(8)), rng.uniform(6, 9), edges="chain")
    noisy_at = [len(b.edges)]
    for _ in range(15):                                        # sigma = 0.5 px
        n = int(rng.randint(3, 7))
        a = int(rng.randint(NCAM - n + 1))
        b.track("noisy", list(range(a, a + n)), rng.uniform(4, 9), sigma=0.5)
    noisy_at.append(len(b.edges))
    rows, X = b.track("outlier", [1, 2, 3, 4, 5], 6.0)         # one observation 30 px off
    b.kp[rows[2]] += np.float32([30.0, 0.0])
    ra, _ = b.track("merge5", [0, 1, 2, 3, 4], 6.5)            # 5 + 3 joined by one wrong edge
    rb, _ = b.track("merge3", [5, 6, 7], 5.0)
    b.edges.append((ra[4], rb[0]))
    b.track("low_parallax", [0, 9], 5.0)                       # baseline 0.002
    r0 = b.row(0, np.float32([40.0, 240.0]))                   # diverging rays: behind the cameras
    r1 = b.row(1, np.float32([600.0, 240.0]))
    b.edges.append((r0, r1))
    b.cases["behind"] = [dict(rows=[r0, r1], X=None, views=[0, 1])]
    rows, _ = b.track("full", list(range(8)), 7.0)             # exactly MAX_TRACK rows: kept
    b.cases["full"][0]["comp"] = b.junk_around(rows, MAX_TRACK)
    rows, _ = b.track("oversized", list(range(1, 9)), 8.0)     # MAX_TRACK + 1 rows: dropped
    b.cases["oversized"][0]["comp"] = b.junk_around(rows, MAX_TRACK + 1)
    N = int(b.set_off[-1])
    invalid = [(-1, -1), (-1, 5), (7, -3), (N, 3), (5, N + 7), (2 ** 31 - 1, 0)]
    same = [b.row(1), b.row(1)]
    invalid += [(same[0], same[1]), (same[1], same[1]), (b.row(4),) * 2]
    b.edges += invalid
    edges = np.asarray(b.edges, dtype=np.int64)
    edges = edges[rng.permutation(len(edges))].astype(np.int32)
    # the long component, on rows the first call leaves isolated; its call also
    # gets the noisy tracks' edges, so both track kernels run in it
    main, b.edges = b.edges, []
    rows, _ = b.track("long", list(range(9)), 7.5)
    b.cases["long"][0]["comp"] = b.junk_around(rows, LONG_ROWS)
    long_edges = np.asarray(b.edges + main[noisy_at[0]:noisy_at[1]], dtype=np.int64)
    long_edges = long_edges[rng.permutation(len(long_edges))].astype(np.int32)
    return dict(kp=b.kp, set_off=b.set_off, cams=b.cams, poses=b.poses, edges=edges,
                long_edges=long_edges, cases=b.cases, n_invalid=len(invalid))
