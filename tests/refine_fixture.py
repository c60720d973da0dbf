"""The inputs of the point-refinement tests: planted single-point systems for
posfeat_refine_point (views at distances 2..40 with focal lengths 400..1600,
every second camera SIMPLE_RADIAL) and a hand-built track table over cameras
with the same spread that holds every case posfeat_refine_points
distinguishes.  Built from fixed numpy seeds; nothing here touches the GPU."""
import numpy as np

import triangulate_ref as tr

THR, MIN_ANGLE, ROUNDS, STEPS = 4.0, 1.5, 3, 10
K1 = -0.05
LANE_TRACK = 16
SYSTEM_SEED, TABLE_SEED = 11, 5
COND_MAX = 1e6


def look_at(C, target, roll=0.0):
    """[R | t] row-major [12] of a camera at C looking at ``target``"""
    z = (target - C) / np.linalg.norm(target - C)
    up = np.array([np.sin(roll), np.cos(roll), 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return np.concatenate([R, (-R @ C)[:, None]], 1).reshape(-1)


def spread_camera(rng, k, target):
    """a camera 2..40 from ``target`` (log-uniform) inside a cone of 50 degrees
    about -z, focal length 400..1600 (log-uniform), every second one with k1"""
    d = float(np.exp(rng.uniform(np.log(2.0), np.log(40.0))))
    f = float(np.exp(rng.uniform(np.log(400.0), np.log(1600.0))))
    th, ph = np.deg2rad(rng.uniform(0.0, 50.0)), rng.uniform(0.0, 2 * np.pi)
    u = np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), -np.cos(th)])
    cam = np.array([f, f, 0.8 * f, 0.6 * f, K1 if k % 2 else 0.0, 0, 0, 0])
    return cam, look_at(target + d * u, target + rng.uniform(-0.1, 0.1, 3) * d, rng.uniform(-0.3, 0.3))


def und_obs(cam, pose, xy):
    return np.concatenate([tr.undistort(cam, float(xy[0]), float(xy[1])), pose])


def normal_condition(obs22, X):
    import refine_ref as rr
    N = np.zeros((3, 3))
    for o in obs22:
        _, J, _ = rr.row_terms(o[2:10], o[10:22], o[0:2], X)
        N += J.T @ J
    return float(np.linalg.cond(N))


def systems(seed=SYSTEM_SEED, count=200):
    """planted systems for posfeat_refine_point: dicts(obs [n, 22], X planted,
    X0 the DLT point, noisy).  2..8 views; odd systems carry 1 px noise.  A
    draw whose normal matrix at the planted point has a condition number above
    COND_MAX, or whose DLT is rejected, is drawn again."""
    rng = np.random.RandomState(seed)
    out = []
    while len(out) < count:
        k = len(out)
        n, noisy = 2 + k % 7, bool(k % 2)
        X = rng.uniform(-0.3, 0.3, 3)
        obs = []
        for v in range(n):
            cam, pose = spread_camera(rng, v + k, np.zeros(3))
            px, py, _ = tr.project(cam, pose, X)
            xy = np.array([px, py]) + (rng.normal(0.0, 1.0, 2) if noisy else 0.0)
            obs.append(np.concatenate([xy, cam, pose]))
        obs = np.asarray(obs)
        X0, _ = tr.dlt([und_obs(o[2:10], o[10:22], o[0:2]) for o in obs])
        if X0 is None or normal_condition(obs, X) > COND_MAX:
            continue
        out.append(dict(obs=obs, X=X, X0=X0, noisy=noisy))
    return out


NSPREAD = 32                                  # sets 0..31 spread; set 32 sits 0.002 from set 0
SET_SIZES = [90 + 7 * (s % 5) for s in range(NSPREAD)] + [40]


class Table:
    """a track table written by hand: rows handed out per set, tracks appended"""

    def __init__(self, seed):
        self.rng = rng = np.random.RandomState(seed)
        cams, poses = zip(*[spread_camera(rng, s, np.zeros(3)) for s in range(NSPREAD)])
        C0 = tr.centre(poses[0])
        R0 = poses[0].reshape(3, 4)[:, :3]
        C32 = C0 + R0[0] * 0.002                                   # along camera 0's x axis
        p32 = np.concatenate([R0, (-R0 @ C32)[:, None]], 1).reshape(-1)
        self.cams = np.asarray(list(cams) + [cams[0].copy()])
        self.poses = np.asarray(list(poses) + [p32])
        self.set_off = np.concatenate([[0], np.cumsum(SET_SIZES)]).astype(np.int32)
        N = int(self.set_off[-1])
        self.kp = np.stack([rng.uniform(0, 1200, N), rng.uniform(0, 900, N)], 1).astype(np.float32)
        self.free = [list(self.set_off[s] + rng.permutation(SET_SIZES[s]))
                     for s in range(len(SET_SIZES))]
        self.rows, self.flags, self.points, self.tinfo, self.off = [], [], [], [], [0]
        self.cases = {}

    def row(self, s, xy=None):
        r = int(self.free[s].pop())
        if xy is not None:
            self.kp[r] = np.asarray(xy, np.float32)
        return r

    def observe(self, s, X, sigma=0.0, shift=(0.0, 0.0)):
        px, py, _ = tr.project(self.cams[s], self.poses[s], X)
        xy = np.array([px, py]) + np.asarray(shift)
        if sigma > 0.0:
            xy = xy + self.rng.normal(0.0, sigma, 2)
        return self.row(s, xy)

    def dlt(self, rows):
        sid = tr.set_of_rows(self.set_off)
        X, _ = tr.dlt([und_obs(self.cams[sid[r]], self.poses[sid[r]],
                               self.kp[r].astype(np.float64)) for r in rows])
        assert X is not None
        return X

    def add(self, case, rows, flags, X0, status=0, info=(7, 1), **kw):
        """the members in ascending row order, as posfeat_triangulate lists them"""
        order = np.argsort(rows)
        rows, flags = [rows[i] for i in order], [flags[i] for i in order]
        self.rows += rows
        self.flags += flags
        self.points.append(np.asarray(X0, np.float64))
        self.tinfo.append((status, int(np.sum(flags)), info[0], info[1]))
        self.off.append(len(self.rows))
        self.cases.setdefault(case, []).append(dict(t=len(self.points) - 1, rows=rows, **kw))
        return len(self.points) - 1

    def noisy_track(self, case, views, sigma=1.0, junk=0):
        """a planted point seen by ``views`` (all flagged, the DLT point as input)
        plus ``junk`` members with random pixels, flagged out"""
        X = self.rng.uniform(-0.3, 0.3, 3)
        rows = [self.observe(s, X, sigma) for s in views]
        extra = [self.row(int(self.rng.randint(NSPREAD))) for _ in range(junk)]
        return self.add(case, rows + extra, [1] * len(rows) + [0] * junk, self.dlt(rows), X=X)

    def views(self, n):
        """n sets of 0..31, each used as evenly as n allows"""
        reps = -(-n // NSPREAD)
        pool = np.concatenate([self.rng.permutation(NSPREAD) for _ in range(reps)])
        return [int(s) for s in pool[:n]]

    def result(self):
        T = len(self.points)
        return dict(kp=self.kp, set_off=self.set_off, cams=self.cams, poses=self.poses,
                    cases=self.cases,
                    tracks=dict(points=np.asarray(self.points).reshape(T, 3),
                                tinfo=np.asarray(self.tinfo, np.int32).reshape(T, 4),
                                track_off=np.asarray(self.off, np.int32),
                                track_rows=np.asarray(self.rows, np.int32),
                                obs_inlier=np.asarray(self.flags, np.uint8),
                                counts=np.array([T, len(self.rows), 0, 0, 0, 0, 0, 0], np.int32)))


def similar_views(b, n):
    """n sets whose cameras weigh a pixel alike: the n closest in focal length
    over distance to the median"""
    w = np.array([b.cams[s, 0] / np.linalg.norm(tr.centre(b.poses[s])) for s in range(NSPREAD)])
    return [int(s) for s in np.argsort(np.abs(np.log(w / np.median(w))))[:n]]


def build_table(seed=TABLE_SEED, extra_tracks=0):
    b = Table(seed)
    rng = b.rng
    for _ in range(40):                                        # volume: 3..7 noisy views
        b.noisy_track("noisy", b.views(int(rng.randint(3, 8))))
    # a 30 px outlier among the input inliers of 14 similar views: round 1 fits it
    # in, the test drops it, round 2 refits
    X = rng.uniform(-0.2, 0.2, 3)
    views = similar_views(b, 14)
    rows = [b.observe(s, X, 0.2, (30.0, 0.0) if k == 5 else (0.0, 0.0)) for k, s in enumerate(views)]
    b.add("outlier", rows, [1] * 14, b.dlt(rows), X=X, outlier=rows[5])
    # an exact member the input had flagged out: the test admits it
    X = rng.uniform(-0.2, 0.2, 3)
    rows = [b.observe(s, X, 0.3) for s in b.views(5)]
    b.add("readmit", rows, [1, 1, 0, 1, 1], b.dlt([rows[i] for i in (0, 1, 3, 4)]), X=X,
          readmitted=rows[2])
    # one inlier left: the two others are 80 px off and flagged out / in
    X = rng.uniform(-0.2, 0.2, 3)
    v = b.views(3)
    rows = [b.observe(v[0], X), b.observe(v[1], X, shift=(80.0, 0.0)),
            b.observe(v[2], X, shift=(0.0, -80.0))]
    b.add("one_inlier", rows, [1, 0, 0], X, X=X)
    v = b.views(3)
    rows = [b.observe(v[0], X, shift=(150.0, 0.0)), b.observe(v[1], X, shift=(-150.0, 90.0)),
            b.observe(v[2], X, shift=(0.0, -150.0))]
    b.add("no_inlier", rows, [1, 1, 1], X, X=X)
    # the only inliers are the 0.002-baseline pair
    X = rng.uniform(-0.2, 0.2, 3)
    rows = [b.observe(0, X), b.observe(NSPREAD, X), b.observe(5, X, shift=(60.0, 60.0))]
    b.add("low_parallax", rows, [1, 1, 0], X, X=X)
    # two inliers in one image and one elsewhere; then the two alone
    X = rng.uniform(-0.2, 0.2, 3)
    rows = [b.observe(3, X, 0.3), b.observe(3, X, 0.3), b.observe(7, X, 0.3)]
    b.add("same_image_plus_one", rows, [1, 1, 1], X, X=X)
    rows = [b.observe(4, X, 0.3), b.observe(4, X, 0.3)]
    b.add("same_image_only", rows, [1, 1], X, X=X)
    # a status-1 input, a non-finite input point, a member row outside the pool
    rows = [b.observe(s, X, 0.3) for s in b.views(3)]
    b.add("status1", rows, [0, 0, 0], np.zeros(3), status=1, info=(-1, 0), X=X)
    rows = [b.observe(s, X, 0.3) for s in b.views(4)]
    b.add("nan_point", rows, [1, 1, 1, 1], [np.nan, 0.0, 1.0], X=X)
    rows = [b.observe(s, X, 0.3) for s in b.views(4)]
    b.add("bad_row", rows + [int(b.set_off[-1]) + 5], [1] * 5, b.dlt(rows), X=X)
    # the sizes at which the kernels change path
    for m in (2, LANE_TRACK, LANE_TRACK + 1, 64, 65, 130):
        junk = 0 if m <= 2 else max(1, m // 8)
        b.noisy_track("size%d" % m, b.views(m - junk), junk=junk)
    for _ in range(extra_tracks):                              # unrelated tracks, at the end
        b.noisy_track("extra", b.views(int(rng.randint(2, 30))))
    return b.result()
