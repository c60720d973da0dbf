"""Numpy restatement of posfeat_split_tracks (include/posfeat_hip.h): sequential
RANSAC over the members a track's own RANSAC left out.  A generation is
``triangulate_track`` of tests/triangulate_ref.py run on the left-over list as
if it were a track; everything else (which parents split, the partition of the
member range, the numbering under the output capacity, the counts) is written
here from the header's definitions in plain loops.  The capacity rule is
walked track by track, not taken from the closed form the library uses.
Nothing here touches the GPU."""
import numpy as np

from triangulate_ref import Scene, triangulate_track

MAX_TRACK = 1024


class _Guard:
    """``arr`` indexed by pool rows: a row outside [0, N) reads as ``fill``, so
    nothing is read through it"""

    def __init__(self, arr, fill):
        self.arr, self.fill = np.asarray(arr), fill

    def __getitem__(self, r):
        r = np.asarray(r, np.int64)
        ok = (r >= 0) & (r < len(self.arr))
        out = np.array(self.arr[np.where(ok, r, 0)])
        if r.ndim == 0:
            if not ok:
                out[...] = self.fill
            return out if out.ndim else out[()]
        out[~ok] = self.fill
        return out


class GuardedScene(Scene):
    """Scene whose rows outside the pool belong to a set of NaNs: never an
    inlier, every hypothesis through one rejected (the DLT is not finite)"""

    def __init__(self, kp, set_off, cams, poses):
        Scene.__init__(self, kp, set_off, cams, poses)
        nsets = len(self.cams)
        self.n = len(self.kp)
        self.cams = np.concatenate([self.cams, np.full((1, 8), np.nan)])
        self.poses = np.concatenate([self.poses, np.full((1, 12), np.nan)])
        self.kp = _Guard(self.kp, np.nan)
        self.und = _Guard(self.und, np.nan)
        self.sid = _Guard(self.sid, nsets)


def split_parent(sc, rows, flags, iters, thr, min_angle_deg, seed, rounds, margins=None):
    """The generations of one parent that may split: rows, flags = its members
    in member order.  -> list of dicts(members = the member numbers of the
    child's inliers, X, err, tinfo, eig)"""
    left = [k for k in range(len(rows)) if flags[k] == 0]
    children = []
    for _ in range(rounds):
        if len(left) < 2:
            break
        with np.errstate(all="ignore"):
            r = triangulate_track(sc, [int(rows[k]) for k in left], iters, thr, min_angle_deg, seed,
                                  margins)
        if r["status"] != 0 or r["n_inliers"] < 2:
            break
        took = [k for k, f in zip(left, r["flags"]) if f]
        children.append(dict(members=took, X=r["X"], err=r["err"], eig=r["eig"],
                             tinfo=(0, r["n_inliers"], r["best_h"], r["refit_kept"])))
        left = [k for k, f in zip(left, r["flags"]) if not f]
    return children


def split(kp, set_off, cams, poses, tracks, tmax, mmax, iters, thr, min_angle_deg, seed, rounds,
          tmax_out):
    """``tracks``: the host dict of a triangulate result (points, err, tinfo,
    track_off, track_rows, obs_inlier, counts).  -> the outputs of
    posfeat_split_tracks trimmed as TrackResult.host() trims them, plus
    'parent_of', 'generation', 'margins' and 'eig_ratio' (per output track,
    nan for a parent)."""
    assert tmax_out >= tmax
    sc = GuardedScene(kp, set_off, cams, poses)
    N = sc.n
    T = min(max(int(tracks["counts"][0]), 0), tmax)
    off_in = np.asarray(tracks["track_off"], np.int64)
    rows_in, flags_in = np.asarray(tracks["track_rows"]), np.asarray(tracks["obs_inlier"])
    margins = {}
    found = []
    for t in range(T):
        off, m = int(off_in[t]), int(off_in[t + 1] - off_in[t])
        usable = off >= 0 and m >= 0 and off + m <= mmax and m <= MAX_TRACK
        kids = []
        if usable and int(tracks["tinfo"][t][0]) == 0 and \
                int((flags_in[off:off + m] == 0).sum()) >= 2:
            kids = split_parent(sc, rows_in[off:off + m], flags_in[off:off + m], iters, thr,
                                min_angle_deg, seed, rounds, margins)
        found.append((usable, kids))
    # the numbering: in output order a child is created iff its number plus the
    # parents still to come stays below tmax_out
    points, err, tinfo, parent_of, generation, eig_ratio = [], [], [], [], [], []
    track_off = []
    track_rows, obs = rows_in.copy(), flags_in.copy()
    point_of_row = np.full(N, -1, np.int32)
    refused = created = nsplit = 0
    for t, (usable, kids) in enumerate(found):
        off, m = int(off_in[t]), int(off_in[t + 1] - off_in[t])
        pid = len(points)
        points.append(np.array(tracks["points"][t])), err.append(tracks["err"][t])
        tinfo.append(tuple(int(v) for v in tracks["tinfo"][t]))
        parent_of.append(t), generation.append(0), eig_ratio.append(np.nan)
        track_off.append(off)
        made = []
        for g, kid in enumerate(kids, 1):
            if len(points) + (T - 1 - t) < tmax_out:
                made.append(kid)
                points.append(kid["X"]), err.append(kid["err"]), tinfo.append(kid["tinfo"])
                parent_of.append(t), generation.append(g)
                e = kid["eig"]
                eig_ratio.append(e[1] / e[-1] if e is not None and e[-1] > 0 else np.nan)
            else:
                refused += 1
        created += len(made)
        nsplit += 1 if made else 0
        if not usable:
            continue
        claimed = {k: g for g, kid in enumerate(made, 1) for k in kid["members"]}
        order = [k for k in range(m) if k not in claimed]
        starts = []
        for g in range(1, len(made) + 1):
            starts.append(off + len(order))
            order += [k for k in range(m) if claimed.get(k) == g]
        for dst, k in enumerate(order, off):
            row, g = int(rows_in[off + k]), claimed.get(k, 0)
            track_rows[dst] = row
            obs[dst] = 1 if g else flags_in[off + k]
            if 0 <= row < N:
                if g:
                    point_of_row[row] = pid + g
                elif flags_in[off + k] != 0 and tinfo[pid][0] == 0:
                    point_of_row[row] = pid
        track_off += starts
    track_off.append(int(off_in[T]))
    Tp = len(points)
    tinfo = np.asarray(tinfo, np.int32).reshape(-1, 4)
    ok = tinfo[:, 0] == 0
    counts = np.array([Tp, int(tracks["counts"][1]), int(ok.sum()), int(tinfo[ok, 1].sum()), refused,
                       0, created, nsplit], np.int32)
    M = int(counts[1])
    return dict(points=np.asarray(points, np.float64).reshape(-1, 3), err=np.asarray(err, np.float64),
                tinfo=tinfo, track_off=np.asarray(track_off, np.int32),
                track_rows=track_rows[:M].astype(np.int32), obs_inlier=obs[:M].astype(np.uint8),
                point_of_row=point_of_row, counts=counts,
                parent_of=np.asarray(parent_of, np.int32),
                generation=np.asarray(generation, np.int32), margins=margins,
                eig_ratio=np.asarray(eig_ratio))
