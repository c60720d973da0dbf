"""The consumer of posfeat_refine_points end to end on the GPU, on the scene of
tests/test_gpu_register_queries.py (a tiny feature directory, a pair list, the
intrinsics files and an .nvm written there): evaluation.verification
.verify_pair_list -> evaluation.reconstruction.triangulate_pair_list with and
without ``refine`` -> write_model -> evaluation.localization
.register_query_list on the refined model."""
import os

import numpy as np
import pytest
import torch

import triangulate_ref as tr
from test_gpu_register_queries import DB, QUERIES, _write_scene

pytestmark = pytest.mark.gpu

THR, MIN_ANGLE, SEED = 4.0, 1.5, 3
KEYS = {"points", "err", "tinfo", "track_off", "track_rows", "obs_inlier", "point_of_row", "counts",
        "images", "set_off", "cams", "poses", "keypoints", "models", "qvecs", "tvecs",
        "skipped_pairs", "summary"}


def test_refine_option_end_to_end(gpu, tmp_path):
    from posfeat_amd import geometry
    from posfeat_amd.evaluation import localization as loc, reconstruction as rc, verification
    root = str(tmp_path)
    _write_scene(root)
    out = os.path.join(root, "verified.npz")
    verification.verify_pair_list(root, os.path.join(root, "pairs.txt"), "test", seed=7, output=out)
    files = (out, root, "test", os.path.join(root, "database_intrinsics.txt"),
             os.path.join(root, "model.nvm"))
    res0 = rc.triangulate_pair_list(*files, thr=THR, min_angle=MIN_ANGLE, seed=SEED)
    off = rc.triangulate_pair_list(*files, thr=THR, min_angle=MIN_ANGLE, seed=SEED, refine=0)
    res3 = rc.triangulate_pair_list(*files, thr=THR, min_angle=MIN_ANGLE, seed=SEED, refine=3)

    # refine = 0 is the call without the option, which is one triangulate_tracks
    # call on the pool: the same keys, the same bits
    assert set(res0) == KEYS and set(off) == KEYS
    ver = np.load(out)
    index = {n: i for i, n in enumerate(res0["images"])}
    pairs = [(str(a), str(b)) for a, b in ver["pairs"].reshape(-1, 2)]
    edges, _ = rc.pair_list_edges(pairs, ver["match_offsets"], ver["matches"], index, res0["set_off"])
    direct = geometry.triangulate_tracks(
        torch.from_numpy(res0["keypoints"]).to(gpu), res0["set_off"],
        torch.from_numpy(res0["cams"]).to(gpu), torch.from_numpy(res0["poses"]).to(gpu),
        torch.from_numpy(edges).to(gpu), iters=64, thr=THR, min_angle=MIN_ANGLE, max_track=256,
        seed=SEED).host()
    for k in direct:
        assert direct[k].tobytes() == res0[k].tobytes() == off[k].tobytes(), k
    assert res0["summary"] == off["summary"]
    rc.write_model(res0, os.path.join(root, "sparse0"))
    rc.write_model(off, os.path.join(root, "sparse_off"))
    for name in ("cameras.txt", "images.txt", "points3D.txt"):
        with open(os.path.join(root, "sparse0", name), "rb") as a, \
                open(os.path.join(root, "sparse_off", name), "rb") as b:
            assert a.read() == b.read(), name

    # refine = 3: the refined result in the same layout, and what it adds
    assert set(res3) == KEYS | {"rinfo", "summary_unrefined", "counts_unrefined"}
    assert res3["summary_unrefined"] == res0["summary"]
    assert np.array_equal(res3["counts_unrefined"], res0["counts"])
    for k in ("track_off", "track_rows", "keypoints", "set_off"):
        assert np.array_equal(res3[k], res0[k]), k
    T = int(res0["counts"][0])
    assert res3["counts"][0] == T and res3["rinfo"].shape == (T, 4)
    assert np.all(res3["rinfo"][:, 0] <= 3) and res3["summary"]["points"] >= 280
    print("summary", res0["summary"], "->", res3["summary"], "counts", res3["counts"].tolist())

    # on the points whose inlier set is unchanged the mean reprojection error
    # (over the observations) does not exceed the unrefined one
    same = (res0["tinfo"][:, 0] == 0) & (res3["tinfo"][:, 0] == 0) & (res0["tinfo"][:, 1] >= 2)
    for t in np.flatnonzero(same):
        sl = slice(int(res0["track_off"][t]), int(res0["track_off"][t + 1]))
        same[t] = np.array_equal(res0["obs_inlier"][sl], res3["obs_inlier"][sl])
    w = res0["tinfo"][same, 1].astype(np.float64)
    before, after = (res0["err"][same] * w).sum() / w.sum(), (res3["err"][same] * w).sum() / w.sum()
    print("unchanged sets: %d points, mean reprojection error %.6f -> %.6f px"
          % (same.sum(), before, after))
    assert same.sum() >= 250 and after <= before

    # the written model, read back: every point reprojects within thr in every
    # image of its track
    rc.write_model(res3, os.path.join(root, "sparse"))
    cameras, images, points = rc.read_model(os.path.join(root, "sparse"))
    assert len(points) == res3["summary"]["points"] and len(images) == 5
    assert sum(len(p["track"]) for p in points.values()) == res3["summary"]["observations"]
    for pid, pt in points.items():
        assert len(pt["track"]) >= 2
        for image_id, idx in pt["track"]:
            im = images[image_id]
            cam = rc.camera_row(*[cameras[im["camera_id"]][i] for i in (0, 3)])
            e2, zd = tr.reproj2(cam, rc.pose_row(im["qvec"], im["tvec"]), pt["xyz"], im["xys"][idx])
            assert zd > 0 and np.sqrt(e2) <= THR
            assert im["point3D_ids"][idx] == pid

    # the queries register against the refined model
    res = loc.register_query_list(out, root, "test", os.path.join(root, "sparse"),
                                  os.path.join(root, "queries_with_intrinsics.txt"), thr=12.0,
                                  iters=256, seed=5)
    assert res["queries"] == QUERIES and res["registered"].tolist() == [True, True, False]
    assert np.all(res["n_corr"][:2] >= 280) and np.all(res["info"][:2, 1] >= 270)
