"""CPU checks of guided matching (posfeat_match_pairs_guided, guided_solve.h):
the host-only record and predicate entries against the numpy restatement
(tests/guided_ref.py) bit for bit on a synthetic two-view scene, the same
comparison by a stand-alone program under the host sanitizers, the ABI's
argument validation (no device work), and the distance between the fp32
predicate and the fp64 Sampson distance it stands for (printed; DESIGN.md
4.1j records the figures)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np

import guided_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 4.0


def _scene():
    rs = np.random.RandomState(11)
    kp1, kp2, F = GR.two_view(rs, 1500)
    hp1, hp2, H = GR.plane_view(rs, 400)
    return kp1, kp2, F, hp1, hp2, H


def _q2_zero():
    """H and an exactly representable point it maps to q2 = 0 (and its
    neighbours, which it maps to huge coordinates of either sign)"""
    H = np.array([[1.0, 0.0, 3.0], [0.0, 1.0, -2.0], [-1.0 / 512, 0.0, 1.0]])
    pts = np.array([[512.0, 300.0], [512.0, 0.0], [511.99997, 7.0], [512.00006, 7.0]], np.float32)
    return H, pts


def _cases():
    """[(model, side, M, pts)] and [(model, ra [ns, 4], cx, cy, cw, thr)]"""
    kp1, kp2, F, hp1, hp2, H = _scene()
    Hz, pz = _q2_zero()
    Z = np.zeros((3, 3))
    rec = [(1, 0, F, kp1), (1, 1, F, kp2), (0, 0, H, hp1), (0, 1, H, hp2), (1, 0, Z, kp1[:50]),
           (1, 1, Z, kp2[:50]), (0, 0, Z, hp1[:50]), (0, 0, Hz, pz), (0, 1, Hz, pz),
           (1, 0, 1e200 * F, kp1[:50]), (1, 1, F * np.nan, kp2[:5])]
    n = 300
    r1, r2 = GR.records(1, 0, F, kp1[:n]), GR.records(1, 1, F, kp2[:n])
    h1, h2 = GR.records(0, 0, H, hp1[:n]), GR.records(0, 1, H, hp2[:n])
    z1 = GR.records(1, 0, Z, kp1[:20])
    hz = GR.records(0, 0, Hz, pz)
    big = GR.records(1, 0, 1e200 * F, kp1[:20])
    adm = [(1, r2, kp1[:n, 0], kp1[:n, 1], r1[:, 3], THR),      # side "rows of sim"
           (1, r1, kp2[:n, 0], kp2[:n, 1], r2[:, 3], THR),      # side "columns"
           (1, r1, kp2[:n, 0], kp2[:n, 1], r2[:, 3], 1e15),
           (1, r1, kp2[:n, 0], kp2[:n, 1], r2[:, 3], 1e25),     # t2 = inf: nothing
           (0, h2, h1[:, 0], h1[:, 1], h1[:, 3], THR),
           (0, h1, h2[:, 0], h2[:, 1], h2[:, 3], THR),
           (0, h1, h2[:, 0], h2[:, 1], h2[:, 3], 1e15),
           (1, z1, kp2[:20, 0], kp2[:20, 1], np.zeros(20, np.float32), THR),   # zero model
           (1, big, kp2[:20, 0], kp2[:20, 1], r2[:20, 3], THR),                # inf records
           (0, hz, pz[:, 0], pz[:, 1], np.zeros(4, np.float32), THR),          # q2 = 0
           (0, hz, pz[:, 0], pz[:, 1], np.zeros(4, np.float32), 1e15)]
    return rec, adm


def test_records_and_predicate_equal_restatement_bit_for_bit():
    from posfeat_amd import geometry
    rec, adm = _cases()
    nrec = nadm = npass = 0
    for model, side, M, pts in rec:
        ref = GR.records(model, side, M, pts)
        for p, r in zip(pts, ref):
            got = geometry.guided_record(model, side, M, p)
            assert got.dtype == np.float32
            assert (got.view(np.uint32) == r.view(np.uint32))[~np.isnan(r)].all() and \
                (np.isnan(got) == np.isnan(r)).all(), (model, side, p, got, r)
            nrec += 1
    for model, ra, cx, cy, cw, thr in adm:
        ref = GR.admissible(model, ra, cx, cy, cw, GR.t2_of(thr))
        step = max(1, ra.shape[0] // 60)          # a sub-grid: one ctypes call per entry
        for i in range(0, ra.shape[0], step):
            for j in range(len(cx)):
                got = geometry.guided_admissible(model, ra[i], (cx[j], cy[j], cw[j]), thr)
                assert got == bool(ref[i, j]), (model, thr, i, j)
                nadm += 1
                npass += got
    assert nrec > 4000 and nadm > 50000 and 0 < npass < nadm
    # the zero model admits nothing; q2 = 0 gives non-finite records that fail
    Hz, pz = _q2_zero()
    hz = GR.records(0, 0, Hz, pz)
    assert not np.isfinite(hz[:2, :2]).any() and np.isfinite(hz[2:, :2]).all()
    assert abs(hz[2, 0]) > 1e6 and hz[2, 0] * hz[3, 0] < 0      # no sign test on q2
    assert not GR.admissible(0, hz[:2], pz[:, 0], pz[:, 1], 0 * pz[:, 0], GR.t2_of(1e15)).any()
    kp1, kp2, F, _, _, _ = _scene()
    okr, okc = GR.pair_masks(1, np.zeros((3, 3)), kp1[:64], kp2[:64], THR)
    assert not okr.any() and not okc.any()
    okr, okc = GR.pair_masks(1, F, kp1[:300], kp2[:300], THR)
    assert okr[np.arange(300), np.arange(300)].all() and okc[np.arange(300), np.arange(300)].all()
    assert okr.mean() < 0.05


def test_guided_check_under_host_sanitizers(tmp_path):
    """tests/host/guided_check.cpp (its own main) built with
    -fsanitize=address,undefined and run directly on the cases written here."""
    cxx = next((c for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++")
                if os.path.exists(c)), None) or shutil.which("clang++")
    assert cxx, "no clang++ (ROCm's LLVM) to build the host check with"
    rec, adm = _cases()
    rdt = np.dtype([("model", "<i4"), ("side", "<i4"), ("M", "<f8", 9), ("pt", "<f4", 2),
                    ("expect", "<f4", 4)])
    adt = np.dtype([("model", "<i4"), ("ra", "<f4", 4), ("col", "<f4", 3), ("t2", "<f4"),
                    ("expect", "<i4")])
    assert rdt.itemsize == 104 and adt.itemsize == 40
    rparts, aparts = [], []
    for model, side, M, pts in rec:
        a = np.zeros(len(pts), rdt)
        a["model"], a["side"], a["M"], a["pt"] = model, side, np.asarray(M).reshape(9), pts
        a["expect"] = GR.records(model, side, M, pts)
        rparts.append(a)
    for model, ra, cx, cy, cw, thr in adm:
        ok = GR.admissible(model, ra, cx, cy, cw, GR.t2_of(thr))
        i, j = np.meshgrid(np.arange(ra.shape[0]), np.arange(len(cx)), indexing="ij")
        a = np.zeros(i.size, adt)
        a["model"], a["ra"], a["t2"] = model, ra[i.ravel()], GR.t2_of(thr)
        a["col"] = np.stack([cx, cy, cw], 1)[j.ravel()]
        a["expect"] = ok.ravel()
        aparts.append(a)
    ra, aa = np.concatenate(rparts), np.concatenate(aparts)
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as f:
        f.write(np.asarray([len(ra), len(aa)], "<i4").tobytes())
        f.write(ra.tobytes())
        f.write(aa.tobytes())
    exe = str(tmp_path / "guided_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-Wno-pass-failed",
                    os.path.join(ROOT, "tests", "host", "guided_check.cpp"), "-o", exe],
                   check=True, timeout=300)
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    assert r.returncode == 0 and "guided ok: %d records, %d predicates" % (len(ra), len(aa)) \
        in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, ctypes.c_void_p(a.ctypes.data)


def test_guided_abi_errors_without_a_device():
    from posfeat_amd import _lib
    L = _lib.lib()
    set_off, so = _i32([0, 300, 300, 1300, 3349])          # set 1 is empty
    pairs, pp = _i32([[0, 2], [2, 3], [1, 0], [3, 3]])
    need = L.posfeat_match_pairs_guided_workspace(so, 4, pp, 4)
    plain = L.posfeat_match_pairs_workspace(so, 4, pp, 4)
    # the records: 16 B per keypoint per side of the three live pairs
    assert need >= plain + 16 * ((300 + 1000) + (1000 + 2049) + (2049 + 2049))
    p = ctypes.c_void_p(4096)                              # dummy, non-null, 256-B aligned

    def call(desc=p, kp=p, so=so, nsets=4, pp=pp, npairs=4, dim=128, mode=0, model=1, M=p,
             thr=4.0, matches=p, counts=p, ws=p, ws_bytes=need):
        return L.posfeat_match_pairs_guided(desc, kp, so, nsets, pp, npairs, dim, mode, 0.95, model,
                                            M, thr, matches, counts, ws, ws_bytes, None)

    for name in ("desc", "kp", "so", "pp", "M", "matches", "counts", "ws"):
        assert call(**{name: None}) == -1, name            # a null pointer
    assert call(M=ctypes.c_void_p(4100)) == -1             # M not 8-B aligned
    assert call(desc=ctypes.c_void_p(4104)) == -1
    assert call(ws=ctypes.c_void_p(4224)) == -1
    for thr in (0.0, -1.0, float("inf"), float("nan")):
        assert call(thr=thr) == -1
    for model in (-1, 2):
        assert call(model=model) == -4
    for mode in (-1, 3):
        assert call(mode=mode) == -4
    assert call(dim=64) == -4
    _, bad_hi = _i32([[0, 2], [2, 4]])
    _, dec = _i32([0, 300, 299, 1300, 3349])
    assert call(pp=bad_hi, npairs=2) == -1
    assert call(so=dec) == -1
    assert call(npairs=0) == -1
    _, big = _i32([0, 1 << 30])
    _, bigp = _i32([[0, 0]] * 3)
    assert call(so=big, nsets=1, pp=bigp, npairs=3, ws_bytes=1 << 62) == -1
    assert call(ws_bytes=need - 1) == -3 and call(ws_bytes=plain) == -3
    assert L.posfeat_match_pairs_guided_workspace(dec, 4, pp, 4) == 0
    assert L.posfeat_match_pairs_guided_workspace(so, 4, bad_hi, 2) == 0
    # the host-only entries
    f4 = np.zeros(4, np.float32)
    f4p = ctypes.c_void_p(f4.ctypes.data)
    m9 = np.zeros(9)
    m9p = ctypes.c_void_p(m9.ctypes.data)
    assert L.posfeat_guided_record(1, 0, m9p, f4p, f4p) == 0
    assert L.posfeat_guided_record(1, 0, None, f4p, f4p) == -1
    assert L.posfeat_guided_record(1, 0, m9p, None, f4p) == -1
    assert L.posfeat_guided_record(1, 0, m9p, f4p, None) == -1
    assert L.posfeat_guided_record(1, 2, m9p, f4p, f4p) == -1
    assert L.posfeat_guided_record(2, 0, m9p, f4p, f4p) == -4
    assert L.posfeat_guided_admissible(1, f4p, f4p, 4.0) == 0       # den = 0
    assert L.posfeat_guided_admissible(0, f4p, f4p, 4.0) == 1       # distance 0
    assert L.posfeat_guided_admissible(0, None, f4p, 4.0) == -1
    assert L.posfeat_guided_admissible(0, f4p, None, 4.0) == -1
    assert L.posfeat_guided_admissible(0, f4p, f4p, 0.0) == -1
    assert L.posfeat_guided_admissible(0, f4p, f4p, float("nan")) == -1
    assert L.posfeat_guided_admissible(-1, f4p, f4p, 4.0) == -4


def test_fp32_predicate_against_fp64_sampson():
    """How far the distance the fp32 predicate compares with thr lies from the
    fp64 Sampson distance, over all candidate pairs of the 1500 x 1500 scene and
    over those within 1 px of thr = 4 (figures in DESIGN.md 4.1j; the GPU
    end-to-end test takes its slack from PREDICATE_DEV below)."""
    kp1, kp2, F, _, _, _ = _scene()
    d64 = GR.sampson(F, kp1, kp2)
    d32 = GR.predicate_distance(F, kp1, kp2)
    dev = np.abs(d32 - d64)
    near = np.abs(d64 - THR) <= 1.0
    _, okc = GR.pair_masks(1, F, kp1, kp2, THR)
    disagree = int((okc != (d64 <= THR)).sum())
    print("fp32 predicate vs fp64 Sampson over %d candidates: max |diff| %.3g px overall, "
          "%.3g px within 1 px of thr (%d candidates), %d decisions differ"
          % (dev.size, dev.max(), dev[near].max(), int(near.sum()), disagree))
    assert near.sum() > 1000
    # a decision can differ only for a candidate closer to thr than the deviation
    assert (np.abs(d64 - THR)[okc != (d64 <= THR)] <= dev.max()).all()
    assert dev[near].max() <= GR.MEASURED_DEV <= PREDICATE_DEV
    assert (dev <= PREDICATE_DEV + 8 * 2.0 ** -24 * d64).all()


# The deviation near the threshold, from the formats (not from a run): e = lx x
# + ly y + lz with l the streamed point's epipolar line; a candidate near the
# threshold lies near the line, so each of the three terms is at most about
# |(x, y)| |l| <= 2000 |l| in a 1600 x 1200 frame.  Three record components, two
# products and two sums are each rounded to 2^-24 relative (8 roundings with
# den's), and sqrt(den) >= |l|: 8 x 2^-24 x 2000 = 9.5e-4 px.  Far from the
# line lz grows with the distance d itself, hence the relative term above.
PREDICATE_DEV = 8 * 2.0 ** -24 * 2000
