"""The front end on the device (ssba_frontend.hip: ssba_frontend_ransac and ssba_frontend_vo) against the long-double
reference of tests/hp_frontend.py, within the bars derived there:

* the 3-point alignment on a ladder of s1 / s2 from 1 to 1e7 (32 triangles per step, the same in another sample order and
  mirrored in their own plane), 16 exactly collinear and 4 coincident samples: rotation, translation and orthonormality
  bars, R v1 = u1 on the collinear ones, and count = 3 everywhere (no hypothesis turned into NaN);
* the inlier test next to its threshold and the count reduction at 3, 63, 64, 65, 255, 256, 257 and 513 points: flags equal
  to the long-double decision on the returned T outside the band 16 u M, count = number of set flags;
* the selection: first maximum past the first 256-lane stride of k_fe_select_T, with ties after it;
* matching at 255, 256, 257 and 512 observations with 3, 200 and all matches, ids ascending and in another order, and the
  two inputs reported as an error;
* the pose chain over 64, 65 and 129 pairs (its 64-pair chunks) and the map initialisation.

tests/test_hp_frontend.py checks on the CPU what these tests take for granted: the reference against 60 digits, which rows
it decides, and that the sequences leave no pair ambiguous in the reference.  Run with -s to see the ratios (FEREF)."""
import ctypes as C
import functools

import numpy as np
import pytest

import hp_frontend as hf
from ceres_slam_amd import capi, frontend, synth

pytestmark = pytest.mark.gpu

U, LD = hf.U, hf.LD
CAM = synth.KITTI_CAMERA
_u32p, _u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)


def _report(tag, **kv):
    print("FEREF", tag, " ".join(f"{k}={v:.3g}" if isinstance(v, float) else f"{k}={v}" for k, v in kv.items()))


def _ransac(pairs, thresh):
    """One ssba_frontend_ransac call: every pair scored with the single hypothesis of its first three points."""
    lib = capi.load()
    sizes = np.array([len(p[0]) for p in pairs])
    offset = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    p0 = np.ascontiguousarray(np.concatenate([p[0] for p in pairs]))
    p1 = np.ascontiguousarray(np.concatenate([p[1] for p in pairs]))
    samples = np.tile(np.array([0, 1, 2], dtype=np.uint32), len(pairs))
    T = np.zeros((len(pairs), 12))
    inl = np.zeros(int(offset[-1]), dtype=np.uint8)
    cnt = np.zeros(len(pairs), dtype=np.uint32)
    cam = capi.Camera(**CAM)
    capi.check(lib.ssba_frontend_ransac(C.byref(cam), -1, len(pairs), offset.ctypes.data_as(_u32p), capi.dptr(p0), capi.dptr(p1),
                                        samples.ctypes.data_as(_u32p), 1, float(thresh), capi.dptr(T), inl.ctypes.data_as(_u8p),
                                        cnt.ctypes.data_as(_u32p), None), "ssba_frontend_ransac")
    return T, [inl[offset[i]:offset[i + 1]].astype(bool) for i in range(len(pairs))], cnt


def _vo(seq, num_iters, thresh=4.0):
    """ssba_frontend_vo on a sequence of hp_frontend: (status, poses, map, initialized, match_count, inlier_count)."""
    lib = capi.load()
    S = len(seq["state_start"]) - 1
    poses = np.zeros((S, 12))
    poses[0] = seq["first_pose"]
    points = np.zeros((seq["num_points"], 3))
    init = np.zeros(seq["num_points"], dtype=np.uint8)
    mcnt, icnt = np.zeros(S - 1, dtype=np.uint32), np.zeros(S - 1, dtype=np.uint32)
    cam = capi.Camera(**CAM)
    rc = lib.ssba_frontend_vo(C.byref(cam), -1, S, seq["state_start"].ctypes.data_as(_u32p), seq["point_id"].ctypes.data_as(_u32p),
                              capi.dptr(seq["uvd"]), seq["num_points"], num_iters, thresh, 1, capi.dptr(poses), capi.dptr(points),
                              init.ctypes.data_as(_u8p), mcnt.ctypes.data_as(_u32p), icnt.ctypes.data_as(_u32p), None)
    return rc, poses, points, init.astype(bool), mcnt, icnt


@functools.lru_cache(maxsize=None)
def _samples(n, num_iters):
    return frontend.ransac_samples(n, num_iters, 1)


def _reference(seq, num_iters, thresh=4.0):
    return hf.vo_pipeline(CAM, seq["state_start"], seq["point_id"], seq["uvd"], seq["num_points"], seq["first_pose"],
                          lambda n: _samples(n, num_iters), thresh)


def _compare_pipeline(tag, seq, num_iters, max_skipped):
    """Device against vo_pipeline.  Pairs are compared up to the first one whose winner the reference cannot name
    (hp_frontend.ransac_pair: decided counts against decided + undecided ones); the poses after it hang on that choice."""
    ref = _reference(seq, num_iters)
    rc, poses, points, init, mcnt, icnt = _vo(seq, num_iters)
    assert rc == 0 and ref["failed"] is None
    assert np.array_equal(mcnt, ref["match_count"])
    P = len(mcnt)
    amb = [k for k, r in enumerate(ref["pairs"]) if not r["unambiguous"]]
    valid = amb[0] if amb else P                      # pairs 0 .. valid - 1 and poses 0 .. valid are comparable
    assert P - valid <= max_skipped, amb
    for k in range(valid):
        r = ref["pairs"][k]
        assert r["lo"][r["winner"]] <= icnt[k] <= r["hi"][r["winner"]], (k, icnt[k])
    d = np.abs(np.asarray(hf._f(poses) - ref["poses"], np.float64))[: valid + 1]
    rR = (d[1:, 3:].max(1) / ref["chain_R"][1:valid + 1]).max()
    rt = (d[1:, :3].max(1) / ref["chain_t"][1:valid + 1]).max()
    # map points: those the reference initialises in a comparable pair, unless one of the landmark's rows is undecided there
    fp = ref["first_pair"]
    open_ = np.zeros(len(fp), dtype=bool)
    for k in range(valid):
        r = ref["pairs"][k]
        ids = seq["point_id"][seq["state_start"][k] + ref["match_pos"][k][0]]
        open_[ids[~r["decided"][r["winner"]]]] = True
    sure = (fp >= 0) & (fp < valid) & ~open_
    if valid == P:
        assert np.array_equal(init[~open_], ref["initialized"][~open_])
    assert init[sure].all()
    rm = (np.abs(np.asarray(hf._f(points[sure]) - ref["map"][sure], np.float64)).max(1) / ref["map_bar"][sure]).max()
    _report(tag, pairs=P, skipped=P - valid, R=float(rR), t=float(rt), map=float(rm), map_points=int(sure.sum()))
    assert rR <= 1 and rt <= 1 and rm <= 1
    return ref, poses


def test_alignment_ladder():
    rng = np.random.default_rng(77)
    groups = []                                       # (tag, p0, p1, reference)
    for kappa in hf.GPU_LADDER:
        p0, p1 = hf.ladder_step(max(kappa, 1.0 + 1e-9), 32, rng)
        ref = hf.align3(p0, p1)
        groups.append((f"kappa={kappa:g}", p0, p1, ref))
        groups.append((f"kappa={kappa:g} order 2,0,1", p0[:, (2, 0, 1)], p1[:, (2, 0, 1)], ref))
        q0, q1 = hf.ladder_step(max(kappa, 1.0 + 1e-9), 32, rng, mirror=True)
        groups.append((f"kappa={kappa:g} mirrored", q0, q1, hf.align3(q0, q1)))
    c0, c1, v1, u1 = hf.collinear_cases()
    z0, z1 = hf.coincident_cases()
    pairs = [(a, b) for _, p0, p1, _ in groups for a, b in zip(p0, p1)] + list(zip(c0, c1)) + list(zip(z0, z1))
    T, masks, cnt = _ransac(pairs, 1e300)
    o, d = hf.orthonormality(T)
    _report("orthonormality (all samples)", orth_u=o.max() / U, det_u=d.max() / U, samples=len(pairs))
    at, failed = 0, []
    for tag, p0, p1, ref in groups:
        rR, rt = hf.align_ratios(T[at:at + len(p0)], ref)
        kap = np.asarray(ref["s1"] / ref["s2"], np.float64)
        _report("align " + tag, s1_over_s2=float(np.median(kap)), R=rR.max(), t=rt.max(), abs_R=float(np.abs(np.asarray(hf._f(T[at:at + len(p0)]) - ref["T"], np.float64))[:, 3:].max()))
        if rR.max() > 1 or rt.max() > 1:
            failed.append((tag, rR.max(), rt.max()))
        at += len(p0)
    assert np.isfinite(T).all()
    assert (cnt == 3).all() and all(m.all() for m in masks)
    assert o.max() <= 16 * U and d.max() <= 16 * U
    assert not failed, failed
    Tc = T[at:at + len(c0)]
    Rv = np.einsum("brc,bc->br", hf._f(Tc)[:, 3:].reshape(-1, 3, 3), v1)
    err = float(np.abs(Rv - u1).max())
    _report("collinear", Rv1_u=err / U)
    assert err <= 16 * U
    # t = c1 - R c0 holds whatever R the completion chose
    for Tz, a, b in list(zip(Tc, c0, c1)) + list(zip(T[at + len(c0):], z0, z1)):
        want = hf._f(b).mean(0) - hf._f(Tz[3:]).reshape(3, 3) @ hf._f(a).mean(0)
        assert np.abs(np.asarray(hf._f(Tz[:3]) - want, np.float64)).max() <= 16 * U * (np.abs(a).mean(0).sum() + np.abs(b).mean(0).max())


def test_inlier_flags_and_counts_next_to_the_threshold():
    thresh = 4.0
    pairs = hf.inlier_pairs(CAM, thresh)
    T, masks, cnt = _ransac([(p0, p1) for p0, p1, _ in pairs], thresh)
    left_out = 0
    for (p0, p1, delta), Tp, m, c in zip(pairs, T, masks, cnt):
        ref = hf.align3(p0[None, :3], p1[None, :3])
        rR, rt = hf.align_ratios(Tp[None], ref)
        assert rR.max() <= 1 and rt.max() <= 1
        flag, decided = hf.inlier_decision(CAM, Tp, p0, p1, thresh)          # on the RETURNED transformation
        assert int(c) == int(m.sum()), (len(p0), c, m.sum())
        assert np.array_equal(m[decided], flag[decided]), (len(p0), np.nonzero(decided & (m != flag))[0])
        assert (np.abs(delta[~decided]) <= 1e-12).all()          # only rows built that close may be left out (nan compares false)
        assert decided[np.abs(delta) >= 1e-9].all()
        left_out += int((~decided).sum())
        _report(f"inlier n={len(p0)}", count=int(c), undecided=int((~decided).sum()), R=rR.max(), t=rt.max())
    _report("inlier rows left out", rows=left_out, of=int(sum(len(p[0]) for p in pairs)))


@pytest.mark.parametrize("num_iters", [257, 600])
def test_selection_takes_the_first_maximum_across_the_stride(num_iters):
    sp = hf.selection_problem(CAM, _samples(40, num_iters))
    ref = _reference(sp, num_iters)
    r = ref["pairs"][0]
    assert r["unambiguous"] and r["winner"] >= 256
    rc, poses, points, init, mcnt, icnt = _vo(sp, num_iters)
    assert rc == 0 and mcnt[0] == 40
    assert icnt[0] == r["count"][r["winner"]] == r["lo"][r["winner"]]
    d = np.abs(np.asarray(hf._f(poses[1]) - ref["poses"][1], np.float64))
    rR, rt = d[3:].max() / ref["chain_R"][1], d[:3].max() / ref["chain_t"][1]
    _report(f"selection iters={num_iters}", winner=int(r["winner"]), count=int(icnt[0]), R=float(rR), t=float(rt))
    assert rR <= 1 and rt <= 1


@pytest.mark.parametrize("shuffle", [False, True])
def test_matching_edges(shuffle):
    seq = hf.matching_edge_sequence(CAM, shuffle=shuffle)
    ref, _ = _compare_pipeline(f"matching shuffle={int(shuffle)}", seq, 16, 0)
    assert list(ref["match_count"]) == seq["shared"][1:]
    if not shuffle:
        bad = hf.matching_edge_sequence(CAM, plan=((255, None), (256, 2), (256, "all")))
        rc, _, _, _, mcnt, _ = _vo(bad, 16)
        assert rc == -3 and list(mcnt) == [2, 256]                # SSBA_ERR_NUMERICAL_FAILURE: fewer than three matches
        dup = hf.matching_edge_sequence(CAM, plan=((255, None), (255, "all"), (255, "all")))
        ids = dup["point_id"].copy()
        ids[255 + 7] = ids[255 + 6]                               # one landmark twice in state 1: its two lists differ in length
        dup["point_id"] = ids
        assert hf.match_states(ids[:255], ids[255:510]) is None
        rc, _, _, _, mcnt, _ = _vo(dup, 16)
        assert rc == -3 and mcnt[0] == 0 and mcnt[1] == 0


@pytest.mark.parametrize("S", [65, 66, 130])
def test_chain_across_its_chunks(S):
    seq = hf.make_sequence(CAM, S, seed=hf.CHAIN_SEED)
    _compare_pipeline(f"chain S={S}", seq, 16, (S - 1) // 20)
