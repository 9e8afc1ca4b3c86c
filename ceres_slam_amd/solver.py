"""Array-level handle over the C ABI (include/ssba.h) for the bench harness, the parity
tests and multi-GPU drivers: one ``StereoBA`` = one ``ssba_problem``.

Everything here is a direct call into libssba.so; numpy is used for host buffers only.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import capi


class DoglegStep(NamedTuple):
    """What ssba_dogleg_step returns (include/ssba.h): the Gauss-Newton step and v of the poses, landmarks and free shared
    blocks, the six sums |gradient_|^2, |gn|_D^2, gradient_ . gn, |J v|^2, |J gn|^2, Jv . Jgn, and the scalar chain."""
    gn_p: np.ndarray
    gn_l: np.ndarray
    gn_b: np.ndarray
    v_p: np.ndarray
    v_l: np.ndarray
    v_b: np.ndarray
    sums: np.ndarray
    alpha: float
    beta: float
    gamma: float
    step_norm: float
    mcc: float
    one_dim: bool
    sub_e: np.ndarray
    sub_g: np.ndarray
    sub_B: np.ndarray


class StereoBA:
    def __init__(self, camera: dict, poses: np.ndarray, points: np.ndarray, obs_pose, obs_point, obs_uvd,
                 stiffness, pose_const=None, huber_a: float = 0.0, device: int = -1, finalize: bool = True,
                 world_size: int = 1, rank: int = 0, lighting: dict = None, shared_free: int = 0, use_bounds: bool = False, points_const: bool = False,
                 partition=None, pose_factors=None, point_const=None):
        self.poses = np.ascontiguousarray(poses, dtype=np.float64)     # caller-owned blocks, updated in place
        self.points = np.ascontiguousarray(points, dtype=np.float64)
        self._obs_pose = np.ascontiguousarray(obs_pose, dtype=np.uint32)
        self._obs_point = np.ascontiguousarray(obs_point, dtype=np.uint32)
        self._obs_uvd = np.ascontiguousarray(obs_uvd, dtype=np.float64)
        S = np.asarray(stiffness, dtype=np.float64)
        self._S_obs = None
        if S.ndim == 3:      # one 3x3 stiffness per residual block (tests/dataset_vo_sun.cpp:56-65)
            self._S_obs = np.ascontiguousarray(S.reshape(-1, 9))
            assert self._S_obs.shape[0] == self._obs_pose.shape[0]
        else:
            self._S = np.ascontiguousarray(S.reshape(9))
        self._create(camera, device)
        P, L = self.poses.shape[0], self.points.shape[0]
        capi.check(self.lib.ssba_add_pose_blocks(self.h, capi.dptr(self.poses), P), "ssba_add_pose_blocks")
        capi.check(self.lib.ssba_add_point_blocks(self.h, capi.dptr(self.points), L), "ssba_add_point_blocks")
        if self._S_obs is None:
            capi.check(self.lib.ssba_add_stereo_observations(
                self.h, self._obs_pose.ctypes.data_as(capi._u32p), self._obs_point.ctypes.data_as(capi._u32p),
                capi.dptr(self._obs_uvd), self._obs_pose.shape[0], capi.dptr(self._S)), "ssba_add_stereo_observations")
        else:                # runs of equal stiffness go in one call each, as the C++ shim lowers them
            n = self._obs_pose.shape[0]
            cut = np.flatnonzero(np.any(self._S_obs[1:] != self._S_obs[:-1], axis=1)) + 1
            for b, e in zip(np.concatenate([[0], cut]), np.concatenate([cut, [n]])):
                b, e = int(b), int(e)
                capi.check(self.lib.ssba_add_stereo_observations(
                    self.h, self._obs_pose[b:e].ctypes.data_as(capi._u32p), self._obs_point[b:e].ctypes.data_as(capi._u32p),
                    capi.dptr(self._obs_uvd[b:e]), e - b, capi.dptr(self._S_obs[b])), "ssba_add_stereo_observations")
        if pose_const is None:
            pose_const = np.zeros(P, dtype=bool)
            if P:
                pose_const[0] = True              # tests/dataset_vo.cpp:62
        for k in np.nonzero(np.asarray(pose_const))[0]:
            capi.check(self.lib.ssba_set_pose_constant(self.h, int(k), 1), "ssba_set_pose_constant")
        if huber_a > 0:
            capi.check(self.lib.ssba_set_huber_loss(self.h, float(huber_a)), "ssba_set_huber_loss")
        for f in (pose_factors or []):      # dicts as for oracle.OracleProblem: pose, type (0 prior / 1 sun), data, stiffness, huber
            dat = np.ascontiguousarray(f["data"], dtype=np.float64).ravel()
            S = np.ascontiguousarray(f["stiffness"], dtype=np.float64).ravel()
            if f["type"] == 2:      # RelativePoseErrorAutomatic between pose and pose2 (tests/blowup_test.cpp:70-76)
                capi.check(self.lib.ssba_add_relative_pose(self.h, int(f["pose"]), int(f["pose2"]), capi.dptr(np.ascontiguousarray(dat[:12])),
                                                           capi.dptr(S), float(f.get("huber", 0.0))), "ssba_add_relative_pose")
            elif f["type"] == 0:
                capi.check(self.lib.ssba_add_pose_prior(self.h, int(f["pose"]), capi.dptr(dat), capi.dptr(S), float(f.get("huber", 0.0))),
                           "ssba_add_pose_prior")
            else:
                obs, exp = np.ascontiguousarray(dat[:3]), np.ascontiguousarray(dat[3:6])
                capi.check(self.lib.ssba_add_sun_observation(self.h, int(f["pose"]), capi.dptr(obs), capi.dptr(exp), capi.dptr(S),
                                                             float(dat[6]), float(dat[7]), float(f.get("huber", 0.0))),
                           "ssba_add_sun_observation")
        self.shared_free = int(shared_free)
        self.use_bounds = bool(use_bounds)
        if lighting is not None:
            self._add_lighting(lighting)
        if points_const:      # stage 2 of --multistage (tests/dataset_ba_phong.cpp:210-228)
            capi.check(self.lib.ssba_set_point_blocks_constant(self.h, 1), "ssba_set_point_blocks_constant")
        if point_const is not None:      # boolean mask over the points: those position blocks are held constant (stereo problems)
            mask = np.asarray(point_const, dtype=bool)
            if mask.shape != (L,):
                raise ValueError(f"point_const has shape {mask.shape}, expected ({L},)")
            idx = np.ascontiguousarray(np.flatnonzero(mask), dtype=np.uint32)
            capi.check(self.lib.ssba_set_point_constant(self.h, idx.ctypes.data_as(capi._u32p), idx.shape[0], 1), "ssba_set_point_constant")
        if world_size > 1:
            capi.check(self.lib.ssba_set_distributed(self.h, world_size, rank), "ssba_set_distributed")
            if partition is not None:     # separator super-blocks of a super-block-aligned sharding (sharding.aligned_partition)
                sep = np.ascontiguousarray(partition, dtype=np.uint32)
                capi.check(self.lib.ssba_set_partition(self.h, sep.ctypes.data_as(capi._u32p), sep.shape[0]), "ssba_set_partition")
        if finalize:
            self.finalize()

    def _create(self, camera: dict, device: int):
        """The handle and the fields every method of the class reads, whatever blocks the constructor then adds."""
        self.lib = capi.load()
        self.h = C.c_void_p()
        self._xcb = None            # keeps the exchange trampoline alive (set_exchange)
        self.normals = None         # lighting terms (_add_lighting)
        cam = capi.Camera(**camera)
        capi.check(self.lib.ssba_create(C.byref(cam), device, C.byref(self.h)), "ssba_create")

    def _add_lighting(self, lt: dict):
        """Config-3 terms (include/ssba.h "config 3"); `lt` has the keys of synth.PhongData.as_oracle_dict()."""
        L, N = self.points.shape[0], self._obs_pose.shape[0]
        self.normals = np.ascontiguousarray(lt["normals"], dtype=np.float64).copy()   # caller-owned block, updated in place
        # shared blocks: caller-owned, updated in place when free (shared_free: bit 0 light, 1 Phong, 2 texture)
        self.phong = np.ascontiguousarray(lt["phong"], dtype=np.float64).copy()
        self.texture = np.ascontiguousarray(lt["texture"], dtype=np.float64).copy()
        self.light = np.ascontiguousarray(lt["light"], dtype=np.float64).copy()
        self._mat = np.ascontiguousarray(lt["material_of_point"], dtype=np.uint32)
        self._int = np.ascontiguousarray(lt["intensity"], dtype=np.float64)
        self._nobs = np.ascontiguousarray(lt["normal_obs"], dtype=np.float64)
        self._Sn = np.ascontiguousarray(np.asarray(lt["normal_stiffness"], dtype=np.float64).reshape(9))
        assert self.normals.shape == (L, 3) and self._int.shape == (N,) and self._nobs.shape == (N, 3)
        capi.check(self.lib.ssba_add_normal_blocks(self.h, capi.dptr(self.normals), L), "ssba_add_normal_blocks")
        capi.check(self.lib.ssba_add_material_blocks(self.h, capi.dptr(self.phong), capi.dptr(self.texture), self.texture.shape[0],
                                                     self._mat.ctypes.data_as(capi._u32p), L), "ssba_add_material_blocks")
        capi.check(self.lib.ssba_add_light_block(self.h, capi.dptr(self.light), int(lt["light_type"])), "ssba_add_light_block")
        for which in range(3):
            capi.check(self.lib.ssba_set_shared_block_constant(self.h, which, 0 if (self.shared_free >> which) & 1 else 1),
                       "ssba_set_shared_block_constant")
        if self.use_bounds:      # tests/dataset_ba_phong.cpp:142-180
            inf = float("inf")
            for which, index, lo, hi in ((1, 0, 0.0, 1.0), (1, 1, 0.0, 1.0), (1, 2, 1.0, inf), (2, 0, 0.0, 1.0)):
                capi.check(self.lib.ssba_set_shared_block_bounds(self.h, which, index, lo, hi), "ssba_set_shared_block_bounds")
        capi.check(self.lib.ssba_add_lighting_observations(self.h, capi.dptr(self._int), float(lt["int_stiffness"]),
                                                           capi.dptr(self._nobs), capi.dptr(self._Sn), N),
                   "ssba_add_lighting_observations")

    @classmethod
    def from_synth(cls, prob, **kw):
        return cls(prob.camera, prob.poses_init.copy(), prob.points_init.copy(), prob.obs_pose, prob.obs_point,
                   prob.obs_uvd, prob.stiffness(), **kw)

    def finalize(self):
        capi.check(self.lib.ssba_finalize(self.h), "ssba_finalize")

    def close(self):
        if self.h:
            self.lib.ssba_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- solving ----------------------------------------------------------------
    def solve(self, options: capi.Options = None):
        o = options or capi.default_options(max_num_iterations=1000, use_nonmonotonic_steps=1)
        s = capi.Summary()
        rc = self.lib.ssba_solve(self.h, C.byref(o), C.byref(s))
        if rc not in (0, -3):
            capi.check(rc, "ssba_solve")
        return s, self.iteration_log()

    def solve_begin(self, options: capi.Options, ignore_convergence: bool = False):
        self._opts = options
        capi.check(self.lib.ssba_solve_begin(self.h, C.byref(options), int(ignore_convergence)), "ssba_solve_begin")

    def step(self, n: int = 1):
        capi.check(self.lib.ssba_solve_step(self.h, n), "ssba_solve_step")

    def restart(self):
        capi.check(self.lib.ssba_solve_restart(self.h), "ssba_solve_restart")

    def synchronize(self):
        capi.check(self.lib.ssba_synchronize(self.h), "ssba_synchronize")

    def solve_end(self):
        s = capi.Summary()
        rc = self.lib.ssba_solve_end(self.h, C.byref(s))
        if rc not in (0, -3):
            capi.check(rc, "ssba_solve_end")
        return s

    def iteration_log(self):
        n = self.lib.ssba_iteration_log(self.h, 0, None, None, None, None, None, None, None)
        names = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius")
        cols = {k: np.zeros(n) for k in names}
        ok = np.zeros(n, dtype=np.int32)
        self.lib.ssba_iteration_log(self.h, n, *[capi.dptr(cols[k]) for k in names], ok.ctypes.data_as(capi._i32p))
        cols["step_is_successful"] = ok
        return cols

    @staticmethod
    def brief_report(s: capi.Summary) -> str:
        buf = C.create_string_buffer(256)
        capi.load().ssba_brief_report(C.byref(s), buf, 256)
        return buf.value.decode()

    # ---- streams / exchange / instrumentation --------------------------------------
    def set_stream(self, stream_ptr: int):
        capi.check(self.lib.ssba_set_stream(self.h, C.c_void_p(stream_ptr)), "ssba_set_stream")

    def set_exchange(self, fn):
        """fn(device_ptr: int, count: int, op: int) -> None, op 0 = sum, 1 = max."""
        if fn is None:
            self._xcb = None
            capi.check(self.lib.ssba_set_exchange(self.h, capi.EXCHANGE_FN(0), None), "ssba_set_exchange")
            return

        def tramp(ctx, ptr, count, op):
            try:
                fn(int(ptr), int(count), int(op))
                return 0
            except Exception:            # never let an exception cross the C ABI
                import traceback
                traceback.print_exc()
                return 1
        self._xcb = capi.EXCHANGE_FN(tramp)
        capi.check(self.lib.ssba_set_exchange(self.h, self._xcb, None), "ssba_set_exchange")

    @staticmethod
    def rccl_unique_id() -> bytes:
        """128 bytes from ncclGetUniqueId (rank 0 calls this and hands them to the other ranks)."""
        buf = C.create_string_buffer(128)
        capi.check(capi.load().ssba_rccl_unique_id(buf, 128), "ssba_rccl_unique_id")
        return buf.raw

    def set_rccl(self, unique_id: bytes):
        """Native exchange: the library enqueues ncclAllReduce itself on its stream (collective call, every rank)."""
        self._xcb = None
        buf = C.create_string_buffer(bytes(unique_id), 128)
        capi.check(self.lib.ssba_set_rccl(self.h, buf, 128), "ssba_set_rccl")

    @staticmethod
    def rccl_describe() -> str:
        """Which librccl.so file this process uses, its version, the IPC / debug environment (ssba_rccl_describe)."""
        buf = C.create_string_buffer(1024)
        capi.check(capi.load().ssba_rccl_describe(buf, 1024), "ssba_rccl_describe")
        return buf.value.decode(errors="replace")

    def rccl_ranks(self) -> int:
        """ncclCommCount of the handle's communicator; 0 when the exchange is not the native one."""
        n = C.c_int()
        capi.check(self.lib.ssba_rccl_ranks(self.h, C.byref(n)), "ssba_rccl_ranks")
        return n.value

    def exchange_size(self) -> int:
        n = C.c_uint64()
        capi.check(self.lib.ssba_exchange_size(self.h, C.byref(n)), "ssba_exchange_size")
        return n.value

    def set_kernel_timing(self, on: bool):
        capi.check(self.lib.ssba_set_kernel_timing(self.h, int(on)), "ssba_set_kernel_timing")

    def kernel_times(self) -> dict:
        rows = (capi.KernelTime * 32)()
        n = C.c_int32()
        capi.check(self.lib.ssba_kernel_times(self.h, rows, 32, C.byref(n)), "ssba_kernel_times")
        return {rows[i].name.decode(): (int(rows[i].launches), float(rows[i].total_ms)) for i in range(n.value)}

    def stats(self) -> capi.Stats:
        st = capi.Stats()
        capi.check(self.lib.ssba_get_stats(self.h, C.byref(st)), "ssba_get_stats")
        return st

    # ---- test hooks -------------------------------------------------------------------
    def evaluate(self):
        P, L = self.poses.shape[0], self.points.shape[0]
        cost = C.c_double()
        ld = 6 if self.normals is not None else 3
        g_p, g_l = np.zeros((P, 6)), np.zeros((L, ld))
        H_pp, H_ll = np.zeros((P, 6, 6)), np.zeros((L, ld, ld))
        capi.check(self.lib.ssba_evaluate(self.h, C.byref(cost), capi.dptr(g_p), capi.dptr(g_l), capi.dptr(H_pp),
                                          capi.dptr(H_ll)), "ssba_evaluate")
        return cost.value, g_p, g_l, H_pp, H_ll

    def pose_covariance(self, pose: int) -> np.ndarray:
        """6x6 block of (J^T J)^-1 of one pose in tangent space (ceres::Covariance, tests/dataset_vo_sun.cpp:159-183)."""
        cov = np.zeros((6, 6))
        capi.check(self.lib.ssba_pose_covariance(self.h, int(pose), capi.dptr(cov)), "ssba_pose_covariance")
        return cov

    def covariance_blocks(self, pairs) -> list:
        """Blocks of (J^T J)^-1 for (("pose" | "point", index), ("pose" | "point", index)) pairs in one call
        (ssba_covariance_blocks): 6 x 6 / 6 x 3 / 3 x 6 / 3 x 3 arrays in request order."""
        kinds = {"pose": capi.COV_POSE, "point": capi.COV_POINT, capi.COV_POSE: capi.COV_POSE, capi.COV_POINT: capi.COV_POINT}
        req = np.zeros((max(len(pairs), 1), 4), dtype=np.uint32)      # ssba_cov_block rows: kind_a, index_a, kind_b, index_b
        for i, ((ka, ia), (kb, ib)) in enumerate(pairs):
            req[i] = (kinds[ka], ia, kinds[kb], ib)
        req = req[:len(pairs)]
        dims = np.where(req[:, [0, 2]] == capi.COV_POINT, 3, 6)
        size = dims[:, 0] * dims[:, 1]
        off = np.concatenate([[0], np.cumsum(size)])
        out = np.zeros(max(int(off[-1]), 1))
        capi.check(self.lib.ssba_covariance_blocks(self.h, np.ascontiguousarray(req).ctypes.data_as(C.POINTER(capi.CovBlock)), len(pairs),
                                                   capi.dptr(out)), "ssba_covariance_blocks")
        return [out[off[i]:off[i + 1]].reshape(dims[i, 0], dims[i, 1]).copy() for i in range(len(pairs))]

    def pose_marginals(self) -> np.ndarray:
        """(P, 6, 6): every pose's marginal covariance in one call (zeros for constant poses)."""
        P = self.poses.shape[0]
        return np.array(self.covariance_blocks([(("pose", k), ("pose", k)) for k in range(P)])).reshape(P, 6, 6)

    def point_marginals(self) -> np.ndarray:
        """(L, 3, 3): every point's marginal covariance in one call."""
        L = self.points.shape[0]
        return np.array(self.covariance_blocks([(("point", j), ("point", j)) for j in range(L)])).reshape(L, 3, 3)

    def border_system(self):
        """Border blocks of the last lm_step (free shared blocks): S_pb, S_bb (damped), rhs_b, delta_b."""
        nb = C.c_uint32()
        capi.check(self.lib.ssba_border_system(self.h, C.byref(nb), None, None, None, None), "ssba_border_system")
        nb = int(nb.value)
        n = 6 * self.stats().num_free_poses
        S_pb, S_bb, rhs_b, db = np.zeros((n, max(nb, 1))), np.zeros((max(nb, 1), max(nb, 1))), np.zeros(max(nb, 1)), np.zeros(max(nb, 1))
        if nb:
            capi.check(self.lib.ssba_border_system(self.h, None, capi.dptr(S_pb), capi.dptr(S_bb), capi.dptr(rhs_b), capi.dptr(db)),
                       "ssba_border_system")
        return S_pb[:, :nb], S_bb[:nb, :nb], rhs_b[:nb], db[:nb]

    def lm_step(self, radius: float, options: capi.Options = None, want_S: bool = True):
        P, L = self.poses.shape[0], self.points.shape[0]
        n = 6 * self.stats().num_free_poses
        S = np.zeros((n, n)) if want_S else None
        rhs = np.zeros(n)
        dp, dl = np.zeros((P, 6)), np.zeros((L, 6 if self.normals is not None else 3))
        mcc = C.c_double()
        o = options or capi.default_options()
        capi.check(self.lib.ssba_lm_step(self.h, C.byref(o), radius, capi.dptr(S) if want_S else None, capi.dptr(rhs),
                                         capi.dptr(dp), capi.dptr(dl), C.byref(mcc)), "ssba_lm_step")
        return S, rhs, dp, dl, mcc.value

    def dogleg_step(self, radius: float, mu: float, options: capi.Options = None) -> DoglegStep:
        """One dogleg step from scratch (ssba_dogleg_step): options.dogleg_type picks TRADITIONAL / SUBSPACE."""
        P, L = self.poses.shape[0], self.points.shape[0]
        ld = 6 if self.normals is not None else 3
        nb = C.c_uint32()
        capi.check(self.lib.ssba_border_system(self.h, C.byref(nb), None, None, None, None), "ssba_border_system")
        nb = int(nb.value)
        gp, vp, gl, vl = np.zeros((P, 6)), np.zeros((P, 6)), np.zeros((L, ld)), np.zeros((L, ld))
        gb, vb = np.zeros(max(nb, 1)), np.zeros(max(nb, 1))
        sc = np.zeros(capi.DOGLEG_NUM_SCALARS)
        o = options or capi.default_options()
        capi.check(self.lib.ssba_dogleg_step(self.h, C.byref(o), radius, mu, capi.dptr(gp), capi.dptr(gl), capi.dptr(gb),
                                             capi.dptr(vp), capi.dptr(vl), capi.dptr(vb), capi.dptr(sc)), "ssba_dogleg_step")
        return DoglegStep(gn_p=gp, gn_l=gl, gn_b=gb[:nb], v_p=vp, v_l=vl, v_b=vb[:nb], sums=sc[0:6], alpha=sc[6], beta=sc[7],
                          gamma=sc[8], step_norm=sc[9], mcc=sc[10], one_dim=bool(sc[11]), sub_e=sc[12:16].reshape(2, 2),
                          sub_g=sc[16:18], sub_B=sc[18:21])

    def line_search_probe(self, alpha: float):
        """One evaluation of the projected line search's function along the step of the last lm_step / dogleg_step
        (ssba_line_search_probe): (ls_out (8), the trial point as a dict of poses, points, normals, light, phong, texture)."""
        out = np.zeros(8)
        if self.normals is None:      # no lighting terms: the call reports SSBA_ERR_STATE
            capi.check(self.lib.ssba_line_search_probe(self.h, float(alpha), capi.dptr(out), *([None] * 6)), "ssba_line_search_probe")
        c = dict(poses=np.zeros_like(self.poses), points=np.zeros_like(self.points), normals=np.zeros_like(self.normals),
                 light=np.zeros_like(self.light), phong=np.zeros_like(self.phong), texture=np.zeros_like(self.texture))
        capi.check(self.lib.ssba_line_search_probe(self.h, float(alpha), capi.dptr(out), *[capi.dptr(c[k]) for k in (
            "poses", "points", "normals", "light", "phong", "texture")]), "ssba_line_search_probe")
        return out, c


class ImageStep(NamedTuple):
    """What ssba_image_step returns (include/ssba.h): the rows, the damped reduced 6 x 6 system and the step."""
    cost: float
    residuals: np.ndarray       # (rows, cols), zero at pixels without a block
    J_pose: np.ndarray          # (rows, cols, 6)
    J_disp: np.ndarray          # (rows, cols)
    S: np.ndarray               # (6, 6)
    rhs: np.ndarray             # (6,)
    delta_pose: np.ndarray      # (6,)
    delta_disp: np.ndarray      # (rows, cols)
    mcc: float


class ImageAlignment(StereoBA):
    """Dense photometric alignment (ssba_add_image_blocks): one pose T_track_ref and one disparity block per reference pixel,
    the reference's ImageError blocks (tests/dense_stereo_test.cpp:94-136).  ``pose`` (12,) and ``disparity`` (rows, cols) are
    the caller-owned blocks, updated in place by a solve.  ``huber_a`` > 0 puts ceres::HuberLoss(huber_a) on every block
    (set_huber_loss changes it later, finalized or not); 0 is the NULL loss.  Solving, the stepwise calls, the iteration log,
    streams, kernel timing and stats are StereoBA's."""

    def __init__(self, camera: dict, pose, disparity, ref, track, gradx, grady, interpolation: int = capi.IMAGE_BILINEAR,
                 disparity_const: bool = False, device: int = -1, finalize: bool = True, huber_a: float = 0.0):
        self.pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(12)
        self.poses = self.pose.reshape(1, 12)           # (the view StereoBA's helpers use)
        self.disparity = np.ascontiguousarray(disparity, dtype=np.float64)
        rows, cols = self.disparity.shape
        self._imgs = [np.ascontiguousarray(a, dtype=np.float64) for a in (ref, track, gradx, grady)]
        for a in self._imgs:
            if a.shape != (rows, cols):
                raise ValueError(f"image of shape {a.shape}, expected {(rows, cols)}")
        self.points = np.zeros((0, 3))
        self._create(camera, device)
        capi.check(self.lib.ssba_add_image_blocks(self.h, capi.dptr(self.pose), capi.dptr(self.disparity), *[capi.dptr(a) for a in self._imgs],
                                                  rows, cols, int(interpolation)), "ssba_add_image_blocks")
        if disparity_const:
            capi.check(self.lib.ssba_set_disparity_blocks_constant(self.h, 1), "ssba_set_disparity_blocks_constant")
        if huber_a > 0.0:
            self.set_huber_loss(huber_a)
        if finalize:
            self.finalize()

    def set_huber_loss(self, a: float):
        """ssba_set_huber_loss on the image blocks: a > 0 the width, a <= 0 the NULL loss again; before or after finalize."""
        capi.check(self.lib.ssba_set_huber_loss(self.h, float(a)), "ssba_set_huber_loss")

    @classmethod
    def from_synth(cls, pair, **kw):
        return cls(pair.camera, pair.pose_init.copy(), pair.disparity.copy(), pair.ref, pair.track, pair.gradx, pair.grady, **kw)

    @classmethod
    def from_pyramid_level(cls, pyramid: "ImagePyramid", level: int, camera: dict, pose, disparity, interpolation: int = capi.IMAGE_BILINEAR,
                           disparity_const: bool = False, finalize: bool = True):
        """The handle of one pyramid level (ssba_add_image_level): the four images stay on the device.  ``camera`` is the camera
        of that level; ``disparity`` the caller-owned map of that level."""
        self = cls.__new__(cls)
        self.pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(12)
        self.poses = self.pose.reshape(1, 12)
        self.disparity = np.ascontiguousarray(disparity, dtype=np.float64)
        rows, cols = pyramid.shape(level)
        if self.disparity.shape != (rows, cols):
            raise ValueError(f"disparity of shape {self.disparity.shape}, level {level} is {(rows, cols)}")
        self._imgs = []
        self._pyramid = pyramid         # read at ssba_finalize
        self.points = np.zeros((0, 3))
        self._create(camera, pyramid.device)
        capi.check(self.lib.ssba_add_image_level(self.h, pyramid.h, int(level), capi.dptr(self.pose), capi.dptr(self.disparity), int(interpolation)),
                   "ssba_add_image_level")
        if disparity_const:
            capi.check(self.lib.ssba_set_disparity_blocks_constant(self.h, 1), "ssba_set_disparity_blocks_constant")
        if finalize:
            self.finalize()
        return self

    def solve(self, options: capi.Options = None):
        return super().solve(options or capi.default_options(use_nonmonotonic_steps=1))      # dense_stereo_test.cpp:120-125

    def image_step(self, radius: float, options: capi.Options = None) -> ImageStep:
        rows, cols = self.disparity.shape
        cost, mcc = C.c_double(), C.c_double()
        r, Jp, Jd, dd = np.zeros((rows, cols)), np.zeros((rows, cols, 6)), np.zeros((rows, cols)), np.zeros((rows, cols))
        S, rhs, dp = np.zeros((6, 6)), np.zeros(6), np.zeros(6)
        o = options or capi.default_options()
        capi.check(self.lib.ssba_image_step(self.h, C.byref(o), float(radius), C.byref(cost), capi.dptr(r), capi.dptr(Jp), capi.dptr(Jd),
                                            capi.dptr(S), capi.dptr(rhs), capi.dptr(dp), capi.dptr(dd), C.byref(mcc)), "ssba_image_step")
        return ImageStep(cost.value, r, Jp, Jd, S, rhs, dp, dd, mcc.value)


def solve_image_batch(alignments, options: capi.Options = None, ignore_convergence: bool = False):
    """ssba_image_solve_batch: the finalized ImageAlignment handles solved together, five launches per iteration of the whole
    batch.  Every member's pose, disparity map, summary and iteration_log() are bit-equal to its own solve().  Returns a list of
    (summary, status), status 0 or -3 (no usable solution: that member's blocks are left as they were); refusals raise."""
    alignments = list(alignments)
    n = len(alignments)
    lib = capi.load()
    o = options or capi.default_options(use_nonmonotonic_steps=1)
    hs = (C.c_void_p * max(n, 1))(*[a.h for a in alignments])
    sums = (capi.Summary * max(n, 1))()
    sts = (C.c_int32 * max(n, 1))()
    rc = lib.ssba_image_solve_batch(hs, n, C.byref(o), int(ignore_convergence), sums, sts)
    if rc != 0 and not (rc == -3 and any(s == -3 for s in sts) and all(s in (0, -3) for s in sts)):
        capi.check(rc, "ssba_image_solve_batch")
    return [(sums[k], int(sts[k])) for k in range(n)]


class PyramidLevel(NamedTuple):
    """What ssba_image_pyramid_level returns for one level, and the level-0 camera scaled to it."""
    ref_u8: np.ndarray          # (rows, cols) uint8
    track_u8: np.ndarray
    ref: np.ndarray             # (rows, cols) float64
    track: np.ndarray
    gradx: np.ndarray
    grady: np.ndarray
    disparity: np.ndarray       # None below disparity_level
    camera: dict                # None when the pyramid was given no camera


class ImagePyramid:
    """The dense driver's pre-processing on the device (ssba_image_pyramid_create; tests/dense_stereo_test.cpp:52-72): every
    level of the 8-bit pair halved as cv::pyrDown does, converted, Sobel gradients, and the disparity map of ONE level carried to
    the coarser ones.  ``camera`` is the level-0 camera (optional: level() and align() scale it).  set_huber_loss(a) gives every
    level's handle of align() / align_batch() that loss."""

    def __init__(self, ref_u8, track_u8, disparity, levels: int, disparity_level: int = 0,
                 gradient_source: int = capi.GRADIENT_OF_TRACKED, gradient_scale: float = 0.125, camera: dict = None, device: int = -1):
        self.lib = capi.load()
        self.h = C.c_void_p()
        ref_u8, track_u8 = (np.ascontiguousarray(a) for a in (ref_u8, track_u8))
        if ref_u8.dtype != np.uint8 or track_u8.dtype != np.uint8 or ref_u8.ndim != 2 or ref_u8.shape != track_u8.shape:
            raise ValueError("the pair must be two uint8 images of one shape")
        rows, cols = ref_u8.shape
        disparity = np.ascontiguousarray(disparity, dtype=np.float64)
        if 0 <= disparity_level < 32 and disparity.shape != (rows >> disparity_level, cols >> disparity_level):
            raise ValueError(f"disparity of shape {disparity.shape}, level {disparity_level} is {(rows >> disparity_level, cols >> disparity_level)}")
        self.rows, self.cols, self.levels, self.disparity_level, self.device = rows, cols, int(levels), int(disparity_level), device
        self.camera = dict(camera) if camera is not None else None
        u8 = C.POINTER(C.c_uint8)
        capi.check(self.lib.ssba_image_pyramid_create(ref_u8.ctypes.data_as(u8), track_u8.ctypes.data_as(u8), capi.dptr(disparity), rows, cols,
                                                      int(levels), int(disparity_level), int(gradient_source), float(gradient_scale), device,
                                                      C.byref(self.h)), "ssba_image_pyramid_create")

    @classmethod
    def create(cls, ref_u8, track_u8, disparity, levels: int, **kw):
        return cls(ref_u8, track_u8, disparity, levels, **kw)

    @classmethod
    def create_stereo(cls, ref_left_u8, ref_right_u8, track_u8, levels: int, disparity_level: int = 0, params: dict = None,
                      gradient_source: int = capi.GRADIENT_OF_TRACKED, gradient_scale: float = 0.125, camera: dict = None, device: int = -1):
        """The pyramid from what a stereo rig delivers (ssba_image_pyramid_create_stereo): the semi-global matcher runs on the
        two 8-bit reference images at disparity_level and its map stays on the device.  ``params``: the matcher's parameters
        (capi.sgbm_params keywords).  level(disparity_level).disparity downloads the map a handle or align() needs."""
        self = cls.__new__(cls)
        self.lib = capi.load()
        self.h = C.c_void_p()
        imgs = [np.ascontiguousarray(a) for a in (ref_left_u8, ref_right_u8, track_u8)]
        if any(a.dtype != np.uint8 or a.ndim != 2 or a.shape != imgs[0].shape for a in imgs):
            raise ValueError("the triple must be three uint8 images of one shape")
        rows, cols = imgs[0].shape
        self.rows, self.cols, self.levels, self.disparity_level, self.device = rows, cols, int(levels), int(disparity_level), device
        self.camera = dict(camera) if camera is not None else None
        u8 = C.POINTER(C.c_uint8)
        q = capi.sgbm_params(**(params or {}))
        capi.check(self.lib.ssba_image_pyramid_create_stereo(*[a.ctypes.data_as(u8) for a in imgs], rows, cols, int(levels), int(disparity_level),
                                                             C.byref(q), int(gradient_source), float(gradient_scale), device, C.byref(self.h)),
                   "ssba_image_pyramid_create_stereo")
        return self

    #: True for a pyramid handed out by an ImageSequence: it owns no device memory, close() only forgets the handle
    borrowed = False

    @classmethod
    def _borrow(cls, h, rows: int, cols: int, levels: int, disparity_level: int, camera: dict, device: int):
        self = cls.__new__(cls)
        self.lib = capi.load()
        self.h = C.c_void_p(h)
        self.borrowed = True
        self.rows, self.cols, self.levels, self.disparity_level, self.device = rows, cols, int(levels), int(disparity_level), device
        self.camera = dict(camera) if camera is not None else None
        return self

    def close(self):
        if self.h:
            if not self.borrowed:
                self.lib.ssba_image_pyramid_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_huber_loss(self, a: float):
        """ssba_image_pyramid_set_huber_loss: the width align and align_batch put on every level's blocks (a <= 0: NULL loss)."""
        capi.check(self.lib.ssba_image_pyramid_set_huber_loss(self.h, float(a)), "ssba_image_pyramid_set_huber_loss")

    def shape(self, level: int):
        if not 0 <= level < self.levels:
            raise ValueError(f"level {level} of a pyramid of {self.levels}")
        return self.rows >> level, self.cols >> level

    def level_camera(self, level: int, camera: dict = None) -> dict:
        """fu, fv, cu, cv over 2^level, b unchanged (pyrDown samples at even pixels)."""
        cam = camera if camera is not None else self.camera
        if cam is None:
            return None
        s = 0.5 ** level
        return dict(fu=cam["fu"] * s, fv=cam["fv"] * s, cu=cam["cu"] * s, cv=cam["cv"] * s, b=cam["b"])

    def level(self, level: int) -> PyramidLevel:
        rows, cols = self.shape(level)
        u8 = [np.zeros((rows, cols), np.uint8) for _ in range(2)]
        f64 = [np.zeros((rows, cols)) for _ in range(4)]
        disp = np.zeros((rows, cols)) if level >= self.disparity_level else None
        r, c = C.c_uint32(), C.c_uint32()
        capi.check(self.lib.ssba_image_pyramid_level(self.h, level, C.byref(r), C.byref(c), *[a.ctypes.data_as(C.POINTER(C.c_uint8)) for a in u8],
                                                     *[capi.dptr(a) for a in f64], capi.dptr(disp) if disp is not None else None),
                   "ssba_image_pyramid_level")
        assert (r.value, c.value) == (rows, cols)
        return PyramidLevel(u8[0], u8[1], *f64, disp, self.level_camera(level))

    def handle(self, level: int, camera: dict, pose, disparity, interpolation: int = capi.IMAGE_BILINEAR, disparity_const: bool = False,
               finalize: bool = True) -> ImageAlignment:
        """An ImageAlignment on one level through ssba_add_image_level.  ``camera`` is the camera OF THAT LEVEL (level_camera, or
        the caller's own, as the reference driver keeps its full-resolution one); None takes level_camera(level)."""
        cam = camera if camera is not None else self.level_camera(level)
        if cam is None:
            raise ValueError("no camera: pass one, or give the pyramid its level-0 camera")
        return ImageAlignment.from_pyramid_level(self, level, cam, pose, disparity, interpolation, disparity_const, finalize)

    def align(self, pose, disparity, coarsest_level: int = None, camera: dict = None, interpolation: int = capi.IMAGE_BILINEAR,
              disparity_const: bool = False, options: capi.Options = None):
        """Coarse to fine (ssba_image_pyramid_align) from ``coarsest_level`` (default: the coarsest) down to disparity_level.
        ``pose`` (12,) and ``disparity`` (the float64 map at disparity_level) are updated in place; ``camera`` is the LEVEL-0
        camera.  Returns (status, summaries): one summary per level solved, coarsest first."""
        cam = camera if camera is not None else self.camera
        if cam is None:
            raise ValueError("no camera: pass the level-0 camera, or give it to the pyramid")
        if not (isinstance(pose, np.ndarray) and pose.dtype == np.float64 and pose.flags.c_contiguous and pose.size == 12):
            raise ValueError("pose must be a contiguous float64 array of 12: it is updated in place")
        if not (isinstance(disparity, np.ndarray) and disparity.dtype == np.float64 and disparity.flags.c_contiguous):
            raise ValueError("disparity must be a contiguous float64 array: it is updated in place")
        if disparity.shape != self.shape(self.disparity_level):
            raise ValueError(f"disparity of shape {disparity.shape}, level {self.disparity_level} is {self.shape(self.disparity_level)}")
        top = self.levels - 1 if coarsest_level is None else int(coarsest_level)
        o = options or capi.default_options(use_nonmonotonic_steps=1)
        sums = (capi.Summary * max(top - self.disparity_level + 1, 1))()
        c = capi.Camera(**cam)
        rc = self.lib.ssba_image_pyramid_align(self.h, C.byref(c), capi.dptr(pose), capi.dptr(disparity), top, int(interpolation),
                                               int(disparity_const), C.byref(o), sums)
        if rc not in (0, -3):
            capi.check(rc, "ssba_image_pyramid_align")
        return rc, list(sums)


    @staticmethod
    def align_batch(pyramids, poses, disparities, coarsest_level: int = None, camera: dict = None, interpolation: int = capi.IMAGE_BILINEAR,
                    disparity_const: bool = False, options: capi.Options = None):
        """Coarse to fine over n pyramids in lockstep (ssba_image_pyramid_align_batch): one shared solve per level.  ``poses``
        (n, 12) and every map of ``disparities`` (float64, at disparity_level) are updated in place; ``camera`` is the level-0
        camera (default: the first pyramid's).  Returns (status, summaries, statuses): summaries[k] is pyramid k's list, coarsest
        level first; statuses[k] is 0, or what stopped pyramid k (it keeps its last usable pose).  Refusals raise."""
        pyramids = list(pyramids)
        n = len(pyramids)
        cam = camera if camera is not None else (pyramids[0].camera if n else None)
        if n and cam is None:
            raise ValueError("no camera: pass the level-0 camera, or give it to the first pyramid")
        if not (isinstance(poses, np.ndarray) and poses.dtype == np.float64 and poses.flags.c_contiguous and poses.size == 12 * n):
            raise ValueError("poses must be a contiguous float64 array of n x 12: it is updated in place")
        disparities = list(disparities)
        if len(disparities) != n:
            raise ValueError("one disparity map per pyramid")
        for k, d in enumerate(disparities):
            if not (isinstance(d, np.ndarray) and d.dtype == np.float64 and d.flags.c_contiguous):
                raise ValueError("every disparity map must be a contiguous float64 array: it is updated in place")
            lvl = pyramids[k].disparity_level
            if 0 <= lvl < pyramids[k].levels and d.shape != pyramids[k].shape(lvl):
                raise ValueError(f"disparity {k} of shape {d.shape}, level {lvl} is {pyramids[k].shape(lvl)}")
        lib = capi.load()
        dl = pyramids[0].disparity_level if n else 0
        top = (pyramids[0].levels - 1 if n else 0) if coarsest_level is None else int(coarsest_level)
        levels = max(top - dl + 1, 1)
        o = options or capi.default_options(use_nonmonotonic_steps=1)
        hs = (C.c_void_p * max(n, 1))(*[p.h for p in pyramids])
        maps = (capi._dp * max(n, 1))(*[capi.dptr(d) for d in disparities])
        sums = (capi.Summary * (max(n, 1) * levels))()
        sts = (C.c_int32 * max(n, 1))()
        c = capi.Camera(**cam) if cam is not None else capi.Camera()
        rc = lib.ssba_image_pyramid_align_batch(hs, n, C.byref(c), capi.dptr(poses), maps, top, int(interpolation), int(disparity_const),
                                                C.byref(o), sums, sts)
        if rc != 0 and not (any(s != 0 for s in sts) and rc == next(s for s in sts if s != 0)):
            capi.check(rc, "ssba_image_pyramid_align_batch")
        return rc, [[sums[k * levels + i] for i in range(levels)] for k in range(n)], [int(s) for s in sts]


def stereo_sgbm(left, right, device: int = -1, **params):
    """The semi-global matcher on a rectified 8-bit pair (ssba_stereo_sgbm; cv::StereoSGBM(0, 64, 15) as the dense driver calls it).
    ``params``: capi.sgbm_params keywords (min_disparity, num_disparities, block_size, p1, p2, disp12_max_diff, pre_filter_cap,
    uniqueness_ratio, ...).  Returns (disp16 int16, disparity float64 with NaN at invalid pixels)."""
    left, right = np.ascontiguousarray(left), np.ascontiguousarray(right)
    if left.dtype != np.uint8 or right.dtype != np.uint8 or left.ndim != 2 or left.shape != right.shape:
        raise ValueError("the pair must be two uint8 images of one shape")
    rows, cols = left.shape
    lib = capi.load()
    q = capi.sgbm_params(**params)
    disp16, disparity = np.zeros((rows, cols), np.int16), np.zeros((rows, cols))
    u8 = C.POINTER(C.c_uint8)
    capi.check(lib.ssba_stereo_sgbm(left.ctypes.data_as(u8), right.ctypes.data_as(u8), rows, cols, C.byref(q), device,
                                    disp16.ctypes.data_as(C.POINTER(C.c_int16)), capi.dptr(disparity)), "ssba_stereo_sgbm")
    return disp16, disparity


def pack_frames(lefts, rights):
    """The frame-major stacks ssba_image_sequence_create reads: (F, rows, cols) uint8 left frames and the (F - 1, rows, cols)
    right frames 0 ... F - 2, each contiguous.  ``rights`` may hold F or F - 1 frames; the last of F is not needed."""
    lefts = [np.asarray(a) for a in lefts]
    rights = [np.asarray(a) for a in rights]
    if len(lefts) < 2:
        raise ValueError("a sequence needs at least 2 frames")
    if len(rights) not in (len(lefts), len(lefts) - 1):
        raise ValueError(f"{len(lefts)} left frames need {len(lefts) - 1} or {len(lefts)} right frames, not {len(rights)}")
    if any(a.dtype != np.uint8 or a.ndim != 2 or a.shape != lefts[0].shape for a in lefts + rights):
        raise ValueError("the frames must be uint8 images of one shape")
    return np.ascontiguousarray(np.stack(lefts)), np.ascontiguousarray(np.stack(rights[:len(lefts) - 1]))


def _pack_pairs(lefts, rights):
    lefts = [np.asarray(a) for a in lefts]
    rights = [np.asarray(a) for a in rights]
    if len(lefts) != len(rights):
        raise ValueError("as many left images as right images")
    if lefts and any(a.dtype != np.uint8 or a.ndim != 2 or a.shape != lefts[0].shape for a in lefts + rights):
        raise ValueError("the pairs must be uint8 images of one shape")
    if not lefts:
        return np.zeros((0, 0, 0), np.uint8), np.zeros((0, 0, 0), np.uint8)
    return np.ascontiguousarray(np.stack(lefts)), np.ascontiguousarray(np.stack(rights))


def stereo_sgbm_batch(lefts, rights, workspace_bytes: int = 0, device: int = -1, **params):
    """stereo_sgbm over n pairs of one shape in shared launches (ssba_stereo_sgbm_batch).  ``workspace_bytes`` bounds the
    matcher's volumes (capi.sgbm_pair_bytes per pair; 0: 1 GiB): the pairs run in chunks of capi.sgbm_chunk_pairs.  Returns
    (disp16 (n, rows, cols) int16, disparity (n, rows, cols) float64), member k bit-equal to stereo_sgbm(lefts[k], rights[k])."""
    L, R = _pack_pairs(lefts, rights)
    n, rows, cols = L.shape
    lib = capi.load()
    q = capi.sgbm_params(**params)
    disp16, disparity = np.zeros((n, rows, cols), np.int16), np.zeros((n, rows, cols))
    u8 = C.POINTER(C.c_uint8)
    capi.check(lib.ssba_stereo_sgbm_batch(L.ctypes.data_as(u8), R.ctypes.data_as(u8), n, rows, cols, C.byref(q), int(workspace_bytes), device,
                                          disp16.ctypes.data_as(C.POINTER(C.c_int16)), capi.dptr(disparity)), "ssba_stereo_sgbm_batch")
    return disp16, disparity


class ImageSequence:
    """A rectified stereo sequence prepared once (ssba_image_sequence_create): every frame goes up once, every left frame's
    levels, double image and gradients are built once, and the semi-global matcher runs over all pairs (left_k, right_k) in
    shared launches.  pyramid(k) is the borrowed ImagePyramid of pair k (reference frame k, tracked frame k + 1), bit-equal to
    ImagePyramid.create_stereo(lefts[k], rights[k], lefts[k + 1], ...); it ends with the sequence."""

    def __init__(self, lefts, rights, levels: int, disparity_level: int = 0, params: dict = None, workspace_bytes: int = 0,
                 gradient_source: int = capi.GRADIENT_OF_TRACKED, gradient_scale: float = 0.125, camera: dict = None, device: int = -1):
        self.lib = capi.load()
        self.h = C.c_void_p()
        self._pyramids = {}
        L, R = pack_frames(lefts, rights)
        self.frames, self.rows, self.cols = L.shape
        self.levels, self.disparity_level, self.device = int(levels), int(disparity_level), device
        self.camera = dict(camera) if camera is not None else None
        u8 = C.POINTER(C.c_uint8)
        q = capi.sgbm_params(**(params or {}))
        capi.check(self.lib.ssba_image_sequence_create(L.ctypes.data_as(u8), R.ctypes.data_as(u8), self.frames, self.rows, self.cols, int(levels),
                                                       int(disparity_level), C.byref(q), int(workspace_bytes), int(gradient_source),
                                                       float(gradient_scale), device, C.byref(self.h)), "ssba_image_sequence_create")

    @classmethod
    def create(cls, lefts, rights, levels: int, **kw):
        return cls(lefts, rights, levels, **kw)

    @property
    def num_pairs(self) -> int:
        return self.frames - 1

    def pyramid(self, k: int) -> ImagePyramid:
        """The borrowed pyramid of pair k (ssba_image_sequence_pyramid): the same object on every call."""
        if not self.h:
            raise ValueError("the sequence is closed")
        if k not in self._pyramids:
            h = C.c_void_p()
            capi.check(self.lib.ssba_image_sequence_pyramid(self.h, int(k), C.byref(h)), "ssba_image_sequence_pyramid")
            self._pyramids[k] = ImagePyramid._borrow(h.value, self.rows, self.cols, self.levels, self.disparity_level, self.camera, self.device)
        return self._pyramids[k]

    def pyramids(self):
        return [self.pyramid(k) for k in range(self.num_pairs)]

    def disparities(self):
        """The F - 1 maps at disparity_level, downloaded: what align() and a handle's block list need."""
        return [self.pyramid(k).level(self.disparity_level).disparity for k in range(self.num_pairs)]

    def align(self, poses, disparities=None, coarsest_level: int = None, camera: dict = None, interpolation: int = capi.IMAGE_BILINEAR,
              disparity_const: bool = False, options: capi.Options = None):
        """ImagePyramid.align_batch over the borrowed pyramids: ``poses`` (F - 1, 12) and the maps are updated in place
        (``disparities`` None: the sequence's own maps are downloaded).  Returns (status, summaries, statuses, disparities)."""
        maps = self.disparities() if disparities is None else list(disparities)
        rc, sums, sts = ImagePyramid.align_batch(self.pyramids(), poses, maps, coarsest_level, camera if camera is not None else self.camera,
                                                 interpolation, disparity_const, options)
        return rc, sums, sts, maps

    def close(self):
        """ssba_image_sequence_destroy: the borrowed pyramids end here."""
        if self.h:
            for p in self._pyramids.values():
                p.h = C.c_void_p()
            self._pyramids = {}
            self.lib.ssba_image_sequence_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
