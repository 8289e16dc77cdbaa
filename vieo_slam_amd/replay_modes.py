"""The sequential replay of replay.py for the other configurations of BASELINE.json -- ONE stream of frames with map growth,
a key frame every `kf_every` frames and its local bundle adjustment applied with the LocalMapping lag:

  RigReplay / RigTrackerReplay        distorted camera rigs, stereo + IMU: the reference's DEFAULT MH05 set-up (2 Radtan
                                      cameras, Examples/RunEuRoC/RunEuRoCVIO.sh:17-18), configs[3] (4 KB8 cameras) and
                                      configs[4] (TUM-VI: 2 KB8 cameras, 1500 features).  Frame::Frame = ExtractORB x
                                      n_cams + ComputeStereoFishEyeMatches (src/Frame.cc:259-316,613-779), the camera loop
                                      in both SearchByProjection overloads, per-camera edges in PoseOptimization and in
                                      LocalBundleAdjustmentNavStatePRV (src/Optimizer.cc:21-769); new map points from the
                                      good stereo groups (Tracking::CreateNewKeyFrame, src/Tracking.cc:2168-2306).
  VisionReplay / VisionTrackerReplay  configs[0]: rectified stereo WITHOUT IMU, 1000 features: TrackWithMotionModel +
                                      TrackLocalMap (src/Tracking.cc:1843-2008) with the constant-velocity prediction and
                                      UpdateLastFrame, vision-only PoseOptimization x 2, LocalBundleAdjustment
                                      (src/Optimizer.cc:1876-2307).

*Replay runs the frame stage by stage on a `stages` object (the C-ABI's host-pointer entries, or the CPU oracle in the
tests: tests/replay_oracle.py); *TrackerReplay runs a frame's tracking as ONE vieo_track_frame call.  The map, the key
frames, the local BA and the staged frame are replay.Replay's, the tracker call is tracker.TrackerCaller's: a mode here is
its constructor's data (the camera table, inertial, one_key_per_kf, lba_its, th_depth) and the few methods that differ.
Same simplifications as replay.Replay."""
from types import SimpleNamespace

import numpy as np

from . import replay, synth_ba, tracker
from . import synth_scene as sc
from .ba_types import POSE_FRAME_DTYPE

NLEVELS = 8


# ================================================================ camera rigs
class RigSequence(replay.Sequence):
    """replay.Sequence (trajectory, IMU samples) seen through the distorted cameras of synth_scene.RigScene."""

    def __init__(self, seed, n_frames, rig="radtan", n_cams=2, dt=0.05):
        super().__init__(seed, n_frames, dt)
        self.scene = sc.RigScene(seed, rig, n_cams)
        self.rig_name, self.n_cams = rig, n_cams

    def images(self, k):
        if k not in self._img:
            R, p, _, _, _ = self.state(self.time(k))
            self._img[k] = self.scene.frame(R, p, 1000 * self.seed + 10 * k)[0]
        return self._img[k]


class HipRigStages:
    """the hot-path calls of the rig replay through libvieo_hot.so (host-pointer entries)"""
    name = "hip"

    def __init__(self, nfeatures, n_cams):
        from .pipeline_rig import HipStages
        self.P = HipStages(nfeatures, n_cams)
        for n in ("extract", "fisheye", "project_last_frame", "search", "pose_vio", "in_frustum"):
            setattr(self, n, getattr(self.P, n))

    def scale_factors(self):
        return self.P.ext[0].GetScaleFactors()

    def preintegrate(self, noise, samples, ti, tj, bg, ba):
        from .imu import imu_preintegrate
        out, prv, st = imu_preintegrate(noise, [samples], [ti], [tj], [bg], [ba])
        return out[0], prv[0], int(st[0])

    def lba_vio(self, params, kfs, pts, close, obs, imu):
        from .optimizer import Optimizer
        return Optimizer.LocalBundleAdjustmentNavStatePRV(params, kfs, pts, close, obs, imu)

    def update_normal_depth(self, *a):
        from .map_point import update_normal_and_depth
        return update_normal_and_depth(*a)


class RigReplay(replay.Replay):
    def __init__(self, seq, stages, nfeatures=1200, **kw):
        from .pipeline_rig import RigFrontEnd
        super().__init__(seq, stages, **kw)
        self.scene, self.nfeatures = seq.scene, nfeatures
        self.fe = fe = RigFrontEnd(self.scene, nfeatures, stages=stages, th_last=self.th_last, th_local=self.th_local)
        # a key frame's keys that see a point: one per camera of the stereo group (a sorted set); ThDepth is 35 as it stands
        self.one_key_per_kf, self.th_depth = False, 35.0
        self.cams = self.scene.cams
        self._set_cameras(fe.rig, fe.K0, fe.bf, fe.bf / fe.K0[0], fe.bounds)

    # ---- Frame::Frame
    def make_frame(self, k):
        fr = self.fe.make_frame(self.seq.images(k))
        f = replay._Frame()
        f.k, f.t = k, self.seq.time(k)
        f.keys, f.desc, f.uright, f.depth, f.N = fr.keys, fr.desc, fr.uright, fr.depth, fr.N
        f.key_cam, f.cam_first = fr.key_cam, fr.cam_first
        f.key_group, f.group_good, f.group_idx, f.group_p3d = (fr.fe[n] for n in ("key_group", "group_good", "group_idx",
                                                                                  "group_p3d"))
        f.mp_ref = np.full(f.N, -1, np.int64)
        f.track_depth = np.full(f.N, np.inf, np.float32)
        return f

    # ---- Tracking::CreateNewKeyFrame: a point per good stereo group none of whose keys holds one; all the keys of the
    #      group then hold it (and observe it: one observation per (key frame, camera))
    def _new_point_candidates(self, kf):
        z, keys, Xc = [], [], []
        for g in np.nonzero(kf.group_good)[0]:
            ks = kf.group_idx[g]
            ks = [int(kf.cam_first[c] + ks[c]) for c in range(self.nc) if ks[c] >= 0]
            if ks and all(kf.mp_ref[i] < 0 for i in ks):
                z.append(float(kf.group_p3d[g][2]))
                keys.append(ks)
                Xc.append(kf.group_p3d[g])
        return np.array(z), keys, np.array(Xc).reshape(-1, 3)


class RigTrackerReplay(tracker.TrackerCaller, RigReplay):
    """every frame's tracking as ONE vieo_track_frame call on a rig tracker (vieo_tracker_create_rig)"""

    def __init__(self, seq, stages, nfeatures=1200, max_local_points=16384, prefetch=False, **kw):
        super().__init__(seq, stages, nfeatures, **kw)
        self._open_tracker(max_local_points, prefetch)

    def _make_tracker(self, max_local_points):
        prm, rg = tracker.rig_params(self.scene, self.nfeatures, max_local_points=max_local_points, th_last=self.th_last,
                                     th_local=self.th_local, noise=self.seq.noise[0], th_depth=self.th_depth)
        return tracker.Tracker(prm, rg)


# ================================================================ rectified stereo without IMU
NFEAT_VISION = 1000


class HipVisionStages(replay.HipStages):
    name = "hip"

    def __init__(self, resident=False):
        from .matching import ORBmatcher
        from .orb_extractor import ORBextractor
        self.extL = ORBextractor(NFEAT_VISION, replay.SCALE, NLEVELS, replay.INI_TH, replay.MIN_TH)
        self.extR = ORBextractor(NFEAT_VISION, replay.SCALE, NLEVELS, replay.INI_TH, replay.MIN_TH)
        self.M = ORBmatcher
        self.resident, self.resident_calls = bool(resident), 0

    def pose(self, F, obs):
        from .optimizer import Optimizer
        return Optimizer.PoseOptimization(F, obs)

    def lba(self, params, kfs, pts, obs):
        from .optimizer import Optimizer
        return Optimizer.LocalBundleAdjustment(params, kfs, pts, obs)


def _T_of(nav):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = synth_ba.quat_to_R(nav["q"]), nav["p"]
    return T


def _nav_of(T, like):
    n = like.copy()
    n["p"], n["q"] = T[:3, 3], synth_ba._R_to_quat(T[:3, :3])
    return n


class VisionReplay(replay.Replay):
    """configs[0].  The body pose plays the NavState's part (p, q; v and the biases are carried along untouched): the
    vision-only PoseOptimization takes the same vieo_pose_frame."""

    def __init__(self, seq, stages, th_local=1.0, **kw):
        super().__init__(seq, stages, th_local=th_local, **kw)
        # no IMU: the motion model, PoseOptimization, LocalBundleAdjustment with its 5 + 10 iterations (src/Optimizer.cc:
        # 2179-2258) on the observed key frames alone, no edge between key frames; the search goes through S.search
        self.inertial, self.lba_its, self.search_last = False, (5, 10), None
        self.velocity = None  # T_b(k-1)<-b(k): the constant-velocity model in the body frame

    def _anchor(self, f):
        """Tracking::UpdateLastFrame (src/Tracking.cc:1790-1841): the last frame's pose follows its reference key frame"""
        kf = self.kfs[f.ref_kf]
        return _T_of(kf.nav) @ f.T_rel

    def _set_ref(self, f):
        f.ref_kf = len(self.kfs) - 1
        f.T_rel = np.linalg.inv(_T_of(self.kfs[f.ref_kf].nav)) @ _T_of(f.nav)

    _after_keyframe = _set_ref  # the key frame is its own reference: T_rel = identity

    def initialise(self):
        super().initialise()
        self._set_ref(self.last)
        self.velocity = np.eye(4)

    def _predict(self, last, t):
        Twb_last = self._anchor(last)
        return SimpleNamespace(nav_last=_nav_of(Twb_last, last.nav), nav_pred=_nav_of(Twb_last @ self.velocity, last.nav))

    def _pose(self, p, nav, obs, marg):
        F = np.zeros(1, POSE_FRAME_DTYPE)
        F[0]["nav"] = nav
        self._camera_into(F[0])
        F[0]["n_obs"] = len(obs)
        r, o = self.S.pose(F, obs)
        return r, r, o

    def _obs(self, f):
        obs, idx = super()._obs(f)
        obs["flags"] = 0  # (the vision-only optimisation has no close-point gate)
        return obs, idx

    def _after_tracking(self, f, p):
        # mVelocity = Tcw_cur * Twc_last (src/Tracking.cc:1178-1189), here between the body poses
        self.velocity = np.linalg.inv(_T_of(p.nav_last)) @ _T_of(f.nav)
        self._set_ref(f)


class VisionTrackerReplay(tracker.TrackerCaller, VisionReplay):
    """every frame's tracking as ONE vieo_track_frame call on a vision-only tracker (params.vision_only = 1)"""

    def __init__(self, seq, stages, max_local_points=16384, prefetch=False, **kw):
        super().__init__(seq, stages, **kw)
        self._open_tracker(max_local_points, prefetch)

    def _make_tracker(self, max_local_points):
        prm = tracker.euroc_params(max_local_points, self.th_last, self.th_local, self.seq.noise[0])
        prm[0]["n_features"], prm[0]["vision_only"] = NFEAT_VISION, 1
        return tracker.Tracker(prm)
