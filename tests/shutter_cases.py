"""Cases and the reference of the shutter-frame tests (sr.h "Shutter frames").

Output frame m of a shutter call is the rounded mean of K sub-frames; sub-frame
j = m K + k is one phase of the sample frame of scene first + j and cams[j].
The reference of every comparison, with no tolerance, is built from the CPU
oracle alone:

    sub_j = oracle.render(scene_j, cam_j, params, ss W, ss H)[py::ss, px::ss]
    out_m = min(255, (sum_k sub_{mK+k} + K // 2) // K)          (numpy, integers)

The cases are chosen so that a wrong kernel cannot pass: a launch that read a
neighbouring sub-frame's scene or camera, resolved one sub-frame alone, froze
the group at its first scene and camera, or wrote a frame to its neighbour's
place gives a frame that differs from the reference on at least 10 % of the
pixels (premise(); tests/test_shutter_cases.py asserts it with the oracle
alone at 68x44 and 400 steps).

  view_k4_ss2   ORBIT40 from scene 0, the static camera "view", 4 frames of 4
                sub-frames, ss 2, default phases
  view_k3_ss1   the same with 3 sub-frames at ss 1
  flyby_k4_ss2  ORBIT40 with the flyby camera at the sub-frames' times
                (m + (k + 1/2) / K) / M
  own_k4_ss2    the context's own scene ("general") under that moving camera
  mix_k2_ss1    MIX: slot, cylinder and object counts change per sub-frame

Scenes, named cameras, test rays, params and textures are World's
(tests/test_gpu_launch_matrix.py) through sequence_cases.Sequences, whose
frame cache the modules of a session share.
"""
import numpy as np

from sequence_cases import Sequences, differing_pixels
from test_gpu_launch_matrix import STEPS, H, W

OWN = -1  # SR_SHUTTER_OWN_SCENE
PREMISE = 0.10  # every wrong frame differs from the reference on at least this share of the pixels


class Case:
    """M frames of K sub-frames at ss: the scenes (`seq` from `first`, or the
    World scene `own`), one camera name per sub-frame (World.cams keys; one
    more than M K, for the premise's shifted groups) and the phase pairs
    (None: the default order)."""

    def __init__(self, name, M, K, ss, cams, seq=None, first=0, own=None, phases=None):
        assert (seq is None) != (own is None) and len(cams) >= M * K
        self.name, self.M, self.K, self.ss = name, M, K, ss
        self.cams, self.seq, self.first, self.own, self.phases = list(cams), seq, first, own, phases

    @property
    def n(self):
        return self.M * self.K

    @property
    def first_scene(self):
        return OWN if self.seq is None else self.first


class Shutter:
    """Sequences with the shutter cases, their sub-frames and references."""

    def __init__(self, pkg, oracle, textures):
        self.pkg, self.oracle = pkg, oracle
        self.sq = Sequences(pkg, oracle, textures)
        self.wd = self.sq.wd
        self._own = {}

    # ---- cameras: the flyby at a time, registered under a name of World.cams
    def flyby(self, t):
        name = f"flyby@{t:.9f}"
        if name not in self.wd.cams:
            self.wd.cams[name] = self.pkg.abi.camera_flyby(float(t), 30.0, 10.0)
        return name

    def flyby_cams(self, M, K, extra=1, angle=360.0):
        """The camera of sub-frame j = m K + k at time (m + (k + 1/2) / K * angle / 360) / M"""
        return [self.flyby(((j // K) + ((j % K) + 0.5) / K * angle / 360.0) / M) for j in range(M * K + extra)]

    def cam(self, name):
        return self.wd.cams[name]

    def case(self, name):
        M = 4
        return {
            "view_k4_ss2": lambda: Case(name, M, 4, 2, ["view"] * (M * 4 + 4 + 1), seq="ORBIT40"),
            "view_k3_ss1": lambda: Case(name, M, 3, 1, ["view"] * (M * 3 + 3 + 1), seq="ORBIT40"),
            "flyby_k4_ss2": lambda: Case(name, M, 4, 2, self.flyby_cams(M, 4, 4 + 1), seq="ORBIT40"),
            "own_k4_ss2": lambda: Case(name, M, 4, 2, self.flyby_cams(M, 4, 4 + 1), own="general"),
            "mix_k2_ss1": lambda: Case(name, 2, 2, 1, ["view"] * 6, seq="MIX"),
        }[name]()

    # ---- the reference
    def phases(self, case, n=None):
        """[n, 2] {x, y}: the case's pairs, or the default ones (sr_phase_order by position in the group)"""
        n = case.n if n is None else n
        if case.phases is not None:
            return np.asarray(case.phases, dtype=np.uint8).reshape(-1, 2)[:n]
        order = self.pkg.abi.phase_order(case.ss)
        return np.array([order[(j % case.K) % (case.ss * case.ss)] for j in range(n)], dtype=np.uint8)

    def sample_frame(self, case, j, cam, w, h, overlay=False, params=None, tag=None):
        """The oracle's RGBA8 sample frame (ss w) x (ss h) of sub-frame j's scene under World camera `cam`"""
        ss = case.ss
        if params is not None:
            key = (case.seq, case.own, case.first + j if case.seq else 0, cam, ss * w, ss * h, overlay, tag)
            if key not in self._own:
                scene = self.sq.scenes(case.seq)[case.first + j] if case.seq else self.wd.scene(case.own)
                out = self.oracle.render(scene, self.cam(cam), params, ss * w, ss * h, self.wd.tex,
                                         self.wd.test_rays[overlay])[0]
                out.setflags(write=False)
                self._own[key] = out
            return self._own[key]
        if case.seq is not None:
            return self.sq.ref(case.seq, case.first + j, overlay, cam, ss * w, ss * h)[0]
        return self.wd.ref(case.own, overlay, cam, ss * w, ss * h)[0]

    def sub_frame(self, case, j, w=W, h=H, overlay=False, scene_j=None, cam_j=None, phase_j=None, params=None, tag=None):
        """Sub-frame j: phase phase_j's (default: j's) image of scene scene_j's (j's) sample frame under camera cam_j's (j's)"""
        sj = j if scene_j is None else scene_j
        cj = j if cam_j is None else cam_j
        px, py = (int(v) for v in self.phases(case, max(case.n, j + 1, (phase_j or 0) + 1))[j if phase_j is None else phase_j])
        S = self.sample_frame(case, sj, case.cams[cj], w, h, overlay, params, tag)
        return S[py::case.ss, px::case.ss]

    @staticmethod
    def resolve(subs):
        """min(255, (sum + K // 2) // K) of K sub-frames, in integers"""
        k = len(subs)
        total = sum(s.astype(np.int64) for s in subs)
        return np.minimum(255, (total + k // 2) // k).astype(np.uint8)

    def frame(self, case, m, w=W, h=H, overlay=False, shift=0, still=False, params=None, tag=None):
        """Output frame m; shift: its sub-frames' scenes and cameras moved on by
        that many sub-frames (the phases stay by position); still: all of them
        the group's first scene and camera"""
        K = case.K
        subs = []
        for k in range(K):
            j = m * K + k
            src = m * K + shift if still else j + shift
            subs.append(self.sub_frame(case, j, w, h, overlay, scene_j=src, cam_j=src, phase_j=j, params=params, tag=tag))
        return self.resolve(subs)

    def reference(self, case, w=W, h=H, overlay=False, params=None, tag=None):
        """[M, h, w, 4]"""
        return np.stack([self.frame(case, m, w, h, overlay, params=params, tag=tag) for m in range(case.M)])

    # ---- the premise
    def premise(self, case, w=W, h=H):
        """Per output frame m: the share of pixels on which it differs from
        (shifted by one sub-frame, the nearest of its own sub-frames, the
        still frame, the next output frame). The next frame of the last one
        is frame M, whose sub-frames the case's cameras and scenes reach
        where they can (None where they do not)."""
        rows = []
        for m in range(case.M):
            out = self.frame(case, m, w, h)
            px = float(out.shape[0] * out.shape[1])
            shifted = differing_pixels(out, self.frame(case, m, w, h, shift=1)) / px
            own = min(differing_pixels(out, self.sub_frame(case, m * case.K + k, w, h)) for k in range(case.K)) / px
            still = differing_pixels(out, self.frame(case, m, w, h, still=True)) / px
            nxt = None
            if (m + 2) * case.K <= len(case.cams) and (case.seq is None or
                                                     case.first + (m + 2) * case.K <= len(self.sq.scenes(case.seq))):
                nxt = differing_pixels(out, self.frame(case, m + 1, w, h)) / px
            rows.append((shifted, own, still, nxt))
        return rows
