"""The README's end-to-end scenes with and without the two-view bundle adjustment, in one run on the GPU: the stereo
block-texture pair, the two-distance scene in both directions (integer keyframes with the uniform PnP, and sub-pixel level
keyframes with the level-aware PnP) and the raw-camera scene after rectification.  Per scene the error of the PnP fit and of
the adjusted fit against the plant: the largest translation component in metres and the rotation angle in radians.  The
stereo scenes use their real baseline of 0.2 m; the two-distance scene is RGB-D and uses the virtual default of 0.1 m.
Prints one JSON line.

    python tools/scenes_visual_ba.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))


def errors(T, plant_t, plant_R=None):
    R = T[:3, :3] if plant_R is None else T[:3, :3] @ plant_R.T
    return (round(float(np.abs(T[:3, 3] - plant_t).max()), 4), round(float(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))), 4))


def record(reg, plant_t, bound=None):
    out = {"matches": len(reg.matches), "pnp_inliers": int(np.count_nonzero(reg.pnp.inliers)), "pnp": errors(reg.pnp.transformation, plant_t),
           "adjusted_inliers": int(np.count_nonzero(reg.inliers)), "adjusted": errors(reg.transformation, plant_t), "status": reg.status,
           "steps": reg.ba_steps, "rounds_discarded": reg.rounds_discarded, "cost": [round(reg.cost_before, 3), round(reg.cost_after, 3)]}
    if bound is not None:
        out["bound_m"] = round(bound, 4)
        out["pnp_inside"], out["adjusted_inside"] = bool(out["pnp"][0] <= bound), bool(out["adjusted"][0] <= bound)
    return out


def main():
    import feat_pyramid_reference as pyr_ref
    import feat_reference
    import rectify_reference
    from cslam_amd import _lib
    from cslam_amd.front_end import rectify as rc
    from cslam_amd.front_end import visual_pyramid as vp
    from cslam_amd.front_end import visual_registration as vr
    from cslam_amd.front_end import visual_stereo as vs
    _lib.require_gpu()
    out = {}
    # the stereo block texture: disparity 10 = 2 m at fx 100, baseline 0.2 m, the views 0.32 m apart
    tex = feat_reference.block_texture(120, 200, seed=7)
    cut = lambda a: np.ascontiguousarray(tex[:, a:a + 160])
    cam = (100.0, 100.0, 80.0, 60.0, 0.2)
    kf_from, kf_to = vs.extract_keyframes_stereo([cut(0), cut(16)], [cut(10), cut(26)], cam)
    out["stereo"] = record(vr.register_pairs_ba([(kf_from, kf_to)], cam[:4], baselines=cam[4])[0], np.array([-0.32, 0.0, 0.0]), 0.04)
    # the two-distance scene (RGB-D): the plane at 2.88 m (A) and 2.0 m (B), 4 levels
    A, B, dA, dB = pyr_ref.scene()
    scam = np.array(pyr_ref.SCENE_CAMERA)
    W = pyr_ref.scene_transform()
    t_bound, _ = pyr_ref.scene_bounds()
    plain = vp.extract_keyframes_pyramid([A, B], [dA, dB], scam, levels=4)
    fine = vp.extract_level_keyframes([A, B], [dA, dB], scam, levels=4)
    for name, i_from, i_to, plant in (("B->A", 1, 0, W), ("A->B", 0, 1, np.linalg.inv(W))):
        for kind, kfs in (("integer keyframes, uniform PnP", plain), ("sub-pixel level keyframes, level-aware PnP", fine)):
            reg = vr.register_pairs_ba([(kfs[i_from], kfs[i_to])], scam)[0]
            out["two distances %s, %s" % (name, kind)] = record(reg, plant[:3, 3], t_bound)
    # the raw-camera scene: the stereo scene behind distorted, rotated cameras, rectified on the GPU
    lefts, rights, lc, rcam = rectify_reference.scene()
    H, Wd = rectify_reference.SCENE_SIZE
    raw = lambda v: rc.RawCamera(v[:4], v[4:12], v[12:21], v[21:26], (H, Wd))
    left, right = raw(lc), raw(rcam)
    rcam5 = rc.stereo_camera(left, right)
    (kf_from, kf_to), _ = rc.extract_keyframes_stereo_raw(lefts, rights, left, right)
    out["raw cameras"] = record(vr.register_pairs_ba([(kf_from, kf_to)], rcam5[:4], baselines=rcam5[4])[0], np.array(rectify_reference.SCENE_PLANT), 0.04)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
