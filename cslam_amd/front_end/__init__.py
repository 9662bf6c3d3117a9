"""The front end on the GPU: what a visual keyframe carries, from the image (visual_features.py) or from a stereo pair
(visual_stereo.py), either over a scale pyramid (visual_pyramid.py), the geometric verification of loop closures between such keyframes (visual_registration.py), and the depth image
and coloured cloud of a stereo keyframe (stereo_depth.py; the RGB-D one is keyframe_clouds.py).  A camera driver's raw frames are
undistorted and rectified in front of all of these by rectify.py."""
from .visual_features import (back_project, corner_response, describe, extract_features, extract_keyframes, is_new_keyframe,  # noqa: F401
                              select_keypoints, to_gray)
from .visual_registration import Keyframe, compute_transformation, register_pairs  # noqa: F401
from .visual_stereo import extract_features_stereo, extract_keyframes_stereo, stereo_match, stereo_match_batch  # noqa: F401
from .visual_pyramid import (build_pyramid, extract_features_pyramid, extract_features_stereo_pyramid, extract_keyframes_pyramid,  # noqa: F401
                             extract_keyframes_stereo_pyramid, level_budgets, level_sizes, merge_levels)
from .rectify import (RawCamera, extract_keyframes_raw, extract_keyframes_stereo_raw, keyframe_clouds_stereo_raw, rectify_depths,  # noqa: F401
                      rectify_images, rectify_maps, stereo_camera)
