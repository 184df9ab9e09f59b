"""The KLT checker (tests/klt_checker.py: the specification of svo_hip_klt_track in numpy f64) against the renderer's exact
correspondences on four scenes: frame 0 tracked into every following frame with the carried flow.  Of the tracked points
whose true position is at least 16 px inside the image, at most 2 % per frame may be farther than 1 px from the truth (a
mistrack must not hide a broken tracker) and every other one is within 0.6 px (translation-only LK under the scenes'
rotation and height change is biased by up to 0.4 px); the fourth scene reaches the bootstrap's gate -- median disparity
>= 50 px with >= 50 points tracked -- within 10 frames."""
import numpy as np
import pytest

import klt_checker
import klt_scenes


@pytest.mark.parametrize("seed,max_step,n_frames", klt_scenes.SCENES)
def test_checker_tracks_the_rendered_scenes(oracle, seed, max_step, n_frames):
    s = klt_scenes.make_scene(seed, max_step, n_frames)
    pyrs = [oracle.create_img_pyramid(im, 5) for im in s.images]
    chain = klt_scenes.checker_chain(pyrs, s.px_ref)
    gate = None
    for k, c in enumerate(chain, start=1):
        ok, text = klt_scenes.truth_violations(s.cam, s.truth[k], c["px"], c["st"])
        _, n, med = klt_checker.summarize(s.px_ref, c["px"].astype(np.float32), c["st"])
        print(f"scene {seed}/{max_step} frame {k}: tracked {n}, median disparity {med:.2f} px, {text}, "
              f"{c['iters'][c['st_in'] != 0].mean():.2f} iterations per point and level")
        assert ok, f"frame {k}: {text}"
        assert n >= 100   # the scenes keep most of their 200 corners
        if gate is None and med >= 50.0 and n >= 50:
            gate = k
    if (seed, max_step) == (12345, 0.03):
        assert gate is not None and gate <= 10, "scene 4 never reaches a median disparity of 50 px with 50 points tracked"
