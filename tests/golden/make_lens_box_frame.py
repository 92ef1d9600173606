"""lens_box_frame.npy: the oracle's box frame (oracle/obb.py oriented_bounds_large) of the lens (2 600 equator vertices, 8 672 points) that
tests/test_gpu_highres.py::test_a_given_up_humerus_whose_redo_overflows_the_candidates_tier runs.  Minutes on one core.
Run from the repository root: python tests/golden/make_lens_box_frame.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
from conftest import lens_surface      # noqa: E402
from oracle import obb                 # noqa: E402

v, f = lens_surface(2600, 6600, seed=2, size=4.0)
np.save(os.path.join(HERE, "lens_box_frame.npy"), obb.oriented_bounds_large(v.astype(np.float64))[0])
