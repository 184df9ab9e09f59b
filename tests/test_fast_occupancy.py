"""FastDetector.occupancy_from_features -- the mirror of AbstractDetector::setExistingFeatures -- on CPU tensors against a plain
loop over the features (tests/fast_cases.py): NaN rows behind a valid feature of cell 0, several features in one cell, pixels
on cell borders and outside the grid.  (tests/test_fast_edges_gpu.py runs the same on the device.)"""
import numpy as np
import torch

import fast_cases as fc


def test_occupancy_from_features_is_the_loop_on_cpu_tensors(hip_lib):
    from rpg_svo_amd.feature_detection import FastDetector
    w, h, cell = fc.OCC_GRID
    px = fc.occupancy_features()
    want = fc.occupancy_loop(px, w, h, cell)
    assert want[0, 0] == 1 and list(np.flatnonzero(want[0])) == [0, 1, 6, 8, 11] and list(np.flatnonzero(want[1])) == [11]
    det = FastDetector(w, h, cell, 2)
    for dt in (torch.float64, torch.float32):
        got = det.occupancy_from_features(torch.from_numpy(px).to(dt))
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want), dt
    # any order of the rows gives the same cells, and no feature at all gives none
    perm = np.random.default_rng(1).permutation(px.shape[1])
    assert np.array_equal(det.occupancy_from_features(torch.from_numpy(px[:, perm])).numpy(), want)
    assert not det.occupancy_from_features(torch.zeros(2, 0, 2, dtype=torch.float64)).any()


def test_nan_rows_do_not_clear_the_cell_of_an_earlier_feature(hip_lib):
    """(a scatter that writes a 0 into cell 0 for every NaN row leaves cell 0 unset after the feature that set it)"""
    from rpg_svo_amd.feature_detection import FastDetector
    w, h, cell = fc.OCC_GRID
    nan = float("nan")
    px = torch.tensor([[[5.0, 5.0], [nan, nan], [65.0, 40.0], [65.0, 41.0]]], dtype=torch.float64)
    got = FastDetector(w, h, cell, 2).occupancy_from_features(px).numpy()
    assert list(np.flatnonzero(got[0])) == [0, 6] and np.array_equal(got, fc.occupancy_loop(px.numpy(), w, h, cell))
