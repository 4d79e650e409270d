"""GPU tier of the lifetime rule of loam_livox_amd/api.py (tests/test_api_handles_host.py is the CPU tier): every class that owns a device
handle is created at small capacities on the device and closed twice; a Cell_map borrowed from a History_buffer closes without taking
the history's map along; a Pose_graph that is too small for its graph creates itself again, larger, and solves as one that was large
enough from the start.  No method is called on a closed handle here: those refusals are the CPU tier's."""
import numpy as np
import pytest

from loam_livox_amd import api

pytestmark = pytest.mark.gpu

# one scan, one cloud, one frame, one entry, one graph; a few dozen points
OWNERS = [
    (api.Livox_laser, dict(max_points=32, max_scans=1)),
    (api.Spinning_laser, dict(max_points=32, max_scans=1, max_line_points=32)),
    (api.VoxelGrid, dict(max_points=32, max_clouds=1)),
    (api.History_buffer, dict(maximum_history_size=1, max_points_per_frame=32)),
    (api.History_buffer_batch, dict(n_sequences=1, maximum_history_size=1, max_points_per_frame=32)),
    (api.Cell_map, dict(max_points=32)),
    (api.Scene_aligner, dict(initial_points=32)),
    (api.Keyframe_bank, dict(initial_entries=1)),
    (api.Map_refine, dict(initial_points=32)),
    (api.Pose_graph, dict(max_graphs=1, max_poses=2, max_edges=1, max_envelope_blocks=1)),
    (api.Map_buffer, dict()),
    (api.Point_cloud_registration, dict(max_scans=1, max_features=32)),
]


@pytest.mark.parametrize("cls, args", OWNERS, ids=[o[0].__name__ for o in OWNERS])
def test_create_and_close_twice(gpu_lib, cls, args):
    obj = cls(**args)
    assert obj.L is gpu_lib and obj.h
    obj.close()
    assert obj.h is None
    obj.close()
    assert obj.h is None


def test_a_borrowed_cell_map_leaves_the_history_its_map(gpu_lib):
    history = api.History_buffer(maximum_history_size=2, max_points_per_frame=32)
    history.enable_cell_map(max_points=64, cell_resolution=1.0)
    cm = history.cell_map(0)
    assert not cm.owned and cm.stats() == (0, 0, 0)
    cm.close()
    cm.close()
    assert cm.h is None
    assert len(history) == 0
    assert history.cell_map(0).stats() == (0, 0, 0)   # the history's map is still there
    history.close()
    assert history.h is None


def test_pose_graph_creates_itself_again_and_solves():
    rng = np.random.default_rng(3)
    truth = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (3, 1))
    truth[1:, 4:] = [[1.0, 0.2, 0.0], [2.0, 0.1, 0.3]]
    start = truth.copy()
    start[1:, 4:] += rng.uniform(-0.05, 0.05, (2, 3))
    graph = dict(poses=start, ab=[[0, 1], [1, 2]], meas=[api.relative_constraint(truth[i], truth[i + 1]) for i in range(2)])
    small, large = api.Pose_graph(1, 2, 1, 1), api.Pose_graph(1, 8, 8, 8)
    poses, summaries = small.solve([graph])            # 3 poses, 2 edges, 3 envelope blocks: it grows once
    assert small.capacity == [1, 6, 4, 6] and small.h and small.h.value is not None
    want, want_summaries = large.solve([graph])
    assert large.capacity == [1, 8, 8, 8]
    assert len(poses) == 1 and poses[0].shape == (3, 7) and np.isfinite(poses[0]).all()
    assert np.array_equal(poses[0], want[0]) and summaries == want_summaries
    # the measurements are those of `truth`, so the optimum is `truth` with no residual: the 0.05 m of the start must be gone, to a
    # bound far below the perturbation and far above where a fp64 Levenberg-Marquardt run on a zero-residual problem stops
    assert np.array_equal(poses[0][0], start[0]) and np.abs(poses[0] - truth).max() < 1e-4
    assert summaries[0]["final_cost"] <= summaries[0]["initial_cost"]
    assert np.array_equal(graph["poses"], start)       # the inputs are not modified
    again, _ = small.solve([graph])                    # it fits now: the same handle answers
    assert small.capacity == [1, 6, 4, 6] and np.array_equal(again[0], poses[0])
    for pg in (small, large):
        pg.close()
        pg.close()
        assert pg.h is None
