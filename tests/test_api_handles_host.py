"""CPU tier of the lifetime rule of loam_livox_amd/api.py, over the recording stand-in (tests/api_standin.py): a class that owns a
device handle destroys it exactly once however often it is closed or collected, never when its constructor raised, and leaves h = None;
a borrowed Cell_map never destroys; Pose_graph grows by destroying and creating again; the test taps return int64 of their documented
lengths; History_buffer.map_cloud passes a negative count on as the library's error."""
import gc

import numpy as np
import pytest

from loam_livox_amd import api, capi
from tests.api_standin import Recording_library

# class, arguments, create and destroy entry points: the twelve classes that own a handle
OWNERS = [
    (api.Livox_laser, dict(max_points=16), "ll_fe_create", "ll_fe_destroy"),
    (api.Spinning_laser, dict(max_points=16), "ll_spin_create", "ll_spin_destroy"),
    (api.VoxelGrid, dict(max_points=16), "ll_voxel_create", "ll_voxel_destroy"),
    (api.History_buffer, dict(maximum_history_size=2, max_points_per_frame=16), "ll_history_create", "ll_history_destroy"),
    (api.History_buffer_batch, dict(n_sequences=2, maximum_history_size=2, max_points_per_frame=16), "ll_history_batch_create", "ll_history_batch_destroy"),
    (api.Cell_map, dict(max_points=16), "ll_cellmap_create", "ll_cellmap_destroy"),
    (api.Scene_aligner, dict(initial_points=16), "ll_scene_align_create", "ll_scene_align_destroy"),
    (api.Keyframe_bank, dict(initial_entries=1), "ll_keyframe_bank_create", "ll_keyframe_bank_destroy"),
    (api.Map_refine, dict(initial_points=64), "ll_map_refine_create", "ll_map_refine_destroy"),
    (api.Pose_graph, dict(max_graphs=1, max_poses=2, max_edges=1, max_envelope_blocks=1), "ll_pose_graph_create", "ll_pose_graph_destroy"),
    (api.Map_buffer, dict(), "ll_map_create", "ll_map_destroy"),
    (api.Point_cloud_registration, dict(max_features=16), "ll_reg_create", "ll_reg_destroy"),
]
IDS = [o[0].__name__ for o in OWNERS]


@pytest.fixture
def lib(monkeypatch):
    lib = Recording_library()
    monkeypatch.setattr(capi, "_lib", lib)
    return lib


def destroys(lib):
    return [c for c in lib.calls if c[0].endswith("_destroy")]


@pytest.mark.parametrize("cls, args, create, destroy", OWNERS, ids=IDS)
def test_one_destroy_per_created_handle(lib, cls, args, create, destroy):
    obj = cls(**args)
    assert obj.L is lib and len(lib.of(create)) == 1
    h = obj.h.value
    assert h and not destroys(lib)
    obj.close()
    assert obj.h is None and destroys(lib) == [[destroy, [{"pointer": h}]]]
    obj.close()
    assert obj.h is None
    del obj
    gc.collect()
    assert destroys(lib) == [[destroy, [{"pointer": h}]]]


@pytest.mark.parametrize("cls, args, create, destroy", OWNERS, ids=IDS)
def test_collection_alone_destroys_once(lib, cls, args, create, destroy):
    obj = cls(**args)
    h = obj.h.value
    del obj
    gc.collect()
    assert destroys(lib) == [[destroy, [{"pointer": h}]]]


@pytest.mark.parametrize("cls, args, create, destroy", OWNERS, ids=IDS)
def test_a_constructor_that_raised_never_destroys(lib, cls, args, create, destroy):
    lib.fail.add(create)
    with pytest.raises(capi.LoamLivoxError, match=create):
        cls(**args)
    gc.collect()
    assert len(lib.of(create)) == 1 and not destroys(lib)
    # before the create call: the object has no h at all, and close() and collection are harmless
    blank = cls.__new__(cls)
    blank.L = lib
    blank.close()
    del blank
    gc.collect()
    assert not destroys(lib)


def test_a_constructor_that_raised_before_create_never_destroys(lib):
    with pytest.raises(AttributeError):
        api.Livox_laser(no_such_tunable=1)
    gc.collect()
    assert not lib.of("ll_fe_create") and not destroys(lib)


@pytest.mark.parametrize("cls, args, create, destroy", OWNERS, ids=IDS)
def test_del_swallows_what_destroy_raises(lib, cls, args, create, destroy):
    obj = cls(**args)

    def broken(h):
        raise RuntimeError("destroy failed")
    setattr(lib, destroy, broken)
    obj.__del__()
    with pytest.raises(RuntimeError):
        obj.close()


def test_a_borrowed_cell_map_never_destroys(lib):
    history = api.History_buffer(2, 16)
    history.enable_cell_map(64, 0.5)
    lib.answer("ll_history_cell_map", ret=0x7000)
    cm = history.cell_map(0)
    assert isinstance(cm, api.Cell_map) and not cm.owned and cm.h.value == 0x7000 and cm.resolution == 0.5
    assert not lib.of("ll_cellmap_create")
    cm.close()
    assert cm.h is None
    cm.close()
    again = history.cell_map(0)
    del cm, again
    gc.collect()
    assert not destroys(lib)
    h = history.h.value
    history.close()
    assert destroys(lib) == [["ll_history_destroy", [{"pointer": h}]]]


def test_pose_graph_grows_by_destroy_then_create(lib):
    pg = api.Pose_graph(1, 2, 1, 1)
    first = pg.h.value
    assert lib.of("ll_pose_graph_create") == [[0, 1, 2, 1, 1, {"byref": "c_void_p", "value": None}]] and pg.capacity == [1, 2, 1, 1]
    chain = dict(poses=np.tile([0, 0, 0, 1, 0, 0, 0.0], (3, 1)), ab=[[0, 1], [1, 2]], meas=np.tile([0, 0, 0, 1, 0, 0, 0.0], (2, 1)))
    poses, summaries = pg.solve([chain])   # 3 poses, 2 edges, 3 envelope blocks: every capacity but the graphs' is short
    assert len(poses) == 1 and poses[0].shape == (3, 7) and len(summaries) == 1
    assert lib.names()[-3:] == ["ll_pose_graph_destroy", "ll_pose_graph_create", "ll_pose_graph_solve"]
    assert lib.of("ll_pose_graph_destroy") == [[{"pointer": first}]]
    assert lib.of("ll_pose_graph_create")[1][:5] == [0, 1, 6, 4, 6] and pg.capacity == [1, 6, 4, 6]
    second = pg.h.value
    assert second != first and lib.of("ll_pose_graph_solve")[0][0] == {"pointer": second}
    pg.solve([chain])                       # it fits now
    assert len(lib.of("ll_pose_graph_create")) == 2
    pg.close()
    pg.close()
    assert pg.h is None and lib.of("ll_pose_graph_destroy") == [[{"pointer": first}], [{"pointer": second}]]


def test_pose_graph_that_cannot_grow_holds_no_handle(lib):
    pg = api.Pose_graph(1, 2, 1, 1)
    lib.fail.add("ll_pose_graph_create")
    chain = dict(poses=np.tile([0, 0, 0, 1, 0, 0, 0.0], (3, 1)), ab=[[0, 1], [1, 2]], meas=np.tile([0, 0, 0, 1, 0, 0, 0.0], (2, 1)))
    with pytest.raises(capi.LoamLivoxError):
        pg.solve([chain])
    assert pg.h is None and len(destroys(lib)) == 1 and not lib.of("ll_pose_graph_solve")
    pg.close()
    assert len(destroys(lib)) == 1


def test_every_tap_is_int64_of_its_documented_length(lib):
    batch = api.History_buffer_batch(2)
    taps = [(batch.cell_map_work, 4), (batch.extract_work, 4), (batch.full_map_work, 4), (batch.scan_log_work, 4), (batch.cell_match_work, 8),
            (api.Scene_aligner(16).work, 4), (api.Keyframe_bank(1).work, 4), (api.Map_refine(64).work, 4), (api.Pose_graph(1, 2, 1, 1).work, 4),
            (api.Point_cloud_registration(max_features=16).debug_cycles, 16)]
    for tap, n in taps:
        before = len(lib.calls)
        out = tap()
        assert isinstance(out, np.ndarray) and out.dtype == np.int64 and out.shape == (n,), tap
        name, args = lib.calls[before]
        assert len(lib.calls) == before + 1 and (args[-1]["dtype"], args[-1]["shape"]) == ("int64", [n]) and not out.any(), name
        lib.fail.add(name)
        with pytest.raises(capi.LoamLivoxError, match=name):
            tap()
    reg = api.Point_cloud_registration(max_features=16)
    assert reg.debug_worklists() == (0, 0) and reg.debug_worklists_by_kind(2) == ((0, 0), (0, 0))
    assert [a[-1]["shape"] for a in lib.of("ll_reg_debug_worklists")] == [[4], [4]]


def test_history_map_cloud_raises_on_a_negative_count(lib):
    """the one case that differs from a3c4a91, where the answer was an empty cloud"""
    history = api.History_buffer(2, 16)
    assert history.map_cloud(0).shape == (0, 4)
    lib.answer("ll_history_map_cloud", ret=3)
    assert history.map_cloud(1).shape == (3, 4) and history.map_cloud(1).dtype == np.float32
    lib.answer("ll_history_map_cloud", ret=-1)
    with pytest.raises(capi.LoamLivoxError, match="ll_history_map_cloud"):
        history.map_cloud(0)
    batch = api.History_buffer_batch(2)
    lib.answer("ll_history_batch_map_cloud", ret=-1)
    with pytest.raises(capi.LoamLivoxError, match="ll_history_batch_map_cloud"):
        batch.map_cloud(1, 0)
