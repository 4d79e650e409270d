"""Builds libloamlivox_hip.so (the C-ABI library of include/loam_livox_hip.h) in-tree with hipcc for gfx950.

hipcc cross-compiles without a GPU.  All translation units are compiled with -ffp-contract=off: label/index
sets and neighbour lists must reproduce the reference's un-contracted fp32/fp64 evaluation; the residual
accumulation (ll_reg_core.h block_accumulate) re-enables contraction locally.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
# LL_LIB_OUT: build an instrumented / A-B variant next to the product library (e.g. with LL_EXTRA_HIPCC_FLAGS=-DLL_SOLVE_TIMING)
# and load it with LOAM_LIVOX_LIB (capi.py); the default is the product library.
LIB = os.environ.get("LL_LIB_OUT") or os.path.join(HERE, "libloamlivox_hip.so")
SOURCES = ["ll_api_common.hip", "ll_api_fe.hip", "ll_api_map.hip", "ll_api_reg.hip", "ll_api_voxel.hip", "ll_api_cellmap.hip", "ll_api_scene_align.hip", "ll_api_keyframe_bank.hip", "ll_api_pose_graph.hip", "ll_api_map_refine.hip", "ll_api_history.hip", "ll_api_history_batch_buffer.hip", "ll_api_history_batch_stores.hip", "ll_api_history_batch_extract.hip", "ll_api_history_batch_cells.hip", "ll_api_history_batch_scanlog.hip", "ll_fe_kernels.hip", "ll_map_kernels.hip", "ll_reg_query_kernels.hip", "ll_reg_solve_kernels.hip", "ll_reg_maps_kernels.hip", "ll_reg_big_maps_kernels.hip", "ll_reg_aux_kernels.hip", "ll_reg_small_kernels.hip", "ll_reg_info_kernels.hip", "ll_knn_kernels.hip", "ll_voxel_kernels.hip", "ll_cellmap_kernels.hip", "ll_cellmap_extract_kernels.hip", "ll_cellmap_select_kernels.hip", "ll_spin_kernels.hip", "ll_spin_api.hip", "ll_history_batch_kernels.hip", "ll_cellmap_batch_kernels.hip", "ll_cellmap_batch_extract_kernels.hip", "ll_cellmatch_batch_kernels.hip", "ll_fullmap_batch_kernels.hip", "ll_scan_log_kernels.hip", "ll_keyframe_bank_kernels.hip", "ll_pose_graph_kernels.hip", "ll_map_refine_kernels.hip"]
HEADERS = ["ll_api_internal.h", "ll_api_history_batch_internal.h", "ll_device.h", "ll_fe_core.h", "ll_knn_core.h", "ll_knn_coop.h", "ll_knn_tile.h", "ll_reg_query.h", "ll_reg_solve_fast.h", "ll_reg_big_path.h", "ll_reg_solve_general.h", "ll_reg_solve_common.h", "ll_lm_wave.h", "ll_reg_small_solve.h", "ll_reg_core.h", "ll_reg_info_core.h", "ll_voxel.h", "ll_voxel_core.h", "ll_cellmap.h", "ll_cellmap_core.h", "ll_cellmap_select_core.h", "ll_spin.h", "ll_spin_core.h", "ll_history_batch.h", "ll_cellmap_batch.h", "ll_cellmap_batch_core.h", "ll_cellmap_batch_extract_core.h", "ll_cellmatch_batch.h", "ll_cellmatch_batch_core.h", "ll_fullmap_batch.h", "ll_fullmap_batch_core.h", "ll_scan_log.h", "ll_scan_log_core.h", "ll_keyframe_bank.h", "ll_keyframe_bank_core.h", "ll_pose_graph.h", "ll_pose_graph_core.h", "ll_map_refine.h", "ll_map_refine_core.h", "ll_ordered_float.h", "../../include/loam_livox_hip.h"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-result"]
FLAGS += os.environ.get("LL_EXTRA_HIPCC_FLAGS", "").split()  # e.g. -DLL_SOLVE_TIMING (instrumented solver, ll_reg_debug_cycles)


def hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (ROCm toolchain required to build libloamlivox_hip.so)")



def needs_build(lib: str = LIB) -> bool:
    if not os.path.exists(lib):
        return True
    t = os.path.getmtime(lib)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False, lib: str = LIB, extra_flags=()) -> str:
    if not force and not needs_build(lib):
        return lib
    cc = hipcc()
    default = os.path.join(HERE, "libloamlivox_hip.so")
    objdir = os.path.join(HERE, "build" if lib == default else "build_" + os.path.basename(lib).replace(".so", ""))
    os.makedirs(objdir, exist_ok=True)
    objs = []
    procs = []
    for src in SOURCES:
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        cmd = [cc] + FLAGS + list(extra_flags) + ["-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        objs.append(obj)
    for src, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{out.decode()}")
        if verbose and out:
            print(out.decode(), file=sys.stderr)
    cmd = [cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib] + objs
    subprocess.check_call(cmd)
    return lib


# A/B variant of the solver kernels with the Levenberg-Marquardt controller on lane 0 (-DLL_LM_LANE0, ll_reg_solve_common.h), for
# tests/test_gpu_lm_wave.py: load it with LOAM_LIVOX_LIB.  Only the units that hold a solver kernel differ from the product library.
LM_LANE0_LIB = os.path.join(HERE, "libloamlivox_hip_lm_lane0.so")
LM_LANE0_SOURCES = ["ll_reg_solve_kernels.hip", "ll_reg_maps_kernels.hip", "ll_reg_big_maps_kernels.hip", "ll_reg_small_kernels.hip"]


def build_lm_lane0(force: bool = False) -> str:
    build()
    if not force and not needs_build(LM_LANE0_LIB) and os.path.getmtime(LM_LANE0_LIB) >= os.path.getmtime(LIB):
        return LM_LANE0_LIB
    flags = ["-DLL_LM_LANE0", "-DLL_LM_COUNTS"]  # (LL_LM_COUNTS: fits and rejected last steps in dbg_cycles[14], [15])
    shared = [os.path.join(HERE, "build", s.replace(".hip", ".o")) for s in SOURCES if s not in LM_LANE0_SOURCES]
    if not all(os.path.exists(o) for o in shared):  # (the product library came without its objects)
        return build(force=True, lib=LM_LANE0_LIB, extra_flags=flags)
    cc = hipcc()
    objdir = os.path.join(HERE, "build_lm_lane0")
    os.makedirs(objdir, exist_ok=True)
    procs = []
    for src in LM_LANE0_SOURCES:
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        procs.append((src, obj, subprocess.Popen([cc] + FLAGS + flags + ["-c", os.path.join(CSRC, src), "-o", obj], stdout=subprocess.PIPE,
                                                 stderr=subprocess.STDOUT)))
    for src, _, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{out.decode()}")
    subprocess.check_call([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LM_LANE0_LIB] + shared + [o for _, o, _ in procs])
    return LM_LANE0_LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
