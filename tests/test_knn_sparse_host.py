"""CPU: the contract the late ICP iterations' sparse tile search rests on (ll_knn_core.h KnnRef, m_strong), on the host build of
the search headers: while a query has moved less than its record's order budget, an exhaustive search at the new position finds
the five neighbours of the record, in the record's order -- so the slot's neighbour record and block flag hold as they are.

Records of both kinds the registrar leaves: from the tile search (ll_knn_tile.h, host model; lanes the tile does not settle get the
budget 0 like in reg_knn_tile_kernel) and from the per-lane search (knn5_search: lists of fewer than five inside the radius have a
budget too -- while it lasts no fifth point enters the radius)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.hostcheck import hc

HERE = os.path.dirname(os.path.abspath(__file__))
CELL = 0.6
N_MAP, N_Q = 2000, 512
TIE_A, TIE_B = 10, 11  # two map points at the same place: an exact distance tie for every query


@pytest.fixture(scope="module")
def ks(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("knn_sparse") / "libknn_sparse_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", lib,
                           os.path.join(HERE, "knn_sparse_host.cpp")])
    return C.CDLL(lib)


@pytest.fixture(scope="module")
def world():
    rng = np.random.default_rng(17)
    pts = rng.uniform(0.0, 6.0, (N_MAP, 3)).astype(np.float32)
    pts[TIE_B] = pts[TIE_A]
    q = rng.uniform(0.0, 6.0, (N_Q, 3)).astype(np.float32)
    q[:64] = rng.uniform(-CELL, 6.0 + CELL, (64, 3)).astype(np.float32)  # up to one cell outside the grid (the box of the map's points)
    q[64] = pts[TIE_A]                                                   # the tied pair leads its list
    q[65:80] = pts[TIE_A] + rng.normal(0, 0.05, (15, 3)).astype(np.float32)
    order = np.lexsort(tuple(np.floor(q / CELL).astype(np.int64).T))     # x fastest, like the cell order of the kernel
    return pts, np.ascontiguousarray(q[order]), hc.Grid(pts, CELL)


def brute(pts, q, max_d2):
    """per query: original indices of the points with d2 < max_d2 in (d2, index) order, the first five; fp32, x, y, z order"""
    out = []
    for p in q:
        d = p[None, :] - pts
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2.dtype == np.float32
        o = np.lexsort((np.arange(len(pts)), d2))[:6]
        out.append([int(j) for j in o if d2[j] < max_d2][:5])
    return out


def moved(rng, q, m_strong):
    """every query displaced by 0 .. 2 x its budget in a random direction (budget 0: by up to 2 cm)"""
    u = rng.normal(size=q.shape)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    s = rng.uniform(0.0, 2.0, len(q)) * np.where(m_strong > 0, m_strong, 0.01)
    s[::7] = 0.0
    return (q.astype(np.float64) + u * s[:, None]).astype(np.float32)


def delta_of(ks, ref, q):
    out = np.zeros(len(q), np.float32)
    ks.ks_delta(len(q), ref.ctypes.data_as(C.c_void_p), np.ascontiguousarray(q).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    return out


def check(ks, pts, q, idx, m_strong, max_d2, seed):
    rng = np.random.default_rng(seed)
    stable_full = stable_short = 0
    for _ in range(3):
        q2 = moved(rng, q, m_strong)
        delta = delta_of(ks, q, q2)
        lists = brute(pts, q2, max_d2)
        for i in np.nonzero(delta < m_strong)[0]:
            want = [int(j) for j in idx[i] if j >= 0]
            if len(want) == 5:
                assert lists[i] == want, (i, delta[i], m_strong[i])
                stable_full += 1
            else:  # fewer than five inside the radius: still so (no block either way)
                assert len(lists[i]) < 5, (i, delta[i], m_strong[i])
                stable_short += 1
    return stable_full, stable_short


@pytest.mark.parametrize("max_d2", [50.0, 0.16])
def test_tile_records_hold_within_their_budget(ks, world, max_d2):
    pts, q, grid = world
    idx, d2, lb2, _, out2, settled = grid.knn5_tile(q, max_d2, bounds=True)
    count = (idx >= 0).sum(axis=1).astype(np.int32)
    m_strong = np.zeros(len(q), np.float32)
    ks.ks_m_strong(len(q), d2.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p), lb2.ctypes.data_as(C.c_void_p),
                   out2.ctypes.data_as(C.c_void_p), C.c_float(max_d2), m_strong.ctypes.data_as(C.c_void_p))
    m_strong[(settled == 0) | (count < 5)] = 0.0  # reg_knn_tile_kernel: only a lane the tile settles with five neighbours gets a budget
    # an exact tie inside the list: no budget, never stable
    tied = np.array([TIE_A in row and TIE_B in row for row in idx.tolist()])
    assert tied.sum() >= 10 and np.all(m_strong[tied] == 0.0)
    assert np.array_equal(idx, grid.knn5(q, max_d2)[0])
    full, _ = check(ks, pts, q, idx, m_strong, max_d2, 1)
    if max_d2 == 50.0:
        assert full > 300  # the budgets are worth something: a good part of the displaced queries stays inside them
        assert (m_strong > 0).mean() > 0.5


@pytest.mark.parametrize("max_d2", [50.0, 0.16])
def test_search_records_hold_within_their_budget(ks, world, max_d2):
    """0.16: a 0.4 m radius holds fewer than five of the map's ~9 points per cubic metre for most queries"""
    pts, q, grid = world
    idx, d2 = grid.knn5(q, max_d2)
    _, _, _, _, m_strong = grid.knn5_bounds(q, max_d2)
    tied = np.array([TIE_A in row and TIE_B in row and min(row) >= 0 for row in idx.tolist()])
    assert np.all(m_strong[tied] == 0.0)
    full, short = check(ks, pts, q, idx, m_strong, max_d2, 2)
    if max_d2 == 50.0:
        assert full > 300
    else:
        assert ((idx >= 0).sum(axis=1) < 5).mean() > 0.5 and short > 100
