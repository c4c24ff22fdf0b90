"""The plan classes of an embedding handle, without a device: tests/util_embed_plan.py restates the rules of mkws_embed_create / launch_gemm /
pick_tile in Python; this file pins what follows from them on a 256-CU device to a literal table -- the handle sizes at which the default plan
changes, and what changes there -- so that a change of a rule in the restatement shows here, and a change of the rule in the C++ shows in
tests/test_embed_handle_boundaries_gpu.py, which holds a device to the restatement on both sides of every row."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import util_embed_plan as up  # noqa: E402

GEMV, GEMM = "gemv", "gemm"
# first max_batch of the class -> {key: (value below, value from here on)}; GEMM layers as (MT, NT, split-K), GEMV as (rows, K-chunk groups)
TABLE_256 = {
    2: {"fuse_cluster_chain": (1, 0), "fuse_mid": (0, 1), "top": ((GEMV, 4, 2), (GEMM, 1, 2, 1)),
        "dense": ((GEMV, 1, 5), (GEMV, 4, 5)), "dense_1": ((GEMV, 1, 8), (GEMV, 4, 8)), "dense_2": ((GEMV, 1, 8), (GEMV, 4, 8))},
    5: {"dense": ((GEMV, 4, 5), (GEMM, 1, 2, 4)), "dense_1": ((GEMV, 4, 8), (GEMM, 1, 2, 4)), "dense_2": ((GEMV, 4, 8), (GEMM, 1, 2, 4))},
    33: {"fuse_cluster": (1, 0)},
    65: {"cluster_buffers": (1, 0)},
    128: {"fuse_walk": (0, 1)},
    129: {"block_tiles": (2, 1), "mid4a_clips": (2, 1), "dense": ((GEMM, 1, 2, 4), (GEMM, 1, 2, 2)), "dense_1": ((GEMM, 1, 2, 4), (GEMM, 1, 2, 2))},
    241: {"dense": ((GEMM, 1, 2, 2), (GEMM, 1, 2, 1)), "dense_1": ((GEMM, 1, 2, 2), (GEMM, 1, 2, 1)), "dense_2": ((GEMM, 1, 2, 4), (GEMM, 1, 2, 2))},
    257: {"block_tiles": (1, 2), "mid4a_clips": (1, 2), "stem_walks": (0, 1)},
    409: {"top": ((GEMM, 1, 2, 1), (GEMM, 2, 2, 1))},
    497: {"dense": ((GEMM, 1, 2, 1), (GEMM, 1, 4, 1)), "dense_1": ((GEMM, 1, 2, 1), (GEMM, 1, 4, 1)), "dense_2": ((GEMM, 1, 2, 2), (GEMM, 1, 2, 1))},
    513: {"pair_mt": (1, 2)},
    993: {"dense": ((GEMM, 1, 4, 1), (GEMM, 2, 4, 1)), "dense_1": ((GEMM, 1, 4, 1), (GEMM, 2, 4, 1))},
    1009: {"dense_2": ((GEMM, 1, 2, 1), (GEMM, 1, 4, 1))},
    1021: {"block_tiles": (2, 3)},
    1024: {"dense": ((GEMM, 2, 4, 1), (GEMM, 1, 4, 1)), "dense_1": ((GEMM, 2, 4, 1), (GEMM, 1, 4, 1))},
    2048: {"dense": ((GEMM, 1, 4, 1), (GEMM, 2, 4, 1)), "dense_1": ((GEMM, 1, 4, 1), (GEMM, 2, 4, 1)), "dense_2": ((GEMM, 1, 4, 1), (GEMM, 2, 4, 1))},
}
# the rows that follow the CU count, on a 304-CU device (the other rows stay where they are)
CU_ROWS_304 = {153: {"block_tiles": (2, 1), "mid4a_clips": (2, 1)}, 305: {"block_tiles": (1, 2), "mid4a_clips": (1, 2), "stem_walks": (0, 1)},
               609: {"pair_mt": (1, 2)}, 1213: {"block_tiles": (2, 3)}}


def _table(cus, upto=2048):
    return {n: {k: (up.plan(n - 1, cus)[k], up.plan(n, cus)[k]) for k in changed} for n, changed in up.boundaries(cus, upto)}


def test_boundaries_of_a_256_cu_device():
    got = _table(256)
    assert sorted(got) == sorted(TABLE_256)
    for n in TABLE_256:
        assert got[n] == TABLE_256[n], n
    # one-clip handles, the class below the first row
    p = up.plan(1, 256)
    assert (p["fuse_cluster"], p["fuse_cluster_chain"], p["cluster_buffers"], p["fuse_mid"], p["fuse_walk"], p["block_tiles"], p["pair_mt"]) == (1, 1, 1, 0, 0, 2, 1)
    assert up.boundaries(256, upto=1024) == [(n, tuple(TABLE_256[n])) for n in sorted(TABLE_256) if n <= 1024]


def test_plan_is_constant_between_boundaries():
    edges = sorted(TABLE_256)
    for lo, hi in zip([1] + edges, edges + [2049]):
        first = up.plan_class(lo, 256)
        for n in (lo + 1, (lo + hi) // 2, hi - 1):
            if lo < n < hi:
                assert up.plan_class(n, 256) == first, (lo, n)
    assert [up.plan(n, 256)["stem_grid"] for n in (1, 100, 256, 257, 2048)] == [1, 100, 256, 256, 256]


def test_another_cu_count_moves_only_the_cu_rows():
    t256, t304 = _table(256), _table(304)

    def without_cu_keys(t):
        rows = {n: {k: v for k, v in row.items() if k not in up.CU_KEYS} for n, row in t.items()}
        return {n: row for n, row in rows.items() if row}

    def only_cu_keys(t):
        rows = {n: {k: v for k, v in row.items() if k in up.CU_KEYS} for n, row in t.items()}
        return {n: row for n, row in rows.items() if row}

    assert without_cu_keys(t256) == without_cu_keys(t304)
    assert only_cu_keys(t304) == CU_ROWS_304
    assert sorted(only_cu_keys(t256)) == [129, 257, 513, 1021]
    for cus in (64, 128, 304):           # and no rule that does not name the CU count reads it
        for n in (1, 4, 5, 64, 128, 500, 1000, 2048):
            a, b = up.plan(n, cus), up.plan(n, 256)
            assert {k: v for k, v in a.items() if k not in up.CU_KEYS} == {k: v for k, v in b.items() if k not in up.CU_KEYS}, (cus, n)


def test_pick_tile_restatement_on_the_shapes_the_code_comments_name():
    # pick_tile's own comments: 1024 clips 1x4 on all three dense layers; 256 clips 1x2, dense_2 over two K slices; 512 clips 1x4 and 1x2 for dense_2
    assert [up.plan(1024, 256)[k] for k in ("dense", "dense_1", "dense_2")] == [(GEMM, 1, 4, 1)] * 3
    assert [up.plan(256, 256)[k] for k in ("dense", "dense_1", "dense_2")] == [(GEMM, 1, 2, 1), (GEMM, 1, 2, 1), (GEMM, 1, 2, 2)]
    assert [up.plan(512, 256)[k] for k in ("dense", "dense_1", "dense_2")] == [(GEMM, 1, 4, 1), (GEMM, 1, 4, 1), (GEMM, 1, 2, 1)]
    assert up.pick_tile(100, 320, 8) == (2, 1, 1)          # one column tile


def test_launch_sequences_match_the_recorded_ones(golden_dir):
    """launches() against tests/golden/embed_launch_sequences.json, which an MI355X wrote: the restatement names every launch of the
    recorded handles as the device did."""
    import json
    want = json.load(open(os.path.join(golden_dir, "embed_launch_sequences.json")))
    for key, seq in want.items():
        mb, b = (int(t.lstrip("maxbtchB_")) for t in key.split("_B"))
        assert up.launches(up.plan(mb, 256), b) == seq, key


def test_launch_sequences_differ_where_the_changed_keys_say():
    for n, changed in up.boundaries(256):
        for fuse_top in (1, 0):
            plo, phi = up.plan(n - 1, 256), up.plan(n, 256)
            diff = up.stages_that_differ(up.launches(plo, n - 1, fuse_top), up.launches(phi, n, fuse_top))
            visible = [k for k in changed if k not in up.INVISIBLE_KEYS]
            # (a split over 4 K slices and one over 2 are the same two kernel names: 129 clips, dense and dense_1)
            visible = [k for k in visible if not (isinstance(plo[k], tuple) and plo[k][0] == phi[k][0] == GEMM and plo[k][1:3] == phi[k][1:3] and min(plo[k][3], phi[k][3]) > 1)
                       ]
            if n > 32 and fuse_top:
                visible = [k for k in visible if k != "top"]          # the top conv is the paired chain's last phase there
            assert diff <= set().union(set(), *(up.STAGES_OF_KEY[k] for k in visible)), (n, diff)
            for k in visible:
                assert diff & up.STAGES_OF_KEY[k], (n, k)


def test_gpu_file_stands_on_both_sides_of_every_edge():
    pytest.importorskip("torch")
    from test_embed_handle_boundaries_gpu import EDGES_256, HANDLE_SIZES
    assert EDGES_256 == sorted(TABLE_256)
    edges = set(TABLE_256)
    for n in edges:
        assert n in HANDLE_SIZES and n - 1 in HANDLE_SIZES, n
    for m in HANDLE_SIZES:
        assert m in edges or m + 1 in edges or m in (1025, 256), m          # 1025: the class of 1024 past one round of pairs; 256 = 257 - 1 (plan_batch)
    # classes never compared with the oracle before: each has a handle of its own here
    for lo, hi in ((993, 1008), (1009, 1020), (1025, 2047), (2048, 2048), (33, 64)):
        assert any(lo <= m <= hi for m in HANDLE_SIZES), (lo, hi)
