"""The shapes of tests/test_gpu_seams.py (tests/seam_shapes.py) held against the constants in the sources: each shape crosses the seam
it is meant for.  Someone who changes a chunk size, a budget or the launch cap sees this fail, instead of the GPU tests quietly
running inside one chunk again."""
import pytest

import seam_shapes as S


def test_every_constant_is_found(monkeypatch):
    for name in ("kPredictChunk", "kPathChunk", "kPsiBudget", "kHyperChunk", "kZPartBudget", "kMaxBlocks", "BS", "KT", "kBlock"):
        assert S.constant(name) > 0, name
    monkeypatch.setitem(S.WHERE, "kNoSuchConstant", "agpl_features.hip")
    with pytest.raises(LookupError):  # a constant that was renamed or removed is an error, not a silent default
        S.constant("kNoSuchConstant")


def _straddles(idx, seam, Ns):
    return {0, seam - 1, seam, seam + 1, Ns - 1} <= set(idx) and max(idx) < Ns and len(set(idx)) == len(idx)


def test_the_chunk_constants_are_what_the_index_lists_straddle():
    for name in ("kPredictChunk", "kPathChunk", "kHyperChunk"):
        assert S.constant(name) == S.CHUNK, name
    assert S.constant("BS") == 128


def test_predict_shapes_cross_the_chunk():
    chunk = S.constant("kPredictChunk")
    assert S.PREDICT_NS > chunk and len(S.chunks(S.PREDICT_NS, chunk)) == 2
    assert (S.PREDICT_NS - chunk) % S.constant("BS") not in (0, S.PREDICT_NS - chunk)  # the second chunk: a full tile and a ragged one
    assert 0 < S.PREDICT_WINDOW < chunk < S.PREDICT_NS and S.PREDICT_WINDOW % S.constant("BS")
    assert S.PREDICT_NS - S.PREDICT_WINDOW <= chunk and S.PREDICT_HEAD <= chunk  # the calls compared with run in one chunk
    assert len(S.PREDICT_GATHER) <= chunk and _straddles(S.PREDICT_GATHER, chunk, S.PREDICT_NS)
    assert 1 in S.PREDICT_LS and max(S.PREDICT_LS) > 1  # both the direct route and the staged one


def test_paths_shapes_cross_the_chunk_and_the_sub_chunk_inside_the_second_chunk():
    chunk = S.constant("kPathChunk")
    F, Ns, idx = S.PATHS_SMALL
    assert Ns > chunk and S.path_sub(F, Ns) >= chunk  # one sub-chunk per chunk: the pure chunk seam
    assert [(c0, q0) for c0, q0, _ in S.path_launches(F, Ns)] == [(0, 0), (chunk, 0)]
    assert _straddles(idx, chunk, Ns)
    F, Ns, idx = S.PATHS_LARGE
    sub = S.path_sub(F, Ns)
    assert Ns > chunk and sub < Ns - chunk and chunk % sub == 0 and chunk // sub > 1
    steps = S.path_launches(F, Ns)
    assert [s for s in steps if s[0] == chunk] == [(chunk, 0, sub), (chunk, sub, Ns - chunk - sub)]  # t0 > 0 inside c0 > 0
    assert len([s for s in steps if s[0] == 0]) == chunk // sub
    assert _straddles(idx, chunk, Ns) and {chunk + sub - 1, chunk + sub, chunk + sub + 1, sub - 1, sub} <= set(idx)
    assert 0 < S.PATHS_WINDOW < chunk and S.PATHS_WINDOW % S.constant("BS") and Ns - S.PATHS_WINDOW <= chunk
    assert 0 < S.PATHS_ZERO_NS < chunk


def test_zgrad_shape_crosses_the_tile_group_and_the_chunk():
    groups = S.zgrad_groups(S.ZGRAD_N, S.ZGRAD_M, S.ZGRAD_D)
    assert groups == S.ZGRAD_GROUPS  # chunk one in two launches, chunk two in one
    assert len(groups[0]) > 1 and len(groups) > 1
    BS = S.constant("BS")
    assert S.ZGRAD_CUT == groups[0][0] * BS  # the first shard is exactly the first group
    assert S.zgrad_groups(S.ZGRAD_CUT, S.ZGRAD_M, S.ZGRAD_D) == [[groups[0][0]]]  # ... and runs as ONE launch
    assert [len(g) for g in S.zgrad_groups(S.ZGRAD_N - S.ZGRAD_CUT, S.ZGRAD_M, S.ZGRAD_D)] == [1]
    assert (S.ZGRAD_N - S.constant("kHyperChunk")) % BS == 44  # the last tile is ragged
    # the largest shapes of tests/test_gpu_zgrad.py never launch twice in a chunk
    assert all(len(g) == 1 for g in S.zgrad_groups(1000, 300, 16) + S.zgrad_groups(65536 + 300, 40, 3))


def test_hyper_shape_crosses_the_chunk():
    chunk = S.constant("kHyperChunk")
    assert S.HYPER_N > chunk and len(S.chunks(S.HYPER_N, chunk)) == 2
    assert S.HYPER_CUT == chunk and S.HYPER_N - S.HYPER_CUT < chunk  # the second shard starts at c0 = 0 with another pitch


def test_predictive_shapes_stride():
    cap, lanes = S.constant("kMaxBlocks"), S.constant("kBlock")
    assert S.PRED_SCALAR_N > cap * lanes  # a scalar likelihood: one point per lane
    assert S.PRED_CAT_N > cap * (lanes // 64)  # categorical: one point per wave
    assert S.cdiv(S.PRED_SCALAR_N, lanes) > cap and S.cdiv(S.PRED_CAT_N, lanes // 64) > cap  # nblk is the cap itself
    for n, slices, per in ((S.PRED_SCALAR_N, S.PRED_SCALAR_SLICES, lanes), (S.PRED_CAT_N, S.PRED_CAT_SLICES, lanes // 64)):
        assert all(0 <= a < b <= n and b - a <= 1000 for a, b in slices)  # short calls: no stride
        assert slices[0][0] == 0 and slices[-1][1] == n
        assert any(a < cap * per < b for a, b in slices)  # one slice across the first strided point
