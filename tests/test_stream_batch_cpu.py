"""The batch form of the streaming analysis (embedding/batch_streaming_analysis.py: eval_stream_tests, batch_streaming_analysis) and
the segmented detector's host side, as far as they go without an embedding: the C-ABI additions, the offset checks, eval_stream_tests on
stored inferences against eval_stream_test target by target, and the directory walk.  Comparisons are exact (==): both sides make the
same IEEE operations on the same numbers.  On a host with a GPU the stored inferences take the device detector; without one, the host
detect() loop: the expected values are the same."""
import ctypes
import os
import pickle
import re

import numpy as np
import pytest

from multilingual_kws_amd import _lib, synth
from multilingual_kws_amd.detector import check_segments
from multilingual_kws_amd.embedding import batch_streaming_analysis as sa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mkws_head_group_forward_segments", "mkws_detect_segments", "mkws_detect_score_segments")


def test_new_symbols_are_declared_exported_and_bound_and_the_abi_is_still_5():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mkws.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mkws_[a-z0-9_]+)\s*\(", src))
    L = ctypes.CDLL(_lib.LIB_PATH)
    bound = {n: args for n, _, args in _lib.SYMBOLS}
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(L, name) and name in bound, name
    assert len(bound["mkws_head_group_forward_segments"]) == 10
    assert len(bound["mkws_detect_segments"]) == 20 and len(bound["mkws_detect_score_segments"]) == 13
    assert _lib.lib().mkws_abi_version() == _lib.ABI_VERSION == 5
    assert "#define MKWS_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "mkws.h")).read()


def test_offset_checks_refuse_bad_lists_before_any_device_is_touched():
    times = [0, 20, 40, 0, 20, 7, 7, 9]
    off, t = check_segments([0, 3, 3, 5, 8], times)                      # a step backwards ACROSS a boundary is two recordings
    assert off.dtype == np.int32 and off.tolist() == [0, 3, 3, 5, 8] and t.dtype == np.int64 and t.tolist() == times
    off, t = check_segments([0], [])
    assert off.tolist() == [0] and t.shape == (0,)
    with pytest.raises(ValueError, match="non-decreasing"):
        check_segments([0, 5, 3, 8], times)
    with pytest.raises(ValueError, match="cover exactly"):
        check_segments([0, 3, 7], times)                                 # mismatched lengths
    with pytest.raises(ValueError, match="cover exactly"):
        check_segments([1, 3, 8], times)
    with pytest.raises(ValueError, match="increasing time order"):
        check_segments([0, 4, 8], times)                                 # 40 -> 0 inside segment 0
    with pytest.raises(ValueError):
        check_segments([], times)
    with pytest.raises(ValueError):
        check_segments([[0, 8]], times)
    # the wrappers run the same checks first: no probabilities are looked at, nothing is uploaded
    from multilingual_kws_amd.detector import detect_segments_on_device, score_segments_on_device
    with pytest.raises(ValueError, match="increasing time order"):
        detect_segments_on_device(None, [0, 4, 8], times, [0.5], 100, 500, 4)
    with pytest.raises(ValueError, match="non-decreasing"):
        score_segments_on_device(None, [0, 5, 3, 8], times, [0.5], [[], [], []], 750, 100, 500, 4)
    with pytest.raises(ValueError, match="ground-truth lists"):
        score_segments_on_device(None, [0, 3, 5, 8], times, [0.5], [[1.0]], 750, 100, 500, 4)


def _bursty(n, seed, centres, width=8):
    rng = np.random.default_rng(seed)
    tgt = np.full(n, 0.02)
    for c in centres:
        tgt[max(0, c - width):c + width] = 0.97
    other = rng.uniform(0, 1, n) * (1 - tgt)
    return np.stack([1 - tgt - other, other, tgt], axis=1).astype(np.float32)


def _write_wav(path, seconds):
    n = int(seconds * 16000)
    pcm = np.concatenate([synth.clips_int16(1, first_clip=i)[0] for i in range(int(np.ceil(seconds)))])[:n]
    with open(path, "wb") as fh:
        fh.write(synth.wav_bytes(pcm))
    return len(sa.window_offsets(n, 16000, 320))


def _targets(src, dest):
    """Four targets on the recordings under `src`, results under `dest`: an empty recording, one whose result pickle exists, one with
    two StreamFlags of different detector settings, one ordinary."""
    def flags(name, kw, **over):
        return sa.StreamFlags(wav=str(src / f"{name}.wav"), ground_truth=str(src / f"{name}.txt"), target_keyword=kw, **over)
    thr = [0.3, 0.6, 0.9]
    return [
        sa.StreamTarget("xx", "empty", "no-model", [flags("empty", "empty", detection_thresholds=thr)], dest / "empty.pkl", dest / "empty.npy"),
        sa.StreamTarget("xx", "done", "no-model", [flags("done", "done", detection_thresholds=thr)], dest / "done.pkl", dest / "done.npy"),
        sa.StreamTarget("yy", "two", "no-model", [flags("two", "two", detection_thresholds=thr),
                                                  flags("two", "two", detection_thresholds=[0.5], average_window_duration_ms=60,
                                                        suppression_ms=200, minimum_count=2)], dest / "two.pkl", dest / "two.npy"),
        sa.StreamTarget("yy", "plain", "no-model", [flags("plain", "plain", detection_thresholds=thr)], dest / "plain.pkl", dest / "plain.npy"),
    ]


def test_eval_stream_tests_on_stored_inferences_equals_eval_stream_test_per_target(tmp_path, capsys):
    src = tmp_path / "src"
    src.mkdir()
    windows = {name: _write_wav(src / f"{name}.wav", sec) for name, sec in (("empty", 0.9), ("done", 1.5), ("two", 5.0), ("plain", 3.2))}
    assert windows == dict(empty=0, done=25, two=200, plain=110)
    centres = dict(empty=[], done=[10], two=[30, 90, 150], plain=[20, 70])
    dests = []
    for side in ("one_by_one", "batch"):
        dest = tmp_path / side
        dest.mkdir()
        for seed, (name, n) in enumerate(windows.items()):
            np.save(dest / f"{name}.npy", _bursty(n, seed, centres[name]))
        with open(dest / "done.pkl", "wb") as fh:
            pickle.dump({"done": "earlier results"}, fh)
        dests.append(dest)
    model = object()                                                     # stored inferences: no model is ever asked for anything
    want = [sa.eval_stream_test(t, live_model=model) for t in _targets(src, dests[0])]
    got = sa.eval_stream_tests(_targets(src, dests[1]), live_models=[model] * 4)
    said = capsys.readouterr().out
    assert said.count("results already present") == 2 and said.count("inferences already present") == 6
    assert want[1] is None and got[1] is None
    assert got == want
    assert want[0] == {"empty": [(_targets(src, dests[0])[0].stream_flags[0], {0.3: ([], []), 0.6: ([], []), 0.9: ([], [])})]}
    (f0, by0), (f1, by1) = got[2]["two"]
    assert list(by0) == [0.3, 0.6, 0.9] and list(by1) == [0.5] and f1.suppression_ms == 200
    assert len(by0[0.6][0]) == 3 and len(by1[0.5][0]) >= 3 and by1[0.5] != by0[0.6]                # the two settings are two detector runs
    assert all(type(t) is int and type(s) is float and kw == "two" for kw, t, s in by0[0.6][1])
    # the same files, with the same contents
    assert sorted(os.listdir(dests[0])) == sorted(os.listdir(dests[1])) == sorted(
        [f"{n}.npy" for n in windows] + [f"{n}.pkl" for n in windows])
    for name in windows:
        with open(dests[0] / f"{name}.pkl", "rb") as a, open(dests[1] / f"{name}.pkl", "rb") as b:
            assert pickle.load(a) == pickle.load(b), name
        assert np.array_equal(np.load(dests[0] / f"{name}.npy"), np.load(dests[1] / f"{name}.npy"))
    with open(dests[1] / "done.pkl", "rb") as fh:
        assert pickle.load(fh) == {"done": "earlier results"}             # left alone
    with pytest.raises(ValueError, match="live models"):
        sa.eval_stream_tests(_targets(src, dests[1]), live_models=[model])


def test_eval_stream_tests_refuses_fewer_stored_rows_than_windows_as_detect_does(tmp_path):
    src, dest = tmp_path / "src", tmp_path / "dest"
    src.mkdir()
    dest.mkdir()
    assert _write_wav(src / "plain.wav", 3.2) == 110
    np.save(dest / "plain.npy", _bursty(100, 1, [20]))
    target = _targets(src, dest)[3]
    with pytest.raises(IndexError):
        sa.eval_stream_test(target, live_model=object())
    with pytest.raises(IndexError):
        sa.eval_stream_tests([target], live_models=[object()])
    # more rows than windows (chunk_audio as shipped yields them) are cut to the windows by both
    np.save(dest / "plain.npy", _bursty(130, 1, [20, 70, 120]))
    got = sa.eval_stream_tests([target], live_models=[object()])
    os.remove(target.destination_result_pkl)                              # (or the second route would find the first one's results)
    assert got == [sa.eval_stream_test(target, live_model=object())] and len(got[0]["plain"][0][1][0.6][0]) == 2


def _tree(root, words):
    for lang, word in words:
        d = root / f"sentences_{lang}" / f"stream_{word}"
        (d / "model" / "the_model").mkdir(parents=True)
        (d / "streaming_test.wav").write_bytes(b"")
        (d / "streaming_labels.txt").write_text("")
    (root / "generate.sh").write_text("# not a language directory")
    return root


def test_batch_streaming_analysis_walks_the_tree_and_refuses_malformed_ones(tmp_path, monkeypatch, capsys):
    seen = []
    monkeypatch.setattr(sa, "eval_stream_tests", lambda targets: seen.append(list(targets)) or [f"result {t.target_word}" for t in targets])
    words = [("de", "haus"), ("de", "zeit"), ("rw", "amakuru")]
    sse, dest = _tree(tmp_path / "sse", words), tmp_path / "results"
    targets, results = sa.batch_streaming_analysis(sse, dest, shuffle=False, suppression_ms=300)
    assert seen == [targets] and results == [f"result {t.target_word}" for t in targets]
    assert sorted((t.target_lang, t.target_word) for t in targets) == sorted(words)
    for t in targets:
        d = sse / f"sentences_{t.target_lang}" / f"stream_{t.target_word}"
        out = dest / f"sentences_{t.target_lang}" / f"stream_{t.target_word}"
        assert t.model_path == d / "model" / "the_model"
        assert t.destination_result_pkl == out / "stream_results.pkl" and t.destination_result_inferences == out / "raw_inferences.npy"
        assert os.path.isdir(out)                                        # every result directory is made
        (flags,) = t.stream_flags
        assert flags.wav == str(d / "streaming_test.wav") and flags.ground_truth == str(d / "streaming_labels.txt")
        assert flags.target_keyword == t.target_word and flags.suppression_ms == 300
        assert flags.detection_thresholds == np.linspace(0.05, 1, 20).tolist()
    targets, _ = sa.batch_streaming_analysis(sse, tmp_path / "other", detection_thresholds=[0.5, 0.7])
    assert sorted(t.target_word for t in targets) == ["amakuru", "haus", "zeit"] and targets[0].stream_flags[0].detection_thresholds == [0.5, 0.7]
    # the reference's three refusals
    (dest / "sentences_de" / "stream_haus" / "raw_inferences.npy").write_bytes(b"")
    with pytest.raises(AssertionError, match="result data already present"):
        sa.batch_streaming_analysis(sse, dest)
    extra = _tree(tmp_path / "extra", words)
    (extra / "sentences_de" / "stream_zeit" / "model" / "another_model").mkdir()
    with pytest.raises(ValueError, match="extra models or no models"):
        sa.batch_streaming_analysis(extra, tmp_path / "r2")
    none = _tree(tmp_path / "none", words)
    (none / "sentences_rw" / "stream_amakuru" / "model" / "the_model").rmdir()
    with pytest.raises(ValueError, match="extra models or no models"):
        sa.batch_streaming_analysis(none, tmp_path / "r3")
    missing = _tree(tmp_path / "missing", words)
    (missing / "sentences_de" / "stream_haus" / "streaming_labels.txt").unlink()
    with pytest.raises(AssertionError, match="missing stream info"):
        sa.batch_streaming_analysis(missing, tmp_path / "r4")
    capsys.readouterr()
