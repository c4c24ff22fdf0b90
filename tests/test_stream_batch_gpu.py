"""eval_stream_tests / stream_operating_curves end to end on the device: three (keyword, recording) targets on one shared synthetic
embedding whose batches of 64 windows straddle the recordings, against eval_stream_test / operating_curves target by target.  The eager
embedding of one handle is bit-identical across batch sizes (tests/test_streaming.py) and a row's head output depends on nothing but the
row and its head (tests/test_head_segments_gpu.py), so the saved inferences are compared with np.array_equal and the results with ==."""
import csv
import os

import numpy as np
import pytest

SECONDS = [1.3, 2.0, 0.9]                    # 15 + 50 + 0 windows: the first batch of 64 ends inside the second recording
WORDS = ["alpha", "beta", "gamma"]
THRESHOLDS = [0.3, 0.6]


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    pytest.importorskip("torch")
    from multilingual_kws_amd import synth
    from multilingual_kws_amd.embedding import batch_streaming_analysis as sa, transfer_learning as tl
    from multilingual_kws_amd.head import Head
    from oracle import head_oracle as ho
    root = tmp_path_factory.mktemp("stream_batch")
    emb, blob = tl.load_base_model("synthetic", max_batch=64)
    models, wavs, labels, samples = [], [], [], []
    for k, (sec, word) in enumerate(zip(SECONDS, WORDS)):
        n = int(sec * 16000)
        pcm = np.concatenate([synth.clips_int16(1, first_clip=10 * k + i)[0] for i in range(int(np.ceil(sec)))])[:n]
        wavs.append(str(root / f"{word}.wav"))
        with open(wavs[-1], "wb") as fh:
            fh.write(synth.wav_bytes(pcm))
        labels.append(str(root / f"{word}.txt"))
        with open(labels[-1], "w") as fh:                                # rows keyword,time_ms: this keyword's, and another's
            csv.writer(fh).writerows([[word, 120 + 200 * k], ["other", 100], [word, 700]])
        p = ho.glorot_uniform_params(seed=3000 + k)
        p[-1] += 1.0 + 0.5 * k                                           # biased towards the target class, so that keywords fire
        models.append(tl.TransferLearnedModel(emb, Head(max_batch=64, params=p), blob, "synthetic"))
        samples.append(n)
    assert [len(sa.window_offsets(n, 16000, 320)) for n in samples] == [15, 50, 0]

    def targets(dest):
        os.makedirs(dest, exist_ok=True)
        return [sa.StreamTarget("xx", w, "unused: live models", [sa.StreamFlags(wav=wavs[k], ground_truth=labels[k], target_keyword=w,
                                                                                detection_thresholds=THRESHOLDS)],
                                os.path.join(dest, f"{w}.pkl"), os.path.join(dest, f"{w}.npy")) for k, w in enumerate(WORDS)]
    return dict(sa=sa, models=models, targets=targets, root=str(root), samples=samples)


@pytest.mark.gpu
def test_batch_pass_equals_eval_stream_test_per_target_and_reuses_stored_inferences(world, capsys):
    import pickle
    sa, models = world["sa"], world["models"]
    one, batch = world["targets"](os.path.join(world["root"], "one_by_one")), world["targets"](os.path.join(world["root"], "batch"))
    want = [sa.eval_stream_test(st, live_model=m) for st, m in zip(one, models)]
    got = sa.eval_stream_tests(batch, live_models=models)
    for a, b, rows in zip(one, batch, (15, 50, 0)):
        x, y = np.load(a.destination_result_inferences), np.load(b.destination_result_inferences)
        assert x.shape == (rows, 3) and x.dtype == y.dtype == np.float32
        assert np.array_equal(x, y), a.target_word
        with open(a.destination_result_pkl, "rb") as fa, open(b.destination_result_pkl, "rb") as fb:
            assert pickle.load(fa) == pickle.load(fb)
    assert got == want
    fires = [len(r[w][0][1][thr][0]) for r, w in zip(got, WORDS) for thr in THRESHOLDS]
    print("fires per (target, threshold):", fires)
    assert sum(fires) >= 2 and fires[4:] == [0, 0]                      # keywords fire; the recording without a window has no events
    x0, x1 = np.load(batch[0].destination_result_inferences), np.load(batch[1].destination_result_inferences)
    assert not np.array_equal(x0, x1[:15])                              # two recordings, two heads
    # the results are there: a repeat returns None for every target, as eval_stream_test does
    capsys.readouterr()
    assert sa.eval_stream_tests(batch, live_models=models) == [None, None, None]
    assert capsys.readouterr().out.count("results already present") == 3
    # without the pickles the stored inferences are re-used: no embedding runs (the models are not even looked at)
    for st in batch:
        os.remove(st.destination_result_pkl)
    stamps = [os.path.getmtime(st.destination_result_inferences) for st in batch]
    again = sa.eval_stream_tests(batch, live_models=[object()] * 3)
    assert capsys.readouterr().out.count("inferences already present") == 3
    assert again == want and stamps == [os.path.getmtime(st.destination_result_inferences) for st in batch]
    # a mixed pass: the second target's inferences are computed again, into rows between two stored ones
    os.remove(batch[1].destination_result_inferences)
    for st in batch:
        os.remove(st.destination_result_pkl)
    assert sa.eval_stream_tests(batch, live_models=models) == want
    assert np.array_equal(np.load(batch[1].destination_result_inferences), x1)
    capsys.readouterr()


@pytest.mark.gpu
def test_stream_operating_curves_equal_operating_curves_per_target(world, capsys):
    sa, models = world["sa"], world["models"]
    targets = world["targets"](os.path.join(world["root"], "curves"))
    got = sa.stream_operating_curves(targets, live_models=models, num_nontarget_words=40)
    assert len(got) == 3 and all(len(c) == 1 and len(c[0]) == len(THRESHOLDS) for c in got)
    for st, m, n, curves in zip(targets, models, world["samples"], got):
        flags = st.stream_flags[0]
        inferences = np.load(st.destination_result_inferences)          # saved by the pass
        with open(flags.ground_truth) as fh:
            rows = [(r[0], float(r[1])) for r in csv.reader(fh) if r]
        if len(inferences):
            want = sa.operating_curves(inferences, flags, THRESHOLDS, rows, sample_rate=16000, data_samples=n, num_nontarget_words=40)
        else:       # operating_curves' device route takes no stream without windows; its specification does: tpr_fpr on detect()'s (empty) lists
            from multilingual_kws_amd.embedding.tpr_fpr import tpr_fpr
            times = [t for k, t in rows if k == st.target_word]
            want = [tpr_fpr(st.target_word, thr, sa.detect(inferences, flags, thr, 16000, data_samples=n)[0], times, n / 16000,
                            flags.time_tolerance_ms, 40) for thr in THRESHOLDS]
        assert curves[0] == want, st.target_word
        assert [type(v) for v in curves[0][0].values()] == [type(v) for v in want[0].values()]
        assert all(d["groundtruth_positives"] == 2 and d["keyword"] == st.target_word for d in want)
    assert sum(d["true_positives"] + d["false_positives"] for c in got for d in c[0]) >= 2
    assert not any(os.path.exists(st.destination_result_pkl) for st in targets)
    # the inference files are now present: re-used, and the curves are the same
    capsys.readouterr()
    assert sa.stream_operating_curves(targets, live_models=[object()] * 3, num_nontarget_words=40) == got
    assert capsys.readouterr().out.count("inferences already present") == 3
