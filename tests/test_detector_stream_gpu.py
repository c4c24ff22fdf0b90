"""The device detector end to end on the bench's own stream shape (configs[4]: 60 s synthetic stream, 2 950 one-second windows, batches
of 256 on four lanes, 50 keyword heads on one shared embedding): run.inference and calculate_streaming_accuracy against detect() run on
the host, list for list and float for float; and the probabilities of that stream against the CPU oracle chain."""
import numpy as np
import pytest

SECONDS = 60
THRESHOLD = 0.5


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    """wav (the 60 clips bench.py concatenates, as 16-bit PCM: synth.clips_float32 is int16 / 32768, so the file holds the same samples),
    its decoded audio, and 50 live models on one 256-window embedding handle, their heads biased towards the target class as in
    tests/test_surface.py so that several keywords fire."""
    pytest.importorskip("torch")
    from multilingual_kws_amd import synth
    from multilingual_kws_amd.embedding import input_data, transfer_learning as tl
    from multilingual_kws_amd.head import Head
    from oracle import head_oracle as ho
    pcm = np.concatenate([synth.clips_int16(1, first_clip=i)[0] for i in range(SECONDS)])
    wav = str(tmp_path_factory.mktemp("stream60") / "stream.wav")
    with open(wav, "wb") as fh:
        fh.write(synth.wav_bytes(pcm))
    with open(wav, "rb") as fh:
        audio, rate = input_data.decode_wav(fh.read())
    assert rate == 16000 and np.array_equal(audio, np.concatenate([synth.clips_float32(1, first_clip=i)[0] for i in range(SECONDS)]))
    emb, blob = tl.load_base_model("synthetic", max_batch=256)
    keywords = [f"kw{k:02d}" for k in range(50)]
    models = []
    for k in range(50):
        p = ho.glorot_uniform_params(seed=2000 + k)
        p[-1] += 0.5 + 0.1 * (k % 7)
        models.append(tl.TransferLearnedModel(emb, Head(max_batch=256, params=p), blob, "synthetic"))
    return dict(wav=wav, audio=audio, blob=blob, keywords=keywords, models=models)


@pytest.mark.gpu
def test_run_inference_and_streaming_accuracy_equal_the_host_detector_on_the_bench_stream(stream, capsys):
    from multilingual_kws_amd import run
    from multilingual_kws_amd.embedding import batch_streaming_analysis as sa, input_data
    ms = input_data.standard_microspeech_model_settings(3)
    wav, audio, keywords, models = stream["wav"], stream["audio"], stream["keywords"], stream["models"]
    n_windows = len(sa.window_offsets(audio.shape[0], 16000, 320))
    assert n_windows == 2950
    det = run.inference(keywords, models, wav, detection_threshold=THRESHOLD)
    d = det["detections"]
    assert det["keywords"] == keywords and det["min_threshold"] == THRESHOLD
    assert len(d) > 10 and len({x["keyword"] for x in d}) > 3
    # the parent's route on the same handle: host copies of streaming_inferences, detect() per keyword, merged and sorted (stable)
    inf = sa.streaming_inferences(models, ms, audio, 16000, 1000, 20, max_chunk_length_sec=1200)
    assert len(inf) == 50 and all(x.shape == (n_windows, 3) and x.dtype == np.float32 for x in inf)
    unsorted = []
    for kw, x in zip(keywords, inf):
        flags = sa.StreamFlags(wav=wav, ground_truth=None, target_keyword=kw, detection_thresholds=[THRESHOLD], max_chunk_length_sec=1200)
        unsorted.extend(sa.detect(x, flags, THRESHOLD, 16000, data_samples=audio.shape[0])[1])
    want = [dict(keyword=k, time_ms=t, confidence=c, groundtruth="ng") for k, t, c in sorted(unsorted, key=lambda e: e[1])]
    assert d == want                                                             # list for list, float for float
    assert all(type(x["confidence"]) is float and type(x["time_ms"]) is int for x in d)
    # the device tensors are the same numbers as the host copies
    dev = sa.streaming_inferences(models, ms, audio, 16000, 1000, 20, max_chunk_length_sec=1200, as_device=True)
    assert dev.is_cuda and tuple(dev.shape) == (50, n_windows, 3) and np.array_equal(dev.cpu().numpy(), np.stack(inf))
    one = sa.streaming_inferences(models[3], ms, audio, as_device=True)
    assert one.is_cuda and tuple(one.shape) == (n_windows, 3) and np.array_equal(one.cpu().numpy(), inf[3])
    # calculate_streaming_accuracy, 20 thresholds in one launch, = detect() per threshold
    thresholds = [round(0.05 * i, 2) for i in range(1, 21)]
    for k in (3, 13):
        flags = sa.StreamFlags(wav=wav, ground_truth="", target_keyword=keywords[k], detection_thresholds=thresholds)
        results, got_inf = sa.calculate_streaming_accuracy(models[k], ms, [flags])
        assert isinstance(got_inf, np.ndarray) and np.array_equal(got_inf, inf[k])
        (got_flags, by_threshold), = results
        assert got_flags == flags and list(by_threshold) == thresholds
        fired = 0
        for thr in thresholds:
            assert by_threshold[thr] == sa.detect(inf[k], flags, thr, 16000, data_samples=audio.shape[0]), (k, thr)
            fired += len(by_threshold[thr][0])
        assert fired > 10
    capsys.readouterr()


@pytest.mark.gpu
def test_bench_stream_probabilities_against_the_cpu_oracle_chain(stream):
    """Every window of the 2 950-window, four-lane, 50-head stream, heads 0, 7, 23 and 49, against the CPU oracle chain (C micro-frontend on
    the window's samples -> PyTorch-CPU EfficientNet -> numpy head) at the tolerance of test_fifty_keyword_detections_from_one_embedding_pass.
    Argmax equality is asserted where the oracle's two largest probabilities differ by more than 2e-4 (two values each within 1e-4 cannot
    swap across a wider gap); those must be at least 95 % of the windows."""
    from multilingual_kws_amd.embedding import batch_streaming_analysis as sa, input_data
    from oracle import head_oracle as ho
    from oracle.efficientnet_oracle import EmbeddingOracle
    from oracle.frontend_oracle import FrontendOracle
    ms = input_data.standard_microspeech_model_settings(3)
    audio, models = stream["audio"], stream["models"]
    inf = sa.streaming_inferences(models, ms, audio)
    offs = sa.window_offsets(audio.shape[0], 16000, 320)
    assert len(offs) == 2950
    ref_emb, oracle, frontend = [], EmbeddingOracle(stream["blob"]), FrontendOracle()
    for s in range(0, len(offs), 512):                                           # in slices: the oracle keeps whole activations
        wins = np.stack([audio[o:o + 16000] for o in offs[s:s + 512]])
        ref_emb.append(oracle.forward(frontend.run_batch_f32(wins)).numpy())
    ref_emb = np.concatenate(ref_emb)
    for k in (0, 7, 23, 49):
        ref, _ = ho.forward(models[k].head.get_params(), ref_emb)
        got = inf[k]
        err = float(np.abs(got - ref).max())
        top = np.sort(ref, axis=1)
        clear = (top[:, -1] - top[:, -2]) > 2e-4
        print(f"head {k}: max abs difference {err:.3e}, {clear.mean() * 100:.2f} % of the windows with a top-two gap above 2e-4")
        assert err < 1e-4, (k, err)
        assert clear.mean() >= 0.95, (k, clear.mean())
        assert np.array_equal(got[clear].argmax(1), ref[clear].argmax(1)), k
