"""LiveSession: audio in, detections out, with the frontend's frames and the detector's state kept on the device.  Each leg is held to
code that exists and is tested on its own: a push's probabilities to StreamingSession.infer on that window (same handle, same launches),
its detections to detect_on_device over the probabilities the session produced."""
import warnings

import numpy as np
import pytest

from multilingual_kws_amd.embedding import batch_streaming_analysis as bsa
from tests.util_data import tone_clip

pytestmark = pytest.mark.gpu
THRESHOLDS = (0.2, 0.5, 0.8)
HOP, CLIP, SAMPLES, WINDOWS = 320, 16000, 32000, 51


def _recording():
    rng = np.random.default_rng(9)
    pcm = np.concatenate([tone_clip(400 + 300 * k, rng, n=8000) for k in range(4)])
    return pcm.astype(np.float32) / 32768


def _models(max_batch=1):
    from multilingual_kws_amd.embedding import transfer_learning as tl
    from multilingual_kws_amd.head import Head
    emb, blob = tl.load_base_model("synthetic", max_batch=max_batch)
    return emb, [tl.TransferLearnedModel(emb, Head(max_batch=max_batch, seed=s), blob, "synthetic") for s in (1, 2, 3)]


def _feed(sess, audio, sizes=(HOP,)):
    out, records, at, k = [], [], 0, 0
    while at < audio.size:
        out += sess.feed(audio[at:at + sizes[k % len(sizes)]])
        records += sess.last_records
        at += sizes[k % len(sizes)]
        k += 1
    return out, records


def test_live_session_equals_its_offline_pieces():
    import torch
    from multilingual_kws_amd.detector import detect_on_device
    from multilingual_kws_amd.embedding import input_data
    from multilingual_kws_amd.frontend import Frontend
    ms = input_data.standard_microspeech_model_settings(3)
    audio = _recording()
    emb, models = _models()
    keywords = ["uno", "dos", "tres"]
    sess = bsa.LiveSession(models, THRESHOLDS, keywords=keywords, fired_only=False)
    assert sess.graph is not None and sess.samples_seen == 0 and sess.windows_seen == 0
    window_loop = bsa.StreamingSession(models, ms, batch=1)
    # (a) hop by hop: every push's probabilities are StreamingSession.infer's on that window, bit for bit
    got, records, probs, spec = [], [], [], []
    for i in range(SAMPLES // HOP):
        before = sess.windows_seen
        got += sess.feed(torch.from_numpy(audio[i * HOP:(i + 1) * HOP]).cuda() if i % 2 else audio[i * HOP:(i + 1) * HOP])
        records += sess.last_records
        spec.append(sess.spec[:sess.windows_seen - before].clone())
        if sess.windows_seen:
            w = sess.windows_seen - 1
            mine = sess.probs.clone()
            assert torch.equal(mine, window_loop.infer(audio[w * HOP:w * HOP + CLIP])), w
            probs.append(mine[:, 0])
    assert sess.windows_seen == WINDOWS == len(probs) and sess.samples_seen == SAMPLES and sess.recaptures == 0
    # every push's spectrogram rows are Frontend.stream's over the whole recording, bit for bit
    fe = Frontend(max_samples=SAMPLES)
    assert torch.equal(torch.cat(spec), fe.stream(torch.from_numpy(audio).cuda(), CLIP, HOP)[:WINDOWS])
    fe.close()
    probs = torch.stack(probs, dim=1)                                       # [3, 51, 3]
    assert torch.isfinite(probs).all()
    # (b) the detections are detect_on_device's over those probabilities
    times = [20 * w for w in range(WINDOWS)]
    f = sess.flags
    want = detect_on_device(probs, times, THRESHOLDS, f.average_window_duration_ms, f.suppression_ms, f.minimum_count, fired_only=False)
    want_records = sorted((int(w), n, k, int(fired), score) for n in range(3) for k in range(3) for w, fired, score in want.events[n][k].tolist())
    assert all(want.counts[n, k] >= 1 for n in range(3) for k in range(3)), "every lane must report something"
    assert records == want_records
    assert got == [[keywords[n] if fired else "_silence_", times[w], score, THRESHOLDS[k]] for w, n, k, fired, score in want_records]
    # (d) ragged chunks, (e) reset and again, (c) an eager session
    sess.reset()
    assert sess.windows_seen == 0 and sess.samples_seen == 0
    assert _feed(sess, audio, (100, 777, 5000, 1)) == (got, records)
    sess.reset()
    assert _feed(sess, audio) == (got, records)
    eager = bsa.LiveSession(models, THRESHOLDS, keywords=keywords, fired_only=False, use_graph=False)
    assert eager.graph is None and _feed(eager, audio, (1280, 333)) == (got, records)
    # fired_only (the default): the fires among them, with detect()'s own lists
    fires = bsa.LiveSession(models, THRESHOLDS, keywords=keywords)
    assert _feed(fires, audio)[0] == [g for g, r in zip(got, records) if r[3]]
    # several hops per push need a handle that takes them
    with pytest.raises(ValueError):
        bsa.LiveSession(models, THRESHOLDS, hops_per_push=2)
    for s in (sess, eager, fires):
        s.close()


def test_live_session_with_four_hops_per_push():
    """h = 4: a push is a batch of four windows on the embedding (another plan than batch 1: equal up to its rounding), the detections
    are detect_on_device's over the session's own probabilities, exactly."""
    import torch
    from multilingual_kws_amd.detector import detect_on_device
    audio = _recording()
    emb, models = _models(max_batch=4)
    sess = bsa.LiveSession(models, THRESHOLDS, hops_per_push=4, fired_only=False)
    records, probs = [], []
    for i in range(SAMPLES // (4 * HOP)):
        before = sess.windows_seen
        sess.feed(audio[i * 4 * HOP:(i + 1) * 4 * HOP])
        records += sess.last_records
        probs.append(sess.probs[:, :sess.windows_seen - before].clone())
    probs = torch.cat(probs, dim=1)
    assert tuple(probs.shape) == (3, WINDOWS, 3) and sess.windows_seen == WINDOWS
    f = sess.flags
    want = detect_on_device(probs, [20 * w for w in range(WINDOWS)], THRESHOLDS, f.average_window_duration_ms, f.suppression_ms, f.minimum_count)
    assert records == sorted((int(w), n, k, int(fired), score) for n in range(3) for k in range(3) for w, fired, score in want.events[n][k].tolist())
    assert len(records) >= 9
    sess.close()


def test_live_session_recaptures_after_a_failed_exchange():
    emb, models = _models()
    if emb.get_option("fuse_pair") != 1:
        pytest.skip("the exchange kernels are not in this handle's plan on this device")
    audio = _recording()
    sess = bsa.LiveSession(models, THRESHOLDS, fired_only=False)
    cut = 60 * HOP                                                          # windows 0 .. 10 exist by then
    _, before = _feed(sess, audio[:cut])
    assert sess.recaptures == 0 and sess.windows_seen == 11
    emb.set_option("inject_exchange_error", 1)                              # as if the previous replay's exchange had failed
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        _, after = _feed(sess, audio[cut:])
    assert sess.recaptures == 1 and sess.windows_seen == WINDOWS and sess.samples_seen == SAMPLES
    assert emb.get_option("exchange_error") == 0 and emb.get_option("fuse_pair") == 0
    # a session that runs on the healed plan from the start
    healed = bsa.LiveSession(models, THRESHOLDS, fired_only=False)
    _, ref = _feed(healed, audio)
    assert healed.recaptures == 0
    ref_after = [r for r in ref if r[0] >= 11]
    assert len(after) >= 9 and [r[:4] for r in after] == [r[:4] for r in ref_after]
    assert np.allclose([r[4] for r in after], [r[4] for r in ref_after], rtol=1e-4, atol=0)
    assert [r[:4] for r in before] == [r[:4] for r in ref if r[0] < 11]
    sess.close()
    healed.close()
