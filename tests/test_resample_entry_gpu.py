"""The entry points that take audio at any rate: input_data.to_sample_rate / read_wav_at, and resample=True of multi_keyword_detections,
multi_keyword_operating_curves and run.inference."""
import numpy as np
import pytest

from multilingual_kws_amd import synth
from multilingual_kws_amd.embedding import batch_streaming_analysis as sa
from multilingual_kws_amd.embedding import input_data

pytestmark = pytest.mark.gpu
KEYWORDS = ["uno", "dos", "tres"]


def _pcm(rate, seconds, seed=0):
    rng = np.random.default_rng(seed)
    n = int(rate * seconds)
    t = np.arange(n) / rate
    f = 400.0 + 300.0 * ((np.arange(n) // (rate // 4)) % 4)
    return np.round(9000 * np.sin(2 * np.pi * f * t) + 1500 * rng.standard_normal(n)).astype(np.int16)


@pytest.fixture(scope="module")
def wavs(tmp_path_factory):
    root = tmp_path_factory.mktemp("rates")
    paths = {}
    for rate in (48000, 16000):
        paths[rate] = str(root / f"stream_{rate}.wav")
        with open(paths[rate], "wb") as fh:
            fh.write(synth.wav_bytes(_pcm(rate, 3.0), rate=rate))
    return paths


def test_read_wav_at(wavs):
    import multilingual_kws.embedding.input_data as by_path
    from multilingual_kws_amd.resample import Resampler
    assert by_path.to_sample_rate is input_data.to_sample_rate and by_path.read_wav_at is input_data.read_wav_at
    with open(wavs[48000], "rb") as fh:
        x, rate = input_data.decode_wav(fh.read())
    assert rate == 48000 and x.shape == (144000,)
    y = input_data.to_sample_rate(x, rate)
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (48000,)
    rs = Resampler(48000)
    assert np.array_equal(y, rs.forward(x, centred=True))
    rs.close()
    assert np.array_equal(input_data.read_wav_at(wavs[48000]), y)
    assert np.array_equal(input_data.read_wav_at(wavs[48000], 16000, 16000), y[:16000])
    padded = input_data.read_wav_at(wavs[48000], 16000, 50000)
    assert padded.shape == (50000,) and np.array_equal(padded[:48000], y) and not padded[48000:].any()
    # a file already at the rate asked for is decoded and nothing else; int16 at equal rates is s / 32768
    assert np.array_equal(input_data.read_wav_at(wavs[16000], 16000, 20000), input_data._read_wav(wavs[16000], 20000))
    assert np.array_equal(input_data.to_sample_rate(_pcm(16000, 0.1), 16000), _pcm(16000, 0.1).astype(np.float32) / np.float32(32768))
    # the time alignment of the centred form: a 1 kHz tone comes back as the same tone, sample for sample
    t48, t16 = np.arange(4800) / 48000, np.arange(1600) / 16000
    tone = input_data.to_sample_rate((0.5 * np.sin(2 * np.pi * 1000 * t48)).astype(np.float32), 48000)
    assert np.abs(tone[200:1400] - 0.5 * np.sin(2 * np.pi * 1000 * t16[200:1400])).max() < 1e-4


def test_multi_keyword_detections_resample(wavs, capsys):
    import torch
    from multilingual_kws_amd import run
    from multilingual_kws_amd.embedding import transfer_learning as tl
    from multilingual_kws_amd.head import Head
    emb, blob = tl.load_base_model("synthetic", max_batch=128)
    models = [tl.TransferLearnedModel(emb, Head(max_batch=128, seed=s), blob, "synthetic") for s in (1, 2, 3)]
    ms = input_data.standard_microspeech_model_settings(3)
    thr = 0.34
    with open(wavs[48000], "rb") as fh:
        x, _ = input_data.decode_wav(fh.read())
    converted = input_data.to_sample_rate(x, 48000)
    seen, real = [], sa.streaming_inferences

    def spy(models_, ms_, audio, sample_rate, *a, **k):
        got = real(models_, ms_, audio, sample_rate, *a, **k)
        seen.append((audio, sample_rate, got))
        return got
    sa.streaming_inferences = spy
    try:
        det = sa.multi_keyword_detections(KEYWORDS, models, wavs[48000], detection_threshold=thr, resample=True)
        audio, rate, got = seen.pop()
        # what was windowed is the converted recording at the model's rate, and the inferences are those of that array
        assert rate == 16000 and torch.is_tensor(audio) and np.array_equal(audio.cpu().numpy(), converted)
        want = real(models, ms, converted, 16000, 1000, 20, max_chunk_length_sec=1200, as_device=True)
        assert tuple(got.shape) == (3, len(sa.window_offsets(48000, 16000, 320)), 3) and torch.equal(got, want)
        flags = sa.StreamFlags(wav=wavs[48000], ground_truth=None, target_keyword="uno", detection_thresholds=[thr], max_chunk_length_sec=1200)
        found = sa.detect_many(want, flags, [thr], 16000, data_samples=48000, keywords=KEYWORDS)
        merged = sorted([d for f in found for d in f[thr][1]], key=lambda d: d[1])
        assert det == dict(keywords=KEYWORDS, min_threshold=thr,
                           detections=[dict(keyword=d[0], time_ms=d[1], confidence=d[2], groundtruth="ng") for d in merged])
        assert all(d["time_ms"] < 3000 for d in det["detections"])
        assert run.inference(KEYWORDS, models, wavs[48000], detection_threshold=thr, resample=True) == det
        assert seen.pop()[1] == 16000
        # the default leaves the recording as it is: the 48 kHz samples and their rate go on to the window loop, as before
        class Stop(Exception):
            pass

        def stop(models_, ms_, audio, sample_rate, *a, **k):
            seen.append((audio, sample_rate))
            raise Stop
        sa.streaming_inferences = stop
        with pytest.raises(Stop):
            sa.multi_keyword_detections(KEYWORDS, models, wavs[48000], detection_threshold=thr)
        audio, rate = seen.pop()
        assert rate == 48000 and isinstance(audio, np.ndarray) and np.array_equal(audio, x)
        # a recording at the model's rate is not converted, whatever resample says
        sa.streaming_inferences = spy
        plain = sa.multi_keyword_detections(KEYWORDS, models, wavs[16000], detection_threshold=thr)
        assert isinstance(seen.pop()[0], np.ndarray)
        assert sa.multi_keyword_detections(KEYWORDS, models, wavs[16000], detection_threshold=thr, resample=True) == plain
        assert isinstance(seen.pop()[0], np.ndarray)
    finally:
        sa.streaming_inferences = real
    capsys.readouterr()


def test_operating_curves_resample(wavs, tmp_path):
    from multilingual_kws_amd.embedding import transfer_learning as tl
    from multilingual_kws_amd.head import Head
    emb, blob = tl.load_base_model("synthetic", max_batch=128)
    models = [tl.TransferLearnedModel(emb, Head(max_batch=128, seed=s), blob, "synthetic") for s in (1, 2)]
    gt = str(tmp_path / "gt.csv")
    with open(gt, "w") as fh:
        fh.write("uno,500\ndos,1500\n")
    seen, real = [], sa.streaming_inferences

    def spy(models_, ms_, audio, sample_rate, *a, **k):
        seen.append(sample_rate)
        return real(models_, ms_, audio, sample_rate, *a, **k)
    sa.streaming_inferences = spy
    try:
        curves = sa.multi_keyword_operating_curves(KEYWORDS[:2], models, wavs[48000], gt, [0.3, 0.6], resample=True)
    finally:
        sa.streaming_inferences = real
    assert seen == [16000] and sorted(curves) == ["dos", "uno"] and all(len(c) == 2 for c in curves.values())
